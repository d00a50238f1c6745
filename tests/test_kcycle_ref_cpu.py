"""tests/kcycle_ref.py held to account before tests/test_gpu_kcycle.py compares the device with it bit for bit:
  * its float64 reductions lie within their derived bars of the exact sums, its long double ones within their own, far smaller bars;
  * its K step is what the definition says — the minimum-residual combination (GCR form), the Galerkin combination (energy form);
  * every defect the GPU test is there to notice, planted in the restatement, moves a scalar past its bar or changes x's bits;
  * the degenerate inputs (rhs = 0; an exact cycle) give the exact results the device is then asked for."""
import numpy as np
import pytest

import kcycle_ref as K
import krylov_ref as kr

SIZES = (1, 2, 3, 511, 1025, 2049, 2051, 70_001)
LD = np.longdouble


def signed(rng, n):
    """[0.5, 2] in magnitude, random sign"""
    return rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)


# ------------------------------------------------------------------------------------------------------------------- 1. the yardstick
@pytest.mark.parametrize("n", SIZES)
def test_reductions_within_their_bars_of_the_exact_sums(n):
    rng = np.random.default_rng(5000 + n)
    a, b0, b1, c1, c2 = (signed(rng, n) for _ in range(5))
    worst = {}

    def hold(kind, got64, gotld, x, y):
        ref, sabs = K.exact_dot(x, y)
        e64 = abs(float(got64) - ref)
        eld = abs(K.exact_dot(x, y, minus=gotld)[0])
        b64, bld = K.bar(kind, n, sabs), K.bar(kind, n, sabs, K.U_LD)
        worst[kind] = max(worst.get(kind, 0.0), e64 / b64)
        assert e64 <= b64, (kind, n, e64, b64)
        assert eld <= bld and bld < b64 / 1000, (kind, n, eld, bld)

    m64, mld = K.mdot2(a, b0, b1), K.mdot2(a, b0, b1, LD)
    hold("mdot", m64[0], mld[0], a, b0); hold("mdot", m64[1], mld[1], a, b1)
    hold("dot", K.dot_dev(a, b0), K.dot_dev(a, b0, LD), a, b0)
    for energy in (False, True):
        # float64: the orthogonalised vectors as the kernel rounds them; long double: g = 0, so that they are the float64 data themselves
        g = 0.37
        d2o, v2o = K.orth_vectors(g, c1, c2, a, b0, energy)
        o64 = K.orth_dots(g, c1, c2, a, b0, b1, energy)
        z2o, w2o = K.orth_vectors(0.0, c1, c2, a, b0, energy)
        assert np.array_equal(w2o, b0) and np.array_equal(z2o, c2 if energy else b0)
        old = K.orth_dots(0.0, c1, c2, a, b0, b1, energy, LD)
        o0 = K.orth_dots(0.0, c1, c2, a, b0, b1, energy)
        for got, x, y in ((o64[0], d2o, v2o), (o64[1], d2o, b1)):
            ref, sabs = K.exact_dot(x, y)
            assert abs(float(got) - ref) <= K.bar("orth", n, sabs), ("orth", n, energy)
            worst["orth"] = max(worst.get("orth", 0.0), abs(float(got) - ref) / K.bar("orth", n, sabs))
        hold("orth", o0[0], old[0], z2o, w2o); hold("orth", o0[1], old[1], z2o, b1)
    print(f"n={n}: largest float64 error/bar " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_depths_are_the_loops():
    """one pair / element per lane below the grids' caps; the strided part of the fold grows by one per 256 partials"""
    assert K.mdot_grid(2048) == 1 and K.mdot_grid(2049) == 1 and K.mdot_grid(2050) == 2 and K.mdot_grid(600_001) == 293
    assert K.orth_grid(1024) == 1 and K.orth_grid(1025) == 2 and K.orth_grid(600_001) == 586
    assert K.dot_grid(256) == 1 and K.dot_grid(257) == 2 and K.dot_grid(70_001) == 274
    assert K.depth("mdot", 2051) == 2 * 3 + 1 + 6 + 4 + 1 + 8           # 1025 pairs on 2 × 256 lanes: three trips, then the odd tail
    assert K.depth("mdot", 2) == 2 + 6 + 4 + 1 + 8
    assert K.depth("dot", 70_001) == 1 + 6 + 4 + 2 + 8 and K.depth("orth", 600_001) == 4 + 6 + 4 + 3 + 8


def test_exact_dot_is_exact():
    """products whose low halves matter: (1 + 2⁻³⁰)² − 1 − 2⁻²⁹ = 2⁻⁶⁰, lost by any 64-bit product"""
    x = np.array([1.0 + 2.0 ** -30, 1.0, 2.0 ** -15])
    y = np.array([1.0 + 2.0 ** -30, -1.0, -2.0 ** -14])
    assert K.exact_dot(x, y)[0] == 2.0 ** -60
    assert K.exact_dot(x, y, minus=LD(2.0) ** -60)[0] == 0.0


# ------------------------------------------------------------------------------------------------------- 2. the step is its definition
def jacobi2(op, omega=0.7):
    """B = two damped-Jacobi sweeps from x = 0 on the banded operator: a fixed linear map"""
    def apply(r):
        w = (omega / op.diags[2]).astype(r.dtype)
        x = w * r
        return x + w * (r - op.apply(x))
    return apply


@pytest.mark.parametrize("spd", [True, False], ids=["spd", "nonsymmetric"])
def test_kstep_is_what_its_definition_says(spd):
    """properties of EXACT arithmetic, checked in 64-bit-mantissa arithmetic (the long double run of the restatement) to 1e-12 relative:
    GCR form: x minimises ‖rhs − A·x‖₂ over span{c1, c2}; energy form (SPD operator): c_j·(rhs − A·x) = 0, j = 1, 2"""
    n = 2051
    op = kr.banded(n, seed=31 + int(spd), spd=spd)
    rhs = signed(np.random.default_rng(77 + int(spd)), n)
    s = K.kstep(jacobi2(op), op.apply, rhs, energy=False, dtype=LD)
    k1, k2 = K.coefficients(s["scal"], LD)
    V = np.stack([s["v1"], s["v2"]], axis=1).astype(np.float64)
    coef, _, rank, sv = np.linalg.lstsq(V, rhs, rcond=None)
    assert rank == 2
    d = max(abs(float(k1) - coef[0]), abs(float(k2) - coef[1])) / np.abs(coef).max()
    print(f"spd={spd}: GCR coefficients ({float(k1):.6f}, {float(k2):.6f}) vs lstsq: {d:.2e} relative; singular values {sv}")
    assert d <= 1e-12, d
    r = LD(1) * rhs - op.apply(s["x"])
    for v in (s["v1"], s["v2"]):        # the normal equations of the same minimum, in long double
        assert abs(kr.dot(v, r)) <= 1e-12 * float(np.sqrt(kr.dot(v, v) * kr.dot(rhs.astype(LD), rhs.astype(LD))))
    if spd:
        e = K.kstep(jacobi2(op), op.apply, rhs, energy=True, dtype=LD)
        r = LD(1) * rhs - op.apply(e["x"])
        for c in (e["c1"], e["c2"]):
            q = abs(kr.dot(c, r)) / float(np.sqrt(kr.dot(c, c) * kr.dot(rhs.astype(LD), rhs.astype(LD))))
            print(f"energy form: c·(rhs − A·x) = {float(q):.2e} relative")
            assert q <= 1e-12
        assert e["scal"][3] > 0 and not K.same_bits(np.asarray(e["x"], dtype=np.float64), np.asarray(s["x"], dtype=np.float64))


# ------------------------------------------------------------------------------------------------------------------- 3. mutations
def scalar_bars(s, energy, aligned=True):
    """(exact value, bar) of the five scalars on the vectors of a float64 run of the step"""
    d1, d2 = (s["c1"], s["c2"]) if energy else (s["v1"], s["v2"])
    n = len(s["rp"])
    g = K.quotient(s["scal"][2], s["scal"][0])
    d2o, v2o = K.orth_vectors(g, s["c1"], s["c2"], s["v1"], s["v2"], energy)
    first = "mdot" if aligned else "dot"
    out = []
    for kind, x, y in ((first, d1, s["v1"]), (first, d1, s["rhs"]), ("dot", d2, s["v1"]), ("orth", d2o, v2o), ("orth", d2o, s["rp"])):
        ref, sabs = K.exact_dot(x, y)
        out.append((ref, K.bar(kind, n, sabs)))
    return out


def caught(clean, bad, energy, aligned=True):
    """does the GPU test's comparison tell `bad` from `clean`: a scalar past its bar from the exact value, or other bits in x"""
    past = [abs(float(v) - ref) > b for v, (ref, b) in zip(bad["scal"], scalar_bars(clean, energy, aligned))]
    return past, not K.same_bits(bad["x"], clean["x"])


def step_on_banded(n, energy, defects=(), aligned=True, spd=True):
    op = kr.banded(n, seed=9, spd=spd)
    rhs = signed(np.random.default_rng(n), n)
    s = K.kstep(jacobi2(op), op.apply, rhs, energy, aligned, defects=defects)
    s["rhs"] = rhs
    return s


@pytest.mark.parametrize("defect,energy,aligned", [("no_tail", False, True), ("no_tail", True, True), ("skip_partial", False, True),
                                                    ("skip_partial", False, False), ("no_g_in_v2o", False, True),
                                                    ("no_g_in_d2o", True, True), ("swap_forms", False, True), ("swap_forms", True, True)])
def test_planted_defects_are_caught(defect, energy, aligned):
    """each planted defect moves a scalar past its bar or changes x's bits.  In the energy form g and a are chosen so that c2'·A·c1 = 0 and
    c1·r' = 0: there g missing from d2' leaves ρ2 and α2 what they are in exact arithmetic and shows as a last-place difference in α2 and
    other bits in x — only a bit comparison notices it — and g missing from v2' (c2'·v2 instead of c2'·v2': the same number but for rounding)
    is no defect of the result, which is why it is not in the list for that form."""
    n = 2051
    clean = step_on_banded(n, energy, aligned=aligned)
    past0, x0 = caught(clean, clean, energy, aligned)
    assert not any(past0) and not x0                   # the clean run passes its own comparison
    bad = step_on_banded(n, energy, defects={defect}, aligned=aligned)
    past, xbits = caught(clean, bad, energy, aligned)
    print(f"{defect} energy={energy} aligned={aligned}: scalars past their bars {past}, x changed {xbits}")
    assert any(past) or xbits, (defect, past, xbits)
    assert any(past) or (defect == "no_g_in_d2o" and not K.same_bits(bad["scal"], clean["scal"]))


def indefinite_step(defects=()):
    """energy form on A = diag(1, −1), B = I, rhs = (1, 1/2): ρ1 = 3/4, a = 5/3, r' = (−2/3, 4/3), γ = −4/3, c2' = (10/9, 20/9),
    ρ2 = (100 − 400)/81 < 0 and α2 = 60/27: the step must stop at its first direction"""
    d = np.array([1.0, -1.0])
    return K.kstep(lambda r: r.copy(), lambda x: d.astype(x.dtype) * x, np.array([1.0, 0.5]), True, defects=defects)


def test_negative_rho2_keeps_the_first_direction_only():
    clean, bad = indefinite_step(), indefinite_step({"rho2_nonzero"})
    assert clean["scal"][3] < 0 and clean["scal"][4] != 0
    k1, k2 = K.coefficients(clean["scal"])
    assert k2 == 0 and k1 == clean["scal"][1] / clean["scal"][0]
    assert np.array_equal(clean["x"], k1 * clean["c1"] + 0.0 * clean["c2"])
    assert K.same_bits(bad["scal"], clean["scal"]) and not K.same_bits(bad["x"], clean["x"])       # only x tells the two branches apart


# ------------------------------------------------------------------------------------------------------------- 4. degenerate inputs
def exact_cycle(n):
    """the two-grid V(1,1) cycle on A = 4·I with ω = 1 and pairs as aggregates, step by step: x1 = ωD⁻¹b = b/4, r = b − A·x1 = 0, A_c = 8·I,
    e_c = 0, x = x1 + P·e_c + ωD⁻¹(r − A·P·e_c) = b/4 — every operation exact (powers of two)"""
    agg = np.arange(n) // 2

    def B(b):
        wd = b.dtype.type(0.25)
        x1 = wd * b
        r = b - b.dtype.type(4) * x1
        ec = np.bincount(agg, weights=r.astype(np.float64)).astype(b.dtype) / b.dtype.type(8)
        pe = ec[agg]
        return x1 + pe + wd * (r - b.dtype.type(4) * pe)
    return B, (lambda x: x.dtype.type(4) * x)


@pytest.mark.parametrize("energy", [False, True], ids=["gcr", "energy"])
@pytest.mark.parametrize("n", [2, 3, 2051])
def test_degenerate_inputs(n, energy):
    op = kr.banded(n, seed=3, spd=True)
    z = K.kstep(jacobi2(op), op.apply, np.zeros(n), energy)
    assert all(v == 0 for v in z["scal"]) and not np.isnan(z["x"]).any()
    assert np.array_equal(z["x"], np.zeros(n)) and not np.signbit(z["x"]).any() and not np.signbit(z["rp"]).any()
    B, A = exact_cycle(n)
    rhs = signed(np.random.default_rng(40 + n), n)
    assert np.array_equal(B(rhs), rhs / 4)
    s = K.kstep(B, A, rhs, energy)
    rho1, alpha1, gamma, rho2, alpha2 = s["scal"]
    assert rho1 == alpha1 and rho1 > 0 and (gamma, rho2, alpha2) == (0, 0, 0)         # a = 1
    assert not s["rp"].any() and not s["c2"].any()
    assert K.same_bits(s["x"], rhs / 4) and K.same_bits(s["x"], s["c1"])
