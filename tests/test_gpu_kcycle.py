"""The K-cycle's two Krylov steps (coarse_solve_inner and the kernels it launches) against the exact host restatement of tests/kcycle_ref.py.

The device serves as its own preconditioner B: c1 = cycle(rhs), v1 = A·c1, c2 = cycle(r'), v2 = A·c2 come from the device with the K step
switched off (cycle and SpMV are pinned elsewhere), the host restates ρ1, α1, r', γ, ρ2, α2 and x from them in the kernels' own association,
and the K step at the entry level (mgs_hier_set_kcycle_entry) must then return
  * the restatement's BITS in each of the five scalars (mgs_hier_kcycle_scalars),
  * each scalar within its derived bar γ_{D+1}·Σ|x_i·y_i| of the exact sum on the same vectors,
  * the restatement's bits in x,
launched eagerly and replayed from the captured graph.  No operator enters the comparison, so its conditioning plays no part.  Sizes: one
element per pair (2), the odd tail (3, 2051), one lane short of a workgroup (511), the first sizes with two workgroups in kc_orth_dots (1025)
and in the multi-dot pass (2050, 2051), more than 256 partials in k_dot_dev's fold (70 001) and in the folds of the other two (600 001).
Further: the 8-byte route of k_mdot (rhs 8 bytes into a longer buffer), the entry step left alone under a non-zero guess, the branches
ρ1 = 0 (rhs = 0) and ρ2 = 0 (an exact cycle: A = 4·I, ω = 1), and on levels ≥ 1 the glue of coarse_solve: the K-cycle of a device-built
hierarchy against pre pass → entry K step of a sub-hierarchy on the same level operators → σ → post pass, bit for bit.

Largest error/bar ratios measured on an MI355X when the tests were written (a scalar passes at ≤ 1; every case also returned the
restatement's bits, eager and replayed), the largest of the five scalars and the three forms per size: n = 2 0.060, 3 0.071, 511 0.068,
1025 0.068, 2050 0.069, 2051 0.071, 70 001 0.058, 600 001 0.050; misaligned rhs 0.061 (energy) / 0.071 / 0.064; the exact cycle 0.043–0.045.
A scalar's ratio is 0 where the device's sum is the correctly rounded exact one (about two scalars in three) and 0.04–0.07 where it is one
unit in the last place away: the bars allow for 20–28 roundings, the reduction trees make one or none."""
import numpy as np
import pytest
import scipy.sparse as sps

import kcycle_ref as K
import krylov_ref as kr
import post_pass_ref as R

pytestmark = pytest.mark.gpu

OMEGA = 0.6
DEFAULTS = (("graph", 1), ("kcycle_energy", 0))          # mgs_internal.hpp (struct mgs_ctx)
SIZES = (2, 3, 511, 1025, 2050, 2051, 70_001, 600_001)
FORMS = {"spd_energy": (True, True), "spd_gcr": (True, False), "nonsymmetric_gcr": (False, False)}      # (SPD operator, energy form)
NAMES = ("rho1", "alpha1", "gamma", "rho2", "alpha2")
GROUPED = 3
INVALID, STATE = -1, -6


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


def restore(ctx):
    for k, v in DEFAULTS:
        ctx.set_option(k, v)


def upload(ctx, M):
    M = M.tocsr(); M.sort_indices()
    return ctx.csr(M.shape[0], M.shape[1], M.indptr, M.indices, M.data)


def build(ctx, mg, A, n, omega=OMEGA):
    """hierarchy on the uploaded operator: pairs as aggregates, then (where there are enough of them) everything onto eight aggregates, so
    that the dense coarsest solve costs nothing.  Above 65 536 pairs runs of 64 pairs come between the two: the Galerkin product of a
    transfer with 37 500 members per aggregate (600 001 rows) was measured at 93 s on an MI355X, the same setup with the level between at
    0.03 s.  The step under test sees the hierarchy only as its B."""
    agg = R.pairs(n); nc = int(agg.max()) + 1
    h = mg.Hierarchy(A, omega, 1, 1)
    h.push_P(upload(ctx, R.agg_P(agg, nc)))
    if nc > 65536:
        nc2 = (nc + 63) // 64
        h.push_P(upload(ctx, R.agg_P((np.arange(nc) // 64).astype(np.int32), nc2)))
        nc = nc2
    if nc >= 16:
        h.push_P(upload(ctx, R.agg_P((np.arange(nc) * 8 // nc).astype(np.int32), 8)))
    return h.finalize()


def misaligned(ctx, mg, a):
    """the array 8 bytes into a longer buffer: (buffer, view)"""
    buf = ctx.vec(np.concatenate([[7.0], a, [7.0]]))
    v = mg.Vec.wrap(ctx, buf.ptr + 8, len(a))
    assert v.ptr % 16 == 8
    return buf, v


def cycle(h, b, x, replay):
    h.vcycle(b, x)
    if replay:                      # the same (b, x): the second call replays the captured graph
        h.vcycle(b, x)
        assert h.graph_info()["captured_cycles"] >= 1, h.graph_info()
    return x.numpy()


def device_step(ctx, h, A, rhs, rhs_v, energy, aligned, replay):
    """the step walked through on the device with the entry K step off, restated on the host from the device's own c and v, then the
    entry K step itself.  Returns the restatement (kcycle_ref.kstep's names), the device's scalars and the device's x"""
    n = len(rhs)
    h.set_kcycle_entry(0)
    c1v = ctx.vec(n)
    c1 = cycle(h, rhs_v, c1v, replay)
    v1 = A.spmv(c1v).numpy()
    rho1, alpha1 = K.first_scalars(c1, v1, rhs, energy, aligned)
    rp = K.update_r(rho1, alpha1, rhs, v1)
    c2v = ctx.vec(n)
    c2 = cycle(h, ctx.vec(rp), c2v, replay)
    v2 = A.spmv(c2v).numpy()
    gamma, rho2, alpha2 = K.second_scalars(rho1, c1, c2, v1, v2, rp, energy)
    scal = [rho1, alpha1, gamma, rho2, alpha2]
    ref = dict(c1=c1, v1=v1, rp=rp, c2=c2, v2=v2, scal=scal, x=K.combine(scal, c1, c2))
    h.set_kcycle_entry(1)
    x = cycle(h, rhs_v, ctx.vec(n), replay)
    got = h.kcycle_scalars(0)
    h.set_kcycle_entry(0)
    return ref, got, x


def check_step(what, ref, got, x, rhs, energy, aligned=True, bars=True):
    """the three assertions of the module docstring; returns the largest error/bar ratio"""
    n = len(rhs)
    worst = 0.0
    if bars:
        d1, d2 = (ref["c1"], ref["c2"]) if energy else (ref["v1"], ref["v2"])
        d2o, v2o = K.orth_vectors(K.quotient(ref["scal"][2], ref["scal"][0]), ref["c1"], ref["c2"], ref["v1"], ref["v2"], energy)
        first = "mdot" if aligned else "dot"
        pairs = ((first, d1, ref["v1"]), (first, d1, rhs), ("dot", d2, ref["v1"]), ("orth", d2o, v2o), ("orth", d2o, ref["rp"]))
        ratios = []
        for (kind, p, q), g in zip(pairs, got):
            exact, sabs = K.exact_dot(p, q)
            ratios.append(abs(g - exact) / K.bar(kind, n, sabs) if sabs else 0.0)
        worst = max(ratios)
        print(f"{what}: scalars {['%.17g' % g for g in got]}, error/bar {['%.3f' % r for r in ratios]}, largest {worst:.3f}")
    for name, g, r in zip(NAMES, got, ref["scal"]):
        assert K.same_bits(g, r), (what, name, "bits", g, float(r), [float(v) for v in ref["scal"]], got)
    if bars:
        assert worst <= 1.0, (what, ratios)
    assert K.same_bits(x, ref["x"]), (what, "x bits", np.flatnonzero(K.bits(x) != K.bits(ref["x"]))[:8], float(np.abs(x - ref["x"]).max()))
    return worst


# ---------------------------------------------------------------------------------------------------- 1. the step at the entry level
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", SIZES)
def test_entry_step_scalars_and_combination(ctx, mg, n, form):
    """eager, then replayed from the captured graph: the same device vectors, the same scalars, the same x — all the restatement's"""
    spd, energy = FORMS[form]
    op = kr.banded(n, seed=200 + int(spd), spd=spd)
    rhs = R.signed(np.random.default_rng(n + 10 * int(energy)), n)
    try:
        ctx.set_option("kcycle_energy", int(energy))
        A = ctx.csr(n, n, *op.csr())
        h = build(ctx, mg, A, n)
        ctx.set_option("graph", 0)
        ref, got, x = device_step(ctx, h, A, rhs, ctx.vec(rhs), energy, True, replay=False)
        assert h.graph_info()["captured_cycles"] == 0
        check_step(f"n={n} {form} eager", ref, got, x, rhs, energy)
        ctx.set_option("graph", 1)
        ref2, got2, x2 = device_step(ctx, h, A, rhs, ctx.vec(rhs), energy, True, replay=True)
        for k in ("c1", "v1", "c2", "v2"):
            assert K.same_bits(ref2[k], ref[k]), (n, form, k, "replayed cycle differs from the eager one")
        check_step(f"n={n} {form} replayed", ref2, got2, x2, rhs, energy, bars=False)       # the same vectors: the bars were held above
        assert got2 == got
    finally:
        restore(ctx)


# ------------------------------------------------------------------------------------------------------------ 2. the 8-byte route
@pytest.mark.parametrize("form", list(FORMS))
def test_entry_step_with_a_misaligned_rhs(ctx, mg, form):
    """rhs starts 8 bytes into a longer buffer: k_mdot falls back to two k_dot_dev reductions for (ρ1, α1)"""
    n = 2051
    spd, energy = FORMS[form]
    op = kr.banded(n, seed=210 + int(spd), spd=spd)
    rhs = R.signed(np.random.default_rng(n + 77), n)
    try:
        ctx.set_option("kcycle_energy", int(energy))
        A = ctx.csr(n, n, *op.csr())
        h = build(ctx, mg, A, n)
        for graph in (0, 1):
            ctx.set_option("graph", graph)
            buf, view = misaligned(ctx, mg, rhs)
            ref, got, x = device_step(ctx, h, A, rhs, view, energy, False, replay=bool(graph))
            check_step(f"n={n} {form} misaligned rhs graph={graph}", ref, got, x, rhs, energy, aligned=False)
            fb = buf.numpy()
            assert fb[0] == 7.0 and fb[-1] == 7.0 and np.array_equal(fb[1:-1], rhs)
            a1 = K.first_scalars(ref["c1"], ref["v1"], rhs, energy, True)
            print(f"   16-byte route on the same vectors would give ρ1, α1 = {float(a1[0])!r}, {float(a1[1])!r}")
            del view
    finally:
        restore(ctx)


# --------------------------------------------------------------------------------------------------------- 3. non-zero guess
def test_entry_step_applies_from_a_zero_guess_only(ctx, mg):
    n = 2051
    op = kr.banded(n, seed=220, spd=True)
    rng = np.random.default_rng(221)
    rhs, x0 = R.signed(rng, n), R.signed(rng, n)
    try:
        A = ctx.csr(n, n, *op.csr())
        h = build(ctx, mg, A, n)
        for graph in (0, 1):
            ctx.set_option("graph", graph)
            plain = h.vcycle(ctx.vec(rhs), ctx.vec(x0), zero_guess=False).numpy()
            h.set_kcycle_entry(1)
            kx = h.vcycle(ctx.vec(rhs), ctx.vec(x0), zero_guess=False).numpy()
            kz = h.vcycle(ctx.vec(rhs)).numpy()
            h.set_kcycle_entry(0)
            assert K.same_bits(kx, plain) and not K.same_bits(kz, h.vcycle(ctx.vec(rhs)).numpy())
    finally:
        restore(ctx)


# ------------------------------------------------------------------------------------------------------- 4. degenerate branches
@pytest.mark.parametrize("energy", [0, 1], ids=["gcr", "energy"])
@pytest.mark.parametrize("graph", [0, 1], ids=["eager", "graph"])
def test_zero_rhs(ctx, mg, energy, graph):
    """ρ1 = 0: every quotient counts as 0, x = +0.0 everywhere, no NaN"""
    n = 2051
    op = kr.banded(n, seed=230, spd=True)
    try:
        ctx.set_option("kcycle_energy", energy); ctx.set_option("graph", graph)
        A = ctx.csr(n, n, *op.csr())
        h = build(ctx, mg, A, n).set_kcycle_entry(1)
        b, x = ctx.vec(np.zeros(n)), ctx.vec(np.full(n, np.nan))
        got = cycle(h, b, x, bool(graph))
        assert h.kcycle_scalars(0) == [0.0] * 5
        assert not np.isnan(got).any() and not got.any() and not np.signbit(got).any()
    finally:
        restore(ctx)


@pytest.mark.parametrize("energy", [0, 1], ids=["gcr", "energy"])
@pytest.mark.parametrize("n", [3, 2051])
def test_exact_cycle(ctx, mg, n, energy):
    """A = 4·I, ω = 1, pairs as aggregates: the cycle is A⁻¹ exactly (tests/test_kcycle_ref_cpu.py walks through it), so a = 1, r' = 0,
    γ = ρ2 = α2 = 0 and x = c1 = rhs/4, bit for bit — the branch ρ2 ≤ 0"""
    rhs = R.signed(np.random.default_rng(240 + n), n)
    try:
        ctx.set_option("kcycle_energy", energy)
        A = upload(ctx, 4.0 * sps.identity(n, format="csr"))
        h = build(ctx, mg, A, n, omega=1.0)
        for graph in (0, 1):
            ctx.set_option("graph", graph)
            ref, got, x = device_step(ctx, h, A, rhs, ctx.vec(rhs), bool(energy), True, replay=bool(graph))
            assert K.same_bits(ref["c1"], rhs / 4) and not ref["rp"].any() and not ref["c2"].any()
            check_step(f"A = 4·I n={n} energy={energy} graph={graph}", ref, got, x, rhs, bool(energy))
            assert got[0] == got[1] > 0 and got[2:] == [0.0, 0.0, 0.0], got
            assert K.same_bits(x, rhs / 4)
    finally:
        restore(ctx)


def test_scalars_refusals(ctx, mg):
    n = 64
    A = ctx.csr(n, n, *kr.banded(n, seed=250, spd=True).csr())
    h = build(ctx, mg, A, n)

    def code_of(fn):
        with pytest.raises(mg.MgsError) as e:
            fn()
        return e.value.code
    assert code_of(lambda: h.kcycle_scalars(-1)) == INVALID and code_of(lambda: h.kcycle_scalars(h.nlev)) == INVALID
    h.vcycle(ctx.vec(np.ones(n)))
    assert code_of(lambda: h.kcycle_scalars(0)) == STATE                  # no K step was ever switched on for the level
    assert mg.lib().mgs_hier_kcycle_scalars(h.h, 0, None) == INVALID
    h.set_kcycle_entry(1).vcycle(ctx.vec(np.ones(n)))
    assert h.kcycle_scalars(0)[0] > 0
    assert code_of(lambda: h.kcycle_scalars(1)) == STATE


# -------------------------------------------------------------------------------------------- 5. levels >= 1: the glue of coarse_solve
def weighted_five_point(n, seed):
    """SPD: the five-point pattern on rows of 264 points with symmetric off-diagonal values from −[0.5, 1] and a diagonal that exceeds the
    absolute row sum by [0.01, 0.05]"""
    rng = np.random.default_rng(seed)
    U = sps.triu(R.stencil_5pt(n, 264), 1).tocoo()
    S = sps.coo_matrix((-rng.uniform(0.5, 1.0, U.nnz), (U.row, U.col)), shape=(n, n)).tocsr()
    S = (S + S.T).tocsr()
    return (S + sps.diags(-np.asarray(S.sum(axis=1)).ravel() + rng.uniform(0.01, 0.05, n))).tocsr()


@pytest.fixture(scope="module")
def deep(ctx, mg):
    """a device-built hierarchy at 70 001 rows (pairwise aggregation, one pass per level: nine levels down to 550 rows) and the sub-hierarchy
    on its level-1 operator with its own aggregate maps pushed level by level.  The operator is a weighted five-point one, weakly
    dominant — the banded operators of tests/krylov_ref.py are so dominant that the matching leaves their rows alone and coarsening stops
    after one level"""
    n = 70_001
    A = upload(ctx, weighted_five_point(n, 260))
    h = mg.Hierarchy(A, OMEGA, 1, 1).coarsen(10.0, 1, 8.0, 600, 32).finalize()
    assert h.nlev >= 4, h.nlev
    sub = mg.Hierarchy(h.level_A(1), OMEGA, 1, 1)
    for l in range(1, h.nlev - 1):
        sub.push_P(upload(ctx, R.agg_P(h.level_P(l).agg(), h.level_shape(l + 1)[0])))
    sub.finalize()
    assert sub.nlev == h.nlev - 1
    for l in range(1, h.nlev):            # which level operator differs, if one does
        for name, p, q in zip(("rowptr", "col", "val"), h.level_A(l).download(), sub.level_A(l - 1).download()):
            assert np.array_equal(p, q) and (name != "val" or K.same_bits(p, q)), f"the sub-hierarchy's level {l - 1} operator differs from level {l}'s in {name}"
    return n, A, h, sub


@pytest.mark.parametrize("levels,sigma,energy", [(1, 1.0, 0), (1, 1.0, 1), (1, 1.6, 0), (1, 1.6, 1), (2, 1.6, 1)])
def test_kcycle_on_levels_below_the_fine_one(ctx, mg, deep, levels, sigma, energy):
    """mgs_hier_set_kcycle(levels) against the composition of pinned pieces: level 0's pre pass (mgs_hier_pre_pass_info), the sub-hierarchy's
    entry K step on r_c (with the K-cycle one level shorter below it), σ as k_axpby(σ, x, 0, x) applies it — one product —, level 0's post
    pass in the form its cycle runs"""
    n, A, h, sub = deep
    b = R.signed(np.random.default_rng(270 + levels), n)
    nc = h.level_shape(1)[0]
    try:
        ctx.set_option("kcycle_energy", energy)
        h.set_correction_scale(sigma).set_kcycle(levels)
        sub.set_correction_scale(sigma).set_kcycle(levels - 1).set_kcycle_entry(1)
        bv = ctx.vec(b)
        want = h.vcycle(bv).numpy()
        plain = h.set_kcycle(0).vcycle(bv).numpy()
        h.set_kcycle(levels)
        assert not K.same_bits(want, plain)                       # the K step is in the cycle under test
        t, r, rc = ctx.vec(n), ctx.vec(n), ctx.vec(nc)
        info = h.pre_pass_info(0, bv, t, r, rc)
        ec = sub.vcycle(rc).numpy()
        scal = sub.kcycle_scalars(0)
        assert scal == h.kcycle_scalars(1), ("level 1's scalars", scal, h.kcycle_scalars(1))
        if levels == 2:
            assert sub.kcycle_scalars(1) == h.kcycle_scalars(2)
        if sigma != 1.0:
            ec = sigma * ec
        x = ctx.vec(n)
        grouped = info["arm"] == GROUPED
        post = h.post_pass(0, t if grouped else r, None if grouped else bv, ctx.vec(ec), x)
        assert bool(post["t_form"]) == grouped, (info, post)
        got = x.numpy()
        print(f"levels={levels} σ={sigma} energy={energy}: {h.nlev} levels, pre arm {info['arm']}, post {post}, level 1's scalars {scal}")
        assert K.same_bits(got, want), ("x bits", np.flatnonzero(K.bits(got) != K.bits(want))[:8], float(np.abs(got - want).max()))
    finally:
        h.set_correction_scale(1.0).set_kcycle(0)
        sub.set_correction_scale(1.0).set_kcycle(0).set_kcycle_entry(0)
        restore(ctx)
