"""mgs_minres on the device against its numpy restatement (tests/minres_ref.py, pinned by tests/test_minres_ref_cpu.py).

1. Scalars and the update pass at their edges, in the form of tests/test_gpu_krylov_scalars.py: 12 fixed steps (tol = 1e-300, no
   preconditioner) on banded_sym(n) for n = 1, 2, 3 (below a pair, one pair, pair + tail), 511, 513 (one workgroup ± tail) and 1 048 579 (odd,
   thousands of workgroups), against the long-double run of the restatement; n <= 3 against the float64 run (status, count and x).
   Bar on x: every case measures and prints the distance of the float64 restatement from the long-double one; the bar is 1e-13 where that is
   at most 2e-16, else 500 × that distance.  Measured on the CPU: n = 1: 2.5e-17, 2: 1.2e-16, 3: 9.8e-17 (bar 1e-13); 511: 2.56e-16 (bar 1.28e-13),
   513: 3.73e-16 (bar 1.87e-13), 1 048 579: 2.67e-16 (bar 1.33e-13).
   n = 1 runs with b = (1): q, δ and v_new = 0 are exact, the method ends by γn == 0 with status 0 after one step on both sides.  n = 2 and 3
   reach the solution after n steps up to rounding; no exact zero decides anything there, the remaining steps run on rounding noise and move
   x below 1e-15: both sides end with status 1 after 12 steps.
2. Parity with the restatement under a hierarchy, with the bars of tests/test_gpu_pcg.py: status equal, iterations within max(2, it/6),
   x within 1e-8 relative at tol 1e-10, the oracle's true residual below 1.5·tol.  Operator: the 8³ saddle system (768 rows), uploaded from
   scipy.  Preconditioner: a hierarchy on block_diag(L, S) with three levels (768 → 108 → 14) from explicit P's, ω = 0.6, V(1,1), the same P's on
   both sides.  The oracle's aggregation orders its rows by a breadth-first search and takes connected graphs only, and block_diag(L, S) is not
   connected (S is diagonal here: every row of it is diagonally dominant and stays outside every aggregate), so the first P is the oracle's
   aggregation of L with empty rows below it for S; the second P is the oracle's aggregation of the Galerkin product, as it stands.
3. The recipe end to end on the device (README.md): K through Csr.bmat, S through scale, @ and add, the hierarchy through coarsen.
4. Exits and refusals.
5. The C++ face: MINRESiml on the 6³ system."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

import krylov_ref as kr
from conftest import REPO
from minres_ref import banded_sym, minres_ref, saddle, saddle_rhs

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
X_BAR = 1e-13
RESID_BAR = 1e-10
STEPS = 12
MGS_ERR_INVALID = -1


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


def dev(ctx, M):
    """scipy CSR or oracle Csr → device Csr"""
    if sps.issparse(M):
        M = M.tocsr()
        return ctx.csr(M.shape[0], M.shape[1], M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64))
    return ctx.csr(M.shape[0], M.shape[1], M.rowptr, M.col, M.val)


def to_scipy(A):
    rp, ci, v = A.download()
    return sps.csr_matrix((v, ci, rp), shape=A.shape)


def true_resid(K, x, b):
    return np.linalg.norm(b - K @ x) / np.linalg.norm(b)


# ------------------------------------------------------------------------------------------- 1. fixed steps on the banded operator
class Case:
    def __init__(self, ctx, n):
        self.n = n
        self.op = banded_sym(n, seed=200)
        self.A = ctx.csr(n, n, *self.op.csr())
        self.b = np.random.default_rng(n).standard_normal(n) if n > 3 else np.array([1.0, -0.5, 0.25][:n])
        r64 = minres_ref(self.op.apply, self.b, None, tol=1e-300, max_iter=STEPS)
        rld = minres_ref(self.op.apply, self.b, None, tol=1e-300, max_iter=STEPS, dtype=np.longdouble)
        self.r64, self.rld = r64, rld
        self.d64 = kr.rel(r64[3], rld[3])
        self.bar = X_BAR if self.d64 <= 2e-16 else 500 * self.d64
        nx = float(np.sqrt(kr.dot(rld[3], rld[3]))); nb = float(np.linalg.norm(self.b))
        # the reported number is the true residual of an FP64 x evaluated in FP64: 5 products + 5 additions per row, x itself rounded,
        # ‖A‖∞ <= 5.5 + 4·1 by construction (the floor of tests/test_gpu_krylov_scalars.py: true_residual_floor)
        self.floor = 8 * U * (9.5 * nx / nb + 1.0)


@pytest.fixture(scope="module")
def cases(ctx):
    made = {}

    def get(n):
        if n not in made:
            made[n] = Case(ctx, n)
        return made[n]
    return get


def check_fixed(tag, c, st, it, resid, x):
    st_r, it_r, res_r, x_r = c.rld if c.n > 3 else c.r64
    d = kr.rel(x, x_r)
    print(f"{tag}: status {st} after {it} (restatement {st_r} after {it_r}); GPU x vs {'long double' if c.n > 3 else 'float64 restatement'} {d:.3e} "
          f"(bar {c.bar:.2e}); float64 vs long double {c.d64:.3e}; resid {resid:.9e} vs {float(res_r):.9e} (floor {c.floor:.1e})")
    assert (st, it) == (st_r, it_r), (tag, st, it, st_r, it_r)
    assert d <= c.bar, (tag, d, c.bar)
    assert abs(resid - float(res_r)) <= RESID_BAR * float(res_r) + c.floor, (tag, resid, float(res_r))


@pytest.mark.parametrize("n", [1, 2, 3, 511, 513, 1_048_579])
def test_fixed_steps(ctx, mg, cases, n):
    c = cases(n)
    assert (c.r64[0], c.r64[1]) == ((0, 1) if n == 1 else (1, STEPS)), c.r64[:3]
    x = ctx.vec(n)
    st, it, resid = mg.minres(c.A, x, ctx.vec(c.b), None, STEPS, 1e-300)
    check_fixed(f"minres n={n}", c, st, it, resid, x.numpy())


def test_fixed_steps_8_byte_arm(ctx, mg, cases):
    """option blas1_vec = 0: the grid-stride kernels; k_minres_update computes every entry with the same expressions, so x differs from the
    16-byte run only through the sums (other orders)"""
    c = cases(513)
    try:
        ctx.set_option("blas1_vec", 0)
        x = ctx.vec(513)
        st, it, resid = mg.minres(c.A, x, ctx.vec(c.b), None, STEPS, 1e-300)
    finally:
        ctx.set_option("blas1_vec", 1)
    check_fixed("minres n=513 blas1_vec=0", c, st, it, resid, x.numpy())


def test_fixed_steps_misaligned_caller_vectors(ctx, mg, cases):
    """x and b start 8 bytes into longer buffers: the update pass takes its 8-byte arm (x is one of its four pointers), every scalar comes
    from library-owned aligned vectors, and the two arms compute an entry with the same expressions — x has the bits of the aligned run and
    the sentinels around the views are untouched"""
    n = 513
    c = cases(n)
    xa = ctx.vec(n)
    ref = mg.minres(c.A, xa, ctx.vec(c.b), None, STEPS, 1e-300)
    S1, S2 = 1.25e300, -7.5e-300
    bx = ctx.vec(np.concatenate([[S1], np.zeros(n), [S2]]))
    bb = ctx.vec(np.concatenate([[S2], c.b, [S1]]))
    wx, wb = mg.Vec.wrap(ctx, bx.ptr + 8, n), mg.Vec.wrap(ctx, bb.ptr + 8, n)
    assert wx.ptr % 16 == 8 and wb.ptr % 16 == 8
    st, it, resid = mg.minres(c.A, wx, wb, None, STEPS, 1e-300)
    fx, fb = bx.numpy(), bb.numpy()
    del wx, wb
    assert fx[0] == S1 and fx[-1] == S2 and fb[0] == S2 and fb[-1] == S1 and np.array_equal(fb[1:-1], c.b)
    check_fixed(f"minres n={n} misaligned", c, st, it, resid, fx[1:-1])
    assert np.array_equal(fx[1:-1], xa.numpy()) and (st, it, resid) == ref


@pytest.mark.parametrize("n", [1, 2, 3, 511, 513, 1_048_579])
def test_update_pass_alone_has_the_restatement_s_bits(ctx, mg, n):
    """k_minres_update through mgs_time_kernel (op 3: one launch with the coefficients inv_g = 0.7, a3 = −0.3, a2 = 1.9, a1 = 2.3, step = 1.1e-3:
    no product or quotient of them is exact, so a fused multiply-add or a reciprocal would show)
    against update_ref, bit for bit, on every arm: 16-byte lanes, 8-byte lanes by option and by a misaligned x, and the streaming store on
    w_prev (option minres_nt; it applies from nt_store's 1 000 000 rows on, so only the largest length takes it); the sentinels around the
    misaligned view are untouched"""
    from minres_ref import update_ref
    rng = np.random.default_rng(n)
    z, wp, w, x = (rng.standard_normal(n) for _ in range(4))
    wn, xn = update_ref(0.7, -0.3, 1.9, 2.3, 1.1e-3, z, wp, w, x)
    A = ctx.csr(n, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))
    zv, wv = ctx.vec(z), ctx.vec(w)
    try:
        for opt, val in (("blas1_vec", 1), ("blas1_vec", 0), ("minres_nt", 1)):
            ctx.set_option(opt, val)
            pv, xv = ctx.vec(wp), ctx.vec(x)
            A.time_kernel(mg.OP_MINRES_UPDATE, zv, wv, pv, xv, 1)
            assert np.array_equal(pv.numpy(), wn) and np.array_equal(xv.numpy(), xn), (n, opt, val)
            ctx.set_option(opt, 1 if opt == "blas1_vec" else 0)
    finally:
        ctx.set_option("blas1_vec", 1); ctx.set_option("minres_nt", 0)
    S1, S2 = 1.25e300, -7.5e-300
    buf = ctx.vec(np.concatenate([[S1], x, [S2]]))
    xw = mg.Vec.wrap(ctx, buf.ptr + 8, n)
    pv = ctx.vec(wp)
    A.time_kernel(mg.OP_MINRES_UPDATE, zv, wv, pv, xw, 1)
    got = buf.numpy()
    del xw
    assert got[0] == S1 and got[-1] == S2 and np.array_equal(got[1:-1], xn) and np.array_equal(pv.numpy(), wn)


# ------------------------------------------------------------------------------------------------ 2. parity under a hierarchy
def explicit_block_levels(orc, sd):
    """the two prolongations of the module docstring and block_diag(L, S), as oracle matrices"""
    B = sps.block_diag([sd["L"], sd["S"]], format="csr")
    PL = orc.Csr.from_scipy(sd["L"]).agmg(10.0, 2, 8.0, strict=False).to_scipy()
    P0 = orc.Csr.from_scipy(sps.vstack([PL, sps.csr_matrix((sd["m"], PL.shape[1]))], format="csr"))
    Bo = orc.Csr.from_scipy(B)
    P1 = Bo.galerkin(P0).agmg(10.0, 2, 8.0, strict=False)
    return Bo, [P0, P1]


class Saddle:
    def __init__(self, orc, N):
        self.sd = saddle(N)
        self.K = self.sd["K"]
        self.rows = self.K.shape[0]
        self.b = saddle_rhs(self.rows)
        self.Ko = orc.Csr.from_scipy(self.K)
        self.Bo, self.Ps = explicit_block_levels(orc, self.sd)
        self.ho = orc.Hier(self.Bo, self.Ps, omega=0.6, nu1=1, nu2=1)
        self._ref = {}

    def ref(self, tol):
        """the restatement with the oracle's cycle, once per tolerance"""
        if tol not in self._ref:
            self._ref[tol] = minres_ref(self.Ko, self.b, self.ho.vcycle, tol=tol, max_iter=500)
        return self._ref[tol]

    def hierarchy(self, mg, ctx, nu1=1, nu2=1):
        h = mg.Hierarchy(dev(ctx, self.Bo), 0.6, nu1, nu2)
        for P in self.Ps:
            h.push_P(dev(ctx, P))
        return h.finalize()


@pytest.fixture(scope="module")
def sad8(orc):
    return Saddle(orc, 8)


@pytest.fixture(scope="module")
def sad6(orc):
    return Saddle(orc, 6)


def explicit_run(mg, ctx, s, tol):
    """device solve with the explicit P's → (status, iterations, reported residual, x)"""
    h = s.hierarchy(mg, ctx)
    assert h.nlev == 3
    x = ctx.vec(s.rows)
    st, it, res = mg.minres(dev(ctx, s.K), x, ctx.vec(s.b), h, 500, tol)
    return st, it, res, x.numpy()


@pytest.mark.parametrize("tol", [1e-6, 1e-10])
def test_parity_with_the_restatement(ctx, mg, sad8, tol):
    s = sad8
    assert [P.shape for P in s.Ps] == [(768, 108), (108, 14)]
    st_r, it_r, res_r, x_r = s.ref(tol)
    st, it, res, xd = explicit_run(mg, ctx, s, tol)
    tr = np.linalg.norm(s.Ko.residual(xd, s.b)) / np.linalg.norm(s.b)
    d = kr.rel(xd, x_r)
    print(f"8³ saddle tol {tol:g}: device status {st}, {it} iterations, reported {res:.4e}, oracle's true residual {tr:.4e}; "
          f"restatement status {st_r}, {it_r} iterations, {res_r:.4e}; x rel diff {d:.3e}")
    assert st == 0 and st_r == 0
    assert abs(it - it_r) <= max(2, it_r // 6), (it, it_r)
    assert tr < 1.5 * tol
    assert abs(res - tr) <= 1e-6 * tr               # *tol is the true residual
    if tol <= 1e-10:
        assert d <= 1e-8


# ------------------------------------------------------------------------------------------- 3. the recipe, end to end on the device
def test_saddle_point_recipe_on_the_device(ctx, mg, sad8):
    s, sd = sad8, sad8.sd
    n, m, tol = sd["n"], sd["m"], 1e-8
    L, D = dev(ctx, sd["L"]), dev(ctx, sd["D"])
    C = mg.Csr.from_diag(ctx, ctx.vec(np.full(m, 1e-2)))
    Cm = mg.Csr.from_diag(ctx, ctx.vec(np.full(m, -1e-2)))
    Dt = D.transpose()
    K = mg.Csr.bmat(ctx, [[L, Dt], [D, Cm]])
    S = C + (D @ D.transpose().scale(left=L.diag_inv()))            # C + D·diag(L)⁻¹·Dᵀ
    h = mg.Hierarchy(mg.Csr.block_diag(ctx, [L, S]), 0.6, 1, 1).coarsen(10.0, 2, 8.0).finalize()
    Ks = to_scipy(K)
    assert abs(Ks - s.K).max() == 0.0 and abs(to_scipy(S) - sd["S"]).max() <= 4 * U
    b = ctx.vec(s.b)
    x = ctx.vec(n + m)
    st, it, res = mg.minres(K, x, b, h, 500, tol)
    tr = true_resid(Ks, x.numpy(), s.b)
    _, it_x, _, _ = explicit_run(mg, ctx, s, tol)
    xp = ctx.vec(n + m)
    st_p, it_p, res_p = mg.pcg(K, xp, b, h, 500, tol)
    xb = ctx.vec(n + m)
    st_b, it_b, res_b = mg.bicgstab(K, xb, b, h, 500, tol)
    tr_b = true_resid(Ks, xb.numpy(), s.b)
    print(f"recipe, 8³ saddle ({n + m} rows), device-built hierarchy of {h.nlev} levels, tol {tol:g}: MINRES status {st}, {it} iterations (cycles), reported "
          f"{res:.4e}, true {tr:.4e}; explicit P's {it_x} iterations; PCG status {st_p} at iteration {it_p}; BiCGSTAB status {st_b}, {it_b} "
          f"iterations ({2 * it_b} cycles), reported {res_b:.4e}, true {tr_b:.4e}")
    assert st == 0 and tr < 1.5 * tol
    assert it <= it_x + max(4, it_x // 4), (it, it_x)
    assert st_p == 3                                 # K is indefinite: that is why the solver exists
    assert st_b == 0 and res_b < tol
    # 768 rows lie below coarsen's default dense limit (2500 rows): the hierarchy above is the exact block solve.  The same recipe with the
    # limit at 50 rows aggregates on the device (S's rows are diagonally dominant and stay outside every aggregate), held to the same margin
    h2 = mg.Hierarchy(mg.Csr.block_diag(ctx, [L, S]), 0.6, 1, 1).coarsen(10.0, 2, 8.0, 50).finalize()
    x2 = ctx.vec(n + m)
    st2, it2, res2 = mg.minres(K, x2, b, h2, 500, tol)
    tr2 = true_resid(Ks, x2.numpy(), s.b)
    print(f"  dense limit 50: {h2.nlev} levels {[h2.level_shape(l)[0] for l in range(h2.nlev)]}, MINRES status {st2}, {it2} iterations, true {tr2:.4e}")
    assert h2.nlev >= 3 and st2 == 0 and tr2 < 1.5 * tol
    assert it2 <= it_x + max(4, it_x // 4), (it2, it_x)


# ------------------------------------------------------------------------------------------------------ 4. exits and refusals
def test_status_2_negative_definite_preconditioner(ctx, mg, sad6):
    """a one-level hierarchy on −L: its dense coarse solve is (−L)⁻¹, z̃·v < 0 at the start"""
    L = sad6.sd["L"]; n = L.shape[0]
    h = mg.Hierarchy(dev(ctx, -L), 0.6, 1, 1).finalize()
    assert h.nlev == 1
    x = ctx.vec(n)
    st, it, res = mg.minres(dev(ctx, L), x, ctx.vec(saddle_rhs(n)), h, 50, 1e-8)
    assert (st, it) == (2, 0) and res == 1.0 and not x.numpy().any()


def test_status_3_and_the_two_by_two_cases(ctx, mg):
    i32 = np.int32
    # [[1, 0], [0, 0]], b = (0, 1): singular and inconsistent, dyadic throughout; a1 == 0 at iteration 1, x is not updated
    A = ctx.csr(2, 2, np.array([0, 1, 1], i32), np.array([0], i32), np.array([1.0]))
    x = ctx.vec(2)
    st, it, res = mg.minres(A, x, ctx.vec(np.array([0.0, 1.0])), None, 10, 1e-12)
    assert (st, it) == (3, 1) and res == 1.0 and not x.numpy().any()
    x = ctx.vec(np.array([0.25, -0.5]))                     # the same residual from a guess that is not zero: x comes back as it went in
    st, it, res = mg.minres(A, x, ctx.vec(np.array([0.25, 1.0])), None, 10, 1e-12)
    assert (st, it) == (3, 1) and res == 1.0 / np.sqrt(0.0625 + 1.0) and np.array_equal(x.numpy(), [0.25, -0.5])
    # [[0, 1], [1, 0]], b = (1, 0): status 0 in 2 iterations, x = (0, 1)
    A = ctx.csr(2, 2, np.array([0, 1, 2], i32), np.array([1, 0], i32), np.array([1.0, 1.0]))
    x = ctx.vec(2)
    st, it, res = mg.minres(A, x, ctx.vec(np.array([1.0, 0.0])), None, 10, 1e-12)
    assert (st, it) == (0, 2) and res == 0.0 and np.array_equal(x.numpy(), [0.0, 1.0])
    # diag(1, −1), b = (1, 1): status 0 in 2 iterations
    A = ctx.csr(2, 2, np.array([0, 1, 2], i32), np.array([0, 1], i32), np.array([1.0, -1.0]))
    x = ctx.vec(2)
    st, it, res = mg.minres(A, x, ctx.vec(np.array([1.0, 1.0])), None, 10, 1e-12)
    assert (st, it) == (0, 2) and res < 1e-12 and np.allclose(x.numpy(), [1.0, -1.0], rtol=0, atol=1e-15)
    # b = 0: converged before the first step, x untouched
    x = ctx.vec(2)
    st, it, res = mg.minres(A, x, ctx.vec(2), None, 10, 1e-12)
    assert (st, it) == (0, 0) and res == 0.0 and not x.numpy().any()


def test_status_1_reports_the_true_residual(ctx, mg, sad6):
    s = sad6
    h = s.hierarchy(mg, ctx)
    x = ctx.vec(s.rows)
    st, it, res = mg.minres(dev(ctx, s.K), x, ctx.vec(s.b), h, 3, 1e-10)
    tr = true_resid(s.K, x.numpy(), s.b)
    st_r, it_r, res_r, _ = minres_ref(s.Ko, s.b, s.ho.vcycle, tol=1e-10, max_iter=3)
    print(f"max_iter 3 on the 6³ saddle: reported {res:.12e}, recomputed {tr:.12e}, restatement {res_r:.12e}")
    assert (st, it) == (1, 3) == (st_r, it_r)
    assert abs(res - tr) <= 1e-12 * tr
    x0 = ctx.vec(s.rows)
    st, it, res = mg.minres(dev(ctx, s.K), x0, ctx.vec(s.b), h, 0, 1e-10)
    assert (st, it) == (1, 0) and res == 1.0 and not x0.numpy().any()


def test_refusals(ctx, mg, sad6):
    s = sad6
    K, b, x = dev(ctx, s.K), ctx.vec(s.b), ctx.vec(s.rows)

    def refused(what, *args):
        with pytest.raises(mg.MgsError) as e:
            mg.minres(*args)
        print(f"{what}: {e.value}")
        assert e.value.code == MGS_ERR_INVALID and "mgs_minres" in str(e.value), (what, str(e.value))
    refused("V(2,1)", K, x, b, s.hierarchy(mg, ctx, 2, 1), 10, 1e-8)
    hk = s.hierarchy(mg, ctx).set_kcycle(1)
    refused("K-cycle", K, x, b, hk, 10, 1e-8)
    refused("K-cycle at the entry", K, x, b, s.hierarchy(mg, ctx).set_kcycle_entry(True), 10, 1e-8)
    refused("x aliasing b", K, b, b, None, 10, 1e-8)
    refused("short x", K, ctx.vec(s.rows - 1), b, None, 10, 1e-8)
    refused("short b", K, x, ctx.vec(s.rows - 1), None, 10, 1e-8)
    Kn = dev(ctx, s.K).set_nullspace("constant")
    refused("declared null space", Kn, x, b, None, 10, 1e-8)
    refused("rectangular", dev(ctx, s.K[:-1, :]), x, b, None, 10, 1e-8)
    assert not x.numpy().any() and np.array_equal(b.numpy(), s.b)
    # what mgs_pcg allows with flexible = 0 is allowed here: the additive form, a correction scale, FP32 operands
    for tweak in (lambda h: h.set_additive(True), lambda h: h.set_correction_scale(1.1), lambda h: h.set_operand_precision(32)):
        h = tweak(s.hierarchy(mg, ctx))
        x.fill(0.0)
        st, it, res = mg.minres(K, x, b, h, 500, 1e-6)
        assert st == 0 and true_resid(s.K, x.numpy(), s.b) < 1.5e-6


def test_repeated_solve_same_bits_and_two_graph_slots(ctx, mg, sad8):
    s = sad8
    h = s.hierarchy(mg, ctx)
    K, b = dev(ctx, s.K), ctx.vec(s.b)
    runs, graphs = [], []
    for _ in range(3):
        x = ctx.vec(s.rows)
        runs.append(mg.minres(K, x, b, h, 500, 1e-8) + (x.numpy(),))
        graphs.append(h.graph_info()["captured_cycles"])
    print(f"three solves: {[r[:3] for r in runs]}, captured cycles after each {graphs}")
    assert runs[0][0] == 0
    for r in runs[1:]:
        assert r[:3] == runs[0][:3] and np.array_equal(r[3], runs[0][3])
    assert graphs[0] == 2 and graphs[2] == graphs[1] == graphs[0]      # the two (v, z̃) pairs, found again at the same addresses


# ---------------------------------------------------------------------------------------------------------- 5. the C++ face
TU = r"""
#include <fstream>
#include "mgs_host.hpp"
using namespace mgs;
int main(int argc, char **argv) {
  if (argc != 6) { std::cout << "usage: K.mtx B.mtx P.mtx b.bin x.bin" << std::endl; return 1; }
  SMatrix K = readMatrix(argv[1]), B = readMatrix(argv[2]), P = readMatrix(argv[3]);
  std::vector<double> hb((size_t)K.rows());
  { std::ifstream f(argv[4], std::ios::binary); f.read((char *)hb.data(), (std::streamsize)(hb.size() * sizeof(double))); if (!f) return 2; }
  MultiGridPrecond::Options o; o.omega = 0.6;
  MultiGridPrecond precond(B, P, o);               // the preconditioner's operator is block_diag(L, S), not K
  DeviceMatrix Kd(K);
  VectorXd x(K.rows()), b(K.rows());
  x.setZero(); b.upload(hb);
  int max_iter = 500; double tol = 1e-8;
  int status = MINRESiml(Kd, x, b, precond, max_iter, tol);
  std::cout.precision(17);
  std::cout << "MINRES " << status << " " << max_iter << " " << tol << std::endl;
  std::vector<double> hx = x.download();
  { std::ofstream f(argv[5], std::ios::binary); f.write((const char *)hx.data(), (std::streamsize)(hx.size() * sizeof(double))); }
  return 0;
}
"""


def test_cpp_minresiml(mg, sad6, tmp_path):
    s = sad6
    libdir = os.path.join(REPO, "multigridsolver_amd")
    src = tmp_path / "minres_gpu_tu.cpp"; src.write_text(TU)
    exe = tmp_path / "minres_gpu_tu"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O1", "-Wall", "-I", os.path.join(libdir, "cpp"), "-o", str(exe), str(src),
                        "-L" + libdir, "-lmgs", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    paths = {k: str(tmp_path / (k + ".mtx")) for k in ("K", "B", "P")}
    for k, M in (("K", s.K), ("B", s.Bo.to_scipy()), ("P", s.Ps[0].to_scipy())):
        M = M.tocsr(); M.sort_indices()
        mg.write_mtx(paths[k], M.shape[0], M.shape[1], M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64))
    b_bin, x_bin = str(tmp_path / "b.bin"), str(tmp_path / "x.bin")
    s.b.astype("<f8").tofile(b_bin)
    r = subprocess.run(["timeout", "-k", "10", "240", str(exe), paths["K"], paths["B"], paths["P"], b_bin, x_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    word, st, it, res = r.stdout.split()[-4:]
    x = np.fromfile(x_bin, dtype="<f8")
    tr = true_resid(s.K, x, s.b)
    print(f"MINRESiml on the 6³ saddle: status {st}, {it} iterations, reported {res}, recomputed {tr:.4e}")
    assert word == "MINRES" and int(st) == 0 and 0 < int(it) < 500
    assert tr < 1.5e-8 and abs(float(res) - tr) <= 1e-6 * tr
