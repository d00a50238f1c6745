"""The scalars of the Krylov solvers (mgs_dot / mgs_nrm2, the pair reductions, the update-with-dots passes, the PCG passes, the
multi-dot and multi-update passes, the SpMV epilogue's inner products) against extended-precision references, at the lengths where
their launchers change path (multigridsolver_amd/csrc/blas1.hip, kernels_spmv.hip: mgs_spmv_dots and the coded kernel's epilogue):

    n                 why
    1, 2, 3           below one pair, one pair, pair + tail
    511, 513          one workgroup ± tail
    1 048 579         odd; the SpMV epilogue has 4097 row-block pairs -> three-stage fold (dot2_mid_kernel); the dot kernels pass
                      2048 pairs -> grown scratch (mgs_ensure_dot_part)
    2 097 665         odd; the 16-byte dot kernels have 4098 workgroups -> three-stage fold
    4 195 329         odd; the multi-update pass has 4098 workgroups -> three-stage fold

The solvers run a FIXED number of steps (tol = 1e-300) on the banded operators of tests/krylov_ref.py and are compared with the
long-double restatements there (pinned by tests/test_krylov_ref_cpu.py).  Bar on x: 1e-13 relative.  The float64 run of the same
restatement sits 1.2e-16 .. 2.0e-16 from the long-double one at these lengths (each test measures and prints it), so 1e-13 is about
500 times the distance of a correct FP64 implementation; one element dropped from one inner product moves x by 1e-7 or more.
Every test prints its measured distances."""
import math

import numpy as np
import pytest

import krylov_ref as kr

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LARGE = (1_048_579, 2_097_665, 4_195_329)
X_BAR = 1e-13
RESID_BAR = 1e-10
DEFAULTS = {"fuse_dots": 1, "blas1_vec": 1, "blas1_pairs": 1, "post_results": 1}

# Longest chain of additions behind one term of a reduction, counted from the kernels (TB = 256 lanes, DOT_BLOCKS = 4096 slots):
#  * 16-byte kernels (dot_block_vec_kernel), default options — one pair per lane, one-shot workgroups:
#      2 products per lane + the odd tail on lane 0 (3), 6 shuffle levels, 4 waves, then
#        up to 4096 workgroups: dot2_final_kernel, <= 16 strided adds + 8 tree levels              3 + 6 + 4 + 16 + 8 = 37
#        above:                 dot2_mid_kernel (chunk <= 256: 1 strided, 6 shuffle levels, 4 waves), then dot2_final_kernel over
#                               256 chunk sums (1 strided + 8 tree levels)                         3 + 6 + 4 + 11 + 9 = 33
#    blas1_pairs = 2 at 2 097 665: 2049 workgroups, 4 products + tail (5), 6, 4, 9 strided, 8                        = 32
#    blas1_pairs = 0 (256 CUs x 8 = 2048 workgroups) at 2 097 665: 3 pairs per lane + tail (7), 6, 4, 8 strided, 8   = 33
#  * 8-byte kernels (dot_partial_kernel: blas1_vec = 0, n = 1, operands off 16-byte alignment) — grid-stride over at most 4096
#    workgroups: ceil(n / (4096 * 256)) products per lane, 6 shuffle levels, 4 waves, dot_final_kernel 16 strided + 8 tree levels.
CHAIN_VEC = 37


def chain_scalar(n):
    return math.ceil(n / (4096 * 256)) + 6 + 4 + 16 + 8


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


class Case:
    """one banded operator: slice form, uploaded CSR form, right-hand side"""

    def __init__(self, ctx, n, spd):
        self.n, self.spd = n, spd
        self.op = kr.banded(n, seed=100 + int(spd), spd=spd)
        self.A = ctx.csr(n, n, *self.op.csr())
        self.b = np.random.default_rng(n + int(spd)).standard_normal(n)
        self.apply = self.op.apply


@pytest.fixture(scope="module")
def cases(ctx):
    made = {}

    def get(n, spd=False):
        if (n, spd) not in made:
            made[(n, spd)] = Case(ctx, n, spd)
        return made[(n, spd)]
    return get


_REFS = {}


def reference(case, solver, steps, restart=0, keep=False):
    """(x_longdouble, resid_longdouble, distance of the float64 run of the same restatement from it); computed once per key when `keep`"""
    key = (case.n, case.spd, solver, steps, restart)
    if key in _REFS:
        return _REFS[key]
    x0 = np.zeros(case.n)
    if solver == "bicgstab" and keep and steps in (1, 3):       # one run of three steps serves the one-step case as well
        snap = {t: {1: None} for t in (np.longdouble, np.float64)}
        full = {t: kr.bicgstab_fixed(case.apply, case.b, x0, 3, dtype=t, snapshots=snap[t]) for t in snap}
        for k, pick in ((1, lambda t: snap[t][1]), (3, lambda t: full[t])):
            (xld, rld), (x64, _) = pick(np.longdouble), pick(np.float64)
            _REFS[(case.n, case.spd, solver, k, restart)] = (xld, float(rld), kr.rel(x64, xld))
        return _REFS[key]

    def run(t):
        if solver == "bicgstab":
            return kr.bicgstab_fixed(case.apply, case.b, x0, steps, dtype=t)
        if solver == "fgcr":
            return kr.fgcr_fixed(case.apply, case.b, x0, steps, restart, dtype=t)
        return kr.pcg_fixed(case.apply, case.b, x0, steps, flexible=(solver == "fpcg"), dtype=t)
    xld, rld = run(np.longdouble)
    x64, _ = run(np.float64)
    out = (xld, float(rld), kr.rel(x64, xld))
    if keep:
        _REFS[key] = out
    return out


def run_gpu(mg, ctx, A, solver, b, steps, restart=0, x=None):
    bv = b if isinstance(b, mg.Vec) else ctx.vec(b)
    x = ctx.vec(len(bv)) if x is None else x
    if solver == "bicgstab":
        st, it, resid = mg.bicgstab(A, x, bv, None, steps, 1e-300)
    elif solver == "fgcr":
        st, it, resid = mg.fgcr(A, x, bv, None, restart, steps, 1e-300)
    else:
        st, it, resid = mg.pcg(A, x, bv, None, steps, 1e-300, flexible=(solver == "fpcg"))
    return st, it, resid, x


def check_fixed(tag, got, ref, steps, x_bar=X_BAR, resid_floor=0.0):
    st, it, resid, x = got
    xld, rld, d64 = ref
    d = kr.rel(x.numpy(), xld)
    print(f"{tag}: GPU vs long double x {d:.3e} (bar {x_bar:.1e}), float64 vs long double {d64:.3e}; resid {resid:.9e} vs {rld:.9e}")
    assert st == 1 and it == steps, (tag, st, it)
    assert d <= x_bar, (tag, d)
    assert abs(resid - rld) <= RESID_BAR * rld + resid_floor, (tag, resid, rld, resid_floor)


def true_residual_floor(case, xld):
    """mgs_fgcr reports the TRUE residual ‖b − A·x‖/‖b‖ of an FP64 x, evaluated in FP64: whatever the method has reached, that number
    carries an absolute error of up to (5 products + 5 additions per row, x itself rounded: 8 roundings)·u·(‖A‖∞·‖x‖ + ‖b‖)/‖b‖, with
    ‖A‖∞ <= 5.5 + 4·1 by the operator's construction.  It matters only once the residual is down at rounding level (GCR(20), 41 steps)."""
    nx = float(np.sqrt(kr.dot(xld, xld))); nb = float(np.linalg.norm(case.b))
    return 8 * U * (9.5 * nx / nb + 1.0)


# ------------------------------------------------------------------------------------------------------- 1. mgs_dot / mgs_nrm2
def exact_dot(x, y):
    """(Σ x_i·y_i, Σ |x_i·y_i|): products in long double (64 of their 106 bits), each split into two doubles, summed exactly by math.fsum —
    the reference's error is 2^-64 per product, 2000 times below the rounding unit of the sums under test"""
    p = x.astype(np.longdouble) * y.astype(np.longdouble)
    hi = p.astype(np.float64)
    lo = (p - hi).astype(np.float64)
    return math.fsum(hi.tolist() + lo.tolist()), float(np.abs(p).sum())


def make_inputs(n, wide):
    rng = np.random.default_rng(1000 + n + int(wide))
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    if wide:                                   # dynamic range 1e8: magnitudes spread over 1e-4 .. 1e4
        x *= 10.0 ** rng.uniform(-4, 4, n); y *= 10.0 ** rng.uniform(-4, 4, n)
    return x, y


def check_dot(tag, vx, vy, x, y, chain):
    c = chain + 2
    ref, sabs = exact_dot(x, y)
    got = vx.dot(vy)
    err = abs(got - ref)
    ref2, _ = exact_dot(x, x)
    gn = vx.nrm2()
    # ‖x‖ = sqrt(s), s = Σx²·(1 + δ), |δ| <= c·u: relative error c·u/2, plus one u for the square root's rounding and one for the second-order terms
    nbar = (c / 2 + 2) * U * math.sqrt(ref2)
    nerr = abs(gn - math.sqrt(ref2))
    print(f"{tag}: dot err {err:.3e} = {err / (U * sabs):.2f} u·Σ|xy| (c = {c}); nrm2 err {nerr:.3e} = {nerr / (U * math.sqrt(ref2)):.2f} u·‖x‖ (bar {c / 2 + 2:.1f})")
    assert err <= c * U * sabs, (tag, err, c * U * sabs)
    assert nerr <= nbar, (tag, nerr, nbar)


@pytest.mark.parametrize("wide", [False, True], ids=["normal", "range1e8"])
@pytest.mark.parametrize("n", (1, 2, 3, 511, 513) + LARGE)
def test_dot_nrm2_exact_sum(ctx, mg, n, wide):
    x, y = make_inputs(n, wide)
    check_dot(f"n={n}", ctx.vec(x), ctx.vec(y), x, y, CHAIN_VEC if n >= 2 else chain_scalar(n))
    # both operands 8 bytes into a longer buffer: the al16() checks select the 8-byte kernels
    bx, by = ctx.vec(np.concatenate([[7.0], x, [7.0]])), ctx.vec(np.concatenate([[-3.0], y, [-3.0]]))
    wx, wy = mg.Vec.wrap(ctx, bx.ptr + 8, n), mg.Vec.wrap(ctx, by.ptr + 8, n)
    check_dot(f"n={n} misaligned", wx, wy, x, y, chain_scalar(n))
    del wx, wy


@pytest.mark.parametrize("opt,val,chain", [("blas1_vec", 0, chain_scalar(2_097_665)), ("blas1_pairs", 0, CHAIN_VEC), ("blas1_pairs", 2, CHAIN_VEC),
                                           ("post_results", 0, CHAIN_VEC)])
def test_dot_nrm2_options(ctx, mg, opt, val, chain):
    n = 2_097_665
    try:
        ctx.set_option(opt, val)
        for wide in (False, True):
            x, y = make_inputs(n, wide)
            check_dot(f"n={n} {opt}={val} wide={wide}", ctx.vec(x), ctx.vec(y), x, y, chain)
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)


# ------------------------------------------------------------------------------------------------------- 2. fixed-step BiCGSTAB
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("n", (513,) + LARGE)
def test_bicgstab_fixed_steps(ctx, mg, cases, n, steps):
    c = cases(n)
    check_fixed(f"bicgstab n={n} steps={steps}", run_gpu(mg, ctx, c.A, "bicgstab", c.b, steps), reference(c, "bicgstab", steps, keep=True), steps)


@pytest.mark.parametrize("opt", ["fuse_dots", "blas1_vec", "blas1_pairs", "post_results"])
def test_bicgstab_fixed_steps_options(ctx, mg, cases, opt):
    """the separate-pass, 8-byte, capped-grid and copy-back forms of the same reductions, against the same reference"""
    n = 2_097_665
    c = cases(n)
    try:
        ctx.set_option(opt, 0)
        for steps in (1, 3):
            check_fixed(f"bicgstab n={n} steps={steps} {opt}=0", run_gpu(mg, ctx, c.A, "bicgstab", c.b, steps), reference(c, "bicgstab", steps, keep=True), steps)
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)


# ------------------------------------------------------------------------------------------------------------ 3. stale partials
def test_stale_partials_of_a_larger_launch(mg, cases):
    """a solve at 4 195 329 with b scaled by 1e100 leaves partials of about 1e200 in the context's scratch; the shorter solves that follow
    in the SAME context must read only what their own launches wrote — a fold that reads one stale slot misses the bar by hundreds of
    orders of magnitude"""
    ctx2 = mg.Context(0)
    try:
        big = cases(LARGE[2])
        A = ctx2.csr(big.n, big.n, *big.op.csr())
        st, it, resid, x = run_gpu(mg, ctx2, A, "bicgstab", big.b * 1e100, 2)
        assert st == 1 and it == 2 and np.isfinite(resid)
        assert 1e98 < np.abs(x.numpy()).max() < 1e102
        del A, x
        for n in (LARGE[0], 513):
            c = cases(n)
            A = ctx2.csr(n, n, *c.op.csr())
            for steps in (1, 3):
                check_fixed(f"after the 1e100 solve: bicgstab n={n} steps={steps}", run_gpu(mg, ctx2, A, "bicgstab", c.b, steps),
                            reference(c, "bicgstab", steps, keep=True), steps)
            del A
    finally:
        ctx2.close()


# ------------------------------------------------------------------------------------- 4. mixed row blocks under the SpMV epilogue
def irregular(op, spd, long_row=False, seed=0):
    """the banded operator with about 30 % of its 256-row blocks (the last, partial one among them) made irregular: every row of such a
    block gets 2..6 extra entries in columns of its own block (values −[0.01, 0.05]; the SPD variant gets the transposed entries too, which
    stay inside the block), so that the block's rows all differ and it is left uncoded, while the other blocks keep their pattern code.  The
    diagonal grows by the extras' absolute row sum: dominance (and positive definiteness) is kept.  One row in the middle of an irregular
    block is emptied (the SPD variant loses the column as well): a row without a pattern between irregular neighbours.
    long_row: one row of a regular block gets 195 more entries (200 in all)."""
    import scipy.sparse as sps
    n = op.n
    rng = np.random.default_rng(seed)
    M = sps.csr_matrix(op.csr()[::-1], shape=(n, n)).tocoo()
    nblk = (n + 255) // 256
    pick = rng.choice(np.arange(1, nblk - 1), size=int(0.3 * nblk) - 1, replace=False)
    pick = np.sort(np.append(pick, nblk - 1))
    rows, cols, vals = [], [], []
    for blk in pick:
        r0, r1 = blk * 256, min(blk * 256 + 256, n)
        k = rng.integers(2, 7, r1 - r0)
        r = np.repeat(np.arange(r0, r1), k)
        cshift = rng.integers(2, r1 - r0 - 2, r.size)                 # never the row itself or its ±1 neighbours' slot twice the same way
        cc = r0 + (r - r0 + cshift) % (r1 - r0)
        rows.append(r); cols.append(cc); vals.append(-rng.uniform(0.01, 0.05, r.size))
    if long_row:
        regular = np.setdiff1d(np.arange(1, nblk - 1), pick)
        lr = int(regular[len(regular) // 2]) * 256 + 100
        cc = lr + 2 + 3 * np.arange(1, 196)                           # 195 columns to the right, none of them a band column of this row
        cc = cc[(cc != lr + kr.BAND)][:195]
        rows.append(np.full(cc.size, lr)); cols.append(cc); vals.append(np.full(cc.size, -0.001))
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    E = sps.coo_matrix((v, (r, c)), shape=(n, n)).tocsr()                # duplicates summed
    if spd:
        E = E + E.T                                                      # (one addition per entry: symmetric to the bit)
    D = sps.diags(np.asarray(abs(E).sum(axis=1)).ravel())
    M = (M.tocsr() + E + D).tocoo()
    e = int(pick[len(pick) // 2]) * 256 + 128                          # the emptied row
    keep = (M.row != e) & ((M.col != e) if spd else True)
    M = sps.coo_matrix((M.data[keep], (M.row[keep], M.col[keep])), shape=(n, n)).tocsr()
    M.sort_indices()
    return M, e


@pytest.mark.parametrize("kind", ["mixed", "long_row", "regular"])
def test_spmv_epilogue_dots_on_mixed_row_blocks(ctx, mg, kind):
    n = 300_007
    nblk = (n + 255) // 256
    for spd, solver in ((False, "bicgstab"), (True, "pcg")):
        op = kr.banded(n, seed=40 + int(spd), spd=spd)
        if kind == "regular":
            rp, ci, v = op.csr()
        else:
            M, e = irregular(op, spd, long_row=(kind == "long_row"), seed=7)
            rp, ci, v = M.indptr, M.indices, M.data
            assert rp[e] == rp[e + 1] and (np.diff(rp).max() == 200 if kind == "long_row" else np.diff(rp).max() <= 64)
            if spd:
                assert abs(M - M.T).max() == 0.0
            off = np.asarray(abs(M).sum(axis=1)).ravel() - abs(M.diagonal())
            assert np.all((M.diagonal() > off) | (np.arange(n) == e))
        A = ctx.csr(n, n, rp, ci, v).optimize()
        info, plan = A.rowcode_info(), A.plan_info()
        print(f"{kind} spd={spd}: rowcode {info}, max_row_len {plan['max_row_len']}")
        assert info["blocks"] == nblk
        if kind == "mixed":
            assert plan["max_row_len"] <= 64
            assert 0.5 * info["blocks"] <= info["coded_blocks"] < info["blocks"]      # coded and uncoded blocks share the fused launch
        elif kind == "long_row":
            assert plan["max_row_len"] >= 200                                          # > 64: the launcher takes the unfused path
        else:
            assert info["coded_blocks"] == info["blocks"]
        b = np.random.default_rng(n + int(spd)).standard_normal(n)
        x0 = np.zeros(n)

        def apply(x):
            return kr.csr_apply(rp, ci, v, x)
        run = (lambda t: kr.bicgstab_fixed(apply, b, x0, 1, dtype=t)) if solver == "bicgstab" else (lambda t: kr.pcg_fixed(apply, b, x0, 1, dtype=t))
        xld, rld = run(np.longdouble)
        x64, _ = run(np.float64)
        check_fixed(f"{kind} {solver} n={n}", run_gpu(mg, ctx, A, solver, b, 1), (xld, float(rld), kr.rel(x64, xld)), 1)


# ------------------------------------------------------------------------------------------------- 5. fixed-step PCG and FGCR
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("solver", ["pcg", "fpcg"])
@pytest.mark.parametrize("n", (513, LARGE[1], LARGE[2]))
def test_pcg_fixed_steps(ctx, mg, cases, n, solver, steps):
    c = cases(n, spd=True)
    check_fixed(f"{solver} n={n} steps={steps}", run_gpu(mg, ctx, c.A, solver, c.b, steps), reference(c, solver, steps), steps)


def test_fgcr_fixed_steps_large(ctx, mg, cases):
    """GCR(3), 7 steps: two window closures and one open window; the multi-update pass has 4098 workgroups"""
    c = cases(LARGE[2])
    ref = reference(c, "fgcr", 7, restart=3)
    check_fixed(f"fgcr(3) n={c.n} steps=7", run_gpu(mg, ctx, c.A, "fgcr", c.b, 7, restart=3), ref, 7, resid_floor=true_residual_floor(c, ref[0]))


def test_fgcr_fixed_steps_long_window(ctx, mg, cases):
    """GCR(20) at n = 100 003: windows of more than 16 vectors, i.e. more than one multi-vector pass per orthogonalisation.  20 steps: the
    first window alone, its closure included.  41 steps: two closures and one open window; by then the float64 restatement itself may have
    moved away from the long-double one, so the bar is raised — only — to 50 times that measured distance where this exceeds 1e-13.  On
    this well-conditioned operator the method is at rounding level after about 30 steps: the reported true residual is then compared up to
    the rounding of its own FP64 evaluation (true_residual_floor)."""
    c = cases(100_003)
    for steps in (20, 41):
        ref = reference(c, "fgcr", steps, restart=20)
        bar = max(X_BAR, 50 * ref[2])
        print(f"fgcr(20) n={c.n} steps={steps}: float64 vs long double {ref[2]:.3e} -> bar {bar:.3e}")
        check_fixed(f"fgcr(20) n={c.n} steps={steps}", run_gpu(mg, ctx, c.A, "fgcr", c.b, steps, restart=20), ref, steps, x_bar=bar,
                    resid_floor=true_residual_floor(c, ref[0]))


# --------------------------------------------------------------------------------------------------- 6. misaligned caller vectors
@pytest.mark.parametrize("solver", ["bicgstab", "pcg", "fgcr"])
def test_misaligned_caller_vectors(ctx, mg, cases, solver):
    """x and b start 8 bytes into longer buffers, so every launcher that touches them takes its 8-byte kernel; every scalar comes from
    library-owned (aligned) vectors and the x updates are element-wise with the same expression in both kernel forms: x has the bits of
    the aligned run, and the sentinels around the views are untouched"""
    n = 100_003
    c = cases(n, spd=(solver == "pcg"))
    restart = 3 if solver == "fgcr" else 0
    got = run_gpu(mg, ctx, c.A, solver, c.b, 3, restart=restart)
    ref = reference(c, solver, 3, restart=restart)
    floor = true_residual_floor(c, ref[0]) if solver == "fgcr" else 0.0
    check_fixed(f"{solver} n={n} aligned", got, ref, 3, resid_floor=floor)
    S1, S2 = 1.25e300, -7.5e-300
    bx = ctx.vec(np.concatenate([[S1], np.zeros(n), [S2]]))
    bb = ctx.vec(np.concatenate([[S2], c.b, [S1]]))
    wx, wb = mg.Vec.wrap(ctx, bx.ptr + 8, n), mg.Vec.wrap(ctx, bb.ptr + 8, n)
    assert wx.ptr % 16 == 8 and wb.ptr % 16 == 8
    st, it, resid, _ = run_gpu(mg, ctx, c.A, solver, wb, 3, restart=restart, x=wx)
    fx, fb = bx.numpy(), bb.numpy()
    assert fx[0] == S1 and fx[-1] == S2 and fb[0] == S2 and fb[-1] == S1 and np.array_equal(fb[1:-1], c.b)
    check_fixed(f"{solver} n={n} misaligned", (st, it, resid, ctx.vec(fx[1:-1])), ref, 3, resid_floor=floor)
    assert np.array_equal(fx[1:-1], got[3].numpy())
    assert resid == got[2]
    del wx, wb


# ------------------------------------------------------------------------------------------------------------ 7. degenerate calls
@pytest.mark.parametrize("solver", ["bicgstab", "pcg", "fpcg", "fgcr"])
def test_degenerate_calls(ctx, mg, cases, solver):
    spd = solver in ("pcg", "fpcg")

    def solve(A, x, b, max_iter, tol):
        if solver == "bicgstab":
            return mg.bicgstab(A, x, b, None, max_iter, tol)
        if solver == "fgcr":
            return mg.fgcr(A, x, b, None, 3, max_iter, tol)
        return mg.pcg(A, x, b, None, max_iter, tol, flexible=(solver == "fpcg"))
    c = cases(513, spd=spd)
    # b = 0: converged before the first step, x untouched
    x = ctx.vec(513)
    st, it, resid = solve(c.A, x, ctx.vec(np.zeros(513)), 50, 1e-10)
    assert (st, it) == (0, 0) and resid == 0.0 and not x.numpy().any()
    # x0 solves the system to the tolerance already
    import scipy.sparse as sps
    rp, ci, v = c.op.csr()
    M = sps.csr_matrix((v, ci, rp), shape=(513, 513))
    xs = np.linalg.solve(M.toarray(), c.b)
    x = ctx.vec(xs)
    st, it, resid = solve(c.A, x, ctx.vec(c.b), 50, 1e-10)
    assert (st, it) == (0, 0) and resid <= 1e-14 and np.array_equal(x.numpy(), xs)
    # n = 1 and n = 2: a Krylov method is exact after n steps
    for n in (1, 2):
        op = kr.banded(n, seed=n, spd=spd)
        rp, ci, v = op.csr()
        A = ctx.csr(n, n, rp, ci, v)
        b = np.array([1.5, -0.75][:n])
        want = np.linalg.solve(sps.csr_matrix((v, ci, rp), shape=(n, n)).toarray(), b)
        x = ctx.vec(n)
        st, it, resid = solve(A, x, ctx.vec(b), 10, 1e-13)
        d = kr.rel(x.numpy(), want)
        print(f"{solver} n={n}: status {st}, {it} iterations, resid {resid:.2e}, x vs numpy.linalg.solve {d:.2e}")
        assert st == 0 and 1 <= it <= n and d <= 8 * np.finfo(np.float64).eps
