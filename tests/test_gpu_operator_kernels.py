"""The standalone operator kernels (mgs_spmv, mgs_residual, mgs_jacobi: every arm of mgs_launch_csr_op_range) against the exact host
restatement of tests/spmv_ref.py, arm by arm.

Every case uploads its matrix with ctx.csr and asserts
  * that Csr.plan_info() equals the restated plan, and that the restated arm of the row blocks of interest is the arm the case was built
    for (staged, sequential, lanes(L), pipe, wave; the serving kernel where a variant falls back);
  * all three ops (Jacobi where rows ≤ cols) into guarded, sentinel-filled outputs: guards intact, every row written;
  * EQUAL BITS with the restatement of that arm's summation order — no tolerance anywhere;
  * the derived per-row bar of spmv_ref's module docstring against the exact (long double) value.
Each case prints its largest error/bar ratio; options are restored in `finally`.

Largest error/bar ratios measured on an MI355X when the tests were written (a row passes at ≤ 1; reported, not asserted beyond that):
row counts 1 … 513 0.30–0.62, 600 × 700 0.63, no entries 0.60, gather widths 4 / 7 / 8 0.65 / 0.62 / 0.65 (the same coded; the twin with a row of 15
0.67), poisoned x 0.65, signed zeros 0.67, budget step 0.55 (sequential arm, coded too) and 0.51 (lanes(4)), block over 5120 entries
0.31 (sequential) and 0.29 (lanes(16)), LANES 4 / 8 … 64 0.46 / 0.41, variant 1 on short rows 0.49, variants 2–4 0.56–0.68 staged and
0.29–0.31 over budget, wave 0.58–0.62 (fallback 0.47), pipe 0.46–0.62 (2047 and 2048 entries 0.23–0.26, 68 blocks 0.58, fallback
0.56), option forms 0.51–0.65.  The largest ratios come from short rows, where the bar is a few u wide."""
import numpy as np
import pytest

import spmv_ref as R
from spmv_ref import RB, SENT, Guarded

pytestmark = pytest.mark.gpu

# the defaults of mgs_internal.hpp (struct mgs_ctx) of every option a test here sets
DEFAULTS = (("spmv_variant", 0), ("rowcode", 1), ("nontemporal", 0), ("xcd_remap", 1), ("blkptr", 1), ("nt_store", 1000000))


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
    return ctx.csr(M.shape[0], M.shape[1], M.indptr, M.indices, M.data)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def launch(A, op, x, b, dinv, omega, out):
    if op == "spmv":
        A.spmv(x, out)
    elif op == "residual":
        A.residual(x, b, out)
    else:
        A.jacobi(dinv, omega, b, x, out)


def check(ctx, mg, M, what, variant=0, arms=None, kernel=None, A=None, coded=False, vecs=None, poisoned=False):
    """the three ops of matrix M under `variant` against the restatement; arms: {row block: arm the case was built for}; kernel: the
    kernel that must serve the launch; A: the uploaded matrix (coded runs reuse it).  Returns A, {op: output}, largest error/bar ratio."""
    A = A or upload(ctx, M)
    n = M.shape[0]
    rp, col, val = M.indptr, M.indices, M.data
    p = R.plan_of(M)
    assert A.plan_info() == R.plan_info(p), (what, A.plan_info(), R.plan_info(p))
    for blk, want in (arms or {}).items():
        assert R.arm(p, blk, variant, coded) == want, (what, blk, R.arm(p, blk, variant, coded), want)
    if kernel:
        assert R.kernel(p, variant, coded) == kernel, (what, R.kernel(p, variant, coded), kernel)
    xh, bh, dh, omega = vecs or R.vectors(M, 5)
    s = R.row_sums(p, variant, rp, col, val, xh, coded)
    x, b, dinv = ctx.vec(xh), ctx.vec(bh), ctx.vec(dh)
    out, worst = {}, 0.0
    ctx.set_option("spmv_variant", variant)
    try:
        for op in R.OPS if M.shape[0] <= M.shape[1] else R.OPS[:2]:
            y = Guarded(ctx, mg, n)
            if n:
                launch(A, op, x, b, dinv, omega, y.v)
            got = y.check(f"{what}/{op}: guard zones")
            assert not np.any(got == SENT), (what, op, "unwritten rows", np.flatnonzero(got == SENT)[:8])
            want = R.apply(op, s, xh, bh, dh, omega)
            ok = np.ones(n, dtype=bool)
            if poisoned:
                assert np.array_equal(np.isnan(got), np.isnan(want)), (what, op, "NaN masks", np.flatnonzero(np.isnan(got) != np.isnan(want))[:8])
                ok = ~np.isnan(want)
                assert (~ok).any() and np.isinf(want).any()
            bad = np.flatnonzero(bits(got)[ok] != bits(want)[ok])
            assert bad.size == 0, (what, op, "bits", np.flatnonzero(ok)[bad][:8], got[ok][bad][:4], want[ok][bad][:4])
            ex, _ = R.exact(op, rp, col, val, xh, bh, dh, omega)
            fin = ok & np.isfinite(want)
            q = R.ratios(got[fin], ex[fin], R.bar(op, rp, col, val, xh, bh, dh, omega)[fin])
            worst = max(worst, float(q.max(initial=0.0)))
            assert q.max(initial=0.0) <= 1.0, (what, op, float(q.max()), int(q.argmax()))
            out[op] = got
    finally:
        ctx.set_option("spmv_variant", 0)
    print(f"{what}: variant={variant} kernel={R.kernel(p, variant, coded)} arms={sorted({R.arm(p, k, variant, coded) for k in range(p['nblocks'])})} "
          f"lds_cap={p['lds_cap']} U={R.gather_width_of(p)} largest error/bar {worst:.3f}")
    return A, out, worst


def check_coded(ctx, mg, M, A, before, what, arms=None):
    """the same matrix with its pattern code (mgs_csr_optimize; the code is sticky, so this comes after the uncoded runs): the same bits"""
    A.optimize()
    nc = R.coded_blocks(M.indptr, M.indices, M.shape[0])
    info = A.rowcode_info()
    assert info["coded_blocks"] == nc and info["blocks"] == R.row_blocks(M.shape[0]), (what, info, nc)
    usable = R.code_usable(R.plan_of(M), nc)
    _, after, _ = check(ctx, mg, M, f"{what} coded_blocks={nc} usable={int(usable)}", 0, arms, "coded" if usable else "slice", A=A, coded=usable)
    for op in after:
        assert np.array_equal(bits(after[op]), bits(before[op])), (what, op)
    return usable


# ---- 1. row counts around the wave, the row block and two row blocks; no rows; no entries ----
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 511, 513])
def test_row_count_edges(ctx, mg, n):
    """default path, no code: every block staged by the slice kernel"""
    try:
        check(ctx, mg, R.edge_case(n), f"rows n={n}", 0, {k: "staged" for k in range(R.row_blocks(n))}, "slice")
    finally:
        restore(ctx)


def test_wide_matrix_with_halo_columns(ctx, mg):
    """600 × 700 (rows ≤ cols: Jacobi runs): the plan's halo figures — no leading halo block, two trailing ones — and the same kernels"""
    try:
        M = R.wide_case()
        p = R.plan_of(M)
        assert (p["halo_lo_blocks"], p["halo_hi_blocks"], p["halo_split_ok"]) == (0, 2, 1)
        A, out, _ = check(ctx, mg, M, "600 x 700", 0, {0: "staged", 1: "staged", 2: "staged"}, "slice")
        for v in (1, 3, 6, 7):
            _, o, _ = check(ctx, mg, M, f"600 x 700 variant={v}", v, A=A)
            assert all(np.array_equal(bits(out[op]), bits(o[op])) for op in out)
    finally:
        restore(ctx)


def test_no_rows_and_no_entries(ctx, mg):
    """a 0-row matrix launches nothing; a matrix without entries returns +0.0, b and x + (ω·dinv)·b"""
    try:
        import scipy.sparse as sps
        check(ctx, mg, sps.csr_matrix((0, 5)), "no rows")
        M = R.empty_rows_case()
        x, b, dinv, omega = R.vectors(M, 5)
        _, out, _ = check(ctx, mg, M, "no entries", 0, {0: "staged", 1: "staged"}, "slice")
        assert np.all(out["spmv"] == 0) and not np.signbit(out["spmv"]).any()
        assert np.array_equal(bits(out["residual"]), bits(b)) and np.array_equal(bits(out["jacobi"]), bits(x + (omega * dinv) * b))
        for v in (1, 2, 3, 4, 6, 7):
            check(ctx, mg, M, f"no entries variant={v}", v)
    finally:
        restore(ctx)


# ---- 2. gather widths 4, 7, 8; the pattern code on the same matrices ----
@pytest.mark.parametrize("u", [4, 7, 8])
def test_gather_widths(ctx, mg, u):
    """lengths 0, 1, U − 1, U, U + 1, 2U(, 2U + 1); the second row block starts at an odd entry index; the matrix's last row ends inside a
    gather step, so the clamped reads past `lim` fall on the last staged entry.  Variant 5 is the same kernel.  Then the pattern code."""
    try:
        M = R.gather_case(u)
        p = R.plan_of(M)
        assert R.gather_width_of(p) == u and M.indptr[RB] % 2 == 1 and (M.indptr[-1] - M.indptr[-2]) % u
        A, out, _ = check(ctx, mg, M, f"gather U={u}", 0, {0: "staged", 1: "staged", 2: "staged"}, "slice")
        _, out5, _ = check(ctx, mg, M, f"gather U={u} variant 5", 5, {0: "staged", 1: "staged", 2: "staged"}, "slice", A=A)
        assert all(np.array_equal(bits(out[op]), bits(out5[op])) for op in out)
        if u == 7:      # one row of 15 entries flips the width to 8
            T = R.gather_case(7, True)
            pt = R.plan_of(T)
            assert pt["max_row_len"] == 15 and R.gather_width_of(pt) == 8 and p["max_row_len"] == 14
            check(ctx, mg, T, "gather U=7 twin with a row of 15 (U=8)", 0, {0: "staged", 2: "staged"}, "slice")
        check_coded(ctx, mg, M, A, out, f"gather U={u}", {0: "staged", 2: "staged"})
    finally:
        restore(ctx)


def test_poisoned_neighbours(ctx, mg):
    """x = NaN at one column and +Inf at another, each referenced by one row: the padded gather steps of the rows above do read them (the
    CPU test shows which) and must discard them by the select, not by a product with zero"""
    try:
        M = R.gather_case(8)
        n = M.shape[0]
        x, b, dinv, omega = R.vectors(M, 5)
        x[n - 2] = np.nan; x[n - 1] = np.inf
        A, out, _ = check(ctx, mg, M, "poisoned x", 0, {0: "staged", 1: "staged"}, "slice", vecs=(x, b, dinv, omega), poisoned=True)
        assert np.flatnonzero(np.isnan(out["spmv"])).tolist() == [R.LONELY_ROWS[0]] and np.flatnonzero(np.isinf(out["spmv"])).tolist() == [R.LONELY_ROWS[1]]
        for v in (3, 6, 7):
            check(ctx, mg, M, f"poisoned x variant={v}", v, A=A, vecs=(x, b, dinv, omega), poisoned=True)
        A.optimize()
        usable = R.code_usable(R.plan_of(M), R.coded_blocks(M.indptr, M.indices, n))
        check(ctx, mg, M, "poisoned x, coded", 0, kernel="coded" if usable else "slice", A=A, coded=usable, vecs=(x, b, dinv, omega), poisoned=True)
    finally:
        restore(ctx)


def test_signed_zeros(ctx, mg):
    """−0.0 among values and x, rows whose every product is −0.0: a sum that starts at +0.0 is +0.0, padded or not"""
    try:
        M, vecs, negrows = R.signed_zero_case()
        A, out, _ = check(ctx, mg, M, "signed zeros", 0, {0: "staged"}, "slice", vecs=vecs)
        assert np.all(out["spmv"][negrows] == 0) and not np.signbit(out["spmv"][negrows]).any()
        for v in (1, 2, 4, 6, 7):
            _, o, _ = check(ctx, mg, M, f"signed zeros variant={v}", v, A=A, vecs=vecs)
            assert not np.signbit(o["spmv"][negrows]).any()
    finally:
        restore(ctx)


# ---- 3. the budget step: one heavy row block among 68 ----
def test_budget_step_sequential_arm(ctx, mg):
    """lds_cap lowered to 969; the heavy block walks its rows of 40 from global memory in the same order; XCD map live (≥ 64 blocks) and
    off: every row written exactly once.  Then the pattern code: the coded kernel's walk of the heavy block."""
    try:
        M = R.budget_case(40)
        p = R.plan_of(M)
        assert p["lds_cap"] == 969 < 5120 and p["has_long_row_blocks"] == 1 and p["max_row_len"] == 40
        arms = {0: "staged", R.BUDGET_HEAVY - 1: "staged", R.BUDGET_HEAVY: "sequential", R.BUDGET_HEAVY + 1: "staged", 67: "staged"}
        A, out, _ = check(ctx, mg, M, "budget step xcd_remap=1", 0, arms, "slice")
        ctx.set_option("xcd_remap", 0)
        _, out0, _ = check(ctx, mg, M, "budget step xcd_remap=0", 0, arms, "slice", A=A)
        assert all(np.array_equal(bits(out[op]), bits(out0[op])) for op in out)
        ctx.set_option("xcd_remap", 1)
        assert check_coded(ctx, mg, M, A, out, "budget step", arms)
        ctx.set_option("xcd_remap", 0)
        check(ctx, mg, M, "budget step coded xcd_remap=0", 0, arms, "coded", A=A, coded=True)
    finally:
        restore(ctx)


def test_budget_step_lanes_arm(ctx, mg):
    """one row of 200 inside the heavy block: the block takes lanes(4), its rows hold the lane-strided sums and the tree's order; every
    other block the sequential order"""
    try:
        M = R.budget_case(40, 200)
        p = R.plan_of(M)
        assert p["max_row_len"] == 200 and p["has_long_row_blocks"] == 1 and R.lanes_of(p) == 4
        arms = {0: "staged", R.BUDGET_HEAVY: "lanes(4)", R.BUDGET_HEAVY + 1: "staged"}
        x = R.vectors(M, 5)[0]
        rows = slice(R.BUDGET_HEAVY * RB, (R.BUDGET_HEAVY + 1) * RB)
        sl = R.row_sums_lanes(M.indptr, M.indices, M.data, x, 4)[rows]
        ss = R.row_sums_sequential(M.indptr, M.indices, M.data, x)[rows]
        assert (bits(sl) != bits(ss)).sum() > 25                       # the two orders differ on this block: the case can tell them apart
        for remap in (1, 0):
            ctx.set_option("xcd_remap", remap)
            _, out, _ = check(ctx, mg, M, f"budget step, row of 200, xcd_remap={remap}", 0, arms, "slice")
            assert np.array_equal(bits(out["spmv"][rows]), bits(sl))
    finally:
        restore(ctx)


@pytest.mark.parametrize("long_row", [0, 70])
def test_block_over_the_staging_cap(ctx, mg, long_row):
    """a block of 5376 entries (> 5120): sequential without a row longer than 64, lanes(16) with one"""
    try:
        M = R.over_cap_case(long_row)
        check(ctx, mg, M, f"block over 5120, longest row {max(21, long_row)}", 0, {0: "staged", 1: "lanes(16)" if long_row else "sequential"}, "slice")
    finally:
        restore(ctx)


# ---- 4. every LANES instantiation (variant 1: nothing staged) ----
@pytest.mark.parametrize("L", [4, 8, 16, 32, 64])
def test_every_lanes_width(ctx, mg, L):
    """mean row length 3, 6, 12, 24, 40 → L = 4 … 64; rows of 0, 1, L − 1, L, L + 1, 3L + 2 and 70 entries; a partial last block, so the
    sub-groups of one wave leave the row loop at different times"""
    try:
        M = R.lanes_case(L)
        p = R.plan_of(M)
        assert R.lanes_of(p) == L and p["max_row_len"] >= 65 and p["nblocks"] == 3
        check(ctx, mg, M, f"lanes L={L}", 1, {k: f"lanes({L})" for k in range(3)}, "slice")
    finally:
        restore(ctx)


def test_variant1_short_rows_take_the_sequential_walk(ctx, mg):
    """no row longer than 64: variant 1 (cap = −1, nothing staged) walks every row sequentially, not with sub-wavefronts"""
    try:
        M = R.lanes_case(4, False)
        assert R.plan_of(M)["max_row_len"] <= 64
        _, o1, _ = check(ctx, mg, M, "variant 1, short rows", 1, {k: "sequential" for k in range(3)}, "slice")
        _, o0, _ = check(ctx, mg, M, "variant 0, short rows", 0, {k: "staged" for k in range(3)}, "slice")
        assert all(np.array_equal(bits(o0[op]), bits(o1[op])) for op in o0)
    finally:
        restore(ctx)


# ---- 5. variants 2, 3, 4: products in LDS, 1 / 2 / 4 entries per lane and step ----
@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("variant", [2, 3, 4])
def test_products_in_lds_staged(ctx, mg, variant, r):
    """row blocks starting at entry indices ≡ 0, 1, 2, 3 (mod 4), the matrix ending at ≡ r: the widened 16-byte loads at both ends of a
    slice and the four-entry pad of the allocation"""
    try:
        M = R.chunk_case(r)
        assert [int(M.indptr[k * RB]) % 4 for k in range(4)] == [0, 1, 2, 3] and M.nnz % 4 == r
        check(ctx, mg, M, f"products in LDS variant={variant} end≡{r}", variant, {k: "staged" for k in range(5)}, "rowblock")
    finally:
        restore(ctx)


@pytest.mark.parametrize("long_row", [0, 70])
@pytest.mark.parametrize("variant", [2, 3, 4])
def test_products_in_lds_over_budget(ctx, mg, variant, long_row):
    """these variants have no sequential walk: the over-budget block takes lanes(16) whether or not a row exceeds 64"""
    try:
        M = R.over_cap_case(long_row)
        check(ctx, mg, M, f"products in LDS variant={variant}, block over 5120, longest row {max(21, long_row)}", variant,
              {0: "staged", 1: "lanes(16)"}, "rowblock")
    finally:
        restore(ctx)


# ---- 6. variant 7: one wave per 64 rows ----
@pytest.mark.parametrize("n", [70, 256, 700])
def test_wave_variant(ctx, mg, n):
    """a 64-row group without entries (rows 128–191), groups that begin behind the last row"""
    try:
        M = R.wave_case(n)
        assert n < 192 or M.indptr[192] == M.indptr[128]
        check(ctx, mg, M, f"wave n={n}", 7, {0: "wave"}, "wave")
    finally:
        restore(ctx)


def test_wave_variant_68_blocks_and_fallback(ctx, mg):
    """XCD map live and off on 68 row blocks; a 64-row group of 4160 entries (> 4096) falls back to the slice kernel"""
    try:
        M = R.budget_case(0)
        A = None
        for remap in (1, 0):
            ctx.set_option("xcd_remap", remap)
            A, _, _ = check(ctx, mg, M, f"wave 68 blocks xcd_remap={remap}", 7, {0: "wave", 67: "wave"}, "wave", A=A)
        ctx.set_option("xcd_remap", 1)
        T = R.wave_over_case()
        assert R.plan_of(T)["max_wave_nnz"] == 4160
        check(ctx, mg, T, "wave falls back", 7, {0: "staged"}, "slice")
    finally:
        restore(ctx)


# ---- 7. variant 6: four row blocks per workgroup, software-pipelined ----
@pytest.mark.parametrize("n", [200, 1024, 1100, 1900])
def test_pipe_variant(ctx, mg, n):
    """1, 4, 5 and 8 row blocks: super blocks of one partial block, of four, of four plus one partial, of two times four"""
    try:
        check(ctx, mg, R.pipe_case(n), f"pipe n={n}", 6, {0: "pipe"}, "pipe")
    finally:
        restore(ctx)


@pytest.mark.parametrize("lo_odd", [0, 1])
@pytest.mark.parametrize("cnt", [2047, 2048])
def test_pipe_boundary(ctx, mg, cnt, lo_odd):
    """a row block of exactly 2047 entries stages in 1024 pairs at either parity of its first entry index: pipe.  One of 2048 needs 1025
    pairs at an odd index — one more than the kernel holds — so the guard admits 2047 at the most and 2048 runs the slice kernel,
    at either parity, with the same sequential bits"""
    try:
        M = R.pipe_boundary_case(cnt, lo_odd)
        lo, hi = int(M.indptr[RB]), int(M.indptr[2 * RB])
        assert hi - lo == cnt and lo % 2 == lo_odd and R.pairs_needed(lo, hi) == (1025 if (cnt, lo_odd) == (2048, 1) else 1024)
        if cnt == 2047:
            check(ctx, mg, M, f"pipe boundary {cnt} lo_odd={lo_odd}", 6, {0: "pipe", 1: "pipe"}, "pipe")
        else:
            check(ctx, mg, M, f"pipe boundary {cnt} lo_odd={lo_odd}", 6, {0: "staged", 1: "staged"}, "slice")
    finally:
        restore(ctx)


def test_pipe_variant_68_blocks_and_fallback(ctx, mg):
    """68 row blocks in 17 super blocks; a lowered budget (max_block_nnz != lds_cap) falls back to the slice kernel"""
    try:
        A = None
        for remap in (1, 0):
            ctx.set_option("xcd_remap", remap)
            A, _, _ = check(ctx, mg, R.budget_case(0), f"pipe 68 blocks xcd_remap={remap}", 6, {0: "pipe", 67: "pipe"}, "pipe", A=A)
        ctx.set_option("xcd_remap", 1)
        T = R.budget_case(7)
        p = R.plan_of(T)
        assert p["max_block_nnz"] == 1792 <= 2047 and p["lds_cap"] < 1792
        check(ctx, mg, T, "pipe falls back: budget lowered", 6, {0: "staged", R.BUDGET_HEAVY: "sequential"}, "slice")
    finally:
        restore(ctx)


# ---- 8. the option forms of the default path: same bits ----
def test_option_forms_same_bits(ctx, mg):
    """block bounds from rowptr instead of blkptr, non-temporal loads, streaming stores from one row up: the same bits"""
    try:
        for M, what in ((R.gather_case(8), "gather U=8"), (R.budget_case(40, 200), "budget step, row of 200")):
            A, ref, _ = check(ctx, mg, M, what, 0, kernel="slice")
            for key, value in (("blkptr", 0), ("nontemporal", 1), ("nt_store", 1)):
                ctx.set_option(key, value)
                _, out, _ = check(ctx, mg, M, f"{what} {key}={value}", 0, kernel="slice", A=A)
                assert all(np.array_equal(bits(ref[op]), bits(out[op])) for op in ref), (what, key)
                restore(ctx)
    finally:
        restore(ctx)


# ---- 9. refusals: MgsError, nothing launched ----
def test_refusals(ctx, mg):
    """y aliasing x; a short x, b, y or dinv; Jacobi on a matrix with more rows than columns: every one an MgsError that leaves the
    output as it was"""
    import scipy.sparse as sps
    n = 65
    M = R.edge_case(n)
    A = upload(ctx, M)
    xh, bh, dh, omega = R.vectors(M, 5)
    x, b, dinv = ctx.vec(xh), ctx.vec(bh), ctx.vec(dh)
    short = ctx.vec(xh[:n - 1])
    y = Guarded(ctx, mg, n)
    ys = Guarded(ctx, mg, n - 1)
    calls = [lambda: A.spmv(x, x), lambda: A.residual(x, b, x), lambda: A.jacobi(dinv, omega, b, x, x),                      # aliasing
             lambda: A.spmv(short, y.v), lambda: A.residual(short, b, y.v), lambda: A.jacobi(dinv, omega, b, short, y.v),      # short x
             lambda: A.residual(x, short, y.v), lambda: A.jacobi(dinv, omega, short, x, y.v),                                # short b
             lambda: A.jacobi(short, omega, b, x, y.v),                                                                     # short dinv
             lambda: A.spmv(x, ys.v), lambda: A.residual(x, b, ys.v), lambda: A.jacobi(dinv, omega, b, x, ys.v)]             # short y
    TM = sps.vstack([M, M[:3]], format="csr"); TM.sort_indices()                                                             # 68 × 65
    T = upload(ctx, TM)
    yt = Guarded(ctx, mg, n + 3)
    bt, dt = ctx.vec(np.r_[bh, bh[:3]]), ctx.vec(np.r_[dh, dh[:3]])
    calls.append(lambda: T.jacobi(dt, omega, bt, x, yt.v))
    for k, call in enumerate(calls):
        with pytest.raises(mg.MgsError):
            call()
        assert np.all(y.check(f"refusal {k}") == SENT) and np.all(ys.check(f"refusal {k}") == SENT) and np.all(yt.check(f"refusal {k}") == SENT), k
    assert np.array_equal(x.numpy(), xh)                 # the aliased calls wrote nothing either
    T.spmv(x, yt.v)                                      # the tall matrix itself is fine for the other ops
    assert np.array_equal(bits(yt.check("tall spmv")), bits(R.row_sums_sequential(TM.indptr, TM.indices, TM.data, xh)))
