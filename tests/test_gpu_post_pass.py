"""The cycle's fused post pass alone (mgs_hier_post_pass) against the exact host restatement of tests/post_pass_ref.py, arm by arm.

Every case builds its operator in numpy (values and vectors from ±[0.5, 2]), pushes an explicit aggregation P (plus a second transfer onto
eight aggregates, so the dense coarsest solve costs nothing), runs both forms into a sentinel-filled guarded vector and asserts
  * from `info` that the arm the case was built for ran (operand, kernel, gather width U, single-step flag, blocks over the staging budget);
  * the derived per-row bar of the module docstring of post_pass_ref against the long-double restatement;
  * equal bits with the FP64 restatement wherever the documented order is a promise: the same operand, no operand row longer than 64.
Each case prints its largest error/bar ratio.  The cases on device-built hierarchies (grouped levels) use the project's own operators.

Largest error/bar ratios measured on an MI355X when the tests were written (a row passes at ≤ 1): row counts × U = 4 / 7 / 8 0.13–0.29,
rows outside every aggregate 0.25–0.28, shuffled aggregates 0.17–0.22, mixed 0.27–0.30, staging budget 0.36, long rows 0.33, gather form on A
0.19, FP32 values 0.15–0.24, grouped levels 0.30 (poisson3d(33)) and 0.42 (CSky3d30), row-block ranges 0.32."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import post_pass_ref as R
from post_pass_ref import Guarded, INT_MAX, SENT

pytestmark = pytest.mark.gpu

# the defaults of mgs_internal.hpp (struct mgs_ctx) of every option a test here sets
DEFAULTS = (("rowcode", 1), ("merge_ap", 1), ("diag_from_values", 1), ("fuse_operands", 1), ("group_sweep", 0), ("xcd_remap", 1),
            ("fuse_restrict", 1), ("group_stray_pct", 6), ("group_min_blocks", 1024), ("group_blocks", 4), ("valcode", 0))


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


def build(ctx, mg, c):
    """hierarchy of the case: its operator, its aggregates, then everything onto eight aggregates"""
    h = mg.Hierarchy(upload(ctx, c.A), c.omega, 1, 1)
    h.push_P(upload(ctx, R.agg_P(c.agg, c.nc)))
    g1 = (np.arange(c.nc) * 8 // c.nc).astype(np.int32)
    h.push_P(upload(ctx, R.agg_P(g1, 8)))
    return h.finalize()


def expected_u(op):
    """the gather width the launchers document for an operand (mgs.h / launch_coded in kernels_spmv.hip, post_gather_width in rowblock.hpp)"""
    mean, mx = op.mean_len, op.max_len
    if 4.5 < mean <= 5.5 and mx <= 10:
        return 5
    return 4 if mean <= 4.5 else (7 if mean <= 7.5 and mx <= 14 else 8)


def run(ctx, mg, h, c, kind, want, what, level=0, bits=None):
    """both forms of the level's post pass against the restatement on operand `kind`; want: info entries the case was built for.
    Returns {form: x} and the largest error/bar ratio."""
    op = c.operand(kind)
    promise = op.max_len <= 64 if bits is None else bits
    out, worst = {}, 0.0
    ec = ctx.vec(c.ec)
    for form, bvec, xin in c.forms():
        x = Guarded(ctx, mg, c.n)
        info = h.post_pass(level, ctx.vec(bvec), ctx.vec(xin) if xin is not None else None, ec, x.v)
        xd = x.check(f"{what}/{form}: guard zones")
        assert not np.any(xd == SENT), (what, form, "unwritten rows", np.flatnonzero(xd == SENT)[:8])
        for k, v in want.items():
            assert (info[k] >= 1 if v == ">=1" else info[k] == v), f"{what}/{form}: {k} should be {v}: {info}"
        if info["kernel"] in (1, 2, 3):
            assert info["U"] == expected_u(op) and (info["flags"] & 1) == int(op.max_len <= info["U"]), f"{what}: {info}, operand rows: mean {op.mean_len:.2f}, longest {op.max_len}"
        xb = R.evaluate(op, c.d, c.agg, c.ec, bvec, xin, np.longdouble)
        q = R.ratios(xd, xb, R.bar(op, c.d, c.agg, c.ec, bvec, xin))
        worst = max(worst, float(q.max()))
        assert q.max() <= 1.0, (what, form, float(q.max()), int(q.argmax()), info)
        if promise:
            xa = R.evaluate(op, c.d, c.agg, c.ec, bvec, xin, np.float64)
            assert np.array_equal(xd, xa), (what, form, "bits", np.flatnonzero(xd != xa)[:8], info)
        out[form] = xd
    print(f"{what}: operand={info['operand']} kernel={info['kernel']} U={info['U']} flags={info['flags']} capv={info['capv']} capi={info['capi']} "
          f"over={info['blocks_over_budget']} largest error/bar {worst:.3f}")
    return out, worst


# ---- 1. row counts around the block size; U = 4, 7 (single step), 8 (loop); pattern code on and off ----
def stencil_band7(n):
    """couplings at distance 2, 4 and 32: with pairs as aggregates every entry of a row falls into an aggregate of its own, seven per row"""
    i = np.arange(n)
    r, c = [], []
    for o in (2, 4, 32):
        r += [i[:-o], i[o:]]; c += [i[o:], i[:-o]]
    return sps.csr_matrix((np.ones(sum(map(len, r))), (np.concatenate(r), np.concatenate(c))), shape=(n, n))


def stencil_9pt(n, w=16):
    i = np.arange(n); x = i % w
    r, c = [], []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == dy == 0:
                continue
            j = i + dx + w * dy
            ok = (x + dx >= 0) & (x + dx < w) & (j >= 0) & (j < n)
            r.append(i[ok]); c.append(j[ok])
    return sps.csr_matrix((np.ones(sum(map(len, r))), (np.concatenate(r), np.concatenate(c))), shape=(n, n))


STENCILS = {"line": (R.stencil_1d2d, 4, 1), "five_point": (R.stencil_5pt, 4, 1), "band7": (stencil_band7, 7, 1), "27_point": (R.stencil_27pt, 8, 0)}


@pytest.mark.parametrize("rowcode", [1, 0])
@pytest.mark.parametrize("n", [255, 256, 257, 513])
@pytest.mark.parametrize("stencil", list(STENCILS))
def test_row_counts_and_gather_widths(ctx, mg, stencil, n, rowcode):
    """a full last block, a one-row last block, partial last blocks; pairs as aggregates; merged A·P.  The line's and the 2-D five-point
    operator's A·P have at most four entries per row (U = 4; a five-point operator cannot reach the U = 7 instance: its A·P has at most
    five entries per row); the band operator's has seven: U = 7 in one step; the 27-point one's eighteen: U = 8 with the loop.  Without
    the pattern code the gather kernel serves the operand."""
    fn, u, single = STENCILS[stencil]
    rng = np.random.default_rng(n)
    c = R.Case(R.randomize(fn(n), rng), R.pairs(n), seed=n + 1)
    try:
        h = build(ctx, mg, c)
        ctx.set_option("rowcode", rowcode)
        want = {"operand": 2, "kernel": 1, "U": u} if rowcode else {"operand": 2, "kernel": 0}
        _, _ = run(ctx, mg, h, c, "merged", want, f"{stencil} n={n} rowcode={rowcode}")
        if rowcode:
            info = h.post_pass(0, ctx.vec(c.t), None, ctx.vec(c.ec), ctx.vec(c.n))
            assert (info["flags"] & 1) == single, info
    finally:
        restore(ctx)


# ---- 2. rows and columns outside every aggregate ----
def test_rows_outside_every_aggregate(ctx, mg):
    """agg = −1 at the first / last row of a row block and in a block's middle, a run of 300 such rows whose columns are unaggregated too
    (empty operand rows, one empty row block), neighbours with some unaggregated columns (dropped in A·P, CODE_NEG / negative col_agg in
    the mapped form).  merge_ap 1 and 0; with 0, ω/a_ii from the streamed diagonal or from wd: the same bits."""
    rng = np.random.default_rng(21)
    c = R.Case(*R.unaggregated_case(1100, rng), seed=22)
    assert c.merged.block_nnz()[3] == 0 and (c.mapped.col < 0).sum() > 300 and (c.agg[[0, 255, 256, 700]] == -1).all()
    try:
        h = build(ctx, mg, c)
        run(ctx, mg, h, c, "merged", {"operand": 2, "kernel": 1}, "unaggregated merge_ap=1")
        ctx.set_option("merge_ap", 0)
        x1, _ = run(ctx, mg, h, c, "mapped", {"operand": 1, "kernel": 1}, "unaggregated merge_ap=0 diag_from_values=1")
        ctx.set_option("diag_from_values", 0)
        x0, _ = run(ctx, mg, h, c, "mapped", {"operand": 1, "kernel": 1}, "unaggregated merge_ap=0 diag_from_values=0")
        assert np.array_equal(x1["t"], x0["t"]) and np.array_equal(x1["rb"], x0["rb"])
        ctx.set_option("rowcode", 0)
        run(ctx, mg, h, c, "mapped", {"operand": 1, "kernel": 0}, "unaggregated merge_ap=0, gather kernel")
    finally:
        restore(ctx)


# ---- 3. aggregates of 1, 2, 3, 8 and 16 members, shuffled, on random graphs ----
@pytest.mark.parametrize("symmetric", [True, False])
def test_shuffled_aggregates_on_random_graphs(ctx, mg, symmetric):
    rng = np.random.default_rng(31 + symmetric)
    n = 3700 if symmetric else 2300
    c = R.Case(R.randomize(R.random_graph(n, 4, rng, symmetric), rng), R.random_aggregates(n, rng), seed=33)
    sizes = np.bincount(c.agg[c.agg >= 0])
    assert {1, 2, 3, 8, 16} <= set(sizes.tolist()) and (c.agg < 0).any()
    try:
        h = build(ctx, mg, c)
        run(ctx, mg, h, c, "merged", {"operand": 2, "kernel": 0}, f"random graph symmetric={symmetric} merge_ap=1")       # rows share no shape: no pattern code
        ctx.set_option("merge_ap", 0)
        run(ctx, mg, h, c, "mapped", {"operand": 1, "kernel": 0}, f"random graph symmetric={symmetric} merge_ap=0")
    finally:
        restore(ctx)


# ---- 4. coded and uncoded row blocks side by side ----
def test_mixed_operator(ctx, mg):
    """a regular five-point part and an irregular part (the `mixed` shape of test_pattern_coded_rows_bit_identical at about 20 000 rows)"""
    rng = np.random.default_rng(41)
    n0, n1 = 17000, 3000; n = n0 + n1
    reg = R.stencil_5pt(n0, 128)
    irr = sps.random(n1, n, density=0.0004, random_state=rng, format="csr")
    pat = sps.vstack([sps.hstack([reg, sps.csr_matrix((n0, n1))]), irr], format="csr")
    c = R.Case(R.randomize(pat, rng), R.pairs(n), seed=42)
    try:
        h = build(ctx, mg, c)
        run(ctx, mg, h, c, "merged", {"operand": 2, "kernel": 1}, "mixed merge_ap=1")
        fi = h.fused_info(0)
        assert 0 < fi["coded_col_agg"] < fi["blocks"], fi
        ctx.set_option("merge_ap", 0)
        run(ctx, mg, h, c, "mapped", {"operand": 1, "kernel": 1}, "mixed merge_ap=0")
    finally:
        restore(ctx)


# ---- 5. row blocks over the staging budget ----
def test_blocks_over_the_staging_budget(ctx, mg):
    """140 row blocks of which two hold eleven times the mean: mgs_plan_csr stages 98.5 % of the blocks and budgets below these two, which
    walk their rows from global memory"""
    rng = np.random.default_rng(51)
    n = 140 * 256
    pat = R.stencil_5pt(n, 128).tolil()
    for blk in (40, 100):
        for i in range(blk * 256, blk * 256 + 256):
            pat[i, rng.choice(n, 44, replace=False)] = 1.0
    c = R.Case(R.randomize(pat.tocsr(), rng), R.pairs(n), seed=52)
    assert c.merged.max_len <= 64
    try:
        h = build(ctx, mg, c)
        run(ctx, mg, h, c, "merged", {"operand": 2, "kernel": 1, "blocks_over_budget": ">=1"}, "staging budget")
        info = h.post_pass(0, ctx.vec(c.t), None, ctx.vec(c.ec), ctx.vec(c.n))
        assert info["blocks_over_budget"] == int((c.merged.block_nnz() > info["capv"]).sum()) == 2, info
    finally:
        restore(ctx)


# ---- 6. operand rows longer than 64 ----
def test_operand_rows_longer_than_64(ctx, mg):
    """the construction of test_galerkin_and_merged_operand_with_long_rows: a band, five dense rows and columns, aggregates of three — the
    gather kernel on A·P; the per-row bar only (no order is promised for such rows)"""
    rng = np.random.default_rng(61)
    n = 4000
    B = sps.diags([1.0, 1.0, 1.0, 1.0], [1, -1, 7, -7], shape=(n, n)).tolil()
    for q in (3, 1000, 1001, 2500, 3998):
        js = rng.choice(n, 500, replace=False); js = js[js != q]
        B[q, js] = 1.0; B[js, q] = 1.0
    c = R.Case(R.randomize(B.tocsr(), rng), (np.arange(n) // 3).astype(np.int32), seed=62)
    assert c.merged.max_len > 64
    try:
        h = build(ctx, mg, c)
        run(ctx, mg, h, c, "merged", {"operand": 2, "kernel": 0}, "long rows", bits=False)
    finally:
        restore(ctx)


# ---- 7. no setup-time operands ----
def test_gather_form_on_A(ctx, mg):
    """fuse_operands = 0: the gather kernel on A with the column-to-aggregate map (FUSE_POST)"""
    rng = np.random.default_rng(71)
    c = R.Case(*R.unaggregated_case(1100, rng), seed=72)
    try:
        ctx.set_option("fuse_operands", 0)
        h = build(ctx, mg, c)
        run(ctx, mg, h, c, "gather", {"operand": 0, "kernel": 0, "U": 8}, "fuse_operands=0")
    finally:
        restore(ctx)


# ---- 8. FP32 operand values ----
@pytest.mark.parametrize("shape", ["u5", "u7", "u4_rounded"])
def test_fp32_operand_values(ctx, mg, shape):
    """values that are multiples of 2⁻¹⁰ below 2¹⁰: every A·P sum is exact, so the float rounding does not depend on the summation order and
    the FP32 restatement is a promise.  u5: the five-point operator with one-member aggregates, A·P = A, mean row length in (4.5, 5.5] and
    longest row 5 — the U = 5 instance; u7: the nine-point operator with pairs (U = 7).  Such values are floats already, so the FP32 level
    must return the FP64 level's bits, from the float kernel (`info`).  u4_rounded: the line operator with unquantized values, whose float
    copies differ from the doubles — the restatement rounds the merged values (summed in the documented order) to float, the result moves."""
    rng = np.random.default_rng(81)
    n = 700
    q = dict(quantum=2.0 ** -10, diag_shift=4.0)
    if shape == "u5":
        c = R.Case(R.randomize(R.stencil_5pt(n), rng, **q), np.arange(n, dtype=np.int32), seed=82)
        assert 4.5 < c.merged.mean_len <= 5.5 and c.merged.max_len <= 10
    elif shape == "u7":
        c = R.Case(R.randomize(stencil_9pt(n), rng, **q), R.pairs(n), seed=83)
    else:
        c = R.Case(R.randomize(R.stencil_1d2d(n), rng), R.pairs(n), seed=84)
    exact = shape != "u4_rounded"
    if exact:
        assert np.array_equal(c.merged.val * 1024, np.round(c.merged.val * 1024)) and np.abs(c.merged.val).max() < 1024
    u = {"u5": 5, "u7": 7, "u4_rounded": 4}[shape]
    try:
        h = build(ctx, mg, c)
        x64, _ = run(ctx, mg, h, c, "merged", {"operand": 2, "kernel": 1, "U": u}, f"fp32 {shape}: FP64 values")
        h.set_operand_precision(32)
        assert h.operand_precision(0) == 32
        x32, _ = run(ctx, mg, h, c, "merged32", {"operand": 2, "kernel": 2, "U": u}, f"fp32 {shape}: FP32 values", bits=True)
        assert np.array_equal(x32["t"], x64["t"]) == exact and np.array_equal(x32["rb"], x64["rb"]) == exact
        # a hierarchy built without pattern codes: the float form stages index slices (its integer region then holds capv + 8 entries)
        ctx.set_option("rowcode", 0)
        hs = build(ctx, mg, c).set_operand_precision(32)
        xs, _ = run(ctx, mg, hs, c, "merged32", {"operand": 2, "kernel": 2, "U": u}, f"fp32 {shape}: FP32 values, index slices", bits=True)
        info = hs.post_pass(0, ctx.vec(c.t), None, ctx.vec(c.ec), ctx.vec(c.n))
        assert info["capi"] == info["capv"] + 8 and hs.fused_info(0)["coded_col_agg"] == 0, f"{info}"
        assert np.array_equal(xs["t"], x32["t"]) and np.array_equal(xs["rb"], x32["rb"])
    finally:
        restore(ctx)


# ---- 9. grouped levels of device-built hierarchies ----
def downloaded_case(h, omega, seed):
    rp, ci, v = h.level_A(0).download(); n = h.level_shape(0)[0]
    return R.Case(sps.csr_matrix((v, ci, rp), shape=(n, n)), h.level_P(0).agg(), omega, seed)


@pytest.mark.parametrize("kind", ["poisson3d_33", "CSky3d30"])
def test_grouped_level(ctx, mg, inputs, kind):
    """device aggregation with the small-level grouping options of test_gpu_pre_nodiag.py: the level's own cycle runs the t-form; the group
    sweep gives the same bits; the device pre pass feeds the post pass (e_c chosen by the test) and the result is the host chain's; and with
    the e_c of a real cycle the two passes reproduce mgs_vcycle.  That last sub-check stays at the cycle tests' 1e-10 in the 2-norm: e_c
    comes from eight damped-Jacobi sweeps restated in FP64 on the host, whose own error is not derived here."""
    A = ctx.poisson3d(33) if kind == "poisson3d_33" else mg.Csr.from_mtx(ctx, inputs[kind])
    try:
        ctx.set_option("group_stray_pct", 60); ctx.set_option("group_min_blocks", 1)
        h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 200, 32).finalize()
        c = downloaded_case(h, 0.6, 91)
        # the 7-point operator's A·P repeats its row shapes: the coded kernel, swept group by group on request; the bundled operator's
        # aggregates follow its variable coefficients, its A·P has no pattern code and the gather kernel serves it whatever group_sweep says
        k0, k1 = (1, 3) if kind == "poisson3d_33" else (0, 0)
        x0, _ = run(ctx, mg, h, c, "merged", {"operand": 2, "kernel": k0, "t_form": 1}, f"grouped {kind} group_sweep=0")
        assert h.group_info(0)["groups"] > 0
        ctx.set_option("group_sweep", 1)
        x1, _ = run(ctx, mg, h, c, "merged", {"operand": 2, "kernel": k1, "t_form": 1}, f"grouped {kind} group_sweep=1")
        assert np.array_equal(x0["t"], x1["t"]) and np.array_equal(x0["rb"], x1["rb"])
        ctx.set_option("group_sweep", 0)
        # pre pass → post pass on the device against the host chain
        n, nc = c.n, c.nc
        b = ctx.vec(c.b); t, r, rc = Guarded(ctx, mg, n), Guarded(ctx, mg, n), Guarded(ctx, mg, nc)
        h.pre_pass(0, b, t.v, r.v, rc.v)
        t_dev = t.check("t"); rc_dev = rc.check("r_c")
        t_host, _, rc_host = R.pre_pass_host(c.A, c.d, c.agg, nc, c.b)
        assert np.linalg.norm(t_dev - t_host) <= 1e-13 * np.linalg.norm(t_host) and np.linalg.norm(rc_dev - rc_host) <= 1e-13 * np.linalg.norm(rc_host)
        x = Guarded(ctx, mg, n)
        info = h.post_pass(0, t.v, None, ctx.vec(c.ec), x.v)
        assert info["t_form"] == 1 and info["kernel"] == k0, f"{info}"
        assert np.array_equal(x.check("x"), R.evaluate(c.merged, c.d, c.agg, c.ec, t_dev, None))
        # the e_c of a real cycle: two levels, the coarsest (more than 8192 rows) smoothed by eight damped-Jacobi sweeps from zero
        h2 = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 1, 8.0, 200, 2).finalize()
        assert h2.nlev == 2 and h2.level_shape(1)[0] > 8192 and h2.group_info(0)["groups"] >= 0
        c2 = downloaded_case(h2, 0.6, 92)
        xv = h2.vcycle(b).numpy()
        rp, ci, v = h2.level_A(1).download()
        Ac = sps.csr_matrix((v, ci, rp), shape=(c2.nc, c2.nc)); wc = 0.6 * (1.0 / Ac.diagonal())
        t2, r2, rc2 = R.pre_pass_host(c2.A, c2.d, c2.agg, c2.nc, c.b)
        e = wc * rc2
        for _ in range(7):
            e = e + wc * (rc2 - Ac @ e)
        x = Guarded(ctx, mg, n)
        info = h2.post_pass(0, ctx.vec(t2), None, ctx.vec(e), x.v)
        xt = x.check("x")
        x = Guarded(ctx, mg, n)
        h2.post_pass(0, ctx.vec(r2), b, ctx.vec(e), x.v)
        xr = x.check("x")
        et, er = np.linalg.norm(xt - xv) / np.linalg.norm(xv), np.linalg.norm(xr - xv) / np.linalg.norm(xv)
        print(f"grouped {kind}: two passes with a real cycle's e_c vs mgs_vcycle: t-form {et:.3e}, (r, b)-form {er:.3e} (level's own: {'t' if info['t_form'] else 'rb'})")
        assert et <= 1e-10 and er <= 1e-10
    finally:
        restore(ctx)


# ---- 10. row-block ranges ----
def blocks_of(rg):
    b0, b1, ga, gl = rg
    return [b + gl if b >= ga else b for b in range(b0, b1)]


@pytest.mark.parametrize("xcd_remap", [1, 0])
def test_row_block_ranges(ctx, mg, xcd_remap):
    """70 row blocks (the XCD remap starts at 64), the last one partial: the whole level, a short range, the boundary launch of a row shard's
    split (5 leading + 4 trailing blocks in one launch) and its interior.  Rows of other blocks keep their sentinel; boundary + interior give
    the whole level's bits."""
    rng = np.random.default_rng(101)
    n = 70 * 256 - 100; nb = 70
    c = R.Case(R.randomize(R.stencil_5pt(n, 64), rng), R.pairs(n), seed=102)
    ranges = {"whole": (0, nb, INT_MAX, 0), "short": (3, 9, INT_MAX, 0), "boundary": (0, 5 + 4, 5, nb - 9), "interior": (5, nb - 4, INT_MAX, 0)}
    assert blocks_of(ranges["boundary"]) == [0, 1, 2, 3, 4, 66, 67, 68, 69]
    try:
        h = build(ctx, mg, c)
        ctx.set_option("xcd_remap", xcd_remap)
        ref, worst = run(ctx, mg, h, c, "merged", {"operand": 2, "kernel": 1}, f"ranges xcd_remap={xcd_remap}: NULL range")
        ec = ctx.vec(c.ec)
        for form, bvec, xin in c.forms():
            got = {}
            for name, rg in ranges.items():
                x = Guarded(ctx, mg, n)
                info = h.post_pass(0, ctx.vec(bvec), ctx.vec(xin) if xin is not None else None, ec, x.v, range=rg)
                assert info["operand"] == 2 and info["kernel"] == 1, info
                xd = x.check(f"{name}/{form}")
                inside = np.zeros(n, dtype=bool)
                for b in blocks_of(rg):
                    inside[b * 256:(b + 1) * 256] = True
                assert np.all(xd[~inside] == SENT), (name, form, "rows outside the range were written", np.flatnonzero(xd[~inside] != SENT)[:8])
                assert np.array_equal(xd[inside], ref[form][inside]), (name, form)
                got[name] = (xd, inside)
            assert np.array_equal(got["whole"][0], ref[form])
            both = np.where(got["boundary"][1], got["boundary"][0], got["interior"][0])
            assert not np.any(got["boundary"][1] & got["interior"][1]) and np.array_equal(both, ref[form])
    finally:
        restore(ctx)


# ---- 11. refusals ----
def code_of(mg, fn):
    with pytest.raises(mg.MgsError) as e:
        fn()
    return e.value.code


def test_refusals(ctx, mg):
    INVALID, STATE = -1, -6
    rng = np.random.default_rng(111)
    n = 600
    c = R.Case(R.randomize(R.stencil_5pt(n), rng), R.pairs(n), seed=112)
    lib = mg.lib()
    try:
        h = mg.Hierarchy(upload(ctx, c.A), 0.6, 1, 1)
        h.push_P(upload(ctx, R.agg_P(c.agg, c.nc))); h.push_P(upload(ctx, R.agg_P((np.arange(c.nc) * 8 // c.nc).astype(np.int32), 8)))
        t, ec, x = ctx.vec(c.t), ctx.vec(c.ec), ctx.vec(n)
        assert code_of(mg, lambda: h.post_pass(0, t, None, ec, x)) == STATE                     # before finalize
        h.finalize()
        h.post_pass(0, t, None, ec, x)
        out = (C.c_int64 * 8)()
        for args in ((None, 0, t.h, None, ec.h, x.h, None, out), (h.h, 0, None, None, ec.h, x.h, None, out), (h.h, 0, t.h, None, None, x.h, None, out),
                     (h.h, 0, t.h, None, ec.h, None, None, out), (h.h, 0, t.h, None, ec.h, x.h, None, None)):
            assert lib.mgs_hier_post_pass(*args) == INVALID                                       # NULL arguments
        assert code_of(mg, lambda: h.post_pass(-1, t, None, ec, x)) == INVALID                  # level out of range
        assert code_of(mg, lambda: h.post_pass(2, t, None, ec, x)) == INVALID                   # the coarsest level has no coarser one
        assert code_of(mg, lambda: h.post_pass(0, ctx.vec(n - 1), None, ec, x)) == INVALID      # vectors too short
        assert code_of(mg, lambda: h.post_pass(0, t, ctx.vec(n - 1), ec, x)) == INVALID
        assert code_of(mg, lambda: h.post_pass(0, t, None, ctx.vec(c.nc - 1), x)) == INVALID
        assert code_of(mg, lambda: h.post_pass(0, t, None, ec, ctx.vec(n - 1))) == INVALID
        for rg in ((0, 4, INT_MAX, 0), (-1, 2, INT_MAX, 0), (2, 1, INT_MAX, 0), (0, 2, 1, 2), (0, 2, 1, -1)):
            assert code_of(mg, lambda: h.post_pass(0, t, None, ec, x, range=rg)) == INVALID     # a range that leaves the level's 3 row blocks
        h.set_smoother(0.6, 2, 1)
        assert code_of(mg, lambda: h.post_pass(0, t, None, ec, x)) == STATE                     # V(2,1): no fused passes
        h.set_smoother(0.6, 1, 1)
        h.post_pass(0, t, None, ec, x)
        # a general P
        N = 24; m = N * N; mc = m // 2
        i = np.arange(m)
        P = sps.coo_matrix((np.r_[np.ones(m), np.full(m, 0.25)], (np.r_[i, i], np.r_[i // 2, np.minimum(i // 2 + 1, mc - 1)])), shape=(m, mc)).tocsr()
        hg = mg.Hierarchy(ctx.poisson2d(N), 0.6, 1, 1).push_P(upload(ctx, P)).finalize()
        assert not hg.level_P(0).is_aggregation
        assert code_of(mg, lambda: hg.post_pass(0, ctx.vec(m), None, ctx.vec(mc), ctx.vec(m))) == STATE
        # a value-coded level
        ctx.set_option("valcode", 1)
        hv = mg.Hierarchy(ctx.poisson3d(12), 0.6, 1, 1).coarsen(10.0, 2, 8.0, 50, 8).finalize()
        assert code_of(mg, lambda: hv.post_pass(0, ctx.vec(12 ** 3), None, ctx.vec(hv.level_shape(1)[0]), ctx.vec(12 ** 3))) == STATE
        ctx.set_option("valcode", 0)
        # a row shard: planes 4..11 of 16 with halo columns, aggregated and coarsened as a shard (no halo on the coarse level)
        As = ctx.poisson3d(16, 4, 12, local_cols=True)
        rows, cols = As.shape
        assert cols > rows
        T, Ac = C.c_void_p(), C.c_void_p()
        assert lib.mgs_aggregate_shard(As.h, 10.0, 1, 8.0, C.byref(T)) == 0
        hc = np.full(cols - rows, -1, dtype=np.int32)
        assert lib.mgs_galerkin_shard(As.h, T, hc.ctypes.data_as(C.POINTER(C.c_int)), 0, C.byref(Ac)) == 0
        hs = mg.Hierarchy(As, 0.6, 1, 1)
        assert lib.mgs_hier_push_level(hs.h, T, Ac) == 0
        hs.finalize()
        ncs = hs.level_shape(1)[0]
        assert code_of(mg, lambda: hs.post_pass(0, ctx.vec(cols), None, ctx.vec(ncs), ctx.vec(cols))) == STATE
    finally:
        restore(ctx)
