"""Option pack7: the fused passes of an unsharded FP64 level stream a packed copy of their operands' values, 7 bytes per entry, in the coded row
blocks whose values span fewer than 8 binades (the format restated in tests/pack7_ref.py).  Nothing is rounded, so every result
must have the bits it has with the option off: each case runs pack7 = 1 against pack7 = 0 in one process, compares with np.array_equal, and
asks mgs_hier_pack_info which arm the launches took."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import pack7_ref as P7
import post_pass_ref as R
from test_gpu_pre_nodiag import banded700

pytestmark = pytest.mark.gpu

DEFAULTS = (("pack7", 1), ("pre_nodiag", 1), ("rowcode", 1), ("fuse_restrict", 1), ("group_stray_pct", 6), ("group_min_blocks", 1024), ("aggpre_max_rows", 300000),
            ("valcode", 0))


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


def small_levels(ctx, stray_pct=100, min_blocks=1):
    """every level groups its row blocks (the grouped pre pass at test sizes); min_blocks: levels with fewer row blocks keep the separate kernels"""
    ctx.set_option("group_stray_pct", stray_pct); ctx.set_option("group_min_blocks", min_blocks)


def upload(ctx, M):
    M = M.tocsr(); M.sort_indices()
    return ctx.csr(M.shape[0], M.shape[1], M.indptr, M.indices, M.data)


def dominant(pattern, rng, lo=1.0, hi=2.0):
    """off-diagonal values from −[lo, hi), rows strictly diagonally dominant: sums of entries of one row do not cancel, so A·P's values and
    Â's stay within a few binades of each other"""
    S = pattern.tocsr().copy(); S.setdiag(0); S.eliminate_zeros()
    S.data = -rng.uniform(lo, hi, S.nnz)
    M = (S + sps.diags(-np.asarray(S.sum(axis=1)).ravel() + rng.uniform(0.5, 1.5, S.shape[0]))).tocsr()
    M.sort_indices()
    return M


def on_off(ctx, fn):
    """fn() with the option on, then off"""
    ctx.set_option("pack7", 1); a = fn()
    ctx.set_option("pack7", 0); b = fn()
    ctx.set_option("pack7", 1)
    return a, b


def pre_width(rowptr):
    """the gather width of the pre pass's walk (rowblock.hpp: gather_width)"""
    ln = np.diff(rowptr); mean = ln.mean()
    return 4 if mean <= 4.5 else (7 if mean <= 7.5 and ln.max() <= 14 else 8)


def passes_alone(ctx, mg, h, level=0, seed=1, want_pre_source=None, need_packed=True, coded_post=False):
    """both passes of one level alone, option on against off; returns (pre width or None, post width, pack info with the option on).
    need_packed: the operator is one whose blocks are eligible — the packed arm must be the one taken; otherwise the packed form of the kernel
    may find every block ineligible and only the bits are held.  coded_post: the pattern code serves A·P, so the post pass must run the coded
    kernel's packed form (on device-built aggregates of small grids it often does not: the gather kernel then reads the FP64 values)"""
    n = h.level_shape(level)[0]; nc = h.level_shape(level + 1)[0]
    rng = np.random.default_rng(seed)
    b = ctx.vec(rng.uniform(-1.0, 1.0, n)); ec = ctx.vec(rng.uniform(-1.0, 1.0, nc)); r = ctx.vec(rng.uniform(-1.0, 1.0, n))
    h.vcycle(ctx.vec(np.ones(h.level_shape(0)[0])))       # the first cycle builds the operands
    upre = None
    info = {}
    if h.group_info(level)["groups"] > 0:
        def pre():
            t, rs, rc = R.Guarded(ctx, mg, n), ctx.vec(np.zeros(n)), R.Guarded(ctx, mg, nc)
            h.pre_pass(level, b, t.v, rs, rc.v)
            return t.check("t"), rs.numpy(), rc.check("r_c"), h.pack_info(level)
        (t1, s1, rc1, i1), (t0, s0, rc0, i0) = on_off(ctx, pre)
        assert i1["pre_ran"] == 1 and i0["pre_ran"] == 0 and i0["pre_packed"] == 0 and (i1["pre_packed"] >= 1 or not need_packed), (i1, i0)
        if want_pre_source is not None:
            assert i1["pre_source"] == want_pre_source, i1
        assert np.array_equal(t1, t0) and np.array_equal(rc1, rc0) and np.array_equal(s1, s0)
        assert np.all(np.isfinite(t1)) and np.any(t1 != b.numpy())
        upre = pre_width(h.level_A(level).download()[0])
        info = i1
    upost = None
    for bvec, xin in ((b, None), (r, b)):                   # the t-form and the (r, b)-form
        def post():
            x = R.Guarded(ctx, mg, n)
            pi = h.post_pass(level, bvec, xin, ec, x.v)
            return x.check("x"), pi, h.pack_info(level)
        (x1, p1, i1), (x0, p0, i0) = on_off(ctx, post)
        assert p1["operand"] == 2 and p1 == p0 and (p1["kernel"] == 1 or not coded_post), (p1, p0)
        assert i1["post_ran"] == int(p1["kernel"] == 1) and i0["post_ran"] == 0 and i0["post_packed"] == 0 and (i1["post_packed"] >= 1 or not need_packed), (i1, i0)
        assert np.array_equal(x1, x0) and np.all(np.isfinite(x1))
        upost = p1["U"]; info = i1
    return upre, upost, info


def coarsened(ctx, mg, A, omega, npass=2):
    return mg.Hierarchy(A, omega, 1, 1).coarsen(10.0, npass, 8.0, 200, 32).finalize()


def csky(ctx, mg, N):
    from multigridsolver_amd import synthetic
    rp, ci, v = synthetic.csky3d(N)
    return ctx.csr(N ** 3, N ** 3, rp, ci, v)


@pytest.mark.parametrize("omega", [0.6, 0.8])
@pytest.mark.parametrize("kind", ["banded700", "poisson3d_9", "poisson3d_16", "csky3d_12"])
def test_passes_alone(ctx, mg, kind, omega):
    """row-to-row different diagonals and a partial last block (the banded matrix, 9³ = 729 rows), the grouped level on the operand without
    diagonal entries (16³), variable coefficients and a nonsymmetric operator (csky3d)"""
    try:
        small_levels(ctx)
        if kind == "banded700":
            A = upload(ctx, banded700())
        elif kind.startswith("poisson3d"):
            A = ctx.poisson3d(int(kind.split("_")[1]))
        else:
            A = csky(ctx, mg, 12)
        h = coarsened(ctx, mg, A, omega)
        upre, upost, info = passes_alone(ctx, mg, h, 0, seed=5, want_pre_source=2 if kind == "poisson3d_16" else None, need_packed=not kind.startswith("csky"))
        assert upre is not None                               # level 0 ran grouped: the pre pass alone was compared
        print(f"{kind} omega={omega}: pre U={upre} post U={upost} {info}")
    finally:
        restore(ctx)


def test_every_gather_width(ctx, mg):
    """U = 4, 5, 7, 8 of the post pass and 4, 7, 8 of the pre pass, each reached by at least one operator: the line, the band and the 27-point
    patterns of tests/test_gpu_post_pass.py with pairs as aggregates, and its five-point operator with one-member aggregates (A·P = A: five
    entries per row)"""
    rng = np.random.default_rng(17)
    pre, post = set(), set()
    try:
        small_levels(ctx)
        for name, fn, n, agg in (("line", R.stencil_1d2d, 600, R.pairs(600)), ("band7", _band7, 600, R.pairs(600)), ("27_point", R.stencil_27pt, 700, R.pairs(700)),
                                 ("five_point_singletons", R.stencil_5pt, 700, np.arange(700, dtype=np.int32))):      # A·P = A: five entries per row
            M = dominant(fn(n), rng)
            nc = int(agg.max()) + 1
            h = mg.Hierarchy(upload(ctx, M), 0.6, 1, 1)
            h.push_P(upload(ctx, R.agg_P(agg, nc)))
            h.push_P(upload(ctx, R.agg_P((np.arange(nc) * 8 // nc).astype(np.int32), 8)))
            h.finalize()
            upre, upost, info = passes_alone(ctx, mg, h, 0, seed=n, coded_post=True)
            print(f"{name}: pre U={upre} post U={upost} {info}")
            pre.add(upre); post.add(upost)
        assert {4, 5, 7, 8} <= post and {4, 7, 8} <= pre, (pre, post)
    finally:
        restore(ctx)


def _band7(n):
    """couplings at distance 2, 4 and 32 (tests/test_gpu_post_pass.py: stencil_band7): with pairs every entry of a row keeps an aggregate of its own"""
    i = np.arange(n)
    r, c = [], []
    for o in (2, 4, 32):
        r += [i[:-o], i[o:]]; c += [i[o:], i[:-o]]
    return sps.csr_matrix((np.ones(sum(map(len, r))), (np.concatenate(r), np.concatenate(c))), shape=(n, n))


def test_mixed_blocks(ctx, mg):
    """four row blocks (1000 rows, pairs as aggregates): rows of block 1 alternate between scales 1 and 2²⁰, so its slices of Â and of A·P span
    far more than 8 binades; block 2 holds an explicitly stored zero; blocks 0 and 3 are plain.  The device must leave exactly the blocks
    unpacked that the host restatement leaves, and the results keep their bits."""
    n = 1000
    rng = np.random.default_rng(23)
    i = np.arange(n)
    pat = sps.csr_matrix((np.ones(4 * n - 6), (np.r_[i[:-1], i[1:], i[:-2], i[2:]], np.r_[i[1:], i[:-1], i[2:], i[:-2]])), shape=(n, n))
    M = dominant(pat, rng)
    s = np.ones(n); s[258:510:2] = 2.0 ** 20             # (the columns that blocks 0 and 2 reach into block 1 stay unscaled)
    M = (sps.diags(s) @ M).tocsr(); M.sort_indices()
    k0 = M.indptr[600] + int(np.flatnonzero(M.indices[M.indptr[600]:M.indptr[601]] == 602)[0])
    M.data[k0] = 0.0                                        # stays stored: the CSR arrays are uploaded as they are
    agg = R.pairs(n); nc = n // 2
    omega = 0.6
    # the host's view of the two operands: Â = A·diag(ω·(1/a_jj)), with and without its diagonal entries, and A·P
    d = omega * (1.0 / M.diagonal())
    hat = M.data * d[M.indices]
    offd = M.indices != np.repeat(i, np.diff(M.indptr))
    ap, _ = R.operand_merged(M, agg)
    e_hat = P7.eligibility(hat, P7.block_bounds(M.indptr))
    e_nd = P7.eligibility(hat[offd], P7.block_bounds(M.indptr, nd=True))
    e_ap = P7.eligibility(ap.val, P7.block_bounds(ap.rowptr))
    for e in (e_hat, e_nd, e_ap):
        assert list(e >= 0) == [True, False, False, True], e          # the fixture has both kinds, where it is meant to
    try:
        small_levels(ctx)
        h = mg.Hierarchy(upload(ctx, M), omega, 1, 1)
        h.push_P(upload(ctx, R.agg_P(agg, nc))); h.push_P(upload(ctx, R.agg_P((np.arange(nc) * 8 // nc).astype(np.int32), 8)))
        h.finalize()
        upre, _, info = passes_alone(ctx, mg, h, 0, seed=29, coded_post=True)
        assert upre is not None                               # level 0 ran grouped
        assert info["pre_blocks"] == 4 and info["post_blocks"] == 4 and info["pre_packed"] == 2 and info["post_packed"] == 2, info
        assert info["pre_source"] in (1, 2)
        b = ctx.vec(n).rand(seed=31)
        x1, x0 = on_off(ctx, lambda: h.vcycle(b).numpy())
        assert np.array_equal(x1, x0)
    finally:
        restore(ctx)


@pytest.mark.parametrize("kind", ["poisson3d_24", "csky3d_16"])
def test_whole_cycle_and_rebuilt_operands(ctx, mg, kind):
    """h.vcycle through all levels — level 0 grouped, the levels below it on the separate kernels, the smallest on the aggregate-parallel kernel —
    then again after a new ω and after new values + refresh: the packed copies follow their sources"""
    N = int(kind.split("_")[1]); n = N ** 3
    try:
        small_levels(ctx, 100, 16); ctx.set_option("aggpre_max_rows", 1000)
        A = ctx.poisson3d(N) if kind.startswith("poisson") else csky(ctx, mg, N)
        h = coarsened(ctx, mg, A, 0.6)
        b = ctx.vec(n).rand(seed=7)
        x1, x0 = on_off(ctx, lambda: h.vcycle(b).numpy())
        assert np.array_equal(x1, x0) and np.all(np.isfinite(x1))
        assert h.nlev >= 4 and h.group_info(0)["groups"] > 0 and h.group_info(1)["groups"] == 0
        h.vcycle(b)
        i0, i1 = h.pack_info(0), h.pack_info(1)
        print(kind, i0, i1, [h.level_shape(l)[0] for l in range(h.nlev)])
        # level 0: the grouped kernel on the operand without diagonal entries; level 1: the separate kernels on Â.  Where the pattern code does not
        # serve an operand (Galerkin levels, variable coefficients) another kernel runs and reports 0
        poisson = kind.startswith("poisson")
        assert i0["pre_ran"] == 1 and i0["pre_source"] == 2 and i0["pre_packed"] >= 1 and i0["post_packed"] >= 1 and i0["post_ran"] in (0, 1), i0
        assert h.level_shape(1)[0] > 1000 and i1["pre_source"] == 1 and i1["pre_ran"] in (0, 1) and i1["post_ran"] in (0, 1), i1
        if poisson:
            assert i0["post_ran"] == 1 and i1["pre_ran"] == 1 and i0["pre_packed"] == i0["pre_blocks"], (i0, i1)
        small = [l for l in range(h.nlev - 1) if h.level_shape(l)[0] <= 1000]
        assert small and all(h.pack_info(l)["pre_ran"] == -1 for l in small)      # the small-level kernel reads Â itself
        # a new ω rescales Â
        h.set_smoother(0.8, 1, 1)
        y1, y0 = on_off(ctx, lambda: h.vcycle(b).numpy())
        assert np.array_equal(y1, y0) and not np.array_equal(y1, x1)
        assert h.pack_info(0)["pre_ran"] == 0
        h.vcycle(b)
        assert h.pack_info(0)["pre_ran"] == 1 and (h.pack_info(0)["pre_packed"] >= 1 or not poisson)      # (csky3d: a few eligible blocks at most)
        # new values on the same pattern
        rp, ci, v = A.download()
        s = 1.0 + 0.2 * np.random.default_rng(3).random(n)
        A.update_values(v * s[np.repeat(np.arange(n), np.diff(rp))] * s[ci] * 1.25); h.refresh()
        z1, z0 = on_off(ctx, lambda: h.vcycle(b).numpy())
        assert np.array_equal(z1, z0) and not np.array_equal(z1, y1)
        h.vcycle(b)
        assert h.pack_info(0)["pre_ran"] == 1 and h.pack_info(0)["post_ran"] == i0["post_ran"] and h.pack_info(1)["pre_ran"] == i1["pre_ran"]
    finally:
        restore(ctx)


def test_refusals_and_neutrality(ctx, mg):
    """a level on FP32 operands, a value-coded context and a row shard report no packed block and keep their results"""
    lib = mg.lib()
    try:
        small_levels(ctx)
        n = 16 ** 3
        b = ctx.vec(n).rand(seed=9)
        # FP32 operand values: the float forms of the kernels
        h = coarsened(ctx, mg, ctx.poisson3d(16), 0.6)
        x64 = h.vcycle(b).numpy()
        assert h.pack_info(0)["pre_packed"] >= 1
        h.set_operand_precision(32)
        x1, x0 = on_off(ctx, lambda: h.vcycle(b).numpy())
        h.vcycle(b)
        i = h.pack_info(0)
        assert np.array_equal(x1, x0) and not np.array_equal(x1, x64) and i["pre_packed"] == 0 and i["post_packed"] == 0 and i["pre_ran"] == 0 and i["post_ran"] == 0, i
        h.set_operand_precision(64)
        assert np.array_equal(h.vcycle(b).numpy(), x64) and h.pack_info(0)["pre_ran"] == 1
        # value tuples
        ctx.set_option("valcode", 1)
        hv = coarsened(ctx, mg, ctx.poisson3d(16), 0.6)
        v1, v0 = on_off(ctx, lambda: hv.vcycle(b).numpy())
        i = hv.pack_info(0)
        assert np.array_equal(v1, v0) and i["pre_packed"] == 0 and i["post_packed"] == 0 and i["pre_ran"] <= 0 and i["post_ran"] <= 0, i
        ctx.set_option("valcode", 0)
        # a row shard: planes 4..11 of 16 with halo columns (the hierarchy of tests/test_gpu_post_pass.py::test_refusals), halo values left at zero
        As = ctx.poisson3d(16, 4, 12, local_cols=True)
        rows, cols = As.shape
        T, Ac = C.c_void_p(), C.c_void_p()
        assert lib.mgs_aggregate_shard(As.h, 10.0, 1, 8.0, C.byref(T)) == 0
        hc = np.full(cols - rows, -1, dtype=np.int32)
        assert lib.mgs_galerkin_shard(As.h, T, hc.ctypes.data_as(C.POINTER(C.c_int)), 0, C.byref(Ac)) == 0
        hs = mg.Hierarchy(As, 0.6, 1, 1)
        assert lib.mgs_hier_push_level(hs.h, T, Ac) == 0
        hs.finalize()
        hs.set_halo_exchange(lambda level, ptr: None)
        hs.set_halo_exchange_fused(lambda level, kind, a, bb, out, phase: None)
        bs = ctx.vec(np.r_[np.random.default_rng(4).uniform(-1, 1, rows), np.zeros(cols - rows)])
        s1, s0 = on_off(ctx, lambda: hs.vcycle(bs, ctx.vec(np.zeros(cols))).numpy()[:rows])
        i = hs.pack_info(0)
        assert np.array_equal(s1, s0, equal_nan=True) and i["pre_packed"] == 0 and i["post_packed"] == 0 and i["pre_ran"] <= 0 and i["post_ran"] <= 0, i
    finally:
        restore(ctx)
