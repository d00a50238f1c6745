"""The cycle's fused pre pass alone (mgs_hier_pre_pass_info) against the exact host restatement of tests/pre_pass_ref.py, arm by arm.

Every case builds its operator in numpy (values and b from ±[0.5, 2]), pushes an explicit aggregation P (plus a second transfer onto eight
aggregates, so the dense coarsest solve costs nothing), runs the pass into sentinel-filled guarded vectors and asserts
  * from `info` that the arm, the kernel and the instantiation the case was built for ran, and that the guard zones are untouched;
  * that the unwritten outputs are exactly those the arm does not write: the grouped arm writes t and r_c everywhere and r on the rows of the
    64-row waves that hold a member of a stray aggregate (predicted on the host from the grouping rule), the other arms write r and r_c
    everywhere and leave t alone;
  * every row and aggregate against the derived bars of the long-double restatement;
  * every row and aggregate for EQUAL BITS with the FP64 restatement — all cases but the one whose rows exceed 64 entries, where the kernels
    promise no order (the bars do not depend on the order, so that case's rows are all still covered).
Each case prints its largest error/bar ratio.  The cases on device-built hierarchies use the project's own operators and aggregates.

Largest error/bar ratios measured on an MI355X when the tests were written (a row or aggregate passes at ≤ 1; every case but the long rows also
returned the restatement's bits): grouped arm, row counts × U = 4 / 7 / 8 (nine-point) / 8 (27-point) 0.20–0.25 / 0.14–0.23 / 0.12–0.19 / 0.09–0.11,
the same under every launch option; group shapes 0.17–0.31 (triples 0.31, rows outside every aggregate 0.29); staging forms 0.26; value forms 0.24
(FP64, packed, without diagonal, pair kernel: one figure, they return the same bits) and 0.24 on FP32 values; device-built levels 0.16 / 0.14
(poisson3d(33), levels 0 / 1) and 0.26 / 0.19 (CSky3d30); aggregate-parallel arm 0.10–0.26; residual on Â 0.10–0.26, long rows 0.23; gather form on A
0.09–0.22."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import pack7_ref as P7
import post_pass_ref as R
import pre_pass_ref as Q
from post_pass_ref import Guarded, SENT
from test_gpu_post_pass import stencil_9pt, stencil_band7, upload

pytestmark = pytest.mark.gpu

# the defaults of mgs_internal.hpp (struct mgs_ctx) of every option a test here sets
DEFAULTS = (("rowcode", 1), ("rowptr_scan", 1), ("stage_unroll", 1), ("nt_store", 1000000), ("pre_nodiag", 1), ("pack7", 1), ("fuse_operands", 1),
            ("fuse_restrict", 1), ("group_stray_pct", 6), ("group_min_blocks", 1024), ("group_blocks", 4), ("group_concurrent", 0),
            ("aggpre_max_rows", 300000), ("valcode", 0), ("merge_ap", 1))
GATHER, RESIDUAL, AGGPAR, GROUPED = 0, 1, 2, 3                      # info["arm"]
K_GATHER, K_CODED, K_CODED32, K_SLICE, K_AGG, K_GROUP, K_PAIR = 0, 1, 2, 4, 5, 6, 7      # info["kernel"]
OMEGA = 0.6
RB = 256


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


def set_grouping(ctx, blocks=4):
    ctx.set_option("group_min_blocks", 1); ctx.set_option("group_stray_pct", 100); ctx.set_option("group_blocks", blocks)


class Level:
    """one level under test: operator, aggregates, b"""
    def __init__(self, A, agg, seed, omega=OMEGA, b=None):
        self.A = A.tocsr(); self.A.sort_indices()
        self.agg = np.asarray(agg, dtype=np.int32); self.n = self.A.shape[0]; self.nc = int(self.agg.max()) + 1
        assert self.nc >= 1 and len(self.agg) == self.n
        self.omega = omega
        self.b = R.signed(np.random.default_rng(seed), self.n) if b is None else b
        self.nblocks = (self.n + RB - 1) // RB
        self.max_len = int(np.diff(self.A.indptr).max()); self.mean_len = self.A.nnz / self.n
        self._ref = {}
        self._tables = None

    @property
    def tables(self):
        if self._tables is None:
            self._tables = predict_tables(self.A)
        return self._tables

    def ref(self, form, f32):
        """(FP64 restatement, long-double restatement, bars), computed once per form"""
        key = (form, f32)
        if key not in self._ref:
            a = (self.A, self.omega, self.agg, self.nc, self.b)
            self._ref[key] = (Q.evaluate(*a, np.float64, form, f32), Q.evaluate(*a, np.longdouble, form, f32), Q.bars(*a, form, f32))
        return self._ref[key]

    @property
    def u(self):
        """the gather width the launchers document for the pre pass's operand (gather_width)"""
        return 4 if self.mean_len <= 4.5 else (7 if self.mean_len <= 7.5 and self.max_len <= 14 else 8)


def build(ctx, mg, c):
    """hierarchy of the level: its operator, its aggregates, then (where there are enough of them) everything onto eight aggregates"""
    h = mg.Hierarchy(upload(ctx, c.A), c.omega, 1, 1)
    h.push_P(upload(ctx, R.agg_P(c.agg, c.nc)))
    if c.nc >= 16:
        h.push_P(upload(ctx, R.agg_P((np.arange(c.nc) * 8 // c.nc).astype(np.int32), 8)))
    return h.finalize()


def predict_groups(agg, n, group_blocks=4):
    """the grouping rule of mgs_build_groups restated: one link per aggregate from its first member's row block to its last member's; links by
    count descending, then block pair ascending; greedy union while a group keeps at most group_blocks blocks.  An aggregate is a stray if it
    has more than six members or a member outside the group of its first member's block.  Returns (groups as block lists, stray ids)."""
    nc = int(np.max(agg)) + 1
    nb = (n + RB - 1) // RB
    cptr, mem = Q.members_of(agg, nc)
    fb, lb = mem[cptr[:-1]] // RB, mem[cptr[1:] - 1] // RB
    cnt = {}
    for a in np.flatnonzero(lb != fb):
        cnt[(int(fb[a]), int(lb[a]))] = cnt.get((int(fb[a]), int(lb[a])), 0) + 1
    if any(sum(1 for k in cnt if k[0] == blk) > 4 for blk in range(nb)):
        return None, None      # more partners than the setup's four vote slots per block: which four the device keeps is not restated here
    parent, size = list(range(nb)), [1] * nb

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v
    for (a, b_), _ in sorted(cnt.items(), key=lambda kv: (-kv[1], kv[0])):
        ra, rb = find(a), find(b_)
        if ra == rb or size[ra] + size[rb] > group_blocks:
            continue
        ra, rb = min(ra, rb), max(ra, rb)
        parent[rb] = ra; size[ra] += size[rb]
    root = np.array([find(q) for q in range(nb)])
    groups = [np.flatnonzero(root == q).tolist() for q in range(nb) if root[q] == q]
    strays = [a for a in range(nc) if cptr[a + 1] - cptr[a] > 6 or np.any(root[mem[cptr[a]:cptr[a + 1]] // RB] != root[fb[a]])]
    return groups, np.asarray(strays, dtype=np.int64)


def predict_tables(A):
    """the pattern code of mgs_build_rowcode restated, per row block: the table's length in ints (the number of distinct offset tuples plus their
    lengths), 0 where the table would exceed half of the block's entries minus 64 and the block stays uncoded"""
    rp, ci = A.indptr, A.indices
    n = A.shape[0]
    out = []
    for r0 in range(0, n, RB):
        r1 = min(r0 + RB, n)
        tuples = {tuple((ci[rp[i]:rp[i + 1]] - i).tolist()) for i in range(r0, r1)}
        total = len(tuples) + sum(map(len, tuples))
        out.append(total if total <= (rp[r1] - rp[r0]) // 2 - 64 else 0)
    return np.asarray(out, dtype=np.int64)


def predict_blocks(c, info, code, f32):
    """(coded + staged, staged, from global memory) row blocks of a row-block kernel's launch with the LDS budgets it reported: the kernels' own
    block-uniform conditions on the construction's block sizes and predicted tables.  code: "off" no pattern code is handed over, "auto" the
    operator's where it codes at least half of the blocks, "any" the operator's whatever it codes"""
    tl = c.tables if code != "off" else np.zeros(c.nblocks, dtype=np.int64)
    if code == "auto" and (tl > 0).sum() < 0.5 * c.nblocks:
        tl = np.zeros(c.nblocks, dtype=np.int64)
    bounds = c.A.indptr[np.minimum(np.arange(0, c.n + RB, RB), c.n)][:c.nblocks + 1].astype(np.int64)
    lo, hi = bounds[:-1], bounds[1:]
    va = 4 if f32 else 2
    coded = (tl > 0) & (tl <= info["capi"])
    staged = (hi - lo <= info["capv"]) & (coded | (hi - (lo & ~(va - 1)) + va - 1 <= info["capi"]))
    return int((coded & staged).sum()), int(staged.sum()), int((~staged).sum())


def stray_wave_rows(agg, n, strays):
    """rows of the 64-row waves that hold a member of a stray aggregate: where the grouped arm writes r"""
    w = np.zeros((n + 63) // 64, dtype=bool)
    w[np.flatnonzero(np.isin(agg, strays)) // 64] = True
    return np.repeat(w, 64)[:n]


def run(ctx, mg, h, c, want, what, form="hat", f32=False, bits=True, strays=None, level=0, code=None):
    """the level's pre pass into guarded vectors against the restatement; want: info entries the case was built for (">=1": at least one).
    strays: the level's stray aggregates when the arm is the grouped one (predict_groups), or "device" where the grouping is the device's own and
    not restated: r is then written in whole waves, on every member of an aggregate that must be a stray whatever the groups.  Returns (t, r, rc, info, largest error/bar)."""
    t, r, rc = Guarded(ctx, mg, c.n), Guarded(ctx, mg, c.n), Guarded(ctx, mg, c.nc)
    info = h.pre_pass_info(level, ctx.vec(c.b), t.v, r.v, rc.v)
    td, rd, rcd = t.check(f"{what}: guard zones of t"), r.check(f"{what}: guard zones of r"), rc.check(f"{what}: guard zones of r_c")
    for k, v in want.items():
        assert (info[k] >= 1 if v == ">=1" else info[k] == v), f"{what}: {k} should be {v}: {info}"
    assert info["blocks"] == c.nblocks and info["fp32"] == f32, info
    if info["kernel"] != K_AGG:
        assert info["blocks_staged"] + info["blocks_global"] == c.nblocks and 0 <= info["blocks_coded"] <= info["blocks_staged"], info
        if code is not None:
            got = (info["blocks_coded"], info["blocks_staged"], info["blocks_global"])
            assert got == predict_blocks(c, info, code, f32), (what, "row blocks coded / staged / global", got, predict_blocks(c, info, code, f32), info)
    (t64, r64, rc64), (tL, rL, rcL), (bt, br, bc) = c.ref(form, f32)
    assert not np.any(rcd == SENT), (what, "aggregates not written", np.flatnonzero(rcd == SENT)[:8])
    if info["arm"] == GROUPED:
        assert info["U"] == c.u, (what, info, c.mean_len, c.max_len)
        assert not np.any(td == SENT), (what, "rows of t not written", np.flatnonzero(td == SENT)[:8])
        assert strays is not None
        wr = rd != SENT
        if isinstance(strays, str):
            cptr, mem = Q.members_of(c.agg, c.nc)
            blocks_of = [len(set((mem[cptr[a]:cptr[a + 1]] // RB).tolist())) for a in range(c.nc)]
            sure = np.flatnonzero((np.diff(cptr) > 6) | (np.asarray(blocks_of) > 4))      # strays by size, or in more blocks than a group holds
            must = np.isin(c.agg, sure)
            waves = np.r_[wr, np.zeros(-c.n % 64, dtype=bool)].reshape(-1, 64)
            valid = np.r_[np.ones(c.n, dtype=bool), np.zeros(-c.n % 64, dtype=bool)].reshape(-1, 64)
            assert np.all((waves == waves[:, :1]) | ~valid), (what, "r written in part of a wave")
            assert info["stray_aggregates"] >= len(sure) and (info["stray_aggregates"] > 0) == bool(wr.any()), (what, info, len(sure))
        else:
            assert info["stray_aggregates"] == len(strays), (what, info, len(strays))
            must = np.isin(c.agg, strays)
            assert np.array_equal(wr, stray_wave_rows(c.agg, c.n, strays)), (what, "r written outside the stray waves", np.flatnonzero(wr != stray_wave_rows(c.agg, c.n, strays))[:8])
        assert np.all(wr[must]), (what, "members of stray aggregates without r", np.flatnonzero(must & ~wr)[:8])
        checks = [("t", td, t64, tL, bt, slice(None)), ("r", rd, r64, rL, br, wr), ("rc", rcd, rc64, rcL, bc, slice(None))]
    else:
        assert np.all(td == SENT), (what, "t written by an arm that has no t", np.flatnonzero(td != SENT)[:8])
        assert not np.any(rd == SENT), (what, "rows of r not written", np.flatnonzero(rd == SENT)[:8])
        assert info["stray_aggregates"] == 0, info
        checks = [("r", rd, r64, rL, br, slice(None)), ("rc", rcd, rc64, rcL, bc, slice(None))]
    worst = 0.0
    for nm, got, x64, xL, bar_, sel in checks:
        q = Q.ratios(got[sel], xL[sel], bar_[sel])
        if q.size:
            worst = max(worst, float(q.max()))
            assert q.max() <= 1.0, (what, nm, float(q.max()), int(q.argmax()), info)
        if bits:
            assert np.array_equal(got[sel], x64[sel]), (what, nm, "bits", np.flatnonzero(got[sel] != x64[sel])[:8], info)
    print(f"{what}: arm={info['arm']} kernel={info['kernel']} U={info['U']} flags={info['flags']} bits={info['bits']} capv={info['capv']} capi={info['capi']} "
          f"coded/staged/global={info['blocks_coded']}/{info['blocks_staged']}/{info['blocks_global']} strays={info['stray_aggregates']} largest error/bar {worst:.3f}")
    return td, rd, rcd, info, worst


def check_group_info(h, c, groups, strays, what):
    gi = h.group_info(0)
    assert gi == {"groups": len(groups), "paired_groups": c.nblocks - len(groups), "stray_aggregates": len(strays), "blocks": c.nblocks}, (what, gi, groups)


# ---- 1. grouped arm: row counts around the block size × gather widths × launch options ----
GROUPED_STENCILS = {"line": (R.stencil_1d2d, 4), "band7": (stencil_band7, 7), "nine_point": (stencil_9pt, 8),
                    "27_point": (lambda n: R.stencil_27pt(n, 4), 8)}


@pytest.mark.parametrize("n", [255, 256, 257, 513, 1025])
@pytest.mark.parametrize("stencil", list(GROUPED_STENCILS))
def test_grouped_row_counts_and_gather_widths(ctx, mg, stencil, n):
    """a full last block, a one-row last block, partial last blocks; pairs as aggregates (every block a group of its own).  U = 4 (line), 7 (band,
    seven entries per row), 8 (nine-point; 27-point, whose blocks hold more than 1024 16-byte pieces and stage them with the loop).  Pattern
    code on and off (index slices), row ranges from the pattern lengths or from rowptr, staging by DMA or by loop, streaming stores: the flags
    word is the launcher's, the bits are the restatement's every time."""
    fn, u = GROUPED_STENCILS[stencil]
    rng = np.random.default_rng(1000 + n)
    c = Level(R.randomize(fn(n), rng), R.pairs(n), seed=n + 1)
    assert c.u == u
    nnz = np.diff(c.A.indptr[np.minimum(np.arange(0, n + RB, RB), n)])
    assert nnz.max() <= 5120 and (stencil != "27_point" or nnz.max() > 2 * 1024)      # every block fits the LDS budget; 27-point: over the DMA form's 1024 pieces
    groups, strays = predict_groups(c.agg, n)
    assert len(groups) == c.nblocks and len(strays) == 0
    code_serves = (c.tables > 0).sum() >= 0.5 * c.nblocks
    assert code_serves or stencil == "27_point", (stencil, n, c.tables)
    try:
        set_grouping(ctx)
        h = build(ctx, mg, c)
        first = None
        for opts in ({}, {"rowcode": 0}, {"rowptr_scan": 0}, {"stage_unroll": 0}, {"nt_store": 1}, {"rowcode": 0, "stage_unroll": 0, "nt_store": 1}):
            for k, v in opts.items():
                ctx.set_option(k, v)
            flags = (1 if opts.get("nt_store") else 0) | (2 if opts.get("stage_unroll", 1) else 0) | (4 if opts.get("rowptr_scan", 1) else 0)
            code = "auto" if opts.get("rowcode", 1) else "off"
            want = {"arm": GROUPED, "kernel": K_GROUP, "U": u, "flags": flags, "nodiag": True, "packed": code == "auto" and code_serves}
            if code == "off":
                want.update(blocks_coded=0)
            td, _, rcd, info, _ = run(ctx, mg, h, c, want, f"{stencil} n={n} {opts}", strays=strays, code=code)
            check_group_info(h, c, groups, strays, f"{stencil} n={n}")
            if first is None:
                first = (td, rcd)
            assert np.array_equal(td, first[0]) and np.array_equal(rcd, first[1])
            for k, v in DEFAULTS[:4]:
                ctx.set_option(k, v)
    finally:
        restore(ctx)


# ---- 2. grouped arm: group shapes by construction ----
def shape_pairs_256():
    """pairs {i, i + 256}: one group of two blocks; the second block's aggregate range is empty"""
    n = 512
    return n, np.r_[np.arange(256), np.arange(256)], 4, [[0, 1]], 0


def shape_chain():
    """links 0–1, 1–2, 2–3 with 128 aggregates each at n = 1024 + 77: one 4-block group and a single partial block"""
    n = 1024 + 77
    agg = np.full(n, -1, dtype=np.int64)
    nxt = 0
    for blk in range(3):                       # rows 128..255 of block blk... (block 0: rows 0..127) pair with rows 0..127 of block blk + 1
        lo = blk * RB + (128 if blk else 0)
        for j in range(128):
            agg[lo + j] = agg[(blk + 1) * RB + j] = nxt; nxt += 1
    rest = np.flatnonzero(agg < 0)             # the second half of blocks 0 and 3 and the partial block: in-block pairs
    for q in range(0, len(rest) - 1, 2):
        if rest[q] // RB == rest[q + 1] // RB:
            agg[rest[q]] = agg[rest[q + 1]] = nxt; nxt += 1
    return n, agg, 4, [[0, 1, 2, 3], [4]], 0


def shape_pairs_768():
    """pairs {i, i + 768}: the group's two blocks are not adjacent; the blocks between them keep in-block pairs"""
    n = 1024
    agg = np.r_[np.arange(256), 256 + np.arange(512) // 2, np.arange(256)]
    return n, agg, 4, [[0, 3], [1], [2]], 0


def shape_spread():
    """aggregates of 3–6 members spread over one 4-block group, one of them {first row of the first block, a middle row, last row of the fourth
    block}: the position delta 1023"""
    n = 1024
    rng = np.random.default_rng(77)
    agg = np.full(n, -1, dtype=np.int64)
    agg[[0, 500, 1023]] = 0
    rest = rng.permutation(np.setdiff1d(np.arange(n), [0, 500, 1023]))
    k, a = 0, 1
    while k < len(rest):
        s = int(rng.integers(3, 7))
        if len(rest) - k - s < 3:
            s = len(rest) - k if len(rest) - k <= 6 else 3
        agg[rest[k:k + s]] = a; a += 1; k += s
    sizes = np.bincount(agg)
    assert sizes.min() >= 3 and sizes.max() <= 6 and set(sizes.tolist()) == {3, 4, 5, 6}
    return n, agg, 4, [[0, 1, 2, 3]], 0


def shape_big_aggregates():
    """aggregates of 7 and 8 consecutive rows: strays by size, every one of them; every row stores r"""
    n = 1024
    sz = np.tile([7, 8], n // 15 + 1)
    agg = np.repeat(np.arange(len(sz)), sz)[:n]
    return n, agg, 4, None, int(agg.max())            # (the last aggregate is cut short at n: four members)


def shape_triples():
    """triples {i, i + 256, i + 512} under group_blocks = 2: only the first and the last block link, so every triple is a stray"""
    n = 768
    return n, np.r_[np.arange(256), np.arange(256), np.arange(256)], 2, [[0, 2], [1]], 256


def shape_unaggregated():
    """rows outside every aggregate: the first and the last row of a block, a whole block, and the rows behind the last aggregate"""
    n = 1024 + 50
    agg = np.full(n, -1, dtype=np.int64)
    nxt = 0
    for i in range(0, 1000, 2):
        if i // RB == 2 or i in (256, 510) or i + 1 in (256, 511):
            continue
        agg[i] = agg[i + 1] = nxt; nxt += 1
    agg[257] = agg[258]; agg[510] = agg[508]                   # rows 256 and 511 stay outside; their partners join the neighbouring pair
    assert agg[256] == -1 and agg[511] == -1 and np.all(agg[512:768] == -1) and np.all(agg[1000:] == -1) and agg[999] >= 0
    return n, agg, 4, [[0], [1], [2], [3], [4]], 0


SHAPES = {"pairs_256": shape_pairs_256, "chain": shape_chain, "pairs_768": shape_pairs_768, "spread": shape_spread, "big_aggregates": shape_big_aggregates,
          "triples": shape_triples, "unaggregated": shape_unaggregated}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_grouped_group_shapes(ctx, mg, shape):
    n, agg, gblocks, want_groups, want_strays = SHAPES[shape]()
    agg = Q.renumber_by_first_member(agg)
    rng = np.random.default_rng(len(shape))
    c = Level(R.randomize(R.stencil_5pt(n), rng), agg, seed=n + 7)
    groups, strays = predict_groups(c.agg, n, gblocks)
    if want_groups is not None:
        assert groups == want_groups, (shape, groups)
    assert len(strays) == want_strays, (shape, len(strays))
    try:
        set_grouping(ctx, gblocks)
        h = build(ctx, mg, c)
        td, rd, rcd, info, _ = run(ctx, mg, h, c, {"arm": GROUPED, "kernel": K_GROUP, "nodiag": True, "packed": True}, f"shape {shape}", strays=strays, code="auto")
        check_group_info(h, c, groups, strays, shape)
        if max(map(len, groups)) <= 2:         # the 512-thread pair kernel on the same groups: neither ND nor PK, the same bits
            ctx.set_option("group_concurrent", 1)
            t2, r2, rc2, _, _ = run(ctx, mg, h, c, {"arm": GROUPED, "kernel": K_PAIR, "nodiag": False, "packed": False, "flags": 0}, f"shape {shape}, pair kernel", strays=strays, code="auto")
            assert np.array_equal(t2, td) and np.array_equal(r2, rd) and np.array_equal(rc2, rcd)
    finally:
        restore(ctx)


# ---- 3. grouped arm: the three ways a row block reaches its entries ----
def staging_operator(rng):
    """64·256 + 37 five-point rows; block 10 holds rows of 40 entries (over any LDS budget: the unstaged walk), block 20 rows of three entries
    whose offsets differ from row to row (no pattern table pays: the index slice)"""
    n = 64 * RB + 37
    pat = R.stencil_5pt(n, 128).tolil()
    for i in range(10 * RB, 11 * RB):
        pat[i, rng.choice(n, 39, replace=False)] = 1.0
    for j, i in enumerate(range(20 * RB, 21 * RB)):
        pat[i, :] = 0.0
        pat[i, i - 2 - j] = 1.0; pat[i, i + 2 + j] = 1.0
    return n, pat.tocsr()


def test_grouped_staging_forms(ctx, mg):
    rng = np.random.default_rng(301)
    n, pat = staging_operator(rng)
    c = Level(R.randomize(pat, rng), R.pairs(n), seed=302)
    ln = np.diff(c.A.indptr)
    assert ln[10 * RB:11 * RB].min() >= 40 and c.max_len <= 64 and np.all(ln[20 * RB:21 * RB] == 3)
    groups, strays = predict_groups(c.agg, n)
    try:
        set_grouping(ctx)
        h = build(ctx, mg, c)
        _, _, _, info, _ = run(ctx, mg, h, c, {"arm": GROUPED, "kernel": K_GROUP, "blocks_coded": ">=1", "blocks_global": ">=1"}, "staging forms", strays=strays, code="auto")
        assert info["blocks_staged"] - info["blocks_coded"] >= 1, info                      # index slices
        nnz = np.diff(c.A.indptr[np.minimum(np.arange(0, n + RB, RB), n)])
        assert info["blocks_global"] == int((nnz > info["capv"]).sum()) == 1, (info, nnz.max())
        ctx.set_option("stage_unroll", 0)
        run(ctx, mg, h, c, {"arm": GROUPED, "kernel": K_GROUP, "blocks_global": 1}, "staging forms, loop staging", strays=strays, code="auto")
    finally:
        restore(ctx)


# ---- 4. grouped arm: value forms ----
def value_forms_operator(rng):
    """five blocks of five-point rows; block 1's rows scaled by 2⁰ … 2⁹ (its slice of Â spans more than 8 binades), block 2 holds a stored zero"""
    n = 4 * RB + 100
    A = R.randomize(R.stencil_5pt(n), rng).tocsr()
    f = np.ones(n); f[RB:2 * RB] = 2.0 ** (np.arange(RB) * 10 // RB)
    A = (sps.diags(f) @ A).tocsr(); A.sort_indices()
    i = 2 * RB + 17
    k = A.indptr[i] + int(np.flatnonzero(A.indices[A.indptr[i]:A.indptr[i + 1]] != i)[0])
    A.data[k] = 0.0
    return n, A


@pytest.mark.parametrize("pre_nodiag", [1, 0])
def test_grouped_value_forms(ctx, mg, pre_nodiag):
    """operand with and without its diagonal entries × packed and FP64 value streams, FP32 values, the pair kernel: every one of them returns the
    restatement's bits (and therefore each other's); the packed blocks are the ones tests/pack7_ref.py predicts"""
    rng = np.random.default_rng(401)
    n, A = value_forms_operator(rng)
    c = Level(A, Q.renumber_by_first_member(np.r_[np.arange(256), np.arange(256), 256 + np.arange(n - 512) // 2]), seed=402)
    assert len(c.A.data) == c.A.nnz and (c.A.data == 0.0).sum() == 1                        # the stored zero is still stored
    groups, strays = predict_groups(c.agg, n, 2)
    assert groups[0] == [0, 1] and len(strays) == 0
    hat = Q.hat_values(c.A, c.omega)
    offd = c.A.indices != np.repeat(np.arange(n), np.diff(c.A.indptr))
    e0 = P7.eligibility(hat[offd], P7.block_bounds(c.A.indptr, nd=True)) if pre_nodiag else P7.eligibility(hat, P7.block_bounds(c.A.indptr))
    assert list(e0 >= 0) == [True, False, False, True, True], e0
    try:
        set_grouping(ctx, 2)
        ctx.set_option("pre_nodiag", pre_nodiag)
        h = build(ctx, mg, c)
        nd = bool(pre_nodiag)
        t1, r1, rc1, _, _ = run(ctx, mg, h, c, {"arm": GROUPED, "kernel": K_GROUP, "nodiag": nd, "packed": True}, f"pre_nodiag={pre_nodiag} pack7=1", strays=strays)
        pi = h.pack_info(0)
        assert pi["pre_packed"] == int((e0 >= 0).sum()) == 3 and pi["pre_ran"] == 1 and pi["pre_source"] == (2 if nd else 1), pi
        ctx.set_option("pack7", 0)
        t0, r0, rc0, _, _ = run(ctx, mg, h, c, {"arm": GROUPED, "kernel": K_GROUP, "nodiag": nd, "packed": False}, f"pre_nodiag={pre_nodiag} pack7=0", strays=strays)
        assert h.pack_info(0)["pre_packed"] == 0 and h.pack_info(0)["pre_ran"] == 0
        ctx.set_option("pack7", 1)
        ctx.set_option("group_concurrent", 1)
        t2, r2, rc2, _, _ = run(ctx, mg, h, c, {"arm": GROUPED, "kernel": K_PAIR, "nodiag": False, "packed": False}, f"pre_nodiag={pre_nodiag} pair kernel", strays=strays)
        assert h.pack_info(0)["pre_ran"] == 0
        ctx.set_option("group_concurrent", 0)
        for t_, r_, rc_ in ((t0, r0, rc0), (t2, r2, rc2)):
            assert np.array_equal(t_, t1) and np.array_equal(r_, r1) and np.array_equal(rc_, rc1)
        h.set_operand_precision(32)
        assert h.operand_precision(0) == 32
        run(ctx, mg, h, c, {"arm": GROUPED, "kernel": K_GROUP, "nodiag": False, "packed": False}, f"pre_nodiag={pre_nodiag} FP32 values", f32=True, strays=strays)
    finally:
        restore(ctx)


# ---- 5. grouped arm: device-built hierarchies ----
@pytest.mark.parametrize("kind", ["poisson3d_33", "CSky3d30"])
def test_grouped_device_built_levels(ctx, mg, inputs, kind):
    """the project's own aggregation on its own operators, levels 0 and 1: the downloaded operator and level_P(l).agg() feed the restatement"""
    A = ctx.poisson3d(33) if kind == "poisson3d_33" else mg.Csr.from_mtx(ctx, inputs[kind])
    try:
        ctx.set_option("group_stray_pct", 60); ctx.set_option("group_min_blocks", 1)
        h = mg.Hierarchy(A, OMEGA, 1, 1).coarsen(10.0, 2, 8.0, 200, 32).finalize()
        assert h.nlev >= 3
        for l in (0, 1):
            rp, ci, v = h.level_A(l).download(); n = h.level_shape(l)[0]
            c = Level(sps.csr_matrix((v, ci, rp), shape=(n, n)), h.level_P(l).agg(), seed=500 + l)
            assert c.nc == h.level_shape(l + 1)[0] and c.max_len <= 64
            groups, strays = predict_groups(c.agg, n)
            _, _, _, info, _ = run(ctx, mg, h, c, {"arm": GROUPED, "kernel": K_GROUP}, f"{kind} level {l}", strays="device" if strays is None else strays, level=l)
            gi = h.group_info(l)
            assert gi["groups"] > 0 and gi["stray_aggregates"] == info["stray_aggregates"] and (groups is None or gi["groups"] == len(groups)), (gi, info)
    finally:
        restore(ctx)


# ---- 6. the three arms without groups ----
def ungrouped_levels():
    """(name, level, equal bits promised): row counts 3, 255, 257, 1100; row lengths 7, 8, 9, 16, 17 and 64; shuffled aggregates of 1–9 members (more
    than four: the second shuffle round of the aggregate-parallel kernel) with 5 % of the rows outside every aggregate"""
    out = []
    for n in (3, 255, 257, 1100):
        rng = np.random.default_rng(600 + n)
        agg = Q.aggregates_1_to_9(n, rng) if n > 3 else np.array([0, -1, 0], dtype=np.int32)
        out.append((f"lengths_{n}", Level(R.randomize(Q.with_row_lengths(n, (7, 8, 9, 16, 17, 64), rng), rng), agg, seed=601 + n), True))
    rng = np.random.default_rng(650)
    A, agg = R.unaggregated_case(1100, rng)
    out.append(("five_point_1100", Level(A, agg, seed=651), True))
    return out


def long_rows_level():
    """the long-row operator of tests/test_post_pass_ref_cpu.py (a band plus two dense rows and columns) with aggregates of 1–9 members"""
    rng = np.random.default_rng(660)
    n = 1200
    B = R.stencil_5pt(n).tolil()
    for q in (3, 700):
        js = rng.choice(n, 400, replace=False); B[q, js] = 1.0; B[js, q] = 1.0
    c = Level(R.randomize(B.tocsr(), rng), Q.aggregates_1_to_9(n, rng), seed=661)
    assert c.max_len > 64
    return c


UNGROUPED = ungrouped_levels()


@pytest.mark.parametrize("name,c,bits", UNGROUPED, ids=[u[0] for u in UNGROUPED])
def test_aggregate_parallel_arm(ctx, mg, name, c, bits):
    """fuse_restrict = 0 on a small level: agg_pre_kernel, FP64 and FP32 values"""
    assert (c.agg < 0).any() and (c.n < 100 or not name.startswith("lengths") or np.bincount(c.agg[c.agg >= 0]).max() >= 5)
    try:
        ctx.set_option("fuse_restrict", 0)
        h = build(ctx, mg, c)
        run(ctx, mg, h, c, {"arm": AGGPAR, "kernel": K_AGG, "U": 8, "blocks_coded": -1}, f"aggregate-parallel {name}", bits=bits)
        h.set_operand_precision(32)
        assert h.operand_precision(0) == 32
        run(ctx, mg, h, c, {"arm": AGGPAR, "kernel": K_AGG}, f"aggregate-parallel {name}, FP32 values", f32=True, bits=bits)
    finally:
        restore(ctx)


@pytest.mark.parametrize("name,c,bits", UNGROUPED, ids=[u[0] for u in UNGROUPED])
def test_residual_on_hat_arm(ctx, mg, name, c, bits):
    """aggpre_max_rows = 0 and fuse_restrict = 0: the residual kernel on Â (the coded kernel where a pattern code serves the operator, the slice
    kernel otherwise; the coded kernel's float form on an FP32 level) followed by restrict_agg_kernel"""
    try:
        ctx.set_option("fuse_restrict", 0); ctx.set_option("aggpre_max_rows", 0)
        h = build(ctx, mg, c)
        coded = name == "five_point_1100"
        run(ctx, mg, h, c, {"arm": RESIDUAL, "kernel": K_CODED if coded else K_SLICE, "U": c.u}, f"residual on Â {name}", bits=bits, code="auto" if coded else "off")
        if coded:
            ctx.set_option("rowcode", 0)
            run(ctx, mg, h, c, {"arm": RESIDUAL, "kernel": K_SLICE, "U": c.u, "blocks_coded": 0}, f"residual on Â {name}, slice kernel", bits=bits, code="off")
            ctx.set_option("rowcode", 1)
        h.set_operand_precision(32)
        assert h.operand_precision(0) == 32
        run(ctx, mg, h, c, {"arm": RESIDUAL, "kernel": K_CODED32}, f"residual on Â {name}, FP32 values", f32=True, bits=bits, code="any")
    finally:
        restore(ctx)


def test_residual_on_hat_arm_long_rows(ctx, mg):
    """rows of more than 64 entries: the slice kernel splits them among lanes and promises no order — the bars alone, on every row"""
    c = long_rows_level()
    try:
        ctx.set_option("fuse_restrict", 0); ctx.set_option("aggpre_max_rows", 0)
        h = build(ctx, mg, c)
        run(ctx, mg, h, c, {"arm": RESIDUAL, "kernel": K_SLICE}, "residual on Â, long rows", bits=False)
        ctx.set_option("aggpre_max_rows", 300000)          # long rows keep a small level off the aggregate-parallel kernel
        run(ctx, mg, h, c, {"arm": RESIDUAL, "kernel": K_SLICE}, "residual on Â, long rows, small-level option on", bits=False)
    finally:
        restore(ctx)


@pytest.mark.parametrize("name,c,bits", UNGROUPED, ids=[u[0] for u in UNGROUPED])
def test_gather_form_on_A(ctx, mg, name, c, bits):
    """fuse_operands = 0: FUSE_PRE of the gather kernel on A with wd, then restrict_agg_kernel; the products are a_ik·fl(wd_k·b_k)"""
    try:
        ctx.set_option("fuse_operands", 0)
        h = build(ctx, mg, c)
        run(ctx, mg, h, c, {"arm": GATHER, "kernel": K_GATHER, "U": 8, "flags": 0, "blocks_coded": 0}, f"gather form {name}", form="wd", bits=bits, code="off")
    finally:
        restore(ctx)


# ---- 7. refusals ----
def code_of(mg, fn):
    with pytest.raises(mg.MgsError) as e:
        fn()
    return e.value.code


def test_refusals(ctx, mg):
    INVALID, STATE = -1, -6
    rng = np.random.default_rng(711)
    n = 600
    c = Level(R.randomize(R.stencil_5pt(n), rng), R.pairs(n), seed=712)
    lib = mg.lib()
    try:
        h = mg.Hierarchy(upload(ctx, c.A), OMEGA, 1, 1)
        h.push_P(upload(ctx, R.agg_P(c.agg, c.nc))); h.push_P(upload(ctx, R.agg_P((np.arange(c.nc) * 8 // c.nc).astype(np.int32), 8)))
        b, t, r, rc = ctx.vec(c.b), ctx.vec(n), ctx.vec(n), ctx.vec(c.nc)
        assert code_of(mg, lambda: h.pre_pass_info(0, b, t, r, rc)) == STATE                      # before finalize
        h.finalize()
        assert h.pre_pass_info(0, b, t, r, rc)["arm"] == AGGPAR                                  # defaults on a small level
        out = (C.c_int64 * 16)()
        for args in ((None, 0, b.h, t.h, r.h, rc.h, out), (h.h, 0, None, t.h, r.h, rc.h, out), (h.h, 0, b.h, None, r.h, rc.h, out),
                     (h.h, 0, b.h, t.h, None, rc.h, out), (h.h, 0, b.h, t.h, r.h, None, out), (h.h, 0, b.h, t.h, r.h, rc.h, None)):
            assert lib.mgs_hier_pre_pass_info(*args) == INVALID                                   # NULL arguments
        assert code_of(mg, lambda: h.pre_pass_info(-1, b, t, r, rc)) == INVALID                  # level out of range
        assert code_of(mg, lambda: h.pre_pass_info(2, b, t, r, rc)) == INVALID                   # the coarsest level has no coarser one
        assert code_of(mg, lambda: h.pre_pass_info(0, ctx.vec(n - 1), t, r, rc)) == INVALID      # vectors too short
        assert code_of(mg, lambda: h.pre_pass_info(0, b, ctx.vec(n - 1), r, rc)) == INVALID
        assert code_of(mg, lambda: h.pre_pass_info(0, b, t, ctx.vec(n - 1), rc)) == INVALID
        assert code_of(mg, lambda: h.pre_pass_info(0, b, t, r, ctx.vec(c.nc - 1))) == INVALID
        h.set_smoother(OMEGA, 2, 1)
        assert code_of(mg, lambda: h.pre_pass_info(0, b, t, r, rc)) == STATE                      # V(2,1): no fused passes
        h.set_smoother(OMEGA, 1, 1)
        h.pre_pass_info(0, b, t, r, rc)
        # a general P
        N = 24; m = N * N; mc = m // 2
        i = np.arange(m)
        P = sps.coo_matrix((np.r_[np.ones(m), np.full(m, 0.25)], (np.r_[i, i], np.r_[i // 2, np.minimum(i // 2 + 1, mc - 1)])), shape=(m, mc)).tocsr()
        hg = mg.Hierarchy(ctx.poisson2d(N), OMEGA, 1, 1).push_P(upload(ctx, P)).finalize()
        assert not hg.level_P(0).is_aggregation
        assert code_of(mg, lambda: hg.pre_pass_info(0, ctx.vec(m), ctx.vec(m), ctx.vec(m), ctx.vec(mc))) == STATE
        # a value-coded level
        ctx.set_option("valcode", 1)
        hv = mg.Hierarchy(ctx.poisson3d(12), OMEGA, 1, 1).coarsen(10.0, 2, 8.0, 50, 8).finalize()
        m = 12 ** 3
        assert code_of(mg, lambda: hv.pre_pass_info(0, ctx.vec(m), ctx.vec(m), ctx.vec(m), ctx.vec(hv.level_shape(1)[0]))) == STATE
        ctx.set_option("valcode", 0)
        # a row shard: planes 4..11 of 16 with halo columns, aggregated and coarsened as a shard (no halo on the coarse level)
        As = ctx.poisson3d(16, 4, 12, local_cols=True)
        rows, cols = As.shape
        assert cols > rows
        T, Ac = C.c_void_p(), C.c_void_p()
        assert lib.mgs_aggregate_shard(As.h, 10.0, 1, 8.0, C.byref(T)) == 0
        hc = np.full(cols - rows, -1, dtype=np.int32)
        assert lib.mgs_galerkin_shard(As.h, T, hc.ctypes.data_as(C.POINTER(C.c_int)), 0, C.byref(Ac)) == 0
        hs = mg.Hierarchy(As, OMEGA, 1, 1)
        assert lib.mgs_hier_push_level(hs.h, T, Ac) == 0
        hs.finalize()
        assert code_of(mg, lambda: hs.pre_pass_info(0, ctx.vec(cols), ctx.vec(cols), ctx.vec(cols), ctx.vec(hs.level_shape(1)[0]))) == STATE
    finally:
        restore(ctx)
