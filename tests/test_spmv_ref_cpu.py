"""The host restatement of the operator kernels (tests/spmv_ref.py) pinned without a GPU: both summation orders stay inside the derived
bar of the exact sums (math.fsum over long-double products, and the long-double evaluation) on every fixture family of
tests/test_gpu_operator_kernels.py; the sequential order IS the oracle's spmv / residual / jacobi, bit for bit; the restated plan gives
hand-computed figures; the pipelined kernel's guard admits no row block it cannot stage (pairs_needed); every fixture has the properties
its GPU case relies on; and every planted defect changes bits on a fixture of the arm it belongs to."""
import math

import numpy as np
import pytest

import spmv_ref as R
from spmv_ref import RB


def fixtures():
    """(name, matrix, lanes of its lanes arm or None)"""
    out = [(f"edge_{n}", R.edge_case(n), None) for n in (1, 2, 63, 64, 65, 255, 256, 257, 511, 513)]
    out += [("wide", R.wide_case(), None)]
    out += [(f"gather_{u}", R.gather_case(u), None) for u in (4, 7, 8)] + [("gather_7_long", R.gather_case(7, True), None)]
    out += [("budget_seq", R.budget_case(40), None), ("budget_lanes", R.budget_case(40, 200), 4)]
    out += [("over_cap", R.over_cap_case(), 16), ("over_cap_long", R.over_cap_case(70), 16)]
    out += [(f"lanes_{L}", R.lanes_case(L), L) for L in (4, 8, 16, 32, 64)] + [("lanes_4_short", R.lanes_case(4, False), None)]
    out += [(f"chunk_{r}", R.chunk_case(r), None) for r in (1, 2, 3)]
    out += [(f"wave_{n}", R.wave_case(n), None) for n in (70, 256, 700)] + [("wave_over", R.wave_over_case(), None)]
    out += [(f"pipe_{n}", R.pipe_case(n), None) for n in (200, 1024, 1100, 1900)]
    out += [(f"pipe_{c}_{'odd' if o else 'even'}", R.pipe_boundary_case(c, o), None) for c in (2047, 2048) for o in (0, 1)]
    return out


FIXTURES = fixtures()
IDS = [f[0] for f in FIXTURES]
BY_NAME = {f[0]: f[1] for f in FIXTURES}


def csr(M):
    return M.indptr, M.indices, M.data


# ---- 1. both orders inside the bar of the exact sums ----
@pytest.mark.parametrize("name,M,L", FIXTURES, ids=IDS)
def test_both_orders_stay_inside_the_bar(name, M, L):
    assert M.has_sorted_indices and np.all(np.abs(M.data) >= 0.5) and np.all(np.abs(M.data) <= 2.0)
    x, b, dinv, omega = R.vectors(M, 11)
    rp, col, val = csr(M)
    n = M.shape[0]
    # the exact sums twice: long double, and math.fsum over the long-double products (fsum takes Python floats: hi + lo halves)
    ex, _ = R.exact("spmv", rp, col, val, x)
    p = val.astype(np.longdouble) * x.astype(np.longdouble)[col]
    hi = p.astype(np.float64); lo = (p - hi).astype(np.float64)
    fs = np.array([math.fsum(np.r_[hi[rp[i]:rp[i + 1]], lo[rp[i]:rp[i + 1]]]) for i in range(n)])
    bs = R.bar("spmv", rp, col, val, x)
    # the two exact values agree to fsum's one final rounding to FP64 and 2⁻¹⁰ of the bar
    assert np.all(np.abs(fs.astype(np.longdouble) - ex) <= np.longdouble(R.U) * np.abs(ex) + bs / 1024), name
    worst = 0.0
    sums = [R.row_sums_sequential(rp, col, val, x)] + [R.row_sums_lanes(rp, col, val, x, q) for q in ({L} if L else {4, 64})]
    for s in sums:
        for op in R.OPS:
            got = R.apply(op, s, x, b, dinv, omega)
            want, _ = R.exact(op, rp, col, val, x, b, dinv, omega)
            q = R.ratios(got, want, R.bar(op, rp, col, val, x, b, dinv, omega))
            worst = max(worst, float(q.max(initial=0.0)))
            assert q.max(initial=0.0) <= 1.0, (name, op, float(q.max()), int(q.argmax()))
    print(f"{name}: largest error/bar {worst:.3f}")


def test_signed_zeros_and_empty_rows_inside_the_bar():
    """the two families whose values are not all in ±[0.5, 2]: a row of zeros has a bar of 0 and an error of 0"""
    Z, vecs, negrows = R.signed_zero_case()
    E = R.empty_rows_case()
    assert np.all(R.bar("spmv", *csr(Z), vecs[0])[negrows] == 0)
    for name, M, (x, b, dinv, omega) in (("signed zeros", Z, vecs), ("no entries", E, R.vectors(E, 11))):
        rp, col, val = csr(M)
        for s in (R.row_sums_sequential(rp, col, val, x), R.row_sums_lanes(rp, col, val, x, 8)):
            assert not np.signbit(s[s == 0]).any()
            for op in R.OPS:
                q = R.ratios(R.apply(op, s, x, b, dinv, omega), R.exact(op, rp, col, val, x, b, dinv, omega)[0], R.bar(op, rp, col, val, x, b, dinv, omega))
                assert q.max() <= 1.0, (name, op, float(q.max()))
    s = R.row_sums_sequential(*csr(E), x)
    assert np.array_equal(R.apply("residual", s, x, b), b) and np.array_equal(R.apply("jacobi", s, x, b, dinv, omega), x + (omega * dinv) * b)


def test_bar_rejects_what_it_must():
    """a dropped entry moves a row by at least 0.25: twelve orders of magnitude outside the bar, in every non-empty row"""
    M = BY_NAME["gather_8"]; rp, col, val = csr(M)
    x, b, dinv, omega = R.vectors(M, 11)
    ex, _ = R.exact("spmv", rp, col, val, x)
    s = R.row_sums_sequential(rp, col, val, x)
    lens = np.diff(rp)
    s_drop = s.copy(); rows = np.flatnonzero(lens > 0)
    s_drop[rows] -= (val * x[col])[rp[rows + 1] - 1]
    q = R.ratios(s_drop, ex, R.bar("spmv", rp, col, val, x))
    assert np.all(q[rows] > 1e12)


# ---- 2. the sequential order is the oracle's ----
@pytest.mark.parametrize("name", ["edge_257", "gather_4", "gather_7", "gather_8", "budget_lanes", "over_cap_long", "lanes_64", "chunk_3", "wave_700"])
def test_sequential_order_is_the_oracles(orc, name):
    M = BY_NAME[name]; rp, col, val = csr(M)
    x, b, dinv, omega = R.vectors(M, 12)
    A = orc.Csr.from_arrays(M.shape[0], M.shape[1], rp, col, val)
    s = R.row_sums_sequential(rp, col, val, x)
    assert np.array_equal(s, A.spmv(x))
    assert np.array_equal(R.apply("residual", s, x, b), A.residual(x, b))
    assert np.array_equal(R.apply("jacobi", s, x, b, dinv, omega), A.jacobi(dinv[:M.shape[0]], omega, b[:M.shape[0]], x))


# ---- 3. the plan against figures worked out by hand ----
def test_plan_small_matrix_by_hand():
    """3 × 5 with halo columns: rows (0, 4), (1), (0, 2, 3): one row block of 6 entries, longest row 3; far distances: row 0: first column
    0 → 0, last owned column (< 3) is 0 → 0; row 1: 0; row 2: first column 0 → 2, last owned 2 → 0: far_band = (0 + 0 + 2) // 3 = 0;
    lds_cap = max(64, 6) = 64 → (64 + 2)·12 + 16 = 808 bytes; the only block reads halo columns: halo_lo_blocks = 1, no split"""
    p = R.plan([0, 2, 3, 6], [0, 4, 1, 0, 2, 3], 3, 5)
    assert R.plan_info(p) == dict(max_block_nnz=6, max_row_len=3, far_band=0, lds_bytes=808, halo_lo_blocks=1, halo_hi_blocks=0,
                                  halo_split_ok=0, has_long_row_blocks=0)
    assert p["lds_cap"] == 64 and p["max_wave_nnz"] == 6 and p["nblocks"] == 1 and R.lanes_of(p) == 4
    assert R.arm(p, 0, 0) == "staged" and R.arm(p, 0, 1) == "sequential" and R.arm(p, 0, 7) == "wave"
    assert R.arm(p, 0, 6) == "staged"            # max_block_nnz 6 != lds_cap 64: no pipe
    # far band by hand on a 4 × 4 matrix: rows (0, 3), (1), (1, 2), (0, 3): distances 3, 0, 1, 3 → 7 // 4 = 1
    q = R.plan([0, 2, 3, 5, 7], [0, 3, 1, 1, 2, 0, 3], 4, 4)
    assert q["far_band"] == 1 and q["halo_lo_blocks"] == 0 and q["max_row_len"] == 2
    # 600 × 700, row block 0 without halo columns, blocks 1 and 2 with: no leading halo block, two trailing ones, a clean split
    W = R.wide_case()
    assert W.indices[:W.indptr[RB]].max() < 600 and all(W.indices[W.indptr[k * RB]:W.indptr[min((k + 1) * RB, 600)]].max() >= 600 for k in (1, 2))
    w = R.plan_of(W)
    assert (w["halo_lo_blocks"], w["halo_hi_blocks"], w["halo_split_ok"]) == (0, 2, 1)


def test_plan_budget_step_lowers_the_cap():
    """68 row blocks of 3·256 = 768 entries, block 34 with 40·256 = 10240: nnz = 61696, mean per block 907.29…; the cap starts at
    min(10240, 5120) = 5120 > 1.12·mean; first candidate (int)(1.06·907.29) + 8 = 961 + 8 = 969 < 5120 leaves one block over it,
    and 1 ≤ 0.015·68 = 1.02: lds_cap = 969, (969 + 2)·12 + 16 = 11668 bytes"""
    M = R.budget_case(40)
    p = R.plan_of(M)
    assert p["nnz"] == 61696 and p["nblocks"] == 68 and p["max_block_nnz"] == 10240 and p["max_row_len"] == 40
    assert p["lds_cap"] == 969 and p["lds_bytes"] == 11668 and p["has_long_row_blocks"] == 1 and p["max_wave_nnz"] == 2560
    assert [R.arm(p, k, 0) for k in (0, 33, 34, 35, 67)] == ["staged", "staged", "sequential", "staged", "staged"]
    assert [R.arm(p, k, 3) for k in (0, 34)] == ["staged", "lanes(4)"]
    pl = R.plan_of(R.budget_case(40, 200))          # 160 entries more: mean 909.64…, (int)(1.06·909.64) + 8 = 964 + 8
    assert pl["max_row_len"] == 200 and pl["lds_cap"] == 972 and R.arm(pl, 34, 0) == "lanes(4)" and R.arm(pl, 33, 0) == "staged"


def test_plan_budget_step_must_not_lower_at_64_blocks():
    """exactly 64 row blocks, one heavy: every candidate leaves one block over it, and 1 > 0.015·64 = 0.96: the cap stays at the heavy
    block's count.  63·768 + 2560 = 50944 entries, mean 796; 2560 > 1.12·796, so the step does run — and finds nothing"""
    lengths = np.full(64 * RB, 3); lengths[5 * RB:6 * RB] = 10
    M = R.banded(lengths, 64 * RB, np.random.default_rng(1), "stencil")
    p = R.plan_of(M)
    assert p["nblocks"] == 64 and p["nnz"] == 50944 and p["max_block_nnz"] == 2560
    assert p["lds_cap"] == 2560 and p["lds_bytes"] == 2562 * 12 + 16 and p["has_long_row_blocks"] == 0
    # one more block of three per row: 65 blocks, 0.015·65 = 0.975 < 1 still; at 67 blocks 1.005 ≥ 1 and the cap drops
    for nb, lowered in ((65, False), (67, True)):
        lengths = np.full(nb * RB, 3); lengths[5 * RB:6 * RB] = 10
        q = R.plan_of(R.banded(lengths, nb * RB, np.random.default_rng(1), "stencil"))
        assert (q["lds_cap"] < 2560) == lowered, (nb, q["lds_cap"])
    # no entries at all: max(64, 0) = 64; two blocks: no step
    e = R.plan_of(R.empty_rows_case())
    assert e["lds_cap"] == 64 and e["max_block_nnz"] == 0 and e["lds_bytes"] == 808 and R.arm(e, 1, 0) == "staged"
    z = R.plan([0], [], 0, 5)
    assert R.plan_info(z) == dict(max_block_nnz=0, max_row_len=0, far_band=0, lds_bytes=40, halo_lo_blocks=0, halo_hi_blocks=0,
                                  halo_split_ok=0, has_long_row_blocks=0)


def test_gather_width_and_lanes():
    assert [R.gather_width(m, x) for m, x in ((4.5, 99), (4.51, 14), (7.5, 14), (7.5, 15), (7.51, 7), (3.0, 5))] == [4, 7, 7, 8, 8, 4]
    for u in (4, 7, 8):
        assert R.gather_width_of(R.plan_of(R.gather_case(u))) == u
    p7, p7l = R.plan_of(R.gather_case(7)), R.plan_of(R.gather_case(7, True))
    assert p7["max_row_len"] == 14 and p7l["max_row_len"] == 15 and R.gather_width_of(p7l) == 8
    for L in (4, 8, 16, 32, 64):
        p = R.plan_of(R.lanes_case(L))
        assert R.lanes_of(p) == L and p["max_row_len"] >= 65 and [R.arm(p, k, 1) for k in range(3)] == [f"lanes({L})"] * 3
    ps = R.plan_of(R.lanes_case(4, False))
    assert ps["max_row_len"] <= 64 and [R.arm(ps, k, 1) for k in range(3)] == ["sequential"] * 3


# ---- 4. the pipelined kernel's guard: does it admit a block it cannot stage? ----
def test_pipe_guard_pairs_needed():
    """pen and paper: a block of cnt entries from lo needs (cnt + (lo & 1) + 1) >> 1 pairs"""
    assert [R.pairs_needed(lo, lo + cnt) for cnt in (2047, 2048) for lo in (1280, 1281)] == [1024, 1024, 1024, 1025]
    for cnt in range(0, 2050):
        for lo in (0, 1, 6, 7):
            assert R.pairs_needed(lo, lo + cnt) == (cnt + (lo & 1) + 1) >> 1
            assert (R.pairs_needed(lo, lo + cnt) <= R.PIPE_PAIRS) == (cnt <= 2047 or (cnt == 2048 and lo % 2 == 0))
    # the guard as it was (≤ 2048) admitted the 2048-entry block at an odd lo; as it is (≤ 2047) every admitted block stages fully
    odd, even = R.pipe_boundary_case(2048, 1), R.pipe_boundary_case(2048, 0)
    po = R.plan_of(odd)
    assert R.pipe_admitted(po, bound=2048) and R.pairs_needed(int(odd.indptr[RB]), int(odd.indptr[2 * RB])) == 1025 > R.PIPE_PAIRS
    assert not R.pipe_admitted(po) and R.kernel(po, 6) == "slice" and R.arm(po, 1, 6) == "staged"
    assert R.kernel(R.plan_of(even), 6) == "slice"
    for M in [f[1] for f in FIXTURES]:
        p = R.plan_of(M)
        if R.pipe_admitted(p):
            worst = max(R.pairs_needed(int(p["block_lo"][k]), int(p["block_lo"][k + 1])) for k in range(p["nblocks"]))
            assert worst <= R.PIPE_PAIRS
    for o in (0, 1):
        M = R.pipe_boundary_case(2047, o); p = R.plan_of(M)
        assert R.kernel(p, 6) == "pipe" and R.pairs_needed(int(M.indptr[RB]), int(M.indptr[2 * RB])) == 1024 and M.indptr[RB] % 2 == o


# ---- 5. the fixtures have what their GPU cases rely on ----
def test_fixture_properties():
    for u in (4, 7, 8):
        M = R.gather_case(u); n = M.shape[0]; lens = np.diff(M.indptr)
        cyc = set(R.GATHER_CYCLE[u])
        assert cyc <= set(lens.tolist()) and M.indptr[RB] % 2 == 1 and lens[-1] % u != 0 and lens[-1] > 0
        cnt = np.bincount(M.indices, minlength=n)
        assert cnt[n - 2] == 1 and cnt[n - 1] == 1
        # the lonely entries are gathered by the padded last step of another row of their row block (poisoned neighbours)
        for r, c in zip(R.LONELY_ROWS, (n - 2, n - 1)):
            k = int(M.indptr[r + 1]) - 1
            assert M.indices[k] == c
            if u != 8:
                continue
            readers = [i for i in range(r - 3, r) if lens[i] % u and M.indptr[i + 1] <= k < M.indptr[i] + (lens[i] + u - 1) // u * u and i // RB == r // RB]
            assert readers, (u, r)
    M, (x, b, dinv, omega), negrows = R.signed_zero_case()
    prod = M.data * x[M.indices]
    assert len(negrows) > 50 and np.signbit(M.data).any() and np.signbit(x[x == 0]).any() and (x == 0).sum() > 20
    for r in negrows[:40]:
        pr = prod[M.indptr[r]:M.indptr[r + 1]]
        assert np.all(pr == 0) and np.all(np.signbit(pr))
    s = R.row_sums_sequential(M.indptr, M.indices, M.data, x)
    assert not np.signbit(s[negrows]).any() and np.all(s[negrows] == 0)          # a sum that starts at +0.0 is never −0.0
    for r in (1, 2, 3):
        R.chunk_case(r)                                                             # asserts its offsets itself
    for n in (70, 256, 700):
        M = R.wave_case(n); p = R.plan_of(M)
        assert R.kernel(p, 7) == "wave" and (n < 192 or M.indptr[192] == M.indptr[128])
    p = R.plan_of(R.wave_over_case())
    assert p["max_wave_nnz"] == 4160 and p["max_block_nnz"] <= p["lds_cap"] and R.kernel(p, 7) == "slice" and R.arm(p, 0, 7) == "staged"
    assert [R.plan_of(R.pipe_case(n))["nblocks"] for n in (200, 1024, 1100, 1900)] == [1, 4, 5, 8]
    assert all(R.kernel(R.plan_of(R.pipe_case(n)), 6) == "pipe" for n in (200, 1024, 1100, 1900))
    flat = R.plan_of(R.budget_case(0))
    assert R.kernel(flat, 6) == "pipe" and R.kernel(flat, 7) == "wave" and flat["lds_cap"] == 768
    low = R.plan_of(R.budget_case(7))
    assert low["max_block_nnz"] == 1792 and low["lds_cap"] < 1792 and R.kernel(low, 6) == "slice" and R.arm(low, R.BUDGET_HEAVY, 6) == "sequential"
    for twin, want in ((0, "sequential"), (70, "lanes(16)")):
        p = R.plan_of(R.over_cap_case(twin))
        assert p["lds_cap"] == 5120 and [R.arm(p, k, 0) for k in (0, 1)] == ["staged", want]
        assert [R.arm(p, 1, v) for v in (2, 3, 4)] == ["lanes(16)"] * 3               # variants 2–4: no sequential walk
    # the pattern code: the stencil fixtures are coded, the random ones are not
    for M, usable in ((R.budget_case(40), True), (R.gather_case(8), True), (R.gather_case(4), True), (R.gather_case(7), True),
                      (R.edge_case(513), False)):
        nc = R.coded_blocks(M.indptr, M.indices, M.shape[0])
        assert R.code_usable(R.plan_of(M), nc) == usable, (nc, M.shape)


# ---- 6. planted defects: every one changes bits on a fixture of its arm ----
def changed(a, b):
    return int((a.view(np.int64) != b.view(np.int64)).sum())


SEQ_FIXTURES = ["edge_65", "gather_4", "gather_7", "gather_8", "budget_seq", "over_cap", "lanes_4_short", "chunk_2", "wave_700", "pipe_1100", "pipe_2047_odd"]
LANES_FIXTURES = [("budget_lanes", 4), ("over_cap_long", 16)] + [(f"lanes_{L}", L) for L in (4, 8, 16, 32, 64)]


def drop(M, which):
    """M without the first (0) or last (−1) entry of every non-empty row"""
    lens = np.diff(M.indptr); keep = np.ones(M.nnz, dtype=bool)
    rows = np.flatnonzero(lens > 0)
    keep[M.indptr[rows] if which == 0 else M.indptr[rows + 1] - 1] = False
    rp = np.r_[0, np.cumsum(lens - (lens > 0))]
    return rp, M.indices[keep], M.data[keep]


@pytest.mark.parametrize("name", SEQ_FIXTURES)
def test_planted_defects_sequential(name):
    M = BY_NAME[name]; rp, col, val = csr(M); n = M.shape[0]
    x, b, dinv, omega = R.vectors(M, 13)
    s = R.row_sums_sequential(rp, col, val, x)
    lens = np.diff(rp)
    for which in (0, -1):                                                 # first / last entry dropped: every non-empty row
        sd = R.row_sums_sequential(*drop(M, which), x)
        assert np.all((sd != s)[lens > 0]), (name, which)
    # descending order: entries of every row reversed
    rows = np.repeat(np.arange(n), lens); pos = np.arange(M.nnz) - rp[rows]
    rev = rp[rows] + lens[rows] - 1 - pos
    sr = R.row_sums_sequential(rp, col[rev], val[rev], x)
    assert changed(sr, s) > 0.15 * (lens >= 3).sum() > 0, (name, changed(sr, s))
    # the neighbour row's range
    nb = np.r_[s[1:], 0.0]
    assert np.all((nb != s)[:-1][(lens[:-1] > 0) | (lens[1:] > 0)]), name
    # (ω·dinv)·(b − s) re-associated
    good = R.apply("jacobi", s, x, b, dinv, omega)
    bad = x[:n] + omega * (dinv[:n] * (b[:n] - s))
    assert changed(good, bad) > 0.05 * n, (name, changed(good, bad))


@pytest.mark.parametrize("name,L", LANES_FIXTURES)
def test_planted_defects_lanes(name, L):
    M = BY_NAME[name]; rp, col, val = csr(M)
    x, b, dinv, omega = R.vectors(M, 14)
    p = R.plan_of(M)
    variant = 1 if name.startswith("lanes_") else 0
    blocks = [k for k in range(p["nblocks"]) if R.arm(p, k, variant) == f"lanes({L})"]
    assert blocks and R.lanes_of(p) == L
    rows = np.concatenate([np.arange(k * RB, min((k + 1) * RB, M.shape[0])) for k in blocks])
    lens = np.diff(rp)[rows]
    sl = R.row_sums_lanes(rp, col, val, x, L)[rows]
    # the lanes order replaced by the sequential order: rows of three and more entries are the ones that can differ
    ss = R.row_sums_sequential(rp, col, val, x)[rows]
    assert changed(sl, ss) > 0.1 * (lens >= 3).sum() > 0, (name, changed(sl, ss))
    assert np.array_equal(sl[lens <= 2], ss[lens <= 2])
    # the tree run with off ascending: rows that fill more than two lanes
    asc = [1 << q for q in range(L.bit_length() - 1)]
    st = R.row_sums_lanes(rp, col, val, x, L, offsets=asc)[rows]
    assert changed(sl, st) > 0.1 * (lens >= 3).sum(), (name, changed(sl, st))
    # a wrong L is another order too
    so = R.row_sums_lanes(rp, col, val, x, 8 if L == 4 else L // 2)[rows]
    assert changed(sl, so) > 0, name
    # dropped entries, within the lanes order
    for which in (0, -1):
        sd = R.row_sums_lanes(*drop(M, which), x, L)[rows]
        assert np.all((sd != sl)[lens > 0]), (name, which)
    # row_sums puts the lanes order on exactly the blocks of that arm
    mix = R.row_sums(p, variant, rp, col, val, x)
    assert np.array_equal(mix[rows], sl)
    other = np.setdiff1d(np.arange(M.shape[0]), rows)
    assert np.array_equal(mix[other], R.row_sums_sequential(rp, col, val, x)[other])
