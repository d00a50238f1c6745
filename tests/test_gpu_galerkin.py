"""The aggregation Galerkin product on the device — galerkin_lds_kernel's count and fill pass, galerkin_numeric_kernel, the member
lists, the extended column map and the scan around them (multigridsolver_amd/csrc/setup_agmg.hip) — held BIT FOR BIT to the host
restatement of its documented order (tests/galerkin_ref.py): members ascending, entries in storage order, the first entry of a
coarse column stored and later ones added.  No tolerance anywhere in this file.  tests/test_galerkin_ref_cpu.py shows that every
fixture used here tells that order from its reverses and from the oracle's (Pᵀ·A)·P; which instantiation, arm or edge a case
reaches is asserted from the case's own figures."""
import ctypes as C
import time

import numpy as np
import pytest
import scipy.sparse as sps

import galerkin_ref as ref

pytestmark = pytest.mark.gpu

OK, INVALID = 0, -1
_cases, _restated = {}, {}


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


def case_of(name):
    if name not in _cases:
        _cases[name] = ref.FAMILIES[name]()
    return _cases[name]


def restated(name, values="v", ap=False):
    """computed once per (case, values, form) and shared"""
    key = (name, values, ap)
    if key not in _restated:
        _restated[key] = ref.restate(case_of(name), values, ap)
    return _restated[key]


def upload(ctx, case, values="v"):
    return ctx.csr(case["n"], case["cols"], case["rp"], case["ci"], case[values])


def int_ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def xfer_from_agg(mg, ctx, agg, nc):
    """(status, Xfer) of mgs_xfer_from_agg"""
    agg = np.ascontiguousarray(agg, dtype=np.int32)
    T = C.c_void_p()
    rc = mg.lib().mgs_xfer_from_agg(ctx.h, len(agg), nc, int_ptr(agg), C.byref(T))
    return rc, (mg.Xfer(ctx, T) if rc == OK else None)


def assert_equals(M, want, what=""):
    """rowptr (its last entry, the sentinel lane's, included), columns and the values' bits"""
    rp, ci, v = M.download()
    assert np.array_equal(rp, want[0]), what
    assert rp[-1] == want[0][-1] == len(want[1]), what
    assert np.array_equal(ci, want[1]), what
    bad = np.flatnonzero(v.view(np.int64) != want[2].view(np.int64))
    assert ref.same_bits(v, want[2]), (what, len(bad), bad[:5], v[bad[:5]], want[2][bad[:5]], want[3][bad[:5]])
    return rp, ci, v


def galerkin_of(mg, ctx, name):
    case = case_of(name)
    rc, T = xfer_from_agg(mg, ctx, case["agg"], case["nc"])
    assert rc == OK
    assert np.array_equal(T.agg(), case["agg"]) and T.shape == (case["n"], case["nc"])
    return case, upload(ctx, case).galerkin(T)


# ------------------------------------------------------------------ the stand-alone product
@pytest.mark.parametrize("M,nc", ref.MAXUB_CASES)
def test_instantiation_choice_and_workgroup_edges(ctx, mg, M, nc):
    """the longest gathered row is exactly 16, 17, 32, 33, 64: <16,256>, <32,128>, <64,64> at both ends of their range; nc = TBK − 1,
    TBK, TBK + 1, 2·TBK: the count pass's sentinel lane c == nc is the last lane of a workgroup, the first lane of a workgroup of
    its own, or in the middle"""
    name = f"maxub{M}_nc{nc}"
    case, Ac = galerkin_of(mg, ctx, name)
    cap, tbk = ref.slots_of(M)
    assert ref.maxub(case) == M and case["nc"] == nc
    assert (cap, tbk) == {16: (16, 256), 17: (32, 128), 32: (32, 128), 33: (64, 64), 64: (64, 64)}[M]
    assert nc % tbk in (tbk - 1, 0, 1)
    assert Ac.shape == (nc, nc)
    rp, _, _ = assert_equals(Ac, restated(name), name)
    assert np.diff(rp).max() <= M


def test_spill_past_64_columns(ctx, mg):
    """coarse rows of 63, 64, 65, 65, 66, 65 and about 480 distinct columns in the 64-slot kernel: the count pass's re-walk and the
    fill pass's global segment, with the 65th column last, in front, and in the middle with duplicates of held columns after it"""
    case, Ac = galerkin_of(mg, ctx, "spill")
    assert ref.slots_of(ref.maxub(case)) == (64, 64)
    rp, _, _ = assert_equals(Ac, restated("spill"), "spill")
    lens = np.diff(rp)
    assert lens[10:16].tolist() == [63, 64, 65, 65, 66, 65] and lens[16] > 400
    assert (lens > 64).sum() == 5


def test_columns_outside_every_aggregate(ctx, mg):
    """5 % G0 columns, a member row of G0 entries only, a coarse row that comes out empty, empty member rows, and two aggregate ids
    without a member (mgs_xfer_from_agg takes them: an empty member list, an empty coarse row)"""
    case, Ac = galerkin_of(mg, ctx, "g0")
    rp, _, _ = assert_equals(Ac, restated("g0"), "g0")
    for c in case["no_member"] + [case["empty_result"]]:
        assert rp[c + 1] == rp[c]
    assert (case["agg"] < 0).sum() >= 20
    # an id outside [−1, nc) is refused
    bad = case["agg"].copy(); bad[3] = case["nc"]
    assert xfer_from_agg(mg, ctx, bad, case["nc"])[0] == INVALID
    bad[3] = -2
    assert xfer_from_agg(mg, ctx, bad, case["nc"])[0] == INVALID


def test_aggregates_of_1_2_3_8_16_shuffled(ctx, mg):
    case, Ac = galerkin_of(mg, ctx, "sizes")
    assert sorted(set(np.bincount(case["agg"]).tolist())) == [1, 2, 3, 8, 16]
    assert ref.slots_of(ref.maxub(case)) == (64, 64)
    assert_equals(Ac, restated("sizes"), "sizes")


def test_signed_zeros_are_stored_with_their_signs(ctx, mg):
    """a lone −0.0 stays −0.0, +0.0 then −0.0 gives +0.0, an exact cancellation is stored as +0.0"""
    case, Ac = galerkin_of(mg, ctx, "zeros")
    rp, ci, v = assert_equals(Ac, restated("zeros"), "zeros")
    assert rp.tolist() == [0, 2, 4, 7]
    assert ref.same_bits(v[:4], case["expect_head"]) and np.signbit(v[0]) and not np.signbit(v[1]) and not np.signbit(v[2])


# ------------------------------------------------------------------ the row shard
def shard_product(mg, ctx, case, halo_map, nhc):
    rc, T = xfer_from_agg(mg, ctx, case["agg"], case["nc"])
    assert rc == OK
    A = upload(ctx, case)
    hm = np.ascontiguousarray(halo_map, dtype=np.int32)
    Ac = C.c_void_p()
    rc = mg.lib().mgs_galerkin_shard(A.h, T.h, int_ptr(hm), nhc, C.byref(Ac))
    return rc, (mg.Csr(ctx, Ac) if rc == OK else None)


def test_row_shard_with_a_coarse_halo_map(ctx, mg):
    """mgs_galerkin_shard on a 600 × 660 upload: the extended column map is agg followed by the halo map (−1 slots, two slots on one
    coarse halo column, more coarse halo columns than are used); one process, no communicator"""
    case = case_of("shard")
    n, nc, nhc = case["n"], case["nc"], case["n_halo_coarse"]
    assert case["cols"] > n and len(np.unique(case["halo_map"][case["halo_map"] >= 0])) < nhc
    rc, Ac = shard_product(mg, ctx, case, case["halo_map"], nhc)
    assert rc == OK and Ac.shape == (nc, nc + nhc)
    rp, ci, _ = assert_equals(Ac, restated("shard"), "shard")
    assert (ci >= nc).sum() > 100
    # a halo column outside [nc, nc + n_halo_coarse), or an owned one, is refused
    for slot, value in ((7, nc + nhc), (7, nc - 1), (59, -2)):
        hm = case["halo_map"].copy(); hm[slot] = value
        assert shard_product(mg, ctx, case, hm, nhc)[0] == INVALID, (slot, value)


# ------------------------------------------------------------------ A·P, and the refresh of both products
def agg_P(ctx, agg, nc):
    P = sps.csr_matrix((np.ones(len(agg)), (np.arange(len(agg)), agg)), shape=(len(agg), nc))
    return ctx.csr(P.shape[0], P.shape[1], P.indptr, P.indices, P.data)


def two_level(ctx, mg, case, values):
    A = upload(ctx, case, values)
    h = mg.Hierarchy(A, 0.6, 1, 1).push_P(agg_P(ctx, case["agg"], case["nc"])).finalize()
    assert h.nlev == 2
    return A, h


@pytest.mark.parametrize("L", ref.HIER_L)
def test_AP_and_refresh_on_every_arm(ctx, mg, L):
    """Hierarchy(A).push_P(P): A_c from the fill pass and, after the first cycle, A·P (identity member lists) equal the restatement;
    after update_values(v2) and refresh() both equal the restatement on v2 and a twin built from scratch.  The longest row of A_c
    and of A·P is L: galerkin_numeric_kernel<8,256> (L = 8), <16,256> (9, 16), <32,128> (17, 32), <64,64> (33, 64) and its
    global-accumulator arm (80).  Fine rows of 1, 7, 8, 9, 15, 16, 17 entries end the eight-entry look-ahead at every tail."""
    name = f"hier{L}"
    case = case_of(name)
    n, nc = case["n"], case["nc"]
    cap, tbk = ref.numeric_slots_of(L)
    assert nc > tbk and nc % tbk != 0 and n % tbk != 0
    assert {1, 7, 8, 9, 15, 16, 17} <= set(np.diff(case["rp"]).tolist())
    A, h = two_level(ctx, mg, case, "v")
    assert h.level_AP(0) is None                                     # not built before the first cycle
    b = ctx.vec(n).rand(seed=L)
    x1 = h.vcycle(b).numpy()
    assert np.isfinite(x1).all()
    for l in (-1, 1, 2):
        assert h.level_AP(l) is None                                 # out of range, and the coarsest level has no A·P
    rp, _, _ = assert_equals(h.level_A(1), restated(name), "A_c")
    assert np.diff(rp).max() == L and ((np.diff(rp) > 64).any() == (L > 64))
    AP = h.level_AP(0)
    assert AP.shape == (n, nc)
    rp, _, _ = assert_equals(AP, restated(name, "v", True), "A·P")
    assert np.diff(rp).max() == L and ((np.diff(rp) > 64).any() == (L > 64))
    # new values on the same pattern
    A.update_values(case["v2"]); h.refresh()
    info = h.refresh_info()
    assert info["refreshes"] == 1 and info["device_levels"] == 1, info     # (entries outside the kept patterns would have raised)
    assert_equals(h.level_A(1), restated(name, "v2"), "refreshed A_c")
    assert_equals(h.level_AP(0), restated(name, "v2", True), "refreshed A·P")
    A2, h2 = two_level(ctx, mg, case, "v2")
    x2 = h2.vcycle(b).numpy()
    assert_equals(h2.level_A(1), restated(name, "v2"), "twin A_c")
    assert_equals(h2.level_AP(0), restated(name, "v2", True), "twin A·P")
    assert np.array_equal(h.vcycle(b).numpy(), x2) and not np.array_equal(x1, x2)


def test_no_AP_without_merge_ap(ctx, mg):
    case = case_of("hier16")
    ctx.set_option("merge_ap", 0)
    try:
        A, h = two_level(ctx, mg, case, "v")
        h.vcycle(ctx.vec(case["n"]).rand(seed=1))
        assert h.level_AP(0) is None
    finally:
        ctx.set_option("merge_ap", 1)
    h.vcycle(ctx.vec(case["n"]).rand(seed=1))
    assert_equals(h.level_AP(0), restated("hier16", "v", True), "A·P once the option is back")


# ------------------------------------------------------------------ the scan at its edges
@pytest.mark.parametrize("length", ref.SCAN_LENGTHS)
def test_scan_edges_through_transpose(ctx, mg, length):
    """Csr.transpose() of a 3 × cols matrix scans cols + 1 counts: one entry, one 2048-entry tile exactly and one entry more, two
    tiles, 2048 tiles (the tile sums fill one tile), 2049 and 2050 tiles (a third level)"""
    case = ref.fx_scan(length - 1)
    cols = case["cols"]
    tiles = -(-length // 2048)
    assert tiles == {1: 1, 2: 1, 2047: 1, 2048: 1, 2049: 2, 4096: 2, 4097: 3}.get(length, tiles)
    if length >= 2048 ** 2:
        assert tiles - 2048 == {2048 ** 2: 0, 2048 ** 2 + 1: 1, 2048 ** 2 + 2049: 2}[length]
    assert np.isin([j for j in (0, 2047, 2048, cols - 1) if 0 <= j < cols], case["ci"]).all()
    want = ref.transposed(case)
    t0 = time.perf_counter()
    B = upload(ctx, case).transpose()
    rp, ci, v = B.download()
    print(f"transpose 3 x {cols}: {len(case['ci'])} entries, {tiles} scan tiles, {time.perf_counter() - t0:.2f} s on the device path")
    assert B.shape == (cols, 3) and len(rp) == length
    assert np.array_equal(rp, np.r_[0, np.cumsum(np.bincount(case["ci"], minlength=cols))])
    assert np.array_equal(rp, want[0]) and np.array_equal(ci, want[1]) and ref.same_bits(v, want[2])
