"""The host restatement of the aggregation Galerkin product (tests/galerkin_ref.py) is itself checked here, without a device: its two
forms against each other, against the oracle's pattern and math.fsum of every entry's summands, and — what makes the bit-for-bit GPU
tests sharp — every fixture family for its sensitivity to the order of the sums.  The fixtures' own promises (which instantiation,
which arm, which edge) are asserted here too."""
import math

import numpy as np
import pytest
import scipy.sparse as sps

import galerkin_ref as ref

U = 2.0 ** -53
FORMS = [(name, "v", False) for name in sorted(ref.FAMILIES)] + \
        [(f"hier{L}", values, ap) for L in ref.HIER_L for values, ap in (("v2", False), ("v", True), ("v2", True))]
_cases = {}


def case_of(name):
    if name not in _cases:
        _cases[name] = ref.FAMILIES[name]()
    return _cases[name]


def selector(orc, cm, ncols):
    """the 0/1 matrix of a column map: entry (j, cm[j]) where cm[j] ≥ 0"""
    ok = np.flatnonzero(cm >= 0)
    return orc.Csr.from_scipy(sps.csr_matrix((np.ones(len(ok)), (ok, cm[ok])), shape=(len(cm), ncols)))


def oracle_product(orc, case, values="v", ap=False):
    """(Pᵀ·A)·P, the oracle's association (the row selector is P of the owned rows, the column selector covers a shard's halo
    columns too); ap: A·P"""
    Ao = orc.Csr.from_arrays(case["n"], case["cols"], case["rp"], case["ci"], case[values])
    Pc = selector(orc, ref.colmap_of(case), ref.ncols_of(case))
    if ap:
        return Ao.matmul(Pc)
    if case["cols"] == case["n"]:
        return Ao.galerkin(Pc)
    return selector(orc, case["agg"], case["nc"]).transpose().matmul(Ao).matmul(Pc)


def differs(a, b):
    return int((a.view(np.int64) != b.view(np.int64)).sum())


@pytest.mark.parametrize("name,values,ap", FORMS)
def test_restatement_against_its_fast_form_the_oracle_and_fsum(orc, name, values, ap):
    case = case_of(name)
    rp, ci, v, cnt, terms = ref.restate(case, values, ap, with_terms=True)
    frp, fci, fv, fcnt = ref.restate(case, values, ap, fast=True)
    assert np.array_equal(rp, frp) and np.array_equal(ci, fci) and np.array_equal(cnt, fcnt)
    assert ref.same_bits(v, fv)
    assert len(rp) == (case["n"] if ap else case["nc"]) + 1
    for c in range(len(rp) - 1):
        assert (np.diff(ci[rp[c]:rp[c + 1]]) > 0).all()
    O = oracle_product(orc, case, values, ap)
    assert O.shape == (len(rp) - 1, ref.ncols_of(case))
    assert np.array_equal(rp, O.rowptr) and np.array_equal(ci, O.col)
    ov = np.asarray(O.val, dtype=np.float64)
    exact = np.array([math.fsum(t) for t in terms])
    bar = (cnt - 1) * U * np.array([math.fsum(abs(x) for x in t) for t in terms])
    assert (np.abs(v - exact) <= bar).all()
    assert (np.abs(ov - exact) <= bar).all()
    if ap:      # A·P has one association only: the oracle's product walks a row the same way
        assert ref.same_bits(v, ov)


@pytest.mark.parametrize("name,values,ap", FORMS)
def test_the_order_of_the_sums_shows_in_the_bits(orc, name, values, ap):
    """walking the members backwards, walking the rows' entries backwards and the oracle's association each change at least one
    entry's bits — otherwise a bit-for-bit GPU test on this fixture shows nothing.  A·P has no member order and one association:
    there the entries' order is the probe, and the operator's Galerkin form (same matrix, same aggregates) carries the others."""
    case = case_of(name)
    rp, ci, v, cnt = ref.restate(case, values, ap)
    assert (cnt >= 3).sum() > 0, "groups of three and more summands"
    probes = dict(entries=ref.restate(case, values, ap, reverse_entries=True))
    if not ap:
        probes["members"] = ref.restate(case, values, ap, reverse_members=True)
        O = oracle_product(orc, case, values, ap)
        probes["oracle"] = (O.rowptr, O.col, np.asarray(O.val, dtype=np.float64))
    for what, other in probes.items():
        assert np.array_equal(rp, other[0]) and np.array_equal(ci, other[1]), what
        assert differs(v, other[2]) > 0, what
        assert (v.view(np.int64) != other[2].view(np.int64))[cnt < 2].sum() == 0, what        # a lone summand has no order


def test_values_are_not_on_a_grid_and_span_binades():
    for name in ("spill", "sizes", "hier16"):
        v = case_of(name)["v"]
        m, e = np.frexp(v[v != 0])
        assert (v < 0).any() and (v > 0).any()
        assert e.max() - e.min() >= 6, name
        assert ((m * 2.0 ** 20) % 1 != 0).mean() > 0.99, name         # no value is a multiple of 2^-20 of its binade


# ------------------------------------------------------------------ the fixtures' own promises
@pytest.mark.parametrize("M,nc", ref.MAXUB_CASES)
def test_maxub_fixtures_pick_their_instantiation_at_both_ends(M, nc):
    case = case_of(f"maxub{M}_nc{nc}")
    assert case["nc"] == nc and ref.maxub(case) == M
    cap, tbk = ref.slots_of(M)
    assert (cap, tbk) == {16: (16, 256), 17: (32, 128), 32: (32, 128), 33: (64, 64), 64: (64, 64)}[M]
    assert nc in (tbk - 1, tbk, tbk + 1, 2 * tbk)
    lens = np.diff(case["rp"])
    cptr, members = ref.member_lists(case["agg"], nc)
    assert int(lens[members[cptr[nc - 1]:cptr[nc]]].sum()) == M      # the last lane before the sentinel lane c == nc
    assert (np.diff(cptr) >= 1).all() and (lens == 0).any()


def test_maxub_cases_cover_every_workgroup_edge():
    assert sorted({(ref.slots_of(M), nc % ref.slots_of(M)[1]) for M, nc in ref.MAXUB_CASES}) == \
        sorted({(s, r) for s in ((16, 256), (32, 128), (64, 64)) for r in (s[1] - 1, 0, 1)})


def test_spill_fixture():
    case = case_of("spill")
    assert ref.slots_of(ref.maxub(case)) == (64, 64)
    rp, ci, v, cnt, terms = ref.restate(case, with_terms=True)
    lens = np.diff(rp)
    assert lens[10:16].tolist() == case["spill_lens"] == [63, 64, 65, 65, 66, 65] and 440 <= lens[16] <= 520
    cm = case["agg"]

    def walk(c):
        """the coarse columns of row c in the order walked, and the position at which the 65th distinct one appears"""
        seq = [int(cm[j]) for i in (2 * c, 2 * c + 1) for j in case["ci"][case["rp"][i]:case["rp"][i + 1]]]
        seen, at = [], None
        for p, a in enumerate(seq):
            if a not in seen:
                seen.append(a)
                if len(seen) == 65:
                    at = p
        return seq, at, seen
    seq, at, seen = walk(12)
    assert at == len(seq) - 1 and seq[at] == max(seen)                 # the very last entry walked
    seq, at, seen = walk(13)
    assert seq[at] < min(seen[:64])                                    # the front of the global segment
    for c in (14, 15):
        seq, at, seen = walk(c)
        assert min(seen[:64]) < seq[at] < max(seen[:64])
        assert len([a for a in seq[at + 1:] if a in seen[:64]]) >= 3   # later duplicates of columns held before the spill
    assert len(walk(14)[2]) == 66 and len(walk(15)[2]) == 65
    assert (cnt[rp[12]:rp[13]] >= 2).any() and (cnt[rp[16]:rp[17]] >= 2).any()


def test_g0_fixture():
    case = case_of("g0")
    agg, nc = case["agg"], case["nc"]
    assert 0.03 <= (agg < 0).mean() <= 0.08
    r = case["all_g0"]
    cols = case["ci"][case["rp"][r]:case["rp"][r + 1]]
    assert agg[r] >= 0 and len(cols) >= 3 and (agg[cols] < 0).all()
    rp, ci, v, cnt = ref.restate(case)
    cptr, members = ref.member_lists(agg, nc)
    e = case["empty_result"]
    assert cptr[e + 1] - cptr[e] >= 2 and rp[e + 1] == rp[e]
    assert np.diff(case["rp"])[members[cptr[e]]] == 0
    for c in case["no_member"]:
        assert cptr[c + 1] == cptr[c] and rp[c + 1] == rp[c]
    assert case["no_member"] == [7, nc - 1]
    member_rows_empty = np.diff(case["rp"])[members] == 0
    assert member_rows_empty.sum() >= 50
    assert (agg[case["ci"]] < 0).sum() >= 100                           # entries that drop out


def test_sizes_fixture():
    case = case_of("sizes")
    assert sorted(set(np.bincount(case["agg"]).tolist())) == [1, 2, 3, 8, 16]
    cptr, members = ref.member_lists(case["agg"], case["nc"])
    spread = [int(np.ptp(members[cptr[c]:cptr[c + 1]])) for c in range(case["nc"]) if cptr[c + 1] - cptr[c] == 16]
    assert min(spread) > 200                                            # shuffled membership
    assert ref.slots_of(ref.maxub(case)) == (64, 64)


def test_zeros_fixture():
    case = case_of("zeros")
    rp, ci, v, cnt = ref.restate(case)
    assert rp.tolist() == [0, 2, 4, 7] and ci.tolist() == [0, 1, 0, 1, 0, 1, 2] and cnt.tolist() == [1, 2, 2, 2, 8, 8, 16]
    assert ref.same_bits(v[:4], case["expect_head"])
    assert np.signbit(v[0]) and v[0] == 0 and not np.signbit(v[1]) and not np.signbit(v[2]) and v[3] == -2.5
    assert not ref.same_bits(np.array([0.0]), np.array([-0.0])) and np.array_equal(np.array([0.0]), np.array([-0.0]))


def test_shard_fixture():
    case = case_of("shard")
    n, nc, hm = case["n"], case["nc"], case["halo_map"]
    assert case["cols"] == n + len(hm) > n
    assert hm[0] == hm[1] == nc + 4 and (hm[[3, 17, 40]] == -1).all()
    used = np.unique(hm[hm >= 0])
    assert used.min() >= nc and used.max() < nc + case["n_halo_coarse"] and len(used) < case["n_halo_coarse"] - 20
    r0 = case["ci"][case["rp"][0]:case["rp"][1]]
    assert n in r0 and n + 1 in r0
    rp, ci, v, cnt = ref.restate(case)
    assert (ci >= nc).sum() > 100 and ci.max() < nc + case["n_halo_coarse"]
    assert (hm[case["ci"][case["ci"] >= n] - n] < 0).sum() > 0          # entries on −1 slots drop out


@pytest.mark.parametrize("L", ref.HIER_L)
def test_hier_fixtures_pick_their_arm(L):
    case = case_of(f"hier{L}")
    n, nc, rp, ci = case["n"], case["nc"], case["rp"], case["ci"]
    rowid = np.repeat(np.arange(n), np.diff(rp))
    for values in ("v", "v2"):
        v = case[values]
        d = np.zeros(n); d[rowid[ci == rowid]] = v[ci == rowid]
        off = np.bincount(rowid, weights=np.where(ci == rowid, 0.0, np.abs(v)), minlength=n)
        assert (d > 1.15 * off).all() and (d > 0).all()                # strict row dominance, which the aggregated rows inherit
    off = ci != rowid
    assert (np.sign(case["v"][off]) != np.sign(case["v2"][off])).mean() > 0.3
    assert {1, 7, 8, 9, 15, 16, 17} <= set(np.diff(rp).tolist())
    ac, ap = ref.restate(case), ref.restate(case, ap=True)
    assert int(np.diff(ac[0]).max()) == L and int(np.diff(ap[0]).max()) == L
    assert int(np.diff(ap[0])[case["star"]]) == L
    z = ref.restate(case, "v2", ap=True)[2]
    assert ((z == 0) & np.signbit(z)).sum() >= 7 and ((z == 0) & ~np.signbit(z)).sum() >= 1      # the refresh meets signed zeros
    arm = {8: (8, 256), 9: (16, 256), 16: (16, 256), 17: (32, 128), 32: (32, 128), 33: (64, 64), 64: (64, 64), 80: (64, 64)}[L]
    assert ref.numeric_slots_of(L) == arm and nc > arm[1] and nc % arm[1] != 0
    # runs of neighbouring entries in one aggregate, then in the next; and one aggregate across a member boundary
    a = case["agg"][ci]
    same = (a[1:] == a[:-1]) & (rowid[1:] == rowid[:-1])
    assert same.sum() > n and ((~same) & (rowid[1:] == rowid[:-1])).sum() > n
    cptr, members = ref.member_lists(case["agg"], nc)
    across = 0
    for c in range(nc):
        for p in range(cptr[c], cptr[c + 1] - 1):
            i, j = members[p], members[p + 1]
            if rp[i + 1] > rp[i] and rp[j + 1] > rp[j] and a[rp[i + 1] - 1] == a[rp[j]]:
                across += 1
    assert across >= nc // 5


def test_hier_arms_are_all_there():
    assert sorted({(ref.numeric_slots_of(L), L > 64) for L in ref.HIER_L}) == \
        [((8, 256), False), ((16, 256), False), ((32, 128), False), ((64, 64), False), ((64, 64), True)]


@pytest.mark.parametrize("length", [s for s in ref.SCAN_LENGTHS if s <= 4097])
def test_transposed_restatement_against_scipy(length):
    case = ref.fx_scan(length - 1)
    cols = case["cols"]
    for j in (0, 2047, 2048, cols - 1):
        assert not 0 <= j < cols or j in case["ci"]
    rp, ci, v = ref.transposed(case)
    assert len(rp) == length
    T = sps.csr_matrix((case["v"], case["ci"], case["rp"]), shape=(3, cols)).T.tocsr()
    T.sort_indices()
    assert np.array_equal(rp, T.indptr) and np.array_equal(ci, T.indices) and ref.same_bits(v, T.data)
    if cols >= 100:
        assert 0.25 < len(case["ci"]) / (3 * cols) < 0.42
