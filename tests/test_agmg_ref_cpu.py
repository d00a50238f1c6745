"""Pins the yardstick of the device-matching tests, tests/agmg_ref.py, on the CPU: its properties checker accepts the restatement's own
output on every input family of tests/test_gpu_agmg_matching.py (and rejects a broken one), its G0 set is the reference's on CSky3d30, the
uniform chain and the 2-D Poisson operator come out in closed form, and edge_hash equals values computed by hand."""
import numpy as np
import pytest

import agmg_ref as R

KTG = 10.0
SHARD_N = 12


def _csky3d():
    from multigridsolver_amd import synthetic
    rp, ci, v = synthetic.csky3d(12)
    return R.csr(12 ** 3, 12 ** 3, rp, ci, v)


# every input family of tests/test_gpu_agmg_matching.py → (A, origin, zone)
FAMILIES = {
    "chain_2049": lambda: R.chain(2049),
    "poisson2d_33": lambda: R.poisson2d(33),
    "poisson3d_9": lambda: R.poisson3d(9),
    "poisson3d_17": lambda: R.poisson3d(17),
    "random_nonsymmetric": R.random_nonsymmetric,
    "branchy": lambda: R.branchy()[0],
    "hash_chain": R.hash_chain,
    "one_sided_random": R.one_sided_random,
    "forward_chain": R.forward_chain,
    "one_sided_zeros": R.one_sided_zeros,
    "csky3d_12": _csky3d,
    "shard": lambda: (R.poisson3d_shard(SHARD_N, 4, 8)[0], None, None),
    "shard_zoned": lambda: (lambda A, zone: (A, None, zone))(*R.poisson3d_shard(SHARD_N, 4, 8)),
    "poisson2d_16_permuted_origin": lambda: (R.poisson2d(16), np.random.default_rng(8).permutation(256), None),
}


def test_edge_hash_hand_values():
    """edge_hash(a, b): h = a·0x9E3779B1 ^ (b + 0x7F4A7C15)·0x85EBCA77; h ^= h >> 15; h *= 0x2C1B3C6D; h ^= h >> 12; h *= 0x297A2D39;
    h ^= h >> 15, all mod 2^32.  Worked out step by step in unbounded integers, e.g. (0, 1): 0 ^ 0x7F4A7C16·0x85EBCA77 = 0x47BB0A3A →
    0x47BB854C → ·0x2C1B3C6D = 0x9D19915C → 0x9D1040C5 → ·0x297A2D39 = 0x3EE30CDD → 0x3EE3711B; the last pair wraps in the first
    product and sits at the largest origins an int32 index can hold."""
    hand = {(0, 1): 0x3EE3711B, (1, 2): 0x657958E4, (2, 3): 0xABC23B87, (2 ** 31 - 2, 2 ** 31 - 1): 0x3E1B4031, (12345, 4194304): 0xA81A0B05}
    pairs = list(hand)
    got = R.edge_hash(np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]))
    assert [int(g) for g in got] == [hand[p] for p in pairs]
    assert int(R.edge_hash(0, 1)) == 0x3EE3711B and int(R.edge_hash(1, 0)) != 0x3EE3711B        # not symmetric: the key passes (mn, mx)


@pytest.mark.parametrize("n", [5, 6, 40, 41, 2047, 2048, 2049])
def test_uniform_chain_closed_form(n):
    agg, rounds, br = R.pairwise_pass(R.chain(n), KTG, 1)
    cf = R.chain_closed_form(n)
    assert np.array_equal(agg, cf)
    assert rounds == 2 and br["g0"] == 4 and sum(br.values()) == 4
    assert cf[0] == -1 and cf[-1] == -1 and cf[1] == 0
    m = np.arange(1, (n - 1) // 2)                                                    # pairs (2m, 2m+1) with 2m+1 <= n−2
    assert np.array_equal(cf[2 * m], m) and np.array_equal(cf[2 * m + 1], m)
    if n == 41:
        assert list(cf[:6]) == [-1, 0, 1, 1, 2, 2] and list(cf[-3:]) == [19, 19, -1]
    if n == 40:
        assert list(cf[-4:]) == [18, 18, 19, -1]                                      # even n: row n−2 is the last singleton
    R.check_matching(R.chain(n), agg, KTG)


def test_poisson2d_aligned_pairs():
    """n even: an interior row i = y·n + x has the parity of x; all μ are 4, distance 1 beats distance n, and the parity rule makes every
    interior node with 2 <= x <= n−3 pair with i ^ 1 in round 0.  The boundary rows are in G0 (4 >= 1.25·3)."""
    n = 12
    A = R.poisson2d(n)
    agg, rounds, br = R.pairwise_pass(A, KTG, 1)
    y, x = np.divmod(np.arange(n * n), n)
    boundary = (x == 0) | (x == n - 1) | (y == 0) | (y == n - 1)
    assert np.array_equal(agg < 0, boundary)
    inner = np.nonzero(~boundary & (x >= 2) & (x <= n - 3))[0]
    assert np.array_equal(agg[inner], agg[inner ^ 1])
    sizes = np.bincount(agg[agg >= 0])
    assert np.all(sizes[agg[inner]] == 2)
    # the columns x = 1 and x = n−2 are left over and pair along y in round 1 with the same rule: (y even, y + 1)
    for xx in (1, n - 2):
        col = np.nonzero(~boundary & (x == xx) & (y >= 2) & (y <= n - 3))[0]
        assert np.array_equal(agg[col], agg[(col // n ^ 1) * n + xx])
    R.check_matching(A, agg, KTG)


def test_g0_set_is_the_references_on_csky3d30(orc, inputs, golden):
    A = orc.Csr.read(inputs["CSky3d30"]).to_scipy().tocsr(); A.sort_indices()
    pat = R._Pattern(A)
    _, _, g0 = R.node_stats(pat, KTG, True)
    ref = golden("agmg_groups")["CSky3d30_k10_n2_t8_groups"]
    assert np.array_equal(g0, ref < 0) and 0 < g0.sum() < g0.size


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_check_matching_accepts_the_restatement(family):
    A = FAMILIES[family]()
    A, origin, zone = A if isinstance(A, tuple) else (A, None, None)
    for npass in (1, 2, 3):
        Rr = R.aggregate(A, KTG, npass, 8.0, origin, zone)
        R.check_matching(A, Rr.agg, KTG, npass=len(Rr.passes), zone=zone)
        if family.startswith("shard"):
            # rows < cols: every owned row of the two outer planes has one halo column, which enters s_i and the G0 test and never pairs
            assert A.shape == (4 * SHARD_N ** 2, 6 * SHARD_N ** 2)
            assert Rr.passes[0]["branches"]["halo"] == 2 * SHARD_N ** 2
        assert (Rr.passes[0]["branches"]["zone"] > 0) == (zone is not None)
        if origin is not None:
            assert not np.array_equal(Rr.agg, R.aggregate(A, KTG, npass, 8.0).agg)          # the tie-breaks do depend on the origin
        for p, c in zip(Rr.passes, R.check_passes(Rr, KTG)):
            assert p["rounds"] < R.MAX_ROUNDS
            print(family, "npass", npass, "rounds", p["rounds"], "pairs/singletons/G0", R.pass_counts(p["agg"]), p["branches"], c)
        sizes = np.bincount(Rr.agg[Rr.agg >= 0])
        assert sizes.max() <= 2 ** len(Rr.passes)


def test_check_matching_rejects_broken_matchings():
    A = R.random_nonsymmetric(400, 1)
    agg, _, _ = R.pairwise_pass(A, KTG, 1)
    sizes = np.bincount(agg)

    def renumber(labels):                                                               # ids = ranks of the smallest members
        _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
        rank = np.empty(first.size, dtype=np.int32); rank[np.argsort(first)] = np.arange(first.size)
        return rank[inv]
    assert np.array_equal(renumber(agg), agg)
    i, j = np.nonzero(agg == np.nonzero(sizes == 2)[0][0])[0]
    torn = agg.copy(); torn[j] = agg.max() + 1                                          # a pair torn into two singletons
    with pytest.raises(AssertionError, match="join two singletons"):
        R.check_matching(A, renumber(torn), KTG)
    swapped = agg.copy(); swapped[agg == 0], swapped[agg == 1] = 1, 0
    with pytest.raises(AssertionError, match="ranks"):
        R.check_matching(A, swapped, KTG)
    # two unrelated singletons glued together: not a coupling
    single = np.nonzero(sizes == 1)[0]
    pat = R._Pattern(A)
    for a in single:
        for b in single:
            ra, rb = np.nonzero(agg == a)[0][0], np.nonzero(agg == b)[0][0]
            if a < b and not np.any((pat.ui == ra) & (pat.uj == rb)):
                glued = agg.copy(); glued[rb] = a; glued = renumber(glued)
                with pytest.raises(AssertionError, match="not admissible"):
                    R.check_matching(A, glued, KTG)
                return
    pytest.fail("no two uncoupled singletons in the input")


def test_galerkin_sum_order_is_sequential():
    """galerkin() relies on np.add.at adding in index order; a plain Python loop over the member rows gives the same bits"""
    A = R.random_nonsymmetric(300, 4)
    agg = R.aggregate(A, KTG, 2, 8.0).agg
    G = R.galerkin(A, agg)
    nc = G.shape[0]
    for c in range(nc):
        acc = {}
        for i in np.nonzero(agg == c)[0]:
            for k in range(A.indptr[i], A.indptr[i + 1]):
                a = agg[A.indices[k]]
                if a >= 0:
                    acc[a] = acc[a] + A.data[k] if a in acc else A.data[k]
        cols = sorted(acc)
        assert list(G.indices[G.indptr[c]:G.indptr[c + 1]]) == cols
        assert np.array_equal(G.data[G.indptr[c]:G.indptr[c + 1]], np.array([acc[a] for a in cols]))


def test_hash_chain_needs_the_hash_only_rounds():
    agg, rounds, _ = R.pairwise_pass(R.hash_chain(), KTG, 1)
    assert rounds == 28 > R.MU_ROUNDS


def test_one_sided_inputs_pair_along_one_sided_couplings():
    A = R.one_sided_random()
    agg, rounds, _ = R.pairwise_pass(A, KTG, 1)
    assert R._Pattern(A).asymmetric and rounds == 4
    assert R.pass_counts(agg) == (252, 146, 850)
