"""The host restatements of tests/reorder_ref.py held to scipy on every fixture the GPU test (tests/test_gpu_reorder.py) uses:
permute_ref is A[rperm][:, cperm] with sorted indices, bmat_ref is scipy.sparse.bmat; stored zeros (which scipy's arithmetic may drop
and whose NaN neighbours do not compare) are covered by comparing the patterns through distinct non-zero tags.  check_perm and
bmat_refusal name what the device must name.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sps

import reorder_ref as ref


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def tagged(A):
    return ref.with_values(A, np.arange(1, len(A[3]) + 1, dtype=np.float64))


def same(got, want):
    assert got[:2] == want[:2]
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and np.array_equal(bits(got[4]), bits(want[4]))


@pytest.mark.parametrize("name", sorted(ref.MATRICES))
def test_permute_ref_is_scipy_fancy_indexing(name):
    A = ref.MATRICES[name]()
    T = tagged(A)
    S = ref.to_scipy(T)
    for what, (rp, cp) in ref.lists(A[0], A[1]).items():
        C = ref.permute_ref(A, rp, cp)
        M = S
        if rp is not None:
            M = M[rp]
        if cp is not None:
            M = M[:, cp]
        want = ref.csr(M)
        got = ref.permute_ref(T, rp, cp)
        same(ref.matrix(got), want)                                             # the pattern and where every entry went
        assert np.array_equal(got[5], want[4].astype(np.int64) - 1), what      # the tag is the source position + 1: the kept map
        assert np.array_equal(C[5], got[5]) and np.array_equal(bits(C[4]), bits(A[4][C[5]])), what
        assert all((np.diff(C[3][C[2][i]:C[2][i + 1]]) > 0).all() for i in range(C[0])), what      # rows ascend strictly
        # the round trip is the identity, bit for bit
        back = ref.permute_ref(ref.matrix(C), None if rp is None else ref.inverse(rp), None if cp is None else ref.inverse(cp))
        same(ref.matrix(back), A)


def test_fixtures_have_the_properties_the_gpu_test_relies_on():
    P = ref.fx_poisson5()
    lens = np.diff(P[2])
    assert P[0] == 125 and lens.min() == 4 and lens.max() == 7
    A = ref.fx_crafted()
    lens = np.diff(A[2])
    assert A[:2] == (40, 330) and tuple(lens[:8]) == ref.CRAFTED_LENS == (0, 1, 63, 64, 65, 128, 129, 300) and lens[8:].max() <= 12
    assert ref.permute_info(A, None, np.arange(330), True) == {"lane_rows": 36, "wave_rows": 4, "max_row_len": 300, "map_bytes": 4 * len(A[3])}
    assert ref.permute_info(A, np.arange(40), None) == {"lane_rows": 0, "wave_rows": 0, "max_row_len": 300, "map_bytes": 0}
    for M in (P, A):
        b = bits(M[4])
        assert (b == bits(-0.0)).sum() == 1 and (b == np.uint64(ref.NAN_BITS)).sum() == 1 and (b == 0).sum() == 2
    rp, cp = ref.lists(40, 330)["random_both"]
    assert not np.array_equal(rp, np.arange(40)) and sorted(rp) == list(range(40)) and sorted(cp) == list(range(330))


def test_check_perm_names_the_lowest_offender():
    assert ref.check_perm([2, 0, 1], 3, "row") is None
    assert ref.check_perm([], 0, "row") is None
    assert ref.check_perm([0, -1, 5], 3, "row") == ("row", 1, -1, "range")
    assert ref.check_perm([0, 1, 3], 3, "column") == ("column", 2, 3, "range")
    assert ref.check_perm([1, 0, 1, 2], 4, "row") == ("row", 2, 1, "repeat")                     # position 2 repeats position 0
    assert ref.check_perm([1, 0, 1, 9], 4, "row") == ("row", 2, 1, "repeat")                     # the range error sits higher: the repeat is named
    assert ref.check_perm([1, 9, 1, 0], 4, "row") == ("row", 1, 9, "range")                      # ... and lower: the range error is named
    assert ref.check_perm([0, 2 ** 32 + 3, 1, 2], 4, "row") == ("row", 1, 2 ** 32 + 3, "range")  # would narrow to 3 and make a bijection
    assert ref.check_perm(np.array([0, 2 ** 32 + 3, 1, 3], dtype=np.int64), 4, "row") == ("row", 1, 2 ** 32 + 3, "range")
    A = ref.fx_poisson5()
    good, bad = np.arange(125), np.r_[np.arange(124), 7]
    assert ref.refusal(A, good, good) is None and ref.refusal(A, None, None) is None
    assert ref.refusal(A, bad, np.r_[-4, np.arange(124)]) == ("row", 124, 7, "repeat")           # a row violation before any column violation
    assert ref.refusal(A, good, np.r_[-4, np.arange(124)]) == ("column", 0, -4, "range")


@pytest.mark.parametrize("name", sorted(ref.bmat_fixtures()))
def test_bmat_ref_is_scipy_bmat(name):
    mats, grid, rs, cs = ref.bmat_fixtures()[name]
    G = ref.resolve(mats, grid)
    got = ref.bmat_ref(G, rs, cs)
    # patterns through tags (a tag per block position, so a handle used twice is told apart): scipy.sparse.bmat wants a size for an
    # all-None block row or column as an explicit empty matrix
    br, bc = len(G), len(G[0])
    rsz = [next((B[0] for B in G[I] if B is not None), None if rs is None else rs[I]) for I in range(br)]
    csz = [next((G[I][J][1] for I in range(br) if G[I][J] is not None), None if cs is None else cs[J]) for J in range(bc)]
    base, tags, sp = 0, [[None] * bc for _ in range(br)], [[None] * bc for _ in range(br)]
    for I in range(br):
        for J in range(bc):
            if G[I][J] is None:
                sp[I][J] = sps.csr_matrix((rsz[I], csz[J]))
            else:
                tags[I][J] = ref.with_values(G[I][J], base + np.arange(1, len(G[I][J][3]) + 1, dtype=np.float64))
                sp[I][J] = ref.to_scipy(tags[I][J])
                base += len(G[I][J][3])
    want = ref.csr(sps.bmat(sp, format="csr"))
    same(ref.bmat_ref(tags, rs, cs), want)
    assert got[:2] == want[:2] and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    # the values: every entry of C carries the bits of the block entry its tag names
    flat = np.concatenate([np.asarray(G[I][J][4]) for I in range(br) for J in range(bc) if G[I][J] is not None] + [np.zeros(0)])
    assert np.array_equal(bits(got[4]), bits(flat[want[4].astype(np.int64) - 1]))
    info = ref.bmat_info(G, rs, cs)
    assert info["block_rows"] == br and info["block_cols"] == bc and info["max_row_len"] == int(np.diff(want[2]).max())


def test_bmat_fixtures_cover_the_cases():
    fx = ref.bmat_fixtures()
    mats = fx["hstack"][0]
    assert sum(b is None for row in fx["two_by_two_one_null"][1] for b in row) == 1
    assert fx["null_block_row"][1][1] == [None, None] and fx["null_block_row"][2][1] == 5
    C = ref.bmat_ref(ref.resolve(mats, fx["null_block_row"][1]), fx["null_block_row"][2], None)
    assert (np.diff(C[2])[37:42] == 0).all() and C[:2] == (52, 82)
    assert (np.diff(mats["R"][2])[[3, 20, 36]] == 0).all() and (np.diff(mats["S"][2])[[0, 20]] == 0).all()
    assert mats["R"][:2] == (37, 53) and mats["S"][:2] == (37, 29) and mats["T"][:2] == (10, 53) and mats["B"][:2] == (53, 29)
    grid = fx["same_handle_twice"][1]
    assert grid[0][0] == grid[1][1] and grid[0][1] == grid[1][0]


def test_bmat_refusal_by_shapes_and_the_entry_limit():
    mats = ref.bmat_fixtures()["hstack"][0]
    R, S, T, L = mats["R"], mats["S"], mats["T"], mats["L"]
    assert ref.bmat_refusal([[R, S]]) is None
    assert ref.bmat_refusal([[R, T]]) == ("rows", (0, 1))
    assert ref.bmat_refusal([[R], [S]]) == ("cols", (1, 0))
    assert ref.bmat_refusal([[R, S]], [36], None) == ("rows", (0, 0))
    assert ref.bmat_refusal([[R, S], [None, None]]) == ("no row size", 1)
    assert ref.bmat_refusal([[R, None], [T, None]]) == ("no col size", 1)
    assert ref.bmat_refusal([[R, None], [T, None]], None, [53, 4]) is None
    assert ref.bmat_refusal([[L] * 257]) == ("grid", 257) and ref.bmat_refusal([[L] * 16] * 16) is None
    # the limit on the entries, which no test-sized matrix reaches: only shapes and the last rowptr entry are read here
    half = (1, 1, np.array([0, 2 ** 30], dtype=np.int64), None, None)
    almost = (1, 1, np.array([0, 2 ** 30 - 2], dtype=np.int64), None, None)
    assert ref.bmat_refusal([[half], [half]]) == ("entries", 2 ** 31)
    assert ref.bmat_refusal([[half], [almost]]) is None                          # 2³¹ − 2 entries: the largest result
    assert ref.bmat_refusal([[half], [(1, 1, np.array([0, 2 ** 30 - 1], dtype=np.int64), None, None)]]) == ("entries", 2 ** 31 - 1)


def test_two_field_fixture():
    L, cI, K, p = ref.fx_two_field()
    n = L[0]
    assert n == 216 and K[:2] == (432, 432)
    lam = np.linalg.eigvalsh(ref.to_scipy(K).toarray())
    assert lam.min() > 0.3 and abs(np.linalg.eigvalsh(ref.to_scipy(L).toarray()).min() - (6 - 6 * np.cos(np.pi / 7))) < 1e-12
    assert np.array_equal(ref.to_scipy(K).toarray(), ref.to_scipy(K).toarray().T)
    # interleaved: unknown 2k is u_k, 2k + 1 is v_k; the coupling sits on the first off-diagonals of 2 × 2 blocks
    Ki = ref.permute_ref(K, p, p)
    D = ref.to_scipy(ref.matrix(Ki)).toarray()
    assert D[0, 1] == ref.COUPLING and D[1, 0] == ref.COUPLING and D[0, 0] == 6.0 and D[1, 1] == 6.0 and D[0, 2] == -1.0 and D[1, 3] == -1.0 and D[0, 3] == 0.0
    back = ref.permute_ref(ref.matrix(Ki), ref.inverse(p), ref.inverse(p))
    same(ref.matrix(back), K)
