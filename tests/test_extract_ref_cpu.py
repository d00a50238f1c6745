"""The host restatement of mgs_csr_extract / mgs_vec_gather / mgs_vec_scatter (tests/extract_ref.py) is itself checked here, without a
device: against scipy's A[rows][:, cols], and for the properties of its fixtures that the GPU tests rely on — equal bits on the device
then mean the contract of include/mgs.h on every arm of the kernels."""
import numpy as np
import pytest
import scipy.sparse as sps

import extract_ref as ref


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("name", sorted(ref.BLOCK_FIXTURES))
def test_restatement_equals_scipy_slicing(name):
    A, rows, cols = ref.BLOCK_FIXTURES[name]()
    T = ref.tagged(A)                                    # distinct non-zero tags: a stored zero is no question for scipy
    nr, nc, rp, ci, v, src = ref.extract(T, rows, cols)
    M = ref.to_scipy(T)
    M = M if rows is None else M[np.asarray(rows)]
    M = sps.csr_matrix(M if cols is None else M[:, np.asarray(cols)])
    M.sort_indices()
    assert (nr, nc) == M.shape
    assert np.array_equal(rp, M.indptr) and np.array_equal(ci, M.indices) and np.array_equal(v, M.data)
    assert np.array_equal(v, src + 1.0)                  # the tag of an entry is its position in A plus one: src is the source position
    # the real values go through the same positions, bit for bit, and every row ascends
    S = ref.extract(A, rows, cols)
    assert np.array_equal(S[5], src) and np.array_equal(bits(S[4]), bits(A[4][src]))
    for k in range(nr):
        assert (np.diff(ci[rp[k]:rp[k + 1]]) > 0).all()
    assert ref.refusal(A, rows, cols) is None


def test_poisson_fixture_is_the_plane_split():
    A, fixed, free = ref.fx_poisson8()
    assert A[:2] == (512, 512) and len(A[3]) == 7 * 512 - 6 * 64
    assert fixed.tolist() == list(range(64)) and np.array_equal(np.sort(np.r_[fixed, free]), np.arange(512))
    d = A[4][A[3] == np.repeat(np.arange(512), np.diff(A[2]))]
    assert (d == 6.0).all() and len(d) == 512 and set(np.unique(A[4])) == {-1.0, 6.0}
    assert np.diff(A[2]).max() == 7
    for name in ("poisson_ff", "poisson_fc", "poisson_cf", "poisson_cc"):
        M, rows, cols = ref.BLOCK_FIXTURES[name]()
        i = ref.info(M, rows, cols)
        assert i["lane_rows"] == len(rows) and i["wave_rows"] == 0, (name, i)
    # A_fc couples the free plane i = 1 with the fixed plane only: 64 entries, one per row of that plane
    S = ref.extract(A, free, fixed)
    assert len(S[3]) == 64 and np.diff(S[2])[:64].tolist() == [1] * 64 and S[4].tolist() == [-1.0] * 64
    V = ref.fx_poisson8_values(0)
    W = ref.fx_poisson8_values(1)
    assert np.array_equal(V[2], A[2]) and np.array_equal(V[3], A[3]) and not np.array_equal(V[4], W[4])


def test_rect_fixture_has_empty_repeated_and_descending_rows():
    A, rows, cols = ref.fx_rect()
    lens = np.diff(A[2])
    assert A[:2] == (37, 53) and lens[3] == 0 and lens[20] == 0 and lens[36] == 0
    assert (np.diff(rows) <= 0).all() and (np.diff(rows) < 0).any() and (np.diff(rows) == 0).any()      # descending, with repeats
    assert {3, 20, 36} <= set(rows.tolist()) and (np.diff(cols) > 0).all()
    i = ref.info(A, rows, None)
    assert i["lane_rows"] == 0 and i["wave_rows"] == 0 and i["max_row_len"] == lens[rows].max()
    S = ref.extract(A, rows, None)
    assert np.array_equal(np.diff(S[2]), lens[rows])
    full = ref.extract(A, None, None)
    assert np.array_equal(full[2], A[2]) and np.array_equal(full[3], A[3]) and np.array_equal(bits(full[4]), bits(A[4]))
    assert np.array_equal(full[5], np.arange(len(A[3])))
    assert ref.info(A, None, cols)["lane_rows"] == 37
    empty_r = ref.extract(A, np.zeros(0, dtype=np.int32), cols)
    empty_c = ref.extract(A, rows, np.zeros(0, dtype=np.int32))
    assert empty_r[:2] == (0, len(cols)) and empty_r[2].tolist() == [0] and empty_c[:2] == (len(rows), 0) and not empty_c[2].any()


def test_boundary_fixture_has_rows_of_64_and_65():
    A, rows, cols = ref.fx_boundary()
    assert np.diff(A[2]).tolist() == [64, 65] == [ref.LANE_LEN, ref.LANE_LEN + 1]
    i = ref.info(A, rows, cols)
    assert i["lane_rows"] == 1 and i["wave_rows"] == 1
    lens = np.diff(ref.extract(A, rows, cols)[2])
    assert (lens > 0).all() and lens[0] < 64 and lens[1] < 65          # both rows lose and keep entries


def test_wave_fixture_chunks_and_special_values():
    A, rows, cols = ref.fx_wave()
    lens = np.diff(A[2])
    assert lens.tolist() == [ref.WAVE_LONG, 3, 0, 130] and ref.WAVE_LONG == 64 * 3 + 17
    r0 = A[3][:ref.WAVE_LONG]
    kept = np.isin(r0, cols)
    assert kept[:64].sum() >= 20 and kept[:64].sum() < 64            # the first chunk: some
    assert kept[64:128].sum() == 0                                   # a chunk that contributes nothing
    assert kept[128:192].sum() == 64                                 # a chunk that contributes all 64
    assert 5 <= kept[192:].sum() < 17                                # the tail
    assert len(np.setdiff1d(cols, np.r_[r0, A[3][A[2][3]:]])) > 0    # columns nobody stores
    assert (np.diff(cols) > 0).all()
    v0 = A[4][:ref.WAVE_LONG]
    assert kept[133] and v0[133] == 0.0 and np.signbit(v0[133])
    assert kept[168] and np.isnan(v0[168]) and bits(v0[168]) == ref.NAN_BITS
    assert rows.tolist().count(0) == 2
    S = ref.extract(A, rows, cols)
    rp = S[2]
    first, second = slice(rp[0], rp[1]), slice(rp[2], rp[3])
    assert np.array_equal(S[3][first], S[3][second]) and np.array_equal(bits(S[4][first]), bits(S[4][second]))
    assert (bits(S[4][first]) == ref.NAN_BITS).sum() == 1 and (bits(S[4][first]) == bits(-0.0)).sum() == 1
    i = ref.info(A, rows, cols, keep_map=True)
    assert i["wave_rows"] == 3 and i["lane_rows"] == 2 and i["map_bytes"] == 4 * len(S[3])
    assert np.diff(rp)[3] == 0 and np.diff(rp)[4] > 0 and 1 <= np.diff(rp)[1] <= 3      # the short row keeps the column it shares with row 0's third chunk


def test_refusals_name_the_lowest_position():
    A, rows, cols = ref.fx_rect()
    assert ref.refusal(A, np.array([0, -1, 5])) == ("row", 1, -1)
    assert ref.refusal(A, np.array([0, 37, 5, 37])) == ("row", 1, 37)
    assert ref.refusal(A, np.array([2 ** 32 + 3])) == ("row", 0, 2 ** 32 + 3)
    assert ref.refusal(A, None, np.array([0, 5, 53])) == ("column", 2, 53)
    assert ref.refusal(A, None, np.array([0, 5, 5, 9])) == ("ascending", 2, 5)
    assert ref.refusal(A, None, np.array([0, 9, 5, 3])) == ("ascending", 2, 5)
    assert ref.refusal(A, np.array([40]), np.array([3, 3])) == ("row", 0, 40)


def test_gather_and_scatter():
    x, idx, y = ref.fx_vectors()
    assert len(np.unique(idx)) < len(idx) and len(np.unique(idx[:100])) == 100
    g, bad = ref.gather(x, idx)
    assert bad == 0 and np.array_equal(bits(g), bits(x[idx]))
    assert (bits(g) == ref.NAN_BITS).any() and (bits(g) == bits(-0.0)).any()
    out, bad = ref.scatter(x, idx[:100], y)
    assert bad == 0
    want = x.copy(); want[idx[:100]] = y
    assert np.array_equal(bits(out), bits(want))
    # one index outside the vector: +0.0 at its place of the gather, skipped by the scatter
    bad_idx = idx[:100].copy(); bad_idx[7] = 300
    g, bad = ref.gather(x, bad_idx)
    assert bad == 1 and bits(g[7]) == 0 and np.array_equal(bits(np.delete(g, 7)), bits(x[np.delete(bad_idx, 7)]))
    out, bad = ref.scatter(x, bad_idx, y)
    want = x.copy(); want[np.delete(bad_idx, 7)] = np.delete(y, 7)
    assert bad == 1 and np.array_equal(bits(out), bits(want))
