"""The restatement the device COO assembly is held to (tests/ingest_ref.py) checked on its own: against scipy's COO → CSR conversion
(pattern exact; values to 1e-12 relative, scipy's summation order is unspecified) and exactly on duplicates that sum back without
rounding."""
import os

import numpy as np
import scipy.sparse as sps

from conftest import INP
from ingest_ref import coo_to_csr_ref, csr_triples, dyadic_split, permuted


def random_case(seed, rows, cols, ntrip, npos):
    rng = np.random.default_rng(seed)
    pos = rng.choice(rows * cols, size=npos, replace=False)
    pick = np.concatenate([np.arange(npos), rng.integers(0, npos, size=ntrip - npos)])      # every position at least once
    rng.shuffle(pick)
    val = rng.standard_normal(ntrip) * 10.0 ** rng.uniform(-8, 8, size=ntrip)
    return pos[pick] // cols, pos[pick] % cols, val


def test_against_scipy():
    for seed, (rows, cols, ntrip, npos) in enumerate([(300, 300, 5000, 2000), (1, 7, 40, 5), (50, 9, 200, 200), (64, 64, 1, 1)]):
        row, col, val = random_case(seed, rows, cols, ntrip, npos)
        rp, ci, v, order = coo_to_csr_ref(rows, row, col, val)
        S = sps.coo_matrix((val, (row, col)), shape=(rows, cols)).tocsr()
        S.sort_indices()
        assert len(ci) == npos and S.nnz == npos
        assert np.array_equal(rp, S.indptr) and np.array_equal(ci, S.indices)
        # two summation orders of one run differ by at most (run length − 1)·2⁻⁵³·Σ|v|, far inside 1e-12 of the result unless a run cancels
        assert np.all(np.abs(v - S.data) <= 1e-12 * np.abs(S.data)), float(np.max(np.abs(v - S.data) / np.abs(S.data)))
        assert sorted(order.tolist()) == list(range(ntrip))
        assert np.all(np.diff(row[order]) >= 0)


def test_order_is_row_col_then_input_position():
    row = np.array([1, 0, 1, 1, 0]); col = np.array([2, 3, 2, 0, 3]); val = np.array([1.0, 1e16, -1.0, 5.0, 1.0])
    rp, ci, v, order = coo_to_csr_ref(2, row, col, val)
    assert order.tolist() == [1, 4, 3, 0, 2]
    assert rp.tolist() == [0, 1, 3] and ci.tolist() == [3, 0, 2]
    assert v.tolist() == [1e16 + 1.0, 5.0, 0.0]
    # the sum starts from the first value itself: a lone -0.0 keeps its sign, and so does -0.0 + -0.0
    _, _, v, _ = coo_to_csr_ref(1, np.array([0, 0, 0]), np.array([0, 1, 1]), np.array([-0.0, -0.0, -0.0]))
    assert np.signbit(v).tolist() == [True, True]


def test_empty_rows_and_no_triples():
    rp, ci, v, order = coo_to_csr_ref(4, np.array([2]), np.array([1]), np.array([3.0]))
    assert rp.tolist() == [0, 0, 0, 1, 1] and ci.tolist() == [1] and v.tolist() == [3.0]
    rp, ci, v, order = coo_to_csr_ref(3, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
    assert rp.tolist() == [0, 0, 0, 0] and len(ci) == 0 and len(v) == 0 and len(order) == 0


def test_dyadic_split_of_csky3d10_reproduces_read_mtx_exactly():
    import multigridsolver_amd as mg
    n, m, rp, ci, v = mg.read_mtx(os.path.join(INP, "CSky3d10.mtx"))
    assert n == 1000
    row, col, val = csr_triples(rp, ci, v)
    for seed, (r3, c3, v3) in enumerate([dyadic_split(row, col, val), permuted(5, *dyadic_split(row, col, val)), permuted(6, row, col, val)]):
        rp2, ci2, v2, order = coo_to_csr_ref(n, r3, c3, v3)
        assert rp2.dtype == np.int32 and ci2.dtype == np.int32
        assert np.array_equal(rp2, rp) and np.array_equal(ci2, ci), seed
        assert np.array_equal(v2.view(np.uint64), v.view(np.uint64)), seed
