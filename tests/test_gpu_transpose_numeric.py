"""mgs_csr_transpose_numeric: the values of a transposed matrix again, in place, from the current values of its source.

CPU: the restatement (tests/transpose_ref.py: two bisections per entry, the miss count) against scipy's A.T.tocsr().
GPU: after update_values on A, transpose_update(check=True) leaves all three arrays of At bit-equal to a fresh transpose() — on
saddle(7)'s D (172 × 343, rectangular), on a matrix with a row of 200 entries, an empty row and an empty column, on 1 × 1 and on a
matrix without entries; values include −0.0 and a NaN with a payload.  A twin of the same shape and entry count but another pattern is
refused with MGS_ERR_STATE and the restatement's miss count, and what it did place is the restatement's.  Every refusal is checked."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

from minres_ref import saddle
from transpose_ref import transpose_numeric_ref

INVALID, STATE = -1, -6
NAN_PAYLOAD = np.array([0x7FF8_0000_DEAD_BEEF], dtype=np.uint64).view(np.float64)[0]


def long_row_matrix():
    """40 × 260: row 3 holds 200 entries, row 5 is empty, column 7 is empty, the rest a seeded sprinkle"""
    rng = np.random.default_rng(11)
    M = sps.random(40, 260, density=0.03, random_state=rng, format="lil")
    M[3, :] = 0.0
    M[3, 20:220] = 1.0
    M[5, :] = 0.0
    M[:, 7] = 0.0
    M = M.tocsr(); M.eliminate_zeros(); M.sort_indices()
    assert M.indptr[4] - M.indptr[3] == 200 and M.indptr[6] == M.indptr[5] and not (M.indices == 7).any()
    return M


def cases():
    D = saddle(7)["D"]
    assert D.shape == (172, 343)
    return {"saddle(7).D": D.tocsr(), "long row": long_row_matrix(), "1 x 1": sps.csr_matrix(np.array([[2.5]])),
            "no entries": sps.csr_matrix((5, 3))}


def new_values(nnz, seed):
    v = np.random.default_rng(seed).standard_normal(nnz)
    if nnz > 0:
        v[0] = -0.0
    if nnz > 2:
        v[nnz // 2] = NAN_PAYLOAD
    return v


def arrays(M):
    return M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64)


@pytest.mark.parametrize("name", list(cases()))
def test_restatement_against_scipy(name):
    A = cases()[name]
    rp, ci, _ = arrays(A)
    v = new_values(A.nnz, 1)
    # the pattern of the transpose from scipy, with values that must all be overwritten
    T = sps.csr_matrix((np.arange(1, A.nnz + 1, dtype=np.float64), ci, rp), shape=A.shape).T.tocsr(); T.sort_indices()
    got, misses = transpose_numeric_ref(A.shape, rp, ci, v, T.indptr, T.indices, np.full(A.nnz, 123.0))
    want = v[(T.data - 1).astype(np.int64)] if A.nnz else v      # T.data holds 1 + the source position of every entry
    assert misses == 0 and got.tobytes() == want.tobytes()


def twin_of(A):
    """same shape and entry count, another pattern: every column moved one to the right, cyclically"""
    rp, ci, v = arrays(A)
    return sps.csr_matrix((v, (ci + 1) % A.shape[1], rp), shape=A.shape)


def test_restatement_counts_misses():
    A = cases()["saddle(7).D"]
    B = twin_of(A); B.sort_indices()
    assert B.nnz == A.nnz and B.shape == A.shape
    T = A.T.tocsr(); T.sort_indices()
    rp, ci, v = arrays(B)
    got, misses = transpose_numeric_ref(B.shape, rp, ci, v, T.indptr, T.indices, np.full(A.nnz, 123.0))
    both = (abs(A) .multiply(abs(B)) != 0).nnz
    assert misses == A.nnz - both and 0 < misses
    assert (got != 123.0).sum() == both


# ------------------------------------------------------------------------------------------------------------------- the device
@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


def dev(ctx, M):
    return ctx.csr(M.shape[0], M.shape[1], *arrays(M))


def same_arrays(X, Y):
    a, b = X.download(), Y.download()
    return all(p.tobytes() == q.tobytes() for p, q in zip(a, b)) and X.shape == Y.shape


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases()))
def test_same_bits_as_a_fresh_transpose(ctx, mg, name):
    M = cases()[name]
    A = dev(ctx, M)
    At = A.transpose()
    rp0, ci0, _ = At.download()
    ptrs = At.device_ptrs()
    v = new_values(M.nnz, 2)
    if M.nnz:
        A.update_values(v)
    assert At.transpose_update(A, check=True) is At
    fresh = A.transpose()
    assert same_arrays(At, fresh), name
    assert At.device_ptrs() == ptrs                       # nothing moved
    rp, ci, tv = At.download()
    want, misses = transpose_numeric_ref(M.shape, *arrays(M)[:2], v, rp0, ci0, np.zeros(M.nnz))
    assert misses == 0 and tv.tobytes() == want.tobytes() and np.array_equal(rp, rp0) and np.array_equal(ci, ci0)
    if M.nnz > 2:
        bits = tv.view(np.uint64)
        assert (bits == np.uint64(0x7FF8_0000_DEAD_BEEF)).sum() == 1 and (bits == np.uint64(1) << np.uint64(63)).sum() == 1
    # the enqueue-only form, twice: the same bits
    if M.nnz:
        A.update_values(new_values(M.nnz, 3))
    At.transpose_update(A).transpose_update(A)
    assert same_arrays(At, A.transpose())


@pytest.mark.gpu
def test_another_pattern_is_counted_and_never_written(ctx, mg):
    M = cases()["saddle(7).D"]
    B = twin_of(M); B.sort_indices()
    A, Bd = dev(ctx, M), dev(ctx, B)
    At = A.transpose()
    rp, ci, before = At.download()
    want, misses = transpose_numeric_ref(B.shape, *arrays(B), rp, ci, before)
    with pytest.raises(mg.MgsError) as e:
        At.transpose_update(Bd, check=True)
    print(f"twin: {e.value} (restatement: {misses} misses)")
    assert e.value.code == STATE and e.value.misses == misses and str(misses) in str(e.value) and "mgs_csr_transpose_numeric" in str(e.value)
    rp2, ci2, after = At.download()
    assert after.tobytes() == want.tobytes() and np.array_equal(rp2, rp) and np.array_equal(ci2, ci)
    # without the count the call is enqueued and reports nothing
    At.transpose_update(Bd)
    assert At.download()[2].tobytes() == want.tobytes()


@pytest.mark.gpu
def test_refusals(ctx, mg):
    L = mg.lib()
    M = cases()["saddle(7).D"]
    A = dev(ctx, M)
    At = A.transpose()
    before = At.download()[2].tobytes()

    def refused(word, a, at):
        miss = C.c_int64(-5)
        assert L.mgs_csr_transpose_numeric(a, at, C.byref(miss)) == INVALID
        msg = L.mgs_last_error(ctx.h).decode()
        assert "mgs_csr_transpose_numeric" in msg and word in msg, msg
        assert miss.value == -5
    refused("NULL", None, At.h)
    refused("NULL", A.h, None)
    refused("not 343 x 172", A.h, A.h)                                               # At is not cols × rows of A
    narrow = dev(ctx, sps.csr_matrix((343, 171)))                                    # (the handles stay referenced across the calls)
    refused("not 343 x 172", A.h, narrow.h)
    fewer = M.tolil(); fewer[0, 0] = 0.0; fewer = fewer.tocsr(); fewer.eliminate_zeros()
    Af = dev(ctx, fewer)
    refused("entries", Af.h, At.h)                                                   # different entry counts
    c2 = mg.Context(0)
    try:
        other = dev(c2, M.T.tocsr())
        refused("different context", A.h, other.h)
        del other
        c2.set_option("valcode", 1)
        P = c2.poisson3d(8)
        Pt = P.transpose().optimize()
        assert Pt.rowcode_info()["coded_blocks"] > 0
        with pytest.raises(mg.MgsError) as e:
            Pt.transpose_update(P)
        assert e.value.code == INVALID and "valcode" in str(e.value)
        del P, Pt
    finally:
        c2.close()
    assert At.download()[2].tobytes() == before
