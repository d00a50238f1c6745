"""Host restatement of mgs_csr_extract, mgs_csr_extract_info, mgs_vec_gather and mgs_vec_scatter (include/mgs.h), and the fixtures their
CPU and GPU tests share.

extract(A, rows, cols): row k of S is row rows[k] of A restricted to the listed columns, column cols[q] renumbered to q; rows in any order,
repeats allowed, cols strictly ascending; None means every row / every column.  Values are moved by position (numpy fancy indexing copies
the eight bytes), so −0.0 and NaN payloads stay.  src[k] is the position in A's arrays of entry k of S — what keep_map keeps.

A matrix here is the tuple (rows, cols, rowptr, col, val) with int32 / float64 arrays, as in tests/spgemm_ref.py.
"""
import numpy as np
import scipy.sparse as sps

from csr_algebra_ref import EMPTY, fx_rect as algebra_rect, rows_to_csr
from spgemm_ref import csr, pick, to_scipy, with_values  # noqa: F401  (shared helpers, re-exported)

LANE_LEN = 64      # source rows of at most this many entries are counted by one lane, longer ones by one wave


def extract(A, rows=None, cols=None):
    """the restatement → (nr, nc, rowptr, col, val, src)"""
    m, n, rp, ci, v = A
    rows = np.arange(m, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    if cols is None:
        nc, cmap = n, np.arange(n, dtype=np.int64)
    else:
        cols = np.asarray(cols, dtype=np.int64)
        nc, cmap = len(cols), np.full(n, -1, dtype=np.int64)
        cmap[cols] = np.arange(nc)
    srp, scol, src = [0], [], []
    for r in rows:
        seg = np.arange(int(rp[r]), int(rp[r + 1]), dtype=np.int64)
        q = cmap[ci[seg]]
        keep = q >= 0
        scol.append(q[keep]); src.append(seg[keep])
        srp.append(srp[-1] + int(keep.sum()))
    scol = np.concatenate(scol + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    src = np.concatenate(src + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    return len(rows), nc, np.asarray(srp, dtype=np.int32), scol, np.asarray(v, dtype=np.float64)[src], src


def matrix(S):
    """the (rows, cols, rowptr, col, val) part of extract's result"""
    return S[:5]


def refusal(A, rows=None, cols=None):
    """None, or what mgs_csr_extract names: ("row", position, value), ("column", position, value) or ("ascending", position, value) —
    a row violation first, else the column violation at the lowest position (out of range before not ascending at one position)"""
    m, n = A[0], A[1]
    if rows is not None:
        for k, r in enumerate(np.asarray(rows, dtype=np.int64)):
            if r < 0 or r >= m:
                return "row", k, int(r)
    if cols is not None:
        cols = np.asarray(cols, dtype=np.int64)
        for q, c in enumerate(cols):
            if c < 0 or c >= n:
                return "column", q, int(c)
            if q > 0 and cols[q - 1] >= c:
                return "ascending", q, int(c)
    return None


def info(A, rows=None, cols=None, keep_map=False):
    """what mgs_csr_extract_info reports for the block"""
    S = extract(A, rows, cols)
    lens = np.diff(S[2])
    srclen = np.diff(A[2])[np.arange(A[0]) if rows is None else np.asarray(rows, dtype=np.int64)]
    lane = int((srclen <= LANE_LEN).sum()) if cols is not None else 0
    wave = int((srclen > LANE_LEN).sum()) if cols is not None else 0
    return {"lane_rows": lane, "wave_rows": wave, "max_row_len": int(lens.max()) if len(lens) else 0, "map_bytes": 4 * len(S[3]) if keep_map else 0}


def gather(x, idx):
    """(y, bad): y[k] = x[idx[k]], +0.0 where idx[k] lies outside x; bad counts those"""
    x = np.asarray(x, dtype=np.float64); idx = np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0) & (idx < len(x))
    y = np.zeros(len(idx))
    y[ok] = x[idx[ok]]
    return y, int((~ok).sum())


def scatter(x, idx, y):
    """(x', bad): x'[idx[k]] = y[k] for distinct indices, indices outside x skipped; bad counts those"""
    out = np.asarray(x, dtype=np.float64).copy(); idx = np.asarray(idx, dtype=np.int64); y = np.asarray(y, dtype=np.float64)
    ok = (idx >= 0) & (idx < len(out))
    assert len(np.unique(idx[ok])) == int(ok.sum()), "scatter: the indices must be distinct"
    out[idx[ok]] = y[: len(idx)][ok]
    return out, int((~ok).sum())


def tagged(A):
    """A with its values replaced by distinct non-zero tags 1, 2, 3, …: a stored zero is then no question for scipy"""
    return with_values(A, np.arange(1, len(A[3]) + 1, dtype=np.float64))


# ------------------------------------------------------------------ fixtures
NAN_BITS = 0x7FF8000000ABCDEF      # a quiet NaN with a payload


def nan_with_payload():
    return np.array([NAN_BITS], dtype=np.uint64).view(np.float64)[0]


def poisson3d(N):
    """the 7-point operator of mgs_csr_poisson3d: diagonal 6, off-diagonals −1, row e = (i·N + j)·N + k, ascending columns"""
    I = sps.identity(N); T = sps.diags([-1.0, -1.0], [-1, 1], shape=(N, N))
    return csr(sps.kron(sps.kron(T, I), I) + sps.kron(sps.kron(I, T), I) + sps.kron(sps.kron(I, I), T) + 6.0 * sps.identity(N ** 3))


def fx_poisson8():
    """(A, fixed, free): Poisson on 8³, the 64 rows of plane i = 0 and the other 448"""
    return poisson3d(8), np.arange(64, dtype=np.int32), np.arange(64, 512, dtype=np.int32)


def fx_poisson8_values(seed=0):
    """diagonally dominant random values on the 8³ pattern (a hierarchy is built on a block of it): one pattern, a set of values per seed"""
    A = poisson3d(8)
    rng = np.random.default_rng(1908 + seed)
    v = np.where(A[4] > 0, 6.0 + rng.random(len(A[4])), -(0.5 + 0.5 * rng.random(len(A[4]))))
    return with_values(A, v)


def fx_rect():
    """(A, rows, cols): the 37 × 53 matrix of the sums' tests (rows 3, 20 and 36 empty), a row list that descends and repeats rows and
    reaches the empty ones, an ascending column list that leaves out most columns"""
    A = algebra_rect()[1]
    rows = np.array([36, 30, 30, 21, 20, 20, 11, 3, 3, 0], dtype=np.int32)
    cols = np.array([0, 1, 2, 5, 8, 13, 21, 22, 23, 34, 40, 41, 52], dtype=np.int32)
    return A, rows, cols


def fx_boundary():
    """(A, rows, cols): source rows of 64 entries (the last lane row) and 65 (the first wave row) in 200 columns; every other column listed"""
    rng = np.random.default_rng(6465)
    A = rows_to_csr([pick(rng, 0, 200, 64), pick(rng, 0, 200, 65)], 200, rng)
    return A, None, np.arange(0, 200, 2, dtype=np.int32)


WAVE_LONG = 64 * 3 + 17


def fx_wave():
    """(A, rows, cols): row 0 holds 64·3 + 17 entries in 1000 columns.  The column list takes some entries (20 at least) of its first
    chunk of 64, nothing of the second, all 64 of the third and some (5 at least) of the last 17, and lists columns the row does not
    store.  A −0.0 and a NaN with a payload sit among the kept values of the third chunk.  Row 1 is short, row 2 empty, row 3 holds 130
    entries of which every third is listed (those in row 0's second chunk excepted).  The row list selects row 0 twice."""
    rng = np.random.default_rng(20917)
    n = 1000
    r0 = pick(rng, 0, n, WAVE_LONG)
    others = np.setdiff1d(np.arange(n), r0)
    r3 = np.sort(np.r_[rng.choice(r0, size=40, replace=False), rng.choice(others, size=90, replace=False)])
    cols = np.unique(np.r_[r0[rng.choice(64, size=20, replace=False)], r0[128:192], r0[192 + rng.choice(17, size=5, replace=False)],
                           rng.choice(others, size=30, replace=False), r3[::3]])
    cols = np.setdiff1d(cols, r0[64:128])      # r3 may have brought columns of the second chunk back
    A = rows_to_csr([r0, np.array([1, 7, int(r0[130])]), EMPTY, r3], n, rng)
    A[4][128 + 5] = -0.0
    A[4][128 + 40] = nan_with_payload()
    return A, np.array([0, 1, 0, 2, 3], dtype=np.int32), cols.astype(np.int32)


def fx_vectors():
    """(x, idx, y): a vector of 300 entries with a −0.0 and a NaN, 120 indices with repeats for the gather (the first 100 are distinct,
    for the scatter), 100 values to scatter"""
    rng = np.random.default_rng(3001)
    x = rng.standard_normal(300)
    x[17] = -0.0; x[40] = nan_with_payload()
    distinct = rng.permutation(300)[:100]
    distinct[:2] = [17, 40]
    idx = np.r_[distinct, rng.choice(distinct, size=20)]
    return x, idx.astype(np.int32), rng.standard_normal(100)


# every fixture whose blocks the tests compare with scipy (CPU) and bit for bit with the device (GPU): name → (A, rows, cols)
BLOCK_FIXTURES = {
    "poisson_ff": lambda: (fx_poisson8()[0], fx_poisson8()[2], fx_poisson8()[2]),
    "poisson_fc": lambda: (fx_poisson8()[0], fx_poisson8()[2], fx_poisson8()[1]),
    "poisson_cf": lambda: (fx_poisson8()[0], fx_poisson8()[1], fx_poisson8()[2]),
    "poisson_cc": lambda: (fx_poisson8()[0], fx_poisson8()[1], fx_poisson8()[1]),
    "rect_rows": lambda: (fx_rect()[0], fx_rect()[1], None),
    "rect_cols": lambda: (fx_rect()[0], None, fx_rect()[2]),
    "rect_both": fx_rect,
    "rect_all": lambda: (fx_rect()[0], None, None),
    "boundary": fx_boundary,
    "wave": fx_wave,
}
