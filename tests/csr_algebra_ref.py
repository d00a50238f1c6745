"""Host restatement of the arithmetic of mgs_csr_add, mgs_csr_scale and mgs_csr_diag (include/mgs.h), and the fixtures their CPU and GPU
tests share.

add(alpha, A, beta, B): the union of the two stored patterns, columns ascending; an entry stored only in A is fl(alpha·a), only in B
fl(beta·b), in both fl(fl(alpha·a) + fl(beta·b)).  Every np.float64 operation below is one rounding; the three cases are written into
their places separately (never as 0 + x, which would turn a lone −0.0 into +0.0).
scale(A, dl, dr): fl(fl(dl_i·a_ij)·dr_j), a factor that is None is skipped.

A matrix here is the tuple (rows, cols, rowptr, col, val) with int32 / float64 arrays, as in tests/spgemm_ref.py.
"""
import numpy as np
import scipy.sparse as sps

from spgemm_ref import csr, pick, poisson3d_pattern, to_scipy, with_values  # noqa: F401  (shared helpers, re-exported)

LANE_U = 64      # rows with len_A + len_B of at most this are merged by one lane


def rows_of(A):
    return np.repeat(np.arange(A[0], dtype=np.int64), np.diff(A[2]))


def add(alpha, A, beta, B):
    """the restatement"""
    m, n, arp, aci, av = A
    m2, n2, brp, bci, bv = B
    assert (m, n) == (m2, n2)
    alpha, beta = np.float64(alpha), np.float64(beta)
    ka = rows_of(A) * n + aci.astype(np.int64)
    kb = rows_of(B) * n + bci.astype(np.int64)
    keys = np.union1d(ka, kb)                            # sorted by (row, column)
    pa, pb = np.searchsorted(keys, ka), np.searchsorted(keys, kb)
    with np.errstate(all="ignore"):
        ta = alpha * np.asarray(av, dtype=np.float64)    # fl(alpha·a)
        tb = beta * np.asarray(bv, dtype=np.float64)     # fl(beta·b)
        in_a = np.zeros(len(keys), dtype=bool); in_a[pa] = True
        in_b = np.zeros(len(keys), dtype=bool); in_b[pb] = True
        val = np.empty(len(keys), dtype=np.float64)
        val[pa] = ta                                     # only in A (the common places are overwritten below)
        only_b = ~in_a[pb]
        val[pb[only_b]] = tb[only_b]                     # only in B
        both_a, both_b = in_b[pa], in_a[pb]              # the common entries, in the same (ascending) order on either side
        val[pa[both_a]] = ta[both_a] + tb[both_b]        # fl(fl(alpha·a) + fl(beta·b))
    rp = np.searchsorted(keys // n if n else keys, np.arange(m + 1)).astype(np.int32)
    return m, n, rp, (keys % n if n else keys).astype(np.int32), val


def add_info(A, B):
    """what mgs_csr_add_info reports for A + B"""
    u = np.diff(A[2]).astype(np.int64) + np.diff(B[2])
    C = add(1.0, A, 1.0, B)
    lens = np.diff(C[2])
    return {"lane_rows": int((u <= LANE_U).sum()), "wave_rows": int((u > LANE_U).sum()), "max_row_len": int(lens.max()) if len(lens) else 0,
            "common_entries": int(len(A[3]) + len(B[3]) - len(C[3]))}


def scale(A, dl=None, dr=None, right_first=False):
    """the restatement; right_first multiplies a·dr first (the order-sensitivity probe)"""
    m, n, rp, ci, v = A
    v = np.asarray(v, dtype=np.float64).copy()
    with np.errstate(all="ignore"):
        if right_first and dl is not None and dr is not None:
            v = np.asarray(dl, dtype=np.float64)[rows_of(A)] * (v * np.asarray(dr, dtype=np.float64)[ci])
        else:
            if dl is not None:
                v = np.asarray(dl, dtype=np.float64)[rows_of(A)] * v
            if dr is not None:
                v = v * np.asarray(dr, dtype=np.float64)[ci]
    return m, n, rp, ci, v


def diag(A):
    m, n, rp, ci, v = A
    d = np.zeros(min(m, n))
    on = (rows_of(A) == ci)
    d[ci[on]] = v[on]
    return d


# ------------------------------------------------------------------ fixtures
ALPHA, BETA = 1.0 / 3.0, 0.7      # neither product is exact for a random normal: both roundings and the sum's show


def normals(rng, n):
    return rng.standard_normal(n)


def rows_to_csr(rows, ncols, rng):
    """rows: one sorted array of distinct columns per row; random normal values"""
    rp = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
    ci = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows] + [np.zeros(0, dtype=np.int32)])
    return len(rows), ncols, rp, ci, normals(rng, len(ci))


EMPTY = np.zeros(0, dtype=np.int32)


def fx_lane():
    """the 7-point pattern on 8³ plus a 512 × 512 pattern with 5 entries per row, two of them on the row's stencil columns"""
    rng = np.random.default_rng(1801)
    P = poisson3d_pattern(8)
    A = with_values(P, normals(rng, len(P[3])))
    rows = []
    for i in range(512):
        stencil = P[3][P[2][i]:P[2][i + 1]]
        on = rng.choice(stencil, size=2, replace=False)
        off = rng.choice(np.setdiff1d(np.arange(512), on), size=3, replace=False)
        rows.append(np.sort(np.r_[on, off]))
    return ALPHA, A, BETA, rows_to_csr(rows, 512, rng)


def fx_rect():
    """37 × 53: row 3 empty in A only, row 11 in B only, row 20 in both; row 36 (the last) empty in A"""
    rng = np.random.default_rng(13753)
    m, n = 37, 53
    arows = [pick(rng, 0, n, int(rng.integers(1, 9))) for _ in range(m)]
    brows = [np.union1d(pick(rng, 0, n, int(rng.integers(1, 6))), arows[i][:2]) for i in range(m)]      # two common columns per row at least
    arows[3] = EMPTY; brows[11] = EMPTY; arows[20] = EMPTY; brows[20] = EMPTY; arows[36] = EMPTY
    return ALPHA, rows_to_csr(arows, n, rng), BETA, rows_to_csr(brows, n, rng)


def fx_boundary():
    """row 0: 40 + 24 = 64 entries (the last lane row), row 1: 40 + 25 = 65 (the first wave row); ten common columns in each"""
    rng = np.random.default_rng(16465)
    n = 200
    arows, brows = [], []
    for lb in (24, 25):
        a = pick(rng, 0, n, 40)
        b = np.union1d(rng.choice(a, size=10, replace=False), rng.choice(np.setdiff1d(np.arange(n), a), size=lb - 10, replace=False))
        arows.append(a); brows.append(b)
    return ALPHA, rows_to_csr(arows, n, rng), BETA, rows_to_csr(brows, n, rng)


def fx_wave():
    """the wave path: row 0 (150, 131) with 40 common columns spread over every chunk of 64 on either side (the largest column is common);
    row 1 (100, 100) with identical columns; row 2 (90, 90) even against odd columns; row 3 (70, 40) where only the first and the last
    column match; row 4 (60, 50) with all of B's columns below all of A's; row 5 short (a lane row between them); row 6 empty"""
    rng = np.random.default_rng(15013)
    n = 1000
    a0 = np.r_[pick(rng, 0, n - 1, 149), n - 1]
    common = a0[np.r_[np.linspace(0, 148, 39).astype(int), 149]]
    b0 = np.union1d(common, rng.choice(np.setdiff1d(np.arange(n), a0), size=131 - 40, replace=False))
    a1 = pick(rng, 0, n, 100)
    a2 = 2 * pick(rng, 0, n // 2, 90); b2 = a2 + 1
    inner = rng.permutation(np.arange(6, 990))
    a3 = np.r_[5, np.sort(inner[:68]), 990]; b3 = np.r_[5, np.sort(inner[68:106]), 990]
    a4 = pick(rng, 500, n, 60); b4 = pick(rng, 0, 100, 50)
    a5 = np.array([1, 7, 9]); b5 = np.array([0, 7])
    arows = [a0, a1, a2, a3, a4, a5, EMPTY]
    brows = [b0, a1.copy(), b2, b3, b4, b5, EMPTY]
    return ALPHA, rows_to_csr(arows, n, rng), BETA, rows_to_csr(brows, n, rng)


def fx_long():
    """3 × 20000 with a (5000, 4000) row, about a quarter of B's columns common: no limit on the length of a row"""
    rng = np.random.default_rng(15004)
    n = 20000
    a = pick(rng, 0, n, 5000)
    b = np.union1d(rng.choice(a, size=1000, replace=False), rng.choice(np.setdiff1d(np.arange(n), a), size=3000, replace=False))
    return ALPHA, rows_to_csr([np.array([3, 19999]), a, EMPTY], n, rng), BETA, rows_to_csr([np.array([3]), b, EMPTY], n, rng)


def fx_special():
    """2 × 3: A[0] = (x at 0, −0.0 at 1), A[1] = (y at 2); B[0] = (x at 0), B[1] = (0.0 at 0, y at 2).  With alpha = 1, beta = −1: (0, 0) and
    (1, 2) cancel to +0.0 and stay entries, (0, 1) is a lone −0.0 of A, (1, 0) a lone −0.0 of B (−1 · 0.0)"""
    x, y = 1.7, -0.3
    A = (2, 3, np.array([0, 2, 3], dtype=np.int32), np.array([0, 1, 2], dtype=np.int32), np.array([x, -0.0, y]))
    B = (2, 3, np.array([0, 1, 3], dtype=np.int32), np.array([0, 0, 2], dtype=np.int32), np.array([x, 0.0, y]))
    return 1.0, A, -1.0, B


def fx_numeric(seed=0):
    """one pair of patterns (the wave fixture's, so both kernels run), a set of values and scalars per seed"""
    _, A, _, B = fx_wave()
    rng = np.random.default_rng(2500 + seed)
    alpha, beta = (ALPHA, BETA) if seed == 0 else (-0.9, 1.0 / 7.0)
    return alpha, with_values(A, normals(rng, len(A[3]))), beta, with_values(B, normals(rng, len(B[3])))


def fx_scale():
    """the rectangular fixture's A with random normal scalings"""
    _, A, _, _ = fx_rect()
    rng = np.random.default_rng(3753)
    return A, normals(rng, A[0]), normals(rng, A[1])


def fx_missing_diag():
    """6 × 4: rows 1 and 3 store no diagonal entry, rows 4 and 5 lie below the square part; a stored 0.0 on the diagonal of row 2"""
    rows = [np.array([0, 2]), np.array([0, 3]), np.array([1, 2, 3]), np.array([0, 1]), np.array([3]), EMPTY]
    A = rows_to_csr(rows, 4, np.random.default_rng(64))
    A[4][5] = 0.0
    return A


def fx_compose():
    """a random 40 × 25 B (about five entries per row) and a positive diagonal d of 25 entries: S = (B·D⁻¹)·Bᵀ"""
    rng = np.random.default_rng(4025)
    rows = [pick(rng, 0, 25, int(rng.integers(2, 9))) for _ in range(40)]
    return rows_to_csr(rows, 25, rng), 0.5 + rng.random(25)


# every fixture whose sums the GPU tests compare bit for bit with the restatement
VALUE_FIXTURES = {
    "lane": fx_lane,
    "rect": fx_rect,
    "boundary": fx_boundary,
    "wave": fx_wave,
    "long": fx_long,
    "numeric0": lambda: fx_numeric(0),
    "numeric1": lambda: fx_numeric(1),
}
