"""Host restatement of the arithmetic of mgs_csr_spgemm (include/mgs.h), and the fixtures the product's CPU and GPU tests share.

spgemm(A, B): row i of C visits the entries (i, l) of A in storage order and for each the entries (l, j) of B in storage order; every
product is one np.float64 multiplication; the first product that reaches column j is stored, later ones are added in the order met;
the columns of a row come out ascending.  Plain loops and a dict per row — slow and obvious on purpose.

A matrix here is the tuple (rows, cols, rowptr, col, val) with int32 / float64 arrays.
"""
import numpy as np
import scipy.sparse as sps

MAX_ROW = 8192      # MGS_SPGEMM_MAX_ROW


def csr(M):
    """(rows, cols, rowptr, col, val) of a scipy matrix, columns ascending, explicit zeros kept"""
    M = sps.csr_matrix(M)
    M.sort_indices()
    return M.shape[0], M.shape[1], M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64)


def to_scipy(A):
    m, n, rp, ci, v = A
    return sps.csr_matrix((v, ci, rp), shape=(m, n))


def spgemm(A, B, reverse_a=False):
    """the restatement; reverse_a visits every row of A back to front (the order-sensitivity probe)"""
    m, k, arp, aci, av = A
    k2, n, brp, bci, bv = B
    assert k == k2
    av = np.asarray(av, dtype=np.float64); bv = np.asarray(bv, dtype=np.float64)
    rp, ci, val = [0], [], []
    with np.errstate(all="ignore"):
        for i in range(m):
            acc = {}
            ks = range(int(arp[i]), int(arp[i + 1]))
            for ka in (reversed(ks) if reverse_a else ks):
                l, a = int(aci[ka]), av[ka]
                for kb in range(int(brp[l]), int(brp[l + 1])):
                    j, p = int(bci[kb]), a * bv[kb]
                    acc[j] = acc[j] + p if j in acc else p
            for j in sorted(acc):
                ci.append(j); val.append(acc[j])
            rp.append(len(ci))
    return m, n, np.asarray(rp, dtype=np.int32), np.asarray(ci, dtype=np.int32), np.asarray(val, dtype=np.float64)


def galerkin(A, P):
    """(Pᵀ·A)·P in the product's order — what mgs_csr_galerkin computes for a P that is not an aggregation"""
    Pt = csr(to_scipy(P).T)
    return spgemm(spgemm(Pt, A), P)


def row_products(A, B):
    """ub_i = Σ_l len(B_l) over the entries (i, l) of A"""
    m, _, arp, aci, _ = A
    blen = np.diff(B[2])
    return np.array([int(blen[aci[arp[i]:arp[i + 1]]].sum()) for i in range(m)], dtype=np.int64)


# ------------------------------------------------------------------ fixtures
def wide(rng, n, decades=8):
    """values with a wide exponent range: the order of a sum shows in its last bits (fewer decades where a row has few sums: across
    sixteen decades most three-term sums are absorbed by their largest term and do not show the order)"""
    return rng.standard_normal(n) * 10.0 ** rng.integers(-decades, decades, n)


def with_values(M, vals):
    m, n, rp, ci, _ = M
    return m, n, rp, ci, np.asarray(vals, dtype=np.float64)


def poisson3d_pattern(N):
    I = sps.identity(N); T = sps.diags([1, 1], [-1, 1], shape=(N, N))
    L = sps.kron(sps.kron(T, I), I) + sps.kron(sps.kron(I, T), I) + sps.kron(sps.kron(I, I), T) + sps.identity(N ** 3)
    return csr(L)


def poisson2d(n):
    I = sps.identity(n); T = sps.diags([-1, -1], [-1, 1], shape=(n, n))
    return csr(sps.kron(I, sps.diags([4.0], [0], shape=(n, n)) + T) + sps.kron(T, I))


def fx_poisson8():
    """the 7-point pattern on 8³ times itself with wide random values: every row has at most 49 products"""
    rng = np.random.default_rng(801)
    P = poisson3d_pattern(8)
    return with_values(P, wide(rng, len(P[3]))), with_values(P, wide(rng, len(P[3])))


def rows_to_csr(rows, ncols, rng, decades=8):
    """rows: one sorted array of distinct columns per row"""
    rp = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
    ci = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows] + [np.zeros(0, dtype=np.int32)])
    return len(rows), ncols, rp, ci, wide(rng, len(ci), decades)


def pick(rng, lo, hi, count):
    return np.sort(rng.choice(np.arange(lo, hi), size=count, replace=False))


def fx_rect():
    """37 × 53 times 53 × 29: empty rows of A (3, 11), empty rows of B that A selects (5, 20), a product row that is empty although its
    row of A is not (row 7 selects only B's empty rows)"""
    rng = np.random.default_rng(3753)
    m, k, n = 37, 53, 29
    brows = [pick(rng, 0, n, int(rng.integers(1, 9))) for _ in range(k)]
    brows[5] = np.zeros(0, dtype=np.int32); brows[20] = np.zeros(0, dtype=np.int32)
    arows = [pick(rng, 0, k, int(rng.integers(1, 8))) for _ in range(m)]
    arows[3] = np.zeros(0, dtype=np.int32); arows[11] = np.zeros(0, dtype=np.int32)
    arows[7] = np.array([5, 20], dtype=np.int32)
    arows[9] = np.array([4, 5, 30], dtype=np.int32)
    return rows_to_csr(arows, k, rng), rows_to_csr(brows, n, rng)


def fx_boundary():
    """row 0: 4 rows of B with 16 entries each inside 24 columns, 64 products (the last lane row); row 1: 5 rows of B with 13 entries
    each inside 20 columns, 65 products and fewer than 64 distinct columns (the first workgroup row).  Most columns receive three or
    more products: two-term sums commute and would not show the order."""
    rng = np.random.default_rng(6465)
    n = 100
    brows = [pick(rng, 0, 24, 16) for _ in range(4)] + [pick(rng, 50, 70, 13) for _ in range(5)]
    arows = [np.arange(0, 4), np.arange(4, 9)]
    return rows_to_csr(arows, 9, rng, 2), rows_to_csr(brows, n, rng, 2)


def fx_wide():
    """the workgroup path over several steps: row 0 of A has 5 entries, each selects a row of B with 800 entries in a window of 1600
    columns; the windows start 650 columns apart, so a column lies in up to three of them (three-term sums) and new columns are first
    met in every step; about 2900 distinct columns.  Row 1: three steps; row 2: empty."""
    rng = np.random.default_rng(3000)
    n = 4200
    brows = [pick(rng, 650 * r, 650 * r + 1600, 800) for r in range(5)]
    arows = [np.arange(5), np.array([0, 1, 2]), np.zeros(0, dtype=np.int32)]
    return rows_to_csr(arows, 5, rng), rows_to_csr(brows, n, rng)


def fx_limit(length=MAX_ROW):
    """a 2 × 1 A whose row 0 selects a row of B with `length` entries"""
    rng = np.random.default_rng(8192)
    n = 9000
    return rows_to_csr([np.array([0]), np.zeros(0, dtype=np.int32)], 1, rng), rows_to_csr([pick(rng, 0, n, length)], n, rng)


def fx_limit_row3():
    """6 × 2 A: rows 3 and 5 select the row of B with MAX_ROW + 1 entries, the others a short one"""
    rng = np.random.default_rng(8193)
    n = 9000
    arows = [np.array([0]), np.array([0]), np.zeros(0, dtype=np.int32), np.array([0, 1]), np.array([0]), np.array([1])]
    return rows_to_csr(arows, 2, rng), rows_to_csr([pick(rng, 0, n, 10), pick(rng, 0, n, MAX_ROW + 1)], n, rng)


def fx_zeros():
    """C[0, 0] = a·b + (−a)·b = 0.0 stays an entry; C[1, 1] = (−1.0)·0.0 is a lone −0.0"""
    a, b = 1.7, 0.3
    A = (2, 2, np.array([0, 2, 3], dtype=np.int32), np.array([0, 1, 0], dtype=np.int32), np.array([a, -a, -1.0]))
    B = (2, 2, np.array([0, 2, 3], dtype=np.int32), np.array([0, 1, 0], dtype=np.int32), np.array([b, 0.0, b]))
    return A, B


def fx_numeric(seed=0):
    """5-point pattern on 24², diagonally dominant random values (a hierarchy is built on the product): one pattern, a set of values
    per seed"""
    rng = np.random.default_rng(2400 + seed)
    m, n, rp, ci, v = poisson2d(24)
    def vals():
        off = -(0.5 + rng.random(len(v)))
        return np.where(v > 0, 4.0 + rng.random(len(v)), off)
    return (m, n, rp, ci, vals()), (m, n, rp, ci, vals())


def general_P(n, nc):
    """the two-entries-per-row P of test_gpu_parity.py::test_general_P_fallback"""
    rows = np.repeat(np.arange(n), 2)
    cols = np.stack([np.arange(n) // 4, (np.arange(n) // 4 + 1) % nc], 1).ravel()
    return csr(sps.csr_matrix((np.tile([0.75, 0.25], n), (rows, cols)), shape=(n, nc)))


# every fixture whose values the GPU tests compare bit for bit with the restatement
NUMERIC_FIXTURES = {
    "poisson8": fx_poisson8,
    "rect": fx_rect,
    "boundary": fx_boundary,
    "wide": fx_wide,
    "numeric0": lambda: fx_numeric(0),
    "numeric1": lambda: fx_numeric(1),
}
