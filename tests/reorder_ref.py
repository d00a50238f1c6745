"""Host restatement of mgs_csr_permute, mgs_csr_permute_info, mgs_csr_bmat and mgs_csr_bmat_info (include/mgs.h), of the refusals the
device must give, and the fixtures their CPU and GPU tests share.

permute_ref(A, rperm, cperm): C[i, j] = A[rperm[i], cperm[j]] — row i of C holds the entries of A's row rperm[i], every column mapped
through the inverse of cperm, in ascending order of the new column; None is the identity.  An entry's place is its rank among the new
columns of its row (a stable argsort of distinct keys).  Values are moved by position (numpy fancy indexing copies the eight bytes), so
−0.0 and NaN payloads stay.  src[k] is the position in A's arrays of entry k of C — what keep_map keeps.

bmat_ref(grid, row_sizes, col_sizes): row roff_I + i of C is the concatenation over J of row i of block (I, J) with coff_J added to its
columns; None is a zero block.

A matrix here is the tuple (rows, cols, rowptr, col, val) with int32 / float64 arrays, as in tests/spgemm_ref.py.
"""
import numpy as np
import scipy.sparse as sps

from extract_ref import NAN_BITS, nan_with_payload, poisson3d  # noqa: F401  (shared helpers, re-exported)
from spgemm_ref import csr, pick, to_scipy, with_values  # noqa: F401

LANE_LEN = 64            # source rows of at most this many entries are ranked by one lane, longer ones by one wave
MAX_BLOCKS = 256         # MGS_BMAT_MAX_BLOCKS
TOO_MANY = 2 ** 31 - 1   # a result of this many entries (rows, columns) or more is refused


# ------------------------------------------------------------------ permute
def check_perm(perm, n, name):
    """None for a bijection of [0, n), else what the device names: (name, lowest offending position, its value, "range" | "repeat").
    A position offends when its value lies outside [0, n) or repeats the value of an earlier position; entries are taken as 64-bit
    values, so 2³² + 3 is out of range whatever it would narrow to."""
    first = {}
    for k, v in enumerate(np.asarray(perm, dtype=np.int64).tolist()):
        if v < 0 or v >= n:
            return name, k, v, "range"
        if v in first:
            return name, k, v, "repeat"
        first[v] = k
    return None


def refusal(A, rperm=None, cperm=None):
    """None, or the refusal of mgs_csr_permute: a violation of the row list before any of the column list"""
    for name, perm, n in (("row", rperm, A[0]), ("column", cperm, A[1])):
        if perm is not None:
            bad = check_perm(perm, n, name)
            if bad is not None:
                return bad
    return None


def permute_ref(A, rperm=None, cperm=None):
    """the restatement → (rows, cols, rowptr, col, val, src)"""
    m, n, rp, ci, v = A
    assert refusal(A, rperm, cperm) is None
    rperm = np.arange(m, dtype=np.int64) if rperm is None else np.asarray(rperm, dtype=np.int64)
    cinv = np.arange(n, dtype=np.int64)
    if cperm is not None:
        cinv = np.empty(n, dtype=np.int64)
        cinv[np.asarray(cperm, dtype=np.int64)] = np.arange(n)
    crp, ccol, src = [0], [], []
    for r in rperm:
        seg = np.arange(int(rp[r]), int(rp[r + 1]), dtype=np.int64)
        q = cinv[ci[seg]]
        order = np.argsort(q, kind="stable")
        ccol.append(q[order]); src.append(seg[order])
        crp.append(crp[-1] + len(seg))
    ccol = np.concatenate(ccol + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    src = np.concatenate(src + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    return m, n, np.asarray(crp, dtype=np.int32), ccol, np.asarray(v, dtype=np.float64)[src], src


def matrix(C):
    """the (rows, cols, rowptr, col, val) part of a restatement's result"""
    return C[:5]


def permute_info(A, rperm=None, cperm=None, keep_map=False):
    """what mgs_csr_permute_info reports"""
    lens = np.diff(A[2])
    ranked = cperm is not None
    return {"lane_rows": int((lens <= LANE_LEN).sum()) if ranked else 0, "wave_rows": int((lens > LANE_LEN).sum()) if ranked else 0,
            "max_row_len": int(lens.max()) if len(lens) else 0, "map_bytes": 4 * len(A[3]) if keep_map else 0}


def inverse(perm):
    out = np.empty(len(perm), dtype=np.int64)
    out[np.asarray(perm, dtype=np.int64)] = np.arange(len(perm))
    return out


# ------------------------------------------------------------------ bmat
def bmat_refusal(grid, row_sizes=None, col_sizes=None):
    """None, or the refusal of mgs_csr_bmat that the shapes alone decide, in the order the library checks: ("grid", br·bc),
    ("rows", (I, J)) / ("cols", (I, J)) for a block that disagrees with its block row / column, ("no row size", I),
    ("no col size", J), ("entries", total) — the total taken in Python's integers"""
    br, bc = len(grid), len(grid[0])
    if br * bc > MAX_BLOCKS:
        return "grid", br * bc
    rs = [-1] * br if row_sizes is None else [int(s) for s in row_sizes]
    cs = [-1] * bc if col_sizes is None else [int(s) for s in col_sizes]
    for I in range(br):
        for J in range(bc):
            B = grid[I][J]
            if B is None:
                continue
            if rs[I] < 0:
                rs[I] = B[0]
            if rs[I] != B[0]:
                return "rows", (I, J)
            if cs[J] < 0:
                cs[J] = B[1]
            if cs[J] != B[1]:
                return "cols", (I, J)
    for I in range(br):
        if rs[I] < 0:
            return "no row size", I
    for J in range(bc):
        if cs[J] < 0:
            return "no col size", J
    total = sum(int(B[2][-1]) for row in grid for B in row if B is not None)
    if sum(rs) >= TOO_MANY or sum(cs) >= TOO_MANY or total >= TOO_MANY:
        return "entries", total
    return None


def bmat_ref(grid, row_sizes=None, col_sizes=None):
    """the restatement → (rows, cols, rowptr, col, val)"""
    assert bmat_refusal(grid, row_sizes, col_sizes) is None
    br, bc = len(grid), len(grid[0])
    rs = [next((B[0] for B in grid[I] if B is not None), None if row_sizes is None else row_sizes[I]) for I in range(br)]
    cs = [next((grid[I][J][1] for I in range(br) if grid[I][J] is not None), None if col_sizes is None else col_sizes[J]) for J in range(bc)]
    coff = np.r_[0, np.cumsum(cs)].astype(np.int64)
    rp, ci, v = [0], [], []
    count = 0
    for I in range(br):
        for i in range(rs[I]):
            for J in range(bc):
                B = grid[I][J]
                if B is None:
                    continue
                seg = slice(int(B[2][i]), int(B[2][i + 1]))
                ci.append(B[3][seg].astype(np.int64) + coff[J]); v.append(np.asarray(B[4], dtype=np.float64)[seg])
                count += seg.stop - seg.start
            rp.append(count)
    ci = np.concatenate(ci + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    v = np.concatenate(v + [np.zeros(0)])
    return int(sum(rs)), int(sum(cs)), np.asarray(rp, dtype=np.int32), ci, v


def bmat_info(grid, row_sizes=None, col_sizes=None):
    """what mgs_csr_bmat_info reports"""
    lens = np.diff(bmat_ref(grid, row_sizes, col_sizes)[2])
    return {"blocks": sum(B is not None for row in grid for B in row), "block_rows": len(grid), "block_cols": len(grid[0]),
            "max_row_len": int(lens.max()) if len(lens) else 0}


# ------------------------------------------------------------------ fixtures
def salted(A, seed):
    """A with random normal values among which sit a −0.0, a NaN with a payload and two stored zeros"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(len(A[3]))
    at = rng.choice(len(v), size=4, replace=False)
    v[at[0]] = -0.0; v[at[1]] = nan_with_payload(); v[at[2]] = 0.0; v[at[3]] = 0.0
    return with_values(A, v)


def small_ints(A, seed):
    """A with small non-zero integer values: every product and sum of an SpMV with a small-integer vector is exact"""
    rng = np.random.default_rng(seed)
    return with_values(A, rng.integers(1, 8, len(A[3])).astype(np.float64) * rng.choice([-1.0, 1.0], len(A[3])))


def fx_poisson5():
    """Poisson on 5³: 125 rows of 4 to 7 entries (every row on the lane arm), salted values"""
    return salted(poisson3d(5), 2005)


CRAFTED_LENS = (0, 1, 63, 64, 65, 128, 129, 300)


def fx_crafted():
    """40 × 330: rows 0..7 hold 0, 1, 63, 64, 65, 128, 129 and 300 entries — an empty row, the lane | wave boundary (64 | 65), one
    and two full chunks of 64 and one entry more than those, and a row of four chunks and 44; the other 32 rows hold 0 to 12"""
    rng = np.random.default_rng(40330)
    n = 330
    rows = [pick(rng, 0, n, k) for k in CRAFTED_LENS] + [pick(rng, 0, n, int(rng.integers(0, 13))) for _ in range(32)]
    rp = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    return salted((len(rows), n, rp, ci, np.zeros(len(ci))), 40331)


MATRICES = {"poisson5": fx_poisson5, "crafted": fx_crafted}


def lists(m, n):
    """name → (rperm, cperm) for an m × n matrix: a random list (fixed seed), the reversal and the identity, each on the rows only, on
    the columns only and on both sides"""
    rng = np.random.default_rng(1000 * m + n)
    kinds = {"random": lambda k: rng.permutation(k), "reversal": lambda k: np.arange(k)[::-1].copy(), "identity": lambda k: np.arange(k)}
    out = {}
    for kind, make in kinds.items():
        out[kind + "_rows"] = (make(m), None)
        out[kind + "_cols"] = (None, make(n))
        out[kind + "_both"] = (make(m), make(n))
    return out


def rand_csr(seed, m, n, maxlen, empty=()):
    rng = np.random.default_rng(seed)
    rows = [pick(rng, 0, n, int(rng.integers(1, maxlen + 1))) if i not in empty else np.zeros(0, dtype=np.int64) for i in range(m)]
    rp = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    return salted((m, n, rp, ci, np.zeros(len(ci))), seed + 1)


def diagonal(n, seed):
    rng = np.random.default_rng(seed)
    return n, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), rng.standard_normal(n)


def bmat_fixtures():
    """name → (mats, grid, row_sizes, col_sizes): mats maps a name to a matrix, grid is a list of lists of names or None — the same name
    in two places is the same handle on the device"""
    L = salted(poisson3d(4), 404)                                   # 64 × 64
    R = rand_csr(3753, 37, 53, 9, empty=(3, 20, 36))                # rectangular, empty rows
    S = rand_csr(3729, 37, 29, 6, empty=(0, 20))
    T = rand_csr(1053, 10, 53, 12)
    B = rand_csr(5329, 53, 29, 5, empty=(52,))
    mats = {"L": L, "D1": diagonal(64, 1), "D2": diagonal(64, 2), "R": R, "S": S, "T": T, "B": B}
    return {
        "two_by_two_one_null": (mats, [["L", "D1"], ["D2", None]], None, None),
        "null_block_row": (mats, [["R", "S"], [None, None], ["T", None]], [37, 5, 10], None),
        "null_block_column": (mats, [["R", None, "S"]], None, [53, 7, 29]),
        "empty_rows": (mats, [["S", "R"], ["S", "R"]], None, None),
        "same_handle_twice": (mats, [["L", "D1"], ["D1", "L"]], None, None),
        "hstack": (mats, [["R", "S"]], None, None),
        "vstack": (mats, [["R"], ["T"]], None, None),
        "block_diag": (mats, [["R", None, None], [None, "B", None], [None, None, "T"]], None, None),
    }


def resolve(mats, grid):
    return [[mats[b] if b is not None else None for b in row] for row in grid]


COUPLING = 0.25


def fx_two_field():
    """(L, c, K, p): L Poisson on 6³, K = [[L, c·I], [c·I, L]] with c = 0.25 < λ_min(L) = 6 − 6·cos(π/7) ≈ 0.594, so K is SPD;
    p the list that turns the field-major numbering (u₀ u₁ … v₀ v₁ …) into the interleaved one (u₀ v₀ u₁ v₁ …): p[2k] = k, p[2k+1] = n + k"""
    L = poisson3d(6)
    n = L[0]
    cI = (n, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.full(n, COUPLING))
    K = bmat_ref([[L, cI], [cI, L]])
    p = np.empty(2 * n, dtype=np.int64)
    p[0::2] = np.arange(n); p[1::2] = n + np.arange(n)
    return L, cI, K, p
