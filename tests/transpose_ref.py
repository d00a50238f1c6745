"""numpy restatement of mgs_csr_transpose_numeric (include/mgs.h; multigridsolver_amd/csrc/reorder.hip: transpose_numeric_kernel), entry by
entry: entry k of A finds its row i by bisection in A's rowptr (the last i with rowptr[i] <= k), has column j, and finds its place by
bisection of i in At's columns of row j; the value moves as a 64-bit word; an entry whose place does not exist is counted and never
written.  tests/test_gpu_transpose_numeric.py holds it to scipy's A.T.tocsr() on the CPU and the device to it."""
import numpy as np


def row_of_entry(rowptr, rows, k):
    lo, hi = 0, rows
    while hi - lo > 1:
        mid = lo + ((hi - lo) >> 1)
        if rowptr[mid] <= k:
            lo = mid
        else:
            hi = mid
    return lo


def transpose_numeric_ref(a_shape, a_rp, a_ci, a_val, t_rp, t_ci, t_val):
    """→ (the values of At after the call, as a new float64 array with t_val's bits where nothing was written; misses)"""
    rows, cols = a_shape
    nnz = int(a_rp[rows]) if rows else 0
    out = np.array(t_val, dtype=np.float64, copy=True).view(np.uint64)
    src = np.ascontiguousarray(a_val, dtype=np.float64).view(np.uint64)
    misses = 0
    for k in range(nnz):
        i = row_of_entry(a_rp, rows, k)
        j = int(a_ci[k])
        placed = False
        if 0 <= j < cols:
            b, e = int(t_rp[j]), int(t_rp[j + 1])
            if 0 <= b <= e <= nnz:
                p, q = b, e
                while p < q:
                    mid = p + ((q - p) >> 1)
                    if t_ci[mid] < i:
                        p = mid + 1
                    else:
                        q = mid
                if p < e and t_ci[p] == i:
                    out[p] = src[k]
                    placed = True
        if not placed:
            misses += 1
    return out.view(np.float64), misses
