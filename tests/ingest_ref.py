"""Plain numpy / Python restatement of mgs_csr_from_coo_device (include/mgs.h): triples in any order to CSR, columns ascending inside a
row, entries with equal (row, col) summed in input order — left to right, starting from the first value itself (not from 0.0 + v).
Checker only; the sums run in a Python loop so that no library decides their order."""
import numpy as np


def coo_to_csr_ref(rows, row, col, val):
    """→ (rowptr int32, col int32, val float64, order): `order` = the triples' input positions sorted by (row, col, position)"""
    row = np.asarray(row, dtype=np.int64); col = np.asarray(col, dtype=np.int64); val = np.asarray(val, dtype=np.float64)
    n = len(row)
    order = np.lexsort((np.arange(n), col, row))          # last key is the primary one: row, then col, then input position
    r, c = row[order], col[order]
    head = np.ones(n, dtype=bool)
    if n:
        head[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], n)
    out = np.empty(len(starts), dtype=np.float64)
    v = val[order]
    for e, (lo, hi) in enumerate(zip(starts, ends)):
        s = v[lo]
        for q in range(lo + 1, hi):
            s = s + v[q]
        out[e] = s
    rowptr = np.zeros(rows + 1, dtype=np.int64)
    np.add.at(rowptr, r[starts] + 1, 1)
    return np.cumsum(rowptr).astype(np.int32), c[starts].astype(np.int32), out, order


def csr_triples(rowptr, col, val):
    """(row, col, val) of a CSR matrix, in storage order"""
    rowptr = np.asarray(rowptr)
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr)), np.asarray(col, dtype=np.int64), np.asarray(val, dtype=np.float64)


def dyadic_split(row, col, val):
    """every triple as v/2, v/4, v/4 (exact in binary floating point away from the subnormals): the three sum back to v bit for bit
    in that order"""
    return np.repeat(row, 3), np.repeat(col, 3), (np.repeat(val, 3).reshape(-1, 3) * np.array([0.5, 0.25, 0.25])).reshape(-1)


def permuted(seed, *arrays):
    p = np.random.default_rng(seed).permutation(len(arrays[0]))
    return tuple(a[p] for a in arrays)
