"""Numpy restatement of option pack7: the packed copy of an FP64 operand's values, 7 bytes per entry, the same bits.

Sixteen consecutive entries k = 16·R … 16·R + 15 of the source array make one 112-byte record at byte offset 112·R: sixteen low dwords
(mantissa bits 0–31), sixteen 16-bit words (mantissa bits 32–47), sixteen bytes sign << 7 | d << 4 | mantissa bits 48–51 with d = biased
exponent − E0 of the row block that owns the entry.  A row block owns the entries [bounds[q], bounds[q + 1]) of the array and is eligible if every
one of them is a normal number whose biased exponent lies in [E0, E0 + 7], E0 the smallest of the slice; e0[q] = E0, or −1 for a block that is
not packed (a zero, a denormal, an Inf, a NaN, 8 binades or more, or no entry).  The array's end is padded to a whole record."""
import numpy as np

RECORD = 112


def exponents(v):
    return ((np.asarray(v, dtype=np.float64).view(np.uint64) >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)


def eligibility(v, bounds):
    """e0 per block"""
    ex = exponents(v)
    e0 = np.full(len(bounds) - 1, -1, dtype=np.int32)
    for q in range(len(bounds) - 1):
        s = ex[bounds[q]:bounds[q + 1]]
        if s.size and s.min() >= 1 and s.max() <= 2046 and s.max() - s.min() <= 7:
            e0[q] = s.min()
    return e0


def pack(v, bounds):
    """(bytes of the packed array, e0 per block); entries of a block that is not packed are written with d = 0 and are never decoded"""
    v = np.asarray(v, dtype=np.float64)
    bits = v.view(np.uint64)
    e0 = eligibility(v, bounds)
    nrec = (len(v) + 15) // 16
    out = np.zeros(nrec * RECORD, dtype=np.uint8)
    lo = out.reshape(nrec, RECORD)[:, :64].view(np.uint32)          # [nrec, 16] views into out
    mid = out.reshape(nrec, RECORD)[:, 64:96].view(np.uint16)
    top = out.reshape(nrec, RECORD)[:, 96:112]
    k = np.arange(len(v))
    owner = np.searchsorted(np.asarray(bounds), k, side="right") - 1
    base = e0[np.clip(owner, 0, len(e0) - 1)].astype(np.int64)
    hi = (bits >> np.uint64(32)).astype(np.int64)
    d = np.where(base >= 0, ((hi >> 20) & 0x7FF) - base, 0)
    lo[k >> 4, k & 15] = (bits & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    mid[k >> 4, k & 15] = (hi & 0xFFFF).astype(np.uint16)
    top[k >> 4, k & 15] = (((hi >> 31) & 1) << 7 | (d & 7) << 4 | (hi >> 16) & 15).astype(np.uint8)
    return out, e0


def fetch(packed, e, E0):
    """entries e (indices into the source array) decoded against the base exponent E0: the kernels' fetch — a dword, a 16-bit word and a byte"""
    e = np.asarray(e, dtype=np.int64)
    rec = packed.reshape(-1, RECORD)
    lo = rec[:, :64].view(np.uint32)[e >> 4, e & 15].astype(np.uint64)
    mid = rec[:, 64:96].view(np.uint16)[e >> 4, e & 15].astype(np.uint64)
    b = rec[:, 96:112][e >> 4, e & 15].astype(np.uint64)
    hi = ((b & np.uint64(0x80)) << np.uint64(24)) + ((b & np.uint64(0x7F)) << np.uint64(16)) + (np.uint64(E0) << np.uint64(20)) + mid
    return ((hi << np.uint64(32)) | lo).view(np.float64)


def unpack(packed, e0, bounds, source):
    """the array as the kernels see it: a packed block's entries decoded from its records, any other block's read from the FP64 array"""
    out = np.array(source, dtype=np.float64, copy=True)
    for q in range(len(bounds) - 1):
        if e0[q] >= 0:
            out[bounds[q]:bounds[q + 1]] = fetch(packed, np.arange(bounds[q], bounds[q + 1]), int(e0[q]))
    return out


def block_bounds(rowptr, nd=False, rb=256):
    """entry bounds of the 256-row blocks of a CSR operand; nd: of the operand without its diagonal entries (row i starts at rowptr[i] − i)"""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = len(rowptr) - 1
    rows = np.minimum(np.arange(0, n + rb, rb), n)
    if rows[-1] != n or len(rows) < 2:
        rows = np.r_[rows, n]
    rows = np.unique(rows)
    return rowptr[rows] - (rows if nd else 0)
