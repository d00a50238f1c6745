"""Matrices that enter the library from device memory (include/mgs.h: mgs_csr_from_device, mgs_csr_from_coo_device,
mgs_csr_update_values_coo_dev).  The checked CSR copy is held bit for bit to mgs_csr_upload of the same host arrays — accepted
matrices, and for refused ones the error message; the COO assembly bit for bit to the sequential restatement tests/ingest_ref.py
(duplicates summed in input order).  Inputs are placed with torch and made visible with torch.cuda.synchronize().  Shapes are the
smallest at which each kernel path can go wrong: 600 rows put rows 3 and 300 into different workgroups of the column pass (256 rows
each); row lengths sit on both sides of every boundary of the bucket sort (one lane up to 32 triples, one workgroup in LDS padded to
64, 128, ... 8192 keys above)."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sps
import torch

from conftest import INP
from ingest_ref import coo_to_csr_ref, csr_triples, dyadic_split, permuted

pytestmark = pytest.mark.gpu

OK, INVALID, STATE = 0, -1, -6
UNTOUCHED = 0x1234
MAX_ROW = 8192


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).to("cuda:0")
    torch.cuda.synchronize()
    return t


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_csr_equal(M, rp, ci, v, what=""):
    rp2, ci2, v2 = M.download()
    assert rp2.dtype == np.int32 and ci2.dtype == np.int32
    assert np.array_equal(rp2, rp), what
    assert np.array_equal(ci2, ci), what
    assert bits_equal(v2, v), what


def raw_csr(mg, ctx, rows, cols, rp, ci, v, bits, nnz=None):
    """mgs_csr_from_device through ctypes: (return code, message, what `out` holds afterwards)"""
    out = C.c_void_p(UNTOUCHED)
    rc = mg.lib().mgs_csr_from_device(ctx.h, rows, cols, len(ci) if nnz is None else nnz, C.c_void_p(rp.data_ptr()), C.c_void_p(ci.data_ptr()), bits,
                                      C.c_void_p(v.data_ptr()), C.byref(out))
    msg = mg.lib().mgs_last_error(ctx.h).decode()
    if rc == OK:
        mg.lib().mgs_csr_destroy(out)
    return rc, msg, out.value


def raw_coo(mg, ctx, rows, cols, r, c, v, bits, keep=0):
    out = C.c_void_p(UNTOUCHED)
    rc = mg.lib().mgs_csr_from_coo_device(ctx.h, rows, cols, len(r), C.c_void_p(r.data_ptr()), C.c_void_p(c.data_ptr()), bits, C.c_void_p(v.data_ptr()), keep,
                                          C.byref(out))
    msg = mg.lib().mgs_last_error(ctx.h).decode()
    if rc == OK:
        mg.lib().mgs_csr_destroy(out)
    return rc, msg, out.value


def host_upload_message(mg, ctx, rows, cols, rp, ci, v):
    """what mgs_csr_upload says about the same arrays, with the device constructor's name"""
    with pytest.raises(mg.MgsError) as e:
        mg.Csr.upload(ctx, rows, cols, rp, ci, v)
    assert e.value.code == INVALID
    return str(e.value).split(": ", 1)[1].replace("mgs_csr_upload", "mgs_csr_from_device")


# ------------------------------------------------------------------ 1. CSR parity
@pytest.fixture(scope="module")
def csky10(mg):
    return mg.read_mtx(os.path.join(INP, "CSky3d10.mtx"))


@pytest.mark.parametrize("name", ["SmallTestMatrix", "CSky3d10"])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_csr_parity_with_upload(mg, ctx, name, dtype):
    n, m, rp, ci, v = mg.read_mtx(os.path.join(INP, name + ".mtx"))
    A = mg.Csr.upload(ctx, n, m, rp, ci, v)
    B = mg.Csr.from_device(ctx, n, m, dev(rp, dtype), dev(ci, dtype), dev(v))
    assert B.shape == (n, m) and B.nnz == len(ci)
    assert_csr_equal(B, rp, ci, v)
    assert B.plan_info() == A.plan_info()
    assert B.coo_info() == {"triples": 0, "entries": len(ci), "max_row_triples": 0, "map_bytes": 0}
    x = ctx.vec(np.random.default_rng(1).standard_normal(m))
    ya, yb = A.spmv(x).numpy(), B.spmv(x).numpy()
    assert np.linalg.norm(ya) > 0 and bits_equal(ya, yb)
    A.optimize(); B.optimize()
    assert B.rowcode_info() == A.rowcode_info()
    assert bits_equal(A.spmv(x).numpy(), B.spmv(x).numpy())
    if name == "CSky3d10":
        ha = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 100, 32).finalize()
        hb = mg.Hierarchy(B, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 100, 32).finalize()
        assert ha.nlev == hb.nlev and ha.nlev >= 2
        b = ctx.vec(np.random.default_rng(2).standard_normal(n))
        xa, xb = ha.vcycle(b).numpy(), hb.vcycle(b).numpy()
        assert np.isfinite(xa).all() and np.linalg.norm(xa) > 0 and bits_equal(xa, xb)


# ------------------------------------------------------------------ 2. CSR acceptance edges
def random_csr(seed, rows, cols, lo_len, hi_len, col_lo=0):
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo_len, hi_len + 1, size=rows)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate([np.sort(rng.choice(np.arange(col_lo, cols), size=k, replace=False)) for k in lens] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    return rp, ci, rng.standard_normal(len(ci))


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_csr_accepts_the_edges(mg, ctx, dtype):
    rows, cols = 600, 650                                     # cols != rows
    rng = np.random.default_rng(3)
    row_cols = [np.sort(rng.choice(cols, size=rng.integers(1, 9), replace=False)) for _ in range(rows)]
    for empty in (0, 255, 256, 299, 300, 599):                # empty first, middle (also on both sides of a workgroup's edge) and last row
        row_cols[empty] = np.zeros(0, dtype=np.int64)
    row_cols[2] = np.array([10, 400]); row_cols[3] = np.array([5, 400])        # row 3 starts below row 2's last column ...
    row_cols[4] = np.array([400, 649])                                          # ... and row 4 starts exactly on row 3's last column
    row_cols[301] = np.array([7, 8, 9]); row_cols[302] = np.array([9])          # the same in the second workgroup
    rp = np.concatenate([[0], np.cumsum([len(c) for c in row_cols])]).astype(np.int32)
    ci = np.concatenate(row_cols).astype(np.int32)
    v = rng.standard_normal(len(ci))
    A = mg.Csr.upload(ctx, rows, cols, rp, ci, v)
    B = mg.Csr.from_device(ctx, rows, cols, dev(rp, dtype), dev(ci, dtype), dev(v))
    assert_csr_equal(B, rp, ci, v)
    assert B.plan_info() == A.plan_info()
    x = ctx.vec(rng.standard_normal(cols))
    assert bits_equal(A.spmv(x).numpy(), B.spmv(x).numpy())
    # rows = 1
    B = mg.Csr.from_device(ctx, 1, 9, dev([0, 3], dtype), dev([0, 4, 8], dtype), dev(np.array([1.0, -2.0, 3.0])))
    assert_csr_equal(B, [0, 3], [0, 4, 8], [1.0, -2.0, 3.0])
    # nnz = 0: no column or value array at all
    B = mg.Csr.from_device(ctx, 5, 5, dev(np.zeros(6), dtype), dev(np.zeros(0), dtype), dev(np.zeros(0)))
    assert B.nnz == 0 and np.array_equal(B.download()[0], np.zeros(6, dtype=np.int32))


# ------------------------------------------------------------------ 3. CSR refusals
@pytest.fixture(scope="module")
def base600():
    """600 x 650, every row 2..8 entries, columns from 5 upwards (so that a first column of 2**32 + 1 would pass once narrowed to 1)"""
    return (600, 650) + random_csr(4, 600, 650, 2, 8, col_lo=5)


CSR_BAD = {
    "rowptr[0] = 1": lambda rp, ci: rp.__setitem__(0, 1),
    "decreasing rowptr": lambda rp, ci: rp.__setitem__(10, rp[11] + 1),
    "column == cols": lambda rp, ci: ci.__setitem__(int(rp[301]) - 1, 650),
    "column -1": lambda rp, ci: ci.__setitem__(int(rp[7]), -1),
    "equal adjacent columns": lambda rp, ci: ci.__setitem__(int(rp[20]) + 1, ci[int(rp[20])]),
    "descending pair": lambda rp, ci: ci.__setitem__(int(rp[599]), 649),
    "rows 3 and 300 bad": lambda rp, ci: (ci.__setitem__(int(rp[300]), 649), ci.__setitem__(int(rp[3]) + 1, ci[int(rp[3])])),
    "row 300 bad, then row 3 out of range": lambda rp, ci: (ci.__setitem__(int(rp[300]), -7), ci.__setitem__(int(rp[4]) - 1, 651)),
}


@pytest.mark.parametrize("case", list(CSR_BAD))
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_csr_refusals_say_what_upload_says(mg, ctx, base600, case, dtype):
    rows, cols, rp, ci, v = base600
    rp, ci = rp.copy(), ci.copy()
    CSR_BAD[case](rp, ci)
    want = host_upload_message(mg, ctx, rows, cols, rp, ci, v)
    rc, msg, out = raw_csr(mg, ctx, rows, cols, dev(rp, dtype), dev(ci, dtype), dev(v), 32 if dtype is np.int32 else 64)
    assert rc == INVALID and out == UNTOUCHED, (rc, msg)
    assert msg == want, (msg, want)
    if "300" in case:                                         # rows 3 and 300 both bad: the lowest row is the one named
        assert ("row 3 " in msg or msg.endswith("row 3")) and "row 300" not in msg, msg
    with pytest.raises(mg.MgsError):
        mg.Csr.from_device(ctx, rows, cols, dev(rp, dtype), dev(ci, dtype), dev(v))


def test_csr_refusals_of_the_call_itself(mg, ctx, base600):
    rows, cols, rp, ci, v = base600
    d_rp, d_ci, d_v = dev(rp), dev(ci), dev(v)
    # rowptr[rows] != nnz: one entry fewer announced than rowptr ends on
    rc, msg, out = raw_csr(mg, ctx, rows, cols, d_rp, d_ci, d_v, 32, nnz=len(ci) - 1)
    assert rc == INVALID and out == UNTOUCHED and "inconsistent" in msg and f"rowptr[rows]={len(ci)} nnz={len(ci) - 1}" in msg, msg
    rp2 = rp.copy(); rp2[-1] -= 1
    rc, msg, out = raw_csr(mg, ctx, rows, cols, dev(rp2), d_ci, d_v, 32)
    assert rc == INVALID and out == UNTOUCHED and msg == host_upload_message(mg, ctx, rows, cols, rp2, ci, v), msg
    # index_bits = 16
    rc, msg, out = raw_csr(mg, ctx, rows, cols, d_rp, d_ci, d_v, 16)
    assert rc == INVALID and out == UNTOUCHED and "index_bits" in msg, msg
    # the valid arrays are accepted through the same raw path (the refusals above are not the helper's doing)
    assert raw_csr(mg, ctx, rows, cols, d_rp, d_ci, d_v, 32)[0] == OK
    assert raw_csr(mg, ctx, rows, cols, dev(rp, np.int64), dev(ci, np.int64), d_v, 64)[0] == OK


def test_csr_64_bit_indices_are_checked_before_they_are_narrowed(mg, ctx, base600):
    rows, cols, rp, ci, v = base600
    rp64, ci64 = rp.astype(np.int64), ci.astype(np.int64)
    k = int(rp[300])
    assert ci[k] >= 5 and ci[k + 1] > 1                       # narrowed to 32 bits the bad column would read 1: in range and ascending
    bad = ci64.copy(); bad[k] = 2 ** 32 + 1
    rc, msg, out = raw_csr(mg, ctx, rows, cols, dev(rp64), dev(bad), dev(v), 64)
    assert rc == INVALID and out == UNTOUCHED, msg
    assert msg == f"mgs_csr_from_device: column {2 ** 32 + 1} out of range in row 300", msg
    bad = rp64.copy(); bad[0] = 2 ** 32                       # narrowed it would read 0
    rc, msg, out = raw_csr(mg, ctx, rows, cols, dev(bad), dev(ci64), dev(v), 64)
    assert rc == INVALID and out == UNTOUCHED and f"rowptr[0]={2 ** 32}" in msg, msg
    bad = rp64.copy(); bad[200] += 2 ** 32                    # narrowed it would be unchanged
    rc, msg, out = raw_csr(mg, ctx, rows, cols, dev(bad), dev(ci64), dev(v), 64)
    assert rc == INVALID and out == UNTOUCHED and ("row 199" in msg or "row 200" in msg), msg


# ------------------------------------------------------------------ 4. COO against the restatement, bit for bit
def coo(mg, ctx, rows, cols, r, c, v, dtype=np.int64, keep_map=False):
    return mg.Csr.from_coo_device(ctx, rows, cols, dev(r, dtype), dev(c, dtype), dev(v), keep_map=keep_map)


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_coo_csky3d10_permuted_and_split(mg, ctx, csky10, dtype):
    n, m, rp, ci, v = csky10
    r, c, val = permuted(11, *csr_triples(rp, ci, v))
    A = coo(mg, ctx, n, m, r, c, val, dtype)
    assert_csr_equal(A, rp, ci, v, "(a)")
    assert A.plan_info() == mg.Csr.upload(ctx, n, m, rp, ci, v).plan_info()
    r3, c3, v3 = permuted(12, *dyadic_split(*csr_triples(rp, ci, v)))
    B = coo(mg, ctx, n, m, r3, c3, v3, dtype)
    assert_csr_equal(B, rp, ci, v, "(b)")
    assert B.coo_info()["max_row_triples"] == 3 * int(np.diff(rp).max())


@pytest.fixture(scope="module")
def case4c():
    """300 x 300, 5000 triples on 2000 distinct positions, values over sixteen decades; new values for the re-assembly; both restatements"""
    rng = np.random.default_rng(13)
    pos = rng.choice(300 * 300, size=2000, replace=False)
    pick = np.concatenate([np.arange(2000), rng.integers(0, 2000, size=3000)])
    rng.shuffle(pick)
    r, c = pos[pick] // 300, pos[pick] % 300
    v1 = rng.standard_normal(5000) * 10.0 ** rng.uniform(-8, 8, size=5000)
    v2 = rng.standard_normal(5000) * 10.0 ** rng.uniform(-8, 8, size=5000)
    ref1, ref2 = coo_to_csr_ref(300, r, c, v1), coo_to_csr_ref(300, r, c, v2)
    assert len(ref1[1]) == 2000
    return r, c, v1, v2, ref1, ref2


def test_coo_random_duplicates_equal_the_sequential_sums(mg, ctx, case4c):
    r, c, v1, _, (rp, ci, v, _), _ = case4c
    A = coo(mg, ctx, 300, 300, r, c, v1)
    assert_csr_equal(A, rp, ci, v)
    first_bits = A.download()[2].copy()
    for _ in range(2):                                       # the scatter's atomics are scheduled anew: the bits must not move
        assert bits_equal(coo(mg, ctx, 300, 300, r, c, v1, np.int32).download()[2], first_bits)


def test_coo_zeros_and_signs(mg, ctx):
    r = np.array([0, 1, 2, 2, 3]); c = np.array([1, 1, 0, 0, 2]); v = np.array([-0.0, 0.0, 2.5, -2.5, 7.0])
    rp, ci, val = coo(mg, ctx, 4, 3, r, c, v).download()
    assert rp.tolist() == [0, 1, 2, 3, 4] and ci.tolist() == [1, 1, 0, 2]           # the explicit zero and the cancelled pair stay entries
    assert val.tolist() == [0.0, 0.0, 0.0, 7.0]
    assert np.signbit(val).tolist() == [True, False, False, False]                  # a lone -0.0 keeps its sign: the sum starts from the value itself


def test_coo_empty_rows_no_triples_and_one_row(mg, ctx):
    r = np.array([5, 2, 5, 2]); c = np.array([0, 6, 0, 1]); v = np.array([1.0, 2.0, 3.0, 4.0])
    A = coo(mg, ctx, 9, 7, r, c, v)                           # rows 0, 1, 3, 4, 6, 7, 8 empty: both ends and the middle
    assert_csr_equal(A, *coo_to_csr_ref(9, r, c, v)[:3])
    assert A.download()[0].tolist() == [0, 0, 0, 2, 2, 2, 3, 3, 3, 3]
    assert A.spmv(ctx.vec(np.ones(7))).numpy().tolist() == [0, 0, 6.0, 0, 0, 4.0, 0, 0, 0]
    e = np.zeros(0)
    A = coo(mg, ctx, 4, 4, e, e, e, keep_map=True)            # ntrip = 0
    assert A.nnz == 0 and A.download()[0].tolist() == [0, 0, 0, 0, 0]
    A.update_values_coo(dev(e))
    assert A.coo_info()["entries"] == 0
    r = np.zeros(5, dtype=np.int64); c = np.array([6, 0, 3, 6, 0]); v = np.array([1.0, 1e-30, 3.0, 1e30, -1.0])
    A = coo(mg, ctx, 1, 7, r, c, v, np.int32)                 # 1 x 7
    assert_csr_equal(A, [0, 3], [0, 3, 6], [1e-30 + -1.0, 3.0, 1.0 + 1e30])


# ------------------------------------------------------------------ 5. COO row-length classes
LONG_ROWS = {2: 1, 4: 31, 5: 32, 7: 33, 9: 64, 10: 65, 12: 1000, 14: 4096, 15: 4097, 17: 8191, 19: MAX_ROW}


def rows_of_lengths(lengths, rows, cols, seed):
    rng = np.random.default_rng(seed)
    r, c = [], []
    for i in range(rows):
        n = lengths.get(i, int(rng.integers(0, 6)))
        r.append(np.full(n, i))
        c.append(rng.integers(0, max(1, min(cols, (n * 2) // 3 + 1)), size=n))          # fewer columns than triples: duplicates in every long row
    r, c = np.concatenate(r), np.concatenate(c)
    v = rng.standard_normal(len(r)) * 10.0 ** rng.uniform(-3, 3, size=len(r))
    return permuted(seed + 1, r, c, v)


def test_coo_every_row_length_class(mg, ctx):
    rows, cols = 24, 3000
    r, c, v = rows_of_lengths(LONG_ROWS, rows, cols, 21)
    rp, ci, val, _ = coo_to_csr_ref(rows, r, c, v)
    assert all(int(np.count_nonzero(r == i)) == n for i, n in LONG_ROWS.items())
    assert all(rp[i + 1] - rp[i] < n for i, n in LONG_ROWS.items() if n > 32)               # duplicates in each long row
    A = coo(mg, ctx, rows, cols, r, c, v, keep_map=True)
    assert_csr_equal(A, rp, ci, val)
    assert A.coo_info() == {"triples": len(r), "entries": len(ci), "max_row_triples": MAX_ROW, "map_bytes": 4 * (len(r) + len(ci) + 1)}
    assert_csr_equal(coo(mg, ctx, rows, cols, r, c, v, np.int32), rp, ci, val)


def test_coo_row_above_the_limit_is_refused_by_name(mg, ctx):
    lengths = {3: MAX_ROW, 17: MAX_ROW + 1, 21: MAX_ROW + 5}
    r, c, v = rows_of_lengths(lengths, 24, 3000, 23)
    rc, msg, out = raw_coo(mg, ctx, 24, 3000, dev(r), dev(c), dev(v), 64)
    assert rc == INVALID and out == UNTOUCHED, msg
    assert "row 17 " in msg and "MGS_COO_MAX_ROW" in msg, msg


# ------------------------------------------------------------------ 6. COO refusals
@pytest.mark.parametrize("what,k,field,value,dtype", [("row = rows", 70, "r", 300, np.int32), ("row = -1", 4999, "r", -1, np.int64), ("col = cols", 0, "c", 300, np.int32),
                                                       ("col = -1", 2500, "c", -1, np.int64), ("int64 row = 2**32 + 2", 256, "r", 2 ** 32 + 2, np.int64),
                                                       ("int64 col = 2**32", 257, "c", 2 ** 32, np.int64)])
def test_coo_refusals(mg, ctx, case4c, what, k, field, value, dtype):
    r, c, v1 = (a.copy() for a in case4c[:3])
    (r if field == "r" else c)[k] = value
    (r if field == "r" else c)[4000 if k < 4000 else 4999] = value                   # a second bad triple further on: the lowest one is named
    rc, msg, out = raw_coo(mg, ctx, 300, 300, dev(r, dtype), dev(c, dtype), dev(v1), 32 if dtype is np.int32 else 64)
    assert rc == INVALID and out == UNTOUCHED, (what, msg)
    assert f"{'row' if field == 'r' else 'column'} {value} of triple {k} " in msg, (what, msg)
    rc, msg, out = raw_coo(mg, ctx, 300, 300, dev(r, dtype), dev(c, dtype), dev(v1), 16)
    assert rc == INVALID and out == UNTOUCHED and "index_bits" in msg


# ------------------------------------------------------------------ 7. map and re-assembly
def test_coo_map_reassembles_bit_for_bit(mg, ctx, case4c):
    r, c, v1, v2, (rp, ci, val1, _), (_, _, val2, _) = case4c
    A = coo(mg, ctx, 300, 300, r, c, v1, keep_map=True)
    assert A.coo_info() == {"triples": 5000, "entries": 2000, "max_row_triples": int(np.bincount(r).max()), "map_bytes": 4 * (5000 + 2000 + 1)}
    assert_csr_equal(A, rp, ci, val1)
    ptrs = A.device_ptrs()
    assert A.update_values_coo(dev(v2)) is A
    assert_csr_equal(A, rp, ci, val2, "after the update: same pattern, the restatement's sums of the new values")
    assert A.device_ptrs() == ptrs and all(ptrs)
    assert_csr_equal(coo(mg, ctx, 300, 300, r, c, v2), rp, ci, val2, "a fresh assembly of the new values")
    A.update_values_coo(ctx.vec(v1))                          # a Vec as the source
    assert_csr_equal(A, rp, ci, val1)
    # refusals
    with pytest.raises(mg.MgsError) as e:
        A.update_values_coo(dev(v2[:-1]))
    assert e.value.code == INVALID
    with pytest.raises(mg.MgsError) as e:
        A.update_values_coo(dev(np.concatenate([v2, v2])))
    assert e.value.code == INVALID
    assert mg.lib().mgs_csr_update_values_coo_dev(A.h, None, 5000) == INVALID
    assert_csr_equal(A, rp, ci, val1, "a refused update changes nothing")
    B = coo(mg, ctx, 300, 300, r, c, v1)
    assert B.coo_info()["triples"] == 0 and B.coo_info()["map_bytes"] == 0
    with pytest.raises(mg.MgsError) as e:
        B.update_values_coo(dev(v2))
    assert e.value.code == STATE
    with pytest.raises(TypeError):
        A.update_values_coo(dev(v2, np.float32))
    with pytest.raises(TypeError):
        A.update_values_coo(v2)                               # a host array is not uploaded silently


# ------------------------------------------------------------------ 8. assemble, solve, re-assemble, refresh
def poisson_edges(N, coef):
    """7-point operator on the N^3 grid from per-edge contributions: for each node and each of its six directions the edge coefficient
    (coef at the edge's midpoint) goes to the diagonal, and its negative to the neighbour's column where the neighbour exists
    (Dirichlet boundary).  Every off-diagonal appears once, every diagonal as six summed contributions."""
    g = np.arange(N)
    I, J, K = (a.reshape(-1) for a in np.meshgrid(g, g, g, indexing="ij"))
    node = (I * N + J) * N + K
    r, c, v = [], [], []
    for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        k = coef((I + 0.5 * d[0] + 0.5) / N, (J + 0.5 * d[1] + 0.5) / N, (K + 0.5 * d[2] + 0.5) / N)
        r.append(node); c.append(node); v.append(k)
        I2, J2, K2 = I + d[0], J + d[1], K + d[2]
        ok = (I2 >= 0) & (I2 < N) & (J2 >= 0) & (J2 < N) & (K2 >= 0) & (K2 < N)
        r.append(node[ok]); c.append(((I2 * N + J2) * N + K2)[ok]); v.append(-k[ok])
    return np.concatenate(r), np.concatenate(c), np.concatenate(v)


def true_residual(ref, x, b):
    rp, ci, v, _ = ref
    A = sps.csr_matrix((v, ci, rp), shape=(len(rp) - 1, len(rp) - 1))
    return float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))


def test_assemble_solve_reassemble_refresh(mg, ctx):
    N = 16; n = N ** 3
    r, c, v1 = poisson_edges(N, lambda x, y, z: np.ones_like(x))
    r2, c2, v2 = poisson_edges(N, lambda x, y, z: 1.0 + 0.5 * np.sin(2.0 * x + 1.0) * np.cos(3.0 * y) + 0.25 * z)
    assert np.array_equal(r, r2) and np.array_equal(c, c2) and v2[v2 > 0].min() > 0.2
    p = np.random.default_rng(31).permutation(len(r))
    r, c, v1, v2 = r[p], c[p], v1[p], v2[p]
    ref1, ref2 = coo_to_csr_ref(n, r, c, v1), coo_to_csr_ref(n, r, c, v2)
    A = coo(mg, ctx, n, n, r, c, v1, keep_map=True)
    assert_csr_equal(A, *ref1[:3])
    P = ctx.poisson3d(N).download()                           # the unit coefficient gives the library's own 7-point operator
    assert np.array_equal(P[0], ref1[0]) and np.array_equal(P[1], ref1[1]) and bits_equal(P[2], ref1[2])
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 500, 32).finalize()
    assert h.nlev >= 2
    b_np = np.random.default_rng(32).standard_normal(n)
    b, x = ctx.vec(b_np), ctx.vec(n)
    st, it, tol = mg.bicgstab(A, x, b, h, 200, 1e-8)
    res = true_residual(ref1, x.numpy(), b_np)
    print(f"first solve: status {st}, {it} iterations, reported {tol:.3e}, true residual {res:.3e}")
    assert st == 0 and res < 1e-8
    graphs = h.graph_info()["captured_cycles"]
    A.update_values_coo(dev(v2))
    h.refresh()
    assert_csr_equal(A, *ref2[:3])
    info = h.refresh_info()
    assert info["refreshes"] == 1 and info["kept_graphs"] == 1 and h.graph_info()["captured_cycles"] == graphs and graphs > 0
    x.fill(0.0)
    st, it, tol = mg.bicgstab(A, x, b, h, 200, 1e-8)
    res = true_residual(ref2, x.numpy(), b_np)
    print(f"second solve: status {st}, {it} iterations, reported {tol:.3e}, true residual {res:.3e}")
    assert st == 0 and res < 1e-8
    assert true_residual(ref1, x.numpy(), b_np) > 1e-3        # it is the new operator's solution, not the old one's


# ------------------------------------------------------------------ 9. Csr.from_torch
def test_from_torch_coo_and_csr(mg, ctx, case4c, csky10):
    r, c, v1, v2, (rp, ci, val1, _), (_, _, val2, _) = case4c
    t = torch.sparse_coo_tensor(torch.from_numpy(np.stack([r, c])), torch.from_numpy(v1), (300, 300)).to("cuda:0")
    assert not t.is_coalesced()
    A = mg.Csr.from_torch(ctx, t, keep_map=True)
    assert_csr_equal(A, rp, ci, val1)
    assert bits_equal(A.download()[2], coo(mg, ctx, 300, 300, r, c, v1).download()[2])
    A.update_values_coo(dev(v2))
    assert_csr_equal(A, rp, ci, val2)
    n, m, rp3, ci3, v3 = csky10
    crow, cidx = torch.from_numpy(rp3.astype(np.int64)), torch.from_numpy(ci3.astype(np.int64))
    t = torch.sparse_csr_tensor(crow, cidx, torch.from_numpy(v3), size=(n, m)).to("cuda:0")
    assert t.crow_indices().dtype == torch.int64
    B = mg.Csr.from_torch(ctx, t)
    assert_csr_equal(B, rp3, ci3, v3)
    x = ctx.vec(np.random.default_rng(41).standard_normal(m))
    direct = mg.Csr.from_device(ctx, n, m, dev(rp3, np.int64), dev(ci3, np.int64), dev(v3))
    assert bits_equal(B.spmv(x).numpy(), direct.spmv(x).numpy())
    with pytest.raises(TypeError):
        mg.Csr.from_torch(ctx, torch.sparse_csr_tensor(crow, cidx, torch.from_numpy(v3.astype(np.float32)), size=(n, m)).to("cuda:0"))
    with pytest.raises(TypeError):
        mg.Csr.from_torch(ctx, torch.sparse_coo_tensor(torch.from_numpy(np.stack([r, c])), torch.from_numpy(v1.astype(np.float32)), (300, 300)).to("cuda:0"))
    with pytest.raises(TypeError):
        mg.Csr.from_torch(ctx, torch.zeros(3, 3, dtype=torch.float64, device="cuda:0"))
    with pytest.raises(TypeError):
        mg.Csr.from_device(ctx, n, m, dev(rp3, np.int64), dev(ci3, np.int32), dev(v3))      # index widths differ
    with pytest.raises(TypeError):
        mg.Csr.from_device(ctx, n, m, dev(rp3, np.int16), dev(ci3, np.int16), dev(v3))
    with pytest.raises(TypeError):
        mg.Csr.from_device(ctx, n, m, rp3, ci3, v3)                                          # host arrays
