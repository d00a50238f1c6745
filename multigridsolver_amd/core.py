"""Thin Python handles over the C-ABI (include/mgs.h).  Python here is plumbing for tests,
bench.py and the torch.distributed launcher; the host-side solver logic lives in C++
(multigridsolver_amd/csrc/mgs_api.hip, cycle.hip and krylov.hip; multigridsolver_amd/cpp/mgs_host.hpp)."""
import ctypes as C

import numpy as np

from ._lib import ALLREDUCE_FN, HALO_FN, HALO_FUSED_FN, MgsError, check, lib

OP_SPMV, OP_RESIDUAL, OP_JACOBI = 0, 1, 2
OP_MINRES_UPDATE = 3      # Csr.time_kernel only: the update pass of mgs_minres (x = z̃, b = w, dinv = w_prev, out = the solution)
_check = check      # for methods whose own argument is called `check`


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Context:
    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        check(lib().mgs_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(h)))
        self.h = h
        self.device = int(device)
        self._cbs = []

    def close(self):
        if self.h:
            lib().mgs_ctx_destroy(self.h)
            self.h = None

    def sync(self):
        check(lib().mgs_sync(self.h), self.h)

    def trim(self):
        """release the work vectors and scratch the context keeps between solves (mgs_ctx_trim)"""
        check(lib().mgs_ctx_trim(self.h), self.h)

    @property
    def stream(self):
        return lib().mgs_ctx_stream(self.h)

    def set_option(self, key, value):
        check(lib().mgs_ctx_set_option(self.h, key.encode(), int(value)), self.h)

    def set_allreduce(self, fn):
        """fn(np.ndarray of float64) -> None (in-place sum over ranks)"""
        def _cb(_u, ptr, count):
            try:
                fn(np.ctypeslib.as_array(ptr, shape=(count,)))
                return 0
            except Exception:  # noqa: BLE001
                import traceback; traceback.print_exc()
                return 1
        cb = ALLREDUCE_FN(_cb)
        self._cbs.append(cb)
        check(lib().mgs_ctx_set_allreduce(self.h, cb, None), self.h)

    # ---- factories
    def csr(self, rows, cols, rowptr, col, val):
        return Csr.upload(self, rows, cols, rowptr, col, val)

    def vec(self, n_or_array):
        if isinstance(n_or_array, (int, np.integer)):
            return Vec(self, int(n_or_array))
        a = np.ascontiguousarray(n_or_array, dtype=np.float64)
        v = Vec(self, a.size)
        v.upload(a)
        return v

    def poisson3d(self, N, plane_lo=0, plane_hi=None, local_cols=False):
        h = C.c_void_p()
        check(lib().mgs_csr_poisson3d(self.h, N, plane_lo, N if plane_hi is None else plane_hi, int(local_cols), C.byref(h)), self.h)
        return Csr(self, h)

    def poisson2d(self, n):
        h = C.c_void_p()
        check(lib().mgs_csr_poisson2d(self.h, n, C.byref(h)), self.h)
        return Csr(self, h)


def read_mtx(path):
    """readMatrix (reference src/common/MatrixIO.cpp:12-37) → (rows, cols, rowptr, col, val)"""
    rows, cols, nnz = C.c_int(), C.c_int(), C.c_int()
    rp, ci, v = C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_double)()
    check(lib().mgs_mtx_read(path.encode(), C.byref(rows), C.byref(cols), C.byref(nnz), C.byref(rp), C.byref(ci), C.byref(v)))
    try:
        rowptr = np.ctypeslib.as_array(rp, shape=(rows.value + 1,)).copy()
        col = np.ctypeslib.as_array(ci, shape=(max(nnz.value, 1),))[: nnz.value].copy()
        val = np.ctypeslib.as_array(v, shape=(max(nnz.value, 1),))[: nnz.value].copy()
    finally:
        lib().mgs_host_free(rp); lib().mgs_host_free(ci); lib().mgs_host_free(v)
    return rows.value, cols.value, rowptr, col, val


def write_mtx(path, rows, cols, rowptr, col, val):
    """writeMatrix (reference src/common/MatrixIO.cpp:39-57)"""
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32); col = np.ascontiguousarray(col, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float64)
    check(lib().mgs_mtx_write(path.encode(), rows, cols, len(col), _ip(rowptr), _ip(col), _dp(val)))


_NULLSPACE = {None: 0, "constant": 1}      # MGS_NULLSPACE_NONE / MGS_NULLSPACE_CONSTANT (what set_nullspace takes)
_NULLSPACE_NAMES = {0: None, 1: "constant", 2: "fields"}      # ... and MGS_NULLSPACE_FIELDS, entered through set_nullspace_fields only
NULLSPACE_MAX_FIELDS = 8
_INDEX_BITS = {"int32": 32, "int64": 64, "<i4": 32, "<i8": 64}
_FLOAT64 = ("float64", "<f8")


def _dev_array(ctx, a, name, index):
    """(device pointer, element count, index bits or 0) of an array that lives on ctx's device: a torch tensor, an object with
    __cuda_array_interface__, or (values only) a Vec.  Wrong dtype, layout or device: TypeError — nothing is converted."""
    want = "int32 or int64" if index else "float64"
    if isinstance(a, Vec):
        if index:
            raise TypeError(f"{name}: a Vec holds float64 values, {want} indices expected")
        return a.ptr, len(a), 0
    if hasattr(a, "data_ptr") and hasattr(a, "is_contiguous"):          # torch tensor
        dt = str(a.dtype).replace("torch.", "")
        if not a.is_cuda or a.device.index != ctx.device:
            raise TypeError(f"{name}: tensor on {a.device}, the context runs on device {ctx.device}")
        if a.dim() != 1 or not a.is_contiguous():
            raise TypeError(f"{name}: a contiguous one-dimensional tensor expected")
        ptr, n = a.data_ptr(), a.numel()
    elif hasattr(a, "__cuda_array_interface__"):
        cai = a.__cuda_array_interface__
        dt, shape = cai["typestr"], tuple(cai["shape"])
        if len(shape) != 1 or cai.get("strides") not in (None, (int(dt[2:]),)):
            raise TypeError(f"{name}: a contiguous one-dimensional array expected")
        ptr, n = int(cai["data"][0] or 0), shape[0]
    else:
        raise TypeError(f"{name}: a torch tensor, an object with __cuda_array_interface__" + ("" if index else " or a Vec") + f" expected, got {type(a).__name__}")
    if (dt not in _INDEX_BITS) if index else (dt not in _FLOAT64):
        raise TypeError(f"{name}: dtype {dt}, {want} expected (nothing is converted silently)")
    return ptr, n, _INDEX_BITS[dt] if index else 0


class Csr:
    def __init__(self, ctx, h, owned=True):
        self.ctx, self.h, self.owned = ctx, h, owned

    def __del__(self):
        try:
            if self.owned and self.h and self.ctx.h:
                lib().mgs_csr_destroy(self.h)
        except Exception:  # noqa: BLE001
            pass

    @staticmethod
    def upload(ctx, rows, cols, rowptr, col, val):
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32); col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        h = C.c_void_p()
        check(lib().mgs_csr_upload(ctx.h, rows, cols, len(col), _ip(rowptr), _ip(col), _dp(val), C.byref(h)), ctx.h)
        return Csr(ctx, h)

    @staticmethod
    def from_mtx(ctx, path):
        return Csr.upload(ctx, *read_mtx(path))

    @staticmethod
    def from_device(ctx, rows, cols, rowptr, col, val):
        """CSR arrays that live on the context's device (mgs_csr_from_device): int32 or int64 indices, float64 values, checked on the
        device by mgs_csr_upload's rules and copied.  Make them visible first (e.g. torch.cuda.synchronize())."""
        rp, nrp, bits = _dev_array(ctx, rowptr, "rowptr", True)
        ci, nnz, cbits = _dev_array(ctx, col, "col", True)
        v, nv, _ = _dev_array(ctx, val, "val", False)
        if cbits != bits:
            raise TypeError(f"rowptr holds {bits}-bit indices, col {cbits}-bit ones")
        if nrp != rows + 1 or nv != nnz:
            raise ValueError(f"rowptr has {nrp} entries for {rows} rows, col {nnz} and val {nv}")
        h = C.c_void_p()
        check(lib().mgs_csr_from_device(ctx.h, rows, cols, nnz, C.c_void_p(rp), C.c_void_p(ci), bits, C.c_void_p(v), C.byref(h)), ctx.h)
        return Csr(ctx, h)

    @staticmethod
    def from_coo_device(ctx, rows, cols, row, col, val, keep_map=False):
        """triples on the context's device, any order, duplicates summed in input order (mgs_csr_from_coo_device); keep_map=True keeps
        what update_values_coo needs"""
        ri, n, bits = _dev_array(ctx, row, "row", True)
        ci, nc, cbits = _dev_array(ctx, col, "col", True)
        v, nv, _ = _dev_array(ctx, val, "val", False)
        if cbits != bits:
            raise TypeError(f"row holds {bits}-bit indices, col {cbits}-bit ones")
        if nc != n or nv != n:
            raise ValueError(f"row has {n} entries, col {nc} and val {nv}")
        h = C.c_void_p()
        check(lib().mgs_csr_from_coo_device(ctx.h, rows, cols, n, C.c_void_p(ri), C.c_void_p(ci), bits, C.c_void_p(v), int(bool(keep_map)), C.byref(h)), ctx.h)
        return Csr(ctx, h)

    @staticmethod
    def from_torch(ctx, t, keep_map=False):
        """a 2-D float64 torch.sparse_csr or torch.sparse_coo tensor (coalesced or not) on the context's device; torch's current stream
        on that device is synchronised first"""
        import torch
        if t.dim() != 2 or t.layout not in (torch.sparse_csr, torch.sparse_coo):
            raise TypeError(f"from_torch: a 2-D sparse_csr or sparse_coo tensor expected, got layout {t.layout} with {t.dim()} dimensions")
        if t.dtype != torch.float64:
            raise TypeError(f"from_torch: dtype {t.dtype}, float64 expected (nothing is converted silently)")
        if not t.is_cuda or t.device.index != ctx.device:
            raise TypeError(f"from_torch: tensor on {t.device}, the context runs on device {ctx.device}")
        rows, cols = t.shape
        if t.layout == torch.sparse_csr:
            arrays = (t.crow_indices().contiguous(), t.col_indices().contiguous(), t.values().contiguous())
        else:
            if t.sparse_dim() != 2:
                raise TypeError("from_torch: a sparse_coo tensor with two sparse dimensions expected")
            idx = t._indices()
            arrays = (idx[0].contiguous(), idx[1].contiguous(), t._values().contiguous())
        torch.cuda.current_stream(t.device).synchronize()
        if t.layout == torch.sparse_csr:
            return Csr.from_device(ctx, rows, cols, *arrays)
        return Csr.from_coo_device(ctx, rows, cols, *arrays, keep_map=keep_map)

    def update_values_coo(self, val):
        """new triple values (same triples, same order) for a matrix assembled with keep_map=True, through the kept map into the
        existing value array (mgs_csr_update_values_coo_dev; enqueued, not synchronised); returns self.  Follow with Hierarchy.refresh()."""
        v, n, _ = _dev_array(self.ctx, val, "val", False)
        check(lib().mgs_csr_update_values_coo_dev(self.h, C.c_void_p(v), n), self.ctx.h)
        return self

    def coo_info(self):
        out = (C.c_int64 * 4)(); check(lib().mgs_csr_coo_info(self.h, out), self.ctx.h)
        return dict(zip(["triples", "entries", "max_row_triples", "map_bytes"], [int(v) for v in out]))

    def device_ptrs(self):
        """(rowptr, col, val) device addresses of the library's own arrays (mgs_csr_device_ptrs)"""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().mgs_csr_device_ptrs(self.h, C.byref(a), C.byref(b), C.byref(c)), self.ctx.h)
        return a.value or 0, b.value or 0, c.value or 0

    @property
    def shape(self):
        r, c, n = C.c_int(), C.c_int(), C.c_int64()
        lib().mgs_csr_shape(self.h, C.byref(r), C.byref(c), C.byref(n))
        return r.value, c.value

    @property
    def nnz(self):
        n = C.c_int64(); lib().mgs_csr_shape(self.h, None, None, C.byref(n)); return n.value

    def plan_info(self):
        out = (C.c_int64 * 8)(); lib().mgs_csr_plan_info(self.h, out)
        keys = ["max_block_nnz", "max_row_len", "far_band", "lds_bytes", "halo_lo_blocks", "halo_hi_blocks", "halo_split_ok", "has_long_row_blocks"]
        return dict(zip(keys, [int(v) for v in out]))

    def origin(self):
        """finest-level row every row descends from (None: identity) — tie-break space of the device matching"""
        out = np.empty(max(self.shape[0], 1), dtype=np.int32)
        rc = lib().mgs_csr_get_origin(self.h, _ip(out))
        if rc == 1:
            return None
        check(rc, self.ctx.h); return out[: self.shape[0]]

    def set_origin(self, origin):
        o = np.ascontiguousarray(origin, dtype=np.int32)
        check(lib().mgs_csr_set_origin(self.h, _ip(o)), self.ctx.h); return self

    def optimize(self):
        """build the pattern code of the column array (mgs_csr_optimize); returns self"""
        check(lib().mgs_csr_optimize(self.h), self.ctx.h); return self

    def rowcode_info(self):
        out = (C.c_int64 * 4)(); lib().mgs_csr_rowcode_info(self.h, out)
        return dict(zip(["coded_blocks", "blocks", "table_ints", "table_budget"], [int(v) for v in out]))

    def update_values(self, val, n=None):
        """new values, same pattern, in place (mgs_csr_update_values): a host array, or a Vec / a device pointer with its length `n`
        for the device-to-device form; returns self.  Follow with Hierarchy.refresh() on hierarchies built on this matrix."""
        if isinstance(val, Vec):
            check(lib().mgs_csr_update_values_dev(self.h, C.c_void_p(val.ptr), len(val) if n is None else int(n)), self.ctx.h)
        elif isinstance(val, (int, np.integer)):
            if n is None:
                raise ValueError("update_values: a device pointer needs its length n")
            check(lib().mgs_csr_update_values_dev(self.h, C.c_void_p(int(val)), int(n)), self.ctx.h)
        else:
            a = np.ascontiguousarray(val, dtype=np.float64)
            check(lib().mgs_csr_update_values(self.h, _dp(a), a.size), self.ctx.h)
        return self

    def set_nullspace(self, kind):
        """declare the null space: "constant" (A·1 = 0 and 1ᵀ·A = 0: pure-Neumann operators, graph Laplacians) or None; not verified —
        nullspace_defect() is the net.  Hierarchies act on it at their next finalize() / refresh(), the Krylov solvers at their next
        call (mgs_csr_set_nullspace); returns self"""
        if kind not in _NULLSPACE:
            raise ValueError(f"set_nullspace: {kind!r}, expected one of {list(_NULLSPACE)}")
        check(lib().mgs_csr_set_nullspace(self.h, _NULLSPACE[kind]), self.ctx.h); return self

    def nullspace(self):
        """what set_nullspace / set_nullspace_fields declared: "constant", "fields" or None"""
        k = C.c_int(); check(lib().mgs_csr_nullspace(self.h, C.byref(k)), self.ctx.h)
        return _NULLSPACE_NAMES[k.value]

    def set_nullspace_fields(self, labels, nfields=None):
        """declare a field-wise constant null space (mgs_csr_set_nullspace_fields): labels holds one entry per row, f in [0, nfields)
        puts the row in field f, −1 in no field; asserted (not verified): A·z_f = 0 and z_fᵀ·A = 0 for the indicator z_f of every field —
        the pressure constant of enclosed Stokes flow, one constant per component of a graph Laplacian.  labels: a torch int32 / int64
        tensor on the context's device (made visible first) or a numpy integer array (uploaded here); nfields defaults to max + 1.
        Range-checked on the device; served by minres, MinresPlan and pcg.  Returns self."""
        if isinstance(labels, np.ndarray):
            import torch
            if labels.dtype.kind not in "iu":
                raise TypeError(f"set_nullspace_fields: labels of dtype {labels.dtype}, integers expected")
            labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int64)).to(f"cuda:{self.ctx.device}")
            torch.cuda.synchronize(self.ctx.device)
        ptr, n, bits = _dev_array(self.ctx, labels, "labels", True)
        if n != self.shape[0]:
            raise ValueError(f"set_nullspace_fields: labels holds {n} entries, the matrix has {self.shape[0]} rows")
        if nfields is None:
            nfields = int(labels.max()) + 1 if n else 0
        check(lib().mgs_csr_set_nullspace_fields(self.h, C.c_void_p(ptr), bits, int(nfields)), self.ctx.h); return self

    def nullspace_fields(self):
        """(nfields, rows of every field) of a set_nullspace_fields declaration; (0, []) for any other kind"""
        nf = C.c_int(); cnt = (C.c_int64 * NULLSPACE_MAX_FIELDS)()
        check(lib().mgs_csr_nullspace_fields(self.h, C.byref(nf), cnt), self.ctx.h)
        return nf.value, [int(cnt[k]) for k in range(nf.value)]

    def nullspace_defect(self):
        """(‖A·1‖∞ / ‖|A|·1‖∞, the same for Aᵀ): how far the matrix is from the "constant" declaration — on a "fields" matrix the maximum
        over the fields of the same quotients with the field's indicator in the place of 1; a diagnostic, synchronises"""
        out = (C.c_double * 2)(); check(lib().mgs_csr_nullspace_defect(self.h, out), self.ctx.h)
        return float(out[0]), float(out[1])

    def download(self):
        rows, _ = self.shape; nnz = self.nnz
        rp = np.empty(rows + 1, dtype=np.int32); ci = np.empty(max(nnz, 1), dtype=np.int32); v = np.empty(max(nnz, 1))
        check(lib().mgs_csr_download(self.h, _ip(rp), _ip(ci), _dp(v)), self.ctx.h)
        return rp, ci[:nnz], v[:nnz]

    def transpose(self):
        h = C.c_void_p(); check(lib().mgs_csr_transpose(self.h, C.byref(h)), self.ctx.h); return Csr(self.ctx, h)

    def transpose_update(self, A, check=False):
        """this matrix = A.transpose() built earlier: its values again, in place, from the current values of A with its pattern unchanged
        (mgs_csr_transpose_numeric; one launch, no kept map); returns self.  check=False: enqueued, no host wait.  check=True: synchronises
        and raises MgsError (MGS_ERR_STATE, .misses set) when entries of A have no place here (another pattern).  A scaling applied to
        this matrix (scale) is gone after the refill: apply it again.  Follow with Hierarchy.refresh()."""
        if not check:
            _check(lib().mgs_csr_transpose_numeric(A.h, self.h, None), A.ctx.h); return self      # the call reports on A's context
        m = C.c_int64(-1)
        try:
            _check(lib().mgs_csr_transpose_numeric(A.h, self.h, C.byref(m)), A.ctx.h)
        except MgsError as e:
            e.misses = int(m.value)
            raise
        return self

    def galerkin(self, xfer):
        h = C.c_void_p(); check(lib().mgs_csr_galerkin(self.h, xfer.h, C.byref(h)), self.ctx.h); return Csr(self.ctx, h)

    def matmul(self, B):
        """C = self·B on the device (mgs_csr_spgemm): structural pattern, ascending columns, products summed in storage order"""
        if not isinstance(B, Csr):
            raise TypeError(f"matmul: a Csr expected, got {type(B).__name__}")
        h = C.c_void_p(); check(lib().mgs_csr_spgemm(self.h, B.h, C.byref(h)), self.ctx.h); return Csr(self.ctx, h)

    def __matmul__(self, B):
        return self.matmul(B) if isinstance(B, Csr) else NotImplemented

    def matmul_update(self, A, B, check=False):
        """this matrix = A.matmul(B) built earlier: its values again, in place, from the current values of A and B with their patterns
        unchanged (mgs_csr_spgemm_numeric); returns self.  check=False: enqueued, no host wait.  check=True: synchronises and raises
        MgsError (MGS_ERR_STATE, .misses set) when products fall outside this matrix's pattern.  Follow with Hierarchy.refresh()."""
        if not check:
            _check(lib().mgs_csr_spgemm_numeric(A.h, B.h, self.h, None), self.ctx.h); return self
        m = C.c_int64(-1)
        try:
            _check(lib().mgs_csr_spgemm_numeric(A.h, B.h, self.h, C.byref(m)), self.ctx.h)
        except MgsError as e:
            e.misses = int(m.value)
            raise
        return self

    def spgemm_info(self):
        out = (C.c_int64 * 4)(); check(lib().mgs_csr_spgemm_info(self.h, out), self.ctx.h)
        return dict(zip(["lane_rows", "workgroup_rows", "max_row_len", "max_row_products"], [int(v) for v in out]))

    def add(self, B, alpha=1.0, beta=1.0):
        """C = alpha·self + beta·B on the device (mgs_csr_add): the union of the two patterns, ascending columns, every product and sum
        rounded on its own"""
        if not isinstance(B, Csr):
            raise TypeError(f"add: a Csr expected, got {type(B).__name__}")
        h = C.c_void_p(); check(lib().mgs_csr_add(float(alpha), self.h, float(beta), B.h, C.byref(h)), self.ctx.h); return Csr(self.ctx, h)

    def __add__(self, B):
        return self.add(B) if isinstance(B, Csr) else NotImplemented

    def __sub__(self, B):
        return self.add(B, 1.0, -1.0) if isinstance(B, Csr) else NotImplemented

    def add_update(self, A, B, alpha=1.0, beta=1.0, check=False):
        """this matrix = A.add(B, ...) built earlier: its values again, in place, from the current values of A and B with their patterns
        unchanged and the alpha, beta given here (mgs_csr_add_numeric); returns self.  check=False: enqueued, no host wait.  check=True:
        synchronises and raises MgsError (MGS_ERR_STATE, .misses set) when entries are not at their place in this matrix's pattern.
        Follow with Hierarchy.refresh()."""
        if not check:
            _check(lib().mgs_csr_add_numeric(float(alpha), A.h, float(beta), B.h, self.h, None), self.ctx.h); return self
        m = C.c_int64(-1)
        try:
            _check(lib().mgs_csr_add_numeric(float(alpha), A.h, float(beta), B.h, self.h, C.byref(m)), self.ctx.h)
        except MgsError as e:
            e.misses = int(m.value)
            raise
        return self

    def add_info(self):
        out = (C.c_int64 * 4)(); check(lib().mgs_csr_add_info(self.h, out), self.ctx.h)
        return dict(zip(["lane_rows", "wave_rows", "max_row_len", "common_entries"], [int(v) for v in out]))

    def scale(self, left=None, right=None):
        """a_ij ← (left_i·a_ij)·right_j in place (mgs_csr_scale; either Vec may be None: that factor is skipped); enqueued, returns self.
        Follow with Hierarchy.refresh() on hierarchies built on this matrix."""
        check(lib().mgs_csr_scale(self.h, left.h if left is not None else None, right.h if right is not None else None), self.ctx.h); return self

    def diagonal(self):
        """Vec of min(rows, cols) entries: a_ii, 0.0 where row i stores no diagonal entry (mgs_csr_diag)"""
        d = Vec(self.ctx, min(self.shape)); check(lib().mgs_csr_diag(self.h, d.h), self.ctx.h); return d

    @staticmethod
    def from_diag(ctx, vec):
        """the n × n matrix with vec_i stored at (i, i), zeros included (mgs_csr_from_diag)"""
        if not isinstance(vec, Vec):
            raise TypeError(f"from_diag: a Vec expected, got {type(vec).__name__}")
        h = C.c_void_p(); check(lib().mgs_csr_from_diag(ctx.h, vec.h, C.byref(h)), ctx.h); return Csr(ctx, h)

    def extract(self, rows=None, cols=None, keep_map=False):
        """S = self[rows][:, cols] on the device (mgs_csr_extract): index lists on the context's device (torch tensors or objects with
        __cuda_array_interface__, int32 or int64, one width for both; make them visible first); None: every row / every column.  rows
        in any order, repeats allowed; cols strictly ascending, column cols[q] becomes q.  Value bits are copied unchanged.
        keep_map=True keeps what extract_update needs."""
        ptr, n, bits = [None, None], [0, 0], [0, 0]
        for k, (name, a) in enumerate((("rows", rows), ("cols", cols))):
            if a is not None:
                p, n[k], bits[k] = _dev_array(self.ctx, a, name, True)
                ptr[k] = C.c_void_p(p or self.device_ptrs()[0])      # an empty list has no address of its own: any device address, never read
        if bits[0] and bits[1] and bits[0] != bits[1]:
            raise TypeError(f"rows holds {bits[0]}-bit indices, cols {bits[1]}-bit ones")
        h = C.c_void_p()
        check(lib().mgs_csr_extract(self.h, ptr[0], n[0], ptr[1], n[1], bits[0] or bits[1] or 32, int(bool(keep_map)), C.byref(h)), self.ctx.h)
        return Csr(self.ctx, h)

    def extract_update(self, A):
        """this matrix = A.extract(..., keep_map=True) built earlier: its values again, in place, from the current values of A with its
        pattern unchanged (mgs_csr_extract_numeric; enqueued, no host wait); returns self.  Follow with Hierarchy.refresh()."""
        check(lib().mgs_csr_extract_numeric(A.h, self.h), A.ctx.h); return self      # the call reports on A's context

    def extract_info(self):
        out = (C.c_int64 * 4)(); check(lib().mgs_csr_extract_info(self.h, out), self.ctx.h)
        return dict(zip(["lane_rows", "wave_rows", "max_row_len", "map_bytes"], [int(v) for v in out]))

    def permute(self, rows=None, cols=None, keep_map=False):
        """C = self[rows][:, cols] for two permutations on the device (mgs_csr_permute): C[i, j] = self[rows[i], cols[j]].  Index lists
        as in extract (torch tensors or objects with __cuda_array_interface__, int32 or int64, one width for both; make them visible
        first), of exactly shape[0] and shape[1] entries; None: the identity on that side.  Each list must be a bijection (checked on
        the device).  A symmetric reordering passes the same list twice.  Value bits are copied unchanged.  keep_map=True keeps what
        permute_update needs."""
        ptr, bits = [None, None], [0, 0]
        for k, (name, a) in enumerate((("rows", rows), ("cols", cols))):
            if a is not None:
                p, n, bits[k] = _dev_array(self.ctx, a, name, True)
                if n != self.shape[k]:
                    raise ValueError(f"permute: {name} holds {n} entries, the matrix has {self.shape[k]} {name}")
                ptr[k] = C.c_void_p(p or self.device_ptrs()[0])      # an empty list has no address of its own: any device address, never read
        if bits[0] and bits[1] and bits[0] != bits[1]:
            raise TypeError(f"rows holds {bits[0]}-bit indices, cols {bits[1]}-bit ones")
        h = C.c_void_p()
        check(lib().mgs_csr_permute(self.h, ptr[0], ptr[1], bits[0] or bits[1] or 32, int(bool(keep_map)), C.byref(h)), self.ctx.h)
        return Csr(self.ctx, h)

    def permute_update(self, A):
        """this matrix = A.permute(..., keep_map=True) built earlier: its values again, in place, from the current values of A with its
        pattern unchanged (mgs_csr_permute_numeric; enqueued, no host wait); returns self.  Follow with Hierarchy.refresh()."""
        check(lib().mgs_csr_permute_numeric(A.h, self.h), A.ctx.h); return self      # the call reports on A's context

    def permute_info(self):
        out = (C.c_int64 * 4)(); check(lib().mgs_csr_permute_info(self.h, out), self.ctx.h)
        return dict(zip(["lane_rows", "wave_rows", "max_row_len", "map_bytes"], [int(v) for v in out]))

    @staticmethod
    def _block_grid(blocks):
        grid = [list(row) for row in blocks]
        if not grid or not grid[0] or any(len(row) != len(grid[0]) for row in grid):
            raise ValueError("bmat: a non-empty rectangular list of lists of blocks expected")
        for row in grid:
            for b in row:
                if b is not None and not isinstance(b, Csr):
                    raise TypeError(f"bmat: a Csr or None expected, got {type(b).__name__}")
        flat = [b for row in grid for b in row]
        return len(grid), len(grid[0]), flat, (C.c_void_p * len(flat))(*[b.h if b is not None else None for b in flat])

    @staticmethod
    def bmat(ctx, blocks, row_sizes=None, col_sizes=None):
        """the matrix assembled from a grid of blocks on the device (mgs_csr_bmat; scipy.sparse.bmat): blocks is a list of lists of Csr
        or None (a zero block); the same Csr may appear in several places.  row_sizes / col_sizes: the sizes of the block rows /
        columns, needed only where a whole block row or column is None."""
        br, bc, _, arr = Csr._block_grid(blocks)
        sizes = []
        for name, given, count in (("row_sizes", row_sizes, br), ("col_sizes", col_sizes, bc)):
            if given is None:
                sizes.append(None)
            else:
                if len(given) != count:
                    raise ValueError(f"bmat: {name} holds {len(given)} sizes, the grid has {count}")
                sizes.append((C.c_int * count)(*[int(v) for v in given]))
        h = C.c_void_p()
        check(lib().mgs_csr_bmat(ctx.h, br, bc, arr, sizes[0], sizes[1], C.byref(h)), ctx.h)
        return Csr(ctx, h)

    @staticmethod
    def hstack(ctx, blocks):
        """[B0 B1 …] (mgs_csr_bmat with one block row)"""
        return Csr.bmat(ctx, [list(blocks)])

    @staticmethod
    def vstack(ctx, blocks):
        """[B0; B1; …] (mgs_csr_bmat with one block column)"""
        return Csr.bmat(ctx, [[b] for b in blocks])

    @staticmethod
    def block_diag(ctx, blocks):
        """diag(B0, B1, …) (mgs_csr_bmat with None off the diagonal; at most 16 blocks: the grid holds 256 positions)"""
        blocks = list(blocks)
        return Csr.bmat(ctx, [[b if i == j else None for j in range(len(blocks))] for i, b in enumerate(blocks)])

    def bmat_update(self, blocks):
        """this matrix = Csr.bmat(ctx, blocks) built earlier: its values again, in place, from the current values of the blocks with
        their patterns unchanged (mgs_csr_bmat_numeric; one launch); returns self.  Follow with Hierarchy.refresh()."""
        br, bc, _, arr = Csr._block_grid(blocks)
        info = self.bmat_info()      # the C call takes no grid dimensions: it reads as many handles as this matrix recorded
        if info["blocks"] == 0 and info["block_rows"] == 0:
            check(lib().mgs_csr_bmat_numeric(self.h, arr), self.ctx.h)      # not built by bmat: the library's own refusal, which reads no handle
        if (br, bc) != (info["block_rows"], info["block_cols"]):
            raise ValueError(f"bmat_update: a grid of {br} x {bc} blocks given, this matrix was assembled from {info['block_rows']} x {info['block_cols']}")
        check(lib().mgs_csr_bmat_numeric(self.h, arr), self.ctx.h); return self

    def bmat_info(self):
        out = (C.c_int64 * 4)(); check(lib().mgs_csr_bmat_info(self.h, out), self.ctx.h)
        return dict(zip(["blocks", "block_rows", "block_cols", "max_row_len"], [int(v) for v in out]))

    def spmv(self, x, y=None):
        y = y or Vec(self.ctx, self.shape[0])
        check(lib().mgs_spmv(self.h, x.h, y.h), self.ctx.h); return y

    def residual(self, x, b, r=None):
        r = r or Vec(self.ctx, self.shape[0])
        check(lib().mgs_residual(self.h, x.h, b.h, r.h), self.ctx.h); return r

    def diag_inv(self):
        d = Vec(self.ctx, self.shape[0]); check(lib().mgs_diag_inv(self.h, d.h), self.ctx.h); return d

    def jacobi(self, dinv, omega, b, x, out=None):
        out = out or Vec(self.ctx, max(self.shape))
        check(lib().mgs_jacobi(self.h, dinv.h, omega, b.h, x.h, out.h), self.ctx.h); return out

    def time_kernel(self, op, x, b=None, dinv=None, out=None, reps=20):
        out = out or Vec(self.ctx, max(self.shape))
        ms = C.c_double()
        check(lib().mgs_time_kernel(self.h, op, x.h, b.h if b else None, dinv.h if dinv else None, out.h, reps, C.byref(ms)), self.ctx.h)
        return ms.value


class Vec:
    def __init__(self, ctx, n=None, h=None, owned=True):
        self.ctx = ctx
        if h is None:
            h = C.c_void_p(); check(lib().mgs_vec_create(ctx.h, n, C.byref(h)), ctx.h)
        self.h, self.owned = h, owned

    @staticmethod
    def wrap(ctx, device_ptr, n):
        h = C.c_void_p(); check(lib().mgs_vec_wrap(ctx.h, C.c_void_p(device_ptr), n, C.byref(h)), ctx.h)
        return Vec(ctx, h=h)

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                lib().mgs_vec_destroy(self.h)
        except Exception:  # noqa: BLE001
            pass

    def __len__(self):
        return lib().mgs_vec_size(self.h)

    @property
    def ptr(self):
        return lib().mgs_vec_ptr(self.h)

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        check(lib().mgs_vec_upload(self.h, _dp(a), a.size), self.ctx.h); return self

    def numpy(self, n=None):
        n = len(self) if n is None else n
        out = np.empty(n); check(lib().mgs_vec_download(self.h, _dp(out), n), self.ctx.h); return out

    def fill(self, v):
        check(lib().mgs_vec_fill(self.h, float(v)), self.ctx.h); return self

    def rand(self, seed=0, offset=0):
        check(lib().mgs_vec_rand(self.h, seed, offset), self.ctx.h); return self

    def copy_from(self, src):
        check(lib().mgs_vec_copy(src.h, self.h), self.ctx.h); return self

    def _indexed(self, fn, a, idx, b, check):
        p, n, bits = _dev_array(self.ctx, idx, "idx", True)
        if not check:
            _check(fn(a.h, C.c_void_p(p), n, bits, b.h, None), a.ctx.h); return      # the calls report on their first vector's context
        bad = C.c_int64(-1)
        try:
            _check(fn(a.h, C.c_void_p(p), n, bits, b.h, C.byref(bad)), a.ctx.h)
        except MgsError as e:
            e.bad = int(bad.value)
            raise

    def gather(self, idx, out=None, check=False):
        """out[k] = self[idx[k]] (mgs_vec_gather): idx an int32 or int64 index list on the context's device, repeats allowed; an index
        outside the vector is never used, out holds +0.0 there.  check=False: enqueued, no host wait.  check=True: synchronises and
        raises MgsError (MGS_ERR_INVALID, .bad = the number of such indices).  Returns out (a new Vec of len(idx) entries if None)."""
        if out is None:
            out = Vec(self.ctx, _dev_array(self.ctx, idx, "idx", True)[1])
        self._indexed(lib().mgs_vec_gather, self, idx, out, check); return out

    def scatter(self, idx, src, check=False):
        """self[idx[k]] = src[k] (mgs_vec_scatter): the indices must be distinct (with repeats the entry holds one of the values); an
        index outside the vector is skipped; check as in gather.  Returns self."""
        self._indexed(lib().mgs_vec_scatter, src, idx, self, check); return self

    def dot(self, other):
        out = C.c_double(); check(lib().mgs_dot(self.h, other.h, C.byref(out)), self.ctx.h); return out.value

    def nrm2(self):
        out = C.c_double(); check(lib().mgs_nrm2(self.h, C.byref(out)), self.ctx.h); return out.value

    def project_const(self, nrm2=False):
        """self ← self − mean(self) on the device (mgs_vec_project_const) → the mean that was subtracted, read back; nrm2=True:
        (mean, ‖self − mean‖₂ from the same pass)"""
        m, s = C.c_double(), C.c_double()
        check(lib().mgs_vec_project_const(self.h, C.byref(m), C.byref(s) if nrm2 else None), self.ctx.h)
        return (m.value, s.value) if nrm2 else m.value

    def project_fields(self, A, nrm2=False):
        """self ← Πself for the fields A declared (mgs_vec_project_fields): every labelled entry minus its field's mean → the means that
        were subtracted (numpy, one per field), read back; nrm2=True: (means, ‖Πself‖₂ over all rows from the same pass)"""
        nf = A.nullspace_fields()[0]
        m = (C.c_double * max(nf, 1))(); s = C.c_double()
        check(lib().mgs_vec_project_fields(self.h, A.h, m, C.byref(s) if nrm2 else None), self.ctx.h)
        means = np.array([m[k] for k in range(nf)], dtype=np.float64)
        return (means, s.value) if nrm2 else means

    def axpby(self, a, x, b):
        """self = a·x + b·self"""
        check(lib().mgs_axpby(float(a), x.h, float(b), self.h), self.ctx.h); return self

    def axpbypcz(self, a, x, b, y, c):
        """self = a·x + b·y + c·self"""
        check(lib().mgs_axpbypcz(float(a), x.h, float(b), y.h, float(c), self.h), self.ctx.h); return self


class Xfer:
    """Prolongation P (+ restriction Pᵀ) — reference bicg.cpp:32,48."""

    def __init__(self, ctx, h, owned=True):
        self.ctx, self.h, self.owned = ctx, h, owned

    @staticmethod
    def from_csr(P):
        h = C.c_void_p(); check(lib().mgs_xfer_create(P.h, C.byref(h)), P.ctx.h); return Xfer(P.ctx, h)

    def __del__(self):
        try:
            if self.owned and self.h and self.ctx.h:
                lib().mgs_xfer_destroy(self.h)
        except Exception:  # noqa: BLE001
            pass

    @property
    def shape(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        lib().mgs_xfer_shape(self.h, C.byref(a), C.byref(b), C.byref(c)); return a.value, b.value

    @property
    def is_aggregation(self):
        c = C.c_int(); lib().mgs_xfer_shape(self.h, None, None, C.byref(c)); return bool(c.value)

    def agg(self):
        out = np.empty(self.shape[0], dtype=np.int32); check(lib().mgs_xfer_download_agg(self.h, _ip(out)), self.ctx.h); return out

    def restrict(self, r, rc=None):
        rc = rc or Vec(self.ctx, self.shape[1]); check(lib().mgs_restrict(self.h, r.h, rc.h), self.ctx.h); return rc

    def prolong(self, ec, e=None):
        e = e or Vec(self.ctx, self.shape[0]); check(lib().mgs_prolong(self.h, ec.h, e.h), self.ctx.h); return e

    def prolong_add(self, ec, x):
        check(lib().mgs_prolong_add(self.h, ec.h, x.h), self.ctx.h); return x


class Hierarchy:
    """MultiGridPrecond state (reference bicg.cpp:19-62) generalised to a multilevel V-cycle."""

    def __init__(self, A, omega=0.5, nu1=1, nu2=1):
        self.ctx, self.A = A.ctx, A
        h = C.c_void_p(); check(lib().mgs_hier_create(A.ctx.h, A.h, omega, nu1, nu2, C.byref(h)), A.ctx.h)
        self.h = h
        self._cb = None

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                lib().mgs_hier_destroy(self.h)
        except Exception:  # noqa: BLE001
            pass

    def push_P(self, P):
        check(lib().mgs_hier_push_P(self.h, P.h), self.ctx.h); return self

    def coarsen(self, ktg=10.0, npass=2, tou=8.0, coarse_rows=2500, max_levels=32):
        check(lib().mgs_hier_coarsen(self.h, ktg, npass, tou, coarse_rows, max_levels), self.ctx.h); return self

    def finalize(self):
        check(lib().mgs_hier_finalize(self.h), self.ctx.h); return self

    def refresh(self):
        """the fine operator's values changed, its pattern did not (Csr.update_values): recompute the coarse operators, D⁻¹, the fused
        passes' operands and the coarsest inverse in place; aggregates, patterns, codes and cached graphs are kept (mgs_hier_refresh)"""
        check(lib().mgs_hier_refresh(self.h), self.ctx.h); return self

    def refresh_info(self):
        out = (C.c_int64 * 4)(); check(lib().mgs_hier_refresh_info(self.h, out), self.ctx.h)
        return dict(zip(["refreshes", "kept_graphs", "device_levels", "extra_bytes"], [int(v) for v in out]))

    def set_smoother(self, omega, nu1, nu2):
        check(lib().mgs_hier_set_smoother(self.h, omega, nu1, nu2), self.ctx.h); return self

    def set_operand_precision(self, bits, levels=-1):
        """stored precision of the fused passes' matrix operands Â and A·P: 64, or 32 = values rounded to float on the longest eligible
        prefix of at most `levels` levels (< 0: every eligible one); vectors and arithmetic stay FP64 (mgs.h)"""
        check(lib().mgs_hier_set_operand_precision(self.h, int(bits), int(levels)), self.ctx.h); return self

    def operand_precision(self, level):
        """64 or 32: what `level` runs with right now"""
        bits = C.c_int(); check(lib().mgs_hier_operand_precision(self.h, int(level), C.byref(bits)), self.ctx.h); return bits.value

    def set_kcycle(self, levels):
        check(lib().mgs_hier_set_kcycle(self.h, levels), self.ctx.h); return self

    def set_kcycle_entry(self, on=True):
        """K step on level 0 itself when the cycle starts from x = 0 (mgs_hier_set_kcycle_entry)"""
        check(lib().mgs_hier_set_kcycle_entry(self.h, int(bool(on))), self.ctx.h); return self

    def kcycle_scalars(self, level):
        """[ρ1, α1, γ, ρ2, α2] of the last K step of `level` (mgs_hier_kcycle_scalars); waits for the stream"""
        out = (C.c_double * 5)(); check(lib().mgs_hier_kcycle_scalars(self.h, int(level), out), self.ctx.h)
        return [float(v) for v in out]

    def set_correction_scale(self, sigma):
        """over-correction x ← x + σ·P e_c on every level (σ = 1: the reference's form)"""
        check(lib().mgs_hier_set_correction_scale(self.h, float(sigma)), self.ctx.h); return self

    def set_additive(self, on=True):
        """additive form of solve() (reference bicg.cpp:59)"""
        check(lib().mgs_hier_set_additive(self.h, int(bool(on))), self.ctx.h); return self

    @property
    def nlev(self):
        return lib().mgs_hier_nlev(self.h)

    def level_shape(self, l):
        r, n = C.c_int(), C.c_int64(); check(lib().mgs_hier_level_shape(self.h, l, C.byref(r), C.byref(n)), self.ctx.h)
        return r.value, n.value

    def level_A(self, l):
        M = Csr(self.ctx, C.c_void_p(lib().mgs_hier_level_A(self.h, l)), owned=False)
        M._hier = self      # a view into this hierarchy: it keeps the hierarchy alive, so h.level_A(l) may outlive the name h
        return M

    def level_AP(self, l):
        """A·P of level l, the fused post pass's operand (mgs_hier_level_AP): a read-only view like level_A, or None while it has
        not been built (no cycle yet, option merge_ap off, the coarsest level)"""
        p = lib().mgs_hier_level_AP(self.h, l)
        if not p:
            return None
        M = Csr(self.ctx, C.c_void_p(p), owned=False)
        M._hier = self
        return M

    def level_P(self, l):
        T = Xfer(self.ctx, C.c_void_p(lib().mgs_hier_level_P(self.h, l)), owned=False)
        T._hier = self      # as level_A: Hierarchy(...).coarsen(...).level_P(0).agg() must not read a destroyed hierarchy
        return T

    @property
    def vcycle_bytes(self):
        return lib().mgs_hier_vcycle_bytes(self.h)

    def vcycle(self, b, x=None, zero_guess=True):
        x = x or Vec(self.ctx, len(b))
        check(lib().mgs_vcycle(self.h, b.h, x.h, int(zero_guess)), self.ctx.h); return x

    def solve(self, v):
        """MultiGridPrecond::solve (reference bicg.cpp:51-61)"""
        return self.vcycle(v, None, True)

    def fused_info(self, level):
        out = (C.c_int64 * 6)(); check(lib().mgs_hier_fused_info(self.h, level, out), self.ctx.h)
        return dict(zip(["blocks", "has_val_wd", "has_col_agg", "coded_col", "coded_col_halo", "coded_col_agg"], [int(v) for v in out]))

    def group_info(self, level):
        out = (C.c_int64 * 4)(); check(lib().mgs_hier_group_info(self.h, level, out), self.ctx.h)
        return dict(zip(["groups", "paired_groups", "stray_aggregates", "blocks"], [int(v) for v in out]))

    def pack_info(self, level):
        """packed operand values of one level (mgs_hier_pack_info, option pack7): blocks / packed blocks of the pre and the post pass's operand,
        which array the pre pass's copy is of (0 none, 1 Â's values, 2 those without the diagonal entries), whether the last launch of each pass
        ran the packed form (1 / 0, −1 before any launch), and the copies' bytes"""
        out = (C.c_int64 * 8)(); check(lib().mgs_hier_pack_info(self.h, level, out), self.ctx.h)
        return dict(zip(["pre_blocks", "pre_packed", "pre_source", "pre_ran", "post_blocks", "post_packed", "post_ran", "bytes"], [int(v) for v in out]))

    def pre_pass(self, level, b, t, r, rc):
        """the grouped pre pass of one level alone (mgs_hier_pre_pass); returns True if it ran without Â's streamed diagonal"""
        nd = C.c_int(0); check(lib().mgs_hier_pre_pass(self.h, level, b.h, t.h, r.h, rc.h, C.byref(nd)), self.ctx.h)
        return bool(nd.value)

    PRE_PASS_INFO = ["arm", "kernel", "U", "flags", "capv", "capi", "bits", "blocks_coded", "blocks_staged", "blocks_global", "stray_aggregates", "blocks"]

    def pre_pass_info(self, level, b, t, r, rc):
        """the fused pre pass of one level alone, whichever arm its cycle runs (mgs_hier_pre_pass_info).  The grouped arm writes t, rc and the
        r of the stray waves' rows; the other arms write r and rc and leave t alone.  Returns what the launcher decided: arm (0 gather form on
        A, 1 residual on Â, 2 aggregate-parallel, 3 grouped), kernel (0 gather, 1 coded FP64, 2 coded FP32, 4 slice, 5 aggregate-parallel,
        6 grouped sequential sweep, 7 pair kernel), U, flags, capv, capi, bits (1 FP32 values, 2 no diagonal, 4 packed) with fp32 / nodiag /
        packed as booleans, row blocks coded + staged / staged / walking from global memory (−1: not a row-block kernel), the level's stray
        aggregates and row blocks."""
        out = (C.c_int64 * 16)()
        check(lib().mgs_hier_pre_pass_info(self.h, level, b.h, t.h, r.h, rc.h, out), self.ctx.h)
        d = dict(zip(self.PRE_PASS_INFO, [int(v) for v in out]))
        d.update(fp32=bool(d["bits"] & 1), nodiag=bool(d["bits"] & 2), packed=bool(d["bits"] & 4))
        return d

    def post_pass(self, level, bvec, xin, ec, x, range=None):
        """the fused post pass of one level alone (mgs_hier_post_pass): xin None = t-form (bvec holds t = b + r), else bvec = r and xin = b;
        range = (blk_lo, blk_hi, gap_at, gap_len) or None for the whole level.  Returns what the launcher decided."""
        rg = (C.c_int * 4)(*[int(v) for v in range]) if range is not None else None
        out = (C.c_int64 * 8)()
        check(lib().mgs_hier_post_pass(self.h, level, bvec.h, xin.h if xin is not None else None, ec.h, x.h, rg, out), self.ctx.h)
        return dict(zip(["operand", "kernel", "U", "flags", "capv", "capi", "blocks_over_budget", "t_form"], [int(v) for v in out]))

    def graph_info(self):
        out = (C.c_int64 * 4)(); check(lib().mgs_hier_graph_info(self.h, out), self.ctx.h)
        return dict(zip(["captured_cycles", "native_transport", "native_capture_failed", "native_eager_runs"], [int(v) for v in out]))

    def time_vcycle(self, b, x, reps=10):
        ms = C.c_double(); check(lib().mgs_time_vcycle(self.h, b.h, x.h, reps, C.byref(ms)), self.ctx.h); return ms.value

    def set_halo_exchange_split(self, begin, end):
        """begin(level, x_dev_ptr) starts the exchange, end(level, x_dev_ptr) waits for it"""
        def mk(fn):
            def _cb(_u, level, ptr):
                try:
                    fn(level, ptr); return 0
                except Exception:  # noqa: BLE001
                    import traceback; traceback.print_exc(); return 1
            return HALO_FN(_cb)
        self._cb2 = (mk(begin), mk(end))
        check(lib().mgs_hier_set_halo_exchange_split(self.h, self._cb2[0], self._cb2[1], None), self.ctx.h)

    def set_halo_exchange_fused(self, fn):
        """fn(level, kind, a_ptr, b_ptr, halo_out_ptr, phase) — payload exchange of the fused passes"""
        def _cb(_u, level, kind, a, b, out, phase):
            try:
                fn(level, kind, a, b, out, phase); return 0
            except Exception:  # noqa: BLE001
                import traceback; traceback.print_exc(); return 1
        self._cb3 = HALO_FUSED_FN(_cb)
        check(lib().mgs_hier_set_halo_exchange_fused(self.h, self._cb3, None), self.ctx.h)

    def set_halo_exchange(self, fn):
        """fn(level:int, x_dev_ptr:int) -> None"""
        def _cb(_u, level, ptr):
            try:
                fn(level, ptr); return 0
            except Exception:  # noqa: BLE001
                import traceback; traceback.print_exc(); return 1
        self._cb = HALO_FN(_cb)
        check(lib().mgs_hier_set_halo_exchange(self.h, self._cb, None), self.ctx.h)


_GUESS_KIND = {"energy": 0, "residual": 1}      # MGS_GUESS_ENERGY / MGS_GUESS_RESIDUAL


class Guess:
    """Projected initial guesses for successive right-hand sides of one operator (mgs_guess, include/mgs.h): the span of the last
    `capacity` solutions, kept as A-orthonormal ("energy", SPD A) or AᵀA-orthonormal ("residual", any nonsingular A) pairs (x̃, A·x̃).
    A must outlive the guess (it is kept referenced here)."""

    def __init__(self, A, kind="energy", capacity=8):
        if kind not in _GUESS_KIND:
            raise ValueError(f"Guess: kind {kind!r}, expected one of {list(_GUESS_KIND)}")
        self.ctx, self.A, self.kind = A.ctx, A, kind
        h = C.c_void_p(); check(lib().mgs_guess_create(A.h, _GUESS_KIND[kind], int(capacity), C.byref(h)), A.ctx.h)
        self.h = h

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                lib().mgs_guess_destroy(self.h)
        except Exception:  # noqa: BLE001
            pass

    def apply(self, b, x0=None, rel_resid=False):
        """x0 = the projection of b's solution onto the stored span, enqueued; rel_resid=True → (x0, ‖b − A·x0‖/‖b‖) and synchronises"""
        x0 = x0 if x0 is not None else Vec(self.ctx, len(b))
        r = C.c_double()
        check(lib().mgs_guess_apply(self.h, b.h, x0.h, C.byref(r) if rel_resid else None), self.ctx.h)
        return (x0, r.value) if rel_resid else x0

    def update(self, x):
        """offer the solution x to the basis → True if it was added (False: numerically inside the span, or A not positive along it)"""
        a = C.c_int(); check(lib().mgs_guess_update(self.h, x.h, C.byref(a)), self.ctx.h); return bool(a.value)

    def rebase(self):
        """A's values changed (Csr.update_values): recompute every A·x̃ and re-orthonormalise, in place"""
        check(lib().mgs_guess_rebase(self.h), self.ctx.h); return self

    def reset(self):
        check(lib().mgs_guess_reset(self.h), self.ctx.h); return self

    def info(self):
        out = (C.c_int64 * 6)(); check(lib().mgs_guess_info(self.h, out), self.ctx.h)
        return dict(zip(["size", "capacity", "kind", "restarts", "refused", "bytes"], [int(v) for v in out]))

    def coef(self, n=36):
        """α of the last apply, or c¹, c², ν0², ν1², ν2², s, flag of the last update (see mgs_guess_coef); zero padded to n"""
        out = np.zeros(max(int(n), 1)); check(lib().mgs_guess_coef(self.h, _dp(out), int(n)), self.ctx.h); return out[: int(n)]

    def pair(self, k):
        """copies (x̃_k, A·x̃_k) of stored pair k; k = size reads the free slot (x', w' of a refused update, see mgs_guess_pair)"""
        n = self.A.shape[0]
        x, y = Vec(self.ctx, n), Vec(self.ctx, n)
        check(lib().mgs_guess_pair(self.h, int(k), x.h, y.h), self.ctx.h); return x, y

    def gram(self):
        """size × size matrix <q_j, A·x̃_k>: the identity to rounding"""
        k = self.info()["size"]
        out = np.zeros(max(k * k, 1)); check(lib().mgs_guess_gram(self.h, _dp(out)), self.ctx.h); return out[: k * k].reshape(k, k)


class _KrylovPlan:
    """What PcgPlan, BicgstabPlan and FgcrPlan share: the handle's lifetime and the four calls.  _prefix: the C functions are
    mgs_<_prefix>_plan_*; _recursive: mgs_<_prefix>_plan_result has a recursive_resid argument.  A subclass's __init__ sets ctx, A, hier, h."""
    _prefix = None
    _recursive = True
    h = None
    _keep = None

    def _fn(self, name):
        return getattr(lib(), f"mgs_{self._prefix}_plan_{name}")

    def close(self):
        """release the plan's vectors, state block and ring (synchronises); also done when the object goes away"""
        if self.h and self.ctx.h:
            self._fn("destroy")(self.h)
        self.h = None
        self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def solve(self, x, b, max_iter, tol, ahead):
        mi, t, st = C.c_int(max_iter), C.c_double(tol), C.c_int(-1)
        check(self._fn("solve")(self.h, x.h, b.h, int(ahead), C.byref(mi), C.byref(t), C.byref(st)), self.ctx.h)
        return st.value, mi.value, t.value

    def enqueue(self, x, b, iters, tol):
        check(self._fn("enqueue")(self.h, x.h, b.h, int(iters), float(tol)), self.ctx.h)
        self._keep = (self._keep, x, b)
        return self

    def result(self, recursive=False):
        it, r, rec, st = C.c_int(), C.c_double(), C.c_double(), C.c_int(-1)
        if self._recursive:
            rc = self._fn("result")(self.h, C.byref(it), C.byref(r), C.byref(rec) if recursive else None, C.byref(st))
        else:
            rc = self._fn("result")(self.h, C.byref(it), C.byref(r), C.byref(st))
        check(rc, self.ctx.h)
        self._keep = None
        return (st.value, it.value, r.value, rec.value) if recursive else (st.value, it.value, r.value)

    def info(self):
        out = (C.c_int64 * 6)(); check(self._fn("info")(self.h, out), self.ctx.h)
        return [int(v) for v in out]


class PcgPlan(_KrylovPlan):
    """Preconditioned CG with device-resident scalars (mgs_pcg_plan, include/mgs.h): mgs_pcg's arithmetic and bits, with one host look per
    iteration `ahead` iterations behind the queue (solve), or none at all (enqueue, then result).  A and hier must outlive the plan (they are
    kept referenced here)."""
    _prefix, _recursive = "pcg", False

    def __init__(self, A, hier=None, flexible=False):
        self.ctx, self.A, self.hier = A.ctx, A, hier
        h = C.c_void_p()
        check(lib().mgs_pcg_plan_create(A.h, hier.h if hier else None, int(bool(flexible)), C.byref(h)), A.ctx.h)
        self.h = h

    def solve(self, x, b, max_iter=10000, tol=1e-6, ahead=1):
        """mgs_pcg's contract → (status, iterations, achieved_tol)"""
        return super().solve(x, b, max_iter, tol, ahead)

    def enqueue(self, x, b, iters, tol):
        """INIT, `iters` iterations and the final true residual on the context's stream; no host wait.  x and b are kept referenced until result()"""
        return super().enqueue(x, b, iters, tol)

    def result(self):
        """of the last enqueue (synchronises) → (status, iterations done, true relative residual)"""
        return super().result()

    def info(self):
        """[0] device bytes, [1] solves + enqueues, [2] iterations enqueued by the last call, [3] of those run frozen, [4] host waits, [5] restarts"""
        return super().info()


class BicgstabPlan(_KrylovPlan):
    """BiCGSTAB with device-resident scalars (mgs_bicgstab_plan, include/mgs.h): mgs_bicgstab's arithmetic and bits, with one host look per
    iteration `ahead` iterations behind the queue (solve), or none at all (enqueue, then result).  A and hier must outlive the plan (they are
    kept referenced here)."""
    _prefix = "bicgstab"

    def __init__(self, A, hier=None):
        self.ctx, self.A, self.hier = A.ctx, A, hier
        h = C.c_void_p()
        check(lib().mgs_bicgstab_plan_create(A.h, hier.h if hier else None, C.byref(h)), A.ctx.h)
        self.h = h

    def solve(self, x, b, max_iter=10000, tol=1e-6, ahead=1):
        """mgs_bicgstab's contract → (status, iterations, achieved_tol), the tuple bicgstab() returns"""
        return super().solve(x, b, max_iter, tol, ahead)

    def enqueue(self, x, b, iters, tol):
        """INIT, `iters` iterations and the final true residual on the context's stream; no host wait.  x and b are kept referenced until result()"""
        return super().enqueue(x, b, iters, tol)

    def result(self, recursive=False):
        """of the last enqueue (synchronises) → (status, iterations done, true relative residual); recursive=True appends the recursion's residual"""
        return super().result(recursive)

    def info(self):
        """[0] device bytes, [1] solves + enqueues, [2] iterations enqueued by the last call, [3] of those run frozen, [4] host waits, [5] 0"""
        return super().info()


class FgcrPlan(_KrylovPlan):
    """Flexible GCR(restart) with device-resident coefficients (mgs_fgcr_plan, include/mgs.h): mgs_fgcr's arithmetic and bits, with one host look
    per iteration `ahead` iterations behind the queue (solve), or none at all (enqueue, then result).  restart in 1..16.  A and hier must outlive
    the plan (they are kept referenced here)."""
    _prefix = "fgcr"

    def __init__(self, A, hier=None, restart=10):
        self.ctx, self.A, self.hier, self.restart = A.ctx, A, hier, int(restart)
        h = C.c_void_p()
        check(lib().mgs_fgcr_plan_create(A.h, hier.h if hier else None, int(restart), C.byref(h)), A.ctx.h)
        self.h = h

    def solve(self, x, b, max_iter=1000, tol=1e-6, ahead=0):
        """mgs_fgcr's contract → (status, iterations, achieved_tol), the tuple fgcr() returns.  ahead = 0 by default, not the other plans' 1: an iteration
        with a K-cycle is long, and the one that ahead = 1 runs frozen cost 2–3 % of a solve where the look it hides cost nothing measurable
        (profiles/r14_fgcr_plan.md)"""
        return super().solve(x, b, max_iter, tol, ahead)

    def enqueue(self, x, b, iters, tol):
        """INIT, `iters` iterations with their scheduled window closes and FINAL on the context's stream; no host wait.  x and b are kept referenced until result()"""
        return super().enqueue(x, b, iters, tol)

    def result(self, recursive=False):
        """of the last enqueue (synchronises) → (status, iterations done, true relative residual); recursive=True appends the recursion's residual"""
        return super().result(recursive)

    def info(self):
        """[0] device bytes, [1] solves + enqueues, [2] iterations enqueued by the last call, [3] of those run frozen, [4] host waits, [5] restarts from the true residual"""
        return super().info()


class MinresPlan(_KrylovPlan):
    """Preconditioned MINRES with device-resident scalars (mgs_minres_plan, include/mgs.h): mgs_minres's arithmetic and bits, with one host look
    per iteration `ahead` iterations behind the queue (solve), or none at all (enqueue, then result).  hier: V(ν, ν), no K-cycle, no declared
    constant null space; a field-wise one (Csr.set_nullspace_fields on A and on hier's matrix) is served as in minres().  A and hier must
    outlive the plan (they are kept referenced here)."""
    _prefix = "minres"

    def __init__(self, A, hier=None):
        self.ctx, self.A, self.hier = A.ctx, A, hier
        h = C.c_void_p()
        check(lib().mgs_minres_plan_create(A.h, hier.h if hier else None, C.byref(h)), A.ctx.h)
        self.h = h

    def solve(self, x, b, max_iter=10000, tol=1e-6, ahead=1):
        """mgs_minres's contract → (status, iterations, true relative residual), the tuple minres() returns.  ahead = 1 as for the PCG and
        BiCGSTAB plans: against 0 it is 5 % faster where an iteration takes 0.36 ms and 0.8 % slower where it takes 2.3 ms (profiles/r23_minres_plan.md)"""
        return super().solve(x, b, max_iter, tol, ahead)

    def enqueue(self, x, b, iters, tol):
        """INIT, `iters` iterations and the final true residual on the context's stream; no host wait.  x and b are kept referenced until
        result().  There is no recalibration on the device: status 1 with fewer iterations done than asked for means the estimate ran
        ahead of the 2-norm; enqueue again from x"""
        return super().enqueue(x, b, iters, tol)

    def result(self, recursive=False):
        """of the last enqueue (synchronises) → (status, iterations done, true relative residual); recursive=True appends the estimate κ·|η|/‖b‖"""
        return super().result(recursive)

    def info(self):
        """[0] device bytes, [1] solves + enqueues, [2] iterations enqueued by the last call, [3] of those run frozen, [4] host waits, [5] recalibrations"""
        return super().info()


def bicgstab(A, x, b, hier=None, max_iter=10000, tol=1e-6):
    """BiCGSTABiml (reference bicg.cpp:74-136) → (status, iterations, achieved_tol)"""
    mi, t, st = C.c_int(max_iter), C.c_double(tol), C.c_int(-1)
    check(lib().mgs_bicgstab(A.h, x.h, b.h, hier.h if hier else None, C.byref(mi), C.byref(t), C.byref(st)), A.ctx.h)
    return st.value, mi.value, t.value


def fgcr(A, x, b, hier=None, restart=10, max_iter=1000, tol=1e-6):
    """flexible GCR(restart) for the K-cycle preconditioner → (status, iterations, achieved_tol)"""
    mi, t, st = C.c_int(max_iter), C.c_double(tol), C.c_int(-1)
    check(lib().mgs_fgcr(A.h, x.h, b.h, hier.h if hier else None, restart, C.byref(mi), C.byref(t), C.byref(st)), A.ctx.h)
    return st.value, mi.value, t.value


def pcg(A, x, b, hier=None, max_iter=10000, tol=1e-6, flexible=False):
    """preconditioned CG for symmetric positive definite A (reference src/CPU_Matlab/solve.m:28-31) → (status, iterations, achieved_tol);
    status 0 converged on the true residual / 1 max_iter / 2 r·z ≤ 0 / 3 p·A·p ≤ 0.  flexible=True: β = z·(r − r_prev)/ρ_prev, for a
    preconditioner that is not a fixed symmetric operator (V(ν1 ≠ ν2), K-cycle)"""
    mi, t, st = C.c_int(max_iter), C.c_double(tol), C.c_int(-1)
    check(lib().mgs_pcg(A.h, x.h, b.h, hier.h if hier else None, int(bool(flexible)), C.byref(mi), C.byref(t), C.byref(st)), A.ctx.h)
    return st.value, mi.value, t.value


def minres(A, x, b, hier=None, max_iter=10000, tol=1e-6):
    """preconditioned MINRES for symmetric A that may be indefinite (saddle-point systems), hier a symmetric positive definite preconditioner:
    V(ν, ν), no K-cycle (reference src/CPU_Matlab/solve.m:28-33 chooses between pcg and bicgstab; it has no MINRES) → (status, iterations, resid);
    resid is the true relative residual whatever the status; status 0 converged on the true residual / 1 max_iter / 2 z̃·v negative or not a
    number (preconditioner not positive definite) / 3 Krylov space exhausted above the tolerance (singular, inconsistent system).
    A with Csr.set_nullspace_fields (enclosed flow: the pressure constant; hier's matrix declared alike): solves A·x = Πb, resid is
    ‖Π(b − A·x)‖/‖Πb‖, b is only read, the fields of x come back with zero mean"""
    mi, t, st = C.c_int(max_iter), C.c_double(tol), C.c_int(-1)
    check(lib().mgs_minres(A.h, x.h, b.h, hier.h if hier else None, C.byref(mi), C.byref(t), C.byref(st)), A.ctx.h)
    return st.value, mi.value, t.value


def _handles(vecs):
    return (C.c_void_p * max(len(vecs), 1))(*[v.h for v in vecs])


def vecs_gram(U, V, n=None):
    """G = UᵀV for two lists of Vec columns (mgs_vecs_gram) → numpy (len(U), len(V)); one pass per 8 × 8 tile, bit-reproducible; the same
    list on both sides gives a G that is symmetric bit for bit.  n: leading entries that take part (default: len(U[0]))"""
    ctx = U[0].ctx
    n = len(U[0]) if n is None else n
    G = np.empty((len(U), len(V)))
    check(lib().mgs_vecs_gram(ctx.h, n, len(U), _handles(U), len(V), _handles(V), _dp(G)), ctx.h)
    return G


def vecs_combine(S, Cm, out, n=None):
    """out_j = Σ_a Cm[a, j]·S_a for lists of Vec columns (mgs_vecs_combine), added in ascending a, each product and sum rounded on its own;
    an output may be one of the inputs (the whole vector).  Enqueued, no host wait.  → out"""
    ctx = S[0].ctx
    n = len(S[0]) if n is None else n
    Cm = np.ascontiguousarray(Cm, dtype=np.float64).reshape(len(S), len(out))
    check(lib().mgs_vecs_combine(ctx.h, n, len(S), _handles(S), len(out), _handles(out), _dp(Cm)), ctx.h)
    return out


def vecs_info(ctx):
    """launch decisions of the last vecs_gram / vecs_combine: [0] workgroups, [1] [2] tile rows / columns (combine: inputs / outputs),
    [3] 16-byte path, [4] passes, [5] symmetric route, [6] 1 Gram / 2 combine, [7] 0"""
    out = (C.c_int64 * 8)(); check(lib().mgs_vecs_info(ctx.h, out), ctx.h); return [int(v) for v in out]


def lobpcg(A, X, hier=None, max_iter=200, tol=1e-6, B=None):
    """the len(X) smallest eigenpairs of the symmetric A by LOBPCG with hier's cycle as preconditioner (mgs_eig_lobpcg) →
    (status, iterations, theta, resid).  X: list of Vec, start vectors in, orthonormal Ritz vectors out (ascending theta);
    resid[j] = ‖A·x_j − θ_j·x_j‖₂/‖A‖∞ from a fresh A·X; status 0 all below tol / 1 max_iter / 2 start block rank deficient /
    3 trial basis rank deficient or not a number.  A declared null space (Csr.set_nullspace / set_nullspace_fields): the eigenpairs on its
    complement.
    B: a symmetric positive definite Csr: the smallest eigenpairs of A·x = λ·B·x (mgs_eig_lobpcg_gen); X comes back B-orthonormal,
    resid[j] = ‖A·x_j − θ_j·B·x_j‖₂/(‖A‖∞ + |θ_j|·‖B‖∞), status 2 also for a B that XᵀBX shows not to be positive definite; no declared null
    space on A or B.  B=None is the call above, bit for bit"""
    m = len(X)
    th, rs = np.zeros(max(m, 1)), np.zeros(max(m, 1))
    mi, t, st = C.c_int(max_iter), C.c_double(tol), C.c_int(-1)
    check(lib().mgs_eig_lobpcg_gen(A.h, B.h if B is not None else None, hier.h if hier else None, m, _handles(X), _dp(th), _dp(rs), C.byref(mi), C.byref(t),
                                   C.byref(st)), A.ctx.h)
    return st.value, mi.value, th[:m].copy(), rs[:m].copy()


def eig_residual(ax, bx, theta, r):
    """r = ax − θ·bx and → ‖r‖² in one pass (mgs_eig_residual): r_i = fl(ax_i − fl(θ·bx_i)), the sum with mgs_dot's folds, so the result carries
    the bits of r.dot(r).  r may be ax or bx"""
    s = C.c_double(0.0)
    check(lib().mgs_eig_residual(ax.ctx.h, len(r), ax.h, bx.h, float(theta), r.h, C.byref(s)), ax.ctx.h)
    return s.value


def eig_info(ctx):
    """counters of the last lobpcg on ctx: [0] iterations, [1] cycles, [2] SpMVs (of A and, with B, of B), [3] restarts without P, [4] columns
    locked at the end, [5] work vectors, [6] hipGraph captures made during the call, [7] SpMVs of B alone (0 without B)"""
    out = (C.c_int64 * 8)(); check(lib().mgs_eig_info(ctx.h, out), ctx.h); return [int(v) for v in out]
