// mgs_api.hip — C-ABI implementation (include/mgs.h): the arena, context, device containers, primitives and the
// multilevel hierarchy (construction, options, refresh); the operands of the fused passes are hier_operands.hip, the cycle is cycle.hip, the Krylov
// solvers krylov.hip.
// The host logic is C++; every numeric step is a HIP kernel on the context's stream.  No CPU fallback.
#include "mgs_internal.hpp"

#include <cmath>

thread_local std::string g_mgs_last_error;

// ------------------------------------------------------------------ device memory arena (see mgs_internal.hpp)
#include <algorithm>
#include <map>
#include <mutex>
namespace {
struct Arena {
  char *base = nullptr; size_t cap = 0; bool tried = false;
  int device = -1;                          // the arena lives on ONE device (the one current when it was taken) and serves only that one
  std::map<size_t, size_t> free_blocks;     // offset → size, address ordered
  std::map<size_t, size_t> used;            // offset → size
  std::mutex m;
} g_arena;
bool arena_take_locked(size_t cap) {
  void *p = nullptr;
  if (hipMalloc(&p, cap) != hipSuccess) { (void)hipGetLastError(); return false; }
  g_arena.base = (char *)p; g_arena.cap = cap; g_arena.free_blocks[0] = cap;
  if (hipGetDevice(&g_arena.device) != hipSuccess) g_arena.device = -1;
  return true;
}
void arena_init_locked() {
  if (g_arena.tried) return;
  g_arena.tried = true;
  const char *e = getenv("MGS_ARENA_GB");
  const double gb = e ? atof(e) : 0.0;
  if (gb <= 0.0) return;
  if (!arena_take_locked((size_t)(gb * 1024.0) << 20)) fprintf(stderr, "[mgs] arena of %.1f GiB not available: plain hipMalloc\n", gb);
}
}  // namespace
// One arena per process, on the device current at the reservation: a context on another device of the same process allocates with
// plain hipMalloc (its operators must not land in a peer's memory).  Reserved before the library's first device allocation (else MGS_ARENA_GB decides at that allocation).
extern "C" int mgs_arena_reserve(size_t bytes) {
  std::lock_guard<std::mutex> lk(g_arena.m);
  if (g_arena.base) return mgs_fail(nullptr, MGS_ERR_STATE, "mgs_arena_reserve: an arena of %zu bytes exists already", g_arena.cap);
  g_arena.tried = true;
  if (bytes == 0) return MGS_OK;                                   // explicit "no arena", whatever the environment says
  if (!arena_take_locked(bytes)) return mgs_fail(nullptr, MGS_ERR_ALLOC, "mgs_arena_reserve: hipMalloc(%zu bytes) failed", bytes);
  return MGS_OK;
}
extern "C" int mgs_arena_info(size_t out[3]) {                     // capacity, bytes in use, largest free block
  std::lock_guard<std::mutex> lk(g_arena.m);
  size_t used = 0, big = 0;
  for (auto &u : g_arena.used) used += u.second;
  for (auto &f : g_arena.free_blocks) big = std::max(big, f.second);
  out[0] = g_arena.cap; out[1] = used; out[2] = big;
  return MGS_OK;
}
hipError_t mgs_hip_malloc(void **p, size_t bytes) {
  {
    std::lock_guard<std::mutex> lk(g_arena.m);
    arena_init_locked();
    int cur = -1;
    if (g_arena.base && hipGetDevice(&cur) == hipSuccess && cur == g_arena.device) {
      const size_t align = bytes >= ((size_t)1 << 20) ? ((size_t)2 << 20) : (size_t)4096;
      const size_t need = (std::max(bytes, (size_t)1) + align - 1) / align * align;
      for (auto it = g_arena.free_blocks.begin(); it != g_arena.free_blocks.end(); ++it) {
        const size_t off = (it->first + align - 1) / align * align, pad = off - it->first;
        if (it->second < pad + need) continue;
        const size_t bo = it->first, bs = it->second;
        g_arena.free_blocks.erase(it);
        if (pad) g_arena.free_blocks[bo] = pad;
        if (bs > pad + need) g_arena.free_blocks[off + need] = bs - pad - need;
        g_arena.used[off] = need;
        *p = g_arena.base + off;
        return hipSuccess;
      }
    }
  }
  return hipMalloc(p, bytes);
}
hipError_t mgs_hip_free(void *p) {
  if (!p) return hipSuccess;
  {
    std::lock_guard<std::mutex> lk(g_arena.m);
    if (g_arena.base && (char *)p >= g_arena.base && (char *)p < g_arena.base + g_arena.cap) {
      const size_t off = (size_t)((char *)p - g_arena.base);
      auto u = g_arena.used.find(off);
      if (u == g_arena.used.end()) return hipErrorInvalidValue;
      size_t bo = off, bs = u->second;
      g_arena.used.erase(u);
      {   // hipFree's contract: nothing in flight touches the block afterwards — on the ARENA's device, whatever is current
        int cur = -1;
        const bool sw = hipGetDevice(&cur) == hipSuccess && g_arena.device >= 0 && cur != g_arena.device;
        if (sw) (void)hipSetDevice(g_arena.device);
        (void)hipDeviceSynchronize();
        if (sw) (void)hipSetDevice(cur);
      }
      auto nx = g_arena.free_blocks.lower_bound(bo);
      if (nx != g_arena.free_blocks.end() && nx->first == bo + bs) { bs += nx->second; nx = g_arena.free_blocks.erase(nx); }
      if (nx != g_arena.free_blocks.begin()) { auto pv = std::prev(nx); if (pv->first + pv->second == bo) { bo = pv->first; bs += pv->second; g_arena.free_blocks.erase(pv); } }
      g_arena.free_blocks[bo] = bs;
      return hipSuccess;
    }
  }
  return hipFree(p);
}

int mgs_fail(mgs_ctx *ctx, int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  g_mgs_last_error = buf;
  if (ctx) ctx->err = buf;
  return code;
}

extern "C" {

const char *mgs_version(void) { return "multigridsolver_amd 0.1 (gfx950, f64)"; }

// ------------------------------------------------------------------ context
int mgs_ctx_create(int device, void *stream, mgs_ctx **out) {
  if (!out) return mgs_fail(nullptr, MGS_ERR_INVALID, "mgs_ctx_create: out is NULL");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return mgs_fail(nullptr, MGS_ERR_HIP, "no HIP device available (%s): libmgs has no CPU fallback", e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  if (device < 0 || device >= ndev) return mgs_fail(nullptr, MGS_ERR_INVALID, "device %d out of range (0..%d)", device, ndev - 1);
  MGS_HIP(nullptr, hipSetDevice(device));
  mgs_ctx *c = new mgs_ctx();
  c->device = device;
  if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
  else { e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking); if (e != hipSuccess) { delete c; return mgs_fail(nullptr, MGS_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); } c->own_stream = true; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->n_cu = prop.multiProcessorCount;
  c->red_cap = MGS_RED_CAP;  // partials + the folded results + the device-only scalars (the projection's mean), see mgs_internal.hpp
  if (mgs_hip_malloc((void **)&c->red_dev, sizeof(double) * c->red_cap) != hipSuccess || hipHostMalloc((void **)&c->red_host, sizeof(double) * 2 * MGS_RED_VALS, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
    delete c; return mgs_fail(nullptr, MGS_ERR_ALLOC, "context scratch allocation failed");
  }
  for (int q = 0; q < 2 * MGS_RED_VALS; ++q) c->red_host[q] = 0.0;
  if (hipHostGetDevicePointer((void **)&c->red_host_dev, c->red_host, 0) != hipSuccess) { c->red_host_dev = nullptr; (void)hipGetLastError(); }
  // MGS_OPTIONS="key=value,key=value": initial option values of every context (A/B runs of whole test suites)
  if (const char *env = getenv("MGS_OPTIONS")) {
    std::string all(env);
    size_t pos = 0;
    while (pos < all.size()) {
      size_t end = all.find(',', pos); if (end == std::string::npos) end = all.size();
      const std::string kv = all.substr(pos, end - pos); const size_t eq = kv.find('=');
      if (eq != std::string::npos && mgs_ctx_set_option(c, kv.substr(0, eq).c_str(), atoi(kv.c_str() + eq + 1)) != MGS_OK) {
        const std::string msg = g_mgs_last_error; mgs_ctx_destroy(c); return mgs_fail(nullptr, MGS_ERR_INVALID, "MGS_OPTIONS: %s", msg.c_str());
      }
      pos = end + 1;
    }
  }
  *out = c;
  return MGS_OK;
}
int mgs_ctx_destroy(mgs_ctx *c) {
  if (!c) return MGS_OK;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  for (mgs_vec *v : c->ws_free) mgs_vec_destroy(v);
  c->ws_free.clear();
  if (c->red_dev) mgs_hip_free(c->red_dev);
  if (c->dot_part) mgs_hip_free(c->dot_part);
  if (c->vecs_dev) mgs_hip_free(c->vecs_dev);
  if (c->vecs_host) hipHostFree(c->vecs_host);
  for (hipEvent_t e : c->vecs_ev) if (e) hipEventDestroy(e);
  if (c->red_host) hipHostFree(c->red_host);
  if (c->own_stream) hipStreamDestroy(c->stream);
  if (c->comm_stream) hipStreamDestroy(c->comm_stream);
  delete c;
  return MGS_OK;
}
const char *mgs_last_error(const mgs_ctx *ctx) { return ctx ? ctx->err.c_str() : g_mgs_last_error.c_str(); }
int mgs_sync(mgs_ctx *ctx) { MGS_HIP(ctx, hipStreamSynchronize(ctx->stream)); return MGS_OK; }
void *mgs_ctx_stream(mgs_ctx *ctx) { return (void *)ctx->stream; }
// Releases what the context keeps between calls: the Krylov solvers' work vectors (8 vectors of the operator's size after a
// BiCGSTAB solve) and the partial-sum scratch of the fused inner products.
int mgs_ctx_trim(mgs_ctx *ctx) {
  MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (mgs_vec *v : ctx->ws_free) mgs_vec_destroy(v);
  ctx->ws_free.clear();
  if (ctx->dot_part) { mgs_hip_free(ctx->dot_part); ctx->dot_part = nullptr; ctx->dot_part_cap = 0; }
  return MGS_OK;
}
int mgs_ctx_set_option(mgs_ctx *ctx, const char *key, int value) {
  std::string k(key ? key : "");
  if (k == "xcd_remap") ctx->opt_xcd_remap = value;
  else if (k == "nontemporal") ctx->opt_nontemporal = value;
  else if (k == "spmv_variant") ctx->opt_spmv_variant = value;
  else if (k == "graph") ctx->opt_graph = value;
  else if (k == "graph_split_rows") ctx->opt_graph_split_rows = value;
  else if (k == "strip") ctx->opt_strip = value;
  else if (k == "fuse") ctx->opt_fuse = value;
  else if (k == "lds_pad") ctx->opt_lds_pad = value;
  else if (k == "fuse_operands") ctx->opt_fuse_operands = value;
  else if (k == "rowcode") ctx->opt_rowcode = value;
  else if (k == "nt_store") ctx->opt_nt_store = value;
  else if (k == "valcode") ctx->opt_valcode = value;
  else if (k == "split_min_rows") ctx->opt_split_min_rows = value;
  else if (k == "blkptr") ctx->opt_blkptr = value;
  else if (k == "fuse_restrict") ctx->opt_fuse_restrict = value;
  else if (k == "diag_from_values") ctx->opt_diag_from_values = value;
  else if (k == "fuse_dots") ctx->opt_fuse_dots = value;
  else if (k == "merge_ap") ctx->opt_merge_ap = value;
  else if (k == "group_strip") ctx->opt_group_strip = value;
  else if (k == "group_order") ctx->opt_group_order = value;
  else if (k == "group_stray_pct") ctx->opt_group_stray_pct = value;
  else if (k == "group_blocks") ctx->opt_group_blocks = value;
  else if (k == "group_min_link") ctx->opt_group_min_link = value;
  else if (k == "group_concurrent") ctx->opt_group_concurrent = value;
  else if (k == "group_sweep") ctx->opt_group_sweep = value;
  else if (k == "group_min_blocks") ctx->opt_group_min_blocks = value;
  else if (k == "native_graph") ctx->opt_native_graph = value;
  else if (k == "native_overlap") ctx->opt_native_overlap = value;
  else if (k == "blas1_vec") ctx->opt_blas1_vec = value;
  else if (k == "post_results") ctx->opt_post_results = value;
  else if (k == "blas1_pairs") ctx->opt_blas1_pairs = value;
  else if (k == "minres_nt") ctx->opt_minres_nt = value;
  else if (k == "stage_unroll")ctx->opt_stage_unroll = value;
  else if (k == "rowptr_scan") ctx->opt_rowptr_scan = value;
  else if (k == "pre_nodiag") ctx->opt_pre_nodiag = value;
  else if (k == "pack7") ctx->opt_pack7 = value;
  else if (k == "kcycle_energy") ctx->opt_kcycle_energy = value;
  else if (k == "aggpre_max_rows") ctx->opt_aggpre_max_rows = value;
  else if (k == "emu_split_self") ctx->opt_emu_split_self = value;
  else return mgs_fail(ctx, MGS_ERR_INVALID, "unknown option '%s'", k.c_str());
  ++ctx->opt_epoch;      // every captured cycle was recorded under the old options: mgs_vcycle drops them
  return MGS_OK;
}
int mgs_ctx_set_native_allreduce(mgs_ctx *ctx, mgs_comm *c) { ctx->ncomm = c; return MGS_OK; }
int mgs_ctx_set_allreduce(mgs_ctx *ctx, mgs_allreduce_fn fn, void *user) { ctx->allreduce = fn; ctx->allreduce_user = user; return MGS_OK; }

}  // extern "C"

// ------------------------------------------------------------------ CSR
int mgs_csr_alloc(mgs_ctx *ctx, int rows, int cols, int64_t nnz, mgs_csr **out) {
  MGS_CHECK(ctx, rows >= 0 && cols >= 0 && nnz >= 0 && nnz < 2147483647LL, MGS_ERR_INVALID, "csr: bad shape %d x %d nnz %lld", rows, cols, (long long)nnz);
  mgs_csr *A = new mgs_csr();
  A->ctx = ctx; A->rows = rows; A->cols = cols; A->nnz = nnz;
  int rc = mgs_dev_alloc(ctx, &A->rowptr, (size_t)rows + 1);
  if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &A->col, (size_t)nnz + 4);
  if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &A->val, (size_t)nnz + 4);
  if (rc != MGS_OK) { mgs_csr_destroy(A); return rc; }
  *out = A;
  return MGS_OK;
}

extern "C" {

int mgs_csr_upload(mgs_ctx *ctx, int rows, int cols, int64_t nnz, const int *rowptr, const int *col, const double *val, mgs_csr **out) {
  MGS_CHECK(ctx, ctx && out && rowptr && (nnz == 0 || (col && val)), MGS_ERR_INVALID, "mgs_csr_upload: NULL argument");
  MGS_CHECK(ctx, rowptr[0] == 0 && rowptr[rows] == nnz, MGS_ERR_INVALID, "mgs_csr_upload: rowptr[0]=%d rowptr[rows]=%d nnz=%lld inconsistent", rowptr[0], rowptr[rows], (long long)nnz);
  for (int i = 0; i < rows; ++i) {
    MGS_CHECK(ctx, rowptr[i] <= rowptr[i + 1], MGS_ERR_INVALID, "mgs_csr_upload: rowptr not monotone at row %d", i);
    for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) {
      MGS_CHECK(ctx, col[k] >= 0 && col[k] < cols, MGS_ERR_INVALID, "mgs_csr_upload: column %d out of range in row %d", col[k], i);
      MGS_CHECK(ctx, k == rowptr[i] || col[k - 1] < col[k], MGS_ERR_INVALID, "mgs_csr_upload: columns of row %d not strictly ascending", i);
    }
  }
  mgs_csr *A = nullptr;
  MGS_TRY(mgs_csr_alloc(ctx, rows, cols, nnz, &A));
  hipMemcpyAsync(A->rowptr, rowptr, sizeof(int) * ((size_t)rows + 1), hipMemcpyHostToDevice, ctx->stream);
  if (nnz) {
    hipMemcpyAsync(A->col, col, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice, ctx->stream);
    hipMemcpyAsync(A->val, val, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, ctx->stream);
  }
  hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { mgs_csr_destroy(A); return mgs_fail(ctx, MGS_ERR_HIP, "csr upload: %s", hipGetErrorString(e)); }
  int rc = mgs_plan_csr(A);
  if (rc != MGS_OK) { mgs_csr_destroy(A); return rc; }
  *out = A;
  return MGS_OK;
}
// matrices that already live in device memory (ingest.hip)
int mgs_csr_from_device(mgs_ctx *ctx, int rows, int cols, int64_t nnz, const void *rowptr_dev, const void *col_dev, int index_bits, const void *val_dev, mgs_csr **out) {
  return k_csr_from_device(ctx, rows, cols, nnz, rowptr_dev, col_dev, index_bits, val_dev, out);
}
int mgs_csr_from_coo_device(mgs_ctx *ctx, int rows, int cols, int64_t ntrip, const void *row_dev, const void *col_dev, int index_bits, const void *val_dev, int keep_map,
                            mgs_csr **out) {
  return k_csr_from_coo_device(ctx, rows, cols, ntrip, row_dev, col_dev, index_bits, val_dev, keep_map, out);
}
int mgs_csr_coo_info(const mgs_csr *A, int64_t out[4]) {
  MGS_CHECK(nullptr, A && out, MGS_ERR_INVALID, "mgs_csr_coo_info: NULL argument");
  out[0] = A->coo_map ? A->coo_ntrip : 0; out[1] = A->nnz; out[2] = A->coo_max_row;
  out[3] = A->coo_map ? (int64_t)sizeof(int) * (A->coo_ntrip + A->nnz + 1) : 0;
  return MGS_OK;
}
int mgs_csr_download(const mgs_csr *A, int *rowptr, int *col, double *val) {
  mgs_ctx *ctx = A->ctx;
  if (rowptr) MGS_HIP(ctx, hipMemcpyAsync(rowptr, A->rowptr, sizeof(int) * ((size_t)A->rows + 1), hipMemcpyDeviceToHost, ctx->stream));
  if (col && A->nnz) MGS_HIP(ctx, hipMemcpyAsync(col, A->col, sizeof(int) * (size_t)A->nnz, hipMemcpyDeviceToHost, ctx->stream));
  if (val && A->nnz) MGS_HIP(ctx, hipMemcpyAsync(val, A->val, sizeof(double) * (size_t)A->nnz, hipMemcpyDeviceToHost, ctx->stream));
  MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MGS_OK;
}
int mgs_csr_shape(const mgs_csr *A, int *rows, int *cols, int64_t *nnz) {
  if (rows) *rows = A->rows; if (cols) *cols = A->cols; if (nnz) *nnz = A->nnz;
  return MGS_OK;
}
int mgs_csr_device_ptrs(const mgs_csr *A, void **rowptr, void **col, void **val) {
  if (rowptr) *rowptr = A->rowptr; if (col) *col = A->col; if (val) *val = A->val;
  return MGS_OK;
}
int mgs_csr_plan_info(const mgs_csr *A, int64_t out[8]) {
  out[0] = A->max_block_nnz; out[1] = A->max_row_len; out[2] = A->far_band; out[3] = (int64_t)(A->lds_cap + 2) * 12 + 16;
  out[4] = A->halo_lo_blocks; out[5] = A->halo_hi_blocks; out[6] = A->halo_split_ok ? 1 : 0; out[7] = A->max_block_nnz > A->lds_cap ? 1 : 0;
  return MGS_OK;
}
int mgs_csr_get_origin(const mgs_csr *A, int *origin) {
  mgs_ctx *ctx = A->ctx;
  if (!A->origin) return 1;                       // identity (no origin recorded): nothing written
  MGS_HIP(ctx, hipMemcpyAsync(origin, A->origin, sizeof(int) * (size_t)A->rows, hipMemcpyDeviceToHost, ctx->stream));
  MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MGS_OK;
}
int mgs_csr_set_origin(mgs_csr *A, const int *origin) {
  mgs_ctx *ctx = A->ctx;
  if (origin && A->rows > 0) {      // the tie-break key divides by the distance of two origins: distinct and non-negative, checked before anything changes
    std::vector<int> o(origin, origin + A->rows);
    std::sort(o.begin(), o.end());
    MGS_CHECK(ctx, o.front() >= 0, MGS_ERR_INVALID, "mgs_csr_set_origin: negative origin %d", o.front());
    const auto dup = std::adjacent_find(o.begin(), o.end());
    MGS_CHECK(ctx, dup == o.end(), MGS_ERR_INVALID, "mgs_csr_set_origin: origin %d given to more than one row", dup == o.end() ? 0 : *dup);
  }
  if (A->origin) { mgs_hip_free(A->origin); A->origin = nullptr; }
  if (!origin || A->rows == 0) return MGS_OK;
  MGS_TRY(mgs_dev_alloc(ctx, &A->origin, (size_t)A->rows));
  MGS_HIP(ctx, hipMemcpy(A->origin, origin, sizeof(int) * (size_t)A->rows, hipMemcpyHostToDevice));
  return MGS_OK;
}
// New values for an uploaded matrix, same pattern, in place: the device arrays do not move, so hierarchies and captured cycles that
// hold their addresses stay valid.  Every per-matrix cache is pattern-only (blkptr, launch plan, index code, origin) and stays —
// except a value-carrying pattern code (option valcode), which is why that case is refused.
static int update_values_check(mgs_csr *A, const void *src, int64_t nnz, const char *who) {
  MGS_CHECK(nullptr, A, MGS_ERR_INVALID, "%s: NULL matrix", who);
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, nnz == A->nnz, MGS_ERR_INVALID, "%s: %lld values given, the matrix has %lld entries", who, (long long)nnz, (long long)A->nnz);
  MGS_CHECK(ctx, src || nnz == 0, MGS_ERR_INVALID, "%s: NULL values", who);
  MGS_CHECK(ctx, !(A->code && A->code->vtab), MGS_ERR_INVALID, "%s: the matrix carries a value-carrying pattern code (option valcode): upload it again instead", who);
  return MGS_OK;
}
int mgs_csr_update_values(mgs_csr *A, const double *host_val, int64_t nnz) {
  MGS_TRY(update_values_check(A, host_val, nnz, "mgs_csr_update_values"));
  mgs_ctx *ctx = A->ctx;
  if (nnz) MGS_HIP(ctx, hipMemcpyAsync(A->val, host_val, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, ctx->stream));
  MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the caller may reuse host_val right away
  return MGS_OK;
}
int mgs_csr_update_values_dev(mgs_csr *A, const void *device_val, int64_t nnz) {
  MGS_TRY(update_values_check(A, device_val, nnz, "mgs_csr_update_values_dev"));
  mgs_ctx *ctx = A->ctx;
  if (nnz && device_val != (const void *)A->val) MGS_HIP(ctx, hipMemcpyAsync(A->val, device_val, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, ctx->stream));
  return MGS_OK;
}
int mgs_csr_update_values_coo_dev(mgs_csr *A, const void *val_dev, int64_t ntrip) {
  MGS_CHECK(nullptr, A, MGS_ERR_INVALID, "mgs_csr_update_values_coo_dev: NULL matrix");
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, A->coo_map, MGS_ERR_STATE, "mgs_csr_update_values_coo_dev: the matrix keeps no triple map (mgs_csr_from_coo_device with keep_map != 0 does)");
  MGS_CHECK(ctx, ntrip == A->coo_ntrip, MGS_ERR_INVALID, "mgs_csr_update_values_coo_dev: %lld values given, the matrix was assembled from %lld triples", (long long)ntrip,
            (long long)A->coo_ntrip);
  MGS_TRY(update_values_check(A, val_dev, A->nnz, "mgs_csr_update_values_coo_dev"));
  return k_csr_update_values_coo(A, val_dev);
}
int mgs_csr_destroy(mgs_csr *A) {
  if (!A) return MGS_OK;
  if (A->coo_src) mgs_hip_free(A->coo_src);
  if (A->coo_run) mgs_hip_free(A->coo_run);
  if (A->owns) { if (A->rowptr) mgs_hip_free(A->rowptr); if (A->col) mgs_hip_free(A->col); if (A->val) mgs_hip_free(A->val); }
  if (A->blkptr) mgs_hip_free(A->blkptr);
  if (A->origin) mgs_hip_free(A->origin);
  mgs_free_rowcode(A->code);
  mgs_free_spgemm(A->spg);
  mgs_free_add(A->addp);
  mgs_free_extract(A->extp);
  mgs_free_reorder(A->reop);
  mgs_free_nsfields(A->nsf);
  delete A;
  return MGS_OK;
}
int mgs_csr_optimize(mgs_csr *A) {
  if (!A || A->code_tried || !A->ctx->opt_rowcode || A->rows == 0 || A->nnz == 0) return MGS_OK;
  A->code_tried = true;
  return mgs_build_rowcode(A->ctx, A->rows, A->rowptr, A->col, nullptr, 0x7fffffff, &A->code, A->ctx->opt_valcode ? A->val : nullptr);
}
int mgs_csr_rowcode_info(const mgs_csr *A, int64_t out[4]) {
  out[0] = A->code ? A->code->coded_blocks : 0; out[1] = A->code ? A->code->nblocks : mgs_row_blocks(A);
  out[2] = A->code ? A->code->tab_total : 0; out[3] = A->code ? A->code->tab_cap : 0;
  return MGS_OK;
}
int mgs_csr_poisson3d(mgs_ctx *ctx, int N, int plane_lo, int plane_hi, int local_cols, mgs_csr **out) {
  MGS_TRY(k_poisson3d(ctx, N, plane_lo, plane_hi, local_cols, out));
  (*out)->halo_cols = (*out)->cols > (*out)->rows;      // a plane range of the N³ operator: a row shard
  return MGS_OK;
}
int mgs_csr_poisson2d(mgs_ctx *ctx, int n, mgs_csr **out) { return k_poisson2d(ctx, n, out); }
int mgs_csr_transpose(const mgs_csr *A, mgs_csr **out) { return k_transpose(A, out); }
// declared null space: a word on the matrix that hierarchies (finalize / refresh) and the Krylov solvers read; nothing is verified here
int mgs_csr_set_nullspace(mgs_csr *A, int kind) {
  MGS_CHECK(nullptr, A, MGS_ERR_INVALID, "mgs_csr_set_nullspace: NULL matrix");
  MGS_CHECK(A->ctx, kind == MGS_NULLSPACE_NONE || kind == MGS_NULLSPACE_CONSTANT, MGS_ERR_INVALID, "mgs_csr_set_nullspace: unknown kind %d", kind);
  MGS_CHECK(A->ctx, A->rows == A->cols, MGS_ERR_INVALID, "mgs_csr_set_nullspace: the matrix is %d x %d (%s)", A->rows, A->cols,
            A->cols > A->rows ? "halo columns: a row shard" : "not square");
  if (A->nsf) { hipStreamSynchronize(A->ctx->stream); mgs_free_nsfields(A->nsf); A->nsf = nullptr; }      // an enqueued projection may still read the labels
  A->nullspace = kind;
  return MGS_OK;
}
// field-wise constant null space: labels from device memory, checked and narrowed before anything uses them (ingest.hip); the matrix keeps the
// declaration it had on every refusal
int mgs_csr_set_nullspace_fields(mgs_csr *A, const void *labels_dev, int index_bits, int nfields) {
  MGS_CHECK(nullptr, A, MGS_ERR_INVALID, "mgs_csr_set_nullspace_fields: NULL matrix");
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, labels_dev, MGS_ERR_INVALID, "mgs_csr_set_nullspace_fields: NULL labels");
  MGS_CHECK(ctx, index_bits == 32 || index_bits == 64, MGS_ERR_INVALID, "mgs_csr_set_nullspace_fields: index_bits = %d, expected 32 or 64", index_bits);
  MGS_CHECK(ctx, nfields >= 1 && nfields <= MGS_NULLSPACE_MAX_FIELDS, MGS_ERR_INVALID, "mgs_csr_set_nullspace_fields: nfields = %d outside 1..%d", nfields, MGS_NULLSPACE_MAX_FIELDS);
  MGS_CHECK(ctx, A->rows == A->cols && !mgs_csr_is_shard(A), MGS_ERR_INVALID, "mgs_csr_set_nullspace_fields: the matrix is %d x %d (%s)", A->rows, A->cols,
            A->cols > A->rows ? "halo columns: a row shard" : "not square");
  MGS_CHECK(ctx, !ctx->ncomm && !ctx->allreduce, MGS_ERR_INVALID, "mgs_csr_set_nullspace_fields: the context sums over ranks (a row shard)");
  signed char *lab = nullptr; int64_t counts[MGS_NULLSPACE_MAX_FIELDS] = {0}, bad_row = -1; long long bad_val = 0;
  MGS_TRY(k_labels_from_device(ctx, A->rows, labels_dev, index_bits, nfields, &lab, counts, &bad_row, &bad_val));
  MGS_CHECK(ctx, bad_row < 0, MGS_ERR_INVALID, "mgs_csr_set_nullspace_fields: row %lld carries label %lld outside [-1, %d)", (long long)bad_row, bad_val, nfields);
  for (int f = 0; f < nfields; ++f)
    if (counts[f] == 0) { mgs_hip_free(lab); return mgs_fail(ctx, MGS_ERR_INVALID, "mgs_csr_set_nullspace_fields: field %d has no rows", f); }
  mgs_nsfields *F = new mgs_nsfields();
  F->nfields = nfields; F->labels = lab;
  for (int f = 0; f < nfields; ++f) F->counts[f] = counts[f];
  int rc = mgs_dev_alloc(ctx, &F->means, (size_t)MGS_NULLSPACE_MAX_FIELDS);
  if (rc == MGS_OK && hipMemsetAsync(F->means, 0, sizeof(double) * MGS_NULLSPACE_MAX_FIELDS, ctx->stream) != hipSuccess) rc = mgs_fail(ctx, MGS_ERR_HIP, "mgs_csr_set_nullspace_fields: hipMemsetAsync failed");
  if (rc != MGS_OK) { mgs_free_nsfields(F); return rc; }
  if (A->nsf) { hipStreamSynchronize(ctx->stream); mgs_free_nsfields(A->nsf); }
  A->nsf = F; A->nullspace = MGS_NULLSPACE_FIELDS;
  return MGS_OK;
}
int mgs_csr_nullspace_fields(const mgs_csr *A, int *nfields, int64_t counts[MGS_NULLSPACE_MAX_FIELDS]) {
  MGS_CHECK(nullptr, A && nfields && counts, MGS_ERR_INVALID, "mgs_csr_nullspace_fields: NULL argument");
  const bool f = A->nullspace == MGS_NULLSPACE_FIELDS && A->nsf;
  *nfields = f ? A->nsf->nfields : 0;
  for (int k = 0; k < MGS_NULLSPACE_MAX_FIELDS; ++k) counts[k] = f ? A->nsf->counts[k] : 0;
  return MGS_OK;
}
int mgs_csr_nullspace(const mgs_csr *A, int *kind) {
  MGS_CHECK(nullptr, A && kind, MGS_ERR_INVALID, "mgs_csr_nullspace: NULL argument");
  *kind = A->nullspace;
  return MGS_OK;
}
// out[0] = ‖A·1‖∞ / ‖|A|·1‖∞, out[1] the same for Aᵀ.  |Aᵀ| is the transpose's private copy with its values made absolute in place, |A| its
// transpose; the four maxima are folded on the device (bits of non-negative doubles) and read once.
int mgs_csr_nullspace_defect(const mgs_csr *A, double out[2]) {
  MGS_CHECK(nullptr, A && out, MGS_ERR_INVALID, "mgs_csr_nullspace_defect: NULL argument");
  mgs_ctx *ctx = A->ctx;
  out[0] = out[1] = 0.0;
  if (A->rows == 0 || A->cols == 0 || A->nnz == 0) return MGS_OK;
  const int64_t nmax = A->rows > A->cols ? A->rows : A->cols;
  mgs_vec *ones = nullptr, *y = nullptr; mgs_csr *At = nullptr, *Aa = nullptr; unsigned long long *mx = nullptr;
  unsigned long long hm[4] = {0, 0, 0, 0};
  if (A->nullspace == MGS_NULLSPACE_FIELDS && A->nsf) {      // the maximum over the fields of the same two quotients with z_f in the place of 1: one SpMV per field and matrix
    std::vector<unsigned long long> hf(4 * (size_t)A->nsf->nfields, 0ull);
    auto runf = [&]() -> int {
      MGS_TRY(mgs_vec_create(ctx, nmax, &ones)); MGS_TRY(mgs_vec_create(ctx, nmax, &y));
      MGS_TRY(mgs_dev_alloc(ctx, &mx, hf.size()));
      MGS_HIP(ctx, hipMemsetAsync(mx, 0, sizeof(unsigned long long) * hf.size(), ctx->stream));
      MGS_TRY(mgs_csr_transpose(A, &At));
      for (int f = 0; f < A->nsf->nfields; ++f) {
        MGS_TRY(k_label_indicator(ctx, A->rows, A->nsf->labels, f, ones->d));
        MGS_TRY(mgs_spmv(A, ones, y));  MGS_TRY(k_absmax_dev(ctx, A->rows, y->d, mx + 4 * f + 0));
        MGS_TRY(mgs_spmv(At, ones, y)); MGS_TRY(k_absmax_dev(ctx, At->rows, y->d, mx + 4 * f + 2));
      }
      MGS_TRY(k_abs_inplace(ctx, At->nnz, At->val));
      MGS_TRY(mgs_csr_transpose(At, &Aa));
      for (int f = 0; f < A->nsf->nfields; ++f) {
        MGS_TRY(k_label_indicator(ctx, A->rows, A->nsf->labels, f, ones->d));
        MGS_TRY(mgs_spmv(At, ones, y)); MGS_TRY(k_absmax_dev(ctx, At->rows, y->d, mx + 4 * f + 3));
        MGS_TRY(mgs_spmv(Aa, ones, y)); MGS_TRY(k_absmax_dev(ctx, Aa->rows, y->d, mx + 4 * f + 1));
      }
      MGS_HIP(ctx, hipMemcpyAsync(hf.data(), mx, sizeof(unsigned long long) * hf.size(), hipMemcpyDeviceToHost, ctx->stream));
      MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
      return MGS_OK;
    };
    const int rcf = runf();
    if (rcf != MGS_OK) hipStreamSynchronize(ctx->stream);
    mgs_vec_destroy(ones); mgs_vec_destroy(y); mgs_csr_destroy(At); mgs_csr_destroy(Aa);
    if (mx) mgs_hip_free(mx);
    if (rcf != MGS_OK) return rcf;
    for (int f = 0; f < A->nsf->nfields; ++f) {
      double v[4];
      for (int q = 0; q < 4; ++q) memcpy(&v[q], &hf[4 * (size_t)f + q], sizeof(double));
      const double d0 = v[1] != 0.0 ? v[0] / v[1] : 0.0, d1 = v[3] != 0.0 ? v[2] / v[3] : 0.0;
      if (!(d0 <= out[0])) out[0] = d0;      // (a NaN wins)
      if (!(d1 <= out[1])) out[1] = d1;
    }
    return MGS_OK;
  }
  auto run = [&]() -> int {
    MGS_TRY(mgs_vec_create(ctx, nmax, &ones)); MGS_TRY(mgs_vec_create(ctx, nmax, &y));
    MGS_TRY(mgs_dev_alloc(ctx, &mx, 4));
    MGS_HIP(ctx, hipMemsetAsync(mx, 0, sizeof hm, ctx->stream));
    MGS_TRY(mgs_vec_fill(ones, 1.0));
    MGS_TRY(mgs_csr_transpose(A, &At));
    MGS_TRY(mgs_spmv(A, ones, y));  MGS_TRY(k_absmax_dev(ctx, A->rows, y->d, mx + 0));      // ‖A·1‖∞
    MGS_TRY(mgs_spmv(At, ones, y)); MGS_TRY(k_absmax_dev(ctx, At->rows, y->d, mx + 2));     // ‖Aᵀ·1‖∞
    MGS_TRY(k_abs_inplace(ctx, At->nnz, At->val));
    MGS_TRY(mgs_spmv(At, ones, y)); MGS_TRY(k_absmax_dev(ctx, At->rows, y->d, mx + 3));     // ‖|Aᵀ|·1‖∞
    MGS_TRY(mgs_csr_transpose(At, &Aa));
    MGS_TRY(mgs_spmv(Aa, ones, y)); MGS_TRY(k_absmax_dev(ctx, Aa->rows, y->d, mx + 1));     // ‖|A|·1‖∞
    MGS_HIP(ctx, hipMemcpyAsync(hm, mx, sizeof hm, hipMemcpyDeviceToHost, ctx->stream));
    MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MGS_OK;
  };
  const int rc = run();
  if (rc != MGS_OK) hipStreamSynchronize(ctx->stream);
  mgs_vec_destroy(ones); mgs_vec_destroy(y); mgs_csr_destroy(At); mgs_csr_destroy(Aa);
  if (mx) mgs_hip_free(mx);
  if (rc != MGS_OK) return rc;
  double v[4];
  for (int q = 0; q < 4; ++q) memcpy(&v[q], &hm[q], sizeof(double));
  out[0] = v[1] != 0.0 ? v[0] / v[1] : 0.0;
  out[1] = v[3] != 0.0 ? v[2] / v[3] : 0.0;
  return MGS_OK;
}
int mgs_csr_galerkin(const mgs_csr *A, const mgs_xfer *T, mgs_csr **out) {
  MGS_CHECK(A->ctx, T->n_fine == A->rows && A->rows == A->cols, MGS_ERR_INVALID, "galerkin: A is %d x %d, P has %d rows", A->rows, A->cols, T->n_fine);
  return T->aggregation ? k_galerkin_agg(A, T, out) : k_galerkin_general(A, T, out);
}
// sparse products on the device (spgemm.hip)
int mgs_csr_spgemm(const mgs_csr *A, const mgs_csr *B, mgs_csr **C) { return k_spgemm(A, B, C); }
int mgs_csr_spgemm_numeric(const mgs_csr *A, const mgs_csr *B, mgs_csr *C, int64_t *misses) { return k_spgemm_numeric(A, B, C, misses); }
int mgs_csr_spgemm_info(const mgs_csr *C, int64_t out[4]) { return k_spgemm_info(C, out); }
// sums and scalings on the device (csr_algebra.hip)
int mgs_csr_add(double alpha, const mgs_csr *A, double beta, const mgs_csr *B, mgs_csr **C) { return k_csr_add(alpha, A, beta, B, C); }
int mgs_csr_add_numeric(double alpha, const mgs_csr *A, double beta, const mgs_csr *B, mgs_csr *C, int64_t *misses) {
  return k_csr_add_numeric(alpha, A, beta, B, C, misses);
}
int mgs_csr_add_info(const mgs_csr *C, int64_t out[4]) { return k_csr_add_info(C, out); }
int mgs_csr_scale(mgs_csr *A, const mgs_vec *dl, const mgs_vec *dr) { return k_csr_scale(A, dl, dr); }
int mgs_csr_diag(const mgs_csr *A, mgs_vec *d) { return k_csr_diag(A, d); }
int mgs_csr_from_diag(mgs_ctx *ctx, const mgs_vec *d, mgs_csr **out) { return k_csr_from_diag(ctx, d, out); }
// blocks of a device matrix, gather / scatter of a vector by an index list (extract.hip)
int mgs_csr_extract(const mgs_csr *A, const void *rows_dev, int64_t nr, const void *cols_dev, int64_t nc, int index_bits, int keep_map, mgs_csr **S) {
  return k_csr_extract(A, rows_dev, nr, cols_dev, nc, index_bits, keep_map, S);
}
int mgs_csr_extract_numeric(const mgs_csr *A, mgs_csr *S) { return k_csr_extract_numeric(A, S); }
int mgs_csr_extract_info(const mgs_csr *S, int64_t out[4]) { return k_csr_extract_info(S, out); }
// permutations of a device matrix and assembly from a grid of blocks (reorder.hip)
int mgs_csr_permute(const mgs_csr *A, const void *rperm_dev, const void *cperm_dev, int index_bits, int keep_map, mgs_csr **C) {
  return k_csr_permute(A, rperm_dev, cperm_dev, index_bits, keep_map, C);
}
int mgs_csr_permute_numeric(const mgs_csr *A, mgs_csr *C) { return k_csr_permute_numeric(A, C); }
int mgs_csr_permute_info(const mgs_csr *C, int64_t out[4]) { return k_csr_permute_info(C, out); }
int mgs_csr_bmat(mgs_ctx *ctx, int br, int bc, const mgs_csr *const *blocks, const int *row_sizes, const int *col_sizes, mgs_csr **C) {
  return k_csr_bmat(ctx, br, bc, blocks, row_sizes, col_sizes, C);
}
int mgs_csr_bmat_numeric(mgs_csr *C, const mgs_csr *const *blocks) { return k_csr_bmat_numeric(C, blocks); }
int mgs_csr_transpose_numeric(const mgs_csr *A, mgs_csr *At, int64_t *misses) { return k_csr_transpose_numeric(A, At, misses); }
int mgs_csr_bmat_info(const mgs_csr *C, int64_t out[4]) { return k_csr_bmat_info(C, out); }
int mgs_vec_gather(const mgs_vec *x, const void *idx_dev, int64_t n, int index_bits, mgs_vec *y, int64_t *bad) { return k_vec_gather(x, idx_dev, n, index_bits, y, bad); }
int mgs_vec_scatter(const mgs_vec *y, const void *idx_dev, int64_t n, int index_bits, mgs_vec *x, int64_t *bad) { return k_vec_scatter(y, idx_dev, n, index_bits, x, bad); }

// ------------------------------------------------------------------ vectors
int mgs_vec_create(mgs_ctx *ctx, int64_t n, mgs_vec **out) {
  MGS_CHECK(ctx, n >= 0, MGS_ERR_INVALID, "mgs_vec_create: n < 0");
  mgs_vec *v = new mgs_vec(); v->ctx = ctx; v->n = n; v->owns = true;
  int rc = mgs_dev_alloc(ctx, &v->d, (size_t)n);
  if (rc != MGS_OK) { delete v; return rc; }
  hipMemsetAsync(v->d, 0, sizeof(double) * (size_t)(n ? n : 1), ctx->stream);
  *out = v;
  return MGS_OK;
}
int mgs_vec_wrap(mgs_ctx *ctx, void *p, int64_t n, mgs_vec **out) {
  MGS_CHECK(ctx, p || n == 0, MGS_ERR_INVALID, "mgs_vec_wrap: NULL pointer");
  mgs_vec *v = new mgs_vec(); v->ctx = ctx; v->n = n; v->owns = false; v->d = (double *)p;
  *out = v;
  return MGS_OK;
}
int mgs_vec_destroy(mgs_vec *v) { if (!v) return MGS_OK; if (v->owns && v->d) mgs_hip_free(v->d); delete v; return MGS_OK; }
int mgs_vec_upload(mgs_vec *v, const double *host, int64_t n) {
  MGS_CHECK(v->ctx, n <= v->n, MGS_ERR_INVALID, "mgs_vec_upload: %lld > size %lld", (long long)n, (long long)v->n);
  MGS_HIP(v->ctx, hipMemcpyAsync(v->d, host, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, v->ctx->stream));
  MGS_HIP(v->ctx, hipStreamSynchronize(v->ctx->stream));
  return MGS_OK;
}
int mgs_vec_download(const mgs_vec *v, double *host, int64_t n) {
  MGS_CHECK(v->ctx, n <= v->n, MGS_ERR_INVALID, "mgs_vec_download: %lld > size %lld", (long long)n, (long long)v->n);
  MGS_HIP(v->ctx, hipMemcpyAsync(host, v->d, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, v->ctx->stream));
  MGS_HIP(v->ctx, hipStreamSynchronize(v->ctx->stream));
  return MGS_OK;
}
int mgs_vec_fill(mgs_vec *v, double value) { return k_fill(v->ctx, v->d, v->n, value); }
int mgs_vec_copy(const mgs_vec *src, mgs_vec *dst) {
  MGS_CHECK(src->ctx, src->n <= dst->n, MGS_ERR_INVALID, "mgs_vec_copy: size mismatch");
  MGS_HIP(src->ctx, hipMemcpyAsync(dst->d, src->d, sizeof(double) * (size_t)src->n, hipMemcpyDeviceToDevice, src->ctx->stream));
  return MGS_OK;
}
int64_t mgs_vec_size(const mgs_vec *v) { return v->n; }
void *mgs_vec_ptr(const mgs_vec *v) { return v->d; }
int mgs_vec_rand(mgs_vec *v, uint64_t seed, int64_t off) { return k_rand(v->ctx, v->d, v->n, seed, off); }

// ------------------------------------------------------------------ primitives
int mgs_spmv(const mgs_csr *A, const mgs_vec *x, mgs_vec *y) {
  MGS_CHECK(A->ctx, x->n >= A->cols && y->n >= A->rows, MGS_ERR_INVALID, "mgs_spmv: A %d x %d, x %lld, y %lld", A->rows, A->cols, (long long)x->n, (long long)y->n);
  MGS_CHECK(A->ctx, x->d != y->d, MGS_ERR_INVALID, "mgs_spmv: y must not alias x");
  return mgs_launch_csr_op(A, MGS_OP_SPMV, x->d, nullptr, nullptr, 0.0, y->d);
}
int mgs_residual(const mgs_csr *A, const mgs_vec *x, const mgs_vec *b, mgs_vec *r) {
  MGS_CHECK(A->ctx, x->n >= A->cols && b->n >= A->rows && r->n >= A->rows, MGS_ERR_INVALID, "mgs_residual: shape mismatch");
  MGS_CHECK(A->ctx, x->d != r->d, MGS_ERR_INVALID, "mgs_residual: r must not alias x");
  return mgs_launch_csr_op(A, MGS_OP_RESIDUAL, x->d, b->d, nullptr, 0.0, r->d);
}
int mgs_diag_inv(const mgs_csr *A, mgs_vec *dinv) {
  MGS_CHECK(A->ctx, dinv->n >= A->rows, MGS_ERR_INVALID, "mgs_diag_inv: dinv too small");
  int bad = 0;
  MGS_TRY(k_diag_inv(A, dinv->d, &bad));
  MGS_CHECK(A->ctx, bad == 0, MGS_ERR_NUMERIC, "mgs_diag_inv: %d rows have a missing or zero diagonal", bad);
  return MGS_OK;
}
int mgs_jacobi(const mgs_csr *A, const mgs_vec *dinv, double omega, const mgs_vec *b, const mgs_vec *x_in, mgs_vec *x_out) {
  MGS_CHECK(A->ctx, A->rows <= A->cols && x_in->n >= A->cols && b->n >= A->rows && x_out->n >= A->rows && dinv->n >= A->rows, MGS_ERR_INVALID, "mgs_jacobi: shape mismatch");
  MGS_CHECK(A->ctx, x_in->d != x_out->d, MGS_ERR_INVALID, "mgs_jacobi: out of place only (x_out must not alias x_in)");
  return mgs_launch_csr_op(A, MGS_OP_JACOBI, x_in->d, b->d, dinv->d, omega, x_out->d);
}

int mgs_xfer_create(const mgs_csr *P, mgs_xfer **out) { return k_xfer_from_csr(P, out); }
int mgs_xfer_destroy(mgs_xfer *T) {
  if (!T) return MGS_OK;
  if (T->agg) mgs_hip_free(T->agg); if (T->cptr) mgs_hip_free(T->cptr); if (T->members) mgs_hip_free(T->members); if (T->corigin) mgs_hip_free(T->corigin); if (T->halo_cmap) mgs_hip_free(T->halo_cmap);
  if (T->P) mgs_csr_destroy(T->P); if (T->Pt) mgs_csr_destroy(T->Pt);
  delete T;
  return MGS_OK;
}
int mgs_xfer_shape(const mgs_xfer *T, int *n_fine, int *n_coarse, int *is_agg) {
  if (n_fine) *n_fine = T->n_fine; if (n_coarse) *n_coarse = T->n_coarse; if (is_agg) *is_agg = T->aggregation ? 1 : 0;
  return MGS_OK;
}
int mgs_xfer_download_agg(const mgs_xfer *T, int *agg) {
  MGS_CHECK(T->ctx, T->aggregation, MGS_ERR_STATE, "transfer is not in aggregation form");
  MGS_HIP(T->ctx, hipMemcpyAsync(agg, T->agg, sizeof(int) * (size_t)T->n_fine, hipMemcpyDeviceToHost, T->ctx->stream));
  MGS_HIP(T->ctx, hipStreamSynchronize(T->ctx->stream));
  return MGS_OK;
}
int mgs_restrict(const mgs_xfer *T, const mgs_vec *r, mgs_vec *rc) {
  MGS_CHECK(T->ctx, r->n >= T->n_fine && rc->n >= T->n_coarse, MGS_ERR_INVALID, "mgs_restrict: shape mismatch");
  if (T->aggregation) return k_restrict_agg(T->ctx, T->n_coarse, T->cptr, T->members, r->d, rc->d);
  return mgs_launch_csr_op(T->Pt, MGS_OP_SPMV, r->d, nullptr, nullptr, 0.0, rc->d);
}
int mgs_prolong(const mgs_xfer *T, const mgs_vec *ec, mgs_vec *e) {
  MGS_CHECK(T->ctx, e->n >= T->n_fine && ec->n >= T->n_coarse, MGS_ERR_INVALID, "mgs_prolong: shape mismatch");
  if (T->aggregation) return k_prolong_agg(T->ctx, T->n_fine, T->agg, ec->d, e->d, 0);
  return mgs_launch_csr_op(T->P, MGS_OP_SPMV, ec->d, nullptr, nullptr, 0.0, e->d);
}

int mgs_dot(const mgs_vec *x, const mgs_vec *y, double *out) {
  MGS_CHECK(x->ctx, x->n == y->n, MGS_ERR_INVALID, "mgs_dot: size mismatch");
  return k_dot(x->ctx, x->n, x->d, y->d, out);
}
int mgs_nrm2(const mgs_vec *x, double *out) { double s = 0; MGS_TRY(k_dot(x->ctx, x->n, x->d, x->d, &s)); *out = std::sqrt(s); return MGS_OK; }
int mgs_axpby(double a, const mgs_vec *x, double b, mgs_vec *y) {
  MGS_CHECK(x->ctx, x->n == y->n, MGS_ERR_INVALID, "mgs_axpby: size mismatch");
  return k_axpby(x->ctx, x->n, a, x->d, b, y->d);
}
int mgs_axpbypcz(double a, const mgs_vec *x, double b, const mgs_vec *y, double c, mgs_vec *z) {
  MGS_CHECK(x->ctx, x->n == y->n && x->n == z->n, MGS_ERR_INVALID, "mgs_axpbypcz: size mismatch");
  return k_axpbypcz(x->ctx, x->n, a, x->d, b, y->d, c, z->d);
}
int mgs_vec_project_const(mgs_vec *v, double *mean, double *nrm2) {
  MGS_CHECK(nullptr, v, MGS_ERR_INVALID, "mgs_vec_project_const: NULL vector");
  double d2[2] = {0.0, 0.0};
  if (nrm2) { MGS_TRY(k_project_const_nrm2(v->ctx, v->n, v->d, d2)); *nrm2 = std::sqrt(d2[0]); }
  else MGS_TRY(k_project_const(v->ctx, v->n, v->d));
  if (mean) { *mean = 0.0; if (v->n > 0) MGS_TRY(k_project_const_mean(v->ctx, mean)); }
  return MGS_OK;
}
int mgs_vec_project_fields(mgs_vec *v, const mgs_csr *A, double *means, double *nrm2) {
  MGS_CHECK(nullptr, v && A, MGS_ERR_INVALID, "mgs_vec_project_fields: NULL argument");
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, A->nullspace == MGS_NULLSPACE_FIELDS && A->nsf, MGS_ERR_INVALID, "mgs_vec_project_fields: the matrix carries null-space kind %d, not MGS_NULLSPACE_FIELDS", A->nullspace);
  MGS_CHECK(ctx, v->ctx == ctx && v->n >= A->rows, MGS_ERR_INVALID, "mgs_vec_project_fields: a vector of %lld entries (or of another context), the matrix has %d rows", (long long)v->n, A->rows);
  double d2[2] = {0.0, 0.0};
  MGS_TRY(k_project_fields(ctx, A->nsf, A->rows, v->d, true, nrm2 != nullptr, nrm2 ? d2 : nullptr));
  if (nrm2) *nrm2 = std::sqrt(d2[0]);
  if (means) {
    MGS_HIP(ctx, hipMemcpyAsync(means, A->nsf->means, sizeof(double) * (size_t)A->nsf->nfields, hipMemcpyDeviceToHost, ctx->stream));
    MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return MGS_OK;
}
int mgs_halo_pack(mgs_ctx *ctx, const mgs_vec *x, const int *send_idx_dev, int64_t n_send, double *send_buf_dev) {
  return k_gather(ctx, x->d, send_idx_dev, n_send, send_buf_dev);
}

}  // extern "C"

// prolong_add for the general form needs a temporary: e = P ec; x += e
static int prolong_add_impl(const mgs_xfer *T, const double *ec, double *x, double *tmp) {
  if (T->aggregation) return k_prolong_agg(T->ctx, T->n_fine, T->agg, ec, x, 1);
  MGS_TRY(mgs_launch_csr_op(T->P, MGS_OP_SPMV, ec, nullptr, nullptr, 0.0, tmp));
  return k_axpby(T->ctx, T->n_fine, 1.0, tmp, 1.0, x);
}

extern "C" int mgs_prolong_add(const mgs_xfer *T, const mgs_vec *ec, mgs_vec *x) {
  MGS_CHECK(T->ctx, x->n >= T->n_fine && ec->n >= T->n_coarse, MGS_ERR_INVALID, "mgs_prolong_add: shape mismatch");
  if (T->aggregation) return k_prolong_agg(T->ctx, T->n_fine, T->agg, ec->d, x->d, 1);
  mgs_vec *tmp = nullptr;
  MGS_TRY(mgs_vec_create(T->ctx, T->n_fine, &tmp));
  int rc = prolong_add_impl(T, ec->d, x->d, tmp->d);
  hipStreamSynchronize(T->ctx->stream);
  mgs_vec_destroy(tmp);
  return rc;
}

// ------------------------------------------------------------------ hierarchy
// bad_out != NULL (the finest level, mgs_hier_create): rows with a missing or zero diagonal are counted there instead of refused — a
// level that is never smoothed (one-level hierarchy: the dense solve alone, which pivots) does not need D⁻¹; see diag0_needed
static int level_init(mgs_hier *h, mgs_level &L, const mgs_csr *A, bool own, int *bad_out = nullptr) {
  mgs_ctx *ctx = h->ctx;
  L.A = A; L.own_A = own; L.n = A->rows; L.n_ext = A->cols > A->rows ? A->cols : A->rows;
  MGS_TRY(mgs_vec_create(ctx, L.n_ext, &L.dinv));      // row shards: the halo part receives the owners' values once (mgs_prepare_fused)
  MGS_TRY(mgs_vec_create(ctx, L.n_ext, &L.r));
  MGS_TRY(mgs_vec_create(ctx, L.n_ext, &L.tmp));
  MGS_TRY(mgs_vec_create(ctx, L.n_ext, &L.b)); MGS_TRY(mgs_vec_create(ctx, L.n_ext, &L.x));
  if (bad_out) return k_diag_inv(A, L.dinv->d, bad_out);
  return mgs_diag_inv(A, L.dinv);
}
// the finest level is about to be smoothed (a level below it, or the smoothed coarsest form): its diagonal must be complete
static int diag0_needed(mgs_hier *h, const char *who) {
  MGS_CHECK(h->ctx, h->bad_diag0 == 0, MGS_ERR_NUMERIC, "%s: %d rows of the fine operator have a missing or zero diagonal", who, h->bad_diag0);
  return MGS_OK;
}
static void level_free(mgs_level &L) {
  if (L.own_A && L.A) mgs_csr_destroy(const_cast<mgs_csr *>(L.A));
  if (L.T) mgs_xfer_destroy(L.T);
  mgs_vec_destroy(L.dinv); mgs_vec_destroy(L.r); mgs_vec_destroy(L.tmp); mgs_vec_destroy(L.b); mgs_vec_destroy(L.x);
  mgs_operands_free(L);
  if (L.nx) { if (L.nx->send_idx) mgs_hip_free(L.nx->send_idx); if (L.nx->sendbuf) mgs_hip_free(L.nx->sendbuf); delete L.nx; L.nx = nullptr; }
  mgs_vec_destroy(L.kc1); mgs_vec_destroy(L.kv1); mgs_vec_destroy(L.kc2); mgs_vec_destroy(L.kv2); mgs_vec_destroy(L.kr);
  if (L.kscal) mgs_hip_free(L.kscal);
  if (L.ns_lab) mgs_hip_free(L.ns_lab);
  L = mgs_level();
}
void mgs_drop_graph(mgs_hier *h) {
  for (auto &g : h->graphs) { if (g.exec) hipGraphExecDestroy(g.exec); g = mgs_hier::GraphSlot(); }
  if (h->coarse_exec) { hipGraphExecDestroy(h->coarse_exec); h->coarse_exec = nullptr; }
}
bool mgs_hier_sharded(const mgs_hier *h) {      // row-sharded in any form: such hierarchies are rebuilt, not refreshed, and keep FP64 operands
  bool shard = h->halo || h->halo_begin || h->halo_fused || h->native || h->ntail || h->coarse;
  for (auto &L : h->lev) shard = shard || L.A->cols > L.A->rows || L.nx;
  return shard;
}
int mgs_level_in_range(const mgs_hier *h, int level, const char *who) {
  MGS_CHECK(h->ctx, level >= 0 && level < (int)h->lev.size(), MGS_ERR_INVALID, "%s: level %d out of range", who, level); return MGS_OK;
}
extern "C" {

int mgs_hier_create(mgs_ctx *ctx, const mgs_csr *A, double omega, int nu1, int nu2, mgs_hier **out) {
  MGS_CHECK(ctx, A && out, MGS_ERR_INVALID, "mgs_hier_create: NULL argument");
  MGS_CHECK(ctx, A->rows <= A->cols && A->rows > 0, MGS_ERR_INVALID, "mgs_hier_create: operator must have rows <= cols (square, or a row shard with halo columns); got %d x %d", A->rows, A->cols);
  MGS_CHECK(ctx, nu1 >= 0 && nu2 >= 0, MGS_ERR_INVALID, "mgs_hier_create: negative sweep count");
  mgs_hier *h = new mgs_hier();
  h->ctx = ctx; h->omega = omega; h->nu1 = nu1; h->nu2 = nu2;
  h->lev.emplace_back();
  int rc = level_init(h, h->lev.back(), A, false, &h->bad_diag0);
  if (rc != MGS_OK) { mgs_hier_destroy(h); return rc; }
  *out = h;
  return MGS_OK;
}
static void free_native_tail(mgs_hier *h) {
  mgs_native_tail *T = h->ntail;
  if (!T) return;
  if (T->send) mgs_hip_free(T->send); if (T->all) mgs_hip_free(T->all); if (T->gidx) mgs_hip_free(T->gidx); if (T->halo_global) mgs_hip_free(T->halo_global);
  mgs_vec_destroy(T->b); mgs_vec_destroy(T->x);
  delete T; h->ntail = nullptr;
}
int mgs_hier_destroy(mgs_hier *h) {
  if (!h) return MGS_OK;
  hipStreamSynchronize(h->ctx->stream);
  mgs_drop_graph(h);
  for (hipEvent_t e : h->fork_events) hipEventDestroy(e);
  for (auto &L : h->lev) level_free(L);
  if (h->inv) mgs_hip_free(h->inv);
  if (h->refresh_flags) mgs_hip_free(h->refresh_flags);
  if (h->nd_flag) mgs_hip_free(h->nd_flag);
  free_native_tail(h);
  delete h;
  return MGS_OK;
}
int mgs_hier_set_smoother(mgs_hier *h, double omega, int nu1, int nu2) {
  MGS_CHECK(h->ctx, nu1 >= 0 && nu2 >= 0, MGS_ERR_INVALID, "negative sweep count");
  if (omega != h->omega) for (auto &L : h->lev) mgs_operands_mark(L, OPD_WD);      // a new ω: the Â branch of every level
  h->omega = omega; h->nu1 = nu1; h->nu2 = nu2; mgs_drop_graph(h);
  return MGS_OK;
}
// ---- native RCCL transport of a sharded hierarchy (comm_rccl.hip) ----
int mgs_hier_set_native_exchange(mgs_hier *h, int level, mgs_comm *c, const int *send_idx, const int *send_counts, const int *recv_counts) {
  mgs_ctx *ctx = h->ctx;
  MGS_TRY(mgs_level_in_range(h, level, "mgs_hier_set_native_exchange"));
  mgs_level &L = h->lev[level];
  auto free_plan = [](mgs_native_plan *P) { if (!P) return; if (P->send_idx) mgs_hip_free(P->send_idx); if (P->sendbuf) mgs_hip_free(P->sendbuf); delete P; };
  free_plan(L.nx); L.nx = nullptr;
  mgs_drop_graph(h);
  h->native = false; for (auto &q : h->lev) h->native = h->native || q.nx;
  if (!c) return MGS_OK;
  // build and validate the plan aside; it is installed only when complete (a caller that handles the error keeps its callbacks)
  int world = 0; mgs_comm_size(c, &world, nullptr);
  mgs_native_plan *P = new mgs_native_plan();
  P->comm = c; P->scnt.assign(send_counts, send_counts + world); P->rcnt.assign(recv_counts, recv_counts + world);
  for (int p = 0; p < world; ++p) { P->ns += P->scnt[p]; P->nr += P->rcnt[p]; }
  int rc = MGS_OK;
  if (P->nr != (int64_t)L.A->cols - L.A->rows)
    rc = mgs_fail(ctx, MGS_ERR_INVALID, "mgs_hier_set_native_exchange: level %d has %d halo columns, plan delivers %lld", level, L.A->cols - L.A->rows, (long long)P->nr);
  if (rc == MGS_OK && P->ns && !send_idx) rc = mgs_fail(ctx, MGS_ERR_INVALID, "mgs_hier_set_native_exchange: send_idx is NULL");
  if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &P->send_idx, (size_t)P->ns);
  if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &P->sendbuf, (size_t)P->ns);
  if (rc == MGS_OK && P->ns && hipMemcpy(P->send_idx, send_idx, sizeof(int) * (size_t)P->ns, hipMemcpyHostToDevice) != hipSuccess)
    rc = mgs_fail(ctx, MGS_ERR_HIP, "mgs_hier_set_native_exchange: upload of the send list failed");
  if (rc != MGS_OK) { free_plan(P); return rc; }
  // contiguous ranges of every peer's send list (pack-free form, see mgs_native_plan)
  P->sseg_start.assign((size_t)world, {}); P->sseg_len.assign((size_t)world, {}); P->rseg_len.assign((size_t)world, {});
  P->seg_ok = true;
  size_t o = 0;
  for (int p = 0; p < world; ++p) {
    for (int k = 0; k < P->scnt[p]; ++k) {
      const int r = send_idx[o + (size_t)k];
      if (k && r == send_idx[o + (size_t)k - 1] + 1) ++P->sseg_len[p].back();
      else { P->sseg_start[p].push_back(r); P->sseg_len[p].push_back(1); }
    }
    if ((int)P->sseg_len[p].size() > MGS_MAX_SEG) P->seg_ok = false;
    o += (size_t)P->scnt[p];
  }
  // packed mode: one message per peer.  (Rehearsal of a middle rank on one GPU, option emu_split_self: the buffer the rank sends to
  // ITSELF stands for the messages to two neighbours — it goes out as two, so packed and pack-free exchanges are timed on equal terms.)
  P->pseg_len.assign((size_t)world, {}); P->prseg_len.assign((size_t)world, {});
  for (int p = 0; p < world; ++p) {
    const bool split = ctx->opt_emu_split_self && world == 1 && P->scnt[p] == P->rcnt[p] && P->scnt[p] >= 2;
    if (P->scnt[p]) { if (split) { P->pseg_len[p] = {P->scnt[p] / 2, P->scnt[p] - P->scnt[p] / 2}; } else P->pseg_len[p] = {P->scnt[p]}; }
    if (P->rcnt[p]) { if (split) { P->prseg_len[p] = {P->rcnt[p] / 2, P->rcnt[p] - P->rcnt[p] / 2}; } else P->prseg_len[p] = {P->rcnt[p]}; }
  }
  L.nx = P;
  h->native = true;
  return MGS_OK;
}
// What this rank will send to each peer once ranges are switched on: nseg[p] ranges whose lengths follow in seglens (peer after
// peer; a rank whose lists do not split into few ranges reports one range per peer = its packed buffer).  Returns the number of
// lengths written, or a negative error; cap = room in seglens.
int mgs_hier_native_send_segments(const mgs_hier *h, int level, int *nseg, int *seglens, int cap) {
  MGS_CHECK(h->ctx, level >= 0 && level < (int)h->lev.size() && h->lev[level].nx && nseg && seglens, MGS_ERR_STATE, "mgs_hier_native_send_segments: level %d has no native plan", level);
  const mgs_native_plan *P = h->lev[level].nx;
  int w = 0;
  for (size_t p = 0; p < P->scnt.size(); ++p) {
    if (P->seg_ok) {
      nseg[p] = (int)P->sseg_len[p].size();
      for (int len : P->sseg_len[p]) { MGS_CHECK(h->ctx, w < cap, MGS_ERR_INVALID, "mgs_hier_native_send_segments: buffer too small"); seglens[w++] = len; }
    } else {
      nseg[p] = (int)P->pseg_len[p].size();
      for (int len : P->pseg_len[p]) { MGS_CHECK(h->ctx, w < cap, MGS_ERR_INVALID, "mgs_hier_native_send_segments: buffer too small"); seglens[w++] = len; }
    }
  }
  return w;
}
// The ranges the peers will send (their mgs_hier_native_send_segments, shipped by the host side).  COLLECTIVE by contract: every rank
// of the communicator calls it for the level before the next exchange — from this call on this rank, too, sends ranges.
int mgs_hier_set_native_recv_segments(mgs_hier *h, int level, const int *nseg, const int *seglens) {
  mgs_ctx *ctx = h->ctx;
  MGS_CHECK(ctx, level >= 0 && level < (int)h->lev.size() && h->lev[level].nx && nseg && seglens, MGS_ERR_STATE, "mgs_hier_set_native_recv_segments: level %d has no native plan", level);
  mgs_native_plan *P = h->lev[level].nx;
  std::vector<std::vector<int>> rs(P->rcnt.size());
  int w = 0;
  for (size_t p = 0; p < P->rcnt.size(); ++p) {
    int64_t sum = 0;
    for (int q = 0; q < nseg[p]; ++q) { const int len = seglens[w++]; MGS_CHECK(ctx, len > 0, MGS_ERR_INVALID, "mgs_hier_set_native_recv_segments: empty range"); rs[p].push_back(len); sum += len; }
    MGS_CHECK(ctx, sum == P->rcnt[p], MGS_ERR_INVALID, "mgs_hier_set_native_recv_segments: peer %d announces %lld values, the plan expects %d", (int)p, (long long)sum, P->rcnt[p]);
  }
  P->rseg_len.swap(rs);
  P->use_seg = true;
  mgs_drop_graph(h);
  return MGS_OK;
}
int mgs_hier_set_native_tail(mgs_hier *h, mgs_comm *c, mgs_hier *tail, const int *nlocs) {
  mgs_ctx *ctx = h->ctx;
  hipStreamSynchronize(ctx->stream);
  free_native_tail(h);
  mgs_drop_graph(h);
  if (!c || !tail) return MGS_OK;
  int world = 0, rank = 0; mgs_comm_size(c, &world, &rank);
  mgs_native_tail *T = new mgs_native_tail();
  h->ntail = T;                               // free_native_tail releases a half-built one on every error path below
  auto fail = [&](int rc) { free_native_tail(h); return rc; };
  T->comm = c; T->tail = tail; T->n_loc = nlocs[rank];
  std::vector<int> gi;
  for (int p = 0; p < world; ++p) { T->maxn = std::max(T->maxn, nlocs[p]); }
  for (int p = 0; p < world; ++p) { if (p == rank) T->my_off = (int)gi.size(); for (int j = 0; j < nlocs[p]; ++j) gi.push_back(p * T->maxn + j); }
  T->n_t = (int)gi.size();
  T->even = T->maxn > 0; for (int p = 0; p < world; ++p) T->even = T->even && nlocs[p] == T->maxn;
  if (!(T->n_t == tail->lev[0].n && T->n_loc == h->lev.back().n))
    return fail(mgs_fail(ctx, MGS_ERR_INVALID, "mgs_hier_set_native_tail: tail has %d rows, shards sum to %d", tail->lev[0].n, T->n_t));
  int rc = mgs_dev_alloc(ctx, &T->send, (size_t)std::max(T->maxn, 1));
  if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &T->all, (size_t)std::max(T->maxn, 1) * world);
  if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &T->gidx, (size_t)std::max(T->n_t, 1));
  if (rc == MGS_OK && hipMemset(T->send, 0, sizeof(double) * (size_t)std::max(T->maxn, 1)) != hipSuccess) rc = mgs_fail(ctx, MGS_ERR_HIP, "native tail: memset failed");
  if (rc == MGS_OK && T->n_t && hipMemcpy(T->gidx, gi.data(), sizeof(int) * gi.size(), hipMemcpyHostToDevice) != hipSuccess) rc = mgs_fail(ctx, MGS_ERR_HIP, "native tail: upload failed");
  if (rc == MGS_OK) rc = mgs_vec_create(ctx, T->n_t, &T->b);
  if (rc == MGS_OK) rc = mgs_vec_create(ctx, T->n_t, &T->x);
  if (rc != MGS_OK) return fail(rc);
  return MGS_OK;
}
// Global tail row of every halo slot of the LAST sharded level (host array, one int per slot: first row of the owner in the tail's
// numbering + the owner's local row).  The replicated tail's solution holds the neighbours' entries too, so the kernel that hands this
// rank its own slice also fills the level's halo slots from it: the post pass of the level above needs no halo exchange for e_c
// (one exchange less per cycle, same values and the same bits as the exchange would deliver).  n = 0 switches it off.
int mgs_hier_set_native_tail_halo(mgs_hier *h, const int *halo_global, int n) {
  mgs_ctx *ctx = h->ctx;
  MGS_CHECK(ctx, h->ntail, MGS_ERR_STATE, "mgs_hier_set_native_tail_halo: install the native tail first");
  mgs_native_tail *T = h->ntail;
  hipStreamSynchronize(ctx->stream);
  mgs_drop_graph(h);
  if (T->halo_global) { mgs_hip_free(T->halo_global); T->halo_global = nullptr; T->n_halo_global = 0; }
  if (n <= 0 || !halo_global) return MGS_OK;
  const mgs_csr *Al = h->lev.back().A;
  MGS_CHECK(ctx, n == Al->cols - Al->rows, MGS_ERR_INVALID, "mgs_hier_set_native_tail_halo: %d rows given, the last sharded level has %d halo slots", n, Al->cols - Al->rows);
  for (int k = 0; k < n; ++k) MGS_CHECK(ctx, halo_global[k] >= 0 && halo_global[k] < T->n_t, MGS_ERR_INVALID, "mgs_hier_set_native_tail_halo: slot %d maps to row %d outside the tail (%d rows)", k, halo_global[k], T->n_t);
  MGS_TRY(mgs_dev_alloc(ctx, &T->halo_global, (size_t)n));
  MGS_HIP(ctx, hipMemcpy(T->halo_global, halo_global, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
  T->n_halo_global = n;
  return MGS_OK;
}
int mgs_hier_set_halo_exchange_fused(mgs_hier *h, mgs_halo_fused_fn fn, void *user) { h->halo_fused = fn; h->halo_user = user; mgs_drop_graph(h); return MGS_OK; }
int mgs_hier_set_kcycle(mgs_hier *h, int levels) {
  MGS_CHECK(h->ctx, levels >= 0, MGS_ERR_INVALID, "mgs_hier_set_kcycle: negative level count");
  h->kcycle_levels = levels; mgs_drop_graph(h);
  return MGS_OK;
}
int mgs_hier_set_kcycle_entry(mgs_hier *h, int on) { h->kcycle_entry = on != 0; mgs_drop_graph(h); return MGS_OK; }
int mgs_hier_kcycle_scalars(mgs_hier *h, int level, double out[5]) {
  MGS_CHECK(nullptr, h && out, MGS_ERR_INVALID, "mgs_hier_kcycle_scalars: NULL argument");
  mgs_ctx *ctx = h->ctx;
  MGS_TRY(mgs_level_in_range(h, level, "mgs_hier_kcycle_scalars"));
  const mgs_level &L = h->lev[level];
  MGS_CHECK(ctx, L.kscal, MGS_ERR_STATE, "mgs_hier_kcycle_scalars: level %d has run no K step", level);
  MGS_HIP(ctx, hipMemcpyAsync(out, L.kscal, sizeof(double) * 5, hipMemcpyDeviceToHost, ctx->stream));
  MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MGS_OK;
}
int mgs_hier_set_correction_scale(mgs_hier *h, double sigma) {
  MGS_CHECK(h->ctx, sigma > 0.0 && sigma <= 4.0, MGS_ERR_INVALID, "mgs_hier_set_correction_scale: sigma must lie in (0, 4]");
  h->corr_scale = sigma; mgs_drop_graph(h);
  return MGS_OK;
}
int mgs_hier_set_additive(mgs_hier *h, int on) {
  MGS_CHECK(h->ctx, !on || (!h->halo && !h->halo_begin && !h->native), MGS_ERR_STATE, "mgs_hier_set_additive: not offered on row shards");
  h->additive = on != 0; mgs_drop_graph(h);
  return MGS_OK;
}
int mgs_hier_set_halo_exchange(mgs_hier *h, mgs_halo_fn fn, void *user) { h->halo = fn; h->halo_user = user; mgs_drop_graph(h); return MGS_OK; }
int mgs_hier_set_halo_exchange_split(mgs_hier *h, mgs_halo_fn begin, mgs_halo_fn end, void *user) {
  MGS_CHECK(h->ctx, (begin == nullptr) == (end == nullptr), MGS_ERR_INVALID, "split exchange needs both begin and end");
  h->halo_begin = begin; h->halo_end = end; h->halo_user = user; mgs_drop_graph(h);
  return MGS_OK;
}
int mgs_hier_nlev(const mgs_hier *h) { return (int)h->lev.size(); }
int mgs_hier_level_shape(const mgs_hier *h, int l, int *rows, int64_t *nnz) {
  MGS_CHECK(h->ctx, l >= 0 && l < (int)h->lev.size(), MGS_ERR_INVALID, "level %d out of range", l);
  if (rows) *rows = h->lev[l].A->rows; if (nnz) *nnz = h->lev[l].A->nnz;
  return MGS_OK;
}
const mgs_csr *mgs_hier_level_A(const mgs_hier *h, int l) { return (l >= 0 && l < (int)h->lev.size()) ? h->lev[l].A : nullptr; }
const mgs_xfer *mgs_hier_level_P(const mgs_hier *h, int l) { return (l >= 0 && l < (int)h->lev.size()) ? h->lev[l].T : nullptr; }
const mgs_csr *mgs_hier_level_AP(const mgs_hier *h, int l) { return (h && l >= 0 && l < (int)h->lev.size()) ? h->lev[l].AP : nullptr; }

static int push_level(mgs_hier *h, mgs_xfer *T, mgs_csr *Ac) {
  h->lev.back().T = T;
  h->lev.emplace_back();
  int rc = level_init(h, h->lev.back(), Ac, true);
  h->finalized = false; h->refresh_failed = false; mgs_drop_graph(h);
  if (h->inv) { mgs_hip_free(h->inv); h->inv = nullptr; }
  return rc;
}

int mgs_hier_push_P(mgs_hier *h, const mgs_csr *P) {
  mgs_ctx *ctx = h->ctx;
  const mgs_csr *A = h->lev.back().A;
  MGS_CHECK(ctx, A->rows == A->cols, MGS_ERR_STATE, "mgs_hier_push_P: sharded operators take their hierarchy from mgs_hier_coarsen");
  MGS_CHECK(ctx, P->rows == A->rows, MGS_ERR_INVALID, "mgs_hier_push_P: P has %d rows, coarsest operator has %d", P->rows, A->rows);
  MGS_CHECK(ctx, P->cols > 0, MGS_ERR_INVALID, "mgs_hier_push_P: P has no columns");
  MGS_TRY(diag0_needed(h, "mgs_hier_push_P"));
  mgs_xfer *T = nullptr; mgs_csr *Ac = nullptr;
  MGS_TRY(k_xfer_from_csr(P, &T));
  int rc = mgs_csr_galerkin(A, T, &Ac);
  if (rc != MGS_OK) { mgs_xfer_destroy(T); return rc; }
  return push_level(h, T, Ac);
}

int mgs_aggregate_shard(const mgs_csr *A, double ktg, int npass, double tou, mgs_xfer **T) { return mgs_aggregate_shard_zoned(A, ktg, npass, tou, nullptr, T); }
// zone (host, one int per owned row; NULL: none): rows of different zones never share an aggregate.  The host side gives the rows a peer
// sees as halo a zone of their own: the aggregates that peer will ask for at the next level are then exactly the aggregates of those
// rows — a contiguous id range on plane shards, level after level — and every halo exchange sends ranges straight from the vectors.
int mgs_aggregate_shard_zoned(const mgs_csr *A, double ktg, int npass, double tou, const int *zone, mgs_xfer **T) {
  mgs_ctx *ctx = A->ctx;
  mgs_csr *Ac = nullptr;
  int *dz = nullptr;
  if (zone && A->rows) {
    MGS_TRY(mgs_dev_alloc(ctx, &dz, (size_t)A->rows));
    if (hipMemcpy(dz, zone, sizeof(int) * (size_t)A->rows, hipMemcpyHostToDevice) != hipSuccess) { mgs_hip_free(dz); return mgs_fail(ctx, MGS_ERR_HIP, "mgs_aggregate_shard_zoned: upload failed"); }
  }
  const int rc = k_pairwise_aggregate(A, ktg, npass, tou, T, &Ac, dz);
  hipStreamSynchronize(ctx->stream);
  if (dz) mgs_hip_free(dz);
  if (Ac) mgs_csr_destroy(Ac);
  return rc;
}
int mgs_galerkin_shard(const mgs_csr *A, const mgs_xfer *T, const int *halo_coarse_col, int n_halo_coarse, mgs_csr **Ac) {
  mgs_ctx *ctx = A->ctx;
  const int n_halo = A->cols - A->rows;
  MGS_CHECK(ctx, n_halo >= 0 && (n_halo == 0 || halo_coarse_col), MGS_ERR_INVALID, "mgs_galerkin_shard: halo map missing");
  if (n_halo == 0) return k_galerkin_agg(A, T, Ac);
  for (int k = 0; k < n_halo; ++k)
    MGS_CHECK(ctx, halo_coarse_col[k] == -1 || (halo_coarse_col[k] >= T->n_coarse && halo_coarse_col[k] < T->n_coarse + n_halo_coarse), MGS_ERR_INVALID,
              "mgs_galerkin_shard: halo slot %d maps to coarse column %d outside [%d,%d)", k, halo_coarse_col[k], T->n_coarse, T->n_coarse + n_halo_coarse);
  int *d = nullptr;
  MGS_TRY(mgs_dev_alloc(ctx, &d, (size_t)n_halo));
  MGS_HIP(ctx, hipMemcpyAsync(d, halo_coarse_col, sizeof(int) * (size_t)n_halo, hipMemcpyHostToDevice, ctx->stream));
  int rc = k_galerkin_agg_ext(A, T, d, n_halo_coarse, Ac);
  hipStreamSynchronize(ctx->stream);
  if (rc != MGS_OK) { mgs_hip_free(d); return rc; }
  // the map stays with the transfer: the fused post pass runs on A·P whose halo columns are the coarse level's own halo columns
  mgs_xfer *Tm = const_cast<mgs_xfer *>(T);
  if (Tm->halo_cmap) mgs_hip_free(Tm->halo_cmap);
  Tm->halo_cmap = d; Tm->n_halo_fine = n_halo; Tm->n_halo_coarse = n_halo_coarse;
  return MGS_OK;
}
int mgs_hier_push_level(mgs_hier *h, mgs_xfer *T, mgs_csr *Ac) {
  mgs_ctx *ctx = h->ctx;
  MGS_CHECK(ctx, T && Ac && T->n_fine == h->lev.back().A->rows && T->n_coarse == Ac->rows && Ac->rows <= Ac->cols, MGS_ERR_INVALID, "mgs_hier_push_level: shape mismatch");
  MGS_TRY(diag0_needed(h, "mgs_hier_push_level"));
  return push_level(h, T, Ac);
}
int mgs_xfer_from_agg(mgs_ctx *ctx, int n_fine, int n_coarse, const int *agg, mgs_xfer **out) { return k_xfer_from_agg_host(ctx, n_fine, n_coarse, agg, out); }
int mgs_hier_set_coarse_solver(mgs_hier *h, mgs_coarse_fn fn, void *user) { h->coarse = fn; h->coarse_user = user; mgs_drop_graph(h); if (fn) h->finalized = true; return MGS_OK; }

int mgs_hier_coarsen(mgs_hier *h, double ktg, int npass, double tou, int coarse_rows, int max_levels) {
  mgs_ctx *ctx = h->ctx;
  while ((int)h->lev.size() < max_levels && h->lev.back().A->rows > coarse_rows) {
    const mgs_csr *A = h->lev.back().A;
    MGS_CHECK(ctx, A->rows == A->cols, MGS_ERR_STATE, "mgs_hier_coarsen: operator is not square");
    MGS_TRY(diag0_needed(h, "mgs_hier_coarsen"));
    mgs_xfer *T = nullptr; mgs_csr *Ac = nullptr;
    MGS_TRY(k_pairwise_aggregate(A, ktg, npass, tou, &T, &Ac));
    if (Ac->rows == 0 || Ac->rows > (int)(0.9 * A->rows)) {  // coarsening stalled (or everything in G0)
      mgs_xfer_destroy(T); mgs_csr_destroy(Ac);
      break;
    }
    MGS_TRY(push_level(h, T, Ac));
  }
  return MGS_OK;
}

// Constant null space declared on the fine operator: the regularised coarsest solve is valid only if every level inherits the null
// space, P·1_c = 1 — aggregation transfers that cover every row (T->nnz counts the rows inside an aggregate), no row shards.  Structural,
// no tolerance, nothing launched.
static bool hier_nullspace_const(const mgs_hier *h) { return h->lev[0].A->nullspace == MGS_NULLSPACE_CONSTANT; }
static int nullspace_check(mgs_hier *h, const char *who) {
  mgs_ctx *ctx = h->ctx;
  const int nl = (int)h->lev.size();
  MGS_CHECK(ctx, !(h->halo || h->halo_begin || h->halo_fused || h->native || h->ntail || h->coarse), MGS_ERR_INVALID,
            "%s: constant null space declared on a row-sharded hierarchy (halo callbacks, native plans or tail)", who);
  for (int l = 0; l < nl; ++l) {
    const mgs_level &L = h->lev[l];
    MGS_CHECK(ctx, L.A->cols == L.A->rows && !L.nx, MGS_ERR_INVALID, "%s: constant null space declared, level %d is a row shard (halo columns or a native plan)", who, l);
    if (l + 1 >= nl) break;
    MGS_CHECK(ctx, L.T && L.T->aggregation, MGS_ERR_INVALID, "%s: constant null space declared, the transfer of level %d is a general P, not an aggregation", who, l);
    MGS_CHECK(ctx, L.T->nnz == (int64_t)L.T->n_fine, MGS_ERR_INVALID, "%s: constant null space declared, the transfer of level %d leaves %lld rows outside every aggregate", who, l,
              (long long)(L.T->n_fine - L.T->nnz));
  }
  return MGS_OK;
}

// Field-wise null space declared on the fine operator: the structural refusals of the constant kind without the "every row aggregated" rule (rows
// labelled −1 may stay outside), then — build = true — the coarse labels level by level with their check kernel (k_coarse_labels) and the
// coarsest level's rows per field.  mgs_hier_refresh keeps the labels (they depend on the pattern only) and checks the structure alone.
static bool hier_nullspace_fields(const mgs_hier *h) { return h->lev[0].A->nullspace == MGS_NULLSPACE_FIELDS && h->lev[0].A->nsf; }
static int nullspace_fields_prepare(mgs_hier *h, const char *who, bool build) {
  mgs_ctx *ctx = h->ctx;
  const int nl = (int)h->lev.size();
  const mgs_nsfields *F = h->lev[0].A->nsf;
  MGS_CHECK(ctx, !(h->halo || h->halo_begin || h->halo_fused || h->native || h->ntail || h->coarse), MGS_ERR_INVALID,
            "%s: field-wise null space declared on a row-sharded hierarchy (halo callbacks, native plans or tail)", who);
  for (int l = 0; l < nl; ++l) {
    const mgs_level &L = h->lev[l];
    MGS_CHECK(ctx, L.A->cols == L.A->rows && !L.nx, MGS_ERR_INVALID, "%s: field-wise null space declared, level %d is a row shard (halo columns or a native plan)", who, l);
    MGS_CHECK(ctx, l + 1 >= nl || (L.T && L.T->aggregation), MGS_ERR_INVALID, "%s: field-wise null space declared, the transfer of level %d is a general P, not an aggregation", who, l);
  }
  if (!build) {
    for (int l = 1; l < nl; ++l) MGS_CHECK(ctx, h->lev[l].ns_lab, MGS_ERR_STATE, "%s: the field labels of level %d were never built (declare the fields before mgs_hier_finalize)", who, l);
    MGS_CHECK(ctx, h->ns_nf == F->nfields, MGS_ERR_STATE, "%s: the hierarchy was finalized for %d fields, the fine operator declares %d", who, h->ns_nf, F->nfields);
    return MGS_OK;
  }
  unsigned long long *bad = nullptr;
  std::vector<unsigned long long> hb((size_t)nl, ~0ull);
  std::vector<signed char> hl;
  auto run = [&]() -> int {
    MGS_TRY(mgs_dev_alloc(ctx, &bad, (size_t)nl));
    MGS_HIP(ctx, hipMemsetAsync(bad, 0xff, sizeof(unsigned long long) * (size_t)nl, ctx->stream));
    const signed char *lab = F->labels;
    for (int l = 0; l + 1 < nl; ++l) {
      mgs_level &C = h->lev[l + 1];
      if (C.ns_lab) { MGS_HIP(ctx, hipStreamSynchronize(ctx->stream)); mgs_hip_free(C.ns_lab); C.ns_lab = nullptr; }
      MGS_TRY(mgs_dev_alloc(ctx, &C.ns_lab, (size_t)h->lev[l].T->n_coarse + 2));
      MGS_HIP(ctx, hipMemsetAsync(C.ns_lab, 0xff, (size_t)h->lev[l].T->n_coarse + 2, ctx->stream));
      MGS_TRY(k_coarse_labels(ctx, h->lev[l].T, lab, C.ns_lab, bad + l));
      lab = C.ns_lab;
    }
    hl.resize((size_t)h->lev.back().A->rows);
    MGS_HIP(ctx, hipMemcpyAsync(hb.data(), bad, sizeof(unsigned long long) * (size_t)nl, hipMemcpyDeviceToHost, ctx->stream));
    if (!hl.empty()) MGS_HIP(ctx, hipMemcpyAsync(hl.data(), lab, hl.size(), hipMemcpyDeviceToHost, ctx->stream));
    MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MGS_OK;
  };
  const int rc = run();
  if (rc != MGS_OK) hipStreamSynchronize(ctx->stream);
  if (bad) mgs_hip_free(bad);
  MGS_TRY(rc);
  for (int l = 0; l + 1 < nl; ++l) {
    if (hb[l] == ~0ull) continue;
    const long long row = (long long)(hb[l] >> 1);
    if (hb[l] & 1ull) return mgs_fail(ctx, MGS_ERR_INVALID, "%s: field-wise null space declared, row %lld of level %d carries a label and lies outside every aggregate", who, row, l);
    return mgs_fail(ctx, MGS_ERR_INVALID, "%s: field-wise null space declared, row %lld of level %d shares an aggregate with a row of another label", who, row, l);
  }
  h->ns_nf = F->nfields;
  for (int f = 0; f < MGS_NULLSPACE_MAX_FIELDS; ++f) h->ns_ccount[f] = 0.0;
  for (signed char c : hl) if (c >= 0 && c < MGS_NULLSPACE_MAX_FIELDS) h->ns_ccount[(int)c] += 1.0;
  return MGS_OK;
}
static const signed char *coarsest_labels(const mgs_hier *h) { return h->lev.size() > 1 ? h->lev.back().ns_lab : h->lev[0].A->nsf->labels; }

int mgs_hier_finalize(mgs_hier *h) {
  mgs_ctx *ctx = h->ctx;
  const mgs_csr *Ac = h->lev.back().A;
  const bool ns = hier_nullspace_const(h), nsf = hier_nullspace_fields(h);
  if (ns) MGS_TRY(nullspace_check(h, "mgs_hier_finalize"));
  if (nsf) MGS_TRY(nullspace_fields_prepare(h, "mgs_hier_finalize", true));
  MGS_CHECK(ctx, Ac->rows == Ac->cols, MGS_ERR_STATE, "coarsest operator is not square");
  if (h->inv) { mgs_hip_free(h->inv); h->inv = nullptr; }
  h->nc = Ac->rows;
  h->coarse_sweeps = 0;
  h->refresh_failed = false;
  if (Ac->rows > 8192) {
    // Coarsening stopped far above the dense limit (e.g. every row is in G0: the operator is so diagonally
    // dominant that Jacobi alone converges, AGMG.cpp:118-123).  The coarsest level is then smoothed
    // (8 damped-Jacobi sweeps from 0) instead of solved; the cycle stays a fixed linear operator.
    if (h->lev.size() == 1) MGS_TRY(diag0_needed(h, "mgs_hier_finalize (smoothed coarsest level)"));
    h->coarse_sweeps = 8;
    h->finalized = true; mgs_drop_graph(h);
    return MGS_OK;
  }
  if (nsf) MGS_TRY(k_dense_inverse(ctx, Ac, &h->inv, 2, coarsest_labels(h), h->ns_ccount));
  else MGS_TRY(k_dense_inverse(ctx, Ac, &h->inv, ns ? 1 : 0));
  h->finalized = true; mgs_drop_graph(h);
  return MGS_OK;
}

// Values changed, pattern did not: everything in h that depends on matrix VALUES is recomputed from the fine operator's current
// values, level by level from the top — D⁻¹, the next level's operator (numeric Galerkin product into the existing val array), and
// whichever operands of the fused passes mgs_prepare_fused has already built (mgs_operands_fill), each in its existing
// buffer.  Aggregates, patterns, pattern codes, row-block groups, buffers and — because no device buffer moves — the cached cycle
// graphs are kept.  Everything is enqueued on the context's stream; the host reads two counters once, before the dense inverse.
int mgs_hier_refresh(mgs_hier *h) {
  MGS_CHECK(nullptr, h, MGS_ERR_INVALID, "mgs_hier_refresh: NULL hierarchy");
  mgs_ctx *ctx = h->ctx;
  MGS_CHECK(ctx, h->finalized || h->refresh_failed, MGS_ERR_STATE, "mgs_hier_refresh: call mgs_hier_finalize first");
  MGS_CHECK(ctx, !ctx->opt_valcode, MGS_ERR_INVALID, "mgs_hier_refresh: option valcode is on (pattern codes carry the values): rebuild the hierarchy instead");
  MGS_CHECK(ctx, !mgs_hier_sharded(h), MGS_ERR_INVALID, "mgs_hier_refresh: row-sharded hierarchies (halo columns, halo callbacks, native plans or tail) are not refreshed: rebuild them");
  const int nl = (int)h->lev.size();
  for (int l = 0; l < nl; ++l) {
    const mgs_level &L = h->lev[l];
    MGS_CHECK(ctx, l + 1 >= nl || (L.T && L.T->aggregation), MGS_ERR_INVALID, "mgs_hier_refresh: the transfer of level %d is a general P, not an aggregation", l);
    MGS_CHECK(ctx, !(L.A->code && L.A->code->vtab) && !L.code_hat && !(L.code_ap && L.code_ap->vtab), MGS_ERR_INVALID,
              "mgs_hier_refresh: level %d carries a value-carrying pattern code (built under option valcode)", l);
  }
  const bool ns = hier_nullspace_const(h), nsf = hier_nullspace_fields(h);
  if (ns) MGS_TRY(nullspace_check(h, "mgs_hier_refresh"));
  if (nsf) MGS_TRY(nullspace_fields_prepare(h, "mgs_hier_refresh", false));
  bool kept = true;
  if (!h->refresh_flags) MGS_TRY(mgs_dev_alloc(ctx, &h->refresh_flags, 2));
  MGS_HIP(ctx, hipMemsetAsync(h->refresh_flags, 0, 2 * sizeof(int), ctx->stream));
  if (h->nd_flag) MGS_HIP(ctx, hipMemsetAsync(h->nd_flag, 0, sizeof(int), ctx->stream));
  int rc = MGS_OK;
  for (int l = 0; l < nl && rc == MGS_OK; ++l) {
    mgs_level &L = h->lev[l];
    rc = k_diag_inv_async(L.A, L.dinv->d, h->refresh_flags);
    if (l + 1 >= nl) break;
    if (rc == MGS_OK) rc = k_galerkin_numeric(L.A, L.T->n_coarse, L.T->cptr, L.T->members, L.T->agg, const_cast<mgs_csr *>(h->lev[l + 1].A), h->refresh_flags + 1);
    mgs_operands_mark(L, OPD_WD | OPD_AP); if (rc == MGS_OK) rc = mgs_operands_fill(h, l, ~0u);      // the whole chain of derived operands: refilled where built, each in its existing buffer
  }
  int flags[2] = {0, 0}, nd_bad = 0;
  if (rc == MGS_OK && h->nd_flag && hipMemcpyAsync(&nd_bad, h->nd_flag, sizeof nd_bad, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = mgs_fail(ctx, MGS_ERR_HIP, "mgs_hier_refresh: flag copy failed");
  if (rc == MGS_OK && hipMemcpyAsync(flags, h->refresh_flags, sizeof flags, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = mgs_fail(ctx, MGS_ERR_HIP, "mgs_hier_refresh: flag copy failed");
  if (rc == MGS_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = mgs_fail(ctx, MGS_ERR_HIP, "mgs_hier_refresh: %s", hipGetErrorString(hipGetLastError()));
  if (rc == MGS_OK && flags[1]) rc = mgs_fail(ctx, MGS_ERR_STATE, "mgs_hier_refresh: %d entries fall outside the kept coarse patterns (the fine pattern is not the one the hierarchy was built for)", flags[1]);
  if (rc == MGS_OK && nl == 1 && !h->coarse_sweeps) { h->bad_diag0 = flags[0]; flags[0] = 0; }   // one level, solved densely: D⁻¹ is not used (mgs_hier_create)
  if (rc == MGS_OK && flags[0]) rc = mgs_fail(ctx, MGS_ERR_NUMERIC, "mgs_hier_refresh: %d rows of the refreshed operators have a missing or zero diagonal", flags[0]);
  if (rc == MGS_OK && nd_bad) {      // a diagonal entry of some Â no longer fits its byte: those levels stream val_wd again (cached graphs read val_nd)
    for (auto &L : h->lev) L.nd_ok = false;
    kept = false; mgs_drop_graph(h);
  }
  if (rc == MGS_OK && !h->coarse_sweeps) {      // coarsest dense inverse, into the buffer the cached graphs know
    if (!h->inv) { kept = false; mgs_drop_graph(h); }
    rc = nsf ? k_dense_inverse(ctx, h->lev.back().A, &h->inv, 2, coarsest_labels(h), h->ns_ccount) : k_dense_inverse(ctx, h->lev.back().A, &h->inv, ns ? 1 : 0);
  }
  if (rc != MGS_OK) {      // half-refreshed state must not be replayed: no cycle until a later refresh (or finalize) succeeds
    h->finalized = false; h->refresh_failed = true; h->refresh_kept_graphs = 0; mgs_drop_graph(h);
    return rc;
  }
  h->finalized = true; h->refresh_failed = false;
  ++h->refresh_count; h->refresh_kept_graphs = kept ? 1 : 0; h->refresh_dev_levels = nl - 1;
  return MGS_OK;
}
int mgs_hier_refresh_info(const mgs_hier *h, int64_t out[4]) {
  MGS_CHECK(nullptr, h && out, MGS_ERR_INVALID, "mgs_hier_refresh_info: NULL argument");
  out[0] = h->refresh_count; out[1] = h->refresh_kept_graphs; out[2] = h->refresh_dev_levels; out[3] = h->refresh_flags ? (int64_t)(2 * sizeof(int)) : 0;
  return MGS_OK;
}

int mgs_hier_group_info(const mgs_hier *h, int level, int64_t out[4]) {
  MGS_TRY(mgs_level_in_range(h, level, "mgs_hier_group_info"));
  const mgs_groups *G = h->lev[level].grp;
  out[0] = G ? G->ngroups : 0; out[1] = G ? G->nblocks - G->ngroups : 0;   /* blocks merged into another block's group */ out[2] = G ? G->nstray : 0; out[3] = mgs_row_blocks(h->lev[level].A);
  return MGS_OK;
}
int mgs_hier_graph_info(const mgs_hier *h, int64_t out[4]) {
  int n = 0; for (auto &g : h->graphs) n += g.exec != nullptr;
  out[0] = n; out[1] = (h->native || h->ntail) ? 1 : 0; out[2] = h->native_graph_failed ? 1 : 0; out[3] = h->native_eager_runs;
  return MGS_OK;
}

int64_t mgs_hier_vcycle_bytes(const mgs_hier *h) {
  // algorithmic bytes of the kernels one zero-guess cycle actually launches.
  // Every level starts from x = 0: the first pre-sweep is the 24n-byte (ωD⁻¹)b kernel, not a
  // Jacobi pass.  Fused form (V(1,1)): pass A reads the matrix, wd, b and writes r;
  // pass B reads the matrix, r, b, wd, agg, e_c and writes x.
  int64_t tot = 0;
  const int L = (int)h->lev.size();
  for (int l = 0; l < L - 1; ++l) {
    const mgs_level &lv = h->lev[l];
    int64_t n = lv.A->rows, nnz = lv.A->nnz, nc = h->lev[l + 1].A->rows, nnzP = lv.T ? lv.T->nnz : 0;
    const int64_t jac = 12 * nnz + 36 * n + 4, res = 12 * nnz + 28 * n + 4;
    const int64_t restr = 4 * (nc + 1) + 12 * nnzP + 8 * nc;
    const bool fused = h->ctx->opt_fuse && h->nu1 == 1 && h->nu2 == 1 && !h->halo && !h->halo_begin && lv.T && lv.T->aggregation &&
                       lv.A->rows == lv.A->cols;
    // FP32 level: 4 instead of 8 value bytes per entry in both passes
    if (fused) { tot += (12 * nnz + 28 * n + 4) + restr + (12 * nnz + 40 * n + 8 * nc + 4) - (mgs_level_runs_f32(h, l) ? 8 * nnz : 0); continue; }
    if (h->nu1 > 0) tot += 24 * n + (int64_t)(h->nu1 - 1) * jac + res;   // shortcut + sweeps + residual
    // ν1 = 0: r = b, no residual pass
    tot += restr;
    tot += (h->nu1 > 0 ? 20 * n : 12 * n) + 8 * nc;                        // prolong-add / prolong
    tot += (int64_t)h->nu2 * jac;
  }
  if (h->coarse_sweeps > 0) { const mgs_csr *Ac = h->lev.back().A; tot += 24 * (int64_t)Ac->rows + (int64_t)(h->coarse_sweeps - 1) * (12 * Ac->nnz + 36 * (int64_t)Ac->rows + 4); }
  else tot += (int64_t)h->nc * h->nc * 8 + 16 * (int64_t)h->nc;
  return tot;
}

// ------------------------------------------------------------------ instrumentation
int mgs_time_kernel(const mgs_csr *A, int op, const mgs_vec *x, const mgs_vec *b, const mgs_vec *dinv, mgs_vec *out, int reps, double *ms) {
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, reps > 0 && ms && x && out, MGS_ERR_INVALID, "mgs_time_kernel: bad arguments");
  MGS_CHECK(ctx, op == MGS_OP_SPMV || (b && (op == MGS_OP_RESIDUAL || dinv)), MGS_ERR_INVALID, "mgs_time_kernel: missing operand");
  const bool upd = op == 3;      // mgs_minres's update pass: x = z̃, b = w, dinv = w_prev, out = the solution; coefficients that keep every entry bounded
  MGS_CHECK(ctx, !upd || (x->n >= A->rows && b->n >= A->rows && dinv->n >= A->rows && out->n >= A->rows), MGS_ERR_INVALID, "mgs_time_kernel: vectors shorter than %d", A->rows);
  hipEvent_t e0, e1;
  MGS_HIP(ctx, hipEventCreate(&e0)); MGS_HIP(ctx, hipEventCreate(&e1));
  MGS_HIP(ctx, hipEventRecord(e0, ctx->stream));
  for (int i = 0; i < reps; ++i) {
    if (upd) MGS_TRY(k_minres_update(ctx, A->rows, 0.7, -0.3, 1.9, 2.3, 1.1e-3, x->d, dinv->d, b->d, out->d));
    else MGS_TRY(mgs_launch_csr_op(A, op, x->d, b ? b->d : nullptr, dinv ? dinv->d : nullptr, 0.6, out->d));
  }
  MGS_HIP(ctx, hipEventRecord(e1, ctx->stream));
  MGS_HIP(ctx, hipEventSynchronize(e1));
  float t = 0; MGS_HIP(ctx, hipEventElapsedTime(&t, e0, e1));
  hipEventDestroy(e0); hipEventDestroy(e1);
  *ms = (double)t / reps;
  return MGS_OK;
}

}  // extern "C"
