// extract.hip — blocks of a device matrix and index lists on vectors: S = A(rows, cols) with the listed columns renumbered to their place in
// the list (mgs_csr_extract), the values of S again through the kept source positions (mgs_csr_extract_numeric), y[k] = x[idx[k]]
// (mgs_vec_gather) and x[idx[k]] = y[k] (mgs_vec_scatter).  No reference counterpart: the reference reads its operators from files.
//
// The lists are the caller's device arrays.  Ingest rule (ingest.hip): no kernel uses a list entry as an address before it has compared it
// with its bounds as a 64-bit value.  The row list is narrowed into an array of the library's own in which a refused entry is −1, and every
// later kernel passes −1 over; a column enters the column map only if it is in range; the lowest violation of either list comes back
// through one 64-bit atomicMin word each, so the message is deterministic.  The vector kernels check every index where they use it.
//
// Values are moved as 64-bit words: −0.0 stays −0.0 and a NaN keeps its payload.
//
// Phases of the block: lists checked, column map (map[cols[q]] = q, −1 elsewhere) → entries per output row, a 64-bit total beside them →
// scan → columns, values and (keep_map) source positions.  Count and fill have three arms:
//   (a) no column list: the count is the source row's length, the fill is entry-parallel (output entry k finds its row by bisection in
//       S's rowptr, as scale_kernel does), stores coalesced;
//   (b) source row of at most 64 entries: one lane per output row, a serial pass through the map;
//   (c) longer source rows: one wave per output row, four per workgroup, 64 entries at a time, nothing staged, so a row may be of any
//       length.  A kept entry lands at carry + popcount(ballot & lower lanes); whole waves leave early.
// The column list ascends strictly, so a row of S ascends without a sort.  Every place is computed from the row alone, no atomics on values
// or places: two calls give identical arrays (the list of wave rows is filled in any order — it only says which rows arm (c) serves).
#include "mgs_internal.hpp"

struct mgs_extract_plan {
  int *src = nullptr;           // keep_map: position in A's arrays of every entry of S (4 B per entry)
  bool keep = false;
  int64_t n_lane = 0, n_wave = 0;
  int a_rows = 0, a_cols = 0;   // the source as it was: mgs_csr_extract_numeric refuses another shape or entry count
  int64_t a_nnz = 0;
};
void mgs_free_extract(mgs_extract_plan *p) {
  if (!p) return;
  if (p->src) mgs_hip_free(p->src);
  delete p;
}

namespace {
typedef unsigned long long u64;
constexpr int TB = 256;
constexpr int WAVE = 64;
constexpr int EXT_LANE_LEN = 64;      // source rows of at most this many entries: one lane per output row
constexpr u64 NO_ERR = ~0ull;
enum { EXT_COUNT = 0, EXT_FILL = 1 };
enum { ST_ROW = 0, ST_COL = 1, ST_TOTAL = 2, ST_WAVE = 3 };   // lowest bad row position, lowest bad column position << 1 | kind, entries of S, rows listed for arm (c)
enum { BAD_RANGE = 0, BAD_ASCENDING = 1 };

struct DevBuf {  // RAII for temporaries
  void *p = nullptr;
  ~DevBuf() { if (p) mgs_hip_free(p); }
  template <class T> T *as() { return (T *)p; }
};
template <class T>
int dalloc(mgs_ctx *ctx, DevBuf &b, size_t count) { T *q = nullptr; MGS_TRY(mgs_dev_alloc(ctx, &q, count)); b.p = q; return MGS_OK; }

// ------------------------------------------------------------------ the lists: check + narrow
template <class I>
__global__ void ext_rows_kernel(long long nr, int arows, const I *__restrict__ in, int *__restrict__ out, u64 *__restrict__ st) {
  const long long k = (long long)blockIdx.x * TB + threadIdx.x;
  if (k >= nr) return;
  const long long v = (long long)in[k];
  const bool bad = v < 0 || v >= arows;
  if (bad) atomicMin(&st[ST_ROW], (u64)k);
  out[k] = bad ? -1 : (int)v;
}
// map has acols entries, all −1 before this kernel
template <class I>
__global__ void ext_cols_kernel(long long nc, int acols, const I *__restrict__ in, int *__restrict__ map, u64 *__restrict__ st) {
  const long long q = (long long)blockIdx.x * TB + threadIdx.x;
  if (q >= nc) return;
  const long long v = (long long)in[q];
  if (v < 0 || v >= acols) { atomicMin(&st[ST_COL], ((u64)q << 1) | BAD_RANGE); return; }
  if (q > 0 && (long long)in[q - 1] >= v) atomicMin(&st[ST_COL], ((u64)q << 1) | BAD_ASCENDING);
  map[v] = (int)q;
}

// sum of n over the wave into st[ST_TOTAL]; every lane of the wave calls it
__device__ __forceinline__ void ext_add_total(int n, u64 *__restrict__ st) {
  u64 s = (u64)n;
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(&st[ST_TOTAL], s);
}

// ------------------------------------------------------------------ arm (a): no column list
__global__ void ext_len_kernel(int nr, const int *__restrict__ rows, const int *__restrict__ arp, int *__restrict__ cnt, u64 *__restrict__ st) {
  const int k = blockIdx.x * TB + threadIdx.x;
  int n = 0;
  if (k < nr) {
    const int r = rows ? rows[k] : k;
    if (r >= 0) n = arp[r + 1] - arp[r];
    cnt[k] = n;
  }
  ext_add_total(n, st);
}
__global__ void ext_rowcopy_kernel(long long nnz, int nr, const int *__restrict__ rows, const int *__restrict__ arp, const int *__restrict__ aci, const u64 *__restrict__ av,
                                   const int *__restrict__ srp, int *__restrict__ scol, u64 *__restrict__ sval, int *__restrict__ src) {
  const long long k = (long long)blockIdx.x * TB + threadIdx.x;
  if (k >= nnz) return;
  int lo = 0, hi = nr;      // the entry's row: the last o with srp[o] ≤ k (empty rows share their successor's start and are passed over)
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((long long)srp[mid] <= k) lo = mid; else hi = mid;
  }
  const int r = rows ? rows[lo] : lo;
  if (r < 0) return;
  const int a0 = arp[r], off = (int)(k - srp[lo]);
  if (off >= arp[r + 1] - a0) return;      // cannot happen: srp is the scan of these lengths
  scol[k] = aci[a0 + off];
  sval[k] = av[a0 + off];
  if (src) src[k] = a0 + off;
}

// ------------------------------------------------------------------ arm (b): one lane per output row
template <int MODE>
__global__ __launch_bounds__(TB) void ext_lane_kernel(int nr, const int *__restrict__ rows, const int *__restrict__ arp, const int *__restrict__ aci, const u64 *__restrict__ av,
                                                      const int *__restrict__ map, int *__restrict__ cnt, int *__restrict__ wave_rows, u64 *__restrict__ st,
                                                      const int *__restrict__ srp, int *__restrict__ scol, u64 *__restrict__ sval, int *__restrict__ src) {
  const int k = blockIdx.x * TB + threadIdx.x;
  int n = 0;
  if (k < nr) {
    const int r = rows ? rows[k] : k;
    if (r >= 0) {
      const int a0 = arp[r], len = arp[r + 1] - a0;
      if (len <= EXT_LANE_LEN) {
        if (MODE == EXT_COUNT) {
          for (int p = a0; p < a0 + len; ++p) n += map[aci[p]] >= 0 ? 1 : 0;
        } else {
          int dst = srp[k];
          const int end = srp[k + 1];
          for (int p = a0; p < a0 + len; ++p) {
            const int q = map[aci[p]];
            if (q >= 0 && dst < end) {      // dst < end always: the count pass ran the same loop
              scol[dst] = q; sval[dst] = av[p];
              if (src) src[dst] = p;
              ++dst;
            }
          }
        }
      } else if (MODE == EXT_COUNT) {
        wave_rows[atomicAdd(&st[ST_WAVE], 1ull)] = k;      // at most nr rows are listed: wave_rows holds nr
      }
    }
    if (MODE == EXT_COUNT) cnt[k] = n;      // a wave row's 0 is replaced by arm (c)'s count
  }
  if (MODE == EXT_COUNT) ext_add_total(n, st);
}

// ------------------------------------------------------------------ arm (c): one wave per output row, four rows per workgroup
template <int MODE>
__global__ __launch_bounds__(TB) void ext_wave_kernel(int n_wave, const int *__restrict__ wave_rows, const int *__restrict__ rows, const int *__restrict__ arp,
                                                      const int *__restrict__ aci, const u64 *__restrict__ av, const int *__restrict__ map, int *__restrict__ cnt,
                                                      u64 *__restrict__ st, const int *__restrict__ srp, int *__restrict__ scol, u64 *__restrict__ sval, int *__restrict__ src) {
  const int w = blockIdx.x * (TB / WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= n_wave) return;                      // the whole wave leaves: the ballots below see full waves only
  const int k = wave_rows[w];
  const int r = rows ? rows[k] : k;
  if (r < 0) return;                            // wave-uniform; cannot happen: only checked rows are listed
  const int a0 = arp[r], len = arp[r + 1] - a0;
  const u64 below = (1ull << lane) - 1ull;
  int dst = 0, cap = 0;
  if (MODE == EXT_FILL) { dst = srp[k]; cap = srp[k + 1] - dst; }
  int carry = 0;
  for (int base = 0; base < len; base += WAVE) {
    const int p = base + lane;
    const int q = p < len ? map[aci[a0 + p]] : -1;
    const u64 flags = __ballot(q >= 0);
    if (MODE == EXT_FILL && q >= 0) {
      const int pos = carry + __popcll(flags & below);
      if (pos < cap) {                          // always: the count pass ran the same loop
        scol[dst + pos] = q; sval[dst + pos] = av[a0 + p];
        if (src) src[dst + pos] = a0 + p;
      }
    }
    carry += __popcll(flags);
  }
  if (MODE == EXT_COUNT && lane == 0) {
    cnt[k] = carry;
    if (carry) atomicAdd(&st[ST_TOTAL], (u64)carry);
  }
}

// ------------------------------------------------------------------ values again, and the vector kernels
__global__ void ext_numeric_kernel(long long nnz, long long a_nnz, const int *__restrict__ src, const u64 *__restrict__ av, u64 *__restrict__ sval) {
  const long long k = (long long)blockIdx.x * TB + threadIdx.x;
  if (k >= nnz) return;
  const int p = src[k];
  if (p >= 0 && p < a_nnz) sval[k] = av[p];      // always: the map was written by the fill pass of a source with a_nnz entries
}
// one kernel for both directions: GATHER y[k] = x[idx[k]] (+0.0 for a refused index), else x[idx[k]] = y[k] (a refused index is skipped)
template <class I, bool GATHER>
__global__ void vec_index_kernel(long long n, long long xn, const I *__restrict__ idx, const u64 *__restrict__ in, u64 *__restrict__ out, u64 *__restrict__ bad) {
  const long long k = (long long)blockIdx.x * TB + threadIdx.x;
  bool refused = false;
  if (k < n) {
    const long long v = (long long)idx[k];
    refused = v < 0 || v >= xn;
    if (GATHER) out[k] = refused ? 0ull : in[v];
    else if (!refused) out[v] = in[k];
  }
  if (bad) {      // kernel argument: the same in every lane
    const u64 f = __ballot(refused);
    if ((threadIdx.x & 63) == 0 && f) atomicAdd(bad, (u64)__popcll(f));
  }
}

long long fetch_index(const void *dev, long long at, int bits) {   // one element of an input index array, for an error message
  long long v64 = 0; int v32 = 0;
  if (bits == 64) { if (hipMemcpy(&v64, (const long long *)dev + at, 8, hipMemcpyDeviceToHost) != hipSuccess) (void)hipGetLastError(); return v64; }
  if (hipMemcpy(&v32, (const int *)dev + at, 4, hipMemcpyDeviceToHost) != hipSuccess) (void)hipGetLastError();
  return v32;
}
int finish(mgs_ctx *ctx, const char *who) {   // launch errors of everything enqueued so far + the stream's completion
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return mgs_fail(ctx, MGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  return MGS_OK;
}

int extract_build(const mgs_csr *A, const void *rows_dev, int nr, const void *cols_dev, int nc, int bits, int keep_map, mgs_extract_plan *pl, mgs_csr **out) {
  mgs_ctx *ctx = A->ctx;
  hipStream_t s = ctx->stream;
  const char *who = "mgs_csr_extract";
  const u64 *av = (const u64 *)A->val;
  DevBuf rows, map, cnt, wave, st;
  if (rows_dev) MGS_TRY(dalloc<int>(ctx, rows, (size_t)nr));
  if (cols_dev) { MGS_TRY(dalloc<int>(ctx, map, (size_t)A->cols)); MGS_TRY(dalloc<int>(ctx, wave, (size_t)nr)); }
  MGS_TRY(dalloc<int>(ctx, cnt, (size_t)nr + 1));
  MGS_TRY(dalloc<u64>(ctx, st, 4));
  const int *rl = rows_dev ? rows.as<int>() : nullptr;
  // 1. lists, 2. column map, 3. entries per output row (arms (a) and (b)), the rows of arm (c)
  u64 h[4] = {NO_ERR, NO_ERR, 0, 0};
  MGS_HIP(ctx, hipMemcpyAsync(st.p, h, sizeof h, hipMemcpyHostToDevice, s));
  MGS_HIP(ctx, hipMemsetAsync(cnt.p, 0, sizeof(int) * ((size_t)nr + 1), s));
  if (cols_dev && A->cols) MGS_HIP(ctx, hipMemsetAsync(map.p, 0xff, sizeof(int) * (size_t)A->cols, s));
  if (rows_dev && nr) {
    if (bits == 64) hipLaunchKernelGGL(ext_rows_kernel<long long>, dim3(mgs_grid(nr, TB)), dim3(TB), 0, s, (long long)nr, A->rows, (const long long *)rows_dev, rows.as<int>(), st.as<u64>());
    else hipLaunchKernelGGL(ext_rows_kernel<int>, dim3(mgs_grid(nr, TB)), dim3(TB), 0, s, (long long)nr, A->rows, (const int *)rows_dev, rows.as<int>(), st.as<u64>());
  }
  if (cols_dev && nc) {
    if (bits == 64) hipLaunchKernelGGL(ext_cols_kernel<long long>, dim3(mgs_grid(nc, TB)), dim3(TB), 0, s, (long long)nc, A->cols, (const long long *)cols_dev, map.as<int>(), st.as<u64>());
    else hipLaunchKernelGGL(ext_cols_kernel<int>, dim3(mgs_grid(nc, TB)), dim3(TB), 0, s, (long long)nc, A->cols, (const int *)cols_dev, map.as<int>(), st.as<u64>());
  }
  if (nr) {
    if (cols_dev) hipLaunchKernelGGL(ext_lane_kernel<EXT_COUNT>, dim3(mgs_grid(nr, TB)), dim3(TB), 0, s, nr, rl, A->rowptr, A->col, av, map.as<int>(), cnt.as<int>(), wave.as<int>(),
                                     st.as<u64>(), nullptr, nullptr, nullptr, nullptr);
    else hipLaunchKernelGGL(ext_len_kernel, dim3(mgs_grid(nr, TB)), dim3(TB), 0, s, nr, rl, A->rowptr, cnt.as<int>(), st.as<u64>());
  }
  MGS_HIP(ctx, hipMemcpyAsync(h, st.p, sizeof h, hipMemcpyDeviceToHost, s));
  MGS_TRY(finish(ctx, who));
  if (h[ST_ROW] != NO_ERR) {
    const long long k = (long long)h[ST_ROW];
    return mgs_fail(ctx, MGS_ERR_INVALID, "%s: row index %lld at position %lld of the row list is outside [0, %d)", who, fetch_index(rows_dev, k, bits), k, A->rows);
  }
  if (h[ST_COL] != NO_ERR) {
    const long long q = (long long)(h[ST_COL] >> 1);
    if ((h[ST_COL] & 1ull) == BAD_RANGE)
      return mgs_fail(ctx, MGS_ERR_INVALID, "%s: column index %lld at position %lld of the column list is outside [0, %d)", who, fetch_index(cols_dev, q, bits), q, A->cols);
    return mgs_fail(ctx, MGS_ERR_INVALID, "%s: the column list is not strictly ascending at position %lld (%lld follows %lld); a general column permutation is not supported", who, q,
                    fetch_index(cols_dev, q, bits), fetch_index(cols_dev, q - 1, bits));
  }
  MGS_CHECK(ctx, h[ST_WAVE] <= (u64)nr, MGS_ERR_HIP, "%s: %llu long rows counted among %d rows", who, h[ST_WAVE], nr);
  const int n_wave = (int)h[ST_WAVE];
  if (n_wave) {
    hipLaunchKernelGGL(ext_wave_kernel<EXT_COUNT>, dim3(mgs_grid(n_wave, TB / WAVE)), dim3(TB), 0, s, n_wave, wave.as<int>(), rl, A->rowptr, A->col, av, map.as<int>(), cnt.as<int>(),
                       st.as<u64>(), nullptr, nullptr, nullptr, nullptr);
    MGS_HIP(ctx, hipMemcpyAsync(h, st.p, sizeof h, hipMemcpyDeviceToHost, s));
    MGS_TRY(finish(ctx, who));
  }
  const u64 total = h[ST_TOTAL];
  MGS_CHECK(ctx, total < 2147483647ull, MGS_ERR_INVALID, "%s: the block holds %llu entries, 2^31 - 1 or more", who, total);
  // 4. scan, 5. columns, values, source positions
  const int64_t nnz = (int64_t)total;
  mgs_csr *S = nullptr;
  MGS_TRY(mgs_csr_alloc(ctx, nr, nc, nnz, &S));
  *out = S;      // the caller destroys it on failure
  MGS_TRY(k_exclusive_scan_i32(ctx, cnt.as<int>(), S->rowptr, (int64_t)nr + 1, nullptr));
  if (keep_map) MGS_TRY(mgs_dev_alloc(ctx, &pl->src, (size_t)nnz));
  if (nr && nnz) {
    if (!cols_dev)
      hipLaunchKernelGGL(ext_rowcopy_kernel, dim3(mgs_grid(nnz, TB)), dim3(TB), 0, s, (long long)nnz, nr, rl, A->rowptr, A->col, av, S->rowptr, S->col, (u64 *)S->val, pl->src);
    else {
      if (nr > n_wave) hipLaunchKernelGGL(ext_lane_kernel<EXT_FILL>, dim3(mgs_grid(nr, TB)), dim3(TB), 0, s, nr, rl, A->rowptr, A->col, av, map.as<int>(), nullptr, nullptr, nullptr,
                                          S->rowptr, S->col, (u64 *)S->val, pl->src);
      if (n_wave) hipLaunchKernelGGL(ext_wave_kernel<EXT_FILL>, dim3(mgs_grid(n_wave, TB / WAVE)), dim3(TB), 0, s, n_wave, wave.as<int>(), rl, A->rowptr, A->col, av, map.as<int>(),
                                     nullptr, nullptr, S->rowptr, S->col, (u64 *)S->val, pl->src);
    }
  }
  MGS_TRY(finish(ctx, who));
  pl->keep = keep_map != 0;
  pl->n_lane = cols_dev ? (int64_t)nr - n_wave : 0; pl->n_wave = cols_dev ? n_wave : 0;
  pl->a_rows = A->rows; pl->a_cols = A->cols; pl->a_nnz = A->nnz;
  return mgs_plan_csr(S);
}

template <bool GATHER>
int vec_index(const mgs_vec *from, const void *idx_dev, int64_t n, int bits, mgs_vec *to, int64_t *bad, const char *who) {
  MGS_CHECK(from ? from->ctx : (to ? to->ctx : nullptr), from && to && (idx_dev || n == 0), MGS_ERR_INVALID, "%s: NULL argument", who);
  mgs_ctx *ctx = from->ctx;
  MGS_CHECK(ctx, to->ctx == ctx, MGS_ERR_INVALID, "%s: the vectors belong to different contexts", who);
  MGS_CHECK(ctx, bits == 32 || bits == 64, MGS_ERR_INVALID, "%s: index_bits %d is neither 32 nor 64", who, bits);
  const mgs_vec *compact = GATHER ? to : from, *full = GATHER ? from : to;      // y and x of include/mgs.h
  MGS_CHECK(ctx, n >= 0 && n <= compact->n, MGS_ERR_INVALID, "%s: n = %lld, y holds %lld entries", who, (long long)n, (long long)compact->n);
  MGS_CHECK(ctx, from->d != to->d || n == 0, MGS_ERR_INVALID, "%s: x and y are the same array", who);
  DevBuf cnt;
  if (bad) {
    MGS_TRY(dalloc<u64>(ctx, cnt, 1));
    MGS_HIP(ctx, hipMemsetAsync(cnt.p, 0, sizeof(u64), ctx->stream));
  }
  if (n) {
    const dim3 grid(mgs_grid(n, TB)), block(TB);
    if (bits == 64) hipLaunchKernelGGL((vec_index_kernel<long long, GATHER>), grid, block, 0, ctx->stream, (long long)n, (long long)full->n, (const long long *)idx_dev, (const u64 *)from->d,
                                       (u64 *)to->d, cnt.as<u64>());
    else hipLaunchKernelGGL((vec_index_kernel<int, GATHER>), grid, block, 0, ctx->stream, (long long)n, (long long)full->n, (const int *)idx_dev, (const u64 *)from->d, (u64 *)to->d,
                            cnt.as<u64>());
  }
  MGS_HIP(ctx, hipGetLastError());
  if (!bad) return MGS_OK;
  u64 hb = 0;
  MGS_HIP(ctx, hipMemcpyAsync(&hb, cnt.p, sizeof hb, hipMemcpyDeviceToHost, ctx->stream));
  MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *bad = (int64_t)hb;
  MGS_CHECK(ctx, hb == 0, MGS_ERR_INVALID, "%s: %llu of %lld indices are outside [0, %lld) (%s)", who, hb, (long long)n, (long long)full->n,
            GATHER ? "y holds +0.0 there" : "they were skipped");
  return MGS_OK;
}

}  // namespace

int k_csr_extract(const mgs_csr *A, const void *rows_dev, int64_t nr, const void *cols_dev, int64_t nc, int index_bits, int keep_map, mgs_csr **out) {
  const char *who = "mgs_csr_extract";
  MGS_CHECK(A ? A->ctx : nullptr, A && out, MGS_ERR_INVALID, "%s: NULL argument", who);
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, index_bits == 32 || index_bits == 64, MGS_ERR_INVALID, "%s: index_bits %d is neither 32 nor 64", who, index_bits);
  if (!rows_dev) nr = A->rows;
  if (!cols_dev) nc = A->cols;
  MGS_CHECK(ctx, nr >= 0 && nc >= 0, MGS_ERR_INVALID, "%s: negative list length (nr = %lld, nc = %lld)", who, (long long)nr, (long long)nc);
  MGS_CHECK(ctx, nr < 2147483647LL && nc < 2147483647LL, MGS_ERR_INVALID, "%s: a list of 2^31 - 1 entries or more (nr = %lld, nc = %lld)", who, (long long)nr, (long long)nc);
  MGS_CHECK(ctx, !mgs_csr_is_shard(A), MGS_ERR_INVALID, "%s: A is a row shard (%d rows, %d columns with halo columns): blocks of row shards are not supported", who, A->rows,
            A->cols);
  mgs_extract_plan *pl = new mgs_extract_plan();
  mgs_csr *S = nullptr;
  const int rc = extract_build(A, rows_dev, (int)nr, cols_dev, (int)nc, index_bits, keep_map, pl, &S);
  if (rc != MGS_OK) {
    hipStreamSynchronize(ctx->stream);
    mgs_csr_destroy(S); mgs_free_extract(pl);
    return rc;
  }
  S->extp = pl;
  *out = S;
  return MGS_OK;
}

int k_csr_extract_numeric(const mgs_csr *A, mgs_csr *S) {
  const char *who = "mgs_csr_extract_numeric";
  MGS_CHECK(A ? A->ctx : (S ? S->ctx : nullptr), A && S, MGS_ERR_INVALID, "%s: NULL argument", who);
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, S->ctx == ctx, MGS_ERR_INVALID, "%s: S belongs to a different context", who);
  const mgs_extract_plan *pl = S->extp;
  MGS_CHECK(ctx, pl && pl->keep, MGS_ERR_STATE, "%s: S keeps no source map (mgs_csr_extract with keep_map != 0 does)", who);
  MGS_CHECK(ctx, A->rows == pl->a_rows && A->cols == pl->a_cols && A->nnz == pl->a_nnz, MGS_ERR_INVALID, "%s: A is %d x %d with %lld entries, S was taken from %d x %d with %lld", who,
            A->rows, A->cols, (long long)A->nnz, pl->a_rows, pl->a_cols, (long long)pl->a_nnz);
  MGS_CHECK(ctx, !(S->code && S->code->vtab), MGS_ERR_INVALID, "%s: S carries a value-carrying pattern code (option valcode): extract the block again instead", who);
  if (S->nnz) hipLaunchKernelGGL(ext_numeric_kernel, dim3(mgs_grid(S->nnz, TB)), dim3(TB), 0, ctx->stream, (long long)S->nnz, (long long)A->nnz, pl->src, (const u64 *)A->val, (u64 *)S->val);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

int k_csr_extract_info(const mgs_csr *S, int64_t out[4]) {
  MGS_CHECK(nullptr, S && out, MGS_ERR_INVALID, "mgs_csr_extract_info: NULL argument");
  out[0] = out[1] = out[2] = out[3] = 0;
  if (!S->extp) return MGS_OK;
  out[0] = S->extp->n_lane; out[1] = S->extp->n_wave; out[2] = S->max_row_len; out[3] = S->extp->keep ? 4 * S->nnz : 0;
  return MGS_OK;
}

int k_vec_gather(const mgs_vec *x, const void *idx_dev, int64_t n, int index_bits, mgs_vec *y, int64_t *bad) {
  return vec_index<true>(x, idx_dev, n, index_bits, y, bad, "mgs_vec_gather");
}
int k_vec_scatter(const mgs_vec *y, const void *idx_dev, int64_t n, int index_bits, mgs_vec *x, int64_t *bad) {
  return vec_index<false>(y, idx_dev, n, index_bits, x, bad, "mgs_vec_scatter");
}
