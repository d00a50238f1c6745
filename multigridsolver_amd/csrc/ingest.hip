// ingest.hip — matrices that already live in device memory enter the library here, without a host round trip of the data:
//   * k_csr_from_device: CSR arrays with 32- or 64-bit indices.  The acceptance rules of mgs_csr_upload (rowptr ends, monotone
//     rowptr, columns in range and strictly ascending inside a row) are checked on the device in the same passes that copy and
//     narrow the arrays; the lowest violation in the order of mgs_csr_upload's host loop comes back through one 64-bit word.
//   * k_csr_from_coo_device: triples in any order, duplicates summed in input order — what readMatrix does on the host
//     (src/common/MatrixIO.cpp:12-37: bucket by row, sort each row), on the device: count per row, scan, scatter the keys
//     (col << 32 | k) into row buckets, sort every bucket (one lane per short row, one workgroup with a bitonic sort in LDS per
//     long row), flag run heads, scan, write rowptr / col, gather the values run by run.  The keys are distinct, so the sorted
//     order — and with it every sum — does not depend on how the scatter's atomics were scheduled.
//   * k_csr_update_values_coo: the same gather kernel on new triple values through the kept map.
// No kernel uses an input index as an address before it has compared it with its bounds as a 64-bit value.
#include "mgs_internal.hpp"

#include <algorithm>

namespace {
constexpr int TB = 256;
constexpr int RB = 256;          // rows per workgroup of the column pass (its rowptr slice sits in LDS)
constexpr int COO_SHORT = 32;    // rows of at most this many triples are sorted by one lane, longer ones by one workgroup in LDS
constexpr unsigned long long NO_ERR = ~0ull;
enum { BAD_ENDS = 0, BAD_MONOTONE = 1, BAD_RANGE = 2, BAD_ASCENDING = 3 };   // in the order mgs_csr_upload meets them inside one row
// (row, entry, kind) of a CSR violation: atomicMin keeps the one the host loop of mgs_csr_upload would have met first
__device__ __forceinline__ unsigned long long csr_err(long long row, long long k, int kind) {
  return ((unsigned long long)row << 33) | ((unsigned long long)k << 2) | (unsigned long long)kind;
}

struct DevBuf {  // RAII for temporaries
  void *p = nullptr;
  ~DevBuf() { if (p) mgs_hip_free(p); }
  template <class T> T *as() { return (T *)p; }
};
template <class T>
int dalloc(mgs_ctx *ctx, DevBuf &b, size_t count) { T *q = nullptr; MGS_TRY(mgs_dev_alloc(ctx, &q, count)); b.p = q; return MGS_OK; }

// ------------------------------------------------------------------ CSR: check + narrow
// rowptr: ends, monotone; the narrowed copy is clamped to [0, nnz] so the column pass may address with it whatever the input held
template <class I>
__global__ void csr_rowptr_kernel(int rows, long long nnz, const I *__restrict__ rp, int *__restrict__ out, unsigned long long *__restrict__ err) {
  const long long i = (long long)blockIdx.x * TB + threadIdx.x;
  if (i > rows) return;
  const long long v = (long long)rp[i];
  if ((i == 0 && v != 0) || (i == rows && v != nnz)) atomicMin(err, csr_err(0, 0, BAD_ENDS));
  if (i < rows && v > (long long)rp[i + 1]) atomicMin(err, csr_err(i, 0, BAD_MONOTONE));
  out[i] = (int)(v < 0 ? 0 : v > nnz ? nnz : v);
}
// columns of RB rows per workgroup: entries in coalesced order, each entry's row by bisection of the rowptr slice in LDS
template <class I>
__global__ __launch_bounds__(TB) void csr_cols_kernel(int rows, int cols, const int *__restrict__ rp, const I *__restrict__ col, int *__restrict__ col_out,
                                                      unsigned long long *__restrict__ err) {
  __shared__ int sh[RB + 1];
  const int b0 = blockIdx.x * RB, nr = rows - b0 < RB ? rows - b0 : RB;
  for (int t = threadIdx.x; t <= nr; t += TB) sh[t] = rp[b0 + t];
  __syncthreads();
  const int lo = sh[0], hi = sh[nr];
  for (long long k = (long long)lo + threadIdx.x; k < hi; k += TB) {
    const long long c = (long long)col[k];
    int a = 0, b = nr - 1;                       // first row r of the slice with sh[r + 1] > k
    while (a < b) { const int m = (a + b) >> 1; if (sh[m + 1] > k) b = m; else a = m + 1; }
    const bool out_of_range = c < 0 || c >= cols;
    if (out_of_range) atomicMin(err, csr_err(b0 + a, k, BAD_RANGE));
    else if (k > sh[a] && (long long)col[k - 1] >= c) atomicMin(err, csr_err(b0 + a, k, BAD_ASCENDING));   // never across a row boundary
    col_out[k] = out_of_range ? 0 : (int)c;
  }
}

// ------------------------------------------------------------------ COO assembly
// st[0] lowest bad triple (k << 1 | 0: row, 1: column), st[1] most triples in a row, st[2] lowest row above MGS_COO_MAX_ROW, st[3] long rows listed
template <class I>
__global__ void coo_count_kernel(long long n, int rows, int cols, const I *__restrict__ row, const I *__restrict__ col, int *__restrict__ cnt,
                                 unsigned long long *__restrict__ st) {
  const long long k = (long long)blockIdx.x * TB + threadIdx.x;
  if (k >= n) return;
  const long long r = (long long)row[k], c = (long long)col[k];
  if (r < 0 || r >= rows) atomicMin(&st[0], (unsigned long long)k << 1);
  else if (c < 0 || c >= cols) atomicMin(&st[0], ((unsigned long long)k << 1) | 1ull);
  else atomicAdd(&cnt[r], 1);
}
__global__ void coo_class_kernel(int rows, const int *__restrict__ bptr, unsigned long long *__restrict__ st, int *__restrict__ longrows, int cap) {
  const int i = blockIdx.x * TB + threadIdx.x;
  const int len = i < rows ? bptr[i + 1] - bptr[i] : 0;
  int mx = len;
  for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(mx, off); mx = o > mx ? o : mx; }
  if ((threadIdx.x & 63) == 0 && mx > 0) atomicMax(&st[1], (unsigned long long)mx);
  if (len > MGS_COO_MAX_ROW) atomicMin(&st[2], (unsigned long long)i);
  else if (len > COO_SHORT) { const unsigned long long q = atomicAdd(&st[3], 1ull); if (q < (unsigned long long)cap) longrows[q] = i; }
}
// keys (col << 32 | k) into the row buckets; the indices are compared with their bounds again (the arrays are the caller's) and a
// bucket never takes more keys than were counted for it
template <class I>
__global__ void coo_scatter_kernel(long long n, int rows, int cols, const I *__restrict__ row, const I *__restrict__ col, const int *__restrict__ bptr,
                                   int *__restrict__ cursor, unsigned long long *__restrict__ keys) {
  const long long k = (long long)blockIdx.x * TB + threadIdx.x;
  if (k >= n) return;
  const long long r = (long long)row[k], c = (long long)col[k];
  if (r < 0 || r >= rows || c < 0 || c >= cols) return;
  const int lo = bptr[r], len = bptr[r + 1] - lo, q = atomicAdd(&cursor[r], 1);
  if (q < len) keys[(long long)lo + q] = ((unsigned long long)c << 32) | (unsigned long long)k;
}
__global__ void coo_sort_short_kernel(int rows, const int *__restrict__ bptr, unsigned long long *__restrict__ keys) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= rows) return;
  const int lo = bptr[i], hi = bptr[i + 1];
  if (hi - lo > COO_SHORT) return;
  for (int a = lo + 1; a < hi; ++a) {
    const unsigned long long k = keys[a];
    int b = a - 1;
    while (b >= lo && keys[b] > k) { keys[b + 1] = keys[b]; --b; }
    keys[b + 1] = k;
  }
}
// one workgroup per long row: bitonic sort in LDS, the row padded to the next power of two with keys above every real one
__global__ __launch_bounds__(TB) void coo_sort_long_kernel(const int *__restrict__ longrows, const int *__restrict__ bptr, unsigned long long *__restrict__ keys, int cap2) {
  extern __shared__ unsigned long long sk[];
  const int i = longrows[blockIdx.x], lo = bptr[i], len = bptr[i + 1] - lo;
  int n2 = 64;
  while (n2 < len) n2 <<= 1;
  if (n2 > cap2) return;                          // cannot happen: cap2 is sized from the longest row
  for (int t = threadIdx.x; t < n2; t += TB) sk[t] = t < len ? keys[(long long)lo + t] : NO_ERR;
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (n2 >> 1); t += TB) {
        const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
        const unsigned long long x = sk[a], y = sk[b];
        if ((x > y) == ((a & k) == 0)) { sk[a] = y; sk[b] = x; }
      }
      __syncthreads();
    }
  for (int t = threadIdx.x; t < len; t += TB) keys[(long long)lo + t] = sk[t];
}
// run heads: the first key of a row, and every key whose column differs from its predecessor's
__global__ void coo_rowstart_kernel(int rows, const int *__restrict__ bptr, int *__restrict__ flag) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i < rows && bptr[i] < bptr[i + 1]) flag[bptr[i]] = 1;
}
__global__ void coo_colchange_kernel(long long n, const unsigned long long *__restrict__ keys, int *__restrict__ flag) {
  const long long p = (long long)blockIdx.x * TB + threadIdx.x;
  if (p >= 1 && p < n && (keys[p] >> 32) != (keys[p - 1] >> 32)) flag[p] = 1;
}
__global__ void coo_rowptr_kernel(int rows, const int *__restrict__ bptr, const int *__restrict__ epos, int *__restrict__ rowptr) {
  const long long i = (long long)blockIdx.x * TB + threadIdx.x;
  if (i <= rows) rowptr[i] = epos[bptr[i]];
}
// epos: exclusive scan of the head flags (n + 1 entries): key p opens entry epos[p] iff epos[p + 1] > epos[p]
__global__ void coo_write_kernel(long long n, const unsigned long long *__restrict__ keys, const int *__restrict__ epos, int *__restrict__ col,
                                 int *__restrict__ run, int *__restrict__ src) {
  const long long p = (long long)blockIdx.x * TB + threadIdx.x;
  if (p >= n) return;
  const unsigned long long key = keys[p];
  src[p] = (int)(key & 0xffffffffull);
  const int e = epos[p], e1 = epos[p + 1];
  if (e1 > e) { col[e] = (int)(key >> 32); run[e] = (int)p; }
  if (p == n - 1) run[e1] = (int)n;
}
// one output entry = its run of source positions summed in input order, starting from the first value itself
__global__ void coo_gather_kernel(long long nnz, const int *__restrict__ run, const int *__restrict__ src, const double *__restrict__ val_in, double *__restrict__ val) {
  const long long e = (long long)blockIdx.x * TB + threadIdx.x;
  if (e >= nnz) return;
  const int lo = run[e], hi = run[e + 1];
  double s = val_in[src[lo]];
  for (int q = lo + 1; q < hi; ++q) s += val_in[src[q]];
  val[e] = s;
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

template <class I>
int csr_from_device_t(mgs_ctx *ctx, mgs_csr *A, const I *rowptr, const I *col, const double *val, unsigned long long *err_dev, unsigned long long *err_host) {
  hipStream_t s = ctx->stream;
  const int rows = A->rows;
  MGS_HIP(ctx, hipMemcpyAsync(err_dev, err_host, sizeof(unsigned long long), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(csr_rowptr_kernel<I>, dim3(mgs_grid((int64_t)rows + 1, TB)), dim3(TB), 0, s, rows, (long long)A->nnz, rowptr, A->rowptr, err_dev);
  if (rows && A->nnz) hipLaunchKernelGGL(csr_cols_kernel<I>, dim3(mgs_grid(rows, RB)), dim3(TB), 0, s, rows, A->cols, A->rowptr, col, A->col, err_dev);
  if (A->nnz) MGS_HIP(ctx, hipMemcpyAsync(A->val, val, sizeof(double) * (size_t)A->nnz, hipMemcpyDeviceToDevice, s));
  MGS_HIP(ctx, hipMemcpyAsync(err_host, err_dev, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  return finish(ctx, "mgs_csr_from_device");
}

}  // namespace

int k_csr_from_device(mgs_ctx *ctx, int rows, int cols, int64_t nnz, const void *rowptr_dev, const void *col_dev, int index_bits, const void *val_dev, mgs_csr **out) {
  MGS_CHECK(ctx, ctx && out && rowptr_dev && (nnz == 0 || (col_dev && val_dev)), MGS_ERR_INVALID, "mgs_csr_from_device: NULL argument");
  MGS_CHECK(ctx, index_bits == 32 || index_bits == 64, MGS_ERR_INVALID, "mgs_csr_from_device: index_bits %d is neither 32 nor 64", index_bits);
  MGS_CHECK(ctx, rows >= 0 && cols >= 0 && nnz >= 0 && nnz < 2147483647LL, MGS_ERR_INVALID, "mgs_csr_from_device: bad shape %d x %d nnz %lld", rows, cols, (long long)nnz);
  mgs_csr *A = nullptr;
  MGS_TRY(mgs_csr_alloc(ctx, rows, cols, nnz, &A));
  DevBuf err;
  unsigned long long w = NO_ERR;
  int rc = dalloc<unsigned long long>(ctx, err, 1);
  if (rc == MGS_OK)
    rc = index_bits == 64 ? csr_from_device_t<long long>(ctx, A, (const long long *)rowptr_dev, (const long long *)col_dev, (const double *)val_dev, err.as<unsigned long long>(), &w)
                          : csr_from_device_t<int>(ctx, A, (const int *)rowptr_dev, (const int *)col_dev, (const double *)val_dev, err.as<unsigned long long>(), &w);
  if (rc == MGS_OK && w != NO_ERR) {
    const int row = (int)(w >> 33), kind = (int)(w & 3ull);
    const long long k = (long long)((w >> 2) & 0x7fffffffull);
    if (kind == BAD_ENDS)
      rc = mgs_fail(ctx, MGS_ERR_INVALID, "mgs_csr_from_device: rowptr[0]=%lld rowptr[rows]=%lld nnz=%lld inconsistent", fetch_index(rowptr_dev, 0, index_bits),
                    fetch_index(rowptr_dev, rows, index_bits), (long long)nnz);
    else if (kind == BAD_MONOTONE) rc = mgs_fail(ctx, MGS_ERR_INVALID, "mgs_csr_from_device: rowptr not monotone at row %d", row);
    else if (kind == BAD_RANGE) rc = mgs_fail(ctx, MGS_ERR_INVALID, "mgs_csr_from_device: column %lld out of range in row %d", fetch_index(col_dev, k, index_bits), row);
    else rc = mgs_fail(ctx, MGS_ERR_INVALID, "mgs_csr_from_device: columns of row %d not strictly ascending", row);
  }
  if (rc == MGS_OK) rc = mgs_plan_csr(A);
  if (rc != MGS_OK) { mgs_csr_destroy(A); return rc; }
  *out = A;
  return MGS_OK;
}

int k_csr_from_coo_device(mgs_ctx *ctx, int rows, int cols, int64_t ntrip, const void *row_dev, const void *col_dev, int index_bits, const void *val_dev, int keep_map,
                          mgs_csr **out) {
  MGS_CHECK(ctx, ctx && out && (ntrip == 0 || (row_dev && col_dev && val_dev)), MGS_ERR_INVALID, "mgs_csr_from_coo_device: NULL argument");
  MGS_CHECK(ctx, index_bits == 32 || index_bits == 64, MGS_ERR_INVALID, "mgs_csr_from_coo_device: index_bits %d is neither 32 nor 64", index_bits);
  MGS_CHECK(ctx, rows >= 0 && cols >= 0 && ntrip >= 0 && ntrip < 2147483647LL, MGS_ERR_INVALID, "mgs_csr_from_coo_device: bad shape %d x %d, %lld triples", rows, cols,
            (long long)ntrip);
  hipStream_t s = ctx->stream;
  const size_t n = (size_t)ntrip;
  DevBuf cnt, bptr, st, longrows, keys, flag, src, run;
  MGS_TRY(dalloc<int>(ctx, cnt, (size_t)rows + 1));
  MGS_TRY(dalloc<int>(ctx, bptr, (size_t)rows + 1));
  MGS_TRY(dalloc<unsigned long long>(ctx, st, 4));
  const int long_cap = (int)std::min<int64_t>(rows, ntrip / (COO_SHORT + 1)) + 1;
  MGS_TRY(dalloc<int>(ctx, longrows, (size_t)long_cap));
  // 1. range check + triples per row, 2. bucket offsets, row-length classes
  unsigned long long h[4] = {NO_ERR, 0, NO_ERR, 0};
  MGS_HIP(ctx, hipMemcpyAsync(st.p, h, sizeof h, hipMemcpyHostToDevice, s));
  MGS_HIP(ctx, hipMemsetAsync(cnt.p, 0, sizeof(int) * ((size_t)rows + 1), s));
  if (ntrip) {
    if (index_bits == 64)
      hipLaunchKernelGGL(coo_count_kernel<long long>, dim3(mgs_grid(ntrip, TB)), dim3(TB), 0, s, (long long)ntrip, rows, cols, (const long long *)row_dev, (const long long *)col_dev,
                         cnt.as<int>(), st.as<unsigned long long>());
    else
      hipLaunchKernelGGL(coo_count_kernel<int>, dim3(mgs_grid(ntrip, TB)), dim3(TB), 0, s, (long long)ntrip, rows, cols, (const int *)row_dev, (const int *)col_dev, cnt.as<int>(),
                         st.as<unsigned long long>());
  }
  MGS_TRY(k_exclusive_scan_i32(ctx, cnt.as<int>(), bptr.as<int>(), (int64_t)rows + 1, nullptr));
  if (rows) hipLaunchKernelGGL(coo_class_kernel, dim3(mgs_grid(rows, TB)), dim3(TB), 0, s, rows, bptr.as<int>(), st.as<unsigned long long>(), longrows.as<int>(), long_cap);
  MGS_HIP(ctx, hipMemcpyAsync(h, st.p, sizeof h, hipMemcpyDeviceToHost, s));
  MGS_TRY(finish(ctx, "mgs_csr_from_coo_device"));
  if (h[0] != NO_ERR) {
    const long long k = (long long)(h[0] >> 1);
    if (h[0] & 1ull) return mgs_fail(ctx, MGS_ERR_INVALID, "mgs_csr_from_coo_device: column %lld of triple %lld out of range [0,%d)", fetch_index(col_dev, k, index_bits), k, cols);
    return mgs_fail(ctx, MGS_ERR_INVALID, "mgs_csr_from_coo_device: row %lld of triple %lld out of range [0,%d)", fetch_index(row_dev, k, index_bits), k, rows);
  }
  MGS_CHECK(ctx, h[2] == NO_ERR, MGS_ERR_INVALID, "mgs_csr_from_coo_device: row %lld receives more than MGS_COO_MAX_ROW = %d triples (the longest row holds %lld)",
            (long long)h[2], MGS_COO_MAX_ROW, (long long)h[1]);
  const int max_row = (int)h[1], nlong = (int)h[3];
  MGS_CHECK(ctx, nlong <= long_cap, MGS_ERR_HIP, "mgs_csr_from_coo_device: %d long rows counted, room for %d", nlong, long_cap);
  // 3. keys into the buckets, 4. every bucket sorted
  MGS_TRY(dalloc<unsigned long long>(ctx, keys, n));
  MGS_TRY(dalloc<int>(ctx, flag, n + 1));
  MGS_HIP(ctx, hipMemsetAsync(cnt.p, 0, sizeof(int) * ((size_t)rows + 1), s));
  MGS_HIP(ctx, hipMemsetAsync(flag.p, 0, sizeof(int) * (n + 1), s));
  if (ntrip) {
    if (index_bits == 64)
      hipLaunchKernelGGL(coo_scatter_kernel<long long>, dim3(mgs_grid(ntrip, TB)), dim3(TB), 0, s, (long long)ntrip, rows, cols, (const long long *)row_dev, (const long long *)col_dev,
                         bptr.as<int>(), cnt.as<int>(), keys.as<unsigned long long>());
    else
      hipLaunchKernelGGL(coo_scatter_kernel<int>, dim3(mgs_grid(ntrip, TB)), dim3(TB), 0, s, (long long)ntrip, rows, cols, (const int *)row_dev, (const int *)col_dev, bptr.as<int>(),
                         cnt.as<int>(), keys.as<unsigned long long>());
    hipLaunchKernelGGL(coo_sort_short_kernel, dim3(mgs_grid(rows, TB)), dim3(TB), 0, s, rows, bptr.as<int>(), keys.as<unsigned long long>());
    if (nlong) {
      int cap2 = 64;
      while (cap2 < max_row) cap2 <<= 1;
      hipLaunchKernelGGL(coo_sort_long_kernel, dim3(nlong), dim3(TB), sizeof(unsigned long long) * (size_t)cap2, s, longrows.as<int>(), bptr.as<int>(), keys.as<unsigned long long>(), cap2);
    }
    // 5. run heads and their scan: entry of every key, entries in all
    hipLaunchKernelGGL(coo_rowstart_kernel, dim3(mgs_grid(rows, TB)), dim3(TB), 0, s, rows, bptr.as<int>(), flag.as<int>());
    hipLaunchKernelGGL(coo_colchange_kernel, dim3(mgs_grid(ntrip, TB)), dim3(TB), 0, s, (long long)ntrip, keys.as<unsigned long long>(), flag.as<int>());
  }
  int64_t nnz = 0;
  MGS_TRY(k_exclusive_scan_i32(ctx, flag.as<int>(), flag.as<int>(), (int64_t)ntrip + 1, &nnz));
  MGS_TRY(finish(ctx, "mgs_csr_from_coo_device"));
  // 6. rowptr, col, the map, and the values through the map
  mgs_csr *A = nullptr;
  MGS_TRY(mgs_csr_alloc(ctx, rows, cols, nnz, &A));
  int rc = dalloc<int>(ctx, src, n);
  if (rc == MGS_OK) rc = dalloc<int>(ctx, run, (size_t)nnz + 1);
  if (rc == MGS_OK) {
    hipLaunchKernelGGL(coo_rowptr_kernel, dim3(mgs_grid((int64_t)rows + 1, TB)), dim3(TB), 0, s, rows, bptr.as<int>(), flag.as<int>(), A->rowptr);
    if (ntrip) {
      hipLaunchKernelGGL(coo_write_kernel, dim3(mgs_grid(ntrip, TB)), dim3(TB), 0, s, (long long)ntrip, keys.as<unsigned long long>(), flag.as<int>(), A->col, run.as<int>(), src.as<int>());
      hipLaunchKernelGGL(coo_gather_kernel, dim3(mgs_grid(nnz, TB)), dim3(TB), 0, s, (long long)nnz, run.as<int>(), src.as<int>(), (const double *)val_dev, A->val);
    }
    rc = finish(ctx, "mgs_csr_from_coo_device");
  }
  if (rc == MGS_OK) rc = mgs_plan_csr(A);
  if (rc != MGS_OK) { mgs_csr_destroy(A); return rc; }
  A->coo_max_row = max_row;
  if (keep_map) { A->coo_src = src.as<int>(); A->coo_run = run.as<int>(); A->coo_ntrip = ntrip; A->coo_map = true; src.p = run.p = nullptr; }
  *out = A;
  return MGS_OK;
}

// new triple values through the kept map, into A's existing val array (enqueued, not synchronised): the kernel of the assembly itself
int k_csr_update_values_coo(mgs_csr *A, const void *val_dev) {
  mgs_ctx *ctx = A->ctx;
  if (A->nnz) hipLaunchKernelGGL(coo_gather_kernel, dim3(mgs_grid(A->nnz, TB)), dim3(TB), 0, ctx->stream, (long long)A->nnz, A->coo_run, A->coo_src, (const double *)val_dev, A->val);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

// ------------------------------------------------------------------ null-space labels (mgs_csr_set_nullspace_fields): check + narrow + count
// A label is compared with its bounds as a 64-bit value before it is narrowed (2³² does not alias 0); the lowest offending row comes back through
// one 64-bit atomicMin word; a refused label is narrowed to −1.  Rows per field: one integer atomicAdd per wave and field (the result does not
// depend on how they were scheduled).
namespace {
template <class I>
__global__ __launch_bounds__(TB) void labels_kernel(long long rows, int nf, const I *__restrict__ in, signed char *__restrict__ out, unsigned long long *__restrict__ st /* [0] bad row, [1 + f] rows of f */) {
  const long long i = (long long)blockIdx.x * TB + threadIdx.x;
  long long v = -1;
  if (i < rows) {
    v = (long long)in[i];
    if (v < -1 || v >= nf) { atomicMin(&st[0], (unsigned long long)i); v = -1; }
    out[i] = (signed char)v;
  }
  for (int f = 0; f < nf; ++f) {
    const unsigned long long m = __ballot(v == f);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&st[1 + f], (unsigned long long)__popcll(m));
  }
}
}   // namespace
int k_labels_from_device(mgs_ctx *ctx, int64_t rows, const void *labels_dev, int index_bits, int nfields, signed char **lab_out, int64_t *counts, int64_t *bad_row, long long *bad_val) {
  hipStream_t s = ctx->stream;
  DevBuf st, lab;
  unsigned long long h[1 + MGS_NULLSPACE_MAX_FIELDS];
  MGS_TRY(dalloc<unsigned long long>(ctx, st, 1 + MGS_NULLSPACE_MAX_FIELDS));
  MGS_TRY(dalloc<signed char>(ctx, lab, (size_t)rows + 2));
  MGS_HIP(ctx, hipMemsetAsync(st.p, 0, sizeof h, s));
  MGS_HIP(ctx, hipMemsetAsync(st.p, 0xff, sizeof(unsigned long long), s));
  if (rows) {
    if (index_bits == 64) hipLaunchKernelGGL(labels_kernel<long long>, dim3(mgs_grid(rows, TB)), dim3(TB), 0, s, (long long)rows, nfields, (const long long *)labels_dev, lab.as<signed char>(), st.as<unsigned long long>());
    else hipLaunchKernelGGL(labels_kernel<int>, dim3(mgs_grid(rows, TB)), dim3(TB), 0, s, (long long)rows, nfields, (const int *)labels_dev, lab.as<signed char>(), st.as<unsigned long long>());
  }
  MGS_HIP(ctx, hipGetLastError());
  MGS_HIP(ctx, hipMemcpyAsync(h, st.p, sizeof h, hipMemcpyDeviceToHost, s));
  MGS_HIP(ctx, hipStreamSynchronize(s));
  *bad_row = -1; *bad_val = 0;
  if (h[0] != NO_ERR) {
    *bad_row = (int64_t)h[0];
    if (index_bits == 64) { long long v = 0; MGS_HIP(ctx, hipMemcpy(&v, (const long long *)labels_dev + h[0], sizeof v, hipMemcpyDeviceToHost)); *bad_val = v; }
    else { int v = 0; MGS_HIP(ctx, hipMemcpy(&v, (const int *)labels_dev + h[0], sizeof v, hipMemcpyDeviceToHost)); *bad_val = v; }
    return MGS_OK;
  }
  for (int f = 0; f < MGS_NULLSPACE_MAX_FIELDS; ++f) counts[f] = (int64_t)h[1 + f];
  *lab_out = lab.as<signed char>(); lab.p = nullptr;
  return MGS_OK;
}
