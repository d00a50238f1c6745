// spgemm.hip — C = A·B for two device CSR matrices (mgs_csr_spgemm), the values of C again for an unchanged pattern
// (mgs_csr_spgemm_numeric), and through them the general Galerkin product (Pᵀ·A)·P of a prolongation that is not an aggregation
// (k_galerkin_general; reference: the Eigen products `Ptrans * A * P`, bicg.cpp:32-33).
//
// Arithmetic (include/mgs.h states it as the contract): row i of C visits the entries (i, l) of A in storage order and for each the
// entries (l, j) of B in storage order; every product a_il·b_lj is rounded once (the build is -ffp-contract=off); the first product
// that reaches column j is stored, every later one is added to it in the order met.  The accumulators start at −0.0, and
// −0.0 + v == v for every v, signed zeros included — that IS "the first is stored, later ones are added" (galerkin_numeric_kernel).
//
// Phases: product counts per row (ub_i = Σ_l len(B_l)) → count of distinct columns per row → scan → sorted columns → values.  The
// values are a launch of their own, so mgs_csr_spgemm_numeric is that launch alone.  Rows are binned by ub:
//   * ub ≤ 64: one lane per row.  Sorted column slots (and, in the numeric pass, accumulators) in [slot][lane] LDS, 16 / 32 / 64
//     slots per lane as in galerkin_core; a row never needs more slots than products, so nothing spills.  Sequential by construction.
//   * ub > 64: one workgroup per row.  A's entries one after the other, B's row across the lanes; B's columns are strictly ascending
//     inside a row, so no two lanes touch one accumulator in a step, and a barrier between the steps keeps the order met.  Symbolic:
//     a key-only hash table of 16384 slots in 64 KB of LDS (load ≤ ½ at MGS_SPGEMM_MAX_ROW = 8192 distinct columns), then an LDS
//     bitonic sort (ingest.hip's) emits the ascending columns.  Numeric: straight into the row's segment of C->val, position by
//     binary search in the row's sorted columns (staged in LDS).
// A column index is hashed and compared, never used as an address; the only atomics are on hash keys and counters, never on values:
// two identical calls give identical bits.
#include "mgs_internal.hpp"

#include <climits>

struct mgs_spgemm_plan {
  int *ub = nullptr;        // rows: product count of every row (clamped to INT_MAX), the bin key
  int *wg_rows = nullptr;   // n_wg: rows with ub > SPG_LANE_UB, one workgroup each
  int *miss = nullptr;      // device counter of mgs_csr_spgemm_numeric
  int n_wg = 0;
  int64_t n_lane = 0, max_ub = 0;
};
void mgs_free_spgemm(mgs_spgemm_plan *p) {
  if (!p) return;
  if (p->ub) mgs_hip_free(p->ub);
  if (p->wg_rows) mgs_hip_free(p->wg_rows);
  if (p->miss) mgs_hip_free(p->miss);
  delete p;
}

namespace {
constexpr int TB = 256;
constexpr int SPG_LANE_UB = 64;       // rows of at most this many products: one lane per row
constexpr int SPG_HASH = 16384;       // key slots of the workgroup path's table (64 KB)
constexpr int SPG_EMPTY = -1;

struct DevBuf {  // RAII for temporaries
  void *p = nullptr;
  ~DevBuf() { if (p) mgs_hip_free(p); }
  template <class T> T *as() { return (T *)p; }
};
template <class T>
int dalloc(mgs_ctx *ctx, DevBuf &b, size_t count) { T *q = nullptr; MGS_TRY(mgs_dev_alloc(ctx, &q, count)); b.p = q; return MGS_OK; }

// st[0] largest ub of a lane row, st[1] workgroup rows listed, st[2] largest ub (clamped), st[3] lowest row above MGS_SPGEMM_MAX_ROW
__global__ void spgemm_ub_kernel(int m, const int *__restrict__ arp, const int *__restrict__ aci, const int *__restrict__ brp, int *__restrict__ ub,
                                 int *__restrict__ wg_rows, int *__restrict__ st) {
  const int i = blockIdx.x * TB + threadIdx.x;
  long long s = 0;
  if (i < m) for (int k = arp[i]; k < arp[i + 1]; ++k) { const int l = aci[k]; s += brp[l + 1] - brp[l]; }
  const int u = s > INT_MAX ? INT_MAX : (int)s;
  if (i < m) {
    ub[i] = u;
    if (u > SPG_LANE_UB) wg_rows[atomicAdd(&st[1], 1)] = i;      // at most m rows are listed: wg_rows holds m
  }
  int ml = u <= SPG_LANE_UB ? u : 0, mx = u;
  for (int off = 32; off > 0; off >>= 1) { ml = max(ml, __shfl_xor(ml, off)); mx = max(mx, __shfl_xor(mx, off)); }
  if ((threadIdx.x & 63) == 0) { if (ml > 0) atomicMax(&st[0], ml); if (mx > 0) atomicMax(&st[2], mx); }
}

// ------------------------------------------------------------------ one lane per row (ub ≤ 64; CAP covers the launch's lane rows)
// FILL = false: uniq[i] = distinct columns of row i.  FILL = true: the ascending columns into the row's segment of ccol.
template <int CAP, int TBK, bool FILL>
__global__ __launch_bounds__(TBK) void spgemm_lane_symbolic_kernel(int m, const int *__restrict__ ub, const int *__restrict__ arp, const int *__restrict__ aci,
                                                                   const int *__restrict__ brp, const int *__restrict__ bci, const int *__restrict__ crp,
                                                                   int *__restrict__ uniq, int *__restrict__ ccol) {
  __shared__ int keys[CAP * TBK];
  const int i = blockIdx.x * TBK + threadIdx.x, t = threadIdx.x;
  if (i >= m || ub[i] > SPG_LANE_UB) return;
  int cnt = 0;
  for (int ka = arp[i]; ka < arp[i + 1]; ++ka) {
    const int l = aci[ka];
    for (int kb = brp[l]; kb < brp[l + 1]; ++kb) {
      const int j = bci[kb];
      int b = cnt - 1;
      while (b >= 0 && keys[b * TBK + t] > j) --b;
      if (b >= 0 && keys[b * TBK + t] == j) continue;
      if (cnt >= CAP) continue;      // cannot happen: CAP ≥ the row's product count
      for (int q = cnt - 1; q > b; --q) keys[(q + 1) * TBK + t] = keys[q * TBK + t];
      keys[(b + 1) * TBK + t] = j;
      ++cnt;
    }
  }
  if (!FILL) { uniq[i] = cnt; return; }
  const int dst = crp[i], len = crp[i + 1] - dst;
  for (int q = 0; q < cnt && q < len; ++q) ccol[dst + q] = keys[q * TBK + t];
}

// the numeric pass of those rows: C's sorted columns of the row and an accumulator beside each in LDS, position by binary search
template <int CAP, int TBK>
__global__ __launch_bounds__(TBK) void spgemm_lane_numeric_kernel(int m, const int *__restrict__ ub, const int *__restrict__ arp, const int *__restrict__ aci,
                                                                  const double *__restrict__ av, const int *__restrict__ brp, const int *__restrict__ bci,
                                                                  const double *__restrict__ bv, const int *__restrict__ crp, const int *__restrict__ ccol,
                                                                  double *__restrict__ cval, int *__restrict__ miss) {
  __shared__ int keys[CAP * TBK];
  __shared__ double vals[CAP * TBK];
  const int i = blockIdx.x * TBK + threadIdx.x, t = threadIdx.x;
  if (i >= m || ub[i] > SPG_LANE_UB) return;
  const int dst = crp[i];
  int len = crp[i + 1] - dst;
  if (len > CAP) len = CAP;      // cannot happen: CAP ≥ the longest row of C
  for (int q = 0; q < len; ++q) { keys[q * TBK + t] = ccol[dst + q]; vals[q * TBK + t] = -0.0; }
  int missed = 0;
  for (int ka = arp[i]; ka < arp[i + 1]; ++ka) {
    const int l = aci[ka];
    const double a = av[ka];
    for (int kb = brp[l]; kb < brp[l + 1]; ++kb) {
      const int j = bci[kb];
      const double p = a * bv[kb];
      int lo = 0, hi = len - 1, pos = -1;
      while (lo <= hi) {
        const int mid = (lo + hi) >> 1, key = keys[mid * TBK + t];
        if (key == j) { pos = mid; break; }
        if (key < j) lo = mid + 1; else hi = mid - 1;
      }
      if (pos < 0) { ++missed; continue; }
      vals[pos * TBK + t] += p;
    }
  }
  for (int q = 0; q < len; ++q) cval[dst + q] = vals[q * TBK + t];
  if (missed) atomicAdd(miss, missed);
}

// ------------------------------------------------------------------ one workgroup per row (ub > 64)
__device__ __forceinline__ unsigned spg_hash(int j) { return ((unsigned)j * 2654435761u) >> 18; }   // 14 bits

// FILL = false: uniq[i] = distinct columns (a row above MGS_SPGEMM_MAX_ROW: lowest such row into *bad_row, uniq[i] = 0).
// FILL = true: the same table again, compacted and sorted in LDS, into the row's segment of ccol.
template <bool FILL>
__global__ __launch_bounds__(TB) void spgemm_wg_symbolic_kernel(const int *__restrict__ wg_rows, const int *__restrict__ arp, const int *__restrict__ aci,
                                                                const int *__restrict__ brp, const int *__restrict__ bci, const int *__restrict__ crp,
                                                                int *__restrict__ uniq, int *__restrict__ ccol, int *__restrict__ bad_row) {
  __shared__ int table[SPG_HASH];
  __shared__ int sorted[FILL ? MGS_SPGEMM_MAX_ROW : 1];
  __shared__ int cnt, cursor;
  const int i = wg_rows[blockIdx.x];
  for (int t = threadIdx.x; t < SPG_HASH; t += TB) table[t] = SPG_EMPTY;
  if (threadIdx.x == 0) { cnt = 0; cursor = 0; }
  __syncthreads();
  for (int ka = arp[i]; ka < arp[i + 1]; ++ka) {
    const int l = aci[ka], b0 = brp[l], b1 = brp[l + 1];
    for (int kb = b0 + threadIdx.x; kb < b1; kb += TB) {
      if (__atomic_load_n(&cnt, __ATOMIC_RELAXED) > MGS_SPGEMM_MAX_ROW) break;      // the table never fills: at most MAX_ROW + TB keys enter it
      const int j = bci[kb];
      unsigned h = spg_hash(j);
      for (int probe = 0; probe < SPG_HASH; ++probe, h = (h + 1) & (SPG_HASH - 1)) {
        const int old = atomicCAS(&table[h], SPG_EMPTY, j);
        if (old == SPG_EMPTY) { atomicAdd(&cnt, 1); break; }
        if (old == j) break;
      }
    }
    __syncthreads();
    const int seen = cnt;
    __syncthreads();                          // nobody inserts for the next step before everybody has read the count: the exit is uniform
    if (seen > MGS_SPGEMM_MAX_ROW) break;
  }
  const int n = cnt;
  if (!FILL) {
    if (threadIdx.x == 0) {
      if (n > MGS_SPGEMM_MAX_ROW) { atomicMin(bad_row, i); uniq[i] = 0; } else uniq[i] = n;
    }
    return;
  }
  const int dst = crp[i], len = crp[i + 1] - dst;
  if (n > MGS_SPGEMM_MAX_ROW || n != len) return;      // cannot happen: the count pass saw the same table
  int n2 = 64;
  while (n2 < n) n2 <<= 1;
  for (int t = threadIdx.x; t < SPG_HASH; t += TB) { const int j = table[t]; if (j != SPG_EMPTY) sorted[atomicAdd(&cursor, 1)] = j; }
  for (int t = n + threadIdx.x; t < n2; t += TB) sorted[t] = INT_MAX;
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (n2 >> 1); t += TB) {
        const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
        const int x = sorted[a], y = sorted[b];
        if ((x > y) == ((a & k) == 0)) { sorted[a] = y; sorted[b] = x; }
      }
      __syncthreads();
    }
  for (int t = threadIdx.x; t < n; t += TB) ccol[dst + t] = sorted[t];
}

// the numeric pass of those rows: accumulators are the row's segment of C->val itself
__global__ __launch_bounds__(TB) void spgemm_wg_numeric_kernel(const int *__restrict__ wg_rows, const int *__restrict__ arp, const int *__restrict__ aci,
                                                               const double *__restrict__ av, const int *__restrict__ brp, const int *__restrict__ bci,
                                                               const double *__restrict__ bv, const int *__restrict__ crp, const int *__restrict__ ccol,
                                                               double *cval, int *__restrict__ miss) {
  __shared__ int keys[MGS_SPGEMM_MAX_ROW];
  const int i = wg_rows[blockIdx.x];
  const int dst = crp[i], len = crp[i + 1] - dst;
  const bool lds = len <= MGS_SPGEMM_MAX_ROW;      // always, for a C this file built
  for (int t = threadIdx.x; t < len; t += TB) { if (lds) keys[t] = ccol[dst + t]; cval[dst + t] = -0.0; }
  __syncthreads();
  int missed = 0;
  for (int ka = arp[i]; ka < arp[i + 1]; ++ka) {
    const int l = aci[ka], b0 = brp[l], b1 = brp[l + 1];
    const double a = av[ka];
    for (int kb = b0 + threadIdx.x; kb < b1; kb += TB) {
      const int j = bci[kb];
      const double p = a * bv[kb];
      int lo = 0, hi = len - 1, pos = -1;
      while (lo <= hi) {
        const int mid = (lo + hi) >> 1, key = lds ? keys[mid] : ccol[dst + mid];
        if (key == j) { pos = mid; break; }
        if (key < j) lo = mid + 1; else hi = mid - 1;
      }
      if (pos < 0) { ++missed; continue; }
      cval[dst + pos] += p;      // B's columns ascend strictly inside a row: no other lane has this position in this step
    }
    __syncthreads();             // the next entry of A adds after this one: the order met
  }
  if (missed) atomicAdd(miss, missed);
}

__global__ void spgemm_total_kernel(int m, const int *__restrict__ uniq, unsigned long long *__restrict__ total) {
  const int i = blockIdx.x * TB + threadIdx.x;
  unsigned long long s = i < m ? (unsigned long long)uniq[i] : 0ull;
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(total, s);
}

int cap_of(int64_t longest) { return longest <= 16 ? 16 : (longest <= 32 ? 32 : 64); }

template <bool FILL>
void launch_symbolic(const mgs_csr *A, const mgs_csr *B, const mgs_spgemm_plan *pl, int lane_cap, const int *crp, int *uniq, int *ccol, int *bad_row) {
  hipStream_t s = A->ctx->stream;
  const int m = A->rows;
#define SYM_(CAPV, TBV) hipLaunchKernelGGL((spgemm_lane_symbolic_kernel<CAPV, TBV, FILL>), dim3(mgs_grid(m, TBV)), dim3(TBV), 0, s, m, pl->ub, A->rowptr, A->col, \
                                           B->rowptr, B->col, crp, uniq, ccol)
  if (pl->n_lane) { if (lane_cap == 16) SYM_(16, 256); else if (lane_cap == 32) SYM_(32, 128); else SYM_(64, 64); }
#undef SYM_
  if (pl->n_wg) hipLaunchKernelGGL((spgemm_wg_symbolic_kernel<FILL>), dim3(pl->n_wg), dim3(TB), 0, s, pl->wg_rows, A->rowptr, A->col, B->rowptr, B->col, crp, uniq, ccol, bad_row);
}

// the numeric pass: at most two launches on the context's stream, nothing else
int launch_numeric(const mgs_csr *A, const mgs_csr *B, mgs_csr *C, const mgs_spgemm_plan *pl) {
  mgs_ctx *ctx = A->ctx;
  hipStream_t s = ctx->stream;
  const int m = A->rows;
  if (!m || !C->nnz) return MGS_OK;
  const int cap = cap_of(C->max_row_len);      // a lane row of C is no longer than min(64, the longest row)
#define NUM_(CAPV, TBV) hipLaunchKernelGGL((spgemm_lane_numeric_kernel<CAPV, TBV>), dim3(mgs_grid(m, TBV)), dim3(TBV), 0, s, m, pl->ub, A->rowptr, A->col, A->val, \
                                           B->rowptr, B->col, B->val, C->rowptr, C->col, C->val, pl->miss)
  if (pl->n_lane) { if (cap == 16) NUM_(16, 256); else if (cap == 32) NUM_(32, 128); else NUM_(64, 64); }
#undef NUM_
  if (pl->n_wg) hipLaunchKernelGGL(spgemm_wg_numeric_kernel, dim3(pl->n_wg), dim3(TB), 0, s, pl->wg_rows, A->rowptr, A->col, A->val, B->rowptr, B->col, B->val,
                                   C->rowptr, C->col, C->val, pl->miss);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

int finish(mgs_ctx *ctx, const char *who) {   // launch errors of everything enqueued so far + the stream's completion
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return mgs_fail(ctx, MGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  return MGS_OK;
}

// shard: refuse row shards (the public entry points; the Galerkin product multiplies the library's own Pᵀ and P of a square level)
int factors_check(const mgs_csr *A, const mgs_csr *B, bool shard, const char *who) {
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, A->ctx == B->ctx, MGS_ERR_INVALID, "%s: the factors belong to different contexts", who);
  MGS_CHECK(ctx, !shard || (!mgs_csr_is_shard(A) && !mgs_csr_is_shard(B)), MGS_ERR_INVALID,
            "%s: %s is a row shard (%d rows, %d columns with halo columns): products on row shards are not supported", who, mgs_csr_is_shard(A) ? "A" : "B",
            mgs_csr_is_shard(A) ? A->rows : B->rows, mgs_csr_is_shard(A) ? A->cols : B->cols);
  MGS_CHECK(ctx, A->cols == B->rows, MGS_ERR_INVALID, "%s: A is %d x %d, B is %d x %d", who, A->rows, A->cols, B->rows, B->cols);
  return MGS_OK;
}

int spgemm_build(const mgs_csr *A, const mgs_csr *B, mgs_spgemm_plan *pl, mgs_csr **out) {
  mgs_ctx *ctx = A->ctx;
  hipStream_t s = ctx->stream;
  const int m = A->rows;
  const char *who = "mgs_csr_spgemm";
  DevBuf wg_all, st, uniq, total;
  MGS_TRY(mgs_dev_alloc(ctx, &pl->ub, (size_t)m));
  MGS_TRY(mgs_dev_alloc(ctx, &pl->miss, 1));
  MGS_TRY(dalloc<int>(ctx, wg_all, (size_t)m));
  MGS_TRY(dalloc<int>(ctx, st, 4));
  MGS_TRY(dalloc<int>(ctx, uniq, (size_t)m + 1));
  MGS_TRY(dalloc<unsigned long long>(ctx, total, 1));
  // 1. products per row, bins
  int h[4] = {0, 0, 0, INT_MAX};
  MGS_HIP(ctx, hipMemcpyAsync(st.p, h, sizeof h, hipMemcpyHostToDevice, s));
  MGS_HIP(ctx, hipMemsetAsync(pl->miss, 0, sizeof(int), s));
  if (m) hipLaunchKernelGGL(spgemm_ub_kernel, dim3(mgs_grid(m, TB)), dim3(TB), 0, s, m, A->rowptr, A->col, B->rowptr, pl->ub, wg_all.as<int>(), st.as<int>());
  MGS_HIP(ctx, hipMemcpyAsync(h, st.p, sizeof h, hipMemcpyDeviceToHost, s));
  MGS_TRY(finish(ctx, who));
  MGS_CHECK(ctx, h[1] >= 0 && h[1] <= m, MGS_ERR_HIP, "%s: %d long rows counted among %d rows", who, h[1], m);
  pl->n_wg = h[1]; pl->n_lane = (int64_t)m - h[1]; pl->max_ub = h[2];
  const int lane_cap = cap_of(h[0]);
  if (pl->n_wg) {
    MGS_TRY(mgs_dev_alloc(ctx, &pl->wg_rows, (size_t)pl->n_wg));
    MGS_HIP(ctx, hipMemcpyAsync(pl->wg_rows, wg_all.p, sizeof(int) * (size_t)pl->n_wg, hipMemcpyDeviceToDevice, s));
  }
  // 2. distinct columns per row, their 64-bit total, the lowest row beyond the limit
  MGS_HIP(ctx, hipMemsetAsync(uniq.p, 0, sizeof(int) * ((size_t)m + 1), s));
  MGS_HIP(ctx, hipMemsetAsync(total.p, 0, sizeof(unsigned long long), s));
  if (m) {
    launch_symbolic<false>(A, B, pl, lane_cap, nullptr, uniq.as<int>(), nullptr, st.as<int>() + 3);
    hipLaunchKernelGGL(spgemm_total_kernel, dim3(mgs_grid(m, TB)), dim3(TB), 0, s, m, uniq.as<int>(), total.as<unsigned long long>());
  }
  unsigned long long htotal = 0;
  MGS_HIP(ctx, hipMemcpyAsync(h, st.p, sizeof h, hipMemcpyDeviceToHost, s));
  MGS_HIP(ctx, hipMemcpyAsync(&htotal, total.p, sizeof htotal, hipMemcpyDeviceToHost, s));
  MGS_TRY(finish(ctx, who));
  MGS_CHECK(ctx, h[3] == INT_MAX, MGS_ERR_INVALID, "%s: row %d of the product holds more than MGS_SPGEMM_MAX_ROW = %d distinct columns", who, h[3], MGS_SPGEMM_MAX_ROW);
  MGS_CHECK(ctx, htotal < 2147483647ull, MGS_ERR_INVALID, "%s: the product holds %llu entries, more than 2^31 - 1", who, htotal);
  // 3. scan, 4. sorted columns, 5. values
  int64_t nnz = 0;
  MGS_TRY(k_exclusive_scan_i32(ctx, uniq.as<int>(), uniq.as<int>(), (int64_t)m + 1, &nnz));
  mgs_csr *C = nullptr;
  MGS_TRY(mgs_csr_alloc(ctx, m, B->cols, nnz, &C));
  *out = C;      // the caller destroys it on failure
  MGS_HIP(ctx, hipMemcpyAsync(C->rowptr, uniq.p, sizeof(int) * ((size_t)m + 1), hipMemcpyDeviceToDevice, s));
  if (m && nnz) launch_symbolic<true>(A, B, pl, lane_cap, C->rowptr, nullptr, C->col, nullptr);
  MGS_TRY(finish(ctx, who));
  MGS_TRY(mgs_plan_csr(C));      // the longest row of C picks the numeric pass's slots
  MGS_TRY(launch_numeric(A, B, C, pl));
  return finish(ctx, who);
}

int spgemm(const mgs_csr *A, const mgs_csr *B, bool shard_check, mgs_csr **out) {
  MGS_CHECK(A ? A->ctx : (B ? B->ctx : nullptr), A && B && out, MGS_ERR_INVALID, "mgs_csr_spgemm: NULL argument");
  MGS_TRY(factors_check(A, B, shard_check, "mgs_csr_spgemm"));
  mgs_spgemm_plan *pl = new mgs_spgemm_plan();
  mgs_csr *C = nullptr;
  const int rc = spgemm_build(A, B, pl, &C);
  if (rc != MGS_OK) {
    hipStreamSynchronize(A->ctx->stream);
    mgs_csr_destroy(C); mgs_free_spgemm(pl);
    return rc;
  }
  C->spg = pl;
  *out = C;
  return MGS_OK;
}

}  // namespace

int k_spgemm(const mgs_csr *A, const mgs_csr *B, mgs_csr **out) { return spgemm(A, B, true, out); }

int k_spgemm_numeric(const mgs_csr *A, const mgs_csr *B, mgs_csr *C, int64_t *misses) {
  MGS_CHECK(A ? A->ctx : (B ? B->ctx : (C ? C->ctx : nullptr)), A && B && C, MGS_ERR_INVALID, "mgs_csr_spgemm_numeric: NULL argument");
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, C->ctx == ctx, MGS_ERR_INVALID, "mgs_csr_spgemm_numeric: C belongs to a different context");
  MGS_TRY(factors_check(A, B, true, "mgs_csr_spgemm_numeric"));
  MGS_CHECK(ctx, C->spg, MGS_ERR_INVALID, "mgs_csr_spgemm_numeric: C was not built by mgs_csr_spgemm");
  MGS_CHECK(ctx, C->rows == A->rows && C->cols == B->cols, MGS_ERR_INVALID, "mgs_csr_spgemm_numeric: C is %d x %d, A·B is %d x %d", C->rows, C->cols, A->rows, B->cols);
  MGS_CHECK(ctx, !(C->code && C->code->vtab), MGS_ERR_INVALID, "mgs_csr_spgemm_numeric: C carries a value-carrying pattern code (option valcode): build the product again instead");
  MGS_HIP(ctx, hipMemsetAsync(C->spg->miss, 0, sizeof(int), ctx->stream));
  MGS_TRY(launch_numeric(A, B, C, C->spg));
  if (!misses) return MGS_OK;
  int hm = 0;
  MGS_HIP(ctx, hipMemcpyAsync(&hm, C->spg->miss, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *misses = hm;
  MGS_CHECK(ctx, hm == 0, MGS_ERR_STATE, "mgs_csr_spgemm_numeric: %d products fall outside C's pattern (the factors' patterns are not the ones C was built from)", hm);
  return MGS_OK;
}

int k_spgemm_info(const mgs_csr *C, int64_t out[4]) {
  MGS_CHECK(nullptr, C && out, MGS_ERR_INVALID, "mgs_csr_spgemm_info: NULL argument");
  out[0] = out[1] = out[2] = out[3] = 0;
  if (!C->spg) return MGS_OK;
  out[0] = C->spg->n_lane; out[1] = C->spg->n_wg; out[2] = C->max_row_len; out[3] = C->spg->max_ub;
  return MGS_OK;
}

// general P (not an aggregation): T = Pᵀ·A, A_c = T·P — the order of the reference's `Ptrans * A * P` (bicg.cpp:33)
int k_galerkin_general(const mgs_csr *A, const mgs_xfer *T, mgs_csr **out) {
  mgs_csr *PtA = nullptr;
  MGS_TRY(spgemm(T->Pt, A, false, &PtA));
  const int rc = spgemm(PtA, T->P, false, out);
  mgs_csr_destroy(PtA);
  return rc;
}
