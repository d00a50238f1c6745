// csr_algebra.hip — sums and scalings of device matrices: C = α·A + β·B with the union pattern (mgs_csr_add), the values of C again for
// unchanged patterns (mgs_csr_add_numeric), a_ij ← dl_i·a_ij·dr_j in place (mgs_csr_scale), the diagonal as a vector (mgs_csr_diag) and a
// vector as a diagonal matrix (mgs_csr_from_diag).  No reference counterpart: the reference reads its operators from files.
//
// Arithmetic (include/mgs.h states it as the contract; the build is -ffp-contract=off, so every product and sum below is rounded on its
// own): an entry stored only in A is fl(α·a), only in B fl(β·b), in both fl(fl(α·a) + fl(β·b)).  Nothing is accumulated, so a lone −0.0
// stays −0.0 and there is no order to speak of; no atomics on values.
//
// Phases of the sum: u_i = len_A(i) + len_B(i) and the bins → union length per row (a 64-bit total beside it) → scan → columns and
// values.  One merge serves all of them (template <int MODE>): count, fill (columns + values), values only.  Rows are binned by u:
//   * u ≤ 64: one lane per row, a serial two-pointer merge.
//   * u > 64: one wave per row, 64 entries at a time, nothing staged, so a row may be of any length.  The p-th entry of A's row looks its
//     column up in B's row (q = lower bound; a match if B's q-th column equals it) and lands at p + q − (common columns before it); that
//     count is a running prefix of the match flags: ballot, popcount of the lower lanes, a carry from chunk to chunk.  An unmatched
//     q-th entry of B's row lands at q + (lower bound in A's row) − (common columns before it), the same prefix over B's flags.  Every
//     place is computed from the two rows alone: nothing depends on the order in which lanes or waves run.
// The values-only mode compares C's column at the computed place with the entry's before it writes and never writes outside C's row, so a
// numeric call on factors of another pattern counts misses and harms nothing.
#include "mgs_internal.hpp"

#include <climits>

struct mgs_add_plan {
  int *u = nullptr;           // rows: len_A + len_B of every row (clamped to INT_MAX), the bin key
  int *wave_rows = nullptr;   // n_wave: rows with u > ADD_LANE_U, one wave each
  int *miss = nullptr;        // device counter of mgs_csr_add_numeric
  int n_wave = 0;
  int64_t n_lane = 0, both = 0;
};
void mgs_free_add(mgs_add_plan *p) {
  if (!p) return;
  if (p->u) mgs_hip_free(p->u);
  if (p->wave_rows) mgs_hip_free(p->wave_rows);
  if (p->miss) mgs_hip_free(p->miss);
  delete p;
}

namespace {
constexpr int TB = 256;
constexpr int WAVE = 64;
constexpr int ADD_LANE_U = 64;      // rows of at most this many entries of A and B together: one lane per row
enum { ADD_COUNT = 0, ADD_FILL = 1, ADD_VALS = 2 };

struct DevBuf {  // RAII for temporaries
  void *p = nullptr;
  ~DevBuf() { if (p) mgs_hip_free(p); }
  template <class T> T *as() { return (T *)p; }
};
template <class T>
int dalloc(mgs_ctx *ctx, DevBuf &b, size_t count) { T *q = nullptr; MGS_TRY(mgs_dev_alloc(ctx, &q, count)); b.p = q; return MGS_OK; }

// st[0] = rows listed in wave_rows
__global__ void add_u_kernel(int m, const int *__restrict__ arp, const int *__restrict__ brp, int *__restrict__ u, int *__restrict__ wave_rows, int *__restrict__ st) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= m) return;
  const long long s = (long long)(arp[i + 1] - arp[i]) + (long long)(brp[i + 1] - brp[i]);
  const int v = s > INT_MAX ? INT_MAX : (int)s;
  u[i] = v;
  if (v > ADD_LANE_U) wave_rows[atomicAdd(&st[0], 1)] = i;      // at most m rows are listed: wave_rows holds m
}

// one store of the merge.  ADD_FILL: column and value at `pos` of the row's segment [dst, dst + len).  ADD_VALS: the value only, and only
// where C's column there is the entry's; anything else is a miss of `n` entries
template <int MODE>
__device__ __forceinline__ void add_store(int pos, int len, int dst, int j, double v, int n, int *__restrict__ ccol, double *__restrict__ cval, int &missed) {
  if (MODE == ADD_FILL) {
    if (pos < len) { ccol[dst + pos] = j; cval[dst + pos] = v; }      // always: the count pass ran the same merge
  } else {
    if (pos < len && ccol[dst + pos] == j) cval[dst + pos] = v; else missed += n;
  }
}

// ------------------------------------------------------------------ one lane per row (u ≤ 64): serial two-pointer merge
template <int MODE>
__global__ __launch_bounds__(TB) void add_lane_kernel(int m, const int *__restrict__ u, double alpha, const int *__restrict__ arp, const int *__restrict__ aci,
                                                      const double *__restrict__ av, double beta, const int *__restrict__ brp, const int *__restrict__ bci,
                                                      const double *__restrict__ bv, const int *__restrict__ crp, int *__restrict__ uniq, int *__restrict__ ccol,
                                                      double *__restrict__ cval, int *__restrict__ miss) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= m || u[i] > ADD_LANE_U) return;
  int ka = arp[i], kb = brp[i];
  const int ea = arp[i + 1], eb = brp[i + 1];
  int dst = 0, len = 0, cnt = 0, missed = 0;
  if (MODE != ADD_COUNT) { dst = crp[i]; len = crp[i + 1] - dst; }
  while (ka < ea || kb < eb) {
    const bool ha = ka < ea, hb = kb < eb;
    const int ja = ha ? aci[ka] : 0, jb = hb ? bci[kb] : 0;
    const bool ta = ha && (!hb || ja <= jb), tb = hb && (!ha || jb <= ja);
    if (MODE != ADD_COUNT) {
      double v;
      if (ta && tb) { const double pa = alpha * av[ka], pb = beta * bv[kb]; v = pa + pb; }
      else if (ta) v = alpha * av[ka];
      else v = beta * bv[kb];
      add_store<MODE>(cnt, len, dst, ta ? ja : jb, v, (int)ta + (int)tb, ccol, cval, missed);
    }
    ka += ta; kb += tb; ++cnt;
  }
  if (MODE == ADD_COUNT) uniq[i] = cnt;
  if (MODE == ADD_VALS && missed) atomicAdd(miss, missed);
}

// first position in the ascending [base, base + n) whose column is not below j
__device__ __forceinline__ int add_lower_bound(const int *__restrict__ c, int base, int n, int j) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (c[base + mid] < j) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------------ one wave per row (u > 64), four rows per workgroup
template <int MODE>
__global__ __launch_bounds__(TB) void add_wave_kernel(int n_wave, const int *__restrict__ wave_rows, double alpha, const int *__restrict__ arp,
                                                      const int *__restrict__ aci, const double *__restrict__ av, double beta, const int *__restrict__ brp,
                                                      const int *__restrict__ bci, const double *__restrict__ bv, const int *__restrict__ crp, int *__restrict__ uniq,
                                                      int *__restrict__ ccol, double *__restrict__ cval, int *__restrict__ miss) {
  const int w = blockIdx.x * (TB / WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= n_wave) return;                      // the whole wave leaves: the ballots below see full waves only
  const int i = wave_rows[w];
  const int a0 = arp[i], la = arp[i + 1] - a0, b0 = brp[i], lb = brp[i + 1] - b0;
  const unsigned long long below = (1ull << lane) - 1ull;
  int dst = 0, len = 0, missed = 0;
  if (MODE != ADD_COUNT) { dst = crp[i]; len = crp[i + 1] - dst; }
  // A's entries: all of them land, the matched ones carry the sum
  int carry = 0;
  for (int base = 0; base < la; base += WAVE) {
    const int p = base + lane;
    const bool valid = p < la;
    int j = 0, q = 0;
    bool match = false;
    if (valid) {
      j = aci[a0 + p];
      q = add_lower_bound(bci, b0, lb, j);
      match = q < lb && bci[b0 + q] == j;
    }
    const unsigned long long flags = __ballot(match);
    if (MODE != ADD_COUNT && valid) {
      const int pos = p + q - (carry + __popcll(flags & below));
      double v;
      if (match) { const double pa = alpha * av[a0 + p], pb = beta * bv[b0 + q]; v = pa + pb; }
      else v = alpha * av[a0 + p];
      add_store<MODE>(pos, len, dst, j, v, match ? 2 : 1, ccol, cval, missed);
    }
    carry += __popcll(flags);
  }
  if (MODE == ADD_COUNT) {
    if (lane == 0) {
      const long long n = (long long)la + lb - carry;
      uniq[i] = n > INT_MAX ? INT_MAX : (int)n;      // the 64-bit total then refuses the sum
    }
    return;
  }
  // B's entries: the unmatched ones land, the matched ones only count
  carry = 0;
  for (int base = 0; base < lb; base += WAVE) {
    const int q = base + lane;
    const bool valid = q < lb;
    int j = 0, p = 0;
    bool match = false;
    if (valid) {
      j = bci[b0 + q];
      p = add_lower_bound(aci, a0, la, j);
      match = p < la && aci[a0 + p] == j;
    }
    const unsigned long long flags = __ballot(match);
    if (valid && !match) {
      const int pos = q + p - (carry + __popcll(flags & below));
      add_store<MODE>(pos, len, dst, j, beta * bv[b0 + q], 1, ccol, cval, missed);
    }
    carry += __popcll(flags);
  }
  if (MODE == ADD_VALS && missed) atomicAdd(miss, missed);
}

__global__ void add_total_kernel(int m, const int *__restrict__ uniq, unsigned long long *__restrict__ total) {
  const int i = blockIdx.x * TB + threadIdx.x;
  unsigned long long s = i < m ? (unsigned long long)uniq[i] : 0ull;
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(total, s);
}

// the merge over both bins: at most two launches on the context's stream, nothing else
template <int MODE>
void launch_merge(double alpha, const mgs_csr *A, double beta, const mgs_csr *B, const mgs_add_plan *pl, const int *crp, int *uniq, int *ccol, double *cval) {
  hipStream_t s = A->ctx->stream;
  const int m = A->rows;
  if (pl->n_lane) hipLaunchKernelGGL((add_lane_kernel<MODE>), dim3(mgs_grid(m, TB)), dim3(TB), 0, s, m, pl->u, alpha, A->rowptr, A->col, A->val, beta, B->rowptr, B->col,
                                     B->val, crp, uniq, ccol, cval, pl->miss);
  if (pl->n_wave) hipLaunchKernelGGL((add_wave_kernel<MODE>), dim3(mgs_grid(pl->n_wave, TB / WAVE)), dim3(TB), 0, s, pl->n_wave, pl->wave_rows, alpha, A->rowptr, A->col,
                                     A->val, beta, B->rowptr, B->col, B->val, crp, uniq, ccol, cval, pl->miss);
}

int finish(mgs_ctx *ctx, const char *who) {   // launch errors of everything enqueued so far + the stream's completion
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return mgs_fail(ctx, MGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  return MGS_OK;
}

int add_build(double alpha, const mgs_csr *A, double beta, const mgs_csr *B, mgs_add_plan *pl, mgs_csr **out) {
  mgs_ctx *ctx = A->ctx;
  hipStream_t s = ctx->stream;
  const int m = A->rows;
  const char *who = "mgs_csr_add";
  DevBuf wave_all, st, uniq, total;
  MGS_TRY(mgs_dev_alloc(ctx, &pl->u, (size_t)m));
  MGS_TRY(mgs_dev_alloc(ctx, &pl->miss, 1));
  MGS_TRY(dalloc<int>(ctx, wave_all, (size_t)m));
  MGS_TRY(dalloc<int>(ctx, st, 1));
  MGS_TRY(dalloc<int>(ctx, uniq, (size_t)m + 1));
  MGS_TRY(dalloc<unsigned long long>(ctx, total, 1));
  // 1. entries of A and B per row, bins
  int h = 0;
  MGS_HIP(ctx, hipMemsetAsync(st.p, 0, sizeof(int), s));
  MGS_HIP(ctx, hipMemsetAsync(pl->miss, 0, sizeof(int), s));
  if (m) hipLaunchKernelGGL(add_u_kernel, dim3(mgs_grid(m, TB)), dim3(TB), 0, s, m, A->rowptr, B->rowptr, pl->u, wave_all.as<int>(), st.as<int>());
  MGS_HIP(ctx, hipMemcpyAsync(&h, st.p, sizeof h, hipMemcpyDeviceToHost, s));
  MGS_TRY(finish(ctx, who));
  MGS_CHECK(ctx, h >= 0 && h <= m, MGS_ERR_HIP, "%s: %d long rows counted among %d rows", who, h, m);
  pl->n_wave = h; pl->n_lane = (int64_t)m - h;
  if (pl->n_wave) {
    MGS_TRY(mgs_dev_alloc(ctx, &pl->wave_rows, (size_t)pl->n_wave));
    MGS_HIP(ctx, hipMemcpyAsync(pl->wave_rows, wave_all.p, sizeof(int) * (size_t)pl->n_wave, hipMemcpyDeviceToDevice, s));
  }
  // 2. union length per row and its 64-bit total
  MGS_HIP(ctx, hipMemsetAsync(uniq.p, 0, sizeof(int) * ((size_t)m + 1), s));
  MGS_HIP(ctx, hipMemsetAsync(total.p, 0, sizeof(unsigned long long), s));
  if (m) {
    launch_merge<ADD_COUNT>(alpha, A, beta, B, pl, nullptr, uniq.as<int>(), nullptr, nullptr);
    hipLaunchKernelGGL(add_total_kernel, dim3(mgs_grid(m, TB)), dim3(TB), 0, s, m, uniq.as<int>(), total.as<unsigned long long>());
  }
  unsigned long long htotal = 0;
  MGS_HIP(ctx, hipMemcpyAsync(&htotal, total.p, sizeof htotal, hipMemcpyDeviceToHost, s));
  MGS_TRY(finish(ctx, who));
  MGS_CHECK(ctx, htotal < 2147483647ull, MGS_ERR_INVALID, "%s: the sum holds %llu entries, 2^31 - 1 or more", who, htotal);
  // 3. scan, 4. columns and values
  int64_t nnz = 0;
  MGS_TRY(k_exclusive_scan_i32(ctx, uniq.as<int>(), uniq.as<int>(), (int64_t)m + 1, &nnz));
  mgs_csr *C = nullptr;
  MGS_TRY(mgs_csr_alloc(ctx, m, A->cols, nnz, &C));
  *out = C;      // the caller destroys it on failure
  MGS_HIP(ctx, hipMemcpyAsync(C->rowptr, uniq.p, sizeof(int) * ((size_t)m + 1), hipMemcpyDeviceToDevice, s));
  if (m && nnz) launch_merge<ADD_FILL>(alpha, A, beta, B, pl, C->rowptr, nullptr, C->col, C->val);
  MGS_TRY(finish(ctx, who));
  pl->both = A->nnz + B->nnz - nnz;
  return mgs_plan_csr(C);
}

// what mgs_csr_add and mgs_csr_add_numeric ask of their operands alike
int operands_check(const mgs_csr *A, const mgs_csr *B, const char *who) {
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, A->ctx == B->ctx, MGS_ERR_INVALID, "%s: the operands belong to different contexts", who);
  MGS_CHECK(ctx, !mgs_csr_is_shard(A) && !mgs_csr_is_shard(B), MGS_ERR_INVALID,
            "%s: %s is a row shard (%d rows, %d columns with halo columns): sums of row shards are not supported", who, mgs_csr_is_shard(A) ? "A" : "B",
            mgs_csr_is_shard(A) ? A->rows : B->rows, mgs_csr_is_shard(A) ? A->cols : B->cols);
  MGS_CHECK(ctx, A->rows == B->rows && A->cols == B->cols, MGS_ERR_INVALID, "%s: A is %d x %d, B is %d x %d", who, A->rows, A->cols, B->rows, B->cols);
  return MGS_OK;
}

__global__ void scale_kernel(int64_t nnz, int rows, const int *__restrict__ rowptr, const int *__restrict__ col, double *__restrict__ val, const double *__restrict__ dl,
                             const double *__restrict__ dr) {
  const int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x;
  if (k >= nnz) return;
  double v = val[k];
  if (dl) {      // the entry's row: the last i with rowptr[i] ≤ k (empty rows share their successor's start and are passed over)
    int lo = 0, hi = rows;
    while (hi - lo > 1) {
      const int mid = lo + ((hi - lo) >> 1);
      if ((int64_t)rowptr[mid] <= k) lo = mid; else hi = mid;
    }
    v = dl[lo] * v;
  }
  if (dr) v = v * dr[col[k]];
  val[k] = v;
}

__global__ void diag_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val, double *__restrict__ d) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const int a = rowptr[i], len = rowptr[i + 1] - a;
  const int q = add_lower_bound(col, a, len, i);
  d[i] = q < len && col[a + q] == i ? val[a + q] : 0.0;
}

__global__ void from_diag_kernel(int n, const double *__restrict__ d, int *__restrict__ rowptr, int *__restrict__ col, double *__restrict__ val) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i > n) return;
  rowptr[i] = i;
  if (i < n) { col[i] = i; val[i] = d[i]; }
}

}  // namespace

int k_csr_add(double alpha, const mgs_csr *A, double beta, const mgs_csr *B, mgs_csr **out) {
  MGS_CHECK(A ? A->ctx : (B ? B->ctx : nullptr), A && B && out, MGS_ERR_INVALID, "mgs_csr_add: NULL argument");
  MGS_TRY(operands_check(A, B, "mgs_csr_add"));
  mgs_add_plan *pl = new mgs_add_plan();
  mgs_csr *C = nullptr;
  const int rc = add_build(alpha, A, beta, B, pl, &C);
  if (rc != MGS_OK) {
    hipStreamSynchronize(A->ctx->stream);
    mgs_csr_destroy(C); mgs_free_add(pl);
    return rc;
  }
  C->addp = pl;
  *out = C;
  return MGS_OK;
}

int k_csr_add_numeric(double alpha, const mgs_csr *A, double beta, const mgs_csr *B, mgs_csr *C, int64_t *misses) {
  MGS_CHECK(A ? A->ctx : (B ? B->ctx : (C ? C->ctx : nullptr)), A && B && C, MGS_ERR_INVALID, "mgs_csr_add_numeric: NULL argument");
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, C->ctx == ctx, MGS_ERR_INVALID, "mgs_csr_add_numeric: C belongs to a different context");
  MGS_TRY(operands_check(A, B, "mgs_csr_add_numeric"));
  MGS_CHECK(ctx, C->addp, MGS_ERR_INVALID, "mgs_csr_add_numeric: C was not built by mgs_csr_add");
  MGS_CHECK(ctx, C->rows == A->rows && C->cols == A->cols, MGS_ERR_INVALID, "mgs_csr_add_numeric: C is %d x %d, the operands are %d x %d", C->rows, C->cols, A->rows, A->cols);
  MGS_CHECK(ctx, !(C->code && C->code->vtab), MGS_ERR_INVALID, "mgs_csr_add_numeric: C carries a value-carrying pattern code (option valcode): build the sum again instead");
  if (misses) MGS_HIP(ctx, hipMemsetAsync(C->addp->miss, 0, sizeof(int), ctx->stream));
  if (C->rows && C->nnz) launch_merge<ADD_VALS>(alpha, A, beta, B, C->addp, C->rowptr, nullptr, C->col, C->val);
  MGS_HIP(ctx, hipGetLastError());
  if (!misses) return MGS_OK;
  int hm = 0;
  MGS_HIP(ctx, hipMemcpyAsync(&hm, C->addp->miss, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *misses = hm;
  MGS_CHECK(ctx, hm == 0, MGS_ERR_STATE, "mgs_csr_add_numeric: %d entries of A or B are not at their place in C's pattern (the operands' patterns are not the ones C was built from)", hm);
  return MGS_OK;
}

int k_csr_add_info(const mgs_csr *C, int64_t out[4]) {
  MGS_CHECK(nullptr, C && out, MGS_ERR_INVALID, "mgs_csr_add_info: NULL argument");
  out[0] = out[1] = out[2] = out[3] = 0;
  if (!C->addp) return MGS_OK;
  out[0] = C->addp->n_lane; out[1] = C->addp->n_wave; out[2] = C->max_row_len; out[3] = C->addp->both;
  return MGS_OK;
}

int k_csr_scale(mgs_csr *A, const mgs_vec *dl, const mgs_vec *dr) {
  MGS_CHECK(nullptr, A, MGS_ERR_INVALID, "mgs_csr_scale: NULL matrix");
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, (!dl || dl->ctx == ctx) && (!dr || dr->ctx == ctx), MGS_ERR_INVALID, "mgs_csr_scale: a vector belongs to a different context");
  MGS_CHECK(ctx, !mgs_csr_is_shard(A), MGS_ERR_INVALID, "mgs_csr_scale: the matrix is a row shard (%d rows, %d columns with halo columns): not supported", A->rows, A->cols);
  MGS_CHECK(ctx, !dl || dl->n >= A->rows, MGS_ERR_INVALID, "mgs_csr_scale: dl holds %lld entries, the matrix has %d rows", (long long)dl->n, A->rows);
  MGS_CHECK(ctx, !dr || dr->n >= A->cols, MGS_ERR_INVALID, "mgs_csr_scale: dr holds %lld entries, the matrix has %d columns", (long long)dr->n, A->cols);
  MGS_CHECK(ctx, !(A->code && A->code->vtab), MGS_ERR_INVALID, "mgs_csr_scale: the matrix carries a value-carrying pattern code (option valcode): upload it again instead");
  if ((!dl && !dr) || !A->nnz) return MGS_OK;
  hipLaunchKernelGGL(scale_kernel, dim3(mgs_grid(A->nnz, TB)), dim3(TB), 0, ctx->stream, A->nnz, A->rows, A->rowptr, A->col, A->val, dl ? dl->d : nullptr, dr ? dr->d : nullptr);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

int k_csr_diag(const mgs_csr *A, mgs_vec *d) {
  MGS_CHECK(A ? A->ctx : nullptr, A && d, MGS_ERR_INVALID, "mgs_csr_diag: NULL argument");
  mgs_ctx *ctx = A->ctx;
  const int n = A->rows < A->cols ? A->rows : A->cols;
  MGS_CHECK(ctx, d->ctx == ctx, MGS_ERR_INVALID, "mgs_csr_diag: the vector belongs to a different context");
  MGS_CHECK(ctx, d->n >= n, MGS_ERR_INVALID, "mgs_csr_diag: d holds %lld entries, the matrix is %d x %d", (long long)d->n, A->rows, A->cols);
  if (!n) return MGS_OK;
  hipLaunchKernelGGL(diag_kernel, dim3(mgs_grid(n, TB)), dim3(TB), 0, ctx->stream, n, A->rowptr, A->col, A->val, d->d);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

int k_csr_from_diag(mgs_ctx *ctx, const mgs_vec *d, mgs_csr **out) {
  MGS_CHECK(ctx, ctx && d && out, MGS_ERR_INVALID, "mgs_csr_from_diag: NULL argument");
  MGS_CHECK(ctx, d->ctx == ctx, MGS_ERR_INVALID, "mgs_csr_from_diag: the vector belongs to a different context");
  MGS_CHECK(ctx, d->n < 2147483647LL, MGS_ERR_INVALID, "mgs_csr_from_diag: the vector holds %lld entries, 2^31 - 1 or more", (long long)d->n);
  const int n = (int)d->n;
  mgs_csr *A = nullptr;
  MGS_TRY(mgs_csr_alloc(ctx, n, n, n, &A));
  hipLaunchKernelGGL(from_diag_kernel, dim3(mgs_grid((int64_t)n + 1, TB)), dim3(TB), 0, ctx->stream, n, d->d, A->rowptr, A->col, A->val);
  int rc = finish(ctx, "mgs_csr_from_diag");
  if (rc == MGS_OK) rc = mgs_plan_csr(A);
  if (rc != MGS_OK) { mgs_csr_destroy(A); return rc; }
  *out = A;
  return MGS_OK;
}
