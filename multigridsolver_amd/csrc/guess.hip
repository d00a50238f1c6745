// guess.hip — projected initial guesses for successive right-hand sides (mgs_guess, include/mgs.h).
// Nearest reference line: none — the reference solves one right-hand side (bicg.cpp:159-166).  The method is Fischer's projection
// (P. F. Fischer, Comput. Methods Appl. Mech. Engrg. 163 (1998) 193-204); PETSc ships it as KSPGuessFischer.
//
// State: size <= capacity pairs (x̃_k, ỹ_k = A·x̃_k) in one allocation, slot k of X at basis + k·stride and of Y at basis + (capacity + k)·stride.
// ENERGY pairs satisfy <x̃_j, ỹ_k> = δ_jk, RESIDUAL pairs <ỹ_j, ỹ_k> = δ_jk; q_k is the vector that is dotted (x̃_k resp. ỹ_k).
//
// Kernels.  Every streaming kernel runs one-shot workgroups of GTB lanes, lane t of workgroup g owning the two entries 2·(g·GTB + t) and the
// next one — the same assignment on the 16-byte path (every caller operand 16-byte aligned) and on the 8-byte path, so both give the same bits.
// Elementwise results are sums of products in ascending k that start from the first product, one rounding per product and per sum (the build
// uses -ffp-contract=off): given the coefficient bits a host restatement reproduces them bit for bit (tests/guess_ref.py).  Inner products
// leave one partial per workgroup in a fixed layout [row][workgroup]; guess_fold_mid_kernel (only above GFOLD1 workgroups) and
// guess_fold_final_kernel fold them in index order, no atomics: two identical calls give identical bits.  Coefficients never visit the host
// between the kernels that produce and consume them.
#include <algorithm>
#include <cmath>

#include "blas1.hpp"

namespace {
constexpr int GTB = 256;        // lanes per workgroup; a workgroup owns 2·GTB consecutive entries
constexpr int GK = 16;          // most pairs (MGS capacity limit)
constexpr int GROWS = GK + 1;   // partial rows of one pass: the K products and one norm
constexpr int GFOLD1 = 4096;    // workgroups (n <= 2^21) the final kernel folds by itself; above, chunks of GTB partials are folded first
// device scalars (doubles): four blocks of GBLK, then the decision record
constexpr int GBLK = 20;
constexpr int S_ALPHA = 0;           // α_k of the last apply; [16] ‖b‖², [17] ‖r0‖²
constexpr int S_C1 = GBLK;           // c¹_k; [16] ν0²
constexpr int S_C2 = 2 * GBLK;       // c²_k; [16] ν1²
constexpr int S_C3 = 3 * GBLK;       // [16] ν2² (no products are formed in the second pass)
constexpr int S_GRAM = 4 * GBLK;     // one column of mgs_guess_gram
constexpr int S_DEC = 5 * GBLK;      // [0] 1.0 = candidate accepted, [1] s = 1/√ν2²
constexpr int S_TOTAL = 5 * GBLK + 4;

using blas1::vd2; using blas1::al16;

// the lane's pair at i0 (two = both entries exist; else .y = 0): one 16-byte load where the operand allows it
__device__ __forceinline__ vd2 ld2(const double *p, int64_t i0, bool two, bool vec) {
  vd2 r;
  if (two) {
    if (vec) r = *reinterpret_cast<const vd2 *>(p + i0);
    else { r.x = p[i0]; r.y = p[i0 + 1]; }
  } else { r.x = p[i0]; r.y = 0.0; }
  return r;
}
__device__ __forceinline__ void st2(double *p, int64_t i0, bool two, bool vec, vd2 v) {
  if (two) {
    if (vec) *reinterpret_cast<vd2 *>(p + i0) = v;
    else { p[i0] = v.x; p[i0 + 1] = v.y; }
  } else p[i0] = v.x;
}
// workgroup sums of `rows` lane values: 6 shuffle levels inside each wave, then the 4 wave sums in wave order; part[row][workgroup]
__device__ __forceinline__ void block_partials(double (&s)[GROWS], int rows, double *__restrict__ part) {
  __shared__ double sh[GROWS][GTB / 64];
#pragma unroll
  for (int k = 0; k < GROWS; ++k) {
    if (k < rows) {
      double t = s[k];
      for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off);
      if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = t;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < rows) {
    double t = sh[threadIdx.x][0];
    for (int q = 1; q < GTB / 64; ++q) t += sh[threadIdx.x][q];
    part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
  }
}

// rows k < K: <q_k, v>; row K (e != NULL): <e, v>.  v and e are read once.
__global__ __launch_bounds__(GTB) void guess_dots_kernel(int64_t n, int K, const double *__restrict__ Q, int64_t stride, const double *__restrict__ v,
                                                         const double *__restrict__ e, int vec, double *__restrict__ part) {
  double s[GROWS];
#pragma unroll
  for (int k = 0; k < GROWS; ++k) s[k] = 0.0;
  const int64_t i0 = 2 * ((int64_t)blockIdx.x * GTB + threadIdx.x);
  if (i0 < n) {
    const bool two = i0 + 1 < n;
    const vd2 vi = ld2(v, i0, two, vec != 0);
#pragma unroll
    for (int k = 0; k < GK; ++k)
      if (k < K) { const vd2 q = ld2(Q + (int64_t)k * stride, i0, two, true); s[k] = q.x * vi.x; s[k] += q.y * vi.y; }
    if (e) {
      const vd2 ei = (e == v) ? vi : ld2(e, i0, two, vec != 0);
#pragma unroll
      for (int k = 0; k < GROWS; ++k) if (k == K) { s[k] = ei.x * vi.x; s[k] += ei.y * vi.y; }
    }
  }
  block_partials(s, K + (e ? 1 : 0), part);
}

// x0 = Σ α_k·x̃_k; with part: r0 = b − Σ α_k·ỹ_k is formed (not stored) and row 0 receives ‖r0‖²
__global__ __launch_bounds__(GTB) void guess_combine_kernel(int64_t n, int K, const double *__restrict__ X, const double *__restrict__ Y, int64_t stride,
                                                            const double *__restrict__ alpha, double *__restrict__ x0, const double *__restrict__ b, int vec,
                                                            double *__restrict__ part) {
  double s[GROWS];
#pragma unroll
  for (int k = 0; k < GROWS; ++k) s[k] = 0.0;
  const int64_t i0 = 2 * ((int64_t)blockIdx.x * GTB + threadIdx.x);
  if (i0 < n) {
    const bool two = i0 + 1 < n;
    vd2 tx = {0.0, 0.0}, ty = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < GK; ++k) {
      if (k < K) {
        const double a = alpha[k];
        const vd2 xk = ld2(X + (int64_t)k * stride, i0, two, true);
        vd2 p; p.x = a * xk.x; p.y = a * xk.y;
        if (k == 0) tx = p; else { tx.x += p.x; tx.y += p.y; }
        if (part) {
          const vd2 yk = ld2(Y + (int64_t)k * stride, i0, two, true);
          vd2 r; r.x = a * yk.x; r.y = a * yk.y;
          if (k == 0) ty = r; else { ty.x += r.x; ty.y += r.y; }
        }
      }
    }
    st2(x0, i0, two, vec != 0, tx);
    if (part) {
      const vd2 bi = ld2(b, i0, two, vec != 0);
      const double rx = bi.x - ty.x, ry = two ? bi.y - ty.y : 0.0;
      s[0] = rx * rx; s[0] += ry * ry;
    }
  }
  if (part) block_partials(s, 1, part);
}

// Gram-Schmidt against the K stored pairs, on the solution and its image at once: x' = x − Σ c_k·x̃_k, w' = w − Σ c_k·ỹ_k (in place where
// xs == xd resp. ws == wd: a lane reads its own entries before it writes them).  The q_k are in registers when w' is known, so with dots != 0
// rows k < K receive <q_k, w'> and row K ν² = <x', w'> (energy) or <w', w'>; with dots == 0 ν² is row 0, the only one.
__global__ __launch_bounds__(GTB) void guess_pair_kernel(int64_t n, int K, const double *__restrict__ X, const double *__restrict__ Y, int64_t stride, int energy,
                                                         const double *__restrict__ coef, const double *xs, const double *ws, double *xd, double *wd, int vec,
                                                         int dots, double *__restrict__ part) {
  double s[GROWS];
#pragma unroll
  for (int k = 0; k < GROWS; ++k) s[k] = 0.0;
  const int nrow = dots ? K : 0;          // the norm's row: behind the products, or the only one
  const int64_t i0 = 2 * ((int64_t)blockIdx.x * GTB + threadIdx.x);
  if (i0 < n) {
    const bool two = i0 + 1 < n;
    vd2 q[GK];
    vd2 tx = {0.0, 0.0}, tw = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < GK; ++k) {
      if (k < K) {
        const double c = coef[k];
        const vd2 xk = ld2(X + (int64_t)k * stride, i0, two, true), yk = ld2(Y + (int64_t)k * stride, i0, two, true);
        vd2 p, r;
        p.x = c * xk.x; p.y = c * xk.y; r.x = c * yk.x; r.y = c * yk.y;
        if (k == 0) { tx = p; tw = r; } else { tx.x += p.x; tx.y += p.y; tw.x += r.x; tw.y += r.y; }
        q[k] = energy ? xk : yk;
      }
    }
    const vd2 xi = ld2(xs, i0, two, vec != 0), wi = ld2(ws, i0, two, true);
    vd2 xo, wo;
    xo.x = xi.x - tx.x; xo.y = two ? xi.y - tx.y : 0.0;
    wo.x = wi.x - tw.x; wo.y = two ? wi.y - tw.y : 0.0;
    st2(xd, i0, two, true, xo);
    st2(wd, i0, two, true, wo);
    if (dots) {
#pragma unroll
      for (int k = 0; k < GK; ++k) if (k < K) { s[k] = q[k].x * wo.x; s[k] += q[k].y * wo.y; }
    }
    const vd2 ev = energy ? xo : wo;
#pragma unroll
    for (int k = 0; k < GROWS; ++k) if (k == nrow) { s[k] = ev.x * wo.x; s[k] += ev.y * wo.y; }
  }
  block_partials(s, nrow + 1, part);
}

// chunk c of row k: GTB partials, tree fold in a fixed order
__global__ __launch_bounds__(GTB) void guess_fold_mid_kernel(int nb, const double *__restrict__ part, double *__restrict__ mid) {
  __shared__ double sh[GTB];
  const int k = blockIdx.y, i = blockIdx.x * GTB + threadIdx.x;
  sh[threadIdx.x] = i < nb ? part[(size_t)k * nb + i] : 0.0;
  __syncthreads();
  for (int w = GTB / 2; w > 0; w >>= 1) { if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
  if (threadIdx.x == 0) mid[(size_t)k * gridDim.x + blockIdx.x] = sh[0];
}
// one workgroup per row: strided sums in index order, then the tree.  Row k < K lands in out[k], row K + j in out[GK + j].
__global__ __launch_bounds__(GTB) void guess_fold_final_kernel(int nf, int K, const double *__restrict__ src, double *__restrict__ out) {
  __shared__ double sh[GTB];
  const int k = blockIdx.x;
  double s = 0.0;
  for (int i = threadIdx.x; i < nf; i += GTB) s += src[(size_t)k * nf + i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = GTB / 2; w > 0; w >>= 1) { if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
  if (threadIdx.x == 0) out[k < K ? k : GK + (k - K)] = sh[0];
}

// DGKS with η = 1/√2 on the squares: accept when ν2² is finite and positive, ν2² >= ν1²/2 and ν0² > 0 (an energy candidate along which A is
// not positive, a constant candidate of a declared null space, a zero vector).  K == 0 (empty basis, restart): nothing was orthogonalised, ν1² = ν2² = ν0².
// The floor ν2 > 32·2⁻⁵²·ν0 (GUESS_FLOOR2 on the squares; the drop tolerance of PETSc's KSPGuessFischer): what the first pass leaves of a candidate
// inside the span is rounding noise of about u·ν0, which is nearly orthogonal to the few stored pairs — the second pass barely shortens it, and
// the comparison of ν2 with ν1 alone would accept it.
constexpr double GUESS_FLOOR2 = 0x1p-94;
__global__ void guess_decide_kernel(int K, double *__restrict__ st) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double nu0 = st[S_C1 + GK];
  if (K == 0) { st[S_C2 + GK] = nu0; st[S_C3 + GK] = nu0; }
  const double nu1 = st[S_C2 + GK], nu2 = st[S_C3 + GK];
  const bool ok = isfinite(nu2) && nu2 > 0.0 && nu2 >= 0.5 * nu1 && nu0 > 0.0 && nu2 > GUESS_FLOOR2 * nu0;
  st[S_DEC] = ok ? 1.0 : 0.0;
  st[S_DEC + 1] = ok ? 1.0 / sqrt(nu2) : 0.0;
}
// the only copy out of scratch: x̃ = s·x'', ỹ = s·w'' into the new slot, if the candidate was accepted
__global__ __launch_bounds__(GTB) void guess_store_kernel(int64_t n, const double *__restrict__ dec, const double *xs, const double *ws, double *xd, double *yd, int vec) {
  if (dec[0] == 0.0) return;
  const double s = dec[1];
  const int64_t i0 = 2 * ((int64_t)blockIdx.x * GTB + threadIdx.x);
  if (i0 >= n) return;
  const bool two = i0 + 1 < n;
  const vd2 xi = ld2(xs, i0, two, vec != 0), wi = ld2(ws, i0, two, true);
  vd2 xo, wo;
  xo.x = s * xi.x; xo.y = s * xi.y; wo.x = s * wi.x; wo.y = s * wi.y;
  st2(xd, i0, two, true, xo);
  st2(yd, i0, two, true, wo);
}
}   // namespace

struct mgs_guess {
  mgs_ctx *ctx = nullptr;
  const mgs_csr *A = nullptr;
  int kind = 0, capacity = 0, size = 0;
  int64_t n = 0, stride = 0;
  int nb = 1, nmid = 0;              // workgroups of a streaming pass; chunk sums behind them (0: the final kernel folds the partials itself)
  double *basis = nullptr;           // 2·capacity·stride doubles
  double *part = nullptr, *mid = nullptr;
  double *st = nullptr;              // S_TOTAL device scalars
  int64_t restarts = 0, refused = 0, bytes = 0;
  int last = 0, lastK = 0;           // what mgs_guess_coef reports: 0 nothing yet, 1 an apply, 2 an update; pairs it ran against
  double *X(int k) const { return basis + (int64_t)k * stride; }
  double *Y(int k) const { return basis + (int64_t)(capacity + k) * stride; }
  const double *Q() const { return kind == MGS_GUESS_ENERGY ? X(0) : Y(0); }
};

// partials of `rows` rows → out (see guess_fold_final_kernel)
static int fold(mgs_guess *g, int rows, int K, double *out) {
  mgs_ctx *ctx = g->ctx;
  const double *src = g->part; int nf = g->nb;
  if (g->nmid) {
    hipLaunchKernelGGL(guess_fold_mid_kernel, dim3(g->nmid, rows), dim3(GTB), 0, ctx->stream, g->nb, g->part, g->mid);
    src = g->mid; nf = g->nmid;
  }
  hipLaunchKernelGGL(guess_fold_final_kernel, dim3(rows), dim3(GTB), 0, ctx->stream, nf, K, src, out);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
static int read_scalars(mgs_guess *g, int off, int cnt, double *host) {
  MGS_HIP(g->ctx, hipMemcpyAsync(host, g->st + off, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, g->ctx->stream));
  MGS_HIP(g->ctx, hipStreamSynchronize(g->ctx->stream));
  return MGS_OK;
}

int mgs_guess_create(const mgs_csr *A, int kind, int capacity, mgs_guess **out) {
  mgs_ctx *ctx = A ? A->ctx : nullptr;      // kind and capacity are named whether or not a matrix was given
  MGS_CHECK(ctx, out, MGS_ERR_INVALID, "mgs_guess_create: NULL result pointer");
  MGS_CHECK(ctx, kind == MGS_GUESS_ENERGY || kind == MGS_GUESS_RESIDUAL, MGS_ERR_INVALID, "mgs_guess_create: unknown kind %d", kind);
  MGS_CHECK(ctx, capacity >= 1 && capacity <= GK, MGS_ERR_INVALID, "mgs_guess_create: capacity %d outside 1..%d", capacity, GK);
  MGS_CHECK(ctx, A, MGS_ERR_INVALID, "mgs_guess_create: NULL matrix");
  MGS_CHECK(ctx, A->rows == A->cols, MGS_ERR_INVALID, "mgs_guess_create: the matrix is %d x %d (%s)", A->rows, A->cols,
            A->cols > A->rows ? "halo columns: a row shard" : "not square");
  MGS_CHECK(ctx, A->nullspace != MGS_NULLSPACE_FIELDS, MGS_ERR_INVALID, "mgs_guess_create: a field-wise null space (MGS_NULLSPACE_FIELDS) is declared; it is served by mgs_minres / mgs_pcg");
  mgs_guess *g = new mgs_guess();
  g->ctx = ctx; g->A = A; g->kind = kind; g->capacity = capacity; g->n = A->rows;
  g->stride = ((g->n + 31) / 32) * 32; if (g->stride == 0) g->stride = 32;          // every slot 256-byte aligned
  g->nb = (int)std::max<int64_t>(1, (g->n + 2 * GTB - 1) / (2 * GTB));
  g->nmid = g->nb > GFOLD1 ? (g->nb + GTB - 1) / GTB : 0;
  const size_t nbasis = (size_t)2 * capacity * g->stride, npart = (size_t)GROWS * g->nb, nmidd = (size_t)GROWS * std::max(g->nmid, 1);
  int rc = mgs_dev_alloc(ctx, &g->basis, nbasis);
  if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &g->part, npart);
  if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &g->mid, nmidd);
  if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &g->st, (size_t)S_TOTAL);
  if (rc == MGS_OK && (hipMemsetAsync(g->basis, 0, sizeof(double) * nbasis, ctx->stream) != hipSuccess ||
                       hipMemsetAsync(g->st, 0, sizeof(double) * S_TOTAL, ctx->stream) != hipSuccess))
    rc = mgs_fail(ctx, MGS_ERR_HIP, "mgs_guess_create: hipMemsetAsync failed");
  if (rc != MGS_OK) { mgs_guess_destroy(g); return rc; }
  g->bytes = (int64_t)(sizeof(double) * (nbasis + npart + nmidd + S_TOTAL));
  *out = g;
  return MGS_OK;
}
int mgs_guess_destroy(mgs_guess *g) {
  if (!g) return MGS_OK;
  if (g->basis || g->part || g->mid || g->st) hipStreamSynchronize(g->ctx->stream);
  if (g->basis) mgs_hip_free(g->basis);
  if (g->part) mgs_hip_free(g->part);
  if (g->mid) mgs_hip_free(g->mid);
  if (g->st) mgs_hip_free(g->st);
  delete g;
  return MGS_OK;
}
int mgs_guess_reset(mgs_guess *g) {
  MGS_CHECK(g ? g->ctx : nullptr, g, MGS_ERR_INVALID, "mgs_guess_reset: NULL guess");
  g->size = 0;
  return MGS_OK;
}
int mgs_guess_info(const mgs_guess *g, int64_t out[6]) {
  MGS_CHECK(g ? g->ctx : nullptr, g && out, MGS_ERR_INVALID, "mgs_guess_info: NULL argument");
  out[0] = g->size; out[1] = g->capacity; out[2] = g->kind; out[3] = g->restarts; out[4] = g->refused; out[5] = g->bytes;
  return MGS_OK;
}

int mgs_guess_apply(mgs_guess *g, const mgs_vec *b, mgs_vec *x0, double *rel_resid) {
  MGS_CHECK(g ? g->ctx : nullptr, g && b && x0, MGS_ERR_INVALID, "mgs_guess_apply: NULL argument");
  mgs_ctx *ctx = g->ctx;
  const int64_t n = g->n;
  MGS_CHECK(ctx, b->n >= n && x0->n >= n, MGS_ERR_INVALID, "mgs_guess_apply: vectors of %lld and %lld entries, the operator has %lld rows", (long long)b->n,
            (long long)x0->n, (long long)n);
  MGS_CHECK(ctx, b->d != x0->d, MGS_ERR_INVALID, "mgs_guess_apply: x0 must not alias b");
  const int K = g->size;
  g->last = 1; g->lastK = K;
  if (n == 0) { if (rel_resid) *rel_resid = K ? 0.0 : 1.0; return MGS_OK; }
  const int vec = al16(b->d) && al16(x0->d);
  const bool want = rel_resid && K > 0;
  double *st = g->st;
  if (K > 0) {
    hipLaunchKernelGGL(guess_dots_kernel, dim3(g->nb), dim3(GTB), 0, ctx->stream, n, K, g->Q(), g->stride, b->d, want ? b->d : (const double *)nullptr, vec, g->part);
    MGS_TRY(fold(g, K + (want ? 1 : 0), K, st + S_ALPHA));
  }
  hipLaunchKernelGGL(guess_combine_kernel, dim3(g->nb), dim3(GTB), 0, ctx->stream, n, K, g->X(0), g->Y(0), g->stride, st + S_ALPHA, x0->d, b->d, vec,
                     want ? g->part : (double *)nullptr);
  MGS_HIP(ctx, hipGetLastError());
  if (want) {
    MGS_TRY(fold(g, 1, 0, st + S_ALPHA + 1));            // row 0 → [GK + 1]
    double two[2];
    MGS_TRY(read_scalars(g, S_ALPHA + GK, 2, two));
    const double nb = std::sqrt(two[0]), nr = std::sqrt(two[1]);
    *rel_resid = nb > 0.0 ? nr / nb : (nr > 0.0 ? INFINITY : 0.0);
  } else if (rel_resid) *rel_resid = 1.0;                 // empty basis: x0 = 0, r0 = b
  return MGS_OK;
}

// the update proper: x is any vector of n entries (the caller's solution, or a stored x̃_k during a rebase)
static int guess_update(mgs_guess *g, const double *x, int *added) {
  mgs_ctx *ctx = g->ctx;
  const int64_t n = g->n;
  const bool restart = g->size == g->capacity;
  const int K = restart ? 0 : g->size, slot = K;
  const int energy = g->kind == MGS_GUESS_ENERGY;
  MGS_CHECK(ctx, g->A->nullspace != MGS_NULLSPACE_FIELDS, MGS_ERR_INVALID, "mgs_guess_update: a field-wise null space (MGS_NULLSPACE_FIELDS) is declared; it is served by mgs_minres / mgs_pcg");
  const bool ns = g->A->nullspace == MGS_NULLSPACE_CONSTANT;
  mgs_vec *xs = nullptr, *w = nullptr;
  struct Guard { mgs_ctx *c; mgs_vec **a, **b; ~Guard() { mgs_ws_put(c, *a); mgs_ws_put(c, *b); } } guard{ctx, &xs, &w};
  MGS_TRY(mgs_ws_get(ctx, n, n, &xs));
  MGS_TRY(mgs_ws_get(ctx, n, n, &w));
  double *st = g->st;
  const double *xcur = x;          // where the candidate lives right now
  if (ns) {                        // zero-mean copy: every x̃_k, and with them x0, has zero mean
    MGS_HIP(ctx, hipMemcpyAsync(xs->d, x, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
    MGS_TRY(k_project_const(ctx, n, xs->d));
    xcur = xs->d;
  }
  mgs_vec xv; xv.ctx = ctx; xv.n = n; xv.d = const_cast<double *>(xcur); xv.owns = false;
  MGS_TRY(mgs_spmv(g->A, &xv, w));
  int vec = al16(xcur);
  hipLaunchKernelGGL(guess_dots_kernel, dim3(g->nb), dim3(GTB), 0, ctx->stream, n, K, g->Q(), g->stride, w->d, energy ? xcur : (const double *)w->d, vec, g->part);
  MGS_TRY(fold(g, K + 1, K, st + S_C1));
  if (K > 0) {
    // first pass into the free slot itself (after a refused update it still holds x', w': mgs_guess_pair), second pass from there into scratch
    hipLaunchKernelGGL(guess_pair_kernel, dim3(g->nb), dim3(GTB), 0, ctx->stream, n, K, g->X(0), g->Y(0), g->stride, energy, st + S_C1, xcur, w->d, g->X(slot), g->Y(slot),
                       vec, 1, g->part);
    MGS_TRY(fold(g, K + 1, K, st + S_C2));
    hipLaunchKernelGGL(guess_pair_kernel, dim3(g->nb), dim3(GTB), 0, ctx->stream, n, K, g->X(0), g->Y(0), g->stride, energy, st + S_C2, g->X(slot), g->Y(slot), xs->d, w->d,
                       1, 0, g->part);
    MGS_TRY(fold(g, 1, 0, st + S_C3));                    // row 0 → [GK]
    xcur = xs->d; vec = 1;
  }
  hipLaunchKernelGGL(guess_decide_kernel, dim3(1), dim3(64), 0, ctx->stream, K, st);
  hipLaunchKernelGGL(guess_store_kernel, dim3(g->nb), dim3(GTB), 0, ctx->stream, n, st + S_DEC, xcur, w->d, g->X(slot), g->Y(slot), vec);
  MGS_HIP(ctx, hipGetLastError());
  double rec[1];
  MGS_TRY(read_scalars(g, S_DEC, 1, rec));                // the host's bookkeeping; ν0², ν1², ν2² stay readable through mgs_guess_coef
  g->last = 2; g->lastK = K;
  const bool ok = rec[0] != 0.0;
  if (ok) { if (restart) { g->restarts++; g->size = 1; } else g->size++; }
  else g->refused++;
  if (added) *added = ok ? 1 : 0;
  return MGS_OK;
}
int mgs_guess_update(mgs_guess *g, const mgs_vec *x, int *added) {
  MGS_CHECK(g ? g->ctx : nullptr, g && x, MGS_ERR_INVALID, "mgs_guess_update: NULL argument");
  MGS_CHECK(g->ctx, x->n >= g->n, MGS_ERR_INVALID, "mgs_guess_update: a vector of %lld entries, the operator has %lld rows", (long long)x->n, (long long)g->n);
  if (added) *added = 0;
  if (g->n == 0) { g->refused++; return MGS_OK; }
  return guess_update(g, x->d, added);
}
// reset, then update(x̃_k) from the oldest to the newest, in place: the slot written never lies behind the slot read, it is none of the
// pairs the pass orthogonalises against, and where it is the slot read a lane reads its own entries before it writes them
int mgs_guess_rebase(mgs_guess *g) {
  MGS_CHECK(g ? g->ctx : nullptr, g, MGS_ERR_INVALID, "mgs_guess_rebase: NULL guess");
  const int old = g->size;
  g->size = 0;
  for (int k = 0; k < old; ++k) MGS_TRY(guess_update(g, g->X(k), nullptr));
  return MGS_OK;
}

int mgs_guess_pair(const mgs_guess *g, int k, mgs_vec *x, mgs_vec *y) {
  MGS_CHECK(g ? g->ctx : nullptr, g && x && y, MGS_ERR_INVALID, "mgs_guess_pair: NULL argument");
  MGS_CHECK(g->ctx, k >= 0 && k <= g->size && k < g->capacity, MGS_ERR_INVALID, "mgs_guess_pair: slot %d, the guess holds %d of %d pairs", k, g->size, g->capacity);
  MGS_CHECK(g->ctx, x->n >= g->n && y->n >= g->n, MGS_ERR_INVALID, "mgs_guess_pair: vectors shorter than the operator's %lld rows", (long long)g->n);
  if (g->n == 0) return MGS_OK;
  MGS_HIP(g->ctx, hipMemcpyAsync(x->d, g->X(k), sizeof(double) * (size_t)g->n, hipMemcpyDeviceToDevice, g->ctx->stream));
  MGS_HIP(g->ctx, hipMemcpyAsync(y->d, g->Y(k), sizeof(double) * (size_t)g->n, hipMemcpyDeviceToDevice, g->ctx->stream));
  return MGS_OK;
}
int mgs_guess_coef(const mgs_guess *g, double *host, int n) {
  MGS_CHECK(g ? g->ctx : nullptr, g && host, MGS_ERR_INVALID, "mgs_guess_coef: NULL argument");
  MGS_CHECK(g->ctx, n >= 0, MGS_ERR_INVALID, "mgs_guess_coef: n < 0");
  double all[S_TOTAL];
  for (int i = 0; i < S_TOTAL; ++i) all[i] = 0.0;
  if (g->last) MGS_TRY(read_scalars(const_cast<mgs_guess *>(g), 0, S_TOTAL, all));
  std::vector<double> v;
  const int K = g->lastK;
  if (g->last == 1) for (int k = 0; k < K; ++k) v.push_back(all[S_ALPHA + k]);
  if (g->last == 2) {
    for (int k = 0; k < K; ++k) v.push_back(all[S_C1 + k]);
    for (int k = 0; k < K; ++k) v.push_back(all[S_C2 + k]);
    v.push_back(all[S_C1 + GK]); v.push_back(all[S_C2 + GK]); v.push_back(all[S_C3 + GK]);
    v.push_back(all[S_DEC + 1]); v.push_back(all[S_DEC]);
  }
  for (int i = 0; i < n; ++i) host[i] = i < (int)v.size() ? v[i] : 0.0;
  return MGS_OK;
}
int mgs_guess_gram(mgs_guess *g, double *host) {
  MGS_CHECK(g ? g->ctx : nullptr, g && (host || g->size == 0), MGS_ERR_INVALID, "mgs_guess_gram: NULL argument");
  mgs_ctx *ctx = g->ctx;
  const int K = g->size;
  for (int k = 0; k < K; ++k) {           // column k: <q_j, ỹ_k>, j < K
    hipLaunchKernelGGL(guess_dots_kernel, dim3(g->nb), dim3(GTB), 0, ctx->stream, g->n, K, g->Q(), g->stride, g->Y(k), (const double *)nullptr, 1, g->part);
    MGS_TRY(fold(g, K, K, g->st + S_GRAM));
    double col[GK];
    MGS_TRY(read_scalars(g, S_GRAM, K, col));
    for (int j = 0; j < K; ++j) host[(size_t)j * K + k] = col[j];
  }
  return MGS_OK;
}
