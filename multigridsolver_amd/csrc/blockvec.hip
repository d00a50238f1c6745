// blockvec.hip — the two tall-skinny block passes: G = UᵀV for two lists of columns (mgs_vecs_gram) and Y = S·C for a list of columns and a
// small host matrix (mgs_vecs_combine).  A block is a pointer table passed by value, as MDotVecs in blas1.hip; there is no container type.
// gfx950 only.  Built from blas1.hpp: the 16-byte lane type, the alignment predicate and the last fold are the ones of every other reduction,
// and tests/eig_ref.py restates the bits of both passes (a Gram entry is blas1_ref.reduce_terms of the products u_a[i]·v_b[i]).
#include "blas1.hpp"

namespace {
using namespace blas1;

constexpr int GT = 8;               // a Gram tile is at most GT × GT: 64 FP64 accumulators per lane
constexpr int GRAM_BLOCKS = 2048;   // most workgroups of a Gram pass: the partials of an entry never reach fold_mid's 4096, the last stage folds them itself
constexpr int COEF_SLOT = MGS_VECS_MAX * MGS_VECS_MAX;                 // vecs_dev: [0, COEF_SLOT) a Gram matrix's entries, then a combine's coefficients
constexpr int COEF_DOUBLES = MGS_VECS_MAX * 16;                        // most coefficients of one combine
constexpr int VECS_DEV_DOUBLES = COEF_SLOT + COEF_DOUBLES;

struct GramCols { const double *u[GT]; const double *v[GT]; };

// One tile: s[a][b] = Σ_i u_a[i]·v_b[i] for a < tp, b < tq; every column of the tile is read once.  VEC: lane t of workgroup w takes the pairs
// w·TB + t stepping by gridDim.x·TB and adds the product of the first elements, then that of the second (mdot_partial_kernel's order); the odd
// last element goes to lane 0 of workgroup 0 after its loop.  Else one element per step.  Every product and sum is rounded on its own
// (-ffp-contract=off).  Partials: part[(a·tq + b)·gridDim.x + w], waves added in wave order from 0.0.
template <bool VEC>
__global__ __launch_bounds__(TB) void gram_tile_kernel(int64_t n, int tp, int tq, const GramCols T, double *__restrict__ part) {
  __shared__ double sh[GT * GT][TB / 64];
  double s[GT][GT];
#pragma unroll
  for (int a = 0; a < GT; ++a)
#pragma unroll
    for (int b = 0; b < GT; ++b) s[a][b] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * TB;
  if (VEC) {
    const int64_t n2 = n >> 1;
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n2; i += stride) {
      vd2 u[GT], v[GT];
#pragma unroll
      for (int a = 0; a < GT; ++a) if (a < tp) u[a] = reinterpret_cast<const vd2 *>(T.u[a])[i];
#pragma unroll
      for (int b = 0; b < GT; ++b) if (b < tq) v[b] = reinterpret_cast<const vd2 *>(T.v[b])[i];
#pragma unroll
      for (int a = 0; a < GT; ++a)
#pragma unroll
        for (int b = 0; b < GT; ++b)
          if (a < tp && b < tq) { s[a][b] += u[a].x * v[b].x; s[a][b] += u[a].y * v[b].y; }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
      for (int a = 0; a < GT; ++a)
#pragma unroll
        for (int b = 0; b < GT; ++b)
          if (a < tp && b < tq) s[a][b] += T.u[a][n - 1] * T.v[b][n - 1];
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += stride) {
      double u[GT], v[GT];
#pragma unroll
      for (int a = 0; a < GT; ++a) if (a < tp) u[a] = T.u[a][i];
#pragma unroll
      for (int b = 0; b < GT; ++b) if (b < tq) v[b] = T.v[b][i];
#pragma unroll
      for (int a = 0; a < GT; ++a)
#pragma unroll
        for (int b = 0; b < GT; ++b)
          if (a < tp && b < tq) s[a][b] += u[a] * v[b];
    }
  }
#pragma unroll
  for (int a = 0; a < GT; ++a)
#pragma unroll
    for (int b = 0; b < GT; ++b) {
      if (a < tp && b < tq) {
        double t = s[a][b];
        for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off);
        if ((threadIdx.x & 63) == 0) sh[a * tq + b][threadIdx.x >> 6] = t;
      }
    }
  __syncthreads();
  if ((int)threadIdx.x < tp * tq) {
    double t = 0.0;
    for (int w = 0; w < TB / 64; ++w) t += sh[threadIdx.x][w];
    part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
  }
}
// the last stage, one workgroup per entry of the tile: entry e = a·tq + b goes to out[(a0 + a)·ld + b0 + b]
__global__ __launch_bounds__(TB) void gram_final_kernel(int nb, int tq, int a0, int b0, int ld, const double *__restrict__ part, double *__restrict__ out) {
  __shared__ double sh[TB];
  const int e = blockIdx.x;
  const double r = final_fold(nb, part + (size_t)e * nb, sh);
  if (threadIdx.x == 0) out[(size_t)(a0 + e / tq) * ld + b0 + e % tq] = r;
}

struct CombineCols { const double *s[MGS_VECS_MAX]; double *y[16]; };

// Y_j[i] = fl(…fl(fl(C[0][j]·S_0[i]) + fl(C[1][j]·S_1[i])) + …), a ascending.  The coefficients come from device memory into LDS.  A lane loads
// every input element of its row (pair) before it stores any output of that row, so an output may be one of the inputs (no __restrict__ on either).
template <bool VEC>
__global__ __launch_bounds__(TB) void combine_kernel(int64_t n, int k, int q, const CombineCols T, const double *__restrict__ coef) {
  __shared__ double cs[MGS_VECS_MAX * 16];
  for (int e = threadIdx.x; e < k * q; e += TB) cs[e] = coef[e];
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * TB;
  if (VEC) {
    const int64_t n2 = n >> 1;
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n2; i += stride) {
      vd2 s[MGS_VECS_MAX];
#pragma unroll
      for (int a = 0; a < MGS_VECS_MAX; ++a) if (a < k) s[a] = reinterpret_cast<const vd2 *>(T.s[a])[i];
      asm volatile("" ::: "memory");      // (the loads above stay above the stores below)
      for (int j = 0; j < q; ++j) {
        vd2 y;
        y.x = cs[j] * s[0].x; y.y = cs[j] * s[0].y;
#pragma unroll
        for (int a = 1; a < MGS_VECS_MAX; ++a) if (a < k) { const double c = cs[a * q + j]; y.x = y.x + c * s[a].x; y.y = y.y + c * s[a].y; }
        reinterpret_cast<vd2 *>(T.y[j])[i] = y;
      }
    }
    if (!((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)) return;
  }
  // 8-byte form, and the odd last element of the 16-byte form on one lane
  const int64_t lo = VEC ? n - 1 : (int64_t)blockIdx.x * TB + threadIdx.x;
  for (int64_t i = lo; i < n; i += stride) {
    double s[MGS_VECS_MAX];
#pragma unroll
    for (int a = 0; a < MGS_VECS_MAX; ++a) if (a < k) s[a] = T.s[a][i];
    asm volatile("" ::: "memory");
    for (int j = 0; j < q; ++j) {
      double y = cs[j] * s[0];
#pragma unroll
      for (int a = 1; a < MGS_VECS_MAX; ++a) if (a < k) y = y + cs[a * q + j] * s[a];
      T.y[j][i] = y;
    }
  }
}

int ensure_slot(mgs_ctx *ctx) {
  if (ctx->vecs_dev) return MGS_OK;
  MGS_HIP(ctx, hipHostMalloc((void **)&ctx->vecs_host, sizeof(double) * MGS_VECS_RING * COEF_DOUBLES, hipHostMallocDefault));
  return mgs_dev_alloc(ctx, &ctx->vecs_dev, (size_t)VECS_DEV_DOUBLES);
}
// The caller's k·q coefficients into the device slot.  They are copied into a pinned slot of the context's ring before this returns — the caller may
// reuse or free its array at once — and the device copy reads that slot; a slot is written again only after the copy that read it last has run.
int stage_coefficients(mgs_ctx *ctx, const double *C, int count, double *coef_dev) {
  const int slot = ctx->vecs_next;
  ctx->vecs_next = (slot + 1) % MGS_VECS_RING;
  if (ctx->vecs_ev[slot]) MGS_HIP(ctx, hipEventSynchronize(ctx->vecs_ev[slot]));
  else MGS_HIP(ctx, hipEventCreateWithFlags(&ctx->vecs_ev[slot], hipEventDisableTiming));
  double *host = ctx->vecs_host + (size_t)slot * COEF_DOUBLES;
  memcpy(host, C, sizeof(double) * (size_t)count);
  MGS_HIP(ctx, hipMemcpyAsync(coef_dev, host, sizeof(double) * (size_t)count, hipMemcpyHostToDevice, ctx->stream));
  MGS_HIP(ctx, hipEventRecord(ctx->vecs_ev[slot], ctx->stream));
  return MGS_OK;
}
// a list of p columns of at least n entries on ctx, none NULL
int check_cols(mgs_ctx *ctx, const char *who, const char *name, int64_t n, int p, const mgs_vec *const *L) {
  for (int a = 0; a < p; ++a) {
    MGS_CHECK(ctx, L[a] && L[a]->d, MGS_ERR_INVALID, "%s: %s[%d] is NULL", who, name, a);
    MGS_CHECK(ctx, L[a]->ctx == ctx, MGS_ERR_INVALID, "%s: %s[%d] belongs to another context", who, name, a);
    MGS_CHECK(ctx, L[a]->n >= n, MGS_ERR_INVALID, "%s: %s[%d] holds %lld entries, n = %lld", who, name, a, (long long)L[a]->n, (long long)n);
  }
  return MGS_OK;
}
}   // namespace

extern "C" {

int mgs_vecs_gram(mgs_ctx *ctx, int64_t n, int p, const mgs_vec *const *U, int q, const mgs_vec *const *V, double *G) {
  MGS_CHECK(nullptr, ctx, MGS_ERR_INVALID, "mgs_vecs_gram: NULL context");
  MGS_CHECK(ctx, U && V && G, MGS_ERR_INVALID, "mgs_vecs_gram: NULL argument");
  MGS_CHECK(ctx, p >= 1 && p <= MGS_VECS_MAX && q >= 1 && q <= MGS_VECS_MAX, MGS_ERR_INVALID, "mgs_vecs_gram: %d x %d columns (1..%d each)", p, q, MGS_VECS_MAX);
  MGS_CHECK(ctx, n >= 1, MGS_ERR_INVALID, "mgs_vecs_gram: n = %lld", (long long)n);
  MGS_TRY(check_cols(ctx, "mgs_vecs_gram", "U", n, p, U));
  MGS_TRY(check_cols(ctx, "mgs_vecs_gram", "V", n, q, V));
  MGS_TRY(ensure_slot(ctx));
  bool vec = ctx->opt_blas1_vec && n >= 2, sym = p == q;
  for (int a = 0; a < p; ++a) vec = vec && al16(U[a]->d);
  for (int b = 0; b < q; ++b) vec = vec && al16(V[b]->d);
  for (int a = 0; a < p && sym; ++a) sym = U[a]->d == V[a]->d;
  const int64_t work = vec ? n / 2 : n;
  const int nb = (int)std::min<int64_t>(std::max<int64_t>((work + TB - 1) / TB, 1), GRAM_BLOCKS);
  MGS_TRY(mgs_ensure_dot_part(ctx, (int64_t)GT * GT * nb));
  int tiles = 0;
  for (int a0 = 0; a0 < p; a0 += GT) {
    for (int b0 = sym ? a0 : 0; b0 < q; b0 += GT) {      // the same list on both sides: tiles on and above the diagonal, mirrored below
      const int tp = std::min(GT, p - a0), tq = std::min(GT, q - b0);
      GramCols T;
      for (int a = 0; a < GT; ++a) T.u[a] = U[a0 + std::min(a, tp - 1)]->d;
      for (int b = 0; b < GT; ++b) T.v[b] = V[b0 + std::min(b, tq - 1)]->d;
      if (vec) hipLaunchKernelGGL(gram_tile_kernel<true>, dim3(nb), dim3(TB), 0, ctx->stream, n, tp, tq, T, ctx->dot_part);
      else hipLaunchKernelGGL(gram_tile_kernel<false>, dim3(nb), dim3(TB), 0, ctx->stream, n, tp, tq, T, ctx->dot_part);
      hipLaunchKernelGGL(gram_final_kernel, dim3(tp * tq), dim3(TB), 0, ctx->stream, nb, tq, a0, b0, q, ctx->dot_part, ctx->vecs_dev);
      ++tiles;
    }
  }
  MGS_HIP(ctx, hipGetLastError());
  MGS_HIP(ctx, hipMemcpyAsync(G, ctx->vecs_dev, sizeof(double) * (size_t)p * q, hipMemcpyDeviceToHost, ctx->stream));
  MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (sym)
    for (int a = 0; a < p; ++a)
      for (int b = 0; b < a; ++b)
        if (a / GT != b / GT) G[(size_t)a * q + b] = G[(size_t)b * q + a];
  const int64_t info[8] = {nb, std::min(GT, p), std::min(GT, q), vec ? 1 : 0, tiles, sym ? 1 : 0, 1, 0};
  memcpy(ctx->vecs_info, info, sizeof info);
  return MGS_OK;
}

int mgs_vecs_combine(mgs_ctx *ctx, int64_t n, int k, const mgs_vec *const *S, int q, mgs_vec *const *Y, const double *C) {
  MGS_CHECK(nullptr, ctx, MGS_ERR_INVALID, "mgs_vecs_combine: NULL context");
  MGS_CHECK(ctx, S && Y && C, MGS_ERR_INVALID, "mgs_vecs_combine: NULL argument");
  MGS_CHECK(ctx, k >= 1 && k <= MGS_VECS_MAX && q >= 1 && q <= 16, MGS_ERR_INVALID, "mgs_vecs_combine: %d inputs (1..%d), %d outputs (1..16)", k, MGS_VECS_MAX, q);
  MGS_CHECK(ctx, n >= 1, MGS_ERR_INVALID, "mgs_vecs_combine: n = %lld", (long long)n);
  MGS_TRY(check_cols(ctx, "mgs_vecs_combine", "S", n, k, S));
  MGS_TRY(check_cols(ctx, "mgs_vecs_combine", "Y", n, q, Y));
  auto overlap = [n](const double *a, const double *b) { return a < b + n && b < a + n; };
  for (int j = 0; j < q; ++j) {
    for (int i = 0; i < j; ++i)
      MGS_CHECK(ctx, !overlap(Y[i]->d, Y[j]->d), MGS_ERR_INVALID, "mgs_vecs_combine: outputs %d and %d %s", i, j, Y[i]->d == Y[j]->d ? "are the same vector" : "overlap");
    for (int a = 0; a < k; ++a)
      MGS_CHECK(ctx, Y[j]->d == S[a]->d || !overlap(Y[j]->d, S[a]->d), MGS_ERR_INVALID, "mgs_vecs_combine: output %d overlaps input %d partially", j, a);
  }
  MGS_TRY(ensure_slot(ctx));
  double *coef = ctx->vecs_dev + COEF_SLOT;
  MGS_TRY(stage_coefficients(ctx, C, k * q, coef));
  bool vec = ctx->opt_blas1_vec && n >= 2;
  CombineCols T;
  for (int a = 0; a < MGS_VECS_MAX; ++a) { T.s[a] = S[std::min(a, k - 1)]->d; if (a < k) vec = vec && al16(S[a]->d); }
  for (int j = 0; j < 16; ++j) { T.y[j] = Y[std::min(j, q - 1)]->d; if (j < q) vec = vec && al16(Y[j]->d); }
  const int64_t work = vec ? n / 2 : n;
  const int nb = (int)std::min<int64_t>(std::max<int64_t>((work + TB - 1) / TB, 1), 1 << 20);
  if (vec) hipLaunchKernelGGL(combine_kernel<true>, dim3(nb), dim3(TB), 0, ctx->stream, n, k, q, T, coef);
  else hipLaunchKernelGGL(combine_kernel<false>, dim3(nb), dim3(TB), 0, ctx->stream, n, k, q, T, coef);
  MGS_HIP(ctx, hipGetLastError());
  const int64_t info[8] = {nb, k, q, vec ? 1 : 0, 1, 0, 2, 0};
  memcpy(ctx->vecs_info, info, sizeof info);
  return MGS_OK;
}

int mgs_vecs_info(const mgs_ctx *ctx, int64_t out[8]) {
  MGS_CHECK(nullptr, ctx && out, MGS_ERR_INVALID, "mgs_vecs_info: NULL argument");
  memcpy(out, ctx->vecs_info, sizeof ctx->vecs_info);
  return MGS_OK;
}

}   // extern "C"
