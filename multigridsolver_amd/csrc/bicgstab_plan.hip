// bicgstab_plan.hip — BiCGSTAB whose scalars never leave the device (mgs_bicgstab_plan, include/mgs.h).
// Reference: BiCGSTABiml, src/common/bicg.cpp:74-136; the reference has no asynchronous form.
//
// mgs_bicgstab (mgs_api.hip) computes ρ, α, ω, β and three stopping tests on the host: four host looks per iteration (r̃·v → α; ‖s‖; (t·s, t·t)
// → ω; ‖r‖ and the next ρ), each one draining the queue behind it.  Here the same scalars live in one state block in device memory, as
// pcg_plan.hip keeps mgs_pcg's.  One-wave "scalar step" kernels turn the folded inner products the reductions leave in red_dev[MGS_DOT_BLOCKS ..]
// into the next scalars with the very operations the host uses (α = ρ/(r̃·v), ω = (t·s)/(t·t), β = (ρ/ρ_prev)·(α/ω), resid = √(·)/‖b‖ — no
// fast-math in this build, FP64 division and sqrt are correctly rounded), and the vector passes take their coefficients from the state block
// instead of from kernel arguments.  Every pass evaluates the expression of the kernel mgs_bicgstab runs (a·x + b·y (+ c·z), unfused), the passes
// with sums take k_update_dot2's launch decisions, and everything else is the launches mgs_bicgstab makes — the cycle, the projection, the SpMV
// with its dot epilogue, called with a NULL host pointer.  So the bits of every vector agree with mgs_bicgstab's.
//
// One iteration is a fixed launch sequence (bicg.cpp lines in brackets):
//   RHO [:95-99, :103] · p-pass [:100-104] · cycle p → p̂ [:106] · SpMV with r̃·v + fold [:107] · ALPHA [:108] · s-pass + fold [:109] · HALF [:110]
//   · cycle s → ŝ [:116] · SpMV with (t·s, t·t) + fold [:117] · OMEGA [:118] · x-pass [:119, :111 at the half step] · r-pass + fold [:120] · RES [:122-131]
// A solve that converges or breaks down sets `frozen`; from then on every scalar step is a no-op (RHO counts into `wasted`) and every
// workgroup of the four vector passes returns before it touches a vector — except the x-pass of the iteration that converged at its half
// step, which applies x ← α·p̂ + x (`half`).  Cycles, SpMVs and folds of a frozen iteration still run; they write p̂, ŝ, v, t and scratch only.
//
// RES (and INIT) also post (iteration, status, frozen, wasted, resid, ‖b‖) and a ticket into a ring of slots in mapped, coherent host memory.
// mgs_bicgstab_plan_solve looks at one slot per iteration, `ahead` iterations behind the queue; mgs_bicgstab_plan_enqueue never looks.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <deque>
#include <time.h>

#include "mgs_internal.hpp"

namespace {
constexpr int PTB = 256;                 // lanes per workgroup of the vector passes (the BLAS-1 kernels' TB)
constexpr int RING = 1024;               // posted slots; at most RING − 1 posts are outstanding, so no slot is rewritten before the host has read it
constexpr int RED = MGS_DOT_BLOCKS;      // red_dev[RED], red_dev[RED + 1]: what the last fold left
typedef double bd2 __attribute__((ext_vector_type(2)));

// the state block.  status: −1 running, 0 converged (by the recursion, as mgs_bicgstab decides), 2 ρ = 0, 3 ω = 0; after FINAL: see STEP_FINAL
struct BcgState {
  double normb, rho, rho_next, rho_prev, alpha, omega, beta, nbo /* −β·ω */, rtv, ts, tt, ss, rr, resid, true_resid;
  int it;        // the last iteration that ran unfrozen (the one that froze, once frozen)
  int status;
  int frozen;
  int first;     // the next direction is p = r
  int half;      // frozen at the half step of the running iteration: its x-pass still owes x ← α·p̂ + x
  int wasted;    // iterations that ran frozen
};
struct BcgSlot {   // 64 bytes of mapped host memory
  unsigned long long ticket;
  double resid, normb;
  int it, status, frozen, wasted;
  unsigned long long pad[3];
};
static_assert(sizeof(BcgSlot) == 64, "one slot per 64 bytes");

enum { STEP_NORMB = 0, STEP_INIT, STEP_RHO, STEP_ALPHA, STEP_HALF, STEP_OMEGA, STEP_RES, STEP_FINAL };

__device__ __forceinline__ void post_slot(BcgSlot *s, const BcgState *st, unsigned long long ticket) {
  __hip_atomic_store(&s->resid, st->resid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&s->normb, st->normb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&s->it, st->it, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&s->status, st->status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&s->frozen, st->frozen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&s->wasted, st->wasted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&s->ticket, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The scalar steps: one wave, lane 0 works.  red = ctx->red_dev + RED.  `it`: the iteration the step belongs to (FINAL: the iterations
// enqueued); `tol`: the tolerance (INIT, HALF, RES, FINAL); slot = NULL: nothing is posted.
__global__ void bcgp_step_kernel(int step, BcgState *__restrict__ st, const double *__restrict__ red, int it, double tol, BcgSlot *slot, unsigned long long ticket) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  switch (step) {
    case STEP_NORMB: {                      // :80, :85-86  ‖b‖ (‖Πb‖), 0 replaced by 1; a fresh state
      double nb = sqrt(red[0]);
      if (nb == 0.0) nb = 1.0;
      st->normb = nb;
      st->rho = st->rho_next = st->rho_prev = st->alpha = st->omega = st->beta = st->nbo = st->rtv = st->ts = st->tt = st->ss = st->rr = 0.0;
      st->resid = st->true_resid = 0.0;
      st->it = 0; st->status = -1; st->frozen = 0; st->first = 1; st->half = 0; st->wasted = 0;
      break;
    }
    case STEP_INIT: {                       // :88-92  red = (‖r‖², r̃·r)
      st->rr = red[0]; st->rho_next = red[1];
      st->resid = sqrt(red[0]) / st->normb;
      if (st->resid <= tol) { st->frozen = 1; st->status = 0; }
      if (slot) post_slot(slot, st, ticket);
      break;
    }
    case STEP_RHO: {                        // :95-99, :103
      if (st->frozen) { st->wasted += 1; break; }
      st->it = it;
      st->rho = st->rho_next;
      if (st->rho == 0) { st->frozen = 1; st->status = 2; break; }            // resid keeps √rr/‖b‖, the value :96-99 reports
      if (!st->first) {
        st->beta = (st->rho / st->rho_prev) * (st->alpha / st->omega);
        st->nbo = -st->beta * st->omega;
      }
      break;
    }
    case STEP_ALPHA: {                      // :108  no test for zero: a non-finite α propagates as in mgs_bicgstab
      if (st->frozen) break;
      st->rtv = red[0];
      st->alpha = st->rho / st->rtv;
      break;
    }
    case STEP_HALF: {                       // :110
      if (st->frozen) break;
      st->ss = red[0];
      st->resid = sqrt(red[0]) / st->normb;
      if (st->resid < tol) { st->frozen = 1; st->status = 0; st->half = 1; }
      break;
    }
    case STEP_OMEGA: {                      // :118
      if (st->frozen) break;
      st->ts = red[0]; st->tt = red[1];
      st->omega = st->ts / st->tt;
      break;
    }
    case STEP_RES: {                        // :122-131  red = (‖r‖², r̃·r)
      st->half = 0;                         // the x-pass in front of this step has paid the half step
      if (!st->frozen) {
        st->rr = red[0]; st->rho_next = red[1];
        st->rho_prev = st->rho; st->first = 0;
        st->resid = sqrt(red[0]) / st->normb;
        if (st->resid < tol) { st->frozen = 1; st->status = 0; }
        else if (st->omega == 0) { st->frozen = 1; st->status = 3; }
      }
      if (slot) post_slot(slot, st, ticket);
      break;
    }
    case STEP_FINAL: {                      // after the projection of x and t = b − A·x: red[0] = ‖t‖²
      st->true_resid = sqrt(red[0]) / st->normb;
      if (!st->frozen) { st->it = it; st->status = 1; }
      else if (st->status == 0) st->status = (st->it == 0 ? st->true_resid <= tol : st->true_resid < tol) ? 0 : 1;
      st->frozen = 1;
      break;
    }
  }
}

__device__ __forceinline__ void bst2(bd2 *p, bd2 v, bool nt) {      // streaming store, as st2 in kernels_aux.hip
  if (nt) asm volatile("global_store_dwordx4 %0, %1, off nt" : : "v"(p), "v"(v) : "memory");
  else *p = v;
}

// p-pass (:100-104): first: p ← r; else p = 1.0·r + nbo·v + beta·p, axpbypcz_kernel's expression with its c == 0.0 branch (which does not read p).
// The state is read once per workgroup through uniform loads; a frozen workgroup returns at once.
__global__ __launch_bounds__(PTB) void bcgp_p_vec_kernel(int64_t n, const BcgState *__restrict__ st, const double *__restrict__ r, const double *__restrict__ v,
                                                         double *__restrict__ p, int nts) {
  if (st->frozen) return;
  const bool first = st->first != 0;
  const double b = st->nbo, c = st->beta;
  const int64_t n2 = n >> 1;
  const bd2 *__restrict__ rv = reinterpret_cast<const bd2 *>(r);
  const bd2 *__restrict__ vv = reinterpret_cast<const bd2 *>(v);
  bd2 *__restrict__ pv = reinterpret_cast<bd2 *>(p);
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x; i < n2; i += stride) {
    const bd2 ri = rv[i]; bd2 q;
    if (first) q = ri;
    else {
      const bd2 o = vv[i];
      if (c == 0.0) { q.x = 1.0 * ri.x + b * o.x; q.y = 1.0 * ri.y + b * o.y; }
      else { const bd2 w = pv[i]; q.x = 1.0 * ri.x + b * o.x + c * w.x; q.y = 1.0 * ri.y + b * o.y + c * w.y; }
    }
    bst2(pv + i, q, nts != 0);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t k = n - 1;
    if (first) p[k] = r[k];
    else p[k] = c == 0.0 ? 1.0 * r[k] + b * v[k] : 1.0 * r[k] + b * v[k] + c * p[k];
  }
}
__global__ __launch_bounds__(PTB) void bcgp_p_kernel(int64_t n, const BcgState *__restrict__ st, const double *__restrict__ r, const double *__restrict__ v,
                                                     double *__restrict__ p) {
  if (st->frozen) return;
  const bool first = st->first != 0;
  const double b = st->nbo, c = st->beta;
  int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (; i < n; i += stride) {
    if (first) p[i] = r[i];
    else p[i] = c == 0.0 ? 1.0 * r[i] + b * v[i] : 1.0 * r[i] + b * v[i] + c * p[i];
  }
}

// x-pass (:119): x = alpha·p̂ + omega·ŝ + 1.0·x (axpbypcz_kernel's expression); frozen with `half` (:111): x = alpha·p̂ + 1.0·x (axpby_kernel's);
// frozen without: return at once.
__global__ __launch_bounds__(PTB) void bcgp_x_vec_kernel(int64_t n, const BcgState *__restrict__ st, const double *__restrict__ ph, const double *__restrict__ sh,
                                                         double *__restrict__ x, int nts) {
  const bool frozen = st->frozen != 0;
  if (frozen && !st->half) return;
  const double a = st->alpha, b = st->omega;
  const int64_t n2 = n >> 1;
  const bd2 *__restrict__ pv = reinterpret_cast<const bd2 *>(ph);
  const bd2 *__restrict__ sv = reinterpret_cast<const bd2 *>(sh);
  bd2 *__restrict__ xv = reinterpret_cast<bd2 *>(x);
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x; i < n2; i += stride) {
    const bd2 pi = pv[i], xi = xv[i]; bd2 q;
    if (frozen) { q.x = a * pi.x + 1.0 * xi.x; q.y = a * pi.y + 1.0 * xi.y; }
    else { const bd2 si = sv[i]; q.x = a * pi.x + b * si.x + 1.0 * xi.x; q.y = a * pi.y + b * si.y + 1.0 * xi.y; }
    bst2(xv + i, q, nts != 0);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t k = n - 1;
    x[k] = frozen ? a * ph[k] + 1.0 * x[k] : a * ph[k] + b * sh[k] + 1.0 * x[k];
  }
}
__global__ __launch_bounds__(PTB) void bcgp_x_kernel(int64_t n, const BcgState *__restrict__ st, const double *__restrict__ ph, const double *__restrict__ sh,
                                                     double *__restrict__ x) {
  const bool frozen = st->frozen != 0;
  if (frozen && !st->half) return;
  const double a = st->alpha, b = st->omega;
  int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (; i < n; i += stride) x[i] = frozen ? a * ph[i] + 1.0 * x[i] : a * ph[i] + b * sh[i] + 1.0 * x[i];
}

// s-pass (:109, OMEGA = false: z = s, x = r, y = v, coefficient −alpha, no w) and r-pass (:120, OMEGA = true: z = r, x = s, y = t, coefficient −omega,
// w = r̃): z = 1.0·x + (−c)·y with the partial pairs (z·z, w·z) of update_dot2_partial_vec_kernel / update_dot2_partial_kernel — the same
// per-element expression, the same order of additions per lane, the same layout [2][gridDim.x].  Frozen: z and the partials stay as they
// are; the scalar step behind the fold ignores it.
template <bool OMEGA>
__global__ __launch_bounds__(PTB) void bcgp_upd_vec_kernel(int64_t n, const BcgState *__restrict__ st, const double *__restrict__ x, const double *__restrict__ y,
                                                           double *__restrict__ z, const double *__restrict__ w, double *__restrict__ part, int nts) {
  if (st->frozen) return;
  const double a = 1.0, b = OMEGA ? -st->omega : -st->alpha;
  __shared__ double sh[2][PTB / 64];
  const int64_t n2 = n >> 1;
  const bd2 *__restrict__ xv = reinterpret_cast<const bd2 *>(x);
  const bd2 *__restrict__ yv = reinterpret_cast<const bd2 *>(y);
  const bd2 *__restrict__ wv = reinterpret_cast<const bd2 *>(w);
  bd2 *__restrict__ zv = reinterpret_cast<bd2 *>(z);
  double s0 = 0.0, s1 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x; i < n2; i += stride) {
    const bd2 p = xv[i], o = yv[i]; bd2 q;
    q.x = a * p.x + b * o.x; q.y = a * p.y + b * o.y;
    bst2(zv + i, q, nts != 0);
    s0 += q.x * q.x; s0 += q.y * q.y;
    if (OMEGA) { const bd2 ww = wv[i]; s1 += ww.x * q.x; s1 += ww.y * q.y; }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double zi = a * x[n - 1] + b * y[n - 1];
    z[n - 1] = zi; s0 += zi * zi;
    if (OMEGA) s1 += w[n - 1] * zi;
  }
  for (int off = 32; off > 0; off >>= 1) { s0 += __shfl_down(s0, off); s1 += __shfl_down(s1, off); }
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s0; sh[1][threadIdx.x >> 6] = s1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t0 = 0.0, t1 = 0.0;
    for (int q = 0; q < PTB / 64; ++q) { t0 += sh[0][q]; t1 += sh[1][q]; }
    part[blockIdx.x] = t0; part[gridDim.x + blockIdx.x] = t1;
  }
}
template <bool OMEGA>
__global__ __launch_bounds__(PTB) void bcgp_upd_kernel(int64_t n, const BcgState *__restrict__ st, const double *__restrict__ x, const double *__restrict__ y,
                                                       double *__restrict__ z, const double *__restrict__ w, double *__restrict__ part) {
  if (st->frozen) return;
  const double a = 1.0, b = OMEGA ? -st->omega : -st->alpha;
  __shared__ double sh[2][PTB / 64];
  double s0 = 0.0, s1 = 0.0;
  int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (; i < n; i += stride) {
    const double zi = a * x[i] + b * y[i];
    z[i] = zi;
    s0 += zi * zi;
    if (OMEGA) s1 += w[i] * zi;
  }
  for (int off = 32; off > 0; off >>= 1) { s0 += __shfl_down(s0, off); s1 += __shfl_down(s1, off); }
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s0; sh[1][threadIdx.x >> 6] = s1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t0 = 0.0, t1 = 0.0;
    for (int q = 0; q < PTB / 64; ++q) { t0 += sh[0][q]; t1 += sh[1][q]; }
    part[blockIdx.x] = t0; part[gridDim.x + blockIdx.x] = t1;
  }
}

inline bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}   // namespace

struct mgs_bicgstab_plan {
  mgs_ctx *ctx = nullptr;
  const mgs_csr *A = nullptr;
  mgs_hier *h = nullptr;
  bool ns = false;
  int n = 0;
  double *block = nullptr;            // p, p̂, s, ŝ, t, v, r, r̃ (stride doubles each), then the state
  int64_t stride = 0, bytes = 0;
  mgs_vec p, ph, s, sh, t, v, r, rt;  // views into block
  BcgState *st = nullptr;
  BcgSlot *ring = nullptr, *ring_dev = nullptr;       // RING slots, then one BcgState the result is copied into (mapped, coherent host memory)
  BcgState *snap = nullptr;
  unsigned long long seq = 0;         // ticket of the last posting step enqueued
  // what info and result report
  int64_t calls = 0, enq_iters = 0, wasted = 0, waits = 0;
  bool unread = false;                // an enqueue whose result has not been read yet
  int res_it = 0, res_status = 1; double res_resid = 0.0, res_rec = 0.0;
};

namespace {
struct Look { int it, status, frozen, wasted; double resid, normb; };

int step(mgs_bicgstab_plan *P, int which, int it, double tol, bool post) {
  mgs_ctx *ctx = P->ctx;
  BcgSlot *slot = nullptr;
  if (post) { ++P->seq; slot = P->ring_dev + (P->seq % RING); }
  hipLaunchKernelGGL(bcgp_step_kernel, dim3(1), dim3(64), 0, ctx->stream, which, P->st, ctx->red_dev + RED, it, tol, slot, P->seq);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
inline int nts_of(const mgs_ctx *ctx, int64_t n) { return ctx->opt_nt_store > 0 && n >= ctx->opt_nt_store; }

int launch_p(mgs_bicgstab_plan *P) {
  mgs_ctx *ctx = P->ctx; const int64_t n = P->n;
  if (ctx->opt_blas1_vec)
    hipLaunchKernelGGL(bcgp_p_vec_kernel, dim3(mgs_blas1_grid(ctx, (n + 1) / 2)), dim3(PTB), 0, ctx->stream, n, P->st, P->r.d, P->v.d, P->p.d, nts_of(ctx, n));
  else
    hipLaunchKernelGGL(bcgp_p_kernel, dim3(mgs_blas1_grid_capped(ctx, n)), dim3(PTB), 0, ctx->stream, n, P->st, P->r.d, P->v.d, P->p.d);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int launch_x(mgs_bicgstab_plan *P, double *x) {
  mgs_ctx *ctx = P->ctx; const int64_t n = P->n;
  if (ctx->opt_blas1_vec && al16(x))
    hipLaunchKernelGGL(bcgp_x_vec_kernel, dim3(mgs_blas1_grid(ctx, (n + 1) / 2)), dim3(PTB), 0, ctx->stream, n, P->st, P->ph.d, P->sh.d, x, nts_of(ctx, n));
  else
    hipLaunchKernelGGL(bcgp_x_kernel, dim3(mgs_blas1_grid_capped(ctx, n)), dim3(PTB), 0, ctx->stream, n, P->st, P->ph.d, P->sh.d, x);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
// the grids, the partial buffer, the store rule and the fold of k_update_dot2 (the plan's vectors are 256-byte aligned: the 16-byte form whenever
// option blas1_vec is on, as the work vectors of mgs_bicgstab get it)
template <bool OMEGA>
int launch_upd(mgs_bicgstab_plan *P, const double *x, const double *y, double *z, const double *w) {
  mgs_ctx *ctx = P->ctx; const int64_t n = P->n;
  int nb = (int)((n + PTB - 1) / PTB);
  if (nb > MGS_DOT_BLOCKS / 2) nb = MGS_DOT_BLOCKS / 2;
  if (nb < 1) nb = 1;
  if (ctx->opt_blas1_vec) {
    nb = mgs_blas1_grid(ctx, (n + 1) / 2);
    double *part = ctx->red_dev;
    if (nb > MGS_DOT_BLOCKS / 2) { MGS_TRY(mgs_ensure_dot_part(ctx, 2 * (int64_t)nb)); part = ctx->dot_part; }
    hipLaunchKernelGGL(bcgp_upd_vec_kernel<OMEGA>, dim3(nb), dim3(PTB), 0, ctx->stream, n, P->st, x, y, z, w, part, nts_of(ctx, n));
    MGS_HIP(ctx, hipGetLastError());
    return k_dot2_finish(ctx, nb, part, nullptr);
  }
  hipLaunchKernelGGL(bcgp_upd_kernel<OMEGA>, dim3(nb), dim3(PTB), 0, ctx->stream, n, P->st, x, y, z, w, ctx->red_dev);
  MGS_HIP(ctx, hipGetLastError());
  return k_dot2_finish(ctx, nb, ctx->red_dev, nullptr);
}
// M.solve (:106, :116): the cycle (or a copy), projected when the null space is declared; not predicated
int precond(mgs_bicgstab_plan *P, const mgs_vec *in, mgs_vec *out) {
  if (P->h) MGS_TRY(mgs_vcycle(P->h, in, out, 1)); else MGS_TRY(mgs_vec_copy(in, out));
  return P->ns ? k_project_const(P->ctx, P->n, out->d) : MGS_OK;
}
// INIT (:80-92): ‖b‖ (‖Πb‖), r = b − A·x (projected), r̃ ← r, (‖r‖², r̃·r), the freeze with (status 0, it 0) when the residual is within tol already
int enqueue_init(mgs_bicgstab_plan *P, const mgs_vec *xv, const mgs_vec *bv, double tol, bool post) {
  mgs_ctx *ctx = P->ctx; const int64_t n = P->n;
  if (P->ns) MGS_TRY(k_const_dev_nrm2_fold(ctx, n, bv->d)); else MGS_TRY(k_dot(ctx, n, bv->d, bv->d, nullptr));
  MGS_TRY(step(P, STEP_NORMB, 0, 0.0, false));
  MGS_TRY(mgs_residual(P->A, xv, bv, &P->r));
  if (P->ns) MGS_TRY(k_project_const(ctx, n, P->r.d));
  MGS_TRY(mgs_vec_copy(&P->r, &P->rt));
  MGS_TRY(k_dot2(ctx, n, P->r.d, P->r.d, P->rt.d, P->r.d, nullptr));
  return step(P, STEP_INIT, 0, tol, post);
}
int enqueue_iteration(mgs_bicgstab_plan *P, mgs_vec *xv, int it, double tol, bool post) {
  MGS_TRY(step(P, STEP_RHO, it, 0.0, false));
  MGS_TRY(launch_p(P));
  MGS_TRY(precond(P, &P->p, &P->ph));
  MGS_TRY(mgs_spmv_dots(P->A, P->ph.d, P->v.d, P->rt.d, nullptr));                  // v = A·p̂ with r̃·v from the same pass
  MGS_TRY(step(P, STEP_ALPHA, it, 0.0, false));
  MGS_TRY(launch_upd<false>(P, P->r.d, P->v.d, P->s.d, nullptr));                   // s = r − αv with ‖s‖²
  MGS_TRY(step(P, STEP_HALF, it, tol, false));
  MGS_TRY(precond(P, &P->s, &P->sh));
  MGS_TRY(mgs_spmv_dots(P->A, P->sh.d, P->t.d, P->s.d, nullptr));                   // t = A·ŝ with (t·s, t·t) from the same pass
  MGS_TRY(step(P, STEP_OMEGA, it, 0.0, false));
  MGS_TRY(launch_x(P, xv->d));
  MGS_TRY(launch_upd<true>(P, P->s.d, P->t.d, P->r.d, P->rt.d));                    // r = s − ωt with ‖r‖² and the next r̃·r
  P->enq_iters++;
  return step(P, STEP_RES, it, tol, post);
}
// wait until the post with ticket `want` is visible (no slot is rewritten before it has been read: see RING)
int wait_post(mgs_bicgstab_plan *P, unsigned long long want, Look *out) {
  mgs_ctx *ctx = P->ctx;
  BcgSlot *s = P->ring + (want % RING);
  P->waits++;
  const auto t0 = std::chrono::steady_clock::now();
  double next_query = 2e-3;
  for (;;) {
    if (__atomic_load_n(&s->ticket, __ATOMIC_ACQUIRE) == want) break;
    const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (waited < 300e-6) { for (int k = 0; k < 8; ++k) __builtin_ia32_pause(); continue; }
    if (waited > next_query) {           // a queue that has drained (or failed) without the ticket will never deliver it
      next_query = waited + 2e-3;
      const hipError_t e = hipStreamQuery(ctx->stream);
      if (e == hipSuccess) {
        if (__atomic_load_n(&s->ticket, __ATOMIC_ACQUIRE) == want) break;
        return mgs_fail(ctx, MGS_ERR_HIP, "mgs_bicgstab_plan: posted results never reached the host ring");
      }
      if (e != hipErrorNotReady) return mgs_fail(ctx, MGS_ERR_HIP, "mgs_bicgstab_plan: %s", hipGetErrorString(e));
    }
    struct timespec ts = {0, 25000}; nanosleep(&ts, nullptr);
  }
  out->it = s->it; out->status = s->status; out->frozen = s->frozen; out->wasted = s->wasted; out->resid = s->resid; out->normb = s->normb;
  return MGS_OK;
}
int check_call(mgs_bicgstab_plan *P, const mgs_vec *x, const mgs_vec *b, const char *who) {
  mgs_ctx *ctx = P->ctx;
  MGS_CHECK(ctx, x->n >= P->n && b->n >= P->n, MGS_ERR_INVALID, "%s: vectors of %lld and %lld entries, the operator has %d rows", who, (long long)x->n, (long long)b->n, P->n);
  MGS_CHECK(ctx, x->d != b->d, MGS_ERR_INVALID, "%s: x must not alias b", who);
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  MGS_HIP(ctx, hipStreamIsCapturing(ctx->stream, &cs));
  MGS_CHECK(ctx, cs == hipStreamCaptureStatusNone, MGS_ERR_STATE, "%s: the context's stream is being captured", who);
  return MGS_OK;
}
}   // namespace

int mgs_bicgstab_plan_destroy(mgs_bicgstab_plan *P) {
  if (!P) return MGS_OK;
  if (P->block || P->ring) hipStreamSynchronize(P->ctx->stream);
  if (P->block) mgs_hip_free(P->block);
  if (P->ring) hipHostFree(P->ring);
  delete P;
  return MGS_OK;
}

int mgs_bicgstab_plan_create(const mgs_csr *A, mgs_hier *h, mgs_bicgstab_plan **out) {
  mgs_ctx *ctx = A ? A->ctx : (h ? h->ctx : nullptr);
  MGS_CHECK(ctx, A && out, MGS_ERR_INVALID, "mgs_bicgstab_plan_create: NULL argument");
  MGS_CHECK(ctx, A->rows == A->cols && !ctx->ncomm && !ctx->allreduce, MGS_ERR_INVALID, "mgs_bicgstab_plan_create: the matrix is %d x %d%s (row shards are served by mgs_bicgstab)",
            A->rows, A->cols, A->cols > A->rows ? ", halo columns: a row shard" : (A->rows == A->cols ? ", on a context that sums over ranks" : ", not square"));
  MGS_CHECK(ctx, A->rows > 0, MGS_ERR_INVALID, "mgs_bicgstab_plan_create: the matrix has no rows");
  if (h) {
    bool shard = h->halo || h->halo_begin || h->halo_end || h->halo_fused || h->coarse || h->native || h->ntail;
    for (const mgs_level &L : h->lev) shard = shard || L.nx || (L.A && L.A->cols > L.A->rows);
    MGS_CHECK(ctx, !shard, MGS_ERR_INVALID, "mgs_bicgstab_plan_create: the hierarchy has halo columns, exchange callbacks, native plans or a tail (row shards are served by mgs_bicgstab)");
    MGS_CHECK(ctx, h->ctx == ctx && !h->lev.empty() && h->lev[0].n == A->rows, MGS_ERR_INVALID, "mgs_bicgstab_plan_create: the hierarchy's fine level has %d rows, A has %d",
              h->lev.empty() ? 0 : h->lev[0].n, A->rows);
    MGS_CHECK(ctx, h->finalized, MGS_ERR_STATE, "mgs_bicgstab_plan_create: call mgs_hier_finalize first");
  }
  bool ns = false;
  MGS_TRY(mgs_krylov_nullspace(A, h, "mgs_bicgstab_plan_create", &ns));
  MGS_TRY(mgs_csr_optimize(const_cast<mgs_csr *>(A)));
  mgs_bicgstab_plan *P = new mgs_bicgstab_plan();
  P->ctx = ctx; P->A = A; P->h = h; P->ns = ns; P->n = A->rows;
  P->stride = (((int64_t)P->n + 31) / 32) * 32;                                          // every vector 256-byte aligned
  const size_t nstate = (sizeof(BcgState) + 255) / 256 * 32;                             // doubles
  const size_t ndoubles = (size_t)8 * P->stride + nstate;
  int rc = mgs_dev_alloc(ctx, &P->block, ndoubles);
  if (rc == MGS_OK && hipMemsetAsync(P->block, 0, sizeof(double) * ndoubles, ctx->stream) != hipSuccess) rc = mgs_fail(ctx, MGS_ERR_HIP, "mgs_bicgstab_plan_create: hipMemsetAsync failed");
  if (rc == MGS_OK) {
    const size_t hb = sizeof(BcgSlot) * RING + 256;
    if (hipHostMalloc((void **)&P->ring, hb, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { P->ring = nullptr; rc = mgs_fail(ctx, MGS_ERR_ALLOC, "mgs_bicgstab_plan_create: mapped host ring"); }
    else {
      memset(P->ring, 0, hb);
      P->snap = reinterpret_cast<BcgState *>(P->ring + RING);
      if (hipHostGetDevicePointer((void **)&P->ring_dev, P->ring, 0) != hipSuccess) rc = mgs_fail(ctx, MGS_ERR_HIP, "mgs_bicgstab_plan_create: the host ring is not mappable into the device");
    }
  }
  if (rc != MGS_OK) { mgs_bicgstab_plan_destroy(P); return rc; }
  mgs_vec *vs[8] = {&P->p, &P->ph, &P->s, &P->sh, &P->t, &P->v, &P->r, &P->rt};
  for (int k = 0; k < 8; ++k) { vs[k]->ctx = ctx; vs[k]->n = P->n; vs[k]->d = P->block + (int64_t)k * P->stride; vs[k]->owns = false; }
  P->st = reinterpret_cast<BcgState *>(P->block + 8 * P->stride);
  P->bytes = (int64_t)(sizeof(double) * ndoubles);
  // the partial sums of every reduction a solve launches, and the hierarchy's operands and both captured cycles (p → p̂ and s → ŝ on ones): no later call allocates
  const int64_t nb = std::max<int64_t>(mgs_row_blocks(A), mgs_blas1_grid(ctx, ((int64_t)P->n + 1) / 2));
  rc = mgs_ensure_dot_part(ctx, 2 * std::max<int64_t>(nb, 1));
  if (rc == MGS_OK && h) rc = k_fill(ctx, P->p.d, P->n, 1.0);
  if (rc == MGS_OK && h) rc = k_fill(ctx, P->s.d, P->n, 1.0);
  if (rc == MGS_OK && h) rc = mgs_vcycle(h, &P->p, &P->ph, 1);
  if (rc == MGS_OK && h) rc = mgs_vcycle(h, &P->s, &P->sh, 1);
  if (rc != MGS_OK) { mgs_bicgstab_plan_destroy(P); return rc; }
  *out = P;
  return MGS_OK;
}

int mgs_bicgstab_plan_enqueue(mgs_bicgstab_plan *P, mgs_vec *x, const mgs_vec *b, int iters, double tol) {
  MGS_CHECK(P ? P->ctx : nullptr, P && x && b, MGS_ERR_INVALID, "mgs_bicgstab_plan_enqueue: NULL argument");
  mgs_ctx *ctx = P->ctx;
  MGS_CHECK(ctx, iters >= 0, MGS_ERR_INVALID, "mgs_bicgstab_plan_enqueue: iters = %d < 0", iters);
  MGS_TRY(check_call(P, x, b, "mgs_bicgstab_plan_enqueue"));
  mgs_vec xv, bv;
  xv.ctx = bv.ctx = ctx; xv.n = bv.n = P->n; xv.d = x->d; bv.d = b->d; xv.owns = bv.owns = false;
  P->calls++; P->enq_iters = 0; P->wasted = 0; P->waits = 0; P->unread = true;
  MGS_TRY(enqueue_init(P, &xv, &bv, tol, false));
  for (int i = 1; i <= iters; ++i) MGS_TRY(enqueue_iteration(P, &xv, i, tol, false));
  // FINAL: the projection of x, the true residual into t, the status
  if (P->ns) MGS_TRY(k_project_const(ctx, P->n, xv.d));
  MGS_TRY(mgs_residual(P->A, &xv, &bv, &P->t));
  if (P->ns) MGS_TRY(k_project_const_nrm2_fold(ctx, P->n, P->t.d)); else MGS_TRY(k_dot(ctx, P->n, P->t.d, P->t.d, nullptr));
  MGS_TRY(step(P, STEP_FINAL, iters, tol, false));
  MGS_HIP(ctx, hipMemcpyAsync(P->snap, P->st, sizeof(BcgState), hipMemcpyDeviceToHost, ctx->stream));
  return MGS_OK;
}

int mgs_bicgstab_plan_result(mgs_bicgstab_plan *P, int *iters_done, double *resid, double *recursive_resid, int *status) {
  MGS_CHECK(P ? P->ctx : nullptr, P, MGS_ERR_INVALID, "mgs_bicgstab_plan_result: NULL plan");
  mgs_ctx *ctx = P->ctx;
  MGS_CHECK(ctx, P->calls > 0, MGS_ERR_STATE, "mgs_bicgstab_plan_result: nothing has been solved or enqueued");
  if (P->unread) {
    MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    P->res_it = P->snap->it; P->res_status = P->snap->status; P->res_resid = P->snap->true_resid; P->res_rec = P->snap->resid; P->wasted = P->snap->wasted;
    P->unread = false;
  }
  if (iters_done) *iters_done = P->res_it;
  if (resid) *resid = P->res_resid;
  if (recursive_resid) *recursive_resid = P->res_rec;
  if (status) *status = P->res_status;
  return MGS_OK;
}

int mgs_bicgstab_plan_info(const mgs_bicgstab_plan *P, int64_t out[6]) {
  MGS_CHECK(P ? P->ctx : nullptr, P && out, MGS_ERR_INVALID, "mgs_bicgstab_plan_info: NULL argument");
  out[0] = P->bytes; out[1] = P->calls; out[2] = P->enq_iters; out[3] = P->wasted; out[4] = P->waits; out[5] = 0;      // no restart branch (bicg.cpp has none)
  return MGS_OK;
}

int mgs_bicgstab_plan_solve(mgs_bicgstab_plan *P, mgs_vec *x, const mgs_vec *b, int ahead, int *max_iter, double *tol, int *status) {
  MGS_CHECK(P ? P->ctx : nullptr, P && x && b && max_iter && tol && status, MGS_ERR_INVALID, "mgs_bicgstab_plan_solve: NULL argument");
  mgs_ctx *ctx = P->ctx;
  MGS_CHECK(ctx, ahead >= 0, MGS_ERR_INVALID, "mgs_bicgstab_plan_solve: ahead = %d < 0", ahead);
  MGS_TRY(check_call(P, x, b, "mgs_bicgstab_plan_solve"));
  const int n = P->n;
  mgs_vec xv, bv;
  xv.ctx = bv.ctx = ctx; xv.n = bv.n = n; xv.d = x->d; bv.d = b->d; xv.owns = bv.owns = false;
  P->calls++; P->enq_iters = 0; P->wasted = 0; P->waits = 0; P->unread = false;
  const int maxit = *max_iter;
  const double tl = *tol;
  const int win = std::min(ahead, RING - 2);          // at most win + 1 posts are outstanding
  struct Out { int it; unsigned long long seq; };
  std::deque<Out> outq;                               // enqueued, outcome not seen yet
  MGS_TRY(enqueue_init(P, &xv, &bv, tl, true));
  outq.push_back({0, P->seq});
  int next = 1, seen = -1;                            // next iteration to enqueue; outcomes are known through iteration `seen` (0: INIT)
  Look L = {0, -1, 0, 0, 0.0, 1.0};
  while (!L.frozen) {
    while (next <= maxit && next - 1 - win <= seen) {
      MGS_TRY(enqueue_iteration(P, &xv, next, tl, true));
      outq.push_back({next, P->seq});
      ++next;
    }
    if (outq.empty()) break;                          // every iteration up to maxit has been seen and none froze
    // the outcome the next enqueue waits for; with nothing left to enqueue, the last one
    const int need = next <= maxit ? std::max(next - 1 - win, outq.front().it) : outq.back().it;
    while (outq.front().it < need) outq.pop_front();
    MGS_TRY(wait_post(P, outq.front().seq, &L));
    outq.pop_front();
    seen = need;
  }
  // fin(): x ← Πx after its last update (a frozen iteration past the freeze touches no x), then the call waits for the stream as mgs_bicgstab does
  if (P->ns) MGS_TRY(k_project_const(ctx, n, xv.d));
  MGS_HIP(ctx, hipMemcpyAsync(P->snap, P->st, sizeof(BcgState), hipMemcpyDeviceToHost, ctx->stream));
  MGS_TRY(mgs_sync(ctx));
  P->wasted = P->snap->wasted;
  const int st = L.frozen ? L.status : 1;             // :134-135: the iterations are used up
  if (st == 0) *max_iter = L.it;                      // :90, :113, :125; statuses 2 and 3 leave *max_iter as it is (:96-99, :128-131)
  *tol = L.resid; *status = st;
  P->res_it = L.frozen ? L.it : std::max(maxit, 0); P->res_status = st; P->res_resid = L.resid; P->res_rec = L.resid;
  return MGS_OK;
}
