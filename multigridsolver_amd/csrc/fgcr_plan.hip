// fgcr_plan.hip — flexible GCR(m) whose coefficients never leave the device (mgs_fgcr_plan, include/mgs.h).
// Reference: the Krylov driver of src/CPU_Matlab/solve.m:28-33 is the nearest line; the reference has no flexible method and no asynchronous form.
//
// mgs_fgcr (mgs_api.hip) fetches the h_j of the multi-dot, (ρ_k, t) of the orthogonalisation pass and ‖r‖² of the residual pass — three host looks
// per iteration —, hands the coefficients U_jk = h_j/ρ_j to the orthogonalisation kernel by value and solves (I + U)·y = α on the host when a
// window closes.  Here ρ, α, U, y live in one state block in device memory, as bicgstab_plan.hip keeps mgs_bicgstab's scalars.  One-wave "scalar
// step" kernels form every scalar with the operation, and in the order, the host code of mgs_fgcr uses (no fast-math, no contraction; FP64
// division and sqrt are correctly rounded), and three new vector passes evaluate the expressions of maxpy_dot2_kernel and of
// update_dot2_partial(_vec)_kernel with their coefficients read from the state block.  Everything else is the launches mgs_fgcr makes, called
// with a NULL host pointer: the cycle, the projection, the SpMV, k_dot2, k_mdot, mgs_residual and the folds.  So every bit agrees with mgs_fgcr's.
//
// One iteration at window slot k (the host always knows k) is the fixed launch sequence
//   cycle r → C[k] (projected) · SpMV V[k] = A·C[k] · k = 0: k_dot2 (V0·V0, V0·r); k > 0: k_mdot → h_j · COEF · orthogonalisation pass + fold
//   · RHOK · residual pass + fold · RES
// and a window close is YSOLVE · x-pass · (projection of x) · mgs_residual and its norm · WIN.
// A solve that converges by the recursion, converges by a true residual, or breaks down sets `frozen`; from then on COEF, RHOK and RES are no-ops
// (RHOK counts into `wasted`) and the orthogonalisation and residual passes return before they touch a vector.  Cycles, SpMVs and reductions of a
// frozen iteration still run; they write C[k], V[k] of slots behind the open ones (k ≥ m_open) and scratch only.  The x-pass of a close is guarded
// by `m_open`, not by `frozen`: the first close after a freeze applies the open window once, WIN sets m_open = 0, every later close is a no-op.
//
// RES and WIN (and INIT) post (iteration, status, why, frozen, wasted, resid) and a ticket into a ring of slots in mapped, coherent host memory.
// mgs_fgcr_plan_solve looks at one slot per iteration, `ahead` iterations behind the queue, and orchestrates every restart from the true residual
// itself (mgs_fgcr's restart_now); mgs_fgcr_plan_enqueue never looks and its windows are fixed.
#include <algorithm>

#include "krylov_plan.hpp"

namespace {
using namespace krylov;
constexpr int FW = 16;                   // the widest window: one multi-vector pass holds 16 vectors (blas1.hip: MDOT_MAX), a hierarchy caches 16 graphs

// why a solve froze
enum { WHY_NONE = 0, WHY_RECURSION = 1, WHY_BREAKDOWN = 2, WHY_INIT = 3, WHY_TRUE = 4 };
// status: −1 running, 0 converged on a true residual, 2 breakdown, 4 the recursion says converged (no true residual yet), 5 drifted (the recursion
// said converged, the true residual does not); after FINAL: 0, 1 or 2 as mgs_fgcr reports them
enum { ST_RUNNING = -1, ST_OK = 0, ST_BREAKDOWN = 2, ST_RECURSION = 4, ST_DRIFTED = 5 };

struct FgState {
  double normb, resid, true_resid, rr;
  double rho[FW], alpha[FW], hj[FW], y[FW], cf[FW];   // cf_j = −y_j: the coefficients of the x-pass
  double U[FW * FW];                                    // U[j·FW + k] = h_j/ρ_j of iteration k, j < k
  int it;        // the last iteration that ran unfrozen (the one that froze, once frozen)
  int status;
  int frozen;
  int why;
  int m_open;    // directions of the open window that x has not received yet
  int wasted;    // iterations that ran frozen
};
enum { STEP_NORMB = 0, STEP_INIT, STEP_COEF, STEP_RHOK, STEP_RES, STEP_YSOLVE, STEP_WIN, STEP_RESUME, STEP_FINAL };

// The scalar steps: one wave, lane 0 works.  red = ctx->red_dev + RED.  k: the window slot (COEF, RHOK); `it`: the iteration the step belongs to
// (FINAL: the iterations enqueued); `tol`: the tolerance (INIT, RES, WIN, FINAL); slot = NULL: nothing is posted.  Line numbers: mgs_api.hip, mgs_fgcr.
__global__ void fgp_step_kernel(int step, FgState *__restrict__ st, const double *__restrict__ red, int k, int it, double tol, Slot *slot, unsigned long long ticket) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  switch (step) {
    case STEP_NORMB: {                      // ‖b‖ (‖Πb‖), 0 replaced by 1; a fresh state
      double nb = sqrt(red[0]);
      if (nb == 0.0) nb = 1.0;
      st->normb = nb;
      st->resid = st->true_resid = st->rr = 0.0;
      st->it = 0; st->status = ST_RUNNING; st->frozen = 0; st->why = WHY_NONE; st->m_open = 0; st->wasted = 0;
      break;
    }
    case STEP_INIT: {                       // red[0] = ‖b − A·x‖²: the `<=` of iteration 0
      st->rr = red[0];
      const double nr = sqrt(red[0]);
      st->resid = nr / st->normb;
      if (st->resid <= tol) { st->frozen = 1; st->status = ST_OK; st->why = WHY_INIT; }
      if (slot) post_slot(slot, st, ticket, &st->why, &st->m_open);
      break;
    }
    case STEP_COEF: {                       // U_jk = ρ_j != 0 ? h_j/ρ_j : 0
      if (st->frozen) break;
      for (int j = 0; j < k; ++j) st->U[j * FW + k] = st->rho[j] != 0.0 ? st->hj[j] / st->rho[j] : 0.0;
      break;
    }
    case STEP_RHOK: {                       // red = (ρ_k, t)
      if (st->frozen) { st->wasted += 1; break; }
      st->it = it;
      st->rho[k] = red[0];
      st->m_open = k + 1;
      if (st->rho[k] == 0.0) { st->alpha[k] = 0.0; st->frozen = 1; st->status = ST_BREAKDOWN; st->why = WHY_BREAKDOWN; break; }
      st->alpha[k] = red[1] / st->rho[k];
      break;
    }
    case STEP_RES: {                        // red[0] = ‖r‖² of the recursion
      if (!st->frozen) {
        st->rr = red[0];
        st->resid = sqrt(red[0]) / st->normb;
        if (st->resid < tol) { st->frozen = 1; st->status = ST_RECURSION; st->why = WHY_RECURSION; }
      }
      if (slot) post_slot(slot, st, ticket, &st->why, &st->m_open);
      break;
    }
    case STEP_YSOLVE: {                     // close_window: (I + U)·y = α over the m_open directions, cf_j = −y_j
      const int m = st->m_open;
      for (int q = m - 1; q >= 0; --q) {
        double s = st->alpha[q];
        for (int p = q + 1; p < m; ++p) s -= st->U[q * FW + p] * st->y[p];
        st->y[q] = s;
      }
      for (int q = 0; q < m; ++q) st->cf[q] = -st->y[q];
      break;
    }
    case STEP_WIN: {                        // red[0] = ‖b − A·x‖² behind a close
      const double t = sqrt(red[0]) / st->normb;
      st->true_resid = t;
      if (!st->frozen) {
        st->resid = t;
        if (t < tol) { st->frozen = 1; st->status = ST_OK; st->why = WHY_TRUE; }
      } else if (st->why == WHY_RECURSION) { st->resid = t; st->status = t < tol ? ST_OK : ST_DRIFTED; }
      else if (st->why == WHY_BREAKDOWN) { st->resid = t; st->status = t < tol ? ST_OK : ST_BREAKDOWN; }
      st->m_open = 0;
      if (slot) post_slot(slot, st, ticket, &st->why, &st->m_open);
      break;
    }
    case STEP_RESUME: {                     // the host has seen "drifted": go on from the true residual with an empty window
      st->frozen = 0; st->status = ST_RUNNING; st->why = WHY_NONE; st->m_open = 0;
      break;
    }
    case STEP_FINAL: {                      // behind the last close, the projection of x and r = b − A·x: red[0] = ‖r‖²
      const double t = sqrt(red[0]) / st->normb;
      st->true_resid = t;
      if (!st->frozen) { st->it = it; st->status = t < tol ? 0 : 1; }
      else if (st->why == WHY_INIT) st->status = t <= tol ? 0 : 1;
      else if (st->why == WHY_BREAKDOWN) st->status = t < tol ? 0 : 2;
      else st->status = t < tol ? 0 : 1;
      st->frozen = 1; st->m_open = 0;
      break;
    }
  }
}

struct FgVecs { const double *w[FW]; };

// Orthogonalisation pass: v ← v − Σ_{j<K} U_jK·w_j with the partial pairs (v·v, v·u), maxpy_dot2_kernel's expression (its z = x = v, u2 = NULL),
// arms, partial layout [2][gridDim.x] and in-workgroup fold; the coefficients come from the state block.  Frozen: v and the partials stay.
template <bool VEC>
__global__ __launch_bounds__(PTB) void fgp_orth_kernel(int64_t n, int K, const FgState *__restrict__ st, double *v, const FgVecs W, const double *__restrict__ u,
                                                       double *__restrict__ part) {
  if (st->frozen) return;
  __shared__ double sh[2][PTB / 64];
  double cf[FW];
#pragma unroll
  for (int k = 0; k < FW; ++k) cf[k] = k < K ? st->U[k * FW + K] : 0.0;
  double s0 = 0.0, s1 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * PTB;
  if (VEC) {
    const int64_t n2 = n >> 1;
    vd2 *vv = reinterpret_cast<vd2 *>(v);
    const vd2 *__restrict__ uv = reinterpret_cast<const vd2 *>(u);
    for (int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x; i < n2; i += stride) {
      vd2 zi = vv[i];
#pragma unroll
      for (int k = 0; k < FW; ++k)
        if (k < K) { const vd2 wi = reinterpret_cast<const vd2 *>(W.w[k])[i]; zi.x -= cf[k] * wi.x; zi.y -= cf[k] * wi.y; }
      vv[i] = zi;
      s0 += zi.x * zi.x; s0 += zi.y * zi.y;
      const vd2 q = uv[i]; s1 += zi.x * q.x; s1 += zi.y * q.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
      double zi = v[n - 1];
#pragma unroll
      for (int k = 0; k < FW; ++k) if (k < K) zi -= cf[k] * W.w[k][n - 1];
      v[n - 1] = zi;
      s0 += zi * zi;
      s1 += zi * u[n - 1];
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x; i < n; i += stride) {
      double zi = v[i];
#pragma unroll
      for (int k = 0; k < FW; ++k) if (k < K) zi -= cf[k] * W.w[k][i];
      v[i] = zi;
      s0 += zi * zi;
      s1 += zi * u[i];
    }
  }
  BLAS1_FOLD2(s0, s1, sh, part);
}

// x-pass of a window close: x ← x − Σ_{j<m_open} cf_j·c_j, maxpy_dot2_kernel's expression without sums; m_open and cf from the state block.
// Guarded by m_open alone: the close behind a freeze still owes x its window, a close with nothing open touches nothing.
template <bool VEC>
__global__ __launch_bounds__(PTB) void fgp_x_kernel(int64_t n, const FgState *__restrict__ st, double *x, const FgVecs W) {
  const int K = st->m_open;
  if (K <= 0) return;
  double cf[FW];
#pragma unroll
  for (int k = 0; k < FW; ++k) cf[k] = k < K ? st->cf[k] : 0.0;
  const int64_t stride = (int64_t)gridDim.x * PTB;
  if (VEC) {
    const int64_t n2 = n >> 1;
    vd2 *xv = reinterpret_cast<vd2 *>(x);
    for (int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x; i < n2; i += stride) {
      vd2 zi = xv[i];
#pragma unroll
      for (int k = 0; k < FW; ++k)
        if (k < K) { const vd2 wi = reinterpret_cast<const vd2 *>(W.w[k])[i]; zi.x -= cf[k] * wi.x; zi.y -= cf[k] * wi.y; }
      xv[i] = zi;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
      double zi = x[n - 1];
#pragma unroll
      for (int k = 0; k < FW; ++k) if (k < K) zi -= cf[k] * W.w[k][n - 1];
      x[n - 1] = zi;
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x; i < n; i += stride) {
      double zi = x[i];
#pragma unroll
      for (int k = 0; k < FW; ++k) if (k < K) zi -= cf[k] * W.w[k][i];
      x[i] = zi;
    }
  }
}

// Residual pass in place: r ← 1.0·r + (−α_k)·v with the partial pairs (r·r, 0) of update_dot2_partial_vec_kernel<false> / update_dot2_partial_kernel —
// the same per-element expression, the same order of additions per lane, the same layout [2][gridDim.x].  Frozen: r and the partials stay.
__global__ __launch_bounds__(PTB) void fgp_resid_vec_kernel(int64_t n, int k, const FgState *__restrict__ st, double *r, const double *__restrict__ v,
                                                            double *__restrict__ part, int nts) {
  if (st->frozen) return;
  const double a = 1.0, b = -st->alpha[k];
  __shared__ double sh[2][PTB / 64];
  const int64_t n2 = n >> 1;
  vd2 *rv = reinterpret_cast<vd2 *>(r);
  const vd2 *__restrict__ yv = reinterpret_cast<const vd2 *>(v);
  double s0 = 0.0, s1 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x; i < n2; i += stride) {
    const vd2 p = rv[i], o = yv[i]; vd2 q;
    q.x = a * p.x + b * o.x; q.y = a * p.y + b * o.y;
    st2(rv + i, q, nts != 0);
    s0 += q.x * q.x; s0 += q.y * q.y;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double zi = a * r[n - 1] + b * v[n - 1];
    r[n - 1] = zi; s0 += zi * zi;
  }
  BLAS1_FOLD2(s0, s1, sh, part);
}
__global__ __launch_bounds__(PTB) void fgp_resid_kernel(int64_t n, int k, const FgState *__restrict__ st, double *r, const double *__restrict__ v, double *__restrict__ part) {
  if (st->frozen) return;
  const double a = 1.0, b = -st->alpha[k];
  __shared__ double sh[2][PTB / 64];
  double s0 = 0.0, s1 = 0.0;
  int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (; i < n; i += stride) {
    const double zi = a * r[i] + b * v[i];
    r[i] = zi;
    s0 += zi * zi;
  }
  BLAS1_FOLD2(s0, s1, sh, part);
}

// workgroups of maxpy_dot2_kernel (k_maxpy_dot2) and of mdot_partial_kernel (k_mdot)
inline int maxpy_grid(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>((n + (int64_t)PTB * 4 - 1) / ((int64_t)PTB * 4), 1), 1 << 20); }
inline int mdot_grid(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>((n / 2 + (int64_t)PTB * 4 - 1) / ((int64_t)PTB * 4), 1), 2048); }
}   // namespace

struct mgs_fgcr_plan : krylov::Plan<FgState> {
  mgs_fgcr_plan() { name = "mgs_fgcr_plan"; }
  int restart = 0;
  mgs_vec r, C[FW], V[FW];            // r, C[0..restart), V[0..restart): views into block, in this order
};

namespace {
int step(mgs_fgcr_plan *P, int which, int k, int it, double tol, bool post) {
  mgs_ctx *ctx = P->ctx;
  Slot *slot = P->next_slot(post);
  hipLaunchKernelGGL(fgp_step_kernel, dim3(1), dim3(64), 0, ctx->stream, which, P->st, ctx->red_dev + RED, k, it, tol, slot, P->seq);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

// the grid, the arms, the partial buffer and the fold of k_maxpy_dot2 with sums (the plan's vectors are 256-byte aligned: the 16-byte arm whenever n >= 2)
int launch_orth(mgs_fgcr_plan *P, int k) {
  mgs_ctx *ctx = P->ctx; const int64_t n = P->n;
  FgVecs W;
  for (int j = 0; j < FW; ++j) W.w[j] = j < k ? P->V[j].d : P->V[k].d;
  const int nb = maxpy_grid(n);
  double *part = ctx->red_dev;
  if (nb > MGS_DOT_BLOCKS / 2) { MGS_TRY(mgs_ensure_dot_part(ctx, 2 * (int64_t)nb)); part = ctx->dot_part; }
  if (n >= 2) hipLaunchKernelGGL(fgp_orth_kernel<true>, dim3(nb), dim3(PTB), 0, ctx->stream, n, k, P->st, P->V[k].d, W, P->r.d, part);
  else hipLaunchKernelGGL(fgp_orth_kernel<false>, dim3(nb), dim3(PTB), 0, ctx->stream, n, k, P->st, P->V[k].d, W, P->r.d, part);
  MGS_HIP(ctx, hipGetLastError());
  return k_dot2_finish(ctx, nb, part, nullptr);
}
int launch_x(mgs_fgcr_plan *P, double *x) {
  mgs_ctx *ctx = P->ctx; const int64_t n = P->n;
  FgVecs W;
  for (int j = 0; j < FW; ++j) W.w[j] = j < P->restart ? P->C[j].d : x;      // slots at and behind m_open are never read
  const int nb = maxpy_grid(n);
  if (n >= 2 && al16(x)) hipLaunchKernelGGL(fgp_x_kernel<true>, dim3(nb), dim3(PTB), 0, ctx->stream, n, P->st, x, W);
  else hipLaunchKernelGGL(fgp_x_kernel<false>, dim3(nb), dim3(PTB), 0, ctx->stream, n, P->st, x, W);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
// the grids, the partial buffer, the store rule and the fold of k_update_dot2
int launch_resid(mgs_fgcr_plan *P, int k) {
  mgs_ctx *ctx = P->ctx; const int64_t n = P->n;
  int nb = (int)((n + PTB - 1) / PTB);
  if (nb > MGS_DOT_BLOCKS / 2) nb = MGS_DOT_BLOCKS / 2;
  if (nb < 1) nb = 1;
  if (ctx->opt_blas1_vec) {
    nb = mgs_blas1_grid(ctx, (n + 1) / 2);
    double *part = ctx->red_dev;
    if (nb > MGS_DOT_BLOCKS / 2) { MGS_TRY(mgs_ensure_dot_part(ctx, 2 * (int64_t)nb)); part = ctx->dot_part; }
    hipLaunchKernelGGL(fgp_resid_vec_kernel, dim3(nb), dim3(PTB), 0, ctx->stream, n, k, P->st, P->r.d, P->V[k].d, part, nts_of(ctx, n));
    MGS_HIP(ctx, hipGetLastError());
    return k_dot2_finish(ctx, nb, part, nullptr);
  }
  hipLaunchKernelGGL(fgp_resid_kernel, dim3(nb), dim3(PTB), 0, ctx->stream, n, k, P->st, P->r.d, P->V[k].d, ctx->red_dev);
  MGS_HIP(ctx, hipGetLastError());
  return k_dot2_finish(ctx, nb, ctx->red_dev, nullptr);
}
// r = b − A·x (r = Π(b − A·x)) with ‖r‖² left in red: mgs_fgcr's true_residual without its look
int true_residual(mgs_fgcr_plan *P, const mgs_vec *xv, const mgs_vec *bv) {
  MGS_TRY(mgs_residual(P->A, xv, bv, &P->r));
  return P->ns ? k_project_const_nrm2_fold(P->ctx, P->n, P->r.d) : k_dot(P->ctx, P->n, P->r.d, P->r.d, nullptr);
}
// INIT: ‖b‖ (‖Πb‖), x ← Πx, the true residual, the freeze with (status 0, it 0) when it is within tol already
int enqueue_init(mgs_fgcr_plan *P, mgs_vec *xv, const mgs_vec *bv, double tol, bool post) {
  mgs_ctx *ctx = P->ctx; const int64_t n = P->n;
  if (P->ns) MGS_TRY(k_const_dev_nrm2_fold(ctx, n, bv->d)); else MGS_TRY(k_dot(ctx, n, bv->d, bv->d, nullptr));
  MGS_TRY(step(P, STEP_NORMB, 0, 0, 0.0, false));
  if (P->ns) MGS_TRY(k_project_const(ctx, n, xv->d));
  MGS_TRY(true_residual(P, xv, bv));
  return step(P, STEP_INIT, 0, 0, tol, post);
}
int enqueue_iteration(mgs_fgcr_plan *P, int k, int it, double tol, bool post) {
  mgs_ctx *ctx = P->ctx; const int64_t n = P->n;
  if (P->h) MGS_TRY(mgs_vcycle(P->h, &P->r, &P->C[k], 1)); else MGS_TRY(mgs_vec_copy(&P->r, &P->C[k]));
  if (P->ns) MGS_TRY(k_project_const(ctx, n, P->C[k].d));
  MGS_TRY(mgs_spmv(P->A, &P->C[k], &P->V[k]));
  if (k == 0) MGS_TRY(k_dot2(ctx, n, P->V[0].d, P->V[0].d, P->V[0].d, P->r.d, nullptr));
  else {
    const double *w[FW];
    for (int q = 0; q < k; ++q) w[q] = P->V[q].d;
    MGS_TRY(k_mdot(ctx, n, k, P->V[k].d, w, P->st->hj, nullptr));
    MGS_TRY(step(P, STEP_COEF, k, it, 0.0, false));
    MGS_TRY(launch_orth(P, k));
  }
  MGS_TRY(step(P, STEP_RHOK, k, it, 0.0, false));
  MGS_TRY(launch_resid(P, k));
  P->enq_iters++;
  return step(P, STEP_RES, k, it, tol, post);
}
// a window close; `last`: the step behind it is FINAL (enqueue) instead of WIN
int enqueue_close(mgs_fgcr_plan *P, mgs_vec *xv, const mgs_vec *bv, bool project, int it, double tol, bool post, bool last) {
  MGS_TRY(step(P, STEP_YSOLVE, 0, it, 0.0, false));
  MGS_TRY(launch_x(P, xv->d));
  if (project && P->ns) MGS_TRY(k_project_const(P->ctx, P->n, xv->d));
  MGS_TRY(true_residual(P, xv, bv));
  return step(P, last ? STEP_FINAL : STEP_WIN, 0, it, tol, post);
}
}   // namespace

int mgs_fgcr_plan_destroy(mgs_fgcr_plan *P) {
  if (!P) return MGS_OK;
  P->release();
  delete P;
  return MGS_OK;
}

int mgs_fgcr_plan_create(const mgs_csr *A, mgs_hier *h, int restart, mgs_fgcr_plan **out) {
  mgs_ctx *ctx = A ? A->ctx : (h ? h->ctx : nullptr);
  MGS_CHECK(ctx, A && out, MGS_ERR_INVALID, "mgs_fgcr_plan_create: NULL argument");
  MGS_CHECK(ctx, restart >= 1 && restart <= FW, MGS_ERR_INVALID, "mgs_fgcr_plan_create: restart = %d outside 1..%d (wider windows are served by mgs_fgcr)", restart, FW);
  mgs_fgcr_plan *P = new mgs_fgcr_plan();
  int rc = P->validate(A, h, "mgs_fgcr_plan_create", "a square unsharded operator is required");
  if (rc == MGS_OK) rc = P->allocate("mgs_fgcr_plan_create", 1 + 2 * restart);
  if (rc != MGS_OK) { mgs_fgcr_plan_destroy(P); return rc; }
  P->restart = restart;
  P->r = P->view(0);
  for (int k = 0; k < restart; ++k) { P->C[k] = P->view(1 + k); P->V[k] = P->view(1 + restart + k); }
  // the partial sums of every reduction a solve launches, and the hierarchy's operands and one captured cycle r → C[k] per slot: no later call allocates
  int64_t np = 2 * std::max<int64_t>(std::max<int64_t>(mgs_row_blocks(A), mgs_blas1_grid(ctx, ((int64_t)P->n + 1) / 2)), maxpy_grid(P->n));
  np = std::max<int64_t>(np, (int64_t)restart * mdot_grid(P->n));
  rc = mgs_ensure_dot_part(ctx, std::max<int64_t>(np, 2));
  if (rc == MGS_OK && h) rc = k_fill(ctx, P->r.d, P->n, 1.0);
  for (int k = 0; k < restart && rc == MGS_OK && h; ++k) rc = mgs_vcycle(h, &P->r, &P->C[k], 1);
  if (rc != MGS_OK) { mgs_fgcr_plan_destroy(P); return rc; }
  *out = P;
  return MGS_OK;
}

int mgs_fgcr_plan_enqueue(mgs_fgcr_plan *P, mgs_vec *x, const mgs_vec *b, int iters, double tol) {
  MGS_CHECK(P ? P->ctx : nullptr, P && x && b, MGS_ERR_INVALID, "mgs_fgcr_plan_enqueue: NULL argument");
  mgs_ctx *ctx = P->ctx;
  MGS_CHECK(ctx, iters >= 0, MGS_ERR_INVALID, "mgs_fgcr_plan_enqueue: iters = %d < 0", iters);
  MGS_TRY(P->check_call(x, b, "mgs_fgcr_plan_enqueue"));
  mgs_vec xv, bv;
  P->begin_call(x, b, &xv, &bv, true);
  MGS_TRY(enqueue_init(P, &xv, &bv, tol, false));
  int k = 0;
  for (int i = 1; i <= iters; ++i) {
    MGS_TRY(enqueue_iteration(P, k, i, tol, false));
    if (++k == P->restart && i < iters) { MGS_TRY(enqueue_close(P, &xv, &bv, false, i, tol, false, false)); k = 0; }   // a scheduled close: x catches up, r ← b − A·x
  }
  // FINAL: the open window, the projection of x (an x that no iteration followed was projected by INIT), the true residual, the status
  MGS_TRY(enqueue_close(P, &xv, &bv, iters > 0, iters, tol, false, true));
  return P->snapshot();
}

int mgs_fgcr_plan_result(mgs_fgcr_plan *P, int *iters_done, double *resid, double *recursive_resid, int *status) {
  MGS_CHECK(P ? P->ctx : nullptr, P, MGS_ERR_INVALID, "mgs_fgcr_plan_result: NULL plan");
  return P->result("mgs_fgcr_plan_result", iters_done, resid, recursive_resid, status);
}

int mgs_fgcr_plan_info(const mgs_fgcr_plan *P, int64_t out[6]) {
  MGS_CHECK(P ? P->ctx : nullptr, P && out, MGS_ERR_INVALID, "mgs_fgcr_plan_info: NULL argument");
  P->info(out);
  return MGS_OK;
}

int mgs_fgcr_plan_solve(mgs_fgcr_plan *P, mgs_vec *x, const mgs_vec *b, int ahead, int *max_iter, double *tol, int *status) {
  MGS_CHECK(P ? P->ctx : nullptr, P && x && b && max_iter && tol && status, MGS_ERR_INVALID, "mgs_fgcr_plan_solve: NULL argument");
  mgs_ctx *ctx = P->ctx;
  MGS_CHECK(ctx, ahead >= 0, MGS_ERR_INVALID, "mgs_fgcr_plan_solve: ahead = %d < 0", ahead);
  MGS_TRY(P->check_call(x, b, "mgs_fgcr_plan_solve"));
  const int n = P->n, R = P->restart;
  mgs_vec xv, bv;
  P->begin_call(x, b, &xv, &bv, false);
  const int maxit = *max_iter;
  const double tl = *tol;
  Lookahead la(maxit, ahead);
  Look L = {0, ST_RUNNING, 0, 0, WHY_NONE, 0, 0.0, 0.0};      // aux0: why the solve froze
  int r_it = 0, r_status = 1; double r_resid = 0.0;   // what the call returns
  MGS_TRY(enqueue_init(P, &xv, &bv, tl, true));
  la.enqueued(P->seq);
  for (int k = 0;;) {                                 // k: the window slot of the next iteration to enqueue
    while (la.may_enqueue()) {
      // the iteration that fills its window closes it and posts from WIN; the last iteration of all posts from RES and the host closes behind
      // its look: that close projects x, which no iteration run on speculation may do twice
      const bool closing = k == R - 1 && la.next < maxit;
      MGS_TRY(enqueue_iteration(P, k, la.next, tl, !closing));
      if (closing) MGS_TRY(enqueue_close(P, &xv, &bv, false, la.next, tl, true, false));
      la.enqueued(P->seq);
      k = closing ? 0 : k + 1;
    }
    MGS_TRY(P->wait_post(la.take(), &L));
    if (!L.frozen) {
      if (la.seen < maxit) continue;
      if (la.seen == 0) { r_it = 0; r_resid = L.resid; r_status = 1; break; }      // *max_iter <= 0: nothing has touched x since INIT projected it
      // the iterations are used up: x catches up (projected), the true residual decides between 0 and 1
      MGS_TRY(enqueue_close(P, &xv, &bv, true, maxit, tl, true, false));
      MGS_TRY(P->wait_post(P->seq, &L));
      r_it = maxit; r_resid = L.resid; r_status = (L.frozen && L.status == ST_OK) ? 0 : 1;
      break;
    }
    // frozen at iteration L.it: nothing enqueued behind it has changed x, r or the open window
    r_it = L.it;
    if (L.aux0 == WHY_INIT) { r_resid = L.resid; r_status = 0; break; }      // `<=` at iteration 0: x (projected by INIT) stays as it is
    if (L.aux0 == WHY_TRUE) {                        // a full window's true residual is below tol: x ← Πx behind it, as fin() does
      if (P->ns) MGS_TRY(k_project_const(ctx, n, xv.d));
      r_resid = L.resid; r_status = 0;
      break;
    }
    // the recursion says converged, or a breakdown: close (a no-op if a scheduled close has run already), x ← Πx, the true residual decides
    const int why = L.aux0;
    MGS_TRY(enqueue_close(P, &xv, &bv, true, L.it, tl, true, false));
    MGS_TRY(P->wait_post(P->seq, &L));
    r_resid = L.resid;
    if (why == WHY_BREAKDOWN) { r_status = L.status == ST_OK ? 0 : 2; break; }
    if (L.status == ST_OK) { r_status = 0; break; }
    // the recursion had drifted: r holds the true residual, go on from it with an empty window (mgs_fgcr's restart_now)
    P->restarts++;
    r_status = 1;
    if (r_it >= maxit) break;
    MGS_TRY(step(P, STEP_RESUME, 0, r_it, 0.0, false));
    la.restart(r_it); k = 0;
    L.frozen = 0;
  }
  MGS_TRY(P->snapshot());
  MGS_TRY(mgs_sync(ctx));
  P->wasted = P->snap->wasted;
  *max_iter = r_it; *tol = r_resid; *status = r_status;
  P->res_it = r_it; P->res_status = r_status; P->res_resid = r_resid; P->res_rec = P->snap->resid;
  return MGS_OK;
}
