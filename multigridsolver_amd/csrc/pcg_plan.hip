// pcg_plan.hip — preconditioned CG whose scalars never leave the device (mgs_pcg_plan, include/mgs.h).
// Nearest reference line: src/CPU_Matlab/solve.m:28-31 (pcg); the reference has no asynchronous form.
//
// mgs_pcg (mgs_api.hip) computes ρ, α, β and the stopping test on the host: three host looks per iteration, each one draining the queue behind
// it.  Here the same scalars live in one state block in device memory.  One-wave "scalar step" kernels turn the folded inner products the
// reductions leave in red_dev[MGS_DOT_BLOCKS ..] into the next scalars with the very operations the host uses (α = ρ/(p·q), β = ρ/ρ_prev or
// −α·(z·q)/ρ_prev, resid = √(r·r)/‖b‖ — no fast-math in this build, FP64 division and sqrt are correctly rounded), and the vector passes
// take α and β from the state block instead of from kernel arguments.  Everything else is the launches mgs_pcg makes: the cycle, the
// projection, the partial reductions and their folds, the SpMV with its dot epilogue — called with a NULL host pointer, which enqueues and
// folds without fetching (blas1.hip: fetch_or_leave).  So the bits of every vector agree with mgs_pcg's.
//
// One iteration is a fixed launch sequence: cycle (or copy) · projection (declared null space) · dots and fold · RHO · direction ·
// SpMV with p·q and fold · PQ · residual and fold · RES.  A solve that converges or breaks down sets `frozen`; from then on every scalar
// step is a no-op that counts into `wasted` and every workgroup of the three vector passes returns before it touches a vector.  Cycle, SpMV
// and the reductions of a frozen iteration still run (they cannot be predicated without touching the cycle); they write z, q and scratch only,
// which are recomputed after any restart.
//
// RES (and INIT) also post (iteration, status, frozen, resid, ‖b‖) and a ticket into a ring of slots in mapped, coherent host memory —
// the mechanism of begin_post / fetch_results with the plan's own sequence number as the ticket.  mgs_pcg_plan_solve looks at one slot per
// iteration, `ahead` iterations behind the queue; mgs_pcg_plan_enqueue never looks.
#include <algorithm>
#include <cmath>

#include "krylov_plan.hpp"

namespace {
using namespace krylov;

// the state block.  status: −1 running, 0 the recursion says converged (the true residual still decides), 2 r·z not positive, 3 p·q not
// positive; after FINAL: mgs_pcg's status
struct PcgState {
  double normb, rho, rho_prev, alpha, beta, pq, zq, rr, resid, true_resid;
  int it;        // the last iteration that ran unfrozen (the one that froze, once frozen)
  int status;
  int frozen;
  int first;     // the next direction is p = z
  int pending;   // x lags by alpha·p
  int wasted;    // iterations that ran frozen
};
enum { STEP_NORMB = 0, STEP_INIT, STEP_RHO, STEP_PQ, STEP_RES, STEP_FLUSHED, STEP_RESTART, STEP_FINAL };

// The scalar steps: one wave, lane 0 works.  red = ctx->red_dev + RED.  `it`: the iteration the step belongs to (FINAL: the iterations
// enqueued); `val`: the tolerance (INIT, RES, FINAL) or the true residual the host found (RESTART); slot = NULL: nothing is posted.
__global__ void pcgp_step_kernel(int step, PcgState *__restrict__ st, const double *__restrict__ red, int it, double val, int flexible, Slot *slot,
                                 unsigned long long ticket) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  switch (step) {
    case STEP_NORMB: {                      // ‖b‖ (‖Πb‖), 0 replaced by 1; a fresh state
      double nb = sqrt(red[0]);
      if (nb == 0.0) nb = 1.0;
      st->normb = nb;
      st->rho = st->rho_prev = st->alpha = st->beta = st->pq = st->zq = st->rr = st->resid = st->true_resid = 0.0;
      st->it = 0; st->status = -1; st->frozen = 0; st->first = 1; st->pending = 0; st->wasted = 0;
      break;
    }
    case STEP_INIT: {                       // the initial (true) residual
      st->rr = red[0];
      st->resid = sqrt(red[0]) / st->normb;
      if (st->resid <= val) { st->frozen = 1; st->status = 0; }
      if (slot) post_slot(slot, st, ticket);
      break;
    }
    case STEP_RHO: {
      if (st->frozen) { st->wasted += 1; break; }
      st->it = it;
      st->rho = red[0]; st->zq = red[1];
      if (!(st->rho > 0.0)) { st->frozen = 1; st->status = 2; break; }       // preconditioner not positive definite (or not a number)
      if (!st->first) st->beta = flexible ? -st->alpha * st->zq / st->rho_prev : st->rho / st->rho_prev;
      break;
    }
    case STEP_PQ: {
      if (st->frozen) break;
      st->pq = red[0];
      st->first = 0; st->pending = 0;                                         // the direction pass has applied the lagged update
      if (!(st->pq > 0.0)) { st->frozen = 1; st->status = 3; break; }        // A not positive definite along p
      st->alpha = st->rho / st->pq; st->pending = 1;
      break;
    }
    case STEP_RES: {
      if (!st->frozen) {
        st->rr = red[0];
        st->resid = sqrt(red[0]) / st->normb; st->rho_prev = st->rho;
        if (st->resid < val) { st->frozen = 1; st->status = 0; }              // the recursion says converged
      }
      if (slot) post_slot(slot, st, ticket);
      break;
    }
    case STEP_FLUSHED: st->pending = 0; break;
    case STEP_RESTART:                      // the recursion had drifted: r holds the true residual, start over from it
      st->frozen = 0; st->status = -1; st->first = 1; st->pending = 0; st->resid = val;
      break;
    case STEP_FINAL: {                      // after flush, projection and r = b − A·x: red[0] = ‖r‖²
      st->true_resid = sqrt(red[0]) / st->normb;
      st->pending = 0;
      if (!st->frozen) { st->it = it; st->status = 1; }
      else if (st->status == 0) st->status = (st->it == 0 ? st->true_resid <= val : st->true_resid < val) ? 0 : 1;
      st->frozen = 1;
      break;
    }
  }
}

// Direction pass, pcg_dir_vec_kernel / pcg_dir_kernel with the scalars from the state block: first: p ← z (p not read, x not touched);
// else x ← x + a·p, p ← z + beta·p.  The state is read once per workgroup through uniform loads; a frozen workgroup returns at once.
__global__ __launch_bounds__(PTB) void pcgp_dir_vec_kernel(int64_t n, const PcgState *__restrict__ st, double *__restrict__ x, double *__restrict__ p,
                                                           const double *__restrict__ z, int nts) {
  if (st->frozen) return;
  const bool first = st->first != 0;
  const double a = st->alpha, beta = st->beta;
  const int64_t n2 = n >> 1;
  vd2 *__restrict__ xv = reinterpret_cast<vd2 *>(x);
  vd2 *__restrict__ pv = reinterpret_cast<vd2 *>(p);
  const vd2 *__restrict__ zv = reinterpret_cast<const vd2 *>(z);
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x; i < n2; i += stride) {
    const vd2 zi = zv[i];
    if (first) st2(pv + i, zi, nts != 0);
    else {
      const vd2 pi = pv[i], xi = xv[i]; vd2 xo, po;
      xo.x = xi.x + a * pi.x; xo.y = xi.y + a * pi.y;
      po.x = zi.x + beta * pi.x; po.y = zi.y + beta * pi.y;
      st2(xv + i, xo, nts != 0);
      st2(pv + i, po, nts != 0);
    }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    if (first) p[n - 1] = z[n - 1];
    else { const double pi = p[n - 1]; x[n - 1] = x[n - 1] + a * pi; p[n - 1] = z[n - 1] + beta * pi; }
  }
}
__global__ __launch_bounds__(PTB) void pcgp_dir_kernel(int64_t n, const PcgState *__restrict__ st, double *__restrict__ x, double *__restrict__ p,
                                                       const double *__restrict__ z) {
  if (st->frozen) return;
  const bool first = st->first != 0;
  const double a = st->alpha, beta = st->beta;
  int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (; i < n; i += stride) {
    if (first) p[i] = z[i];
    else { const double pi = p[i]; x[i] = x[i] + a * pi; p[i] = z[i] + beta * pi; }
  }
}
// Residual pass in place, pcg_resid_vec_kernel / pcg_resid_kernel with a from the state block: r ← r − a·q with the ‖r‖² partials
// ([2][gridDim.x], the second sum zero so that k_dot2_finish folds them).  Frozen: r and the partials stay as they are; RES ignores the fold.
__global__ __launch_bounds__(PTB) void pcgp_resid_vec_kernel(int64_t n, const PcgState *__restrict__ st, double *__restrict__ r, const double *__restrict__ q,
                                                             double *__restrict__ part, int nts) {
  if (st->frozen) return;
  const double a = st->alpha;
  __shared__ double sh[PTB / 64];
  const int64_t n2 = n >> 1;
  vd2 *__restrict__ rv = reinterpret_cast<vd2 *>(r);
  const vd2 *__restrict__ qv = reinterpret_cast<const vd2 *>(q);
  double s0 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x; i < n2; i += stride) {
    const vd2 ri = rv[i], qi = qv[i]; vd2 o;
    o.x = ri.x - a * qi.x; o.y = ri.y - a * qi.y;
    st2(rv + i, o, nts != 0);
    s0 += o.x * o.x; s0 += o.y * o.y;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) { const double ri = r[n - 1] - a * q[n - 1]; r[n - 1] = ri; s0 += ri * ri; }
  BLAS1_FOLD1(s0, sh, part, true);
}
__global__ __launch_bounds__(PTB) void pcgp_resid_kernel(int64_t n, const PcgState *__restrict__ st, double *__restrict__ r, const double *__restrict__ q,
                                                         double *__restrict__ part) {
  if (st->frozen) return;
  const double a = st->alpha;
  __shared__ double sh[PTB / 64];
  double s0 = 0.0;
  int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (; i < n; i += stride) { const double ri = r[i] - a * q[i]; r[i] = ri; s0 += ri * ri; }
  BLAS1_FOLD1(s0, sh, part, true);
}
// Flush: x ← x + a·p when `pending` (mgs_pcg: mgs_axpby(alpha, p, 1, x) = a·p + 1·x, the same bits: 1·x is exact and the sum commutes).
// Not predicated on `frozen`: it is the frozen solve whose x lags.
__global__ __launch_bounds__(PTB) void pcgp_flush_vec_kernel(int64_t n, const PcgState *__restrict__ st, double *__restrict__ x, const double *__restrict__ p, int nts) {
  if (!st->pending) return;
  const double a = st->alpha;
  const int64_t n2 = n >> 1;
  vd2 *__restrict__ xv = reinterpret_cast<vd2 *>(x);
  const vd2 *__restrict__ pv = reinterpret_cast<const vd2 *>(p);
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x; i < n2; i += stride) {
    const vd2 pi = pv[i], xi = xv[i]; vd2 xo;
    xo.x = a * pi.x + xi.x; xo.y = a * pi.y + xi.y;
    st2(xv + i, xo, nts != 0);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) x[n - 1] = a * p[n - 1] + x[n - 1];
}
__global__ __launch_bounds__(PTB) void pcgp_flush_kernel(int64_t n, const PcgState *__restrict__ st, double *__restrict__ x, const double *__restrict__ p) {
  if (!st->pending) return;
  const double a = st->alpha;
  int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (; i < n; i += stride) x[i] = a * p[i] + x[i];
}

}   // namespace

struct mgs_pcg_plan : krylov::Plan<PcgState> {
  mgs_pcg_plan() { name = "mgs_pcg_plan"; }
  int flexible = 0;
  mgs_vec r, z, p, q;                 // views into block, in this order
};

namespace {
int step(mgs_pcg_plan *P, int which, int it, double val, bool post) {
  mgs_ctx *ctx = P->ctx;
  Slot *slot = P->next_slot(post);
  hipLaunchKernelGGL(pcgp_step_kernel, dim3(1), dim3(64), 0, ctx->stream, which, P->st, ctx->red_dev + RED, it, val, P->flexible, slot, P->seq);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

int launch_direction(mgs_pcg_plan *P, double *x) {
  mgs_ctx *ctx = P->ctx; const int64_t n = P->n;
  if (!n) return MGS_OK;
  if (ctx->opt_blas1_vec && al16(x))
    hipLaunchKernelGGL(pcgp_dir_vec_kernel, dim3(mgs_blas1_grid(ctx, (n + 1) / 2)), dim3(PTB), 0, ctx->stream, n, P->st, x, P->p.d, P->z.d, nts_of(ctx, n));
  else
    hipLaunchKernelGGL(pcgp_dir_kernel, dim3(mgs_blas1_grid_capped(ctx, n)), dim3(PTB), 0, ctx->stream, n, P->st, x, P->p.d, P->z.d);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
// the grids, the partial buffer and the fold of k_pcg_residual
int launch_residual(mgs_pcg_plan *P) {
  mgs_ctx *ctx = P->ctx; const int64_t n = P->n;
  if (ctx->opt_blas1_vec) {
    const int nb = mgs_blas1_grid(ctx, (n + 1) / 2);
    double *part = ctx->red_dev;
    if (nb > MGS_DOT_BLOCKS / 2) { MGS_TRY(mgs_ensure_dot_part(ctx, 2 * (int64_t)nb)); part = ctx->dot_part; }
    hipLaunchKernelGGL(pcgp_resid_vec_kernel, dim3(nb), dim3(PTB), 0, ctx->stream, n, P->st, P->r.d, P->q.d, part, nts_of(ctx, n));
    MGS_HIP(ctx, hipGetLastError());
    return k_dot2_finish(ctx, nb, part, nullptr);
  }
  int nb = (int)((n + PTB - 1) / PTB);
  if (nb > MGS_DOT_BLOCKS / 2) nb = MGS_DOT_BLOCKS / 2;
  if (nb < 1) nb = 1;
  hipLaunchKernelGGL(pcgp_resid_kernel, dim3(nb), dim3(PTB), 0, ctx->stream, n, P->st, P->r.d, P->q.d, ctx->red_dev);
  MGS_HIP(ctx, hipGetLastError());
  return k_dot2_finish(ctx, nb, ctx->red_dev, nullptr);
}
int launch_flush(mgs_pcg_plan *P, double *x) {
  mgs_ctx *ctx = P->ctx; const int64_t n = P->n;
  if (n) {
    if (ctx->opt_blas1_vec && al16(x))
      hipLaunchKernelGGL(pcgp_flush_vec_kernel, dim3(mgs_blas1_grid(ctx, (n + 1) / 2)), dim3(PTB), 0, ctx->stream, n, P->st, x, P->p.d, nts_of(ctx, n));
    else
      hipLaunchKernelGGL(pcgp_flush_kernel, dim3(mgs_blas1_grid_capped(ctx, n)), dim3(PTB), 0, ctx->stream, n, P->st, x, P->p.d);
    MGS_HIP(ctx, hipGetLastError());
  }
  return step(P, STEP_FLUSHED, 0, 0.0, false);
}
// r = b − A·x (constant null space: Π(b − A·x)) with ‖r‖² folded into red_dev[RED]
int launch_true_residual(mgs_pcg_plan *P, const mgs_vec *xv, const mgs_vec *bv) {
  MGS_TRY(mgs_residual(P->A, xv, bv, &P->r));
  return P->ns ? k_project_const_nrm2_fold(P->ctx, P->n, P->r.d) : k_dot(P->ctx, P->n, P->r.d, P->r.d, nullptr);
}
// INIT: ‖b‖ (‖Πb‖), the initial residual, the freeze with (status 0, it 0) when it is below tol already
int enqueue_init(mgs_pcg_plan *P, const mgs_vec *xv, const mgs_vec *bv, double tol, bool post) {
  mgs_ctx *ctx = P->ctx;
  if (P->ns) MGS_TRY(k_const_dev_nrm2_fold(ctx, P->n, bv->d)); else MGS_TRY(k_dot(ctx, P->n, bv->d, bv->d, nullptr));
  MGS_TRY(step(P, STEP_NORMB, 0, 0.0, false));
  MGS_TRY(launch_true_residual(P, xv, bv));
  return step(P, STEP_INIT, 0, tol, post);
}
// `first`: the host's copy of the state's flag for an iteration that runs unfrozen (a frozen one launches the same kernels and uses none)
int enqueue_iteration(mgs_pcg_plan *P, mgs_vec *xv, int it, double tol, bool first, bool post) {
  mgs_ctx *ctx = P->ctx; const int64_t n = P->n;
  if (P->h) MGS_TRY(mgs_vcycle(P->h, &P->r, &P->z, 1)); else MGS_TRY(mgs_vec_copy(&P->r, &P->z));
  if (P->ns) MGS_TRY(k_project_const(ctx, n, P->z.d));                               // z ← Πz: the preconditioner seen is ΠMΠ
  if (P->flexible && !first) MGS_TRY(k_dot2(ctx, n, P->r.d, P->z.d, P->q.d, P->z.d, nullptr));
  else MGS_TRY(k_dot(ctx, n, P->r.d, P->z.d, nullptr));
  MGS_TRY(step(P, STEP_RHO, it, 0.0, false));
  MGS_TRY(launch_direction(P, xv->d));
  MGS_TRY(mgs_spmv_dots(P->A, P->p.d, P->q.d, P->p.d, nullptr));                     // q = A·p with p·q from the same pass
  MGS_TRY(step(P, STEP_PQ, it, 0.0, false));
  MGS_TRY(launch_residual(P));
  P->enq_iters++;
  return step(P, STEP_RES, it, tol, post);
}
}   // namespace

int mgs_pcg_plan_destroy(mgs_pcg_plan *P) {
  if (!P) return MGS_OK;
  P->release();
  delete P;
  return MGS_OK;
}

int mgs_pcg_plan_create(const mgs_csr *A, mgs_hier *h, int flexible, mgs_pcg_plan **out) {
  mgs_ctx *ctx = A ? A->ctx : (h ? h->ctx : nullptr);
  MGS_CHECK(ctx, A && out, MGS_ERR_INVALID, "mgs_pcg_plan_create: NULL argument");
  mgs_pcg_plan *P = new mgs_pcg_plan();
  int rc = P->validate(A, h, "mgs_pcg_plan_create", "row shards are served by mgs_pcg");
  if (rc == MGS_OK && !(flexible || !h || (h->nu1 == h->nu2 && h->kcycle_levels <= 0 && !h->kcycle_entry)))
    rc = mgs_fail(ctx, MGS_ERR_INVALID, "mgs_pcg_plan_create: flexible = 0 needs a fixed symmetric preconditioner (nu1 == nu2, no K-cycle); pass flexible = 1");
  if (rc == MGS_OK) rc = P->allocate("mgs_pcg_plan_create", 4);
  if (rc != MGS_OK) { mgs_pcg_plan_destroy(P); return rc; }
  P->flexible = flexible ? 1 : 0;
  P->r = P->view(0); P->z = P->view(1); P->p = P->view(2); P->q = P->view(3);
  // the partial sums of every reduction a solve launches, and the hierarchy's operands and captured cycle (one cycle on r = 1): no later call allocates
  const int64_t nb = std::max<int64_t>(mgs_row_blocks(A), mgs_blas1_grid(ctx, ((int64_t)P->n + 1) / 2));
  rc = mgs_ensure_dot_part(ctx, 2 * std::max<int64_t>(nb, 1));
  if (rc == MGS_OK && h) rc = k_fill(ctx, P->r.d, P->n, 1.0);
  if (rc == MGS_OK && h) rc = mgs_vcycle(h, &P->r, &P->z, 1);
  if (rc != MGS_OK) { mgs_pcg_plan_destroy(P); return rc; }
  *out = P;
  return MGS_OK;
}

int mgs_pcg_plan_enqueue(mgs_pcg_plan *P, mgs_vec *x, const mgs_vec *b, int iters, double tol) {
  MGS_CHECK(P ? P->ctx : nullptr, P && x && b, MGS_ERR_INVALID, "mgs_pcg_plan_enqueue: NULL argument");
  mgs_ctx *ctx = P->ctx;
  MGS_CHECK(ctx, iters >= 0, MGS_ERR_INVALID, "mgs_pcg_plan_enqueue: iters = %d < 0", iters);
  MGS_TRY(P->check_call(x, b, "mgs_pcg_plan_enqueue"));
  mgs_vec xv, bv;
  P->begin_call(x, b, &xv, &bv, true);
  MGS_TRY(enqueue_init(P, &xv, &bv, tol, false));
  for (int i = 1; i <= iters; ++i) MGS_TRY(enqueue_iteration(P, &xv, i, tol, i == 1, false));
  // FINAL: the predicated flush, the projection, the true residual, the status
  MGS_TRY(launch_flush(P, xv.d));
  if (P->ns) MGS_TRY(k_project_const(ctx, P->n, xv.d));
  MGS_TRY(launch_true_residual(P, &xv, &bv));
  MGS_TRY(step(P, STEP_FINAL, iters, tol, false));
  return P->snapshot();
}

int mgs_pcg_plan_result(mgs_pcg_plan *P, int *iters_done, double *resid, int *status) {
  MGS_CHECK(P ? P->ctx : nullptr, P, MGS_ERR_INVALID, "mgs_pcg_plan_result: NULL plan");
  return P->result("mgs_pcg_plan_result", iters_done, resid, nullptr, status);
}

int mgs_pcg_plan_info(const mgs_pcg_plan *P, int64_t out[6]) {
  MGS_CHECK(P ? P->ctx : nullptr, P && out, MGS_ERR_INVALID, "mgs_pcg_plan_info: NULL argument");
  P->info(out);
  return MGS_OK;
}

int mgs_pcg_plan_solve(mgs_pcg_plan *P, mgs_vec *x, const mgs_vec *b, int ahead, int *max_iter, double *tol, int *status) {
  MGS_CHECK(P ? P->ctx : nullptr, P && x && b && max_iter && tol && status, MGS_ERR_INVALID, "mgs_pcg_plan_solve: NULL argument");
  mgs_ctx *ctx = P->ctx;
  MGS_CHECK(ctx, ahead >= 0, MGS_ERR_INVALID, "mgs_pcg_plan_solve: ahead = %d < 0", ahead);
  MGS_TRY(P->check_call(x, b, "mgs_pcg_plan_solve"));
  const int n = P->n;
  mgs_vec xv, bv;
  P->begin_call(x, b, &xv, &bv, false);
  const int maxit = *max_iter;
  const double tl = *tol;
  Lookahead la(maxit, ahead);
  int proj_it = -1;                                   // x was projected after this iteration's update (−1: never)
  // mgs_pcg's `done`: x is flushed by the caller; x ← Πx unless no update has touched it since the last projection
  auto done = [&](int it, int st, double resid, bool updated) -> int {
    if (P->ns && (updated || proj_it < 0)) MGS_TRY(k_project_const(ctx, n, xv.d));
    MGS_TRY(P->snapshot());
    MGS_TRY(mgs_sync(ctx));
    P->wasted = P->snap->wasted;
    P->res_it = it; P->res_status = st; P->res_resid = resid;
    *max_iter = it; *tol = resid; *status = st;
    return MGS_OK;
  };
  MGS_TRY(enqueue_init(P, &xv, &bv, tl, true));
  la.enqueued(P->seq);
  bool first = true;
  Look L = {0, -1, 0, 0, 0, 0, 0.0, 1.0};
  for (;;) {
    while (la.may_enqueue()) {
      MGS_TRY(enqueue_iteration(P, &xv, la.next, tl, first, true));
      first = false;
      la.enqueued(P->seq);
    }
    if (la.idle()) break;                             // every iteration up to maxit has been seen and none froze
    MGS_TRY(P->wait_post(la.take(), &L));
    if (!L.frozen) continue;
    const int i = L.it;
    if (L.status == 2 || L.status == 3) {             // x holds every completed update: flush what the iteration before left pending
      MGS_TRY(launch_flush(P, xv.d));
      return done(i, L.status, L.resid, i - 1 > proj_it);
    }
    if (i == 0) return done(0, 0, L.resid, false);    // the initial residual is a true one
    // the recursion says converged at iteration i: the true residual decides (a synchronising look, as in mgs_pcg)
    MGS_TRY(launch_flush(P, xv.d));
    if (P->ns) MGS_TRY(k_project_const(ctx, n, xv.d));
    proj_it = i;
    MGS_TRY(mgs_residual(P->A, &xv, &bv, &P->r));
    double s = 0;
    if (P->ns) { double s2[2]; MGS_TRY(k_project_const_nrm2(ctx, n, P->r.d, s2)); s = s2[0]; }
    else MGS_TRY(k_dot(ctx, n, P->r.d, P->r.d, &s));
    const double resid = std::sqrt(s) / L.normb;
    if (resid < tl) return done(i, 0, resid, false);
    if (i == maxit) return done(maxit, 1, resid, false);
    // the recursion had drifted: r holds the true residual, start over from it.  The iterations enqueued past i ran frozen and are enqueued again.
    MGS_TRY(step(P, STEP_RESTART, i, resid, false));
    P->restarts++;
    first = true; la.restart(i);
    L.frozen = 0; L.resid = resid; L.it = i;
  }
  // the iterations are used up (maxit = 0: INIT alone, nothing pending)
  MGS_TRY(launch_flush(P, xv.d));
  return done(maxit, 1, L.resid, maxit > proj_it);
}
