// minres_plan.hip — preconditioned MINRES whose scalars never leave the device (mgs_minres_plan, include/mgs.h).
// Nearest reference line: src/CPU_Matlab/solve.m:28-33; the reference has neither MINRES nor an asynchronous form.
//
// mgs_minres (minres.hip) forms δ, the Lanczos coefficients, the Givens rotation and the stopping estimate on the host: two host looks per
// iteration (q·z̃ and z̃_new·v_new), each one draining the queue behind it.  Here the same scalars live in one state block in device memory.
// One-wave "scalar step" kernels turn the folded inner products the reductions leave in red_dev[MGS_DOT_BLOCKS ..] into the next scalars
// with the very operations, in the order, of mgs_minres's host code (no fast-math in this build: FP64 division and sqrt are correctly
// rounded; contraction is off), and the two vector passes take their coefficients from the state block instead of from kernel arguments:
// the Lanczos pass with the expression and the arms of axpbypcz_kernel / axpbypcz_vec_kernel, the update pass with minres_entry's expression
// and the arms of k_minres_update.  Everything else is the launches mgs_minres makes — mgs_residual, mgs_spmv_dots, k_dot, the cycle on the
// two (v[k], z̃[k]) pairs, k_fill — called with a NULL host pointer, which enqueues and folds without fetching.  So the bits of every vector
// agree with mgs_minres's.
//
// One iteration j is a fixed launch sequence; (v, z̃) = (v[c], z̃[c]) with c = (j − 1) & 1, w = w[1 − c], and the other of each pair is the
// one before (the host picks the roles by the parity of j, so a solve that goes on after a refused check resumes with the right ones):
//   SpMV     q = A·z̃ with q·z̃ from the same pass
//   LANCZOS  (step) δ = (q·z̃)/(γ·γ); a = 1/γ, b = −(δ/γ), c = −(γ/γ_prev); frozen: counts into `wasted`, clears `apply`
//   pass     v_new = a·q + b·v + c·v_prev over v_prev
//   cycle    z̃_new = M·v_new (a copy when h is NULL)
//   dot      γn² = z̃_new·v_new
//   ROTATE   (step) γn² negative or not a number: frozen, status 2.  a0 = c1·δ − c0·s1·γ, a1 = √(a0·a0 + γn²), a2 = s1·δ + c0·c1·γ,
//            a3 = s0·γ; a1 == 0: frozen, status 3 (x not updated).  cn = a0/a1, sn = γn/a1; step = cn·η, `apply` set; η ← −sn·η; the
//            rotation of (s0, s1, c0, c1, γ_prev, γ); est = κ·|η|/‖b‖; est < tol or γn == 0: frozen, status 0, `why`.  The post.
//   pass     `apply`: w_new = ((1/γ)·z̃ − a3·w_prev − a2·w)/a1 over w_prev, x ← x + step·w_new
// Two step launches: δ must exist before the Lanczos pass and γn² after the cycle, and nothing else orders the scalars.  The iteration
// that freezes as "converged" still applies its update (mgs_minres updates x before it tests): the update pass is predicated on `apply`,
// which ROTATE sets and the next LANCZOS step clears, not on `frozen`.
//
// Frozen iterations still run SpMV, cycle and folds, and here that is not only scratch: a frozen iteration's cycle rewrites a z̃ from its
// unchanged v, and every second one of them rewrites the live z̃.  The bits are the same because the cycle is deterministic (a replayed
// graph of kernels with fixed summation orders); q is formed again by the next unfrozen iteration before it is read.
//
// ROTATE and INIT also post (iteration, status, frozen, wasted, why, resid, ‖b‖) and a ticket into the plan's ring in mapped host memory.
// mgs_minres_plan_solve looks at one slot per iteration, `ahead` iterations behind the queue; on a posted freeze with status 0 it forms the
// true residual into q (a synchronising look, as in mgs_minres) and returns, or enqueues the recalibration step (κ = resid·‖b‖/|η| with
// the true residual passed by value, `frozen` cleared) and enqueues again the iterations that ran frozen.  The recurrence is never
// restarted.  mgs_minres_plan_enqueue never looks; it has no recalibration on the device: FINAL reports status 1 with fewer iterations
// done than asked for when the estimate ran ahead of the 2-norm, and the caller enqueues again from x, which measures κ afresh.
#include <algorithm>
#include <cmath>

#include "krylov_plan.hpp"

// every product, sum and quotient of this unit is rounded on its own, as in minres.hip
#pragma clang fp contract(off)

namespace {
using namespace krylov;

// the state block.  status: −1 running, 0 the estimate says converged or γn == 0 (the true residual still decides), 2 z̃·v not positive
// (INIT) / negative or not a number, 3 a1 == 0; after FINAL: mgs_minres's status.  resid: the estimate κ·|η|/‖b‖; after INIT the initial
// true residual
struct MinresState {
  double normb, gam, gam_prev, eta, kappa, delta, s0, s1, c0, c1;
  double la, lb, lc;                      // the Lanczos pass: v_new = la·q + lb·v + lc·v_prev
  double inv_g, a3, a2, a1, step;         // the update pass
  double resid, true_resid;
  int it;        // the last iteration that ran unfrozen (the one that froze, once frozen)
  int status;
  int frozen;
  int why;       // of a freeze with status 0: WHY_EST the estimate fell below tol, WHY_GAMMA γn == 0 (both may be set)
  int wasted;    // iterations that ran frozen
  int apply;     // this iteration's update is to be applied
};
enum { WHY_EST = 1, WHY_GAMMA = 2 };
enum { STEP_NORMB = 0, STEP_INIT_RES, STEP_INIT, STEP_LANCZOS, STEP_ROTATE, STEP_RECAL, STEP_FINAL };

// The scalar steps: one wave, lane 0 works.  red = ctx->red_dev + RED.  `it`: the iteration the step belongs to (FINAL: the iterations
// enqueued); `val`: the tolerance (INIT_RES, ROTATE, FINAL) or the true residual the host found (RECAL); slot = NULL: nothing is posted.
__global__ void minp_step_kernel(int step, MinresState *__restrict__ st, const double *__restrict__ red, int it, double val, Slot *slot, unsigned long long ticket) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  switch (step) {
    case STEP_NORMB: {                      // ‖b‖, 0 replaced by 1; a fresh state
      double nb = sqrt(red[0]);
      if (nb == 0.0) nb = 1.0;
      st->normb = nb;
      st->gam = st->gam_prev = st->eta = st->kappa = st->delta = st->s0 = st->s1 = st->c0 = st->c1 = 0.0;
      st->la = st->lb = st->lc = st->inv_g = st->a3 = st->a2 = st->a1 = st->step = st->resid = st->true_resid = 0.0;
      st->it = 0; st->status = -1; st->frozen = 0; st->why = 0; st->wasted = 0; st->apply = 0;
      break;
    }
    case STEP_INIT_RES: {                   // the initial (true) residual
      st->resid = sqrt(red[0]) / st->normb;
      st->true_resid = st->resid;
      if (st->resid <= val) { st->frozen = 1; st->status = 0; }
      break;
    }
    case STEP_INIT: {                       // g2 = z̃·v
      if (!st->frozen) {
        const double g2 = red[0];
        if (!(g2 > 0.0)) { st->frozen = 1; st->status = 2; }                  // the preconditioner is not positive definite (or not a number)
        else {
          const double gam = sqrt(g2);
          st->gam = gam; st->gam_prev = 1.0; st->eta = gam; st->kappa = st->resid * st->normb / gam;
          st->s0 = 0.0; st->s1 = 0.0; st->c0 = 1.0; st->c1 = 1.0;
        }
      }
      if (slot) post_slot(slot, st, ticket, &st->why);
      break;
    }
    case STEP_LANCZOS: {
      st->apply = 0;
      if (st->frozen) { st->wasted += 1; break; }
      st->it = it;
      const double gam = st->gam;
      const double delta = red[0] / (gam * gam);
      st->delta = delta;
      st->la = 1.0 / gam; st->lb = -(delta / gam); st->lc = -(gam / st->gam_prev);
      break;
    }
    case STEP_ROTATE: {
      if (!st->frozen) {
        const double gn2 = red[0];
        const double gam = st->gam, delta = st->delta, eta = st->eta, s0 = st->s0, s1 = st->s1, c0 = st->c0, c1 = st->c1;
        if (!(gn2 >= 0.0)) { st->frozen = 1; st->status = 2; }
        else {
          const double gamn = sqrt(gn2);
          const double a0 = c1 * delta - c0 * s1 * gam;
          const double a1 = sqrt(a0 * a0 + gn2);
          const double a2 = s1 * delta + c0 * c1 * gam;
          const double a3 = s0 * gam;
          if (a1 == 0.0) { st->frozen = 1; st->status = 3; }                 // x is not updated
          else {
            const double cn = a0 / a1, sn = gamn / a1;
            st->inv_g = 1.0 / gam; st->a3 = a3; st->a2 = a2; st->a1 = a1; st->step = cn * eta; st->apply = 1;
            const double etan = -sn * eta;
            st->eta = etan;
            st->s0 = s1; st->s1 = sn; st->c0 = c1; st->c1 = cn; st->gam_prev = gam; st->gam = gamn;
            st->resid = st->kappa * fabs(etan) / st->normb;
            const int why = (st->resid < val ? WHY_EST : 0) | (gamn == 0.0 ? WHY_GAMMA : 0);
            if (why) { st->frozen = 1; st->status = 0; st->why = why; }      // the true residual decides
          }
        }
      }
      if (slot) post_slot(slot, st, ticket, &st->why);
      break;
    }
    case STEP_RECAL:                        // the true residual did not confirm: κ from it; the recurrence goes on undisturbed
      st->kappa = val * st->normb / fabs(st->eta);
      st->resid = val; st->true_resid = val;
      st->frozen = 0; st->status = -1; st->why = 0; st->apply = 0;
      break;
    case STEP_FINAL: {                      // after q = b − A·x: red[0] = ‖q‖²
      st->true_resid = sqrt(red[0]) / st->normb;
      st->apply = 0;
      if (!st->frozen) { st->it = it; st->status = 1; }
      else if (st->status == 0) {
        if (st->it == 0 ? st->true_resid <= val : st->true_resid < val) st->status = 0;
        else st->status = (st->why & WHY_GAMMA) ? 3 : 1;
      }
      st->frozen = 1;
      break;
    }
  }
}

// Lanczos pass, axpbypcz_vec_kernel / axpbypcz_kernel with a, b, c from the state block: z ← a·x + b·y + c·z, left to right, and the
// c == 0.0 form that does not read z.  The state is read once per workgroup through uniform loads; a frozen workgroup returns at once.
__global__ __launch_bounds__(PTB) void minp_lanczos_vec_kernel(int64_t n, const MinresState *__restrict__ st, const double *__restrict__ x, const double *__restrict__ y,
                                                               double *__restrict__ z, int nts) {
  if (st->frozen) return;
  const double a = st->la, b = st->lb, c = st->lc;
  const bool hasc = !(c == 0.0);
  const int64_t n2 = n >> 1;
  const vd2 *__restrict__ xv = reinterpret_cast<const vd2 *>(x);
  const vd2 *__restrict__ yv = reinterpret_cast<const vd2 *>(y);
  vd2 *__restrict__ zv = reinterpret_cast<vd2 *>(z);
  const int64_t stride = (int64_t)gridDim.x * PTB;
  if (hasc) {      // (no unroll request: grid_vec's workgroups are one-shot, a lane runs one trip)
    for (int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x; i < n2; i += stride) {
      const vd2 p = xv[i], o = yv[i], w = zv[i]; vd2 q;
      q.x = a * p.x + b * o.x + c * w.x; q.y = a * p.y + b * o.y + c * w.y;
      st2(zv + i, q, nts != 0);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x; i < n2; i += stride) {
      const vd2 p = xv[i], o = yv[i]; vd2 q;
      q.x = a * p.x + b * o.x; q.y = a * p.y + b * o.y;
      st2(zv + i, q, nts != 0);
    }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) z[n - 1] = hasc ? a * x[n - 1] + b * y[n - 1] + c * z[n - 1] : a * x[n - 1] + b * y[n - 1];
}
__global__ __launch_bounds__(PTB) void minp_lanczos_kernel(int64_t n, const MinresState *__restrict__ st, const double *__restrict__ x, const double *__restrict__ y,
                                                           double *__restrict__ z) {
  if (st->frozen) return;
  const double a = st->la, b = st->lb, c = st->lc;
  int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * PTB;
  if (c == 0.0) { for (; i < n; i += stride) z[i] = a * x[i] + b * y[i]; }
  else { for (; i < n; i += stride) z[i] = a * x[i] + b * y[i] + c * z[i]; }
}

// Update pass, minres_update_vec_kernel / minres_update_kernel (minres.hip) with (1/γ, a3, a2, a1, step) from the state block.  Predicated
// on `apply`: the iteration that froze as converged still updates x, a frozen iteration behind it does not.
__device__ __forceinline__ double minp_entry(double inv_g, double a3, double a2, double a1, double z, double wp, double w) {
  double t = inv_g * z - a3 * wp;
  t = t - a2 * w;
  return t / a1;
}
__global__ __launch_bounds__(PTB) void minp_update_vec_kernel(int64_t n, const MinresState *__restrict__ st, const double *__restrict__ z, double *__restrict__ w_prev,
                                                              const double *__restrict__ w, double *__restrict__ x, int nts) {
  if (!st->apply) return;
  const double inv_g = st->inv_g, a3 = st->a3, a2 = st->a2, a1 = st->a1, step = st->step;
  const int64_t n2 = n >> 1;
  const vd2 *__restrict__ zv = reinterpret_cast<const vd2 *>(z);
  vd2 *__restrict__ pv = reinterpret_cast<vd2 *>(w_prev);
  const vd2 *__restrict__ wv = reinterpret_cast<const vd2 *>(w);
  vd2 *__restrict__ xv = reinterpret_cast<vd2 *>(x);
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x; i < n2; i += stride) {
    const vd2 zi = zv[i], pi = pv[i], wi = wv[i], xi = xv[i]; vd2 wn, xo;
    wn.x = minp_entry(inv_g, a3, a2, a1, zi.x, pi.x, wi.x);
    wn.y = minp_entry(inv_g, a3, a2, a1, zi.y, pi.y, wi.y);
    xo.x = xi.x + step * wn.x; xo.y = xi.y + step * wn.y;
    st2(pv + i, wn, nts != 0);
    xv[i] = xo;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double wn = minp_entry(inv_g, a3, a2, a1, z[n - 1], w_prev[n - 1], w[n - 1]);
    w_prev[n - 1] = wn;
    x[n - 1] = x[n - 1] + step * wn;
  }
}
__global__ __launch_bounds__(PTB) void minp_update_kernel(int64_t n, const MinresState *__restrict__ st, const double *__restrict__ z, double *__restrict__ w_prev,
                                                          const double *__restrict__ w, double *__restrict__ x) {
  if (!st->apply) return;
  const double inv_g = st->inv_g, a3 = st->a3, a2 = st->a2, a1 = st->a1, step = st->step;
  int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (; i < n; i += stride) {
    const double wn = minp_entry(inv_g, a3, a2, a1, z[i], w_prev[i], w[i]);
    w_prev[i] = wn;
    x[i] = x[i] + step * wn;
  }
}

}   // namespace

struct mgs_minres_plan : krylov::Plan<MinresState> {
  mgs_minres_plan() { name = "mgs_minres_plan"; }
  mgs_vec v[2], zt[2], q, w[2];       // views into block, in the order v0, z̃0, v1, z̃1, q, w0, w1
};

namespace {
int step(mgs_minres_plan *P, int which, int it, double val, bool post) {
  mgs_ctx *ctx = P->ctx;
  Slot *slot = P->next_slot(post);
  hipLaunchKernelGGL(minp_step_kernel, dim3(1), dim3(64), 0, ctx->stream, which, P->st, ctx->red_dev + RED, it, val, slot, P->seq);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
// k_axpbypcz's launch decisions (the plan's vectors are 256-byte aligned)
int launch_lanczos(mgs_minres_plan *P, const double *x, const double *y, double *z) {
  mgs_ctx *ctx = P->ctx; const int64_t n = P->n;
  if (!n) return MGS_OK;
  if (ctx->opt_blas1_vec && al16(x) && al16(y) && al16(z))
    hipLaunchKernelGGL(minp_lanczos_vec_kernel, dim3(mgs_blas1_grid(ctx, (n + 1) / 2)), dim3(PTB), 0, ctx->stream, n, P->st, x, y, z, nts_of(ctx, n));
  else
    hipLaunchKernelGGL(minp_lanczos_kernel, dim3(mgs_blas1_grid_capped(ctx, n)), dim3(PTB), 0, ctx->stream, n, P->st, x, y, z);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
// k_minres_update's launch decisions: x may be the caller's misaligned view, then the 8-byte arm runs
int launch_update(mgs_minres_plan *P, const double *z, double *w_prev, const double *w, double *x) {
  mgs_ctx *ctx = P->ctx; const int64_t n = P->n;
  if (!n) return MGS_OK;
  if (ctx->opt_blas1_vec && al16(z) && al16(w_prev) && al16(w) && al16(x)) {
    const int nts = ctx->opt_minres_nt && nts_of(ctx, n);
    hipLaunchKernelGGL(minp_update_vec_kernel, dim3(mgs_blas1_grid(ctx, (n + 1) / 2)), dim3(PTB), 0, ctx->stream, n, P->st, z, w_prev, w, x, nts);
  } else
    hipLaunchKernelGGL(minp_update_kernel, dim3(mgs_blas1_grid_capped(ctx, n)), dim3(PTB), 0, ctx->stream, n, P->st, z, w_prev, w, x);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
// z̃ = M·v; MGS_NULLSPACE_FIELDS (P->ns): z̃ = Π(M·v), the projection enqueued behind the cycle with its means on the device, as in mgs_minres
int precond(mgs_minres_plan *P, const mgs_vec *in, mgs_vec *out) {
  MGS_TRY(P->h ? mgs_vcycle(P->h, in, out, 1) : mgs_vec_copy(in, out));
  return P->ns ? k_ns_project(P->A, P->n, out->d) : MGS_OK;
}
// into = b − A·x with ‖into‖² folded into red_dev[RED]; fields: x ← Πx first, into = Π(b − A·x), its norm² from the shift pass.  host2: fetch (a synchronising look)
int launch_true_residual(mgs_minres_plan *P, mgs_vec *xv, const mgs_vec *bv, mgs_vec *into, double *host2 = nullptr) {
  if (P->ns) {
    MGS_TRY(k_ns_project(P->A, P->n, xv->d));
    MGS_TRY(mgs_residual(P->A, xv, bv, into));
    return k_ns_project_nrm2(P->A, P->n, into->d, host2);
  }
  MGS_TRY(mgs_residual(P->A, xv, bv, into));
  return k_dot(P->ctx, P->n, into->d, into->d, host2);
}
// INIT: mgs_minres's start.  Nothing behind the first freeze test depends on the host: a start that is frozen runs the cycle and the fills all the same
int enqueue_init(mgs_minres_plan *P, mgs_vec *xv, const mgs_vec *bv, double tol, bool post) {
  mgs_ctx *ctx = P->ctx; const int64_t n = P->n;
  if (P->ns) MGS_TRY(k_ns_dev_nrm2(P->A, n, bv->d, nullptr));      // ‖Πb‖², b only read
  else MGS_TRY(k_dot(ctx, n, bv->d, bv->d, nullptr));
  MGS_TRY(step(P, STEP_NORMB, 0, 0.0, false));
  MGS_TRY(launch_true_residual(P, xv, bv, &P->v[0]));                                 // v = b − A·x
  MGS_TRY(step(P, STEP_INIT_RES, 0, tol, false));
  MGS_TRY(precond(P, &P->v[0], &P->zt[0]));                                           // z̃ = M·v
  MGS_TRY(k_dot(ctx, n, P->zt[0].d, P->v[0].d, nullptr));
  MGS_TRY(step(P, STEP_INIT, 0, 0.0, post));
  for (mgs_vec *t : {&P->v[1], &P->w[0], &P->w[1]}) MGS_TRY(k_fill(ctx, t->d, n, 0.0));   // v_prev = w_prev = w = 0
  return MGS_OK;
}
int enqueue_iteration(mgs_minres_plan *P, mgs_vec *xv, int it, double tol, bool post) {
  mgs_ctx *ctx = P->ctx; const int64_t n = P->n;
  const int cur = (it - 1) & 1, wc = 1 - cur;        // mgs_minres: cur = 0, wc = 1 at j = 1, both flip every iteration
  mgs_vec *vc = &P->v[cur], *vp = &P->v[1 - cur], *zc = &P->zt[cur], *zn = &P->zt[1 - cur];
  MGS_TRY(mgs_spmv_dots(P->A, zc->d, P->q.d, zc->d, nullptr));                        // q = A·z̃ with q·z̃ from the same pass
  MGS_TRY(step(P, STEP_LANCZOS, it, 0.0, false));
  MGS_TRY(launch_lanczos(P, P->q.d, vc->d, vp->d));                                   // v_new over v_prev
  MGS_TRY(precond(P, vp, zn));                                                        // z̃_new = M·v_new
  MGS_TRY(k_dot(ctx, n, zn->d, vp->d, nullptr));
  P->enq_iters++;
  MGS_TRY(step(P, STEP_ROTATE, it, tol, post));
  return launch_update(P, zc->d, P->w[1 - wc].d, P->w[wc].d, xv->d);                  // w_new over w_prev, x ← x + step·w_new
}
}   // namespace

extern "C" {

int mgs_minres_plan_destroy(mgs_minres_plan *P) {
  if (!P) return MGS_OK;
  P->release();
  delete P;
  return MGS_OK;
}

int mgs_minres_plan_create(const mgs_csr *A, mgs_hier *h, mgs_minres_plan **out) {
  mgs_ctx *ctx = A ? A->ctx : (h ? h->ctx : nullptr);
  MGS_CHECK(ctx, A && out, MGS_ERR_INVALID, "mgs_minres_plan_create: NULL argument");
  MGS_CHECK(ctx, !h || (h->nu1 == h->nu2 && h->kcycle_levels <= 0 && !h->kcycle_entry), MGS_ERR_INVALID,
            "mgs_minres_plan_create: needs a fixed symmetric preconditioner (nu1 == nu2, no K-cycle)");
  mgs_minres_plan *P = new mgs_minres_plan();
  int rc = P->validate(A, h, "mgs_minres_plan_create", "row shards are served by mgs_bicgstab");
  if (rc == MGS_OK && !(A->nullspace != MGS_NULLSPACE_CONSTANT && (!h || h->lev[0].A->nullspace != MGS_NULLSPACE_CONSTANT)))
    rc = mgs_fail(ctx, MGS_ERR_INVALID, "mgs_minres_plan_create: a declared constant null space is not served (the constant vector is not the null space of a saddle system; declare the fields: mgs_csr_set_nullspace_fields)");
  if (rc == MGS_OK) rc = P->allocate("mgs_minres_plan_create", 7, true);
  if (rc != MGS_OK) { mgs_minres_plan_destroy(P); return rc; }
  mgs_vec *vs[7] = {&P->v[0], &P->zt[0], &P->v[1], &P->zt[1], &P->q, &P->w[0], &P->w[1]};
  for (int k = 0; k < 7; ++k) *vs[k] = P->view(k);
  // the partial sums of every reduction a solve launches, and the hierarchy's operands and both captured cycles (v[k] → z̃[k] on ones): no later call allocates
  const int64_t nb = std::max<int64_t>(mgs_row_blocks(A), mgs_blas1_grid(ctx, ((int64_t)P->n + 1) / 2));
  if (rc == MGS_OK) rc = mgs_ensure_dot_part(ctx, (P->ns ? MGS_NULLSPACE_MAX_FIELDS : 2) * std::max<int64_t>(nb, 1));      // (fields: [nfields][workgroups] partials of the projection's sum pass)
  for (int k = 0; k < 2 && h; ++k) {
    if (rc == MGS_OK) rc = k_fill(ctx, P->v[k].d, P->n, 1.0);
    if (rc == MGS_OK) rc = mgs_vcycle(h, &P->v[k], &P->zt[k], 1);
  }
  if (rc != MGS_OK) { mgs_minres_plan_destroy(P); return rc; }
  *out = P;
  return MGS_OK;
}

int mgs_minres_plan_enqueue(mgs_minres_plan *P, mgs_vec *x, const mgs_vec *b, int iters, double tol) {
  MGS_CHECK(P ? P->ctx : nullptr, P && x && b, MGS_ERR_INVALID, "mgs_minres_plan_enqueue: NULL argument");
  mgs_ctx *ctx = P->ctx;
  MGS_CHECK(ctx, iters >= 0, MGS_ERR_INVALID, "mgs_minres_plan_enqueue: iters = %d < 0", iters);
  MGS_TRY(P->check_call(x, b, "mgs_minres_plan_enqueue"));
  mgs_vec xv, bv;
  P->begin_call(x, b, &xv, &bv, true);
  MGS_TRY(enqueue_init(P, &xv, &bv, tol, false));
  for (int i = 1; i <= iters; ++i) MGS_TRY(enqueue_iteration(P, &xv, i, tol, false));
  // FINAL: the true residual into q, the status
  MGS_TRY(launch_true_residual(P, &xv, &bv, &P->q));
  MGS_TRY(step(P, STEP_FINAL, iters, tol, false));
  return P->snapshot();
}

int mgs_minres_plan_result(mgs_minres_plan *P, int *iters_done, double *resid, double *recursive_resid, int *status) {
  MGS_CHECK(P ? P->ctx : nullptr, P, MGS_ERR_INVALID, "mgs_minres_plan_result: NULL plan");
  return P->result("mgs_minres_plan_result", iters_done, resid, recursive_resid, status);
}

int mgs_minres_plan_info(const mgs_minres_plan *P, int64_t out[6]) {
  MGS_CHECK(P ? P->ctx : nullptr, P && out, MGS_ERR_INVALID, "mgs_minres_plan_info: NULL argument");
  P->info(out);                                       // out[5]: recalibrations (the base's `restarts`)
  return MGS_OK;
}

int mgs_minres_plan_solve(mgs_minres_plan *P, mgs_vec *x, const mgs_vec *b, int ahead, int *max_iter, double *tol, int *status) {
  MGS_CHECK(P ? P->ctx : nullptr, P && x && b && max_iter && tol && status, MGS_ERR_INVALID, "mgs_minres_plan_solve: NULL argument");
  mgs_ctx *ctx = P->ctx;
  MGS_CHECK(ctx, ahead >= 0, MGS_ERR_INVALID, "mgs_minres_plan_solve: ahead = %d < 0", ahead);
  MGS_TRY(P->check_call(x, b, "mgs_minres_plan_solve"));
  mgs_vec xv, bv;
  P->begin_call(x, b, &xv, &bv, false);
  const int maxit = *max_iter;
  const double tl = *tol;
  Lookahead la(maxit, ahead);
  double est = 0.0;                                   // what the last look saw: the estimate (INIT: the initial true residual)
  auto done = [&](int it, int st, double resid) -> int {
    MGS_TRY(P->snapshot());
    MGS_TRY(mgs_sync(ctx));
    P->wasted = P->snap->wasted;
    P->res_it = it; P->res_status = st; P->res_resid = resid; P->res_rec = est;
    *max_iter = it; *tol = resid; *status = st;
    return MGS_OK;
  };
  auto true_residual = [&](double normb, double *resid) -> int {      // q = b − A·x, *resid = ‖q‖/‖b‖: a synchronising look, as in mgs_minres
    double s2[2] = {0, 0};
    MGS_TRY(launch_true_residual(P, &xv, &bv, &P->q, s2));
    *resid = std::sqrt(s2[0]) / normb;
    return MGS_OK;
  };
  MGS_TRY(enqueue_init(P, &xv, &bv, tl, true));
  la.enqueued(P->seq);
  Look L = {0, -1, 0, 0, 0, 0, 0.0, 1.0};
  double resid = 0.0;
  for (;;) {
    while (la.may_enqueue()) {
      MGS_TRY(enqueue_iteration(P, &xv, la.next, tl, true));
      la.enqueued(P->seq);
    }
    if (la.idle()) break;                             // every iteration up to maxit has been seen and none froze
    MGS_TRY(P->wait_post(la.take(), &L));
    est = L.resid;
    if (!L.frozen) continue;
    const int i = L.it;
    if (i == 0) return done(0, L.status, L.resid);    // the start: converged already (0) or z̃·v not positive (2); the initial residual is a true one
    MGS_TRY(true_residual(L.normb, &resid));
    if (L.status == 2 || L.status == 3) return done(i, L.status, resid);
    // the estimate says converged, or γn == 0, at iteration i: the true residual decides
    if (resid < tl) return done(i, 0, resid);
    if (L.aux0 & WHY_GAMMA) return done(i, 3, resid); // the Krylov space is exhausted above the tolerance
    if (i == maxit) return done(maxit, 1, resid);
    // recalibrate; the recurrence goes on undisturbed.  The iterations enqueued past i ran frozen and are enqueued again.
    MGS_TRY(step(P, STEP_RECAL, i, resid, false));
    P->restarts++;
    la.restart(i);
    L.frozen = 0; L.it = i;
  }
  // the iterations are used up (maxit <= 0: INIT alone, its residual is a true one)
  if (maxit <= 0) return done(0, 1, L.resid);
  MGS_TRY(true_residual(L.normb, &resid));
  return done(maxit, 1, resid);
}

}  // extern "C"
