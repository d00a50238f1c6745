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

#include "krylov_plan.hpp"

namespace {
using namespace krylov;

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
enum { STEP_NORMB = 0, STEP_INIT, STEP_RHO, STEP_ALPHA, STEP_HALF, STEP_OMEGA, STEP_RES, STEP_FINAL };

// The scalar steps: one wave, lane 0 works.  red = ctx->red_dev + RED.  `it`: the iteration the step belongs to (FINAL: the iterations
// enqueued); `tol`: the tolerance (INIT, HALF, RES, FINAL); slot = NULL: nothing is posted.
__global__ void bcgp_step_kernel(int step, BcgState *__restrict__ st, const double *__restrict__ red, int it, double tol, Slot *slot, unsigned long long ticket) {
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

// p-pass (:100-104): first: p ← r; else p = 1.0·r + nbo·v + beta·p, axpbypcz_kernel's expression with its c == 0.0 branch (which does not read p).
// The state is read once per workgroup through uniform loads; a frozen workgroup returns at once.
__global__ __launch_bounds__(PTB) void bcgp_p_vec_kernel(int64_t n, const BcgState *__restrict__ st, const double *__restrict__ r, const double *__restrict__ v,
                                                         double *__restrict__ p, int nts) {
  if (st->frozen) return;
  const bool first = st->first != 0;
  const double b = st->nbo, c = st->beta;
  const int64_t n2 = n >> 1;
  const vd2 *__restrict__ rv = reinterpret_cast<const vd2 *>(r);
  const vd2 *__restrict__ vv = reinterpret_cast<const vd2 *>(v);
  vd2 *__restrict__ pv = reinterpret_cast<vd2 *>(p);
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x; i < n2; i += stride) {
    const vd2 ri = rv[i]; vd2 q;
    if (first) q = ri;
    else {
      const vd2 o = vv[i];
      if (c == 0.0) { q.x = 1.0 * ri.x + b * o.x; q.y = 1.0 * ri.y + b * o.y; }
      else { const vd2 w = pv[i]; q.x = 1.0 * ri.x + b * o.x + c * w.x; q.y = 1.0 * ri.y + b * o.y + c * w.y; }
    }
    st2(pv + i, q, nts != 0);
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
  const vd2 *__restrict__ pv = reinterpret_cast<const vd2 *>(ph);
  const vd2 *__restrict__ sv = reinterpret_cast<const vd2 *>(sh);
  vd2 *__restrict__ xv = reinterpret_cast<vd2 *>(x);
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x; i < n2; i += stride) {
    const vd2 pi = pv[i], xi = xv[i]; vd2 q;
    if (frozen) { q.x = a * pi.x + 1.0 * xi.x; q.y = a * pi.y + 1.0 * xi.y; }
    else { const vd2 si = sv[i]; q.x = a * pi.x + b * si.x + 1.0 * xi.x; q.y = a * pi.y + b * si.y + 1.0 * xi.y; }
    st2(xv + i, q, nts != 0);
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
  const vd2 *__restrict__ xv = reinterpret_cast<const vd2 *>(x);
  const vd2 *__restrict__ yv = reinterpret_cast<const vd2 *>(y);
  const vd2 *__restrict__ wv = reinterpret_cast<const vd2 *>(w);
  vd2 *__restrict__ zv = reinterpret_cast<vd2 *>(z);
  double s0 = 0.0, s1 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * PTB;
  for (int64_t i = (int64_t)blockIdx.x * PTB + threadIdx.x; i < n2; i += stride) {
    const vd2 p = xv[i], o = yv[i]; vd2 q;
    q.x = a * p.x + b * o.x; q.y = a * p.y + b * o.y;
    st2(zv + i, q, nts != 0);
    s0 += q.x * q.x; s0 += q.y * q.y;
    if (OMEGA) { const vd2 ww = wv[i]; s1 += ww.x * q.x; s1 += ww.y * q.y; }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double zi = a * x[n - 1] + b * y[n - 1];
    z[n - 1] = zi; s0 += zi * zi;
    if (OMEGA) s1 += w[n - 1] * zi;
  }
  BLAS1_FOLD2(s0, s1, sh, part);
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
  BLAS1_FOLD2(s0, s1, sh, part);
}
}   // namespace

struct mgs_bicgstab_plan : krylov::Plan<BcgState> {
  mgs_bicgstab_plan() { name = "mgs_bicgstab_plan"; }
  mgs_vec p, ph, s, sh, t, v, r, rt;  // p, p̂, s, ŝ, t, v, r, r̃: views into block, in this order
};

namespace {
int step(mgs_bicgstab_plan *P, int which, int it, double tol, bool post) {
  mgs_ctx *ctx = P->ctx;
  Slot *slot = P->next_slot(post);
  hipLaunchKernelGGL(bcgp_step_kernel, dim3(1), dim3(64), 0, ctx->stream, which, P->st, ctx->red_dev + RED, it, tol, slot, P->seq);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

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
}   // namespace

int mgs_bicgstab_plan_destroy(mgs_bicgstab_plan *P) {
  if (!P) return MGS_OK;
  P->release();
  delete P;
  return MGS_OK;
}

int mgs_bicgstab_plan_create(const mgs_csr *A, mgs_hier *h, mgs_bicgstab_plan **out) {
  mgs_ctx *ctx = A ? A->ctx : (h ? h->ctx : nullptr);
  MGS_CHECK(ctx, A && out, MGS_ERR_INVALID, "mgs_bicgstab_plan_create: NULL argument");
  mgs_bicgstab_plan *P = new mgs_bicgstab_plan();
  int rc = P->validate(A, h, "mgs_bicgstab_plan_create", "row shards are served by mgs_bicgstab");
  if (rc == MGS_OK) rc = P->allocate("mgs_bicgstab_plan_create", 8);
  if (rc != MGS_OK) { mgs_bicgstab_plan_destroy(P); return rc; }
  mgs_vec *vs[8] = {&P->p, &P->ph, &P->s, &P->sh, &P->t, &P->v, &P->r, &P->rt};
  for (int k = 0; k < 8; ++k) *vs[k] = P->view(k);
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
  MGS_TRY(P->check_call(x, b, "mgs_bicgstab_plan_enqueue"));
  mgs_vec xv, bv;
  P->begin_call(x, b, &xv, &bv, true);
  MGS_TRY(enqueue_init(P, &xv, &bv, tol, false));
  for (int i = 1; i <= iters; ++i) MGS_TRY(enqueue_iteration(P, &xv, i, tol, false));
  // FINAL: the projection of x, the true residual into t, the status
  if (P->ns) MGS_TRY(k_project_const(ctx, P->n, xv.d));
  MGS_TRY(mgs_residual(P->A, &xv, &bv, &P->t));
  if (P->ns) MGS_TRY(k_project_const_nrm2_fold(ctx, P->n, P->t.d)); else MGS_TRY(k_dot(ctx, P->n, P->t.d, P->t.d, nullptr));
  MGS_TRY(step(P, STEP_FINAL, iters, tol, false));
  return P->snapshot();
}

int mgs_bicgstab_plan_result(mgs_bicgstab_plan *P, int *iters_done, double *resid, double *recursive_resid, int *status) {
  MGS_CHECK(P ? P->ctx : nullptr, P, MGS_ERR_INVALID, "mgs_bicgstab_plan_result: NULL plan");
  return P->result("mgs_bicgstab_plan_result", iters_done, resid, recursive_resid, status);
}

int mgs_bicgstab_plan_info(const mgs_bicgstab_plan *P, int64_t out[6]) {
  MGS_CHECK(P ? P->ctx : nullptr, P && out, MGS_ERR_INVALID, "mgs_bicgstab_plan_info: NULL argument");
  P->info(out);                                       // out[5] = 0: no restart branch (bicg.cpp has none)
  return MGS_OK;
}

int mgs_bicgstab_plan_solve(mgs_bicgstab_plan *P, mgs_vec *x, const mgs_vec *b, int ahead, int *max_iter, double *tol, int *status) {
  MGS_CHECK(P ? P->ctx : nullptr, P && x && b && max_iter && tol && status, MGS_ERR_INVALID, "mgs_bicgstab_plan_solve: NULL argument");
  mgs_ctx *ctx = P->ctx;
  MGS_CHECK(ctx, ahead >= 0, MGS_ERR_INVALID, "mgs_bicgstab_plan_solve: ahead = %d < 0", ahead);
  MGS_TRY(P->check_call(x, b, "mgs_bicgstab_plan_solve"));
  const int n = P->n;
  mgs_vec xv, bv;
  P->begin_call(x, b, &xv, &bv, false);
  const int maxit = *max_iter;
  const double tl = *tol;
  Lookahead la(maxit, ahead);
  MGS_TRY(enqueue_init(P, &xv, &bv, tl, true));
  la.enqueued(P->seq);
  Look L = {0, -1, 0, 0, 0, 0, 0.0, 1.0};
  while (!L.frozen) {
    while (la.may_enqueue()) {
      MGS_TRY(enqueue_iteration(P, &xv, la.next, tl, true));
      la.enqueued(P->seq);
    }
    if (la.idle()) break;                             // every iteration up to maxit has been seen and none froze
    MGS_TRY(P->wait_post(la.take(), &L));
  }
  // fin(): x ← Πx after its last update (a frozen iteration past the freeze touches no x), then the call waits for the stream as mgs_bicgstab does
  if (P->ns) MGS_TRY(k_project_const(ctx, n, xv.d));
  MGS_TRY(P->snapshot());
  MGS_TRY(mgs_sync(ctx));
  P->wasted = P->snap->wasted;
  const int st = L.frozen ? L.status : 1;             // :134-135: the iterations are used up
  if (st == 0) *max_iter = L.it;                      // :90, :113, :125; statuses 2 and 3 leave *max_iter as it is (:96-99, :128-131)
  *tol = L.resid; *status = st;
  P->res_it = L.frozen ? L.it : std::max(maxit, 0); P->res_status = st; P->res_resid = L.resid; P->res_rec = L.resid;
  return MGS_OK;
}
