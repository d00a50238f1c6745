// minres.hip — preconditioned MINRES for symmetric indefinite systems (mgs_minres) and the one vector pass of its own (k_minres_update).
// gfx950 only.  The method is the form of Elman, Silvester and Wathen, Alg. 4.1 (Paige-Saunders): Lanczos vectors v and preconditioned
// vectors z̃ = M·v stored unnormalised, γ = √(z̃·v).  tests/minres_ref.py restates every statement below.
#include "blas1.hpp"

// every product, sum and quotient of this unit is rounded on its own (the build's -ffp-contract=off, spelled out: update_ref states the bits)
#pragma clang fp contract(off)

namespace {
using namespace blas1;

// ------------------------------------------------------------------ the update pass
// w_new = ((1/γ)·z̃ − a3·w_prev − a2·w)/a1 over w_prev's storage, x ← x + step·w_new.  Four read streams, two write streams, 48 B per row.
// The quotient is a division by a1 (correctly rounded: no fast-math), not a product with a reciprocal.
__device__ __forceinline__ double minres_entry(double inv_g, double a3, double a2, double a1, double z, double wp, double w) {
  double t = inv_g * z - a3 * wp;
  t = t - a2 * w;
  return t / a1;
}
__global__ void minres_update_kernel(int64_t n, double inv_g, double a3, double a2, double a1, double step, const double *__restrict__ z,
                                     double *__restrict__ w_prev, const double *__restrict__ w, double *__restrict__ x) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const double wn = minres_entry(inv_g, a3, a2, a1, z[i], w_prev[i], w[i]);
    w_prev[i] = wn;
    x[i] = x[i] + step * wn;
  }
}
// 16-byte form (same per-element expressions: same bits).  nts: w_prev leaves with the streaming store (it is read again two passes later);
// x is read again by the next pass and keeps plain stores.
__global__ __launch_bounds__(TB) void minres_update_vec_kernel(int64_t n, double inv_g, double a3, double a2, double a1, double step,
                                                               const double *__restrict__ z, double *__restrict__ w_prev,
                                                               const double *__restrict__ w, double *__restrict__ x, int nts) {
  const int64_t n2 = n >> 1;
  const vd2 *__restrict__ zv = reinterpret_cast<const vd2 *>(z);
  vd2 *__restrict__ pv = reinterpret_cast<vd2 *>(w_prev);
  const vd2 *__restrict__ wv = reinterpret_cast<const vd2 *>(w);
  vd2 *__restrict__ xv = reinterpret_cast<vd2 *>(x);
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n2; i += stride) {
    const vd2 zi = zv[i], pi = pv[i], wi = wv[i], xi = xv[i]; vd2 wn, xo;
    wn.x = minres_entry(inv_g, a3, a2, a1, zi.x, pi.x, wi.x);
    wn.y = minres_entry(inv_g, a3, a2, a1, zi.y, pi.y, wi.y);
    xo.x = xi.x + step * wn.x; xo.y = xi.y + step * wn.y;
    st2(pv + i, wn, nts != 0);
    xv[i] = xo;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double wn = minres_entry(inv_g, a3, a2, a1, z[n - 1], w_prev[n - 1], w[n - 1]);
    w_prev[n - 1] = wn;
    x[n - 1] = x[n - 1] + step * wn;
  }
}
}   // namespace

int k_minres_update(mgs_ctx *ctx, int64_t n, double inv_g, double a3, double a2, double a1, double step,
                    const double *z, double *w_prev, const double *w, double *x) {
  if (!n) return MGS_OK;
  if (ctx->opt_blas1_vec && al16(z) && al16(w_prev) && al16(w) && al16(x)) {
    const dim3 g(mgs_blas1_grid(ctx, (n + 1) / 2));
    const int nts = ctx->opt_minres_nt && nts_of(ctx, n);
    hipLaunchKernelGGL(minres_update_vec_kernel, g, dim3(TB), 0, ctx->stream, n, inv_g, a3, a2, a1, step, z, w_prev, w, x, nts);
  } else
    hipLaunchKernelGGL(minres_update_kernel, dim3(mgs_blas1_grid_capped(ctx, n)), dim3(TB), 0, ctx->stream, n, inv_g, a3, a2, a1, step, z, w_prev, w, x);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

extern "C" {

// Preconditioned MINRES for symmetric A (indefinite allowed) with a symmetric positive definite preconditioner M: short recurrences, one
// cycle and one SpMV per iteration, a residual that is monotone in the M⁻¹ norm.  Nearest reference line: src/CPU_Matlab/solve.m:28-33, whose
// driver chooses between pcg and bicgstab — the reference has no MINRES.
// Seven work vectors from the context's pool (v ×2, z̃ ×2, q, w ×2), returned last-taken-first so that a repeated solve finds them at the same
// addresses; the cycle is applied to two alternating (v, z̃) pairs and replays from two cached graph slots.  Per iteration beside cycle and SpMV:
//   * mgs_spmv_dots(A, z̃, q, z̃):  q = A·z̃ with q·z̃ from the same pass                     (host look 1)
//   * k_axpbypcz:                  v_new = (1/γ)·q − (δ/γ)·v − (γ/γ_prev)·v_prev over v_prev   32 B per row
//   * k_dot:                       z̃_new·v_new                                               16 B per row (host look 2)
//   * k_minres_update:             w_new over w_prev, x ← x + (cn·η)·w_new                     48 B per row
// 96 B per row of vector passes (mgs_pcg: 80).  |η| is ‖r‖ in the M⁻¹ norm, not the 2-norm: est = κ·|η|/‖b‖ with κ = ‖r‖₂/‖r‖_{M⁻¹} as last
// measured; when est falls below tol the TRUE residual b − A·x decides (formed into q, which is free there), and where it does not confirm,
// κ is recalibrated from it and the recurrence goes on undisturbed — no restart, no tuned constant.  Every return writes the true relative
// residual to *tol: one more SpMV where none was just made.
int mgs_minres(const mgs_csr *A, mgs_vec *x, const mgs_vec *b, mgs_hier *h, int *max_iter, double *tol, int *status) {
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, max_iter && tol && status, MGS_ERR_INVALID, "mgs_minres: NULL out parameter");
  MGS_CHECK(ctx, !h || (h->nu1 == h->nu2 && h->kcycle_levels <= 0 && !h->kcycle_entry), MGS_ERR_INVALID,
            "mgs_minres: needs a fixed symmetric preconditioner (nu1 == nu2, no K-cycle)");
  MGS_CHECK(ctx, A->rows == A->cols && !ctx->ncomm && !ctx->allreduce, MGS_ERR_INVALID, "mgs_minres: the matrix is %d x %d%s (row shards are served by mgs_bicgstab)", A->rows, A->cols,
            A->cols > A->rows ? ", halo columns: a row shard" : (A->rows == A->cols ? ", on a context that sums over ranks" : ", not square"));
  MGS_CHECK(ctx, A->rows > 0, MGS_ERR_INVALID, "mgs_minres: the matrix has no rows");
  if (h) {
    bool shard = h->halo || h->halo_begin || h->halo_end || h->halo_fused || h->coarse || h->native || h->ntail;
    for (const mgs_level &L : h->lev) shard = shard || L.nx || (L.A && L.A->cols > L.A->rows);
    MGS_CHECK(ctx, !shard, MGS_ERR_INVALID, "mgs_minres: the hierarchy has halo columns, exchange callbacks, native plans or a tail (row shards are served by mgs_bicgstab)");
    MGS_CHECK(ctx, h->ctx == ctx && !h->lev.empty() && h->lev[0].n == A->rows, MGS_ERR_INVALID, "mgs_minres: the hierarchy's fine level has %d rows, A has %d",
              h->lev.empty() ? 0 : h->lev[0].n, A->rows);
  }
  MGS_CHECK(ctx, A->nullspace != MGS_NULLSPACE_CONSTANT && (!h || h->lev[0].A->nullspace != MGS_NULLSPACE_CONSTANT), MGS_ERR_INVALID,
            "mgs_minres: a declared constant null space is not served (the constant vector is not the null space of a saddle system; declare the fields: mgs_csr_set_nullspace_fields)");
  bool ns = false;                                         // MGS_NULLSPACE_FIELDS: K·x = Πb, every projection through the dispatch on A's record
  MGS_TRY(mgs_krylov_nullspace(A, h, "mgs_minres", &ns, true));
  const int n = A->rows;
  MGS_CHECK(ctx, x->n >= n && b->n >= n, MGS_ERR_INVALID, "mgs_minres: vectors shorter than %d", n);
  MGS_CHECK(ctx, x->d != b->d, MGS_ERR_INVALID, "mgs_minres: x must not alias b");
  MGS_TRY(mgs_csr_optimize(const_cast<mgs_csr *>(A)));
  mgs_vec *v[2] = {0, 0}, *zt[2] = {0, 0}, *q = 0, *w[2] = {0, 0};
  krylov_frame f{ctx, h, n, ns, true, {}, A};      // returned last-taken-first: the next solve takes the same vectors in the same roles
  for (mgs_vec **t : {&v[0], &zt[0], &v[1], &zt[1], &q, &w[0], &w[1]}) MGS_TRY(f.take(t, n));
  mgs_vec xv = f.view(x), bv = f.view(b);
  double normb = 0, resid = 0, s = 0, d2[2] = {0, 0};
  auto precond = [&](const mgs_vec *in, mgs_vec *out) -> int {      // z̃ = M·v; fields: z̃ = Π(M·v), the preconditioner seen is ΠMΠ
    MGS_TRY(h ? mgs_vcycle(h, in, out, 1) : mgs_vec_copy(in, out));
    return ns ? k_ns_project(A, n, out->d) : MGS_OK;
  };
  auto true_residual = [&](mgs_vec *into) -> int {        // into = b − A·x, resid = ‖into‖/‖b‖; fields: x ← Πx first, into = Π(b − A·x), resid = ‖into‖/‖Πb‖
    if (ns) {
      double s2[2];
      MGS_TRY(k_ns_project(A, n, xv.d));
      MGS_TRY(mgs_residual(A, &xv, &bv, into));
      MGS_TRY(k_ns_project_nrm2(A, n, into->d, s2));
      s = s2[0];
    } else {
      MGS_TRY(mgs_residual(A, &xv, &bv, into));
      MGS_TRY(k_dot(ctx, n, into->d, into->d, &s));
    }
    resid = std::sqrt(s) / normb;
    return MGS_OK;
  };
  auto done = [&](int it, int st) -> int { *max_iter = it; *tol = resid; *status = st; return mgs_sync(ctx); };
  MGS_TRY(f.norm_b(bv, &normb));
  MGS_TRY(true_residual(v[0]));                            // v = b − A·x
  if (resid <= *tol) return done(0, 0);
  MGS_TRY(precond(v[0], zt[0]));                           // z̃ = M·v
  double g2 = 0;
  MGS_TRY(k_dot(ctx, n, zt[0]->d, v[0]->d, &g2));
  if (!(g2 > 0)) return done(0, 2);                        // the preconditioner is not positive definite (or not a number)
  double gam = std::sqrt(g2), gam_prev = 1, eta = gam, kappa = resid * normb / gam;
  double s0 = 0, s1 = 0, c0 = 1, c1 = 1;
  for (mgs_vec *t : {v[1], w[0], w[1]}) MGS_TRY(k_fill(ctx, t->d, n, 0.0));   // v_prev = w_prev = w = 0 (a pool vector may hold anything, 0·NaN = NaN)
  int cur = 0, wc = 1;                                     // (v, z̃) = (v[cur], zt[cur]), v_prev = v[1 − cur]; w = w[wc], w_prev = w[1 − wc]
  const int maxit = *max_iter;
  for (int j = 1; j <= maxit; ++j) {
    mgs_vec *vc = v[cur], *vp = v[1 - cur], *zc = zt[cur], *zn = zt[1 - cur];
    MGS_TRY(mgs_spmv_dots(A, zc->d, q->d, zc->d, d2));    // q = A·z̃ with q·z̃ from the same pass
    const double delta = d2[0] / (gam * gam);
    MGS_TRY(k_axpbypcz(ctx, n, 1.0 / gam, q->d, -(delta / gam), vc->d, -(gam / gam_prev), vp->d));   // v_new over v_prev
    MGS_TRY(precond(vp, zn));                              // z̃_new = M·v_new
    double gn2 = 0;
    MGS_TRY(k_dot(ctx, n, zn->d, vp->d, &gn2));
    if (!(gn2 >= 0)) { MGS_TRY(true_residual(q)); return done(j, 2); }
    const double gamn = std::sqrt(gn2);
    const double a0 = c1 * delta - c0 * s1 * gam;
    const double a1 = std::sqrt(a0 * a0 + gn2);
    const double a2 = s1 * delta + c0 * c1 * gam;
    const double a3 = s0 * gam;
    if (a1 == 0) { MGS_TRY(true_residual(q)); return done(j, 3); }      // x is not updated
    const double cn = a0 / a1, sn = gamn / a1;
    MGS_TRY(k_minres_update(ctx, n, 1.0 / gam, a3, a2, a1, cn * eta, zc->d, w[1 - wc]->d, w[wc]->d, xv.d));   // w_new over w_prev, x ← x + (cn·η)·w_new
    eta = -sn * eta;
    cur = 1 - cur; wc = 1 - wc;
    s0 = s1; s1 = sn; c0 = c1; c1 = cn; gam_prev = gam; gam = gamn;
    bool fresh = false;                                    // resid holds the true residual of the present x
    if (kappa * std::fabs(eta) / normb < *tol || gamn == 0) {
      MGS_TRY(true_residual(q)); fresh = true;
      if (resid < *tol) return done(j, 0);
      if (gamn == 0) return done(j, 3);                    // the Krylov space is exhausted above the tolerance
      kappa = resid * normb / std::fabs(eta);              // recalibrate; the recurrence goes on undisturbed
    }
    if (j == maxit && !fresh) MGS_TRY(true_residual(q));
  }
  return done(maxit < 0 ? 0 : maxit, 1);                   // (no iteration allowed: resid is the start's true residual)
}

}  // extern "C"
