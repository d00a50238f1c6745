// krylov.hip — the host-driven Krylov solvers (mgs_bicgstab, mgs_pcg, mgs_fgcr), the context's pool of work vectors and the null-space
// rule they share with the plans.  No kernel lives here; every numeric step is a launch on the context's stream.
#include "mgs_internal.hpp"

#include <algorithm>
#include <cmath>

// Work vectors of the solvers come from the context and go back to it: a solve no longer pays 8 × (hipMalloc + memset + hipFree,
// the last one a device synchronisation) per call, and — what matters more — a repeated solve finds its vectors at the SAME
// addresses, so the captured cycles keyed by (rhs, out) are replayed instead of captured again.  The solvers write every vector
// before they read it; only the halo slots behind the owned entries of a row shard are cleared on reuse.
int mgs_ws_get(mgs_ctx *ctx, int64_t n, int64_t owned, mgs_vec **out) {
  for (size_t i = ctx->ws_free.size(); i-- > 0;) {
    if (ctx->ws_free[i]->n == n) {
      *out = ctx->ws_free[i]; ctx->ws_free.erase(ctx->ws_free.begin() + (long)i);
      if (n > owned) MGS_HIP(ctx, hipMemsetAsync((*out)->d + owned, 0, sizeof(double) * (size_t)(n - owned), ctx->stream));
      return MGS_OK;
    }
  }
  return mgs_vec_create(ctx, n, out);
}
void mgs_ws_put(mgs_ctx *ctx, mgs_vec *v) {
  if (!v) return;
  if (ctx->ws_free.size() >= 24) { mgs_vec *old = ctx->ws_free.front(); ctx->ws_free.erase(ctx->ws_free.begin()); mgs_vec_destroy(old); }
  ctx->ws_free.push_back(v);
}

// A declared MGS_NULLSPACE_CONSTANT: the solvers below solve A·x = Πb, Π = I − 1·1ᵀ/n (k_project_const), and return the x of zero mean.
// *ns_out = whether to project.  Refused: a declared row shard; a hierarchy whose fine operator carries another kind than A.
// A declared MGS_NULLSPACE_FIELDS: served by the callers that say so (mgs_minres, mgs_minres_plan, mgs_pcg: Π = I − Σ_f z_f·z_fᵀ/n_f through the
// dispatch k_ns_project*), refused by every other one.  The hierarchy's fine operator must then carry the same number of fields with the same
// rows per field; that the two label arrays agree entry by entry is the caller's responsibility (mgs.h).
int mgs_krylov_nullspace(const mgs_csr *A, const mgs_hier *h, const char *who, bool *ns_out, bool serves_fields) {
  mgs_ctx *ctx = A->ctx;
  const bool fields = A->nullspace == MGS_NULLSPACE_FIELDS;
  const bool hfields = h && h->lev[0].A->nullspace == MGS_NULLSPACE_FIELDS;
  MGS_CHECK(ctx, serves_fields || !(fields || hfields), MGS_ERR_INVALID, "%s: a field-wise null space (MGS_NULLSPACE_FIELDS) is declared; it is served by mgs_minres / mgs_pcg", who);
  const bool ns = fields || A->nullspace == MGS_NULLSPACE_CONSTANT;
  MGS_CHECK(ctx, !ns || (A->cols == A->rows && !ctx->ncomm && !ctx->allreduce), MGS_ERR_INVALID, "%s: %s null space declared on a row shard", who, fields ? "field-wise" : "constant");
  MGS_CHECK(ctx, !h || h->lev[0].A->nullspace == A->nullspace, MGS_ERR_INVALID,
            "%s: the hierarchy's fine operator carries null-space kind %d, A carries %d (a hierarchy built for a regular twin of A?)", who, h->lev[0].A->nullspace, A->nullspace);
  if (fields && h) {
    const mgs_nsfields *a = A->nsf, *b = h->lev[0].A->nsf;
    MGS_CHECK(ctx, a->nfields == b->nfields, MGS_ERR_INVALID, "%s: A declares %d fields, the hierarchy's fine operator %d", who, a->nfields, b->nfields);
    for (int f = 0; f < a->nfields; ++f)
      MGS_CHECK(ctx, a->counts[f] == b->counts[f], MGS_ERR_INVALID, "%s: field %d has %lld rows on A and %lld on the hierarchy's fine operator", who, f, (long long)a->counts[f],
                (long long)b->counts[f]);
  }
  *ns_out = ns;
  return MGS_OK;
}

extern "C" {

// BiCGSTABiml, reference src/common/bicg.cpp:74-136, statement by statement on device vectors.
int mgs_bicgstab(const mgs_csr *A, mgs_vec *x, const mgs_vec *b, mgs_hier *h, int *max_iter, double *tol, int *status) {
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, max_iter && tol && status, MGS_ERR_INVALID, "mgs_bicgstab: NULL out parameter");
  bool ns = false;
  MGS_TRY(mgs_krylov_nullspace(A, h, "mgs_bicgstab", &ns));
  MGS_TRY(mgs_csr_optimize(const_cast<mgs_csr *>(A)));
  const int n = A->rows, next = A->cols > n ? A->cols : n;
  MGS_CHECK(ctx, x->n >= n && b->n >= n, MGS_ERR_INVALID, "mgs_bicgstab: vectors shorter than %d", n);
  mgs_vec *p = 0, *phat = 0, *s = 0, *shat = 0, *t = 0, *v = 0, *r = 0, *rt = 0, *xe = 0;
  krylov_frame f{ctx, h, n, ns, false, {}};
  for (mgs_vec **q : {&p, &phat, &s, &shat, &t, &v, &r, &rt}) MGS_TRY(f.take(q, q == &phat || q == &shat ? next : n));
  mgs_vec xv = f.view(x), bv = f.view(b), phv = f.view(phat), shv = f.view(shat);
  const mgs_vec *xin = x;
  if (x->n < next) { MGS_TRY(f.take(&xe, next)); MGS_TRY(mgs_vec_copy(&xv, xe)); xin = xe; }
  auto precond = [&](const mgs_vec *in, mgs_vec *out) -> int {       // M.solve (bicg.cpp:106,116); constant null space: Π·M
    if (!h) { mgs_vec ov = f.view(out); MGS_TRY(mgs_vec_copy(in, &ov)); }
    else MGS_TRY(mgs_vcycle(h, in, out, 1));
    return ns ? k_project_const(ctx, n, out->d) : MGS_OK;
  };
  auto fin = [&]() -> int { if (ns) MGS_TRY(k_project_const(ctx, n, xv.d)); return mgs_sync(ctx); };   // constant null space: x ← Πx after its last update
  double rho_1 = 0, rho_2 = 0, alpha = 0, beta = 0, omega = 0, resid = 0, normb = 0, tmp = 0;
  double d2[2];
  MGS_TRY(f.norm_b(bv, &normb));                                                      // :80, :85-86
  MGS_TRY(f.halo(const_cast<mgs_vec *>(xin)));
  MGS_TRY(mgs_residual(A, xin, &bv, r));                                              // :82
  if (ns) MGS_TRY(k_project_const(ctx, n, r->d));                                     // r = Π(b − A·x)
  MGS_TRY(mgs_vec_copy(r, rt));                                                       // :83
  MGS_TRY(k_dot2(ctx, n, r->d, r->d, rt->d, r->d, d2));             // ‖r‖² and (r̃,r) in one pass / one round trip
  if ((resid = std::sqrt(d2[0]) / normb) <= *tol) { *tol = resid; *max_iter = 0; *status = 0; return ns ? fin() : MGS_OK; }   // :88-92
  for (int i = 1; i <= *max_iter; ++i) {                                              // :94
    rho_1 = d2[1];                                                                    // :95 (computed with the last ‖r‖)
    if (rho_1 == 0) { *tol = std::sqrt(d2[0]) / normb; *status = 2; return ns ? fin() : MGS_OK; }  // :96-99
    if (i == 1) MGS_TRY(mgs_vec_copy(r, p));                                          // :100-101
    else {
      beta = (rho_1 / rho_2) * (alpha / omega);                                       // :103
      MGS_TRY(mgs_axpbypcz(1.0, r, -beta * omega, v, beta, p));                       // :104
    }
    MGS_TRY(precond(p, phat));                                                        // :106
    MGS_TRY(f.halo(phat));
    MGS_TRY(mgs_spmv_dots(A, phat->d, v->d, rt->d, d2)); alpha = rho_1 / d2[0];      // :107-108  v = A·p̂ with r̃·v from the same pass
    MGS_TRY(k_update_dot2(ctx, n, 1.0, r->d, -alpha, v->d, s->d, nullptr, d2));      // :109 s = r − αv, with ‖s‖² in the same pass
    tmp = std::sqrt(d2[0]);
    if ((resid = tmp / normb) < *tol) {                                               // :110-115
      MGS_TRY(mgs_axpby(alpha, &phv, 1.0, &xv));
      *max_iter = i; *tol = resid; *status = 0; return fin();
    }
    MGS_TRY(precond(s, shat));                                                        // :116
    MGS_TRY(f.halo(shat));
    MGS_TRY(mgs_spmv_dots(A, shat->d, t->d, s->d, d2)); omega = d2[0] / d2[1];       // :117-118  t = A·ŝ with (t·s, t·t) from the same pass
    MGS_TRY(mgs_axpbypcz(alpha, &phv, omega, &shv, 1.0, &xv));                        // :119
    MGS_TRY(k_update_dot2(ctx, n, 1.0, s->d, -omega, t->d, r->d, rt->d, d2));       // :120 r = s − ωt with ‖r‖² (:123) and the next (r̃,r) (:95)
    rho_2 = rho_1;                                                                    // :122
    if ((resid = std::sqrt(d2[0]) / normb) < *tol) { *tol = resid; *max_iter = i; *status = 0; return fin(); }   // :123-127
    if (omega == 0) { *tol = resid; *status = 3; return fin(); }              // :128-131
  }
  *tol = resid; *status = 1;                                                          // :134-135
  return fin();
}

// Preconditioned conjugate gradients for symmetric positive definite A: the reference's Matlab driver, src/CPU_Matlab/solve.m:28-31
// (`symm == 1` → pcg).  Four work vectors (r, z, p, q) where BiCGSTAB holds eight, one cycle and one SpMV per iteration where it runs two.
// Beside those an iteration is three vector passes, 80 B per row (88 flexible):
//   * dots:       r·z, flexible also q·z (k_dot / k_dot2);
//   * direction:  x ← x + α_prev·p and p ← z + β·p in ONE pass (k_pcg_direction): the x update of step i rides on the direction pass of
//                 step i + 1, which reads the old p anyway.  `pending` says that x is one step behind; it is flushed (k_axpby) before
//                 every return and before every true-residual pass;
//   * SpMV q = A·p with p·q from its epilogue (mgs_spmv_dots), then the residual in place r ← r − α·q with ‖r‖² (k_pcg_residual).
// flexible: β = z·(r − r_prev)/ρ_prev (Polak-Ribière form, Notay, SISC 22 (2000)) = −α·(z·q)/ρ_prev since r − r_prev = −α·q and q is
// still alive — no fifth vector.  It tolerates a preconditioner that is not a fixed symmetric operator (V(ν1 ≠ ν2), K-cycle).
// Status 0 is reported only on the TRUE residual b − A·x, as mgs_fgcr does; when the recursion said converged and the true residual
// does not, the method restarts from it (p = z).  r and z keep their addresses for the whole solve, and — the vectors go back to the
// pool in reverse order — across solves: the cycle replays from one cached graph slot keyed by (r, z).
int mgs_pcg(const mgs_csr *A, mgs_vec *x, const mgs_vec *b, mgs_hier *h, int flexible, int *max_iter, double *tol, int *status) {
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, max_iter && tol && status, MGS_ERR_INVALID, "mgs_pcg: NULL out parameter");
  MGS_CHECK(ctx, flexible || !h || (h->nu1 == h->nu2 && h->kcycle_levels <= 0 && !h->kcycle_entry), MGS_ERR_INVALID,
            "mgs_pcg: flexible = 0 needs a fixed symmetric preconditioner (nu1 == nu2, no K-cycle); pass flexible = 1");
  bool ns = false;
  MGS_TRY(mgs_krylov_nullspace(A, h, "mgs_pcg", &ns, true));
  MGS_TRY(mgs_csr_optimize(const_cast<mgs_csr *>(A)));
  const int n = A->rows, next = A->cols > n ? A->cols : n;
  MGS_CHECK(ctx, x->n >= n && b->n >= n, MGS_ERR_INVALID, "mgs_pcg: vectors shorter than %d", n);
  mgs_vec *r = 0, *z = 0, *p = 0, *q = 0, *xe = 0;
  krylov_frame f{ctx, h, n, ns, true, {}, A};      // returned last-taken-first so that the next solve takes the same vectors in the same roles
  for (mgs_vec **w : {&r, &z, &p, &q}) MGS_TRY(f.take(w, w == &p ? next : n));
  mgs_vec xv = f.view(x), bv = f.view(b), pv = f.view(p);
  if (x->n < next) MGS_TRY(f.take(&xe, next));
  double normb = 0, resid = 0, rho = 0, rho_prev = 0, alpha = 0, beta = 0, d2[2] = {0, 0};
  bool pending = false;                                    // x is one step behind: x += alpha·p not applied yet
  bool x_mean = ns;                                        // declared null space (constant or field-wise, one dispatch: k_ns_project): x may carry a constant component (the guess's, or an update's rounding)
  auto flush = [&]() -> int {
    if (pending) { MGS_TRY(mgs_axpby(alpha, &pv, 1.0, &xv)); pending = false; }
    return MGS_OK;
  };
  auto project_x = [&]() -> int {                         // x ← Πx (x flushed by the caller): after the last update, before the final true residual
    if (x_mean) { MGS_TRY(k_ns_project(A, n, xv.d)); x_mean = false; }
    return MGS_OK;
  };
  auto true_residual = [&]() -> int {                     // r = b − A·x (x flushed by the caller), resid = ‖r‖/‖b‖; constant null space: r = Π(b − A·x), ‖r‖/‖Πb‖
    mgs_vec *xin = x;
    if (xe) { MGS_TRY(mgs_vec_copy(&xv, xe)); xin = xe; }
    MGS_TRY(f.halo(xin));
    MGS_TRY(mgs_residual(A, xin, &bv, r));
    double s = 0;
    if (ns) { double s2[2]; MGS_TRY(k_ns_project_nrm2(A, n, r->d, s2)); s = s2[0]; }
    else MGS_TRY(k_dot(ctx, n, r->d, r->d, &s));
    resid = std::sqrt(s) / normb;
    return MGS_OK;
  };
  auto done = [&](int it, int st) -> int {
    int rc = flush(); if (rc == MGS_OK) rc = project_x();
    *max_iter = it; *tol = resid; *status = st; return rc != MGS_OK ? rc : mgs_sync(ctx);
  };
  MGS_TRY(f.norm_b(bv, &normb));
  MGS_TRY(true_residual());
  if (resid <= *tol) return done(0, 0);
  const int maxit = *max_iter;
  bool restart = true;                                     // the next direction is p = z
  for (int i = 1; i <= maxit; ++i) {
    if (h) MGS_TRY(mgs_vcycle(h, r, z, 1)); else MGS_TRY(mgs_vec_copy(r, z));
    if (ns) MGS_TRY(k_ns_project(A, n, z->d));        // z ← Πz: the preconditioner seen is ΠMΠ
    if (flexible && !restart) { MGS_TRY(k_dot2(ctx, n, r->d, z->d, q->d, z->d, d2)); rho = d2[0]; }
    else MGS_TRY(k_dot(ctx, n, r->d, z->d, &rho));
    if (!(rho > 0)) return done(i, 2);                     // preconditioner not positive definite (or not a number)
    if (restart) {
      MGS_TRY(flush());
      MGS_TRY(k_pcg_direction(ctx, n, 1, 0.0, 0.0, xv.d, p->d, z->d));
      restart = false;
    } else {
      beta = flexible ? -alpha * d2[1] / rho_prev : rho / rho_prev;
      MGS_TRY(k_pcg_direction(ctx, n, 0, alpha, beta, xv.d, p->d, z->d));
      pending = false;
    }
    MGS_TRY(f.halo(p));
    MGS_TRY(mgs_spmv_dots(A, p->d, q->d, p->d, d2));      // q = A·p with p·q from the same pass
    if (!(d2[0] > 0)) return done(i, 3);                   // A not positive definite along p
    alpha = rho / d2[0]; pending = true; x_mean = ns;
    MGS_TRY(k_pcg_residual(ctx, n, alpha, r->d, q->d, d2));
    resid = std::sqrt(d2[0]) / normb; rho_prev = rho;
    if (resid < *tol) {                                    // the recursion says converged: the true residual decides
      MGS_TRY(flush());
      MGS_TRY(project_x());
      MGS_TRY(true_residual());
      if (resid < *tol) return done(i, 0);
      restart = true;                                      // the recursion had drifted: r holds the true residual, start over from it
    }
  }
  return done(maxit, 1);
}

// Flexible GCR(m): c_k = B_k r (variable preconditioner), v_k = A c_k orthogonalised against the v_j of the restart window, r ← r − α_k v_k.
// Device passes per iteration beside the preconditioner and the SpMV (round 3 ran 8 vector passes and 3 host round trips PER EARLIER
// DIRECTION — 39 % of a 512³ solve outside the preconditioner):
//   * one multi-dot pass: h_j = v_j·v_k for every j < k, v_k read once (classical Gram-Schmidt; the window is ≤ 64 and restarted);
//   * one update pass:    v_k ← v_k − Σ (h_j/ρ_j) v_j with ρ_k = v_k·v_k and t = v_k·r from the same pass;
//   * one residual pass:  r ← r − (t/ρ_k) v_k with ‖r‖²;
// and the directions c_k are NOT orthogonalised at all: with U_jk = h_j/ρ_j (strictly upper triangular) the orthogonalised directions are
// Ĉ = C (I + U)⁻¹, so x − x₀ = Ĉ α = C y with (I + U) y = α — a back substitution on k ≤ 64 numbers on the host and ONE pass
// x ← x + Σ y_j c_j when the window closes (restart, convergence, or the iteration limit).
// The recursively updated residual drifts from b − A·x (finite-precision orthogonality, and a K-cycle is a different operator at every
// call), so the TRUE residual b − A·x replaces it at every restart and decides every return with status 0: the method never reports a
// tolerance it has not reached.  (A sliding window instead of the restart was measured on the CPU restatement,
// tools/kcycle_diag_cpu.py, 64³: K-cycle on all levels 25 iterations restarted, 28–40 with a window of 10 — the restart stays.)
int mgs_fgcr(const mgs_csr *A, mgs_vec *x, const mgs_vec *b, mgs_hier *h, int restart, int *max_iter, double *tol, int *status) {
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, max_iter && tol && status && restart >= 1 && restart <= 64, MGS_ERR_INVALID, "mgs_fgcr: bad arguments");
  MGS_CHECK(ctx, A->rows == A->cols && x->n >= A->rows && b->n >= A->rows, MGS_ERR_INVALID, "mgs_fgcr: square unsharded operator required");
  bool ns = false;
  MGS_TRY(mgs_krylov_nullspace(A, h, "mgs_fgcr", &ns));
  MGS_TRY(mgs_csr_optimize(const_cast<mgs_csr *>(A)));
  const int n = A->rows;
  constexpr int CH = 16;                             // vectors per multi-vector pass (blas1.hip: MDOT_MAX)
  krylov_frame f{ctx, h, n, ns, false, {}};
  mgs_vec *r = nullptr; MGS_TRY(f.take(&r, n));
  std::vector<mgs_vec *> C((size_t)restart, nullptr), V((size_t)restart, nullptr);
  std::vector<double> rho((size_t)restart, 0.0), alpha((size_t)restart, 0.0), U((size_t)restart * restart, 0.0), hj((size_t)restart, 0.0), y((size_t)restart, 0.0);
  mgs_vec xv = f.view(x), bv = f.view(b);
  double normb = 0, nr = 0;
  MGS_TRY(f.norm_b(bv, &normb));
  // r = b − A·x, ‖r‖/‖b‖.  Constant null space: r = Π(b − A·x), ‖r‖/‖Πb‖; with `last` (the call may decide a return: the recursion says
  // converged, the iterations are used up, a breakdown) x ← Πx first.  An ordinary restart leaves x as it is (A·Πx = A·x); should its true
  // residual end the solve all the same, fin() projects x behind it.
  bool x_mean = ns;                                 // x may carry a constant component (the guess's, or a window's rounding)
  auto true_residual = [&](double *resid_out, bool last) -> int {
    if (last && x_mean) { MGS_TRY(k_project_const(ctx, n, xv.d)); x_mean = false; }
    MGS_TRY(mgs_residual(A, &xv, &bv, r));
    if (ns) { double s2[2]; MGS_TRY(k_project_const_nrm2(ctx, n, r->d, s2)); nr = std::sqrt(s2[0]); }
    else MGS_TRY(mgs_nrm2(r, &nr));
    *resid_out = nr / normb;
    return MGS_OK;
  };
  // x ← x + Σ_{j<m} y_j c_j, (I + U) y = α over the m directions of the open window
  auto fin = [&]() -> int { if (x_mean) { MGS_TRY(k_project_const(ctx, n, xv.d)); x_mean = false; } return mgs_sync(ctx); };
  auto close_window = [&](int m) -> int {
    if (m <= 0) return MGS_OK;
    x_mean = ns;
    for (int k = m - 1; k >= 0; --k) { double s = alpha[k]; for (int q = k + 1; q < m; ++q) s -= U[(size_t)k * restart + q] * y[q]; y[k] = s; }
    for (int c0 = 0; c0 < m; c0 += CH) {
      const int K = std::min(CH, m - c0);
      const double *w[CH]; double cf[CH];
      for (int q = 0; q < K; ++q) { w[q] = C[c0 + q]->d; cf[q] = -y[c0 + q]; }
      MGS_TRY(k_maxpy_dot2(ctx, n, K, xv.d, w, cf, xv.d, nullptr, nullptr, nullptr));
    }
    return MGS_OK;
  };
  double resid = 0.0;
  MGS_TRY(true_residual(&resid, true));
  if (resid <= *tol) { *tol = resid; *max_iter = 0; *status = 0; return ns ? mgs_sync(ctx) : MGS_OK; }
  int it = 0;
  while (it < *max_iter) {
    int m = 0;                                       // directions in the open window
    bool restart_now = false;
    for (int k = 0; k < restart && it < *max_iter && !restart_now; ++k) {
      if (!C[k]) { MGS_TRY(f.take(&C[k], n)); MGS_TRY(f.take(&V[k], n)); }
      if (h) MGS_TRY(mgs_vcycle(h, r, C[k], 1)); else MGS_TRY(mgs_vec_copy(r, C[k]));
      if (ns) MGS_TRY(k_project_const(ctx, n, C[k]->d));      // c_k ← Πc_k before v_k = A·c_k
      MGS_TRY(mgs_spmv(A, C[k], V[k]));
      double d2[2];
      if (k == 0) {
        MGS_TRY(k_dot2(ctx, n, V[0]->d, V[0]->d, V[0]->d, r->d, d2));
      } else {
        for (int c0 = 0; c0 < k; c0 += CH) {           // every h_j against the SAME (not yet updated) v_k
          const int K = std::min(CH, k - c0);
          const double *w[CH];
          for (int q = 0; q < K; ++q) w[q] = V[c0 + q]->d;
          MGS_TRY(k_mdot(ctx, n, K, V[k]->d, w, nullptr, &hj[(size_t)c0]));
        }
        for (int j = 0; j < k; ++j) U[(size_t)j * restart + k] = rho[j] != 0.0 ? hj[j] / rho[j] : 0.0;
        for (int c0 = 0; c0 < k; c0 += CH) {
          const int K = std::min(CH, k - c0);
          const bool last = c0 + CH >= k;
          const double *w[CH]; double cf[CH];
          for (int q = 0; q < K; ++q) { w[q] = V[c0 + q]->d; cf[q] = U[(size_t)(c0 + q) * restart + k]; }
          MGS_TRY(k_maxpy_dot2(ctx, n, K, V[k]->d, w, cf, V[k]->d, last ? r->d : nullptr, nullptr, last ? d2 : nullptr));
        }
      }
      rho[k] = d2[0];
      ++it; m = k + 1;
      if (rho[k] == 0.0) {                             // A·c_k lies in the span of the window: nothing more to gain from it
        alpha[k] = 0.0;
        MGS_TRY(close_window(m));
        MGS_TRY(true_residual(&resid, true)); *status = resid < *tol ? 0 : 2; *tol = resid; *max_iter = it; return fin();
      }
      alpha[k] = d2[1] / rho[k];
      MGS_TRY(k_update_dot2(ctx, n, 1.0, r->d, -alpha[k], V[k]->d, r->d, nullptr, d2));   // r ← r − α v with ‖r‖²
      resid = std::sqrt(d2[0]) / normb;
      if (resid < *tol) {                         // the recursion says converged: the true residual decides
        MGS_TRY(close_window(m)); m = 0;
        MGS_TRY(true_residual(&resid, true));
        if (resid < *tol) { *tol = resid; *max_iter = it; *status = 0; return fin(); }
        restart_now = true;                       // not yet: restart from the true residual (r holds it)
      }
    }
    if (m) {                                      // window full (or out of iterations): x catches up, r ← b − A·x
      MGS_TRY(close_window(m));
      MGS_TRY(true_residual(&resid, it >= *max_iter));
      if (resid < *tol) { *tol = resid; *max_iter = it; *status = 0; return fin(); }
    }
  }
  *status = resid < *tol ? 0 : 1; *tol = resid; *max_iter = it;
  return fin();
}

}  // extern "C"
