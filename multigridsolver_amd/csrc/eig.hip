// eig.hip — mgs_eig_lobpcg: the m smallest eigenpairs of a symmetric operator by LOBPCG (Knyazev, SISC 23 (2001)) with the hierarchy's cycle as
// preconditioner.  The host drives; every pass over the vectors is mgs_spmv, mgs_vcycle, a null-space projection or one of the two block passes
// of blockvec.hip, and the dense problems of order at most 3m = 24 are solved on the host (eig_dense.hpp).  The one kernel here is the row sums
// of |a_ij| behind ‖A‖∞.  mgs_eig_lobpcg_gen is the same loop for A·x = λ·B·x in the B inner product; its residual pass, mgs_eig_residual, is a
// kernel of blas1.hip (it ends in k_dot's folds).  gfx950 only.
#include "mgs_internal.hpp"
#include "eig_dense.hpp"

namespace {
constexpr int TB = 256;
__global__ __launch_bounds__(TB) void abs_rowsum_kernel(int n, const int *__restrict__ rowptr, const double *__restrict__ val, double *__restrict__ out) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) s += fabs(val[k]);
  out[i] = s;
}
// ‖A‖∞ = max_i Σ_j |a_ij|: the row sums into `tmp` (n entries), their maximum folded on the device (k_absmax_dev) and read once
int norm_inf(const mgs_csr *A, double *tmp, double *out) {
  mgs_ctx *ctx = A->ctx;
  unsigned long long *mx = reinterpret_cast<unsigned long long *>(ctx->red_dev + MGS_ABSMAX_SLOT), bits = 0;
  MGS_HIP(ctx, hipMemsetAsync(mx, 0, sizeof bits, ctx->stream));
  hipLaunchKernelGGL(abs_rowsum_kernel, dim3(mgs_grid(A->rows, TB)), dim3(TB), 0, ctx->stream, A->rows, A->rowptr, A->val, tmp);
  MGS_HIP(ctx, hipGetLastError());
  MGS_TRY(k_absmax_dev(ctx, A->rows, tmp, mx));
  MGS_HIP(ctx, hipMemcpyAsync(&bits, mx, sizeof bits, hipMemcpyDeviceToHost, ctx->stream));
  MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(out, &bits, sizeof bits);
  return MGS_OK;
}
}   // namespace

extern "C" {

// Work vectors, from the context's pool: the staging pair (residual, result) of the cycle, then A·X, W, A·W, P, A·P with m columns each: 5m + 2.
int mgs_eig_lobpcg(const mgs_csr *A, mgs_hier *h, int m, mgs_vec *const *X, double *theta, double *resid, int *max_iter, double *tol, int *status) {
  MGS_CHECK(nullptr, A, MGS_ERR_INVALID, "mgs_eig_lobpcg: NULL matrix");
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, X && theta && resid && max_iter && tol && status, MGS_ERR_INVALID, "mgs_eig_lobpcg: NULL argument");
  MGS_CHECK(ctx, m >= 1 && m <= MGS_EIG_MAX_BLOCK, MGS_ERR_INVALID, "mgs_eig_lobpcg: block of %d columns (1..%d)", m, MGS_EIG_MAX_BLOCK);
  MGS_TRY(mgs_check_unsharded(A, h, "mgs_eig_lobpcg", "row shards are not served"));
  if (h) {
    MGS_CHECK(ctx, h->nu1 == h->nu2 && h->kcycle_levels <= 0 && !h->kcycle_entry, MGS_ERR_INVALID,
              "mgs_eig_lobpcg: the preconditioner must be a fixed symmetric operator (nu1 == nu2, no K-cycle)");
  }
  bool ns = false;
  MGS_TRY(mgs_krylov_nullspace(A, h, "mgs_eig_lobpcg", &ns, true));
  const int n = A->rows;
  const int nnull = A->nullspace == MGS_NULLSPACE_FIELDS ? A->nsf->nfields : (A->nullspace == MGS_NULLSPACE_CONSTANT ? 1 : 0);
  MGS_CHECK(ctx, n >= 3 * m + nnull, MGS_ERR_INVALID, "mgs_eig_lobpcg: %d rows, a block of %d with %d declared null vectors needs %d", n, m, nnull, 3 * m + nnull);
  for (int j = 0; j < m; ++j) {
    MGS_CHECK(ctx, X[j] && X[j]->d && X[j]->ctx == ctx, MGS_ERR_INVALID, "mgs_eig_lobpcg: X[%d] is NULL or of another context", j);
    MGS_CHECK(ctx, X[j]->n >= n, MGS_ERR_INVALID, "mgs_eig_lobpcg: X[%d] holds %lld entries, A has %d rows", j, (long long)X[j]->n, n);
    for (int i = 0; i < j; ++i)
      MGS_CHECK(ctx, !(X[i]->d < X[j]->d + n && X[j]->d < X[i]->d + n), MGS_ERR_INVALID, "mgs_eig_lobpcg: X[%d] and X[%d] %s", i, j, X[i]->d == X[j]->d ? "are the same vector" : "overlap");
  }
  MGS_TRY(mgs_csr_optimize(const_cast<mgs_csr *>(A)));
  int64_t *info = ctx->eig_info;
  for (int q = 0; q < 8; ++q) info[q] = 0;
  const int64_t captures0 = ctx->graph_captures;

  krylov_frame f{ctx, h, n, ns, true, {}, A};      // returned last-taken-first: the next call finds the staging pair at the same addresses (one cached cycle graph)
  mgs_vec *rs = nullptr, *ws = nullptr;
  MGS_TRY(f.take(&rs, n)); MGS_TRY(f.take(&ws, n));
  mgs_vec *AX[MGS_EIG_MAX_BLOCK], *W[MGS_EIG_MAX_BLOCK], *AW[MGS_EIG_MAX_BLOCK], *P[MGS_EIG_MAX_BLOCK], *AP[MGS_EIG_MAX_BLOCK];
  for (auto *blk : {AX, W, AW, P, AP}) for (int j = 0; j < m; ++j) MGS_TRY(f.take(&blk[j], n));
  info[5] = (int64_t)f.taken.size();
  auto finish = [&](int st, int it) -> int {
    double worst = 0.0;
    for (int j = 0; j < m; ++j) if (!(resid[j] <= worst)) worst = resid[j];
    *status = st; *max_iter = it; *tol = worst;
    info[0] = it; info[6] = ctx->graph_captures - captures0;
    return mgs_sync(ctx);
  };
  using eig_dense::cholesky; using eig_dense::inverse_t;
  double G[MGS_VECS_MAX * MGS_VECS_MAX], GA[MGS_VECS_MAX * MGS_VECS_MAX], L[MGS_VECS_MAX * MGS_VECS_MAX], C[MGS_VECS_MAX * MGS_VECS_MAX], Z[MGS_VECS_MAX * MGS_VECS_MAX], ev[MGS_VECS_MAX];
  // Cholesky QR of W or P in place, B ← B·C, and the same factor on a second block (A·B).  The columns differ in length by orders of magnitude (they are
  // residuals), so the pivot rule is applied to the Gram matrix of the normalised columns (eig_dense::qr_factor); false through *ok when it refuses
  auto chol_qr = [&](int q, mgs_vec *const *B, mgs_vec *const *AB, bool *ok) -> int {
    MGS_TRY(mgs_vecs_gram(ctx, n, q, B, q, B, G));
    *ok = eig_dense::qr_factor(q, G, m, L, C);
    if (!*ok) return MGS_OK;
    MGS_TRY(mgs_vecs_combine(ctx, n, q, B, q, B, C));
    if (AB) MGS_TRY(mgs_vecs_combine(ctx, n, q, AB, q, AB, C));
    return MGS_OK;
  };
  auto apply_A = [&](int q, mgs_vec *const *B, mgs_vec *const *AB) -> int {
    for (int j = 0; j < q; ++j) { MGS_TRY(mgs_spmv(A, B[j], AB[j])); ++info[2]; }
    return MGS_OK;
  };

  // ---- start: X ← ΠX, Cholesky QR, Rayleigh–Ritz on X
  double anorm = 0.0;
  MGS_TRY(norm_inf(A, rs->d, &anorm));
  if (!(anorm > 0.0)) anorm = 1.0;
  for (int j = 0; j < m; ++j) { theta[j] = 0.0; resid[j] = 0.0; }
  // The start block: with a declared null space ΠX is formed in W, so that X is still the caller's when the pivot rule of XᵀX refuses (status 2); the
  // rule is applied to XᵀX as it stands, the factor goes from the source block into X.
  mgs_vec *const *X0 = X;
  if (ns) {
    for (int j = 0; j < m; ++j) {
      MGS_HIP(ctx, hipMemcpyAsync(W[j]->d, X[j]->d, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
      MGS_TRY(k_ns_project(A, n, W[j]->d));
    }
    X0 = W;
  }
  MGS_TRY(mgs_vecs_gram(ctx, n, m, X0, m, X0, G));
  if (!cholesky(m, G, m, L)) return finish(2, 0);
  inverse_t(m, L, C);
  MGS_TRY(mgs_vecs_combine(ctx, n, m, X0, m, X, C));
  bool ok = false;
  MGS_TRY(apply_A(m, X, AX));
  MGS_TRY(mgs_vecs_gram(ctx, n, m, X, m, AX, GA));
  for (int a = 0; a < m; ++a) for (int b = 0; b < m; ++b) G[a * m + b] = 0.5 * (GA[a * m + b] + GA[b * m + a]);
  if (eig_dense::jacobi(m, G, theta, Z) < 0) return finish(3, 0);
  MGS_TRY(mgs_vecs_combine(ctx, n, m, X, m, X, Z));
  MGS_TRY(mgs_vecs_combine(ctx, n, m, AX, m, AX, Z));

  // column j's residual A·x_j − θ_j·x_j into the staging vector and its norm over ‖A‖∞
  auto residual = [&](int j, double *r) -> int {
    const mgs_vec *S2[2] = {X[j], AX[j]};
    const double c2[2] = {-theta[j], 1.0};
    double s = 0.0;
    MGS_TRY(mgs_vecs_combine(ctx, n, 2, S2, 1, &rs, c2));
    MGS_TRY(k_dot(ctx, n, rs->d, rs->d, &s));
    *r = std::sqrt(s) / anorm;
    return MGS_OK;
  };
  const double bar = *tol;
  const int maxit = *max_iter;
  bool hasP = false, fresh = true;      // fresh: A·X came from SpMVs on the X that stands, not from the recurrence
  int it = 0;
  for (;;) {
    // residuals; an active column (at or above the bar) goes through the preconditioner from the staging pair and is orthogonalised against X
    int act[MGS_EIG_MAX_BLOCK], na = 0;
    bool bad = false;
    for (int j = 0; j < m; ++j) {
      MGS_TRY(residual(j, &resid[j]));
      if (!std::isfinite(resid[j])) bad = true;
      if (resid[j] < bar || bad || it >= maxit) continue;
      mgs_vec *z = rs;
      if (h) { MGS_TRY(mgs_vcycle(h, rs, ws, 1)); ++info[1]; z = ws; }
      if (ns) MGS_TRY(k_ns_project(A, n, z->d));
      const mgs_vec *zc = z;
      MGS_TRY(mgs_vecs_gram(ctx, n, m, X, 1, &zc, G));
      const mgs_vec *S[MGS_EIG_MAX_BLOCK + 1]; double c[MGS_EIG_MAX_BLOCK + 1];
      S[0] = z; c[0] = 1.0;
      for (int a = 0; a < m; ++a) { S[a + 1] = X[a]; c[a + 1] = -G[a]; }
      MGS_TRY(mgs_vecs_combine(ctx, n, m + 1, S, 1, &W[na], c));
      act[na++] = j;
    }
    if (bad) return finish(3, it);
    if (na == 0) {      // every column below the bar by the recurrence, or out of iterations: the true residuals decide
      if (!fresh) { MGS_TRY(apply_A(m, X, AX)); fresh = true; if (it < maxit) continue; for (int j = 0; j < m; ++j) MGS_TRY(residual(j, &resid[j])); }
      bool all = true;
      for (int j = 0; j < m; ++j) { if (!std::isfinite(resid[j])) return finish(3, it); all = all && resid[j] < bar; }
      info[4] = 0; for (int j = 0; j < m; ++j) info[4] += resid[j] < bar;
      return finish(all ? 0 : 1, it);
    }
    MGS_TRY(chol_qr(na, W, nullptr, &ok));
    if (!ok) return finish(3, it);
    MGS_TRY(apply_A(na, W, AW));
    mgs_vec *Pa[MGS_EIG_MAX_BLOCK], *APa[MGS_EIG_MAX_BLOCK];
    for (int q = 0; q < na; ++q) { Pa[q] = P[act[q]]; APa[q] = AP[act[q]]; }
    bool useP = hasP;
    if (useP) { MGS_TRY(chol_qr(na, Pa, APa, &ok)); if (!ok) { useP = false; ++info[3]; } }
    for (;;) {      // Rayleigh–Ritz on S = [X W P]; when SᵀS fails the pivot rule the iteration is redone on [X W]
      const int k = m + na + (useP ? na : 0);
      const mgs_vec *S[MGS_VECS_MAX], *AS[MGS_VECS_MAX];
      for (int a = 0; a < m; ++a) { S[a] = X[a]; AS[a] = AX[a]; }
      for (int a = 0; a < na; ++a) { S[m + a] = W[a]; AS[m + a] = AW[a]; if (useP) { S[m + na + a] = Pa[a]; AS[m + na + a] = APa[a]; } }
      MGS_TRY(mgs_vecs_gram(ctx, n, k, S, k, AS, GA));
      MGS_TRY(mgs_vecs_gram(ctx, n, k, S, k, S, G));
      const int sw = eig_dense::generalized(k, GA, G, m, ev, Z);
      if (sw < 0) return finish(3, it);
      if (sw == 0) { if (!useP) return finish(3, it); useP = false; ++info[3]; continue; }
      // one coefficient matrix for both combines: columns [0, m) the new X (and A·X), [m, 2m) the new P (and A·P) = the W and P parts alone
      for (int a = 0; a < k; ++a)
        for (int j = 0; j < m; ++j) { C[a * 2 * m + j] = Z[a * k + j]; C[a * 2 * m + m + j] = a < m ? 0.0 : Z[a * k + j]; }
      mgs_vec *Y[2 * MGS_EIG_MAX_BLOCK], *AY[2 * MGS_EIG_MAX_BLOCK];
      for (int j = 0; j < m; ++j) { Y[j] = X[j]; Y[m + j] = P[j]; AY[j] = AX[j]; AY[m + j] = AP[j]; }
      MGS_TRY(mgs_vecs_combine(ctx, n, k, S, 2 * m, Y, C));
      MGS_TRY(mgs_vecs_combine(ctx, n, k, AS, 2 * m, AY, C));
      for (int j = 0; j < m; ++j) theta[j] = ev[j];
      break;
    }
    hasP = true; fresh = false; ++it;
  }
}

// r = ax − θ·bx and ‖r‖² in one pass (the kernel and its launch decisions: k_eig_residual, blas1.hip)
int mgs_eig_residual(mgs_ctx *ctx, int64_t n, const mgs_vec *ax, const mgs_vec *bx, double theta, mgs_vec *r, double *nrm2) {
  MGS_CHECK(nullptr, ctx, MGS_ERR_INVALID, "mgs_eig_residual: NULL context");
  MGS_CHECK(ctx, ax && bx && r && ax->d && bx->d && r->d, MGS_ERR_INVALID, "mgs_eig_residual: NULL vector");
  MGS_CHECK(ctx, ax->ctx == ctx && bx->ctx == ctx && r->ctx == ctx, MGS_ERR_INVALID, "mgs_eig_residual: a vector belongs to another context");
  MGS_CHECK(ctx, n >= 1 && ax->n >= n && bx->n >= n && r->n >= n, MGS_ERR_INVALID, "mgs_eig_residual: n = %lld, ax, bx, r hold %lld, %lld, %lld entries", (long long)n,
            (long long)ax->n, (long long)bx->n, (long long)r->n);
  for (const mgs_vec *s : {ax, bx})
    MGS_CHECK(ctx, r->d == s->d || !(r->d < s->d + n && s->d < r->d + n), MGS_ERR_INVALID, "mgs_eig_residual: r overlaps %s without being that vector", s == ax ? "ax" : "bx");
  return k_eig_residual(ctx, n, ax->d, bx->d, theta, r->d, nrm2);
}

// The generalised problem A·x = λ·B·x: mgs_eig_lobpcg's loop with B·X, B·W and B·P carried beside the A-blocks, every Gram matrix that was
// VᵀV taken as Vᵀ(B·V), and the residual A·x_j − θ_j·B·x_j from the fused pass.  Work vectors: the staging pair, then A·X, B·X, W, A·W, B·W, P, A·P,
// B·P with m columns each: 8m + 2.
int mgs_eig_lobpcg_gen(const mgs_csr *A, const mgs_csr *B, mgs_hier *h, int m, mgs_vec *const *X, double *theta, double *resid, int *max_iter, double *tol, int *status) {
  if (!B) return mgs_eig_lobpcg(A, h, m, X, theta, resid, max_iter, tol, status);
  static const char who[] = "mgs_eig_lobpcg_gen";
  MGS_CHECK(nullptr, A, MGS_ERR_INVALID, "%s: NULL matrix", who);
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, X && theta && resid && max_iter && tol && status, MGS_ERR_INVALID, "%s: NULL argument", who);
  MGS_CHECK(ctx, m >= 1 && m <= MGS_EIG_MAX_BLOCK, MGS_ERR_INVALID, "%s: block of %d columns (1..%d)", who, m, MGS_EIG_MAX_BLOCK);
  MGS_TRY(mgs_check_unsharded(A, h, who, "row shards are not served"));
  MGS_CHECK(ctx, B->ctx == ctx, MGS_ERR_INVALID, "%s: B belongs to another context than A", who);
  MGS_CHECK(ctx, B->rows == B->cols && B->rows == A->rows, MGS_ERR_INVALID, "%s: B is %d x %d%s, A is %d x %d", who, B->rows, B->cols,
            B->cols > B->rows ? " (halo columns: a row shard)" : "", A->rows, A->cols);
  MGS_CHECK(ctx, A->nullspace == MGS_NULLSPACE_NONE && B->nullspace == MGS_NULLSPACE_NONE, MGS_ERR_INVALID,
            "%s: a null space is declared on %s; its complement would have to be B-orthogonal, which is not served (mgs_eig_lobpcg serves B = I)", who,
            A->nullspace != MGS_NULLSPACE_NONE ? "A" : "B");
  if (h) {
    MGS_CHECK(ctx, h->nu1 == h->nu2 && h->kcycle_levels <= 0 && !h->kcycle_entry, MGS_ERR_INVALID,
              "%s: the preconditioner must be a fixed symmetric operator (nu1 == nu2, no K-cycle)", who);
  }
  bool ns = false;
  MGS_TRY(mgs_krylov_nullspace(A, h, who, &ns, true));      // (a hierarchy built for a null-space twin of A is refused here)
  const int n = A->rows;
  MGS_CHECK(ctx, n >= 3 * m, MGS_ERR_INVALID, "%s: %d rows, a block of %d needs %d", who, n, m, 3 * m);
  for (int j = 0; j < m; ++j) {
    MGS_CHECK(ctx, X[j] && X[j]->d && X[j]->ctx == ctx, MGS_ERR_INVALID, "%s: X[%d] is NULL or of another context", who, j);
    MGS_CHECK(ctx, X[j]->n >= n, MGS_ERR_INVALID, "%s: X[%d] holds %lld entries, A has %d rows", who, j, (long long)X[j]->n, n);
    for (int i = 0; i < j; ++i)
      MGS_CHECK(ctx, !(X[i]->d < X[j]->d + n && X[j]->d < X[i]->d + n), MGS_ERR_INVALID, "%s: X[%d] and X[%d] %s", who, i, j, X[i]->d == X[j]->d ? "are the same vector" : "overlap");
  }
  MGS_TRY(mgs_csr_optimize(const_cast<mgs_csr *>(A)));
  MGS_TRY(mgs_csr_optimize(const_cast<mgs_csr *>(B)));
  int64_t *info = ctx->eig_info;
  for (int q = 0; q < 8; ++q) info[q] = 0;
  const int64_t captures0 = ctx->graph_captures;

  krylov_frame f{ctx, h, n, false, true, {}, A};      // last-taken-first, as mgs_eig_lobpcg: the staging pair keeps its addresses (one cached cycle graph)
  mgs_vec *rs = nullptr, *ws = nullptr;
  MGS_TRY(f.take(&rs, n)); MGS_TRY(f.take(&ws, n));
  mgs_vec *AX[MGS_EIG_MAX_BLOCK], *BX[MGS_EIG_MAX_BLOCK], *W[MGS_EIG_MAX_BLOCK], *AW[MGS_EIG_MAX_BLOCK], *BW[MGS_EIG_MAX_BLOCK], *P[MGS_EIG_MAX_BLOCK], *AP[MGS_EIG_MAX_BLOCK],
      *BP[MGS_EIG_MAX_BLOCK];
  for (auto *blk : {AX, BX, W, AW, BW, P, AP, BP}) for (int j = 0; j < m; ++j) MGS_TRY(f.take(&blk[j], n));
  info[5] = (int64_t)f.taken.size();
  auto finish = [&](int st, int it) -> int {
    double worst = 0.0;
    for (int j = 0; j < m; ++j) if (!(resid[j] <= worst)) worst = resid[j];
    *status = st; *max_iter = it; *tol = worst;
    info[0] = it; info[6] = ctx->graph_captures - captures0;
    return mgs_sync(ctx);
  };
  using eig_dense::cholesky; using eig_dense::inverse_t;
  double G[MGS_VECS_MAX * MGS_VECS_MAX], GA[MGS_VECS_MAX * MGS_VECS_MAX], L[MGS_VECS_MAX * MGS_VECS_MAX], C[MGS_VECS_MAX * MGS_VECS_MAX], Z[MGS_VECS_MAX * MGS_VECS_MAX], ev[MGS_VECS_MAX];
  // G ← ½(Vᵀ(B·V) + (Vᵀ(B·V))ᵀ): B is symmetric, the two lists are not the same, so the pass does not return a symmetric matrix by itself
  auto gram_b = [&](int q, const mgs_vec *const *V, const mgs_vec *const *BV) -> int {
    MGS_TRY(mgs_vecs_gram(ctx, n, q, V, q, BV, GA));
    for (int a = 0; a < q; ++a) for (int b = 0; b < q; ++b) G[a * q + b] = 0.5 * (GA[a * q + b] + GA[b * q + a]);
    return MGS_OK;
  };
  // Cholesky QR of W or P in the B inner product, V ← V·C with the pivot rule on the normalised columns of Vᵀ(B·V); the same factor on B·V and A·V
  auto chol_qr = [&](int q, mgs_vec *const *V, mgs_vec *const *BV, mgs_vec *const *AV, bool *ok) -> int {
    MGS_TRY(gram_b(q, V, BV));
    *ok = eig_dense::qr_factor(q, G, m, L, C);
    if (!*ok) return MGS_OK;
    MGS_TRY(mgs_vecs_combine(ctx, n, q, V, q, V, C));
    MGS_TRY(mgs_vecs_combine(ctx, n, q, BV, q, BV, C));
    if (AV) MGS_TRY(mgs_vecs_combine(ctx, n, q, AV, q, AV, C));
    return MGS_OK;
  };
  auto apply_A = [&](int q, mgs_vec *const *V, mgs_vec *const *AV) -> int {
    for (int j = 0; j < q; ++j) { MGS_TRY(mgs_spmv(A, V[j], AV[j])); ++info[2]; }
    return MGS_OK;
  };
  auto apply_B = [&](int q, mgs_vec *const *V, mgs_vec *const *BV) -> int {
    for (int j = 0; j < q; ++j) { MGS_TRY(mgs_spmv(B, V[j], BV[j])); ++info[2]; ++info[7]; }
    return MGS_OK;
  };

  // ---- start: Cholesky QR of X in the B inner product (B·X formed in B·W's vectors, so that X is the caller's when the rule refuses), Rayleigh–Ritz on X
  double anorm = 0.0, bnorm = 0.0;
  MGS_TRY(norm_inf(A, rs->d, &anorm));
  MGS_TRY(norm_inf(B, rs->d, &bnorm));
  if (!(anorm > 0.0)) anorm = 1.0;
  if (!(bnorm > 0.0)) bnorm = 1.0;
  for (int j = 0; j < m; ++j) { theta[j] = 0.0; resid[j] = 0.0; }
  MGS_TRY(apply_B(m, X, BW));
  MGS_TRY(gram_b(m, X, BW));
  if (!cholesky(m, G, m, L)) return finish(2, 0);
  inverse_t(m, L, C);
  MGS_TRY(mgs_vecs_combine(ctx, n, m, X, m, X, C));
  MGS_TRY(mgs_vecs_combine(ctx, n, m, BW, m, BX, C));
  bool ok = false;
  MGS_TRY(apply_A(m, X, AX));
  MGS_TRY(mgs_vecs_gram(ctx, n, m, X, m, AX, GA));
  for (int a = 0; a < m; ++a) for (int b = 0; b < m; ++b) G[a * m + b] = 0.5 * (GA[a * m + b] + GA[b * m + a]);
  if (eig_dense::jacobi(m, G, theta, Z) < 0) return finish(3, 0);
  for (auto *blk : {(mgs_vec *const *)X, (mgs_vec *const *)AX, (mgs_vec *const *)BX}) MGS_TRY(mgs_vecs_combine(ctx, n, m, blk, m, blk, Z));

  // column j's residual A·x_j − θ_j·B·x_j into the staging vector and its norm over ‖A‖∞ + |θ_j|·‖B‖∞
  auto residual = [&](int j, double *r) -> int {
    double s = 0.0;
    MGS_TRY(k_eig_residual(ctx, n, AX[j]->d, BX[j]->d, theta[j], rs->d, &s));
    *r = std::sqrt(s) / (anorm + std::fabs(theta[j]) * bnorm);
    return MGS_OK;
  };
  const double bar = *tol;
  const int maxit = *max_iter;
  bool hasP = false, fresh = true;      // fresh: A·X and B·X came from SpMVs on the X that stands, not from the recurrence
  int it = 0;
  for (;;) {
    // residuals; an active column goes through the preconditioner from the staging pair and is B-orthogonalised against X: W ← W − X·((B·X)ᵀW)
    int act[MGS_EIG_MAX_BLOCK], na = 0;
    bool bad = false;
    for (int j = 0; j < m; ++j) {
      MGS_TRY(residual(j, &resid[j]));
      if (!std::isfinite(resid[j])) bad = true;
      if (resid[j] < bar || bad || it >= maxit) continue;
      mgs_vec *z = rs;
      if (h) { MGS_TRY(mgs_vcycle(h, rs, ws, 1)); ++info[1]; z = ws; }
      const mgs_vec *zc = z;
      MGS_TRY(mgs_vecs_gram(ctx, n, m, BX, 1, &zc, G));
      const mgs_vec *S[MGS_EIG_MAX_BLOCK + 1]; double c[MGS_EIG_MAX_BLOCK + 1];
      S[0] = z; c[0] = 1.0;
      for (int a = 0; a < m; ++a) { S[a + 1] = X[a]; c[a + 1] = -G[a]; }
      MGS_TRY(mgs_vecs_combine(ctx, n, m + 1, S, 1, &W[na], c));
      act[na++] = j;
    }
    if (bad) return finish(3, it);
    if (na == 0) {      // every column below the bar by the recurrences, or out of iterations: the true residuals decide
      if (!fresh) {
        MGS_TRY(apply_A(m, X, AX)); MGS_TRY(apply_B(m, X, BX)); fresh = true;
        if (it < maxit) continue;
        for (int j = 0; j < m; ++j) MGS_TRY(residual(j, &resid[j]));
      }
      bool all = true;
      for (int j = 0; j < m; ++j) { if (!std::isfinite(resid[j])) return finish(3, it); all = all && resid[j] < bar; }
      info[4] = 0; for (int j = 0; j < m; ++j) info[4] += resid[j] < bar;
      return finish(all ? 0 : 1, it);
    }
    MGS_TRY(apply_B(na, W, BW));
    MGS_TRY(chol_qr(na, W, BW, nullptr, &ok));
    if (!ok) return finish(3, it);
    MGS_TRY(apply_A(na, W, AW));
    mgs_vec *Pa[MGS_EIG_MAX_BLOCK], *APa[MGS_EIG_MAX_BLOCK], *BPa[MGS_EIG_MAX_BLOCK];
    for (int q = 0; q < na; ++q) { Pa[q] = P[act[q]]; APa[q] = AP[act[q]]; BPa[q] = BP[act[q]]; }
    bool useP = hasP;
    if (useP) { MGS_TRY(chol_qr(na, Pa, BPa, APa, &ok)); if (!ok) { useP = false; ++info[3]; } }
    for (;;) {      // Rayleigh–Ritz on S = [X W P] with GA = SᵀAS and GB = ½(Sᵀ(BS) + its transpose); when GB fails the pivot rule the iteration is redone on [X W]
      const int k = m + na + (useP ? na : 0);
      const mgs_vec *S[MGS_VECS_MAX], *AS[MGS_VECS_MAX], *BS[MGS_VECS_MAX];
      for (int a = 0; a < m; ++a) { S[a] = X[a]; AS[a] = AX[a]; BS[a] = BX[a]; }
      for (int a = 0; a < na; ++a) {
        S[m + a] = W[a]; AS[m + a] = AW[a]; BS[m + a] = BW[a];
        if (useP) { S[m + na + a] = Pa[a]; AS[m + na + a] = APa[a]; BS[m + na + a] = BPa[a]; }
      }
      MGS_TRY(gram_b(k, S, BS));                                 // G ← GB (through GA, which the next call overwrites)
      MGS_TRY(mgs_vecs_gram(ctx, n, k, S, k, AS, GA));
      const int sw = eig_dense::generalized(k, GA, G, m, ev, Z);
      if (sw < 0) return finish(3, it);
      if (sw == 0) { if (!useP) return finish(3, it); useP = false; ++info[3]; continue; }
      // one coefficient matrix for the three combines: columns [0, m) the new X (A·X, B·X), [m, 2m) the new P (A·P, B·P) = the W and P parts alone
      for (int a = 0; a < k; ++a)
        for (int j = 0; j < m; ++j) { C[a * 2 * m + j] = Z[a * k + j]; C[a * 2 * m + m + j] = a < m ? 0.0 : Z[a * k + j]; }
      mgs_vec *Y[2 * MGS_EIG_MAX_BLOCK], *AY[2 * MGS_EIG_MAX_BLOCK], *BY[2 * MGS_EIG_MAX_BLOCK];
      for (int j = 0; j < m; ++j) { Y[j] = X[j]; Y[m + j] = P[j]; AY[j] = AX[j]; AY[m + j] = AP[j]; BY[j] = BX[j]; BY[m + j] = BP[j]; }
      MGS_TRY(mgs_vecs_combine(ctx, n, k, S, 2 * m, Y, C));
      MGS_TRY(mgs_vecs_combine(ctx, n, k, AS, 2 * m, AY, C));
      MGS_TRY(mgs_vecs_combine(ctx, n, k, BS, 2 * m, BY, C));
      for (int j = 0; j < m; ++j) theta[j] = ev[j];
      break;
    }
    hasP = true; fresh = false; ++it;
  }
}

int mgs_eig_info(const mgs_ctx *ctx, int64_t out[8]) {
  MGS_CHECK(nullptr, ctx && out, MGS_ERR_INVALID, "mgs_eig_info: NULL argument");
  memcpy(out, ctx->eig_info, sizeof ctx->eig_info);
  return MGS_OK;
}

}   // extern "C"
