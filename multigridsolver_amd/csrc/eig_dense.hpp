// eig_dense.hpp — the host dense algebra of mgs_eig_lobpcg (eig.hip): Cholesky with the dense coarse solve's pivot rule, triangular solves, a cyclic
// Jacobi eigensolver and the generalised symmetric problem of order at most 24 built from them.  Plain C++, no HIP header and no LAPACK: a
// stand-alone CPU program compiles it (tests/test_eig_dense_cpu.py).  Matrices are row-major with leading dimension n.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <vector>

namespace eig_dense {

// G = L·Lᵀ, L lower triangular (its upper part is zeroed).  The pivot rule: a pivot that is not greater than 8·m·DBL_EPSILON·max_i G_ii refuses the
// matrix (a NaN anywhere on the way refuses it too, every comparison is written so that a NaN fails it).  → true when L is complete.
inline bool cholesky(int n, const double *G, int m_rule, double *L) {
  double dmax = 0.0;
  for (int i = 0; i < n; ++i) { const double d = G[(size_t)i * n + i]; if (!(d <= dmax)) dmax = d; }
  const double bar = 8.0 * (double)m_rule * DBL_EPSILON * dmax;
  if (!(dmax > 0.0) || !std::isfinite(dmax)) return false;
  for (int i = 0; i < n * n; ++i) L[i] = 0.0;
  for (int j = 0; j < n; ++j) {
    double d = G[(size_t)j * n + j];
    for (int k = 0; k < j; ++k) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
    if (!(d > bar) || !std::isfinite(d)) return false;
    const double l = std::sqrt(d);
    L[(size_t)j * n + j] = l;
    for (int i = j + 1; i < n; ++i) {
      double s = G[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) s -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
      s /= l;
      if (!std::isfinite(s)) return false;
      L[(size_t)i * n + j] = s;
    }
  }
  return true;
}
// B ← L⁻¹·B (n × q, row-major, leading dimension q)
inline void solve_lower(int n, const double *L, int q, double *B) {
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < q; ++c) {
      double s = B[(size_t)i * q + c];
      for (int k = 0; k < i; ++k) s -= L[(size_t)i * n + k] * B[(size_t)k * q + c];
      B[(size_t)i * q + c] = s / L[(size_t)i * n + i];
    }
}
// B ← L⁻ᵀ·B
inline void solve_lower_t(int n, const double *L, int q, double *B) {
  for (int i = n - 1; i >= 0; --i)
    for (int c = 0; c < q; ++c) {
      double s = B[(size_t)i * q + c];
      for (int k = i + 1; k < n; ++k) s -= L[(size_t)k * n + i] * B[(size_t)k * q + c];
      B[(size_t)i * q + c] = s / L[(size_t)i * n + i];
    }
}
// Rinv = L⁻ᵀ (upper triangular): the matrix a Cholesky QR multiplies its block with, X ← X·L⁻ᵀ
inline void inverse_t(int n, const double *L, double *Rinv) {
  for (int i = 0; i < n * n; ++i) Rinv[i] = 0.0;
  for (int i = 0; i < n; ++i) Rinv[(size_t)i * n + i] = 1.0;
  solve_lower_t(n, L, n, Rinv);
}

// The factor of a Cholesky QR on columns of any scale: with d_j = 1/√G_jj the pivot rule is applied to the Gram matrix of the NORMALISED columns,
// D·G·D = L·Lᵀ (unit diagonal, so the rule measures linear dependence, not a difference in length), and C = D·L⁻ᵀ, so that B·C is orthonormal.
// → false when a diagonal entry is not positive and finite or the rule refuses.  (L: n·n scratch.)
inline bool qr_factor(int n, const double *G, int m_rule, double *L, double *C) {
  std::vector<double> d((size_t)n), Gs((size_t)n * n);
  for (int i = 0; i < n; ++i) {
    const double g = G[(size_t)i * n + i];
    if (!(g > 0.0) || !std::isfinite(g)) return false;
    d[(size_t)i] = 1.0 / std::sqrt(g);
  }
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) Gs[(size_t)i * n + j] = d[(size_t)i] * G[(size_t)i * n + j] * d[(size_t)j];
  if (!cholesky(n, Gs.data(), m_rule, L)) return false;
  inverse_t(n, L, C);
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) C[(size_t)i * n + j] *= d[(size_t)i];
  return true;
}

// Cyclic Jacobi on the symmetric A (only its upper triangle is trusted; A is destroyed): eigenvalues ascending in w, eigenvectors in the columns
// of V (row-major).  Sweeps run until a whole sweep made no rotation, at most 60.  An off-diagonal entry is set to zero without a rotation when it is
// below ε/8 of the geometric mean of its two diagonal entries or below ε²·‖A‖_F (the second bar keeps a zero diagonal entry from asking for an exact zero).
// → the sweeps done (the last one made no rotation); −1 for a NaN / Inf entry; −2 when the 60th sweep still rotated.
inline int jacobi(int n, double *A, double *w, double *V) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      if (!std::isfinite(A[(size_t)i * n + j])) return -1;
      V[(size_t)i * n + j] = i == j ? 1.0 : 0.0;
      if (j < i) A[(size_t)i * n + j] = A[(size_t)j * n + i];
    }
  double fro = 0.0;
  for (int i = 0; i < n * n; ++i) fro += A[i] * A[i];
  const double floor_abs = DBL_EPSILON * DBL_EPSILON * std::sqrt(fro);
  int sweeps = 0;
  bool rotated = true;
  for (; sweeps < 60 && rotated; ++sweeps) {
    rotated = false;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[(size_t)p * n + q];
        if (apq == 0.0) continue;
        const double app = A[(size_t)p * n + p], aqq = A[(size_t)q * n + q];
        if (std::fabs(apq) <= 0.125 * DBL_EPSILON * std::sqrt(std::fabs(app) * std::fabs(aqq)) || std::fabs(apq) <= floor_abs) { A[(size_t)p * n + q] = A[(size_t)q * n + p] = 0.0; continue; }
        const double tau = (aqq - app) / (2.0 * apq);
        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
        rotated = true;
        for (int k = 0; k < n; ++k) {
          const double akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
          A[(size_t)k * n + p] = c * akp - s * akq; A[(size_t)k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {
          const double apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
          A[(size_t)p * n + k] = c * apk - s * aqk; A[(size_t)q * n + k] = s * apk + c * aqk;
        }
        A[(size_t)p * n + q] = A[(size_t)q * n + p] = 0.0;
        for (int k = 0; k < n; ++k) {
          const double vkp = V[(size_t)k * n + p], vkq = V[(size_t)k * n + q];
          V[(size_t)k * n + p] = c * vkp - s * vkq; V[(size_t)k * n + q] = s * vkp + c * vkq;
        }
      }
  }
  if (rotated) return -2;
  for (int i = 0; i < n; ++i) w[i] = A[(size_t)i * n + i];
  for (int i = 0; i < n - 1; ++i) {      // ascending, columns of V along (selection sort: n <= 24)
    int lo = i;
    for (int j = i + 1; j < n; ++j) if (w[j] < w[lo]) lo = j;
    if (lo != i) {
      const double t = w[i]; w[i] = w[lo]; w[lo] = t;
      for (int k = 0; k < n; ++k) { const double v = V[(size_t)k * n + i]; V[(size_t)k * n + i] = V[(size_t)k * n + lo]; V[(size_t)k * n + lo] = v; }
    }
  }
  for (int i = 0; i < n; ++i) if (!std::isfinite(w[i])) return -1;
  return sweeps;
}

// G_A·v = θ·G_B·v for symmetric G_A and symmetric positive definite G_B: G_B = L·Lᵀ by the pivot rule with m_rule, M = L⁻¹·G_A·L⁻ᵀ (symmetrised),
// Jacobi on M, V = L⁻ᵀ·Z, so VᵀG_BV = I and VᵀG_AV = diag(θ), θ ascending.
// → the Jacobi sweeps (> 0); 0: G_B was refused by the pivot rule; −1: a NaN or Inf appeared; −2: Jacobi did not converge in 60 sweeps.
inline int generalized(int n, const double *GA, const double *GB, int m_rule, double *theta, double *V) {
  std::vector<double> L((size_t)n * n), M((size_t)n * n), T((size_t)n * n);
  for (int i = 0; i < n * n; ++i) if (!std::isfinite(GA[i]) || !std::isfinite(GB[i])) return GB[i] != GB[i] || std::isinf(GB[i]) ? 0 : -1;
  if (!cholesky(n, GB, m_rule, L.data())) return 0;
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) M[(size_t)i * n + j] = 0.5 * (GA[(size_t)i * n + j] + GA[(size_t)j * n + i]);
  solve_lower(n, L.data(), n, M.data());                                    // L⁻¹·G_A
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) T[(size_t)i * n + j] = M[(size_t)j * n + i];
  solve_lower(n, L.data(), n, T.data());                                    // L⁻¹·(L⁻¹·G_A)ᵀ = L⁻¹·G_A·L⁻ᵀ
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) M[(size_t)i * n + j] = 0.5 * (T[(size_t)i * n + j] + T[(size_t)j * n + i]);
  const int sweeps = jacobi(n, M.data(), theta, V);
  if (sweeps < 0) return sweeps;
  solve_lower_t(n, L.data(), n, V);
  return sweeps;
}
}   // namespace eig_dense
