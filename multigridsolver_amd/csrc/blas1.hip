// blas1.hip — vector updates and deterministic reductions: axpby / axpbypcz, dot, dot2, update + dot2, the PCG passes, sum / mean / shift for the
// constant null space, the label-segmented sum / shift for the field-wise one, the eigenresidual r = ax − θ·bx with its norm, several inner products in one pass (mdot), the multi-axpy with two sums (maxpy), the K-cycle's orthogonalised pair, and
// the host half of every reduction: partial buffers, the staged fold, results posted to the host.  gfx950 only.
// Every reduction pass leaves one partial (pair) per workgroup in a fixed layout and ends in the folds of blas1.hpp; the 8- and 16-byte forms
// of a pass are separate kernels, their summation orders differ on purpose (tests/blas1_ref.py restates both).
#include "blas1.hpp"

#include <chrono>
#include <time.h>

namespace {
using namespace blas1;

// ------------------------------------------------------------------ elementwise
__global__ void axpby_kernel(int64_t n, double a, const double *__restrict__ x, double b, double *__restrict__ y) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (b == 0.0) { for (; i < n; i += stride) y[i] = a * x[i]; }
  else { for (; i < n; i += stride) y[i] = a * x[i] + b * y[i]; }
}
__global__ void axpbypcz_kernel(int64_t n, double a, const double *__restrict__ x, double b,
                                const double *__restrict__ y, double c, double *__restrict__ z) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (c == 0.0) { for (; i < n; i += stride) z[i] = a * x[i] + b * y[i]; }
  else { for (; i < n; i += stride) z[i] = a * x[i] + b * y[i] + c * z[i]; }
}

// 16-byte forms of the two update kernels (option blas1_vec, default on; used when every operand is 16-byte aligned): each lane
// moves a pair of doubles per load/store and the loop is unrolled so that several loads per stream are in flight per wave — the
// 8-byte grid-stride loops above stop at ≈ 4 TB/s on this part, a pure stream wants ≥ 16 B per lane (MI355X_MICROARCH.md, HBM:
// 6.3 TB/s for a float4 copy).  Element i is computed by the same expression as above, so the results have the same bits.
template <bool HASB>
__global__ __launch_bounds__(TB) void axpby_vec_kernel(int64_t n, double a, const double *__restrict__ x, double b, double *__restrict__ y, int nts) {
  const int64_t n2 = n >> 1;
  const vd2 *__restrict__ xv = reinterpret_cast<const vd2 *>(x);
  vd2 *__restrict__ yv = reinterpret_cast<vd2 *>(y);
  const int64_t stride = (int64_t)gridDim.x * TB;
#pragma unroll 4
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n2; i += stride) {
    const vd2 p = xv[i]; vd2 q;
    if (HASB) { const vd2 o = yv[i]; q.x = a * p.x + b * o.x; q.y = a * p.y + b * o.y; }
    else { q.x = a * p.x; q.y = a * p.y; }
    st2(yv + i, q, nts != 0);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) y[n - 1] = HASB ? a * x[n - 1] + b * y[n - 1] : a * x[n - 1];
}
template <bool HASC>
__global__ __launch_bounds__(TB) void axpbypcz_vec_kernel(int64_t n, double a, const double *__restrict__ x, double b,
                                                          const double *__restrict__ y, double c, double *__restrict__ z, int nts) {
  const int64_t n2 = n >> 1;
  const vd2 *__restrict__ xv = reinterpret_cast<const vd2 *>(x);
  const vd2 *__restrict__ yv = reinterpret_cast<const vd2 *>(y);
  vd2 *__restrict__ zv = reinterpret_cast<vd2 *>(z);
  const int64_t stride = (int64_t)gridDim.x * TB;
#pragma unroll 4
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n2; i += stride) {
    const vd2 p = xv[i], o = yv[i]; vd2 q;
    if (HASC) { const vd2 w = zv[i]; q.x = a * p.x + b * o.x + c * w.x; q.y = a * p.y + b * o.y + c * w.y; }
    else { q.x = a * p.x + b * o.x; q.y = a * p.y + b * o.y; }
    st2(zv + i, q, nts != 0);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) z[n - 1] = HASC ? a * x[n - 1] + b * y[n - 1] + c * z[n - 1] : a * x[n - 1] + b * y[n - 1];
}

// ------------------------------------------------------------------ reductions
// Two-stage deterministic dot: fixed grid of partials (independent of scheduling), then one
// block folds them in index order.  reference bicg.cpp:64-72 (dot/norm helpers).
// where the last stage of a reduction posts its results for the host (see fetch_results): mapped host buffer + ticket; hv = NULL: nowhere
struct Post { double *hv; unsigned long long *ht; unsigned long long ticket; };
__device__ __forceinline__ void post_to_host(const Post &pa, const double *vals, int cnt) {
  for (int q = 0; q < cnt; ++q) __hip_atomic_store(pa.hv + q, vals[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(pa.ht, pa.ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
constexpr int DOT_BLOCKS = 4096;   // partial slots (a pair kernel uses half of them per sum): 8 workgroups per CU on 256 CUs
__global__ __launch_bounds__(TB) void dot_partial_kernel(int64_t n, const double *__restrict__ x, const double *__restrict__ y, double *__restrict__ part) {
  __shared__ double sh[TB / 64];
  double s = 0.0;
  int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TB;
  for (; i < n; i += stride) s += x[i] * y[i];
  BLAS1_FOLD1(s, sh, part, false);      // up to DOT_BLOCKS single partials: there is no room for a second row
}
__global__ __launch_bounds__(TB) void dot_final_kernel(int nb, const double *__restrict__ part, double *__restrict__ out, Post pa) {
  __shared__ double sh[TB];
  const double r = final_fold(nb, part, sh);
  if (threadIdx.x == 0) { out[0] = r; if (pa.hv) post_to_host(pa, &r, 1); }
}

// two inner products in one pass and one host round trip: (x·y, z·w) — BiCGSTAB's (t·s, t·t) and (r·r, r̃·r)
__global__ __launch_bounds__(TB) void dot2_partial_kernel(int64_t n, const double *__restrict__ x, const double *__restrict__ y,
                                                          const double *__restrict__ z, const double *__restrict__ w, double *__restrict__ part) {
  __shared__ double sh[2][TB / 64];
  double s0 = 0.0, s1 = 0.0;
  int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TB;
  for (; i < n; i += stride) { s0 += x[i] * y[i]; s1 += z[i] * w[i]; }
  BLAS1_FOLD2(s0, s1, sh, part);
}
__global__ __launch_bounds__(TB) void dot2_final_kernel(int nb, const double *__restrict__ part, double *__restrict__ out, Post pa) {
  __shared__ double sh[TB];
  double res[2] = {0.0, 0.0};
  for (int q = 0; q < 2; ++q) {
    res[q] = final_fold(nb, part + q * nb, sh);
    if (threadIdx.x == 0) out[q] = res[q];
    __syncthreads();
  }
  if (threadIdx.x == 0 && pa.hv) post_to_host(pa, res, 2);
}

// z = a·x + b·y fused with (z·z, w·z): BiCGSTAB's s = r − αv with ‖s‖² and r = s − ωt with (‖r‖², r̃·r) in one pass each
__global__ __launch_bounds__(TB) void update_dot2_partial_kernel(int64_t n, double a, const double *__restrict__ x, double b, const double *__restrict__ y,
                                                                 double *__restrict__ z, const double *__restrict__ w, double *__restrict__ part) {
  __shared__ double sh[2][TB / 64];
  double s0 = 0.0, s1 = 0.0;
  int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TB;
  for (; i < n; i += stride) {
    const double zi = a * x[i] + b * y[i];
    z[i] = zi;
    s0 += zi * zi;
    if (w) s1 += w[i] * zi;
  }
  BLAS1_FOLD2(s0, s1, sh, part);
}

// 16-byte form of the kernel above (same per-element expression; the partial sums associate differently: lane t adds its pairs
// x then y, a fixed order that does not depend on scheduling)
template <bool HASW>
__global__ __launch_bounds__(TB) void update_dot2_partial_vec_kernel(int64_t n, double a, const double *__restrict__ x, double b, const double *__restrict__ y,
                                                                     double *__restrict__ z, const double *__restrict__ w, double *__restrict__ part, int nts) {
  __shared__ double sh[2][TB / 64];
  const int64_t n2 = n >> 1;
  const vd2 *__restrict__ xv = reinterpret_cast<const vd2 *>(x);
  const vd2 *__restrict__ yv = reinterpret_cast<const vd2 *>(y);
  const vd2 *__restrict__ wv = reinterpret_cast<const vd2 *>(w);
  vd2 *__restrict__ zv = reinterpret_cast<vd2 *>(z);
  double s0 = 0.0, s1 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * TB;
#pragma unroll 4
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n2; i += stride) {
    const vd2 p = xv[i], o = yv[i]; vd2 q;
    q.x = a * p.x + b * o.x; q.y = a * p.y + b * o.y;
    st2(zv + i, q, nts != 0);
    s0 += q.x * q.x; s0 += q.y * q.y;
    if (HASW) { const vd2 ww = wv[i]; s1 += ww.x * q.x; s1 += ww.y * q.y; }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double zi = a * x[n - 1] + b * y[n - 1];
    z[n - 1] = zi; s0 += zi * zi;
    if (HASW) s1 += w[n - 1] * zi;
  }
  BLAS1_FOLD2(s0, s1, sh, part);
}

// ------------------------------------------------------------------ preconditioned CG (mgs_pcg): the two passes beside dots, cycle and SpMV
// Direction pass with the LAGGED x update: x ← x + a·p (the step the previous iteration decided; its p is read here anyway), then
// p ← z + beta·p.  40 B per row (read x, p, z; write x, p) — applied eagerly the x update is a pass of its own (24 B per row more).
// FIRST (first direction, and the one after a restart): p ← z only; p is NOT read (a pool vector may hold anything, 0·NaN = NaN)
// and x is not touched (the caller has flushed every pending update before).
template <bool FIRST>
__global__ __launch_bounds__(TB) void pcg_dir_kernel(int64_t n, double a, double beta, double *__restrict__ x, double *__restrict__ p,
                                                     const double *__restrict__ z) {
  int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (; i < n; i += stride) {
    if (FIRST) p[i] = z[i];
    else { const double pi = p[i]; x[i] = x[i] + a * pi; p[i] = z[i] + beta * pi; }
  }
}
// 16-byte form (same per-element expressions: same bits)
template <bool FIRST>
__global__ __launch_bounds__(TB) void pcg_dir_vec_kernel(int64_t n, double a, double beta, double *__restrict__ x, double *__restrict__ p,
                                                         const double *__restrict__ z, int nts) {
  const int64_t n2 = n >> 1;
  vd2 *__restrict__ xv = reinterpret_cast<vd2 *>(x);
  vd2 *__restrict__ pv = reinterpret_cast<vd2 *>(p);
  const vd2 *__restrict__ zv = reinterpret_cast<const vd2 *>(z);
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n2; i += stride) {
    const vd2 zi = zv[i];
    if (FIRST) st2(pv + i, zi, nts != 0);
    else {
      const vd2 pi = pv[i], xi = xv[i]; vd2 xo, po;
      xo.x = xi.x + a * pi.x; xo.y = xi.y + a * pi.y;
      po.x = zi.x + beta * pi.x; po.y = zi.y + beta * pi.y;
      st2(xv + i, xo, nts != 0);
      st2(pv + i, po, nts != 0);
    }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    if (FIRST) p[n - 1] = z[n - 1];
    else { const double pi = p[n - 1]; x[n - 1] = x[n - 1] + a * pi; p[n - 1] = z[n - 1] + beta * pi; }
  }
}
// Residual pass IN PLACE: r ← r − a·q with ‖r‖² (24 B per row: read r, q; write r).  update_dot2_partial*_kernel is out of place
// (`__restrict__` on source and destination) and must not be aliased.  Partial pair per workgroup, the second sum stays zero so
// that the staged fold of the pairs (k_dot2_finish) serves.
__global__ __launch_bounds__(TB) void pcg_resid_kernel(int64_t n, double a, double *__restrict__ r, const double *__restrict__ q, double *__restrict__ part) {
  __shared__ double sh[TB / 64];
  double s0 = 0.0;
  int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (; i < n; i += stride) { const double ri = r[i] - a * q[i]; r[i] = ri; s0 += ri * ri; }
  BLAS1_FOLD1(s0, sh, part, true);
}
// 16-byte form (same per-element expression; lane t adds its pair x then y, a fixed order that does not depend on scheduling)
__global__ __launch_bounds__(TB) void pcg_resid_vec_kernel(int64_t n, double a, double *__restrict__ r, const double *__restrict__ q, double *__restrict__ part, int nts) {
  __shared__ double sh[TB / 64];
  const int64_t n2 = n >> 1;
  vd2 *__restrict__ rv = reinterpret_cast<vd2 *>(r);
  const vd2 *__restrict__ qv = reinterpret_cast<const vd2 *>(q);
  double s0 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n2; i += stride) {
    const vd2 ri = rv[i], qi = qv[i]; vd2 o;
    o.x = ri.x - a * qi.x; o.y = ri.y - a * qi.y;
    st2(rv + i, o, nts != 0);
    s0 += o.x * o.x; s0 += o.y * o.y;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) { const double ri = r[n - 1] - a * q[n - 1]; r[n - 1] = ri; s0 += ri * ri; }
  BLAS1_FOLD1(s0, sh, part, true);
}

// one or two inner products, one pair of elements per lane, one-shot workgroups (see grid_vec): partial pair per workgroup ([2][gridDim.x];
// NP = 1 leaves the second sum at zero so that the staged fold of the pairs serves both)
template <int NP>
__global__ __launch_bounds__(TB) void dot_block_vec_kernel(int64_t n, const double *__restrict__ x, const double *__restrict__ y,
                                                           const double *__restrict__ z, const double *__restrict__ w, double *__restrict__ part) {
  __shared__ double sh[2][TB / 64];
  const int64_t n2 = n >> 1;
  const vd2 *__restrict__ xv = reinterpret_cast<const vd2 *>(x);
  const vd2 *__restrict__ yv = reinterpret_cast<const vd2 *>(y);
  const vd2 *__restrict__ zv = reinterpret_cast<const vd2 *>(z);
  const vd2 *__restrict__ wv = reinterpret_cast<const vd2 *>(w);
  double s0 = 0.0, s1 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n2; i += stride) {
    const vd2 p = xv[i], q = yv[i];
    s0 += p.x * q.x; s0 += p.y * q.y;
    if (NP == 2) { const vd2 a = zv[i], b = wv[i]; s1 += a.x * b.x; s1 += a.y * b.y; }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) { s0 += x[n - 1] * y[n - 1]; if (NP == 2) s1 += z[n - 1] * w[n - 1]; }
  BLAS1_FOLD2(s0, s1, sh, part);
}

// ------------------------------------------------------------------ eigenresidual (mgs_eig_residual): r = ax − θ·bx with ‖r‖², one pass
// Per entry t = fl(θ·bx_i), r_i = fl(ax_i − t), and fl(r_i·r_i) is added (-ffp-contract=off keeps the three roundings apart).  32 B per row: three
// reads and one write, where a 2 → 1 combine followed by k_dot moves 40 B in two launches.  The sums are k_dot's: the 8-byte form leaves one
// partial per workgroup for dot_final_kernel, the 16-byte form a pair (second sum zero) for k_dot2_finish, lane t adding its pair x then y and the
// odd last element going to lane 0 of workgroup 0 — ‖r‖² carries the bits of k_dot(r, r).  r may be ax or bx: a lane loads its entry (pair) of
// both inputs before it stores, and no lane reads what another one stores (no __restrict__ on the three).
__global__ __launch_bounds__(TB) void eig_residual_kernel(int64_t n, const double *ax, const double *bx, double theta, double *r, double *__restrict__ part) {
  __shared__ double sh[TB / 64];
  double s = 0.0;
  int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (; i < n; i += stride) { const double t = theta * bx[i]; const double ri = ax[i] - t; r[i] = ri; s += ri * ri; }
  BLAS1_FOLD1(s, sh, part, false);
}
__global__ __launch_bounds__(TB) void eig_residual_vec_kernel(int64_t n, const double *ax, const double *bx, double theta, double *r, double *__restrict__ part, int nts) {
  __shared__ double sh[2][TB / 64];
  const int64_t n2 = n >> 1;
  const vd2 *av = reinterpret_cast<const vd2 *>(ax);
  const vd2 *bv = reinterpret_cast<const vd2 *>(bx);
  vd2 *rv = reinterpret_cast<vd2 *>(r);
  double s0 = 0.0, s1 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n2; i += stride) {
    const vd2 a = av[i], b = bv[i]; vd2 t, o;
    t.x = theta * b.x; t.y = theta * b.y;
    o.x = a.x - t.x; o.y = a.y - t.y;
    st2(rv + i, o, nts != 0);
    s0 += o.x * o.x; s0 += o.y * o.y;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) { const double t = theta * bx[n - 1]; const double ri = ax[n - 1] - t; r[n - 1] = ri; s0 += ri * ri; }
  BLAS1_FOLD2(s0, s1, sh, part);
}

// ------------------------------------------------------------------ constant null space: v ← v − mean(v) (k_project_const)
// Two launches beside the fold, the scalar stays on the device.  Sum pass: one partial per workgroup in a fixed layout ([2][gridDim.x], the
// second sum zero so that dot2_mid_kernel / k_dot2_finish serve), folded in index order by one workgroup whose last step stores m = sum/n —
// the order does not depend on scheduling, so m and with it every shifted entry is bit-reproducible from run to run.  Shift pass:
// v_i ← v_i − m with m loaded once per lane; NRM adds ‖v − m‖² (partial pair per workgroup); STORE = false leaves v as it is (‖Πb‖ of the
// caller's const right-hand side).  24 B per row for the pair (read, read, write).
__global__ __launch_bounds__(TB) void sum_partial_kernel(int64_t n, const double *__restrict__ v, double *__restrict__ part) {
  __shared__ double sh[TB / 64];
  double s = 0.0;
  int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (; i < n; i += stride) s += v[i];
  BLAS1_FOLD1(s, sh, part, true);
}
// 16-byte form (lane t adds its pair x then y, a fixed order)
__global__ __launch_bounds__(TB) void sum_partial_vec_kernel(int64_t n, const double *__restrict__ v, double *__restrict__ part) {
  __shared__ double sh[TB / 64];
  const int64_t n2 = n >> 1;
  const vd2 *__restrict__ vv = reinterpret_cast<const vd2 *>(v);
  double s = 0.0;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n2; i += stride) { const vd2 p = vv[i]; s += p.x; s += p.y; }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) s += v[n - 1];
  BLAS1_FOLD1(s, sh, part, true);
}
__global__ __launch_bounds__(TB) void mean_final_kernel(int nb, const double *__restrict__ part, double n, double *__restrict__ mean) {
  __shared__ double sh[TB];
  const double r = final_fold(nb, part, sh);
  if (threadIdx.x == 0) mean[0] = r / n;
}
template <bool STORE, bool NRM>
__global__ __launch_bounds__(TB) void shift_const_kernel(int64_t n, double *__restrict__ v, const double *__restrict__ mean, double *__restrict__ part) {
  __shared__ double sh[TB / 64];
  const double m = mean[0];
  double s0 = 0.0;
  int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (; i < n; i += stride) { const double o = v[i] - m; if (STORE) v[i] = o; if (NRM) s0 += o * o; }
  if (!NRM) return;
  BLAS1_FOLD1(s0, sh, part, true);
}
// 16-byte form (same per-element expression: same bits)
template <bool STORE, bool NRM>
__global__ __launch_bounds__(TB) void shift_const_vec_kernel(int64_t n, double *__restrict__ v, const double *__restrict__ mean, double *__restrict__ part, int nts) {
  __shared__ double sh[TB / 64];
  const double m = mean[0];
  const int64_t n2 = n >> 1;
  vd2 *__restrict__ vv = reinterpret_cast<vd2 *>(v);
  double s0 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n2; i += stride) {
    const vd2 p = vv[i]; vd2 o;
    o.x = p.x - m; o.y = p.y - m;
    if (STORE) st2(vv + i, o, nts != 0);
    if (NRM) { s0 += o.x * o.x; s0 += o.y * o.y; }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) { const double o = v[n - 1] - m; if (STORE) v[n - 1] = o; if (NRM) s0 += o * o; }
  if (!NRM) return;
  BLAS1_FOLD1(s0, sh, part, true);
}

// ------------------------------------------------------------------ field-wise constant null space: v_i ← v_i − m[label_i] (k_project_fields)
// The same two launches beside the fold with a label per row (int8, −1 = in no field).  Sum pass: one walk over v and the labels, one
// accumulator per field and lane, an entry added only to the accumulator of its own label (an unlabelled NaN poisons nothing); partials in a
// fixed [nf][gridDim.x] layout, no atomics; fields_mean_final_kernel folds each field's partials in index order and stores m_f = sum_f/n_f
// in the matrix's own slots.  A pair (or entry) without a labelled row is not loaded at all: on a saddle system only the pressure rows are
// streamed.  Shift pass: the means sit in LDS, rows labelled −1 keep their bits (a pair without a labelled row is not stored); NRM adds
// ‖Πv‖² over ALL rows (partial pair per workgroup); STORE = false leaves v as it is.  25 B per labelled row for the pair of passes.
constexpr int NSF = MGS_NULLSPACE_MAX_FIELDS;
struct FieldCounts { double n[NSF]; };
typedef signed char lab2 __attribute__((ext_vector_type(2)));
// the end of the sum pass: every lane's NSF accumulators → part[f][blockIdx.x], waves added in wave order from 0.0
#define FIELDS_FOLD(s, nf, sh, part)                                                                                       \
  do {                                                                                                                     \
    _Pragma("unroll") for (int k = 0; k < NSF; ++k) {                                                                      \
      if (k < nf) {                                                                                                        \
        double t = s[k];                                                                                                   \
        for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off);                                                   \
        if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = t;                                                          \
      }                                                                                                                    \
    }                                                                                                                      \
    __syncthreads();                                                                                                       \
    if ((int)threadIdx.x < nf) {                                                                                           \
      double t = 0.0;                                                                                                      \
      for (int q = 0; q < TB / 64; ++q) t += sh[threadIdx.x][q];                                                           \
      part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = t;                                                              \
    }                                                                                                                      \
  } while (0)
__global__ __launch_bounds__(TB) void fields_sum_kernel(int64_t n, int nf, const double *__restrict__ v, const signed char *__restrict__ lab, double *__restrict__ part) {
  __shared__ double sh[NSF][TB / 64];
  double s[NSF];
#pragma unroll
  for (int k = 0; k < NSF; ++k) s[k] = 0.0;
  int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (; i < n; i += stride) {
    const int l = lab[i];
    if (l < 0) continue;
    const double x = v[i];
#pragma unroll
    for (int k = 0; k < NSF; ++k) if (l == k) s[k] += x;
  }
  FIELDS_FOLD(s, nf, sh, part);
}
// 16-byte form: the labels of a pair are one 2-byte load (lane t adds its pair x then y, a fixed order)
__global__ __launch_bounds__(TB) void fields_sum_vec_kernel(int64_t n, int nf, const double *__restrict__ v, const signed char *__restrict__ lab, double *__restrict__ part) {
  __shared__ double sh[NSF][TB / 64];
  double s[NSF];
#pragma unroll
  for (int k = 0; k < NSF; ++k) s[k] = 0.0;
  const int64_t n2 = n >> 1;
  const vd2 *__restrict__ vv = reinterpret_cast<const vd2 *>(v);
  const lab2 *__restrict__ lv = reinterpret_cast<const lab2 *>(lab);
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n2; i += stride) {
    const lab2 l = lv[i];
    const int lx = l.x, ly = l.y;
    if (lx < 0 && ly < 0) continue;
    const vd2 p = vv[i];
#pragma unroll
    for (int k = 0; k < NSF; ++k) { if (lx == k) s[k] += p.x; if (ly == k) s[k] += p.y; }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int l = lab[n - 1];
    if (l >= 0) {
      const double x = v[n - 1];
#pragma unroll
      for (int k = 0; k < NSF; ++k) if (l == k) s[k] += x;
    }
  }
  FIELDS_FOLD(s, nf, sh, part);
}
#undef FIELDS_FOLD
// middle stage for long partial arrays, one row of workgroups per field (dot2_mid_kernel's chunks): out [nf][gridDim.x]
__global__ __launch_bounds__(TB) void fields_mid_kernel(int nb, int chunk, const double *__restrict__ part, double *__restrict__ out) {
  __shared__ double sh[TB / 64];
  const int lo = blockIdx.x * chunk, hi = min(lo + chunk, nb);
  const double *__restrict__ p = part + (size_t)blockIdx.y * nb;
  double *__restrict__ o = out + (size_t)blockIdx.y * gridDim.x;
  double s = 0.0;
  for (int i = lo + threadIdx.x; i < hi; i += TB) s += p[i];
  BLAS1_FOLD1(s, sh, o, false);
}
__global__ __launch_bounds__(TB) void fields_mean_final_kernel(int nb, int nf, const double *__restrict__ part, const FieldCounts cnt, double *__restrict__ means) {
  __shared__ double sh[TB];
  for (int k = 0; k < nf; ++k) {
    const double r = final_fold(nb, part + (size_t)k * nb, sh);
    if (threadIdx.x == 0) means[k] = r / cnt.n[k];
    __syncthreads();
  }
}
template <bool STORE, bool NRM>
__global__ __launch_bounds__(TB) void fields_shift_kernel(int64_t n, int nf, double *__restrict__ v, const signed char *__restrict__ lab, const double *__restrict__ means,
                                                          double *__restrict__ part) {
  __shared__ double sh[TB / 64];
  __shared__ double sm[NSF];
  if ((int)threadIdx.x < NSF) sm[threadIdx.x] = (int)threadIdx.x < nf ? means[threadIdx.x] : 0.0;
  __syncthreads();
  double s0 = 0.0;
  int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (; i < n; i += stride) {
    const int l = lab[i];
    if (!NRM && l < 0) continue;
    double o = v[i];
    if (l >= 0) { o = o - sm[l & (NSF - 1)]; if (STORE) v[i] = o; }
    if (NRM) s0 += o * o;
  }
  if (!NRM) return;
  BLAS1_FOLD1(s0, sh, part, true);
}
// 16-byte form (same per-element expression: same bits)
template <bool STORE, bool NRM>
__global__ __launch_bounds__(TB) void fields_shift_vec_kernel(int64_t n, int nf, double *__restrict__ v, const signed char *__restrict__ lab, const double *__restrict__ means,
                                                              double *__restrict__ part, int nts) {
  __shared__ double sh[TB / 64];
  __shared__ double sm[NSF];
  if ((int)threadIdx.x < NSF) sm[threadIdx.x] = (int)threadIdx.x < nf ? means[threadIdx.x] : 0.0;
  __syncthreads();
  const int64_t n2 = n >> 1;
  vd2 *__restrict__ vv = reinterpret_cast<vd2 *>(v);
  const lab2 *__restrict__ lv = reinterpret_cast<const lab2 *>(lab);
  double s0 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n2; i += stride) {
    const lab2 l = lv[i];
    const int lx = l.x, ly = l.y;
    const bool any = lx >= 0 || ly >= 0;
    if (!NRM && !any) continue;
    vd2 o = vv[i];
    if (lx >= 0) o.x = o.x - sm[lx & (NSF - 1)];
    if (ly >= 0) o.y = o.y - sm[ly & (NSF - 1)];
    if (STORE && any) st2(vv + i, o, nts != 0);
    if (NRM) { s0 += o.x * o.x; s0 += o.y * o.y; }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int l = lab[n - 1];
    double o = v[n - 1];
    if (l >= 0) { o = o - sm[l & (NSF - 1)]; if (STORE) v[n - 1] = o; }
    if (NRM) s0 += o * o;
  }
  if (!NRM) return;
  BLAS1_FOLD1(s0, sh, part, true);
}

// ------------------------------------------------------------------ several inner products against one vector, one pass
// s_k = Σ a_i·b_k[i], k < K ≤ MDOT_MAX: `a` is read once.  Partials [K][gridDim.x] in a fixed order (no atomics), folded by
// mdot_final_kernel — the K-cycle's (ρ1, α1) and the flexible Krylov methods' orthogonalisation coefficients.
constexpr int MDOT_MAX = 16;
struct MDotVecs { const double *b[MDOT_MAX]; };
__global__ __launch_bounds__(TB) void mdot_partial_kernel(int64_t n, int K, const double *__restrict__ a, const MDotVecs B, double *__restrict__ part) {
  __shared__ double sh[MDOT_MAX][TB / 64];
  double s[MDOT_MAX];
#pragma unroll
  for (int k = 0; k < MDOT_MAX; ++k) s[k] = 0.0;
  const int64_t n2 = n >> 1, stride = (int64_t)gridDim.x * TB;
  const vd2 *__restrict__ av = reinterpret_cast<const vd2 *>(a);
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n2; i += stride) {
    const vd2 ai = av[i];
#pragma unroll
    for (int k = 0; k < MDOT_MAX; ++k)
      if (k < K) { const vd2 bi = reinterpret_cast<const vd2 *>(B.b[k])[i]; s[k] += ai.x * bi.x; s[k] += ai.y * bi.y; }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < MDOT_MAX; ++k) if (k < K) s[k] += a[n - 1] * B.b[k][n - 1];
  }
#pragma unroll
  for (int k = 0; k < MDOT_MAX; ++k) {
    if (k < K) {
      double t = s[k];
      for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off);
      if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = t;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < K) {
    double t = 0.0;
    for (int q = 0; q < TB / 64; ++q) t += sh[threadIdx.x][q];
    part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
  }
}
// fold of K partial arrays of nb entries each (one workgroup, fixed order); out (device) and, with pa.hv, the host's mapped buffer
__global__ __launch_bounds__(TB) void mdot_final_kernel(int nb, int K, const double *__restrict__ part, double *__restrict__ out, Post pa) {
  __shared__ double sh[TB];
  __shared__ double res[MDOT_MAX + 4];
  for (int k = 0; k < K; ++k) {
    const double r = final_fold(nb, part + (size_t)k * nb, sh);
    if (threadIdx.x == 0) { res[k] = r; if (out) out[k] = r; }
    __syncthreads();
  }
  if (threadIdx.x == 0 && pa.hv) post_to_host(pa, res, K);
}

// z = x − Σ_{j<K} coef_j·w_j (coefficients by value: they come from the host, which needed them for its own bookkeeping), with
// (z·z, z·u) accumulated in the same pass (u = NULL: second sum stays 0) — the orthogonalisation update of the flexible Krylov
// methods: the new direction against the window, its norm and its product with the residual, one read of every vector.
struct MAxpyArgs { const double *w[MDOT_MAX]; double coef[MDOT_MAX]; };
template <bool VEC>
__global__ __launch_bounds__(TB) void maxpy_dot2_kernel(int64_t n, int K, const double *__restrict__ x, const MAxpyArgs W, double *__restrict__ z,
                                                        const double *__restrict__ u, const double *__restrict__ u2, double *__restrict__ part) {
  __shared__ double sh[2][TB / 64];
  double s0 = 0.0, s1 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * TB;
  if (VEC) {              // 16 bytes per lane and stream (every operand 16-byte aligned; an odd last element goes to one lane below)
    const int64_t n2 = n >> 1;
    const vd2 *__restrict__ xv = reinterpret_cast<const vd2 *>(x);
    vd2 *__restrict__ zv = reinterpret_cast<vd2 *>(z);
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n2; i += stride) {
      vd2 zi = xv[i];
#pragma unroll
      for (int k = 0; k < MDOT_MAX; ++k)
        if (k < K) { const vd2 wi = reinterpret_cast<const vd2 *>(W.w[k])[i]; zi.x -= W.coef[k] * wi.x; zi.y -= W.coef[k] * wi.y; }
      zv[i] = zi;
      if (part) {
        if (u2) { const vd2 q = reinterpret_cast<const vd2 *>(u2)[i]; s0 += zi.x * q.x; s0 += zi.y * q.y; } else { s0 += zi.x * zi.x; s0 += zi.y * zi.y; }
        if (u) { const vd2 q = reinterpret_cast<const vd2 *>(u)[i]; s1 += zi.x * q.x; s1 += zi.y * q.y; }
      }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
      double zi = x[n - 1];
      for (int k = 0; k < K; ++k) zi -= W.coef[k] * W.w[k][n - 1];
      z[n - 1] = zi;
      s0 += zi * (u2 ? u2[n - 1] : zi);
      if (u) s1 += zi * u[n - 1];
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += stride) {
      double zi = x[i];
#pragma unroll
      for (int k = 0; k < MDOT_MAX; ++k) if (k < K) zi -= W.coef[k] * W.w[k][i];
      z[i] = zi;
      s0 += zi * (u2 ? u2[i] : zi);
      if (u) s1 += zi * u[i];
    }
  }
  if (!part) return;                               // plain multi-axpy
  BLAS1_FOLD2(s0, s1, sh, part);
}

// (ρ2, α2) of the K-cycle's orthogonalised second direction (cycle.hip; the scalars are described at kc_update_r_kernel in kernels_aux.hip):
// g = γ/ρ1, v2' = v2 − g·v1, d2' = c2 − g·c1 (energy form) or v2'; sums d2'·v2' and d2'·r'.  Partial pair per workgroup.
template <bool ENERGY>
__global__ __launch_bounds__(TB) void kc_orth_dots_kernel(int n, const double *__restrict__ scal, const double *__restrict__ c1, const double *__restrict__ c2,
                                                          const double *__restrict__ v1, const double *__restrict__ v2, const double *__restrict__ rp,
                                                          double *__restrict__ part) {
  __shared__ double sh[2][TB / 64];
  const double rho1 = scal[0], g = rho1 != 0.0 ? scal[2] / rho1 : 0.0;
  double s0 = 0.0, s1 = 0.0;
  const int stride = gridDim.x * TB;
  for (int i = blockIdx.x * TB + threadIdx.x; i < n; i += stride) {
    const double v2o = v2[i] - g * v1[i];
    const double d2o = ENERGY ? c2[i] - g * c1[i] : v2o;
    s0 += d2o * v2o;
    s1 += d2o * rp[i];
  }
  BLAS1_FOLD2(s0, s1, sh, part);
}
}  // namespace

// middle stage for long partial arrays (one pair per row block of a 512³ operator = 2 × 524 288): workgroup g sums the g-th
// contiguous chunk of each array in a fixed order
__global__ __launch_bounds__(TB) void dot2_mid_kernel(int nb, int chunk, const double *__restrict__ part, double *__restrict__ out /*[2][gridDim.x]*/) {
  __shared__ double sh[2][TB / 64];
  const int lo = blockIdx.x * chunk, hi = min(lo + chunk, nb);
  double s0 = 0.0, s1 = 0.0;
  for (int i = lo + threadIdx.x; i < hi; i += TB) { s0 += part[i]; s1 += part[nb + i]; }
  BLAS1_FOLD2(s0, s1, sh, out);
}

// ============================================================ host launchers
// Grid of the 16-byte update kernels: ONE pair per lane, one-shot workgroups (the loop in the kernels then runs once).  Measured at
// 512³ (tools/studies_r1_r3/blas1_grid.py): axpby 0.695 ms with the capped persistent grid (n_cu × 8 workgroups, grid-stride, unroll 4), 0.541 ms
// one-shot (5.96 TB/s); 2 / 4 / 8 pairs per lane: 0.568 / 0.623 / 0.671 ms — on this part a stream wants many short-lived
// workgroups, not a few resident ones (the row-block kernels are one-shot already; tools/microbench/rw_mix.hip shows the same).
// Option blas1_pairs = k: k pairs per lane (0: the capped grid), for that A/B.
static inline int grid_vec(int64_t n2, const mgs_ctx *ctx) {
  const int iters = ctx->opt_blas1_pairs;
  int64_t g = (n2 + TB - 1) / TB;
  if (iters > 0) { g = (g + iters - 1) / iters; return (int)(g < 1 ? 1 : g); }
  const int64_t cap = (int64_t)ctx->n_cu * 8;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}
// grid of an 8-byte grid-stride launch: one lane per entry, at most cap workgroups, at least one
static inline int grid_cap(int64_t n, int64_t cap) {
  const int64_t g = (n + TB - 1) / TB;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}
int mgs_blas1_grid(const mgs_ctx *ctx, int64_t n2) { return grid_vec(n2, ctx); }
int mgs_blas1_grid_capped(const mgs_ctx *ctx, int64_t n) { return grid_cap(n, (int64_t)ctx->n_cu * 8); }
// per-workgroup partial pairs of a one-shot reduction launch ([2][nb] doubles; grown outside any capture)
int mgs_ensure_dot_part(mgs_ctx *ctx, int64_t doubles) {
  if (ctx->dot_part_cap >= doubles) return MGS_OK;
  if (ctx->dot_part) { MGS_HIP(ctx, hipStreamSynchronize(ctx->stream)); mgs_hip_free(ctx->dot_part); ctx->dot_part = nullptr; ctx->dot_part_cap = 0; }
  MGS_TRY(mgs_dev_alloc(ctx, &ctx->dot_part, (size_t)doubles));
  ctx->dot_part_cap = doubles;
  return MGS_OK;
}
// where a pass leaves `doubles` partials: the context's own scratch while they fit, the grown buffer above
static int part_buf(mgs_ctx *ctx, int64_t doubles, double **part) {
  *part = ctx->red_dev;
  if (doubles > DOT_BLOCKS) { MGS_TRY(mgs_ensure_dot_part(ctx, doubles)); *part = ctx->dot_part; }
  return MGS_OK;
}
// A reduction launch with a partial pair per workgroup: how many workgroups, where the partials go, the store mode.  vec: the 16-byte kernel over
// n2 pairs (one-shot grid, grown scratch above DOT_BLOCKS / 2 workgroups); else the 8-byte kernel, clamped so that the pairs fit red_dev.
// Which of the two runs is the launcher's decision: the alignment predicates differ from pass to pass.
struct RedLaunch { int nb; double *part; int nts; };
static int red_launch(mgs_ctx *ctx, int64_t n, bool vec, int64_t n2, RedLaunch *L) {
  L->nts = nts_of(ctx, n);
  L->nb = vec ? grid_vec(n2, ctx) : grid_cap(n, DOT_BLOCKS / 2);
  return part_buf(ctx, 2 * (int64_t)L->nb, &L->part);
}

int k_axpby(mgs_ctx *ctx, int64_t n, double a, const double *x, double b, double *y) {
  if (n && ctx->opt_blas1_vec && al16(x) && al16(y)) {
    const dim3 g(grid_vec((n + 1) / 2, ctx));
    const int nts = nts_of(ctx, n);
    if (b == 0.0) hipLaunchKernelGGL(axpby_vec_kernel<false>, g, dim3(TB), 0, ctx->stream, n, a, x, b, y, nts);
    else hipLaunchKernelGGL(axpby_vec_kernel<true>, g, dim3(TB), 0, ctx->stream, n, a, x, b, y, nts);
  } else
  if (n) hipLaunchKernelGGL(axpby_kernel, dim3(mgs_blas1_grid_capped(ctx, n)), dim3(TB), 0, ctx->stream, n, a, x, b, y);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_axpbypcz(mgs_ctx *ctx, int64_t n, double a, const double *x, double b, const double *y, double c, double *z) {
  if (n && ctx->opt_blas1_vec && al16(x) && al16(y) && al16(z)) {
    const dim3 g(grid_vec((n + 1) / 2, ctx));
    const int nts = nts_of(ctx, n);
    if (c == 0.0) hipLaunchKernelGGL(axpbypcz_vec_kernel<false>, g, dim3(TB), 0, ctx->stream, n, a, x, b, y, c, z, nts);
    else hipLaunchKernelGGL(axpbypcz_vec_kernel<true>, g, dim3(TB), 0, ctx->stream, n, a, x, b, y, c, z, nts);
  } else
  if (n) hipLaunchKernelGGL(axpbypcz_kernel, dim3(mgs_blas1_grid_capped(ctx, n)), dim3(TB), 0, ctx->stream, n, a, x, b, y, c, z);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

// ---- results of a reduction to the host without a copy engine and without an interrupt
// The last stage of a reduction (one workgroup) stores the folded values into red_dev[DOT_BLOCKS ..] and, for the host, into the
// context's mapped, coherent host buffer, then a ticket (system-scope release); the host polls the ticket.  Against hipMemcpyAsync + hipStreamSynchronize this removes
// the blit/SDMA hop and the interrupt wake-up from every inner product of a Krylov loop: four per BiCGSTAB iteration — ≈ 60 of the
// 135 µs of an iteration on the bundled operators, and on a freshly started box, where the first process' wake-ups take milliseconds,
// 13 of 33 ms per iteration at 512³ (tools/studies_r1_r3/solve_repeat.py).  Option post_results = 0 restores copy + synchronize; so does any
// transport that sums over ranks in between (ncomm / all-reduce callback), and a wait that sees no ticket for 2 s.
static Post begin_post(mgs_ctx *ctx) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  const bool posted = ctx->opt_post_results && ctx->red_host_dev && !ctx->ncomm && hipStreamIsCapturing(ctx->stream, &cs) == hipSuccess &&
                      cs == hipStreamCaptureStatusNone;
  if (!posted) return Post{nullptr, nullptr, 0ull};
  return Post{ctx->red_host_dev, reinterpret_cast<unsigned long long *>(ctx->red_host_dev + MGS_RED_VALS), ++ctx->red_ticket};
}
// the reduction's last kernel (launched with `pa`) has been enqueued: wait for its results
static int fetch_results(mgs_ctx *ctx, int cnt, double *out_host, const Post &pa) {
  if (pa.hv) {
    volatile unsigned long long *tk = reinterpret_cast<volatile unsigned long long *>(ctx->red_host + MGS_RED_VALS);
    const unsigned long long want = pa.ticket;
    MGS_HIP(ctx, hipGetLastError());
    const auto t0 = std::chrono::steady_clock::now();
    bool seen = false;
    for (;;) {
      if (__atomic_load_n(const_cast<unsigned long long *>(tk), __ATOMIC_ACQUIRE) == want) { seen = true; break; }
      const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (waited > 2.0) break;                                   // never seen: fall back to the stream's own completion below
      if (waited < 300e-6) { for (int q = 0; q < 8; ++q) __builtin_ia32_pause(); }
      else { struct timespec ts = {0, 25000}; nanosleep(&ts, nullptr); }     // long kernels ahead of the ticket: stop burning the core
    }
    if (!seen) {
      MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
      if (__atomic_load_n(const_cast<unsigned long long *>(tk), __ATOMIC_ACQUIRE) != want)
        return mgs_fail(ctx, MGS_ERR_HIP, "reduction results never reached the host buffer");
    }
    for (int q = 0; q < cnt; ++q) out_host[q] = ctx->red_host[q];
  } else {
    MGS_HIP(ctx, hipMemcpyAsync(ctx->red_host, ctx->red_dev + DOT_BLOCKS, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, ctx->stream));
    MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int q = 0; q < cnt; ++q) out_host[q] = ctx->red_host[q];
  }
  if (ctx->allreduce && !ctx->ncomm) {
    int rc = ctx->allreduce(ctx->allreduce_user, out_host, cnt);
    if (rc) return mgs_fail(ctx, MGS_ERR_STATE, "allreduce callback failed (%d)", rc);
  }
  return MGS_OK;
}

// "Enqueue and fold" without "fetch" (mgs_pcg_plan, pcg_plan.hip): a reduction called with a NULL host pointer launches exactly what it
// launches otherwise, posts nothing and returns as soon as the fold is enqueued; the folded values stay in red_dev[DOT_BLOCKS ..], where the
// next kernel on the stream finds them.  With a host pointer nothing changes.
static const Post NO_POST = {nullptr, nullptr, 0ull};
static int fetch_or_leave(mgs_ctx *ctx, int cnt, double *out_host, const Post &pa) {
  if (out_host) return fetch_results(ctx, cnt, out_host, pa);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

// long partial arrays (more than 4096 pairs): 256 chunk sums first, left in red_dev, which the last stage then folds
static void fold_mid(mgs_ctx *ctx, int *nb, const double **part) {
  if (*nb <= 4096) return;
  const int groups = 256, chunk = (*nb + groups - 1) / groups;
  hipLaunchKernelGGL(dot2_mid_kernel, dim3(groups), dim3(TB), 0, ctx->stream, *nb, chunk, *part, ctx->red_dev);
  *part = ctx->red_dev; *nb = groups;
}
// the staged fold of nb partial pairs into out_dev[0..1]: two stages, or three (row-block partials → 256 chunk sums → the pair)
static int dot2_fold_into(mgs_ctx *ctx, int nb, const double *part, double *out_dev, const Post &pa) {
  fold_mid(ctx, &nb, &part);
  hipLaunchKernelGGL(dot2_final_kernel, dim3(1), dim3(TB), 0, ctx->stream, nb, part, out_dev, pa);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_dot2_finish(mgs_ctx *ctx, int nb, const double *part, double *out_host2) {
  const Post pa = out_host2 ? begin_post(ctx) : NO_POST;
  MGS_TRY(dot2_fold_into(ctx, nb, part, ctx->red_dev + DOT_BLOCKS, pa));
  if (ctx->ncomm) MGS_TRY(mgs_comm_allreduce_sum(ctx->ncomm, ctx->red_dev + DOT_BLOCKS, 2));
  return fetch_or_leave(ctx, 2, out_host2, pa);
}

int k_dot(mgs_ctx *ctx, int64_t n, const double *x, const double *y, double *out_host) {
  if (ctx->opt_blas1_vec && n >= 2 && al16(x) && al16(y)) {       // one-shot workgroups, staged fold (as the fused update kernels)
    RedLaunch L;
    MGS_TRY(red_launch(ctx, n, true, n / 2, &L));
    hipLaunchKernelGGL(dot_block_vec_kernel<1>, dim3(L.nb), dim3(TB), 0, ctx->stream, n, x, y, x, y, L.part);
    MGS_HIP(ctx, hipGetLastError());
    if (!out_host) return k_dot2_finish(ctx, L.nb, L.part, nullptr);
    double two[2] = {0.0, 0.0};
    MGS_TRY(k_dot2_finish(ctx, L.nb, L.part, two));
    *out_host = two[0];
    return MGS_OK;
  }
  const int nb = grid_cap(n, DOT_BLOCKS);
  hipLaunchKernelGGL(dot_partial_kernel, dim3(nb), dim3(TB), 0, ctx->stream, n, x, y, ctx->red_dev);
  const Post pa = out_host ? begin_post(ctx) : NO_POST;
  hipLaunchKernelGGL(dot_final_kernel, dim3(1), dim3(TB), 0, ctx->stream, nb, ctx->red_dev, ctx->red_dev + DOT_BLOCKS, pa);
  if (ctx->ncomm) MGS_TRY(mgs_comm_allreduce_sum(ctx->ncomm, ctx->red_dev + DOT_BLOCKS, 1));   // sum over the row shards, on this stream
  return fetch_or_leave(ctx, 1, out_host, pa);
}
// r = ax − θ·bx and ‖r‖² (mgs_eig_residual): k_dot's launch decisions with r among the pointers that must start on 16 bytes, k_dot's folds, so the
// norm is k_dot(r, r) bit for bit.  out_host = NULL: enqueue and fold, do not fetch.
int k_eig_residual(mgs_ctx *ctx, int64_t n, const double *ax, const double *bx, double theta, double *r, double *out_host) {
  if (ctx->opt_blas1_vec && n >= 2 && al16(ax) && al16(bx) && al16(r)) {
    RedLaunch L;
    MGS_TRY(red_launch(ctx, n, true, n / 2, &L));
    hipLaunchKernelGGL(eig_residual_vec_kernel, dim3(L.nb), dim3(TB), 0, ctx->stream, n, ax, bx, theta, r, L.part, L.nts);
    MGS_HIP(ctx, hipGetLastError());
    if (!out_host) return k_dot2_finish(ctx, L.nb, L.part, nullptr);
    double two[2] = {0.0, 0.0};
    MGS_TRY(k_dot2_finish(ctx, L.nb, L.part, two));
    *out_host = two[0];
    return MGS_OK;
  }
  const int nb = grid_cap(n, DOT_BLOCKS);
  hipLaunchKernelGGL(eig_residual_kernel, dim3(nb), dim3(TB), 0, ctx->stream, n, ax, bx, theta, r, ctx->red_dev);
  const Post pa = out_host ? begin_post(ctx) : NO_POST;
  hipLaunchKernelGGL(dot_final_kernel, dim3(1), dim3(TB), 0, ctx->stream, nb, ctx->red_dev, ctx->red_dev + DOT_BLOCKS, pa);
  if (ctx->ncomm) MGS_TRY(mgs_comm_allreduce_sum(ctx->ncomm, ctx->red_dev + DOT_BLOCKS, 1));
  return fetch_or_leave(ctx, 1, out_host, pa);
}
int k_dot_dev(mgs_ctx *ctx, int64_t n, const double *x, const double *y, double *out_dev) {
  const int nb = grid_cap(n, DOT_BLOCKS);
  hipLaunchKernelGGL(dot_partial_kernel, dim3(nb), dim3(TB), 0, ctx->stream, n, x, y, ctx->red_dev);
  hipLaunchKernelGGL(dot_final_kernel, dim3(1), dim3(TB), 0, ctx->stream, nb, ctx->red_dev, out_dev, NO_POST);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_dot2(mgs_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w, double *out_host2) {
  const bool vec = ctx->opt_blas1_vec && n >= 2 && al16(x) && al16(y) && al16(z) && al16(w);
  RedLaunch L;
  MGS_TRY(red_launch(ctx, n, vec, n / 2, &L));
  if (vec) hipLaunchKernelGGL(dot_block_vec_kernel<2>, dim3(L.nb), dim3(TB), 0, ctx->stream, n, x, y, z, w, L.part);
  else hipLaunchKernelGGL(dot2_partial_kernel, dim3(L.nb), dim3(TB), 0, ctx->stream, n, x, y, z, w, L.part);
  MGS_HIP(ctx, hipGetLastError());
  return k_dot2_finish(ctx, L.nb, L.part, out_host2);
}
int k_update_dot2(mgs_ctx *ctx, int64_t n, double a, const double *x, double b, const double *y, double *z, const double *w, double *out_host2) {
  // 16-byte form: one-shot workgroups (see grid_vec); either way one partial pair per workgroup, folded in fixed order by k_dot2_finish
  const bool vec = ctx->opt_blas1_vec && al16(x) && al16(y) && al16(z) && al16(w);
  RedLaunch L;
  MGS_TRY(red_launch(ctx, n, vec, (n + 1) / 2, &L));
  if (!vec) hipLaunchKernelGGL(update_dot2_partial_kernel, dim3(L.nb), dim3(TB), 0, ctx->stream, n, a, x, b, y, z, w, L.part);
  else if (w) hipLaunchKernelGGL(update_dot2_partial_vec_kernel<true>, dim3(L.nb), dim3(TB), 0, ctx->stream, n, a, x, b, y, z, w, L.part, L.nts);
  else hipLaunchKernelGGL(update_dot2_partial_vec_kernel<false>, dim3(L.nb), dim3(TB), 0, ctx->stream, n, a, x, b, y, z, w, L.part, L.nts);
  MGS_HIP(ctx, hipGetLastError());
  return k_dot2_finish(ctx, L.nb, L.part, out_host2);
}
// mgs_pcg, direction pass: first != 0: p ← z (p not read, x not touched); else x ← x + a·p, p ← z + beta·p
int k_pcg_direction(mgs_ctx *ctx, int64_t n, int first, double a, double beta, double *x, double *p, const double *z) {
  if (!n) return MGS_OK;
  if (ctx->opt_blas1_vec && al16(p) && al16(z) && (first || al16(x))) {
    const dim3 g(grid_vec((n + 1) / 2, ctx));
    const int nts = nts_of(ctx, n);
    if (first) hipLaunchKernelGGL(pcg_dir_vec_kernel<true>, g, dim3(TB), 0, ctx->stream, n, a, beta, x, p, z, nts);
    else hipLaunchKernelGGL(pcg_dir_vec_kernel<false>, g, dim3(TB), 0, ctx->stream, n, a, beta, x, p, z, nts);
  } else {
    const dim3 g(mgs_blas1_grid_capped(ctx, n));
    if (first) hipLaunchKernelGGL(pcg_dir_kernel<true>, g, dim3(TB), 0, ctx->stream, n, a, beta, x, p, z);
    else hipLaunchKernelGGL(pcg_dir_kernel<false>, g, dim3(TB), 0, ctx->stream, n, a, beta, x, p, z);
  }
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
// mgs_pcg, residual pass in place: r ← r − a·q, out_host2[0] = ‖r‖² (summed over the row shards), out_host2[1] = 0
int k_pcg_residual(mgs_ctx *ctx, int64_t n, double a, double *r, const double *q, double *out_host2) {
  const bool vec = ctx->opt_blas1_vec && al16(r) && al16(q);
  RedLaunch L;
  MGS_TRY(red_launch(ctx, n, vec, (n + 1) / 2, &L));
  if (vec) hipLaunchKernelGGL(pcg_resid_vec_kernel, dim3(L.nb), dim3(TB), 0, ctx->stream, n, a, r, q, L.part, L.nts);
  else hipLaunchKernelGGL(pcg_resid_kernel, dim3(L.nb), dim3(TB), 0, ctx->stream, n, a, r, q, L.part);
  MGS_HIP(ctx, hipGetLastError());
  return k_dot2_finish(ctx, L.nb, L.part, out_host2);
}
// ---- constant null space: v ← v − mean(v)
// The mean stays on the device, behind the folded results of the reductions (red_dev[DOT_BLOCKS + MGS_RED_VALS]).
constexpr int MEAN_SLOT = DOT_BLOCKS + MGS_RED_VALS;
static_assert(DOT_BLOCKS == MGS_DOT_BLOCKS && MEAN_SLOT < MGS_RED_CAP, "the mean slot lies behind the folded results, inside mgs_ctx::red_dev");
// store: v is shifted in place (else only read); nrm2_host != NULL: nrm2_host[0] = ‖v − m‖² reaches the host (k_dot2_finish), nrm2_host[1] = 0
static int project_const_impl(mgs_ctx *ctx, int64_t n, double *v, bool store, double *nrm2_host, bool nrm2_fold = false) {
  if (n <= 0) { if (nrm2_host) nrm2_host[0] = nrm2_host[1] = 0.0; return MGS_OK; }
  const bool vec = ctx->opt_blas1_vec && al16(v);
  RedLaunch L;
  MGS_TRY(red_launch(ctx, n, vec, (n + 1) / 2, &L));
  const int nb = L.nb, nts = L.nts;
  double *part = L.part, *mean = ctx->red_dev + MEAN_SLOT;
  hipStream_t s = ctx->stream;
  if (vec) hipLaunchKernelGGL(sum_partial_vec_kernel, dim3(nb), dim3(TB), 0, s, n, v, part);
  else hipLaunchKernelGGL(sum_partial_kernel, dim3(nb), dim3(TB), 0, s, n, v, part);
  const double *fold = part; int nf = nb;
  fold_mid(ctx, &nf, &fold);
  hipLaunchKernelGGL(mean_final_kernel, dim3(1), dim3(TB), 0, s, nf, fold, (double)n, mean);
  const bool nrm = nrm2_host != nullptr || nrm2_fold;
#define SHIFT_(ST, NR)                                                                                                              \
  do {                                                                                                                              \
    if (vec) hipLaunchKernelGGL((shift_const_vec_kernel<ST, NR>), dim3(nb), dim3(TB), 0, s, n, v, mean, part, nts);                  \
    else hipLaunchKernelGGL((shift_const_kernel<ST, NR>), dim3(nb), dim3(TB), 0, s, n, v, mean, part);                               \
  } while (0)
  if (store && nrm) SHIFT_(true, true); else if (store) SHIFT_(true, false); else if (nrm) SHIFT_(false, true);
#undef SHIFT_
  MGS_HIP(ctx, hipGetLastError());
  return nrm ? k_dot2_finish(ctx, nb, part, nrm2_host) : MGS_OK;
}
int k_project_const(mgs_ctx *ctx, int64_t n, double *v) { return project_const_impl(ctx, n, v, true, nullptr); }
int k_project_const_nrm2(mgs_ctx *ctx, int64_t n, double *v, double *out_host2) { return project_const_impl(ctx, n, v, true, out_host2); }
int k_const_dev_nrm2(mgs_ctx *ctx, int64_t n, const double *v, double *out_host2) { return project_const_impl(ctx, n, const_cast<double *>(v), false, out_host2); }
// the same two with the norm left on the device (red_dev[DOT_BLOCKS], see fetch_or_leave): no host round trip
int k_project_const_nrm2_fold(mgs_ctx *ctx, int64_t n, double *v) { return project_const_impl(ctx, n, v, true, nullptr, true); }
int k_const_dev_nrm2_fold(mgs_ctx *ctx, int64_t n, const double *v) { return project_const_impl(ctx, n, const_cast<double *>(v), false, nullptr, true); }
// the mean the last projection on this context subtracted (diagnostics; synchronises)
int k_project_const_mean(mgs_ctx *ctx, double *mean_host) {
  MGS_HIP(ctx, hipMemcpyAsync(mean_host, ctx->red_dev + MEAN_SLOT, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MGS_OK;
}
// ---- field-wise constant null space: v_i ← v_i − m[label_i]
// The launch decisions of project_const_impl: the 16-byte arm when v is 16-byte aligned (the labels array is the matrix's own allocation, so a
// pair's two labels are one aligned 2-byte load), the same grids, the `nt` hint under nts_of, fold_mid's chunk stage above 4096 workgroups.
// The partials ([nf][nb], then the shift pass's pair [2][nb]) live in red_dev while they fit, else in the grown scratch.
int k_project_fields(mgs_ctx *ctx, const mgs_nsfields *F, int64_t n, double *v, bool store, bool nrm, double *out_host2) {
  if (n <= 0) { if (out_host2) out_host2[0] = out_host2[1] = 0.0; return MGS_OK; }
  const int nf = F->nfields;
  const bool vec = ctx->opt_blas1_vec && al16(v);
  const int nts = nts_of(ctx, n);
  const int nb = vec ? grid_vec((n + 1) / 2, ctx) : grid_cap(n, DOT_BLOCKS / NSF);
  // sum pass with more than two fields: nf pairs per lane instead of one, so that the nf wave folds at a workgroup's end are paid once per nf pairs
  // (measured with 8 fields at 256³, tools/ab_nullspace_fields.py: profiles/r24_nullspace_fields.md)
  const int nbs = vec && nf > 2 ? (nb + nf - 1) / nf : nb;
  double *part;
  MGS_TRY(part_buf(ctx, std::max((int64_t)nf * nbs, 2 * (int64_t)nb), &part));
  hipStream_t s = ctx->stream;
  if (vec) hipLaunchKernelGGL(fields_sum_vec_kernel, dim3(nbs), dim3(TB), 0, s, n, nf, v, F->labels, part);
  else hipLaunchKernelGGL(fields_sum_kernel, dim3(nbs), dim3(TB), 0, s, n, nf, v, F->labels, part);
  const double *fold = part; int nfold = nbs;
  if (nbs > 4096) {      // (the partials are in the grown scratch then: red_dev is free for the chunk sums)
    const int groups = 256, chunk = (nbs + groups - 1) / groups;
    hipLaunchKernelGGL(fields_mid_kernel, dim3(groups, nf), dim3(TB), 0, s, nbs, chunk, part, ctx->red_dev);
    fold = ctx->red_dev; nfold = groups;
  }
  FieldCounts cnt;
  for (int k = 0; k < NSF; ++k) cnt.n[k] = k < nf ? (double)F->counts[k] : 1.0;
  hipLaunchKernelGGL(fields_mean_final_kernel, dim3(1), dim3(TB), 0, s, nfold, nf, fold, cnt, F->means);
#define SHIFT_(ST, NR)                                                                                                                  \
  do {                                                                                                                                  \
    if (vec) hipLaunchKernelGGL((fields_shift_vec_kernel<ST, NR>), dim3(nb), dim3(TB), 0, s, n, nf, v, F->labels, F->means, part, nts);  \
    else hipLaunchKernelGGL((fields_shift_kernel<ST, NR>), dim3(nb), dim3(TB), 0, s, n, nf, v, F->labels, F->means, part);               \
  } while (0)
  if (store && nrm) SHIFT_(true, true); else if (store) SHIFT_(true, false); else if (nrm) SHIFT_(false, true);
#undef SHIFT_
  MGS_HIP(ctx, hipGetLastError());
  return nrm ? k_dot2_finish(ctx, nb, part, out_host2) : MGS_OK;
}
// the one dispatch on the matrix's null-space record
int k_ns_project(const mgs_csr *A, int64_t n, double *v) {
  return A->nullspace == MGS_NULLSPACE_FIELDS ? k_project_fields(A->ctx, A->nsf, n, v, true, false, nullptr) : k_project_const(A->ctx, n, v);
}
int k_ns_project_nrm2(const mgs_csr *A, int64_t n, double *v, double *out_host2) {
  if (A->nullspace == MGS_NULLSPACE_FIELDS) return k_project_fields(A->ctx, A->nsf, n, v, true, true, out_host2);
  return out_host2 ? k_project_const_nrm2(A->ctx, n, v, out_host2) : k_project_const_nrm2_fold(A->ctx, n, v);
}
int k_ns_dev_nrm2(const mgs_csr *A, int64_t n, const double *v, double *out_host2) {
  if (A->nullspace == MGS_NULLSPACE_FIELDS) return k_project_fields(A->ctx, A->nsf, n, const_cast<double *>(v), false, true, out_host2);
  return out_host2 ? k_const_dev_nrm2(A->ctx, n, v, out_host2) : k_const_dev_nrm2_fold(A->ctx, n, v);
}
// workgroups of a multi-vector reduction pass: one-shot at small sizes, a few elements per lane at large ones (partials stay short)
static int mdot_grid(int64_t n) {
  int64_t nb = (n / 2 + (int64_t)TB * 4 - 1) / ((int64_t)TB * 4);
  return (int)std::min<int64_t>(std::max<int64_t>(nb, 1), 2048);
}
// s_k = a·b_k, k < K ≤ MDOT_MAX: to device scalars (out_dev) and/or, summed over the ranks, to the host (out_host)
int k_mdot(mgs_ctx *ctx, int64_t n, int K, const double *a, const double *const *b, double *out_dev, double *out_host) {
  MGS_CHECK(ctx, K >= 1 && K <= MDOT_MAX && K <= MGS_RED_VALS, MGS_ERR_INVALID, "k_mdot: %d inner products (at most %d)", K, MDOT_MAX);
  MDotVecs B;
  bool aligned = al16(a);
  for (int k = 0; k < MDOT_MAX; ++k) { B.b[k] = k < K ? b[k] : a; if (k < K && !al16(b[k])) aligned = false; }
  const int nb = mdot_grid(n);
  double *part;        // (the K-cycle's pairs always fit the context's own scratch: nothing is allocated inside a captured cycle)
  MGS_TRY(part_buf(ctx, (int64_t)K * nb, &part));
  double *res = out_dev ? out_dev : ctx->red_dev + DOT_BLOCKS;
  if (!aligned) {      // operands that do not start on 16 bytes (views into the middle of a vector): K two-vector reductions
    for (int k = 0; k < K; ++k) MGS_TRY(k_dot_dev(ctx, n, a, b[k], res + k));
    if (!out_host) return MGS_OK;
    if (ctx->ncomm) {
      if (res != ctx->red_dev + DOT_BLOCKS) MGS_HIP(ctx, hipMemcpyAsync(ctx->red_dev + DOT_BLOCKS, res, sizeof(double) * (size_t)K, hipMemcpyDeviceToDevice, ctx->stream));
      MGS_TRY(mgs_comm_allreduce_sum(ctx->ncomm, ctx->red_dev + DOT_BLOCKS, (size_t)K));
      res = ctx->red_dev + DOT_BLOCKS;
    }
    MGS_HIP(ctx, hipMemcpyAsync(ctx->red_host, res, sizeof(double) * (size_t)K, hipMemcpyDeviceToHost, ctx->stream));
    MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < K; ++k) out_host[k] = ctx->red_host[k];
    if (ctx->allreduce && !ctx->ncomm && ctx->allreduce(ctx->allreduce_user, out_host, K)) return mgs_fail(ctx, MGS_ERR_STATE, "allreduce callback failed");
    return MGS_OK;
  }
  hipLaunchKernelGGL(mdot_partial_kernel, dim3(nb), dim3(TB), 0, ctx->stream, n, K, a, B, part);
  const Post pa = out_host ? begin_post(ctx) : NO_POST;
  hipLaunchKernelGGL(mdot_final_kernel, dim3(1), dim3(TB), 0, ctx->stream, nb, K, part, res, pa);
  MGS_HIP(ctx, hipGetLastError());
  if (!out_host) return MGS_OK;
  if (res != ctx->red_dev + DOT_BLOCKS) MGS_HIP(ctx, hipMemcpyAsync(ctx->red_dev + DOT_BLOCKS, res, sizeof(double) * (size_t)K, hipMemcpyDeviceToDevice, ctx->stream));   // where fetch_results looks
  if (ctx->ncomm) MGS_TRY(mgs_comm_allreduce_sum(ctx->ncomm, ctx->red_dev + DOT_BLOCKS, (size_t)K));
  return fetch_results(ctx, K, out_host, pa);
}
// z = x − Σ_{j<K} coef_j·w_j with (z·u2 — or z·z when u2 is NULL —, z·u) to the host in the same pass (out_host2 = NULL: no sums, no round trip)
int k_maxpy_dot2(mgs_ctx *ctx, int64_t n, int K, const double *x, const double *const *w, const double *coef, double *z, const double *u, const double *u2, double *out_host2) {
  MGS_CHECK(ctx, K >= 0 && K <= MDOT_MAX, MGS_ERR_INVALID, "k_maxpy_dot2: %d terms (at most %d)", K, MDOT_MAX);
  MAxpyArgs W;
  for (int k = 0; k < MDOT_MAX; ++k) { W.w[k] = k < K ? w[k] : x; W.coef[k] = k < K ? coef[k] : 0.0; }
  bool vec = n >= 2 && al16(x) && al16(z) && (!u || al16(u)) && (!u2 || al16(u2));
  for (int k = 0; k < K; ++k) vec = vec && al16(w[k]);
  int64_t nbl = (n + (int64_t)TB * 4 - 1) / ((int64_t)TB * 4);       // two 16-byte (or four 8-byte) elements per lane
  const int nb = (int)std::min<int64_t>(std::max<int64_t>(nbl, 1), 1 << 20);
  double *part = nullptr;
  if (out_host2) MGS_TRY(part_buf(ctx, 2 * (int64_t)nb, &part));
  if (vec) hipLaunchKernelGGL(maxpy_dot2_kernel<true>, dim3(nb), dim3(TB), 0, ctx->stream, n, K, x, W, z, u, u2, part);
  else hipLaunchKernelGGL(maxpy_dot2_kernel<false>, dim3(nb), dim3(TB), 0, ctx->stream, n, K, x, W, z, u, u2, part);
  MGS_HIP(ctx, hipGetLastError());
  return out_host2 ? k_dot2_finish(ctx, nb, part, out_host2) : MGS_OK;
}
// scal[3] = ρ2, scal[4] = α2 of the explicitly orthogonalised second direction (see kc_orth_dots_kernel); at most DOT_BLOCKS / 2 partial pairs
int k_kc_orth_dots(mgs_ctx *ctx, int n, bool energy, double *scal, const double *c1, const double *c2, const double *v1, const double *v2, const double *rp) {
  const int nb = std::max(1, std::min(mgs_grid(n, TB * 4), DOT_BLOCKS / 2));
  if (energy) hipLaunchKernelGGL(kc_orth_dots_kernel<true>, dim3(nb), dim3(TB), 0, ctx->stream, n, scal, c1, c2, v1, v2, rp, ctx->red_dev);
  else hipLaunchKernelGGL(kc_orth_dots_kernel<false>, dim3(nb), dim3(TB), 0, ctx->stream, n, scal, c1, c2, v1, v2, rp, ctx->red_dev);
  return dot2_fold_into(ctx, nb, ctx->red_dev, scal + 3, NO_POST);
}
