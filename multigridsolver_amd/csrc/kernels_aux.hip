// kernels_aux.hip — grid transfer (restriction / prolongation), setup-time operand preparation, the K-cycle's two elementwise
// kernels, coarsest dense solve, on-device operator generators, tail scatter.  gfx950 only.  BLAS-1 and reductions: blas1.hip.
#include "mgs_internal.hpp"

#include <cfloat>

namespace {
constexpr int TB = 256;

// ------------------------------------------------------------------ diag / elementwise
// dinv_i = 1/a_ii (reference src/CPU_Matlab/solve.m:17).  Binary search in the sorted row,
// as src/GPU_CUDAC++/MatrixAccess.cu:28-47 does for element access.
__global__ void diag_inv_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                const double *__restrict__ val, double *__restrict__ dinv, int *__restrict__ bad) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int lo = rowptr[i], hi = rowptr[i + 1] - 1;
  double d = 0.0;
  while (lo <= hi) {
    int mid = lo + ((hi - lo) >> 1);   // lo + hi would overflow int32 near 2^31 entries
    int c = col[mid];
    if (c == i) { d = val[mid]; break; }
    if (c < i) lo = mid + 1; else hi = mid - 1;
  }
  if (d == 0.0) { atomicAdd(bad, 1); dinv[i] = 0.0; }
  else dinv[i] = 1.0 / d;
}

__global__ void fill_kernel(double *__restrict__ d, int64_t n, double v) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) d[i] = v;
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__global__ void rand_kernel(double *__restrict__ d, int64_t n, uint64_t seed, int64_t off) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint64_t h = splitmix64(seed * 0xD1342543DE82EF95ull + (uint64_t)(i + off));
    d[i] = (double)(h >> 11) * (1.0 / 9007199254740992.0);
  }
}

// first damped-Jacobi sweep from x = 0: x = 0 + (ωD⁻¹)(b − A·0) = (ω·dinv_i)·b_i, bit-identical
__global__ void jacobi_zero_kernel(int n, double omega, const double *__restrict__ dinv, const double *__restrict__ b, double *__restrict__ x) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = (omega * dinv[i]) * b[i];
}

// ------------------------------------------------------------------ grid transfer
// r_c = Pᵀ r for an aggregation P (unit values are not loaded): `Ptrans * vec`,
// reference bicg.cpp:48.  One lane per aggregate, members summed in ascending fine-row
// order == Eigen's row-major SpMV order with values 1.0 → bit-identical.
__global__ void restrict_agg_kernel(int nc, const int *__restrict__ cptr, const int *__restrict__ members,
                                    const double *__restrict__ r, double *__restrict__ rc) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  // aggregates of the pairwise passes hold at most 4 members: the first four member indices, then their four residuals, are loaded
  // together (predicated, no loop: a loop drains every outstanding load at its header, and member → residual is a dependent pair,
  // i.e. eight serialized memory latencies per lane in the looped form); the sum keeps the ascending order.  Longer lists continue in a loop.
  const int k0 = cptr[c], e = cptr[c + 1];
  int m[4]; double v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) m[q] = k0 + q < e ? members[k0 + q] : -1;
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = m[q] >= 0 ? r[m[q]] : 0.0;
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) if (k0 + q < e) s += v[q];
  for (int k = k0 + 4; k < e; ++k) s += r[members[k]];
  rc[c] = s;
}
// Small levels (launch-bound, a few µs per dispatch whatever they do): the zero-guess pre pass r = b − Â·b and the restriction
// r_c = Pᵀr in ONE kernel, aggregate-parallel — four lanes per aggregate, lane q walks the row of member q (plain CSR of Â, ascending
// columns, unfused multiply/add from 0.0: the row-block kernel's arithmetic), stores r for the post pass, and lane 0 adds the members'
// residuals in ascending member order (restrict_agg_kernel's order): same bits as the two kernels it replaces, one dispatch less per
// level.  Rows outside every aggregate (G0) get their residual from the tail of the grid.  hv: halo payload of a row shard (NULL: none).
// VT = float: valhat holds the values rounded to FP32 (operand precision of the level); widened before the product, sums in FP64.
template <class VT>
__global__ __launch_bounds__(TB) void agg_pre_kernel(int n, int nc, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                      const VT *__restrict__ valhat, const double *__restrict__ b, const double *__restrict__ hv,
                                                      const int *__restrict__ cptr, const int *__restrict__ members, const int *__restrict__ agg,
                                                      double *__restrict__ r_out, double *__restrict__ rc_out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  auto row_residual = [&](int m) -> double {
    // eight entries per step, every load of a step issued before the first is waited for (a loop over single entries drains its
    // loads at every header: two serialized memory latencies per ENTRY); the sum itself stays sequential in ascending column order
    double s = 0.0;
    const int e0 = rowptr[m], ee = rowptr[m + 1];
    const double bm = b[m];
    for (int e = e0; e < ee; e += 8) {
      int c[8]; double v[8], xv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) c[q] = e + q < ee ? col[e + q] : -1;
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = e + q < ee ? (double)valhat[e + q] : 0.0;
#pragma unroll
      for (int q = 0; q < 8; ++q) xv[q] = c[q] < 0 ? 0.0 : (c[q] < n ? b[c[q]] : hv[c[q] - n]);
#pragma unroll
      for (int q = 0; q < 8; ++q) if (e + q < ee) s += v[q] * xv[q];
    }
    return bm - s;
  };
  const int a = t >> 2, q = t & 3;
  if (a < nc) {                                   // the four lanes of a group share a: same trip counts, converged shuffles
    const int k0 = cptr[a], ke = cptr[a + 1];
    double acc = 0.0;
    for (int kb = k0; kb < ke; kb += 4) {         // one round for the aggregates of the pairwise passes (≤ 4 members)
      double rm = 0.0;
      if (kb + q < ke) { const int m = members[kb + q]; rm = row_residual(m); r_out[m] = rm; }
#pragma unroll
      for (int j = 0; j < 4; ++j) { const double v = __shfl(rm, j, 4); if (kb + j < ke) acc += v; }
    }
    if (q == 0) rc_out[a] = acc;
  } else {
    const int row = t - 4 * nc;
    if (row < n && agg[row] < 0) r_out[row] = row_residual(row);
  }
}
// e = P e_c / x += P e_c: `P * (...)`, reference bicg.cpp:48; P has ≤1 unit entry per row
// (src/CPU_C++/AGMG.cpp:181-186) so e_i = e_c[agg(i)] or 0 for G0 rows.
template <int ADD>
__global__ void prolong_agg_kernel(int n, const int *__restrict__ agg, const double *__restrict__ ec, double *__restrict__ x) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int a = agg[i];
  double e = a >= 0 ? ec[a] : 0.0;
  if (ADD) x[i] += e; else x[i] = e;
}

__global__ void gather_kernel(const double *__restrict__ x, const int *__restrict__ idx, int64_t n, double *__restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = x[idx[i]];
}

// setup-time operands of the fused cycle passes (unsharded levels): scaled values and aggregate-mapped columns
// position of the diagonal entry inside its row (0..254; 255 = absent or further in): the t-form post pass reads a_ii from there
__global__ void diag_pos_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col, unsigned char *__restrict__ dpos) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int a = rowptr[i];
  int lo = a, hi = rowptr[i + 1] - 1, pos = 255;
  while (lo <= hi) {
    int mid = lo + ((hi - lo) >> 1);
    int c = col[mid];
    if (c == i) { pos = mid - a < 255 ? mid - a : 255; break; }
    if (c < i) lo = mid + 1; else hi = mid - 1;
  }
  dpos[i] = (unsigned char)pos;
}
// out_k = a_k·wd[col_k], one lane per ENTRY (the rows play no part: coalesced streams of val, col and out, one gather).
// Row shards: wd's halo part holds the owners' ω/a_jj (fetched once at setup), so a halo column is scaled like an owned one and
// the pre pass's payload is the peers' raw right-hand side.
__global__ void scale_vals_kernel(int64_t nnz, const int *__restrict__ col, const double *__restrict__ val, const double *__restrict__ wd, double *__restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < nnz) out[k] = val[k] * wd[col[k]];
}
// Compact operand of the grouped pre pass (option pre_nodiag): Â's values in storage order without each row's diagonal entry.  Every row
// holds exactly one (diag_count_kernel), so row i's remaining entries start at rowptr[i] − i.  The diagonal entry itself is ω up to a few
// units of the last place; code[i] keeps its distance from omega, counted on the bit patterns (consecutive doubles of one sign are consecutive
// integers), so that the kernel rebuilds the stored entry exactly.  Rows whose entry lies further away than a byte holds are counted in *bad.
__global__ void diag_count_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col, int *__restrict__ bad) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int cnt = 0;
  for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) cnt += col[k] == i;
  if (cnt != 1) atomicAdd(bad, 1);
}
__global__ void drop_diag_vals_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val, double omega,
                                      double *__restrict__ out, signed char *__restrict__ code, int *__restrict__ bad) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int a = rowptr[i], e = rowptr[i + 1];
  int o = a - i;
  long long d = 0;
  for (int k = a; k < e; ++k) {
    if (col[k] != i) out[o++] = val[k];
    else d = (long long)((unsigned long long)__double_as_longlong(val[k]) - (unsigned long long)__double_as_longlong(omega));
  }
  if (d < -127 || d > 127) { atomicAdd(bad, 1); d = 0; }
  code[i] = (signed char)d;
}
// Packed copy of an FP64 operand of the fused passes (option pack7): 7 bytes per entry, the same bits.  Row block blk owns the
// entries [blkptr[blk] − s(blk), blkptr[blk + 1] − s(blk + 1)) of src, s(q) = 0 for an operand in CSR storage order and min(q·256, nd_rows) for
// the operand without diagonal entries (nd_rows ≥ 0: its row i starts at rowptr[i] − i).  Pass 1: one workgroup per row block finds the block's
// smallest biased exponent E0; e0[blk] = E0 if every entry is a normal number with exponent in [E0, E0 + 7], −1 otherwise (zero, denormal, Inf,
// NaN, 8 binades or more, or no entry at all: such a block keeps reading src).  Pass 2: entry k goes into the 112-byte record k / 16 — sixteen
// low dwords, sixteen 16-bit words (mantissa bits 32–47), sixteen bytes sign << 7 | (exponent − E0) << 4 | mantissa bits 48–51 — coded against
// the E0 of the block that owns it (a record may straddle two blocks; a kernel decodes only its own block's entries).
__device__ __forceinline__ void pack7_slice(const int *__restrict__ blkptr, int blk, int nd_rows, int &a, int &b) {
  a = blkptr[blk]; b = blkptr[blk + 1];
  if (nd_rows >= 0) { a -= min(blk * MGS_RB, nd_rows); b -= min((blk + 1) * MGS_RB, nd_rows); }
}
__global__ __launch_bounds__(MGS_RB) void pack7_scan_kernel(const int *__restrict__ blkptr, int nd_rows, const double *__restrict__ src, int *__restrict__ e0) {
  __shared__ int s_min, s_max;
  const int blk = blockIdx.x, tid = threadIdx.x;
  int a, b;
  pack7_slice(blkptr, blk, nd_rows, a, b);
  if (tid == 0) { s_min = 0x7fffffff; s_max = -1; }
  __syncthreads();
  int mn = 0x7fffffff, mx = -1;
  for (int k = a + tid; k < b; k += MGS_RB) {
    const int ex = (int)((unsigned long long)__double_as_longlong(src[k]) >> 52) & 0x7ff;
    mn = min(mn, ex); mx = max(mx, ex);
  }
  if (mx >= 0) { atomicMin(&s_min, mn); atomicMax(&s_max, mx); }
  __syncthreads();
  // exponent 0: zero or denormal, 2047: Inf or NaN
  if (tid == 0) e0[blk] = (s_max >= 0 && s_min >= 1 && s_max <= 2046 && s_max - s_min <= 7) ? s_min : -1;
}
__global__ __launch_bounds__(MGS_RB) void pack7_fill_kernel(const int *__restrict__ blkptr, int nd_rows, const double *__restrict__ src, const int *__restrict__ e0,
                                                             unsigned char *__restrict__ out) {
  const int blk = blockIdx.x, tid = threadIdx.x;
  int a, b;
  pack7_slice(blkptr, blk, nd_rows, a, b);
  const int E0 = e0[blk];
  for (int k = a + tid; k < b; k += MGS_RB) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(src[k]);
    const unsigned hi = (unsigned)(bits >> 32);
    const int d = E0 >= 0 ? (int)((hi >> 20) & 0x7ffu) - E0 : 0;      // a block that is not packed: its bytes are never decoded
    unsigned char *rec = out + (size_t)112 * (size_t)(k >> 4);
    const int i = k & 15;
    reinterpret_cast<unsigned *>(rec)[i] = (unsigned)bits;
    reinterpret_cast<unsigned short *>(rec + 64)[i] = (unsigned short)(hi & 0xffffu);
    rec[96 + i] = (unsigned char)(((hi >> 31) << 7) | ((unsigned)(d & 7) << 4) | ((hi >> 16) & 15u));
  }
}
__global__ void map_cols_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col, const int *__restrict__ cmap, int *__restrict__ out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) out[k] = cmap[col[k]];
}
__global__ void concat_i32_kernel(const int *__restrict__ a, int na, const int *__restrict__ b, int nb, int *__restrict__ out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < na) out[i] = a[i]; else if (i < na + nb) out[i] = b[i - na];
}

// |v_i| in place (mgs_csr_nullspace_defect: |A| of a private copy)
__global__ void abs_vals_kernel(int64_t n, double *__restrict__ v) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) v[i] = fabs(v[i]);
}

// ------------------------------------------------------------------ K-cycle helpers (device-resident scalars)
// Two Krylov steps on the coarse problem (Notay, SISC 34 (2012), K-cycle; docs/AGMG_For_Convection_Diffusion.pdf §3.1) with the second
// direction orthogonalised EXPLICITLY: scal = {ρ1 = d1·v1, α1 = d1·r, γ = d2·v1, ρ2 = d2'·v2', α2 = d2'·r'} with g = γ/ρ1,
// c2' = c2 − g·c1, v2' = v2 − g·v1 and d = v (GCR form) or d = c (energy form).  ρ2 is a sum of products of the orthogonalised vectors,
// not the difference β − γ²/ρ1 of two nearly equal numbers (round 3: lost up to five digits where c2 is almost parallel to c1).
// No host round trip, graph-capturable.  The two elementwise kernels are here; the pair (ρ2, α2) is a reduction: kc_orth_dots_kernel, blas1.hip.
__global__ void kc_update_r_kernel(int n, const double *__restrict__ scal, const double *__restrict__ r, const double *__restrict__ v1, double *__restrict__ rp) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double rho1 = scal[0], a = rho1 != 0.0 ? scal[1] / rho1 : 0.0;
  rp[i] = r[i] - a * v1[i];
}
// x = (α1/ρ1)·c1 + (α2/ρ2)·(c2 − g·c1)
__global__ void kc_combine_kernel(int n, const double *__restrict__ scal, const double *__restrict__ c1, const double *__restrict__ c2, double *__restrict__ x) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double rho1 = scal[0], alpha1 = scal[1], gamma = scal[2], rho2 = scal[3], alpha2 = scal[4];
  double k1 = 0.0, k2 = 0.0;
  if (rho1 != 0.0) {
    k1 = alpha1 / rho1;
    if (rho2 > 0.0) { k2 = alpha2 / rho2; k1 -= (gamma / rho1) * k2; }
  }
  x[i] = k1 * c1[i] + k2 * c2[i];
}

// ------------------------------------------------------------------ coarsest level: dense
// x = A⁻¹ b with the explicit inverse (stands in for SparseLU::solve, reference bicg.cpp:48).
// One wavefront per row, lanes stride the columns (coalesced), shuffle reduction.
__global__ __launch_bounds__(TB) void dense_gemv_kernel(int n, const double *__restrict__ M, const double *__restrict__ b, double *__restrict__ x) {
  int row = blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (row >= n) return;
  const double *m = M + (size_t)row * n;
  double s = 0.0;
  for (int j = lane; j < n; j += 64) s += m[j] * b[j];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
  if (lane == 0) x[row] = s;
}

// Gauss-Jordan inversion with partial pivoting on the augmented matrix [A | I] (n × 2n).
__global__ void dense_scatter_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val, double *__restrict__ W) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double *w = W + (size_t)i * 2 * n;
  for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) w[col[k]] += val[k];
  w[n + i] = 1.0;
}
// max |a_ij| of the operator, as the bits of a non-negative double (they order like unsigned integers; a NaN sorts above +Inf and so wins):
// the scale of the singularity test in gj_pivot_kernel
__global__ __launch_bounds__(TB) void dense_absmax_kernel(int64_t nnz, const double *__restrict__ val, unsigned long long *__restrict__ amax_bits) {
  unsigned long long m = 0ull;
  const int64_t stride = (int64_t)gridDim.x * TB;
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < nnz; i += stride) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(val[i]));
    m = b > m ? b : m;
  }
  for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_down(m, off); m = o > m ? o : m; }
  if ((threadIdx.x & 63) == 0) atomicMax(amax_bits, m);      // one atomic per wavefront
}
// Constant null space (mgs_csr_set_nullspace): A_c + (s/n)·1·1ᵀ with s = max|a_ij| as dense_absmax_kernel left it on the device — added to the left
// half of W between the scatter and the elimination.  For a symmetric semidefinite A_c with null vector 1 the inverse is A_c⁺ + (1/s)·1·1ᵀ/n.
__global__ void dense_reg_const_kernel(int n, double *__restrict__ W, const unsigned long long *__restrict__ amax_bits) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  int i = blockIdx.y;
  if (j < n) W[(size_t)i * 2 * n + j] += __longlong_as_double((long long)amax_bits[0]) / (double)n;
}
// Field-wise constant null space (mgs_csr_set_nullspace_fields): A_c + Σ_f (s/n_f)·z_f·z_fᵀ — s/n_f is added where row and column carry the same
// label f >= 0 (lab: the coarsest level's labels, cnt: its rows per field).  For a symmetric A_c whose null space is span{z_f} the inverse is
// A_c⁺ + Σ_f (1/s)·z_f·z_fᵀ/n_f: exactly A_c⁺·b on a right-hand side orthogonal to every z_f.
struct DenseFieldCounts { double n[MGS_NULLSPACE_MAX_FIELDS]; };
__global__ void dense_reg_fields_kernel(int n, double *__restrict__ W, const unsigned long long *__restrict__ amax_bits, const signed char *__restrict__ lab, const DenseFieldCounts cnt) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  int i = blockIdx.y;
  if (j >= n) return;
  const int li = lab[i], lj = lab[j];
  if (li < 0 || li != lj) return;
  double nf = 1.0;
#pragma unroll
  for (int k = 0; k < MGS_NULLSPACE_MAX_FIELDS; ++k) if (li == k) nf = cnt.n[k];
  W[(size_t)i * 2 * n + j] += __longlong_as_double((long long)amax_bits[0]) / nf;
}
// Coarse labels of a level under a field-wise null space, and the two checks that make the coarse indicators P-images of the fine ones: fine row i
// with aggregate a compares its label with that of a's first member (which writes the aggregate's label); a labelled row outside every
// aggregate is refused.  bad: min over (row << 1 | kind) — the lowest offending fine row, deterministic.
__global__ void coarse_labels_kernel(int n, const int *__restrict__ agg, const int *__restrict__ cptr, const int *__restrict__ members, const signed char *__restrict__ lab,
                                     signed char *__restrict__ clab, unsigned long long *__restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int a = agg[i], l = lab[i];
  if (a < 0) { if (l >= 0) atomicMin(bad, ((unsigned long long)i << 1) | 1ull); return; }
  const int first = members[cptr[a]];
  if (i == first) clab[a] = (signed char)l;
  else if (lab[first] != l) atomicMin(bad, (unsigned long long)i << 1);
}
// z_f as a vector: 1.0 where the row carries label f, 0.0 elsewhere (mgs_csr_nullspace_defect on a fields matrix)
__global__ void label_indicator_kernel(int n, const signed char *__restrict__ lab, int f, double *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = lab[i] == f ? 1.0 : 0.0;
}
// Singularity rule: the operator is refused (piv[1] = 1) when a pivot is not greater than GJ_SINGULAR_FACTOR·n·DBL_EPSILON·max|a_ij|.
// Written as !(|pivot| > threshold) so that a NaN pivot and a NaN or Inf scale are refused as well.  Basis of the constant (NumPy model
// of this algorithm, FP64): singular weighted graph Laplacians of n = 4..500 end with a pivot <= 0.31·n·eps·max|a|; regular matrices of
// cond 1e12 keep every pivot >= 4.8e3·n·eps·max|a|, cond 1e10 >= 5.9e5, the Dirichlet Laplacian >= 5e12.  8 sits 25x above the first
// group and 600x below the second.
constexpr double GJ_SINGULAR_FACTOR = 8.0;
__global__ __launch_bounds__(TB) void gj_pivot_kernel(int n, int k, const double *__restrict__ W, int *__restrict__ piv, double *__restrict__ pivval,
                                                      const unsigned long long *__restrict__ amax_bits) {
  __shared__ double bv[TB]; __shared__ int bi[TB];
  double best = -1.0; int idx = k;
  for (int i = k + threadIdx.x; i < n; i += TB) {
    double v = fabs(W[(size_t)i * 2 * n + k]);
    if (v > best) { best = v; idx = i; }
  }
  bv[threadIdx.x] = best; bi[threadIdx.x] = idx;
  __syncthreads();
  for (int w = TB / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
      double o = bv[threadIdx.x + w]; int oi = bi[threadIdx.x + w];
      if (o > bv[threadIdx.x] || (o == bv[threadIdx.x] && oi < bi[threadIdx.x])) { bv[threadIdx.x] = o; bi[threadIdx.x] = oi; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double thr = GJ_SINGULAR_FACTOR * (double)n * DBL_EPSILON * __longlong_as_double((long long)amax_bits[0]);
    piv[0] = bi[0]; if (!(bv[0] > thr)) piv[1] = 1; pivval[0] = W[(size_t)bi[0] * 2 * n + k];
  }
}
__global__ void gj_swap_scale_kernel(int n, int k, double *__restrict__ W, const int *__restrict__ piv, const double *__restrict__ pivval) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  int p = piv[0];
  if (j < 2 * n) {
    double a = W[(size_t)k * 2 * n + j], b = W[(size_t)p * 2 * n + j];
    double d = pivval[0];
    if (d == 0.0) d = 1.0;
    W[(size_t)p * 2 * n + j] = a;       // (p == k: a == b, harmless)
    W[(size_t)k * 2 * n + j] = b / d;
  }
}
__global__ void gj_colsave_kernel(int n, int k, const double *__restrict__ W, double *__restrict__ colk) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) colk[i] = (i == k) ? 0.0 : W[(size_t)i * 2 * n + k];
}
__global__ void gj_eliminate_kernel(int n, int k, double *__restrict__ W, const double *__restrict__ colk) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  int i = blockIdx.y;
  if (j >= 2 * n) return;
  double f = colk[i];
  if (f != 0.0) W[(size_t)i * 2 * n + j] -= f * W[(size_t)k * 2 * n + j];
}
__global__ void gj_extract_kernel(int n, const double *__restrict__ W, double *__restrict__ inv) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  int i = blockIdx.y;
  if (j < n) inv[(size_t)i * n + j] = W[(size_t)i * 2 * n + n + j];
}

// ------------------------------------------------------------------ generators
// 7-point 3-D Poisson, SURVEY §8d row d2 (3-D extension of reference src/common/poisson.cpp:11-33).
// closed-form rowptr: entries before row e = 7e − (#missing neighbours in rows < e)
__device__ __forceinline__ int64_t p3_rowptr(int N, int64_t e) {
  const int64_t N2 = (int64_t)N * N;
  if (e >= N2 * N) return 7 * N2 * N - 6 * N2;
  int i = (int)(e / N2); int rem = (int)(e - (int64_t)i * N2); int j = rem / N; int k = rem - j * N;
  // missing i−: rows with i==0 before e; missing i+: rows with i==N-1 before e
  int64_t miss = 0;
  miss += (i > 0) ? N2 : rem;                     // i == 0 rows
  miss += (i == N - 1) ? rem : 0;                 // i == N-1 rows
  // j == 0 rows before e: per full plane N, in current plane: (j>0 ? N : k)
  miss += (int64_t)i * N + ((j > 0) ? N : k);
  miss += (int64_t)i * N + ((j == N - 1) ? k : 0);   // j == N-1 rows
  // k == 0 rows before e: one per line
  int64_t lines = (int64_t)i * N + j;
  miss += lines + (k > 0 ? 1 : 0);
  miss += lines;                                      // k == N-1 rows of complete lines
  return 7 * e - miss;
}
__global__ void poisson3d_kernel(int N, int plane_lo, int64_t n_loc, int local_cols, int has_lo, int has_hi,
                                 int *__restrict__ rowptr, int *__restrict__ col, double *__restrict__ val) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t > n_loc) return;
  const int64_t N2 = (int64_t)N * N;
  const int64_t e0 = (int64_t)plane_lo * N2;
  const int64_t base = p3_rowptr(N, e0);
  const int64_t e = e0 + t;
  const int64_t p0 = p3_rowptr(N, e) - base;
  rowptr[t] = (int)p0;
  if (t == n_loc) return;
  int i = (int)(e / N2); int rem = (int)(e - (int64_t)i * N2); int j = rem / N; int k = rem - j * N;
  int64_t p = p0;
  // local numbering: owned rows [0,n_loc), lower halo plane [n_loc, n_loc+N2), upper after it
  const int64_t lo_halo = n_loc, hi_halo = n_loc + (has_lo ? N2 : 0);
  auto cidx = [&](int64_t g) -> int {
    if (!local_cols) return (int)g;
    int64_t l = g - e0;
    if (l < 0) return (int)(lo_halo + (l + N2));
    if (l >= n_loc) return (int)(hi_halo + (l - n_loc));
    return (int)l;
  };
  // rows stay sorted by (local) column: with local numbering the halo columns are the largest,
  // so an off-shard e−N² / e+N² neighbour moves to the end of the row
  const bool lo_is_halo = local_cols && i > 0 && i == plane_lo;
  const bool hi_is_halo = local_cols && i < N - 1 && (e + N2 - e0) >= n_loc;
  if (i > 0 && !lo_is_halo)     { col[p] = cidx(e - N2); val[p++] = -1.0; }
  if (j > 0)     { col[p] = cidx(e - N);  val[p++] = -1.0; }
  if (k > 0)     { col[p] = cidx(e - 1);  val[p++] = -1.0; }
  col[p] = cidx(e); val[p++] = 6.0;
  if (k < N - 1) { col[p] = cidx(e + 1);  val[p++] = -1.0; }
  if (j < N - 1) { col[p] = cidx(e + N);  val[p++] = -1.0; }
  if (i < N - 1 && !hi_is_halo) { col[p] = cidx(e + N2); val[p++] = -1.0; }
  if (lo_is_halo) { col[p] = cidx(e - N2); val[p++] = -1.0; }
  if (hi_is_halo) { col[p] = cidx(e + N2); val[p++] = -1.0; }
}
// 2-D 5-point, exactly reference src/common/poisson.cpp:9-37.
__global__ void poisson2d_kernel(int n, int *__restrict__ rowptr, int *__restrict__ col, double *__restrict__ val) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  int N = n * n;
  if (e > N) return;
  auto rp = [&](int r) -> int {
    if (r >= N) return 5 * N - 4 * n;
    int i = r / n, j = r % n;
    // missing: i==0 rows, i==n-1 rows, j==0 rows, j==n-1 rows before r
    int miss = (i > 0 ? n : j) + (i == n - 1 ? j : 0) + (i + (j > 0 ? 1 : 0)) + i;
    return 5 * r - miss;
  };
  int p = rp(e);
  rowptr[e] = p;
  if (e == N) return;
  int i = e / n, j = e % n;
  if (i > 0)     { col[p] = e - n; val[p++] = -1.0; }
  if (j > 0)     { col[p] = e - 1; val[p++] = -1.0; }
  col[p] = e; val[p++] = 4.0;
  if (j < n - 1) { col[p] = e + 1; val[p++] = -1.0; }
  if (i < n - 1) { col[p] = e + n; val[p++] = -1.0; }
}

}  // namespace

// ============================================================ host launchers
int k_diag_inv(const mgs_csr *A, double *dinv, int *bad_count_host) {
  mgs_ctx *ctx = A->ctx;
  int *bad = nullptr;
  MGS_TRY(mgs_dev_alloc(ctx, &bad, 1));
  MGS_HIP(ctx, hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
  if (A->rows)
    hipLaunchKernelGGL(diag_inv_kernel, dim3(mgs_grid(A->rows, TB)), dim3(TB), 0, ctx->stream, A->rows, A->rowptr, A->col, A->val, dinv, bad);
  MGS_HIP(ctx, hipMemcpyAsync(bad_count_host, bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  MGS_HIP(ctx, mgs_hip_free(bad));
  return MGS_OK;
}

// the same kernel without the host round trip (mgs_hier_refresh): the count of bad rows is ADDED to *bad_dev, which the caller reads later
int k_diag_inv_async(const mgs_csr *A, double *dinv, int *bad_dev) {
  mgs_ctx *ctx = A->ctx;
  if (A->rows)
    hipLaunchKernelGGL(diag_inv_kernel, dim3(mgs_grid(A->rows, TB)), dim3(TB), 0, ctx->stream, A->rows, A->rowptr, A->col, A->val, dinv, bad_dev);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

int k_diag_pos(const mgs_csr *A, unsigned char *dpos) {
  mgs_ctx *ctx = A->ctx;
  if (A->rows) hipLaunchKernelGGL(diag_pos_kernel, dim3(mgs_grid(A->rows, TB)), dim3(TB), 0, ctx->stream, A->rows, A->rowptr, A->col, dpos);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_agg_pre(const mgs_csr *A, const double *valhat, const double *b, const double *hv, const mgs_xfer *T, double *r_out, double *rc_out,
              const float *valhat32) {
  mgs_ctx *ctx = A->ctx;
  const int64_t threads = 4 * (int64_t)T->n_coarse + (T->nnz < (int64_t)A->rows ? A->rows : 0);   // rows outside every aggregate only where there are any
  if (threads && valhat32)
    hipLaunchKernelGGL(agg_pre_kernel<float>, dim3(mgs_grid(threads, TB)), dim3(TB), 0, ctx->stream, A->rows, T->n_coarse, A->rowptr, A->col, valhat32, b, hv,
                       T->cptr, T->members, T->agg, r_out, rc_out);
  else if (threads)
    hipLaunchKernelGGL(agg_pre_kernel<double>, dim3(mgs_grid(threads, TB)), dim3(TB), 0, ctx->stream, A->rows, T->n_coarse, A->rowptr, A->col, valhat, b, hv,
                       T->cptr, T->members, T->agg, r_out, rc_out);
  report_launch(ctx, 5, 8, 0, 0, 0, valhat32 ? 1 : 0);      // aggregate-parallel: steps of 8 entries, no LDS
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_restrict_agg(mgs_ctx *ctx, int nc, const int *cptr, const int *members, const double *r, double *rc) {
  if (nc) hipLaunchKernelGGL(restrict_agg_kernel, dim3(mgs_grid(nc, TB)), dim3(TB), 0, ctx->stream, nc, cptr, members, r, rc);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_prolong_agg(mgs_ctx *ctx, int n, const int *agg, const double *ec, double *x, int add) {
  if (n) {
    if (add) hipLaunchKernelGGL(prolong_agg_kernel<1>, dim3(mgs_grid(n, TB)), dim3(TB), 0, ctx->stream, n, agg, ec, x);
    else hipLaunchKernelGGL(prolong_agg_kernel<0>, dim3(mgs_grid(n, TB)), dim3(TB), 0, ctx->stream, n, agg, ec, x);
  }
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_jacobi_zero(mgs_ctx *ctx, int n, double omega, const double *dinv, const double *b, double *x) {
  if (n) hipLaunchKernelGGL(jacobi_zero_kernel, dim3(mgs_grid(n, TB)), dim3(TB), 0, ctx->stream, n, omega, dinv, b, x);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_fill(mgs_ctx *ctx, double *d, int64_t n, double v) {
  if (n) hipLaunchKernelGGL(fill_kernel, dim3(mgs_blas1_grid_capped(ctx, n)), dim3(TB), 0, ctx->stream, d, n, v);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_rand(mgs_ctx *ctx, double *d, int64_t n, uint64_t seed, int64_t off) {
  if (n) hipLaunchKernelGGL(rand_kernel, dim3(mgs_blas1_grid_capped(ctx, n)), dim3(TB), 0, ctx->stream, d, n, seed, off);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_gather(mgs_ctx *ctx, const double *x, const int *idx, int64_t n, double *out) {
  if (n) hipLaunchKernelGGL(gather_kernel, dim3(mgs_grid(n, TB)), dim3(TB), 0, ctx->stream, x, idx, n, out);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

// FP32 copy of an operand's values: round to nearest (the conversion instruction's default mode)
__global__ void round_vals_kernel(const double *__restrict__ in, float *__restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (float)in[i];
}
int k_round_vals(mgs_ctx *ctx, const double *in, float *out, int64_t n) {
  if (n) hipLaunchKernelGGL(round_vals_kernel, dim3(mgs_grid(n, TB)), dim3(TB), 0, ctx->stream, in, out, n);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_scale_vals(mgs_ctx *ctx, const mgs_csr *A, const double *wd, double *out) {
  if (A->nnz) hipLaunchKernelGGL(scale_vals_kernel, dim3(mgs_grid(A->nnz, TB)), dim3(TB), 0, ctx->stream, A->nnz, A->col, A->val, wd, out);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_diag_count(const mgs_csr *A, int *bad_count_host) {
  mgs_ctx *ctx = A->ctx;
  int *bad = nullptr;
  MGS_TRY(mgs_dev_alloc(ctx, &bad, 1));
  MGS_HIP(ctx, hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
  if (A->rows) hipLaunchKernelGGL(diag_count_kernel, dim3(mgs_grid(A->rows, TB)), dim3(TB), 0, ctx->stream, A->rows, A->rowptr, A->col, bad);
  MGS_HIP(ctx, hipMemcpyAsync(bad_count_host, bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  MGS_HIP(ctx, mgs_hip_free(bad));
  return MGS_OK;
}
int k_drop_diag_vals(mgs_ctx *ctx, const mgs_csr *A, const double *val, double omega, double *out, signed char *code, int *bad_dev) {
  if (A->rows) hipLaunchKernelGGL(drop_diag_vals_kernel, dim3(mgs_grid(A->rows, TB)), dim3(TB), 0, ctx->stream, A->rows, A->rowptr, A->col, val, omega, out, code, bad_dev);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_pack7(mgs_ctx *ctx, const int *blkptr, int nblocks, int nd_rows, const double *src, int *e0, unsigned char *out) {
  if (nblocks > 0) {
    hipLaunchKernelGGL(pack7_scan_kernel, dim3(nblocks), dim3(MGS_RB), 0, ctx->stream, blkptr, nd_rows, src, e0);
    hipLaunchKernelGGL(pack7_fill_kernel, dim3(nblocks), dim3(MGS_RB), 0, ctx->stream, blkptr, nd_rows, src, e0, out);
  }
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_map_cols(mgs_ctx *ctx, const mgs_csr *A, const int *cmap, int *out) {
  if (A->rows) hipLaunchKernelGGL(map_cols_kernel, dim3(mgs_grid(A->rows, TB)), dim3(TB), 0, ctx->stream, A->rows, A->rowptr, A->col, cmap, out);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
// last sharded level: own slice of the replicated tail's solution, and the level's halo slots from the same vector (it holds the
// neighbours' entries too) — what the copy of the slice plus a halo exchange would deliver, in one dispatch and without the wire
__global__ void tail_scatter_kernel(const double *__restrict__ xt, int my_off, int n_loc, const int *__restrict__ halo_global, int n_halo, double *__restrict__ x) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n_loc) x[j] = xt[my_off + j];
  else if (j < n_loc + n_halo) x[j] = xt[halo_global[j - n_loc]];
}
int k_tail_scatter(mgs_ctx *ctx, const double *xt, int my_off, int n_loc, const int *halo_global, int n_halo, double *x) {
  if (n_loc + n_halo) hipLaunchKernelGGL(tail_scatter_kernel, dim3(mgs_grid(n_loc + n_halo, TB)), dim3(TB), 0, ctx->stream, xt, my_off, n_loc, halo_global, n_halo, x);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_concat_i32(mgs_ctx *ctx, const int *a, int na, const int *b, int nb, int *out) {
  if (na + nb) hipLaunchKernelGGL(concat_i32_kernel, dim3(mgs_grid(na + nb, TB)), dim3(TB), 0, ctx->stream, a, na, b, nb, out);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_abs_inplace(mgs_ctx *ctx, int64_t n, double *v) {
  if (n) hipLaunchKernelGGL(abs_vals_kernel, dim3(mgs_blas1_grid_capped(ctx, n)), dim3(TB), 0, ctx->stream, n, v);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
// max_i |v_i| as the bits of a non-negative double, folded into *amax_bits_dev (the caller zeroes it; a NaN wins): dense_absmax_kernel
int k_absmax_dev(mgs_ctx *ctx, int64_t n, const double *v, unsigned long long *amax_bits_dev) {
  if (n) hipLaunchKernelGGL(dense_absmax_kernel, dim3(mgs_blas1_grid_capped(ctx, n)), dim3(TB), 0, ctx->stream, n, v, amax_bits_dev);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_label_indicator(mgs_ctx *ctx, int n, const signed char *lab, int f, double *out) {
  if (n) hipLaunchKernelGGL(label_indicator_kernel, dim3(mgs_grid(n, TB)), dim3(TB), 0, ctx->stream, n, lab, f, out);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_coarse_labels(mgs_ctx *ctx, const mgs_xfer *T, const signed char *lab, signed char *clab, unsigned long long *bad_dev) {
  if (T->n_fine) hipLaunchKernelGGL(coarse_labels_kernel, dim3(mgs_grid(T->n_fine, TB)), dim3(TB), 0, ctx->stream, T->n_fine, T->agg, T->cptr, T->members, lab, clab, bad_dev);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_kc_update_r(mgs_ctx *ctx, int n, const double *scal, const double *r, const double *v1, double *rp) {
  if (n) hipLaunchKernelGGL(kc_update_r_kernel, dim3(mgs_grid(n, TB)), dim3(TB), 0, ctx->stream, n, scal, r, v1, rp);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
int k_kc_combine(mgs_ctx *ctx, int n, const double *scal, const double *c1, const double *c2, double *x) {
  if (n) hipLaunchKernelGGL(kc_combine_kernel, dim3(mgs_grid(n, TB)), dim3(TB), 0, ctx->stream, n, scal, c1, c2, x);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

int k_dense_gemv(mgs_ctx *ctx, int n, const double *M, const double *b, double *x) {
  if (n) hipLaunchKernelGGL(dense_gemv_kernel, dim3(mgs_grid(n, TB / 64)), dim3(TB), 0, ctx->stream, n, M, b, x);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

// *inv_out == NULL: the n·n result is allocated here (and released again on failure); else it is written into the caller's buffer
// (mgs_hier_refresh: the cached graphs hold that pointer), which stays the caller's whatever happens.  MGS_ERR_NUMERIC: a pivot not
// greater than 8·n·DBL_EPSILON·max|a_ij| (see gj_pivot_kernel), which also refuses NaN and Inf among the values.  The work buffers are
// released on every exit.  reg_const == 1: A + (max|a_ij|/n)·1·1ᵀ is inverted (constant null space declared; dense_reg_const_kernel); 2: A + Σ_f (max|a_ij|/n_f)·z_f·z_fᵀ
// for the labels lab (device) with fcount[f] rows each (field-wise null space; dense_reg_fields_kernel).
int k_dense_inverse(mgs_ctx *ctx, const mgs_csr *A, double **inv_out, int reg_const, const signed char *lab, const double *fcount) {
  const int n = A->rows;
  double *const into = *inv_out;
  MGS_CHECK(ctx, A->cols == n, MGS_ERR_INVALID, "coarsest operator is not square (%d x %d)", A->rows, A->cols);
  double *W = nullptr, *colk = nullptr, *inv = into; int *piv = nullptr;
  unsigned long long *amax = nullptr;
  hipStream_t s = ctx->stream;
  int h[2] = {0, 0};
  auto run = [&]() -> int {
    MGS_TRY(mgs_dev_alloc(ctx, &W, (size_t)n * 2 * n));
    MGS_TRY(mgs_dev_alloc(ctx, &colk, (size_t)n + 1));
    if (!into) MGS_TRY(mgs_dev_alloc(ctx, &inv, (size_t)n * n));
    MGS_TRY(mgs_dev_alloc(ctx, &piv, 2));
    MGS_TRY(mgs_dev_alloc(ctx, &amax, 1));
    MGS_HIP(ctx, hipMemsetAsync(W, 0, sizeof(double) * (size_t)n * 2 * n, s));
    MGS_HIP(ctx, hipMemsetAsync(piv, 0, 2 * sizeof(int), s));
    MGS_HIP(ctx, hipMemsetAsync(amax, 0, sizeof(unsigned long long), s));
    if (A->nnz) hipLaunchKernelGGL(dense_absmax_kernel, dim3(mgs_blas1_grid_capped(ctx, A->nnz)), dim3(TB), 0, s, (int64_t)A->nnz, A->val, amax);
    if (n) hipLaunchKernelGGL(dense_scatter_kernel, dim3(mgs_grid(n, TB)), dim3(TB), 0, s, n, A->rowptr, A->col, A->val, W);
    if (n && reg_const == 1) hipLaunchKernelGGL(dense_reg_const_kernel, dim3(mgs_grid(n, TB), n), dim3(TB), 0, s, n, W, amax);
    if (n && reg_const == 2) {
      DenseFieldCounts fc;
      for (int k = 0; k < MGS_NULLSPACE_MAX_FIELDS; ++k) fc.n[k] = fcount[k] > 0.0 ? fcount[k] : 1.0;
      hipLaunchKernelGGL(dense_reg_fields_kernel, dim3(mgs_grid(n, TB), n), dim3(TB), 0, s, n, W, amax, lab, fc);
    }
    for (int k = 0; k < n; ++k) {
      hipLaunchKernelGGL(gj_pivot_kernel, dim3(1), dim3(TB), 0, s, n, k, W, piv, colk + n, amax);
      hipLaunchKernelGGL(gj_swap_scale_kernel, dim3(mgs_grid(2 * n, TB)), dim3(TB), 0, s, n, k, W, piv, colk + n);
      hipLaunchKernelGGL(gj_colsave_kernel, dim3(mgs_grid(n, TB)), dim3(TB), 0, s, n, k, W, colk);
      hipLaunchKernelGGL(gj_eliminate_kernel, dim3(mgs_grid(2 * n, TB), n), dim3(TB), 0, s, n, k, W, colk);
    }
    if (n) hipLaunchKernelGGL(gj_extract_kernel, dim3(mgs_grid(n, TB), n), dim3(TB), 0, s, n, W, inv);
    MGS_HIP(ctx, hipGetLastError());
    MGS_HIP(ctx, hipMemcpyAsync(h, piv, sizeof h, hipMemcpyDeviceToHost, s));
    MGS_HIP(ctx, hipStreamSynchronize(s));
    return MGS_OK;
  };
  int rc = run();
  if (rc != MGS_OK) hipStreamSynchronize(s);      // nothing enqueued above may still touch the buffers released below
  if (W) mgs_hip_free(W);
  if (colk) mgs_hip_free(colk);
  if (piv) mgs_hip_free(piv);
  if (amax) mgs_hip_free(amax);
  if (rc == MGS_OK && h[1]) rc = mgs_fail(ctx, MGS_ERR_NUMERIC, "coarsest operator (%d rows) is singular to working precision, or holds NaN/Inf", n);
  if (rc != MGS_OK) { if (!into && inv) mgs_hip_free(inv); return rc; }
  *inv_out = inv;
  return MGS_OK;
}

int k_poisson3d(mgs_ctx *ctx, int N, int plane_lo, int plane_hi, int local_cols, mgs_csr **out) {
  MGS_CHECK(ctx, N >= 2 && plane_lo >= 0 && plane_hi <= N && plane_lo < plane_hi, MGS_ERR_INVALID, "poisson3d: bad N/planes");
  const int64_t N2 = (int64_t)N * N, n_loc = (int64_t)(plane_hi - plane_lo) * N2;
  // nnz of the shard = rowptr(e1) − rowptr(e0); computed on host with the same closed form
  auto rp = [&](int64_t e) -> int64_t {
    if (e >= N2 * N) return 7 * N2 * N - 6 * N2;
    int64_t i = e / N2;  // e is a plane boundary here
    // rows before plane i: 7 per row minus missing neighbours
    int64_t rows = i * N2;
    int64_t miss = (i > 0 ? N2 : 0) + 0 /*i==N-1 rows before: none unless i==N*/ + 2 * i * N /*j==0,N-1*/ + 2 * i * N /*k==0,N-1*/;
    return 7 * rows - miss;
  };
  const int64_t nnz = rp((int64_t)plane_hi * N2) - rp((int64_t)plane_lo * N2);
  MGS_CHECK(ctx, nnz < 2147483647LL && n_loc < 2147483647LL, MGS_ERR_INVALID, "poisson3d shard too large for int32 indices");
  const int has_lo = plane_lo > 0, has_hi = plane_hi < N;
  int64_t ncols = local_cols ? n_loc + (has_lo + has_hi) * N2 : N2 * N;
  MGS_CHECK(ctx, ncols < 2147483647LL, MGS_ERR_INVALID, "poisson3d: too many columns for int32");
  mgs_csr *A = nullptr;
  MGS_TRY(mgs_csr_alloc(ctx, (int)n_loc, (int)ncols, nnz, &A));
  hipLaunchKernelGGL(poisson3d_kernel, dim3(mgs_grid(n_loc + 1, TB)), dim3(TB), 0, ctx->stream, N, plane_lo, n_loc, local_cols, has_lo, has_hi, A->rowptr, A->col, A->val);
  MGS_HIP(ctx, hipGetLastError());
  MGS_TRY(mgs_plan_csr(A));
  *out = A;
  return MGS_OK;
}

int k_poisson2d(mgs_ctx *ctx, int n, mgs_csr **out) {
  MGS_CHECK(ctx, n >= 2 && (int64_t)n * n < 400000000LL, MGS_ERR_INVALID, "poisson2d: bad n");
  int N = n * n; int64_t nnz = 5LL * N - 4LL * n;
  mgs_csr *A = nullptr;
  MGS_TRY(mgs_csr_alloc(ctx, N, N, nnz, &A));
  hipLaunchKernelGGL(poisson2d_kernel, dim3(mgs_grid(N + 1, TB)), dim3(TB), 0, ctx->stream, n, A->rowptr, A->col, A->val);
  MGS_HIP(ctx, hipGetLastError());
  MGS_TRY(mgs_plan_csr(A));
  *out = A;
  return MGS_OK;
}
