// kernels_variants.hip — the A/B-only forms of y = A x, r = b − A x and the damped Jacobi sweep (rowblock.hpp; option spmv_variant):
// the earlier "products in LDS" kernel (variants 2–4), the slice kernel software-pipelined over four row blocks (6) and with one wave per
// workgroup (7).  Kept for A/B runs (tools/studies_r1_r3/ab_spmv.py) as they were; held arm by arm by tests/test_gpu_operator_kernels.py.
// No launch runs them by default: mgs_launch_csr_op_range (kernels_spmv.hip) reaches them through launch_variant, at the end of this file.
#include "rowblock.hpp"

namespace {

template <int OP, bool NT, int LANES, int CHUNK>
__global__ __launch_bounds__(RB) void csr_rowblock_kernel(
    int n, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val,
    const double *__restrict__ x, const double *__restrict__ b, const double *__restrict__ dinv, double omega,
    double *__restrict__ out, int cap, BlockMap bm) {
  extern __shared__ double prod[];
  const int vb = map_block(bm, blockIdx.x);
  if (vb < 0) return;
  const int r0 = (bm.base + vb) * RB;
  const int r1 = min(r0 + RB, n);
  const int tid = threadIdx.x;
  const int lo = rowptr[r0];
  const int hi = rowptr[r1];
  if (hi - lo <= cap) {
    const int row = r0 + tid;
    int my_lo = 0, my_hi = 0;
    if (row < r1) { my_lo = rowptr[row] - lo; my_hi = rowptr[row + 1] - lo; }
    // phase 1: coalesced stream of the block's matrix slice, products to LDS
    if (CHUNK == 1) {
      const int *__restrict__ cp = col + lo;
      const double *__restrict__ vp = val + lo;
      const int cnt = hi - lo;
#pragma unroll 8
      for (int k = tid; k < cnt; k += RB) {
        const int c = ld_stream<NT>(cp + k);
        const double v = ld_stream<NT>(vp + k);
        prod[k] = v * x[c];
      }
    } else if (CHUNK == 2) {
      // 2 entries per lane per step: val as one 16-byte load, col as one 8-byte load.  The slice is
      // widened to even element offsets (allocation is padded; out-of-slice lanes are masked).
      const int start = lo & ~1;
      const int nch = (hi - start + 1) >> 1;
#pragma unroll 4
      for (int c = tid; c < nch; c += RB) {
        const int k = start + 2 * c;
        const int2_t cc = ld_stream<NT>(reinterpret_cast<const int2_t *>(col + k));
        const double2_t vv = ld_stream<NT>(reinterpret_cast<const double2_t *>(val + k));
        if (k >= lo) prod[k - lo] = vv.x * x[cc.x];
        if (k + 1 < hi) prod[k + 1 - lo] = vv.y * x[cc.y];
      }
    } else {
      // 4 entries per lane per step: col as one 16-byte load, val as two 16-byte loads
      const int start = lo & ~3;
      const int nch = (hi - start + 3) >> 2;
#pragma unroll 2
      for (int c = tid; c < nch; c += RB) {
        const int k = start + 4 * c;
        const int4_t cc = ld_stream<NT>(reinterpret_cast<const int4_t *>(col + k));
        const double2_t v01 = ld_stream<NT>(reinterpret_cast<const double2_t *>(val + k));
        const double2_t v23 = ld_stream<NT>(reinterpret_cast<const double2_t *>(val + k + 2));
        if (k >= lo && k < hi) prod[k - lo] = v01.x * x[cc.x];
        if (k + 1 >= lo && k + 1 < hi) prod[k + 1 - lo] = v01.y * x[cc.y];
        if (k + 2 >= lo && k + 2 < hi) prod[k + 2 - lo] = v23.x * x[cc.z];
        if (k + 3 >= lo && k + 3 < hi) prod[k + 3 - lo] = v23.y * x[cc.w];
      }
    }
    __syncthreads();
    // phase 2: sequential per-row sum in ascending column order
    if (row < r1) {
      double s = 0.0;
      for (int k = my_lo; k < my_hi; ++k) s += prod[k];
      epilogue<OP>(row, s, x, b, dinv, omega, out);
    }
  } else {
    // long-row block: LANES lanes cooperate on one row, shuffle reduction
    const int sub = tid / LANES, lane = tid % LANES;
    for (int row = r0 + sub; row < r1; row += RB / LANES) {
      double s = 0.0;
      const int e = rowptr[row + 1];
      for (int k = rowptr[row] + lane; k < e; k += LANES) s += val[k] * x[col[k]];
#pragma unroll
      for (int off = LANES / 2; off > 0; off >>= 1) s += __shfl_down(s, off, LANES);
      if (lane == 0) epilogue<OP>(row, s, x, b, dinv, omega, out);
    }
  }
}

// Variant D: variant B (the slice kernel, kernels_spmv.hip) with ONE WAVE per workgroup (64 rows, ~5 KB of LDS).  No workgroup barrier at
// all — a wave's LDS writes are ordered before its own reads — so every wave streams, gathers and
// stores at its own pace and the CU always has waves in each phase.  Four consecutive 64-row groups of
// one 256-row block map to the same XCD (locality as in variant B).
template <int OP>
__global__ __launch_bounds__(64) void csr_wave_slice_kernel(
    int n, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val,
    const double *__restrict__ x, const double *__restrict__ b, const double *__restrict__ dinv, double omega,
    double *__restrict__ out, int cap, BlockMap bm) {
  extern __shared__ double lds_raw[];
  const int bid = blockIdx.x;
  int vb, sub;
  if (bm.remap) { const int idx = bid >> 3; vb = map_block_xi(bm, bid & 7, idx >> 2); sub = idx & 3; }
  else { vb = (bid >> 2) < bm.nblocks ? (bid >> 2) : -1; sub = bid & 3; }
  if (vb < 0) return;
  const int r0 = (bm.base + vb) * RB + sub * 64;
  if (r0 >= n) return;
  const int r1 = min(r0 + 64, n);
  const int tid = threadIdx.x;
  const int lo = rowptr[r0];
  const int hi = rowptr[r1];
  double *__restrict__ vals = lds_raw;
  int *__restrict__ cols = reinterpret_cast<int *>(lds_raw + cap + 2);
  const int row = r0 + tid;
  const int start = lo & ~1;
  int my_a = 0, my_e = 0;
  double bi = 0.0, di = 0.0, xi = 0.0;
  if (row < r1) {
    my_a = rowptr[row] - start; my_e = rowptr[row + 1] - start;
    if (OP != MGS_OP_SPMV) bi = b[row];
    if (OP == MGS_OP_JACOBI) { di = dinv[row]; xi = x[row]; }
  }
  const int nch = (hi - start + 1) >> 1;
#pragma unroll 4
  for (int c = tid; c < nch; c += 64) {
    const int k = start + 2 * c;
    *reinterpret_cast<int2_t *>(cols + 2 * c) = *reinterpret_cast<const int2_t *>(col + k);
    *reinterpret_cast<double2_t *>(vals + 2 * c) = *reinterpret_cast<const double2_t *>(val + k);
  }
  __syncthreads();   // single-wave workgroup: lowers to a wait on the wave's own LDS writes
  if (row < r1) {
    double s = 0.0;
    for (int k = my_a; k < my_e; k += 8) {
      double xv[8];
      const int rem = my_e - k;
#pragma unroll
      for (int q = 0; q < 8; ++q) xv[q] = q < rem ? x[cols[k + q]] : 0.0;
#pragma unroll
      for (int q = 0; q < 8; ++q) if (q < rem) s += vals[k + q] * xv[q];
    }
    if (OP == MGS_OP_SPMV) out[row] = s;
    else if (OP == MGS_OP_RESIDUAL) out[row] = bi - s;
    else out[row] = xi + (omega * di) * (bi - s);
  }
}

// Variant C: variant B software-pipelined over G consecutive row blocks per workgroup.  The slice of
// row block i+1 is already in flight (registers) while the lanes gather x and sum row block i, so the
// val/col stream never waits for the gather phase of its own workgroup.  Same arithmetic, same order.
template <int OP, bool NT, int ITER, int G>
__global__ __launch_bounds__(RB) void csr_rowblock_pipe_kernel(
    int n, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val,
    const double *__restrict__ x, const double *__restrict__ b, const double *__restrict__ dinv, double omega,
    double *__restrict__ out, int cap, BlockMap bm, int nrb_total /*row blocks of the launched range*/) {
  extern __shared__ double lds_raw[];
  double *__restrict__ vals = lds_raw;
  int *__restrict__ cols = reinterpret_cast<int *>(lds_raw + cap + 2);
  const int sb = map_block(bm, blockIdx.x);      // super block index (G row blocks each)
  if (sb < 0) return;
  const int tid = threadIdx.x;
  const int first = sb * G;
  const int nblk = min(G, nrb_total - first);
  int bnd[G + 1];
#pragma unroll
  for (int j = 0; j <= G; ++j) { const int r = min((bm.base + first + j) * RB, n); bnd[j] = rowptr[r]; }
  double2_t rv[ITER]; int2_t rc[ITER];
  auto issue = [&](int j) {
    const int start = bnd[j] & ~1;
    const int nch = (bnd[j + 1] - start + 1) >> 1;
#pragma unroll
    for (int q = 0; q < ITER; ++q) {
      const int c = tid + q * RB;
      if (c < nch) {
        rc[q] = ld_stream<NT>(reinterpret_cast<const int2_t *>(col + start + 2 * c));
        rv[q] = ld_stream<NT>(reinterpret_cast<const double2_t *>(val + start + 2 * c));
      }
    }
  };
  issue(0);
#pragma unroll
  for (int j = 0; j < G; ++j) {
    if (j >= nblk) break;
    const int r0 = (bm.base + first + j) * RB, r1 = min(r0 + RB, n);
    const int lo = bnd[j], hi = bnd[j + 1];
    const int start = lo & ~1;
    const int nch = (hi - start + 1) >> 1;
    const int row = r0 + tid;
    int my_a = 0, my_e = 0;
    double bi = 0.0, di = 0.0, xi = 0.0;
    if (row < r1) {
      my_a = rowptr[row] - start; my_e = rowptr[row + 1] - start;
      if (OP != MGS_OP_SPMV) bi = b[row];
      if (OP == MGS_OP_JACOBI) { di = dinv[row]; xi = x[row]; }
    }
#pragma unroll
    for (int q = 0; q < ITER; ++q) {
      const int c = tid + q * RB;
      if (c < nch) {
        *reinterpret_cast<double2_t *>(vals + 2 * c) = rv[q];
        *reinterpret_cast<int2_t *>(cols + 2 * c) = rc[q];
      }
    }
    __syncthreads();
    if (j + 1 < nblk) issue(j + 1);
    if (row < r1) {
      double s = 0.0;
      int k = my_a;
      for (; k + 8 <= my_e; k += 8) {
        double xv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) xv[q] = x[cols[k + q]];
#pragma unroll
        for (int q = 0; q < 8; ++q) s += vals[k + q] * xv[q];
      }
      {
        double xv[8];
        const int rem = my_e - k;
#pragma unroll
        for (int q = 0; q < 8; ++q) xv[q] = q < rem ? x[cols[k + q]] : 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) if (q < rem) s += vals[k + q] * xv[q];
      }
      if (OP == MGS_OP_SPMV) out[row] = s;
      else if (OP == MGS_OP_RESIDUAL) out[row] = bi - s;
      else out[row] = xi + (omega * di) * (bi - s);
    }
    __syncthreads();
  }
}

// entries per lane and step of the products-in-LDS kernel
template <class F> void with_chunk(int n, F f) {
  if (n == 1) f(int_c<1>{}); else if (n == 2) f(int_c<2>{}); else f(int_c<4>{});
}

// products in LDS (variants 2, 3, 4 = 1, 2, 4 entries per lane and step)
int launch_lanes(const mgs_csr *A, int op, int chunk, dim3 grid, const double *x, const double *b, const double *dinv, double omega,
                 double *out, int cap, const BlockMap &bm) {
  mgs_ctx *ctx = A->ctx;
  const size_t lds = sizeof(double) * (size_t)(cap > 0 ? cap : 1);
  const bool known = with_csr_op(op, [&](auto O) {
    with_bool(ctx->opt_nontemporal > 0, [&](auto NT) {
      with_lanes(long_row_lanes(A), [&](auto LN) {
        with_chunk(chunk, [&](auto CH) {
          hipLaunchKernelGGL((csr_rowblock_kernel<decltype(O)::value, decltype(NT)::value, decltype(LN)::value, decltype(CH)::value>), grid, dim3(RB),
                             lds, ctx->stream, A->rows, A->rowptr, A->col, A->val, x, b, dinv, omega, out, cap, bm);
        });
      });
    });
  });
  if (!known) return mgs_fail(ctx, MGS_ERR_INVALID, "unknown csr op %d", op);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
// pipelined variant (6): G row blocks per workgroup; block map over super blocks
int launch_pipe(const mgs_csr *A, int op, const double *x, const double *b, const double *dinv, double omega, double *out, int cap,
                const BlockMap &bm) {
  mgs_ctx *ctx = A->ctx;
  constexpr int G = 4;
  const int nrb = bm.nblocks;
  BlockMap sm = bm;
  // base stays in row-block units inside the kernel: bm.base + first + j
  dim3 g = plan_map(ctx, sm, bm.base, (nrb + G - 1) / G, ((A->far_band + RB - 1) / RB + G - 1) / G, 64,
                    ctx->opt_strip > 0 ? std::max(1, ctx->opt_strip / G) : 16);
  const size_t lds = (size_t)(cap + 2) * 12 + 16;
  const bool known = with_csr_op(op, [&](auto O) {
    with_bool(ctx->opt_nontemporal != 0, [&](auto NT) {
      hipLaunchKernelGGL((csr_rowblock_pipe_kernel<decltype(O)::value, decltype(NT)::value, 4, G>), g, dim3(RB), lds, ctx->stream, A->rows, A->rowptr,
                         A->col, A->val, x, b, dinv, omega, out, cap, sm, nrb);
    });
  });
  if (!known) return mgs_fail(ctx, MGS_ERR_INVALID, "unknown csr op %d", op);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
// wave variant (7): four workgroups of one wave per row block
int launch_wave(const mgs_csr *A, int op, const double *x, const double *b, const double *dinv, double omega, double *out, dim3 grid,
                const BlockMap &bm) {
  mgs_ctx *ctx = A->ctx;
  const int capw = A->max_wave_nnz;
  dim3 g(grid.x * 4);
  const size_t ldsw = (size_t)(capw + 2) * 12 + 16;
  const bool known = with_csr_op(op, [&](auto O) {
    hipLaunchKernelGGL((csr_wave_slice_kernel<decltype(O)::value>), g, dim3(64), ldsw, ctx->stream, A->rows, A->rowptr, A->col, A->val, x, b, dinv,
                       omega, out, capw, bm);
  });
  if (!known) return mgs_fail(ctx, MGS_ERR_INVALID, "unknown csr op %d", op);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

}  // namespace

// The guards, in the order mgs_launch_csr_op_range always took them (tests/spmv_ref.py restates them); a variant whose guard fails, and
// every other value of the option, is the caller's: the pattern-coded kernel or the slice kernel.
bool launch_variant(const mgs_csr *A, int op, const double *x, const double *b, const double *dinv, double omega, double *out, int cap,
                    dim3 grid, const BlockMap &bm, int *rc) {
  const int variant = A->ctx->opt_spmv_variant;
  // pipe: ITER·RB = 1024 sixteen-byte pairs per row block.  A block of cnt entries from entry lo on needs (cnt + (lo & 1) + 1) >> 1 pairs
  // (its slice starts at lo & ~1): 1024 for cnt = 2047 at either parity of lo, 1025 for cnt = 2048 at an odd lo — so 2047 is the bound
  // (tests/spmv_ref.py pairs_needed, tests/test_spmv_ref_cpu.py); heavier matrices run the slice kernel
  if (variant == 6 && A->max_block_nnz <= 2047 && A->max_block_nnz == A->lds_cap) { *rc = launch_pipe(A, op, x, b, dinv, omega, out, cap, bm); return true; }
  if (variant == 7 && A->max_wave_nnz <= 4096) { *rc = launch_wave(A, op, x, b, dinv, omega, out, grid, bm); return true; }
  if (variant < 2 || variant > 4) return false;
  if (A->pk7) A->pk7->ran = 0;      // the products-in-LDS kernel reads no packed copy (mgs_hier_pack_info)
  *rc = launch_lanes(A, op, variant == 2 ? 1 : (variant == 3 ? 2 : 4), grid, x, b, dinv, omega, out, cap, bm);
  return true;
}
