// kernels_spmv.hip — the fine-level hot path: what a SpMV, residual or Jacobi launch runs by default (row-block design: rowblock.hpp).
//
//   y = A x                       (`A * v`,           reference src/common/bicg.cpp:57,82,107,117)
//   r = b − A x                   (                   reference src/common/bicg.cpp:82)
//   x' = x + ωD⁻¹(b − A x)        (damped Jacobi,     reference src/CPU_Matlab/solve.m:17)
//
// Default path for operators whose rows repeat their shape (stencils, their Galerkin levels): the row-block
// kernel with a PATTERN-CODED column index (csr_rowblock_coded_kernel, mgs_csr_optimize) — 8 B per entry streamed
// instead of 12, same products in the same order; irregular row blocks keep their index slice.  Every other operator runs the slice kernel
// (csr_rowblock_slice_kernel).  The coded kernel's body also serves the cycle's post pass (FUSE_POST_MAPPED; kernels_fused.hip calls
// launch_coded).  The A/B-only variants live in kernels_variants.hip, the pattern code's setup in rowblock_setup.hip.
#include "rowblock.hpp"

namespace {

// Variant B ("slice in LDS, row-parallel gather").  Phase 1 parks the block's raw val/col slice
// in LDS (coalesced 16-byte / 8-byte loads, no dependent gather in the streaming
// phase).  Phase 2: lane t walks row t; on step q the 64 lanes of a wave gather x[col] for 64
// CONSECUTIVE rows, which for stencil-like operators is one contiguous run (4–5 cache lines per
// wave instruction instead of ~12 when 64 consecutive entries are gathered) — 2.5× less L2→L1
// traffic and TA work for the x gather.  Sum order is still the ascending column order of the
// row, so the result stays bit-identical to the scalar CPU loop.
template <int OP, bool NT, int LANES, int U>
__global__ __launch_bounds__(RB) void csr_rowblock_slice_kernel(
    int n, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val,
    const double *__restrict__ x, const double *__restrict__ b, const double *__restrict__ dinv, double omega,
    double *__restrict__ out, int cap, BlockMap bm, int seq_overflow, const int *__restrict__ blkptr, int nts) {
  extern __shared__ double lds_raw[];
  const int vb = map_block(bm, blockIdx.x);
  if (vb < 0) return;
  const int blk = block_of(bm, vb);
  const int r0 = blk * RB;
  const int r1 = min(r0 + RB, n);
  const int tid = threadIdx.x;
  // block bounds from the compact per-block copy of rowptr (consecutive workgroups share cache lines;
  // rowptr[r0] itself is 1 KiB apart from block to block)
  const int lo = blkptr ? blkptr[blk] : rowptr[r0];
  const int hi = blkptr ? blkptr[blk + 1] : rowptr[r1];
  if (hi - lo <= cap) {
    double *__restrict__ vals = lds_raw;                                   // cap + 2 doubles
    int *__restrict__ cols = reinterpret_cast<int *>(lds_raw + cap + 2);   // cap + 2 ints
    const int row = r0 + tid;
    const int start = lo & ~1;                 // even element offset → 16-byte aligned val pairs
    int my_a = 0, my_e = 0;
    double bi = 0.0, di = 0.0, xi = 0.0;
    if (row < r1) {
      my_a = rowptr[row] - start; my_e = rowptr[row + 1] - start;
      if (OP != MGS_OP_SPMV) bi = b[row];
      if (OP == MGS_OP_JACOBI) { di = dinv[row]; xi = x[row]; }
    }
    const int nch = (hi - start + 1) >> 1;
    // (a loop-free form of this staging — four predicated int2 + double2 loads per lane — measured 1.5 % SLOWER here, 2.553 against
    // 2.515 ms: 64 instead of 46 VGPRs; the coded kernels, which stage values only, gain 5–7 % from it)
#pragma unroll 4
    for (int c = tid; c < nch; c += RB) {
      const int k = start + 2 * c;
      const int2_t cc = ld_stream<NT>(reinterpret_cast<const int2_t *>(col + k));
      const double2_t vv = ld_stream<NT>(reinterpret_cast<const double2_t *>(val + k));
      *reinterpret_cast<double2_t *>(vals + 2 * c) = vv;
      *reinterpret_cast<int2_t *>(cols + 2 * c) = cc;
    }
    __syncthreads();
    if (row < r1) {
      // U entries per step, branch-free: the column reads past the row's end stay inside the staged slice
      // and are clamped to the last staged entry, so every gathered index is a real column; their products are replaced by +0.0, which
      // leaves the running sum bit-identical.  All U gathers are in flight before the first add.
      double s = 0.0;
      const int lim = hi - start - 1;                  // last staged index
      for (int k = my_a; k < my_e; k += U) {
        int cq[U]; double xv[U], vq[U];
#pragma unroll
        for (int q = 0; q < U; ++q) cq[q] = cols[min(k + q, lim)];
#pragma unroll
        for (int q = 0; q < U; ++q) xv[q] = x[cq[q]];   // past the row's end: some staged entry's column, always a valid x index
#pragma unroll
        for (int q = 0; q < U; ++q) vq[q] = vals[min(k + q, lim)];
#pragma unroll
        for (int q = 0; q < U; ++q) s += (k + q < my_e) ? vq[q] * xv[q] : 0.0;
      }
      st_stream(out + row, OP == MGS_OP_SPMV ? s : (OP == MGS_OP_RESIDUAL ? bi - s : xi + (omega * di) * (bi - s)), (nts & 1) != 0);
    }
  } else if (seq_overflow) {
    // heavier-than-budget block of short rows: lane t walks row t straight from global memory, same
    // ascending order (bit-identical to the staged path)
    const int row = r0 + tid;
    if (row < r1) {
      double s = 0.0;
      for (int k = rowptr[row], e = rowptr[row + 1]; k < e; ++k) s += val[k] * x[col[k]];
      epilogue<OP>(row, s, x, b, dinv, omega, out);
    }
  } else {
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

// Pattern-coded rows (format: rowblock.hpp; setup: rowblock_setup.hip).
// (round 1: the post pass took 68 VGPRs unbounded = 7 waves per SIMD, bounded to 8 waves it measured 2 % faster, the other ops 0.5–0.8 % slower;
// since its prologue was rewritten it needs 52–56, the other ops 58–64, and the bound no longer binds)
// VAL: the tuples carry the values as well (`vtab`, option valcode): a coded block then streams no matrix entry at all.
// one 256-row block of the pattern-coded kernel (the two __global__ wrappers below call it once per workgroup, or once per row block
// of a group of blocks)
// PK (option pack7; RESIDUAL and the post pass on FP64 values, no halo, no value tuples): a coded + staged block whose pk_e0 entry is not −1 stages
// its slice of the packed copy pk (7/8 as many 16-byte pieces, from the block's first entry rounded down to a multiple of 16) and fetches every
// value through pk7_fetch; indices, products and their order are those of the FP64 walk.  Every other block reads val as before.
template <int OP, int U, bool HALO, bool VAL, class VT = double, bool PK = false>
__device__ __forceinline__ void coded_block_body(
    const int blk, int n, const int *__restrict__ rowptr, const int *__restrict__ idx, const VT *__restrict__ val,
    const unsigned char *__restrict__ pid, const int *__restrict__ tptr, const int *__restrict__ tab,
    const double *__restrict__ x /*gather source: x, or e_c for the post pass*/, const double *__restrict__ b /*b, or r for the post pass*/,
    const double *__restrict__ dinv /*dinv, or wd for the post pass*/, double omega, const double *__restrict__ xin /*post pass: b*/,
    const int *__restrict__ agg /*post pass*/, double *__restrict__ out, int capv, int capi, const int *__restrict__ blkptr,
    const double *__restrict__ hv /*row shards: values of the indices >= split*/, int split, const double *__restrict__ vtab,
    const unsigned char *__restrict__ dpos /*t-form post pass: position of a_ii inside the row (NULL: read wd)*/,
    const double *__restrict__ dot_w1, double *__restrict__ dot_part /*SpMV: (y·w1, y·y) partials [2][nblocks] of this launch (NULL: none)*/,
    int dot_nb, int flags /*kernel-uniform; bit 0: no row is longer than U → the gather step runs once, without a loop; bit 1: loop-free staging (option stage_unroll); bit 2: option rowptr_scan*/,
    const unsigned char *__restrict__ pk = nullptr, const int *__restrict__ pk_e0 = nullptr) {
  extern __shared__ double lds_raw[];
  constexpr bool POST = OP == FUSE_POST_MAPPED;
  static_assert(!PK || (sizeof(VT) == 8 && !HALO && !VAL && (OP == MGS_OP_RESIDUAL || POST)), "packed values: pre and post pass of an unsharded FP64 level only");
  constexpr bool F32 = sizeof(VT) == 4;      // FP32 operand values: no value tuples, no fused dots, ωD⁻¹ from wd; the code may be absent (tptr = NULL)
  constexpr int VA = val_traits<VT>::VA;
  typedef typename val_traits<VT>::v16 v16_t;
  typedef typename val_traits<VT>::i16 i16_t;
  static_assert(!F32 || (!VAL && !HALO && (OP == MGS_OP_RESIDUAL || POST)), "float values: pre and post pass of an unsharded level only");
  const int r0 = blk * RB;
  const int r1 = min(r0 + RB, n);
  const int tid = threadIdx.x;
  const int lo = blkptr[blk], hi = blkptr[blk + 1];
  int t0 = 0, tlen = 0;
  if (!F32 || tptr) { t0 = tptr[blk]; tlen = tptr[blk + 1] - t0; }
  const int capi_abs = capi < 0 ? -capi : capi;
  VT *__restrict__ vals = reinterpret_cast<VT *>(lds_raw);                                // capv + 2 doubles (capv + 8 floats)
  int *__restrict__ ints = reinterpret_cast<int *>(lds_raw + val_region<VT>(capv));       // capi ints: the block's table, or its index slice
  const int row = r0 + tid;
  const int start = lo & ~(VA - 1);
  const int nent = hi - start;
  const bool coded = tlen > 0 && tlen <= capi_abs && (!VAL || tlen <= capv);
  const bool staged = hi - lo <= capv && (coded || nent + VA - 1 <= capi_abs);     // block-uniform
  // PK: records of the block's packed slice, and whether the block runs on it (block-uniform; the records must fit the value region)
  int pk_nrec = 0, pk_e = -1;
  bool packed = false;
  if constexpr (PK) {
    pk_nrec = ((hi + 15) >> 4) - (lo >> 4);
    pk_e = pk_e0[blk];
    packed = coded && staged && pk_e >= 0 && 14 * pk_nrec <= val_region<VT>(capv);
  }
  int ga = 0, ge = 0, base = row;
  double bi = 0.0, di = 0.0, xi = 0.0, pei = 0.0;
  const bool dmode = POST && dpos != nullptr && xin == nullptr;    // ωD⁻¹ from the streamed diagonal entry (same bits as wd = ω·(1/a_ii))
  unsigned dp = 255;
  int mypid = 0;      // the row's pattern id: loaded HERE, with the other per-row loads — behind the barrier it was one more full memory latency in series
  const bool scan = coded && staged && (flags & 4);      // block-uniform: row ranges from the pattern lengths (coded_row_range)
  int wave_first = 0;
  if (scan) wave_first = rowptr[min(r0 + (tid & ~63), n)];
  if (row < r1) {
    if (!scan) { ga = rowptr[row]; ge = rowptr[row + 1]; }
    if (coded) mypid = pid[row];
    if (OP == MGS_OP_SPMV && dot_part) bi = dot_w1[row];       // fused dots: w1 of this row (bi is free in this op); loaded here, not behind the store
    if (OP != MGS_OP_SPMV) bi = b[row];
    if (OP == MGS_OP_JACOBI) { di = dinv[row]; xi = x[row]; }
    if (POST) {                                                     // xin = NULL: b holds t = b + r
      // Every load of this prologue is independent of the others and none is waited for before the value slice below is in flight:
      // the ISA of the first form (dpos → branch → dinv → wait; agg → wait → e_c[agg]) held four serialized memory latencies per
      // workgroup in front of the staging loop, which is why the post pass ran slower per byte than the other ops.  The loads that
      // depend on agg (e_c of the own aggregate) and on the diagonal's position are issued behind the barrier with the gathers.
      base = agg[row];
      if (dmode) dp = dpos[row]; else di = dinv[row];               // kernel-uniform branch
      if (xin) xi = xin[row];                                       // scaled by di in the epilogue
    }
  }
  auto late_loads = [&]() {      // POST: what depends on the prologue's loads
    if (POST && row < r1) {
      pei = base >= 0 ? x[base] : 0.0;
      if (dmode && dp == 255) di = dinv[row];                       // diagonal not found in the row: the wd vector after all
    }
  };
  double s = 0.0;
  if (staged) {
    const int nch = (PK && packed) ? 7 * pk_nrec : (nent + VA - 1) >> (VA == 4 ? 2 : 1);      // 16-byte pieces of the value slice
    if (PK && packed) {      // the packed slice: whole records from the block's first entry rounded down to a multiple of 16, staged like the values
      const v16_t *__restrict__ psrc = reinterpret_cast<const v16_t *>(pk + (size_t)112 * (size_t)(lo >> 4));
      if (nch <= 4 * RB && (flags & 2)) {
        v16_t rr[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int c = tid + k * RB; if (c < nch) rr[k] = psrc[c]; }
        int tw = 0;
        if (tid < tlen) tw = tab[t0 + tid];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int c = tid + k * RB; if (c < nch) reinterpret_cast<v16_t *>(vals)[c] = rr[k]; }
        if (tid < tlen) ints[tid] = tw;
        for (int c = tid + RB; c < tlen; c += RB) ints[c] = tab[t0 + c];
      } else {
#pragma unroll 4
        for (int c = tid; c < nch; c += RB) reinterpret_cast<v16_t *>(vals)[c] = psrc[c];
        for (int c = tid; c < tlen; c += RB) ints[c] = tab[t0 + c];
      }
    } else if (coded) {
      if (VAL) { for (int c = tid; c < tlen; c += RB) vals[c] = vtab[t0 + c]; }     // value tuples instead of the value slice (tlen <= capv)
      else if (nch <= 4 * RB && (flags & 2)) {
        // No loop in front of the barrier: four predicated 16-byte loads per lane, all in flight together with the prologue's per-row
        // loads.  A loop here makes the compiler drain every outstanding load at its header (s_waitcnt vmcnt(0) in the ISA: wait counts
        // across a back edge are not tracked), i.e. a workgroup paid one full memory latency for rowptr/b/agg/… and a second one for
        // its value slice.
        v16_t rr[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int c = tid + k * RB; if (c < nch) rr[k] = *reinterpret_cast<const v16_t *>(val + start + VA * c); }
        int tw = 0;
        if (tid < tlen) tw = tab[t0 + tid];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int c = tid + k * RB; if (c < nch) *reinterpret_cast<v16_t *>(vals + VA * c) = rr[k]; }
        if (tid < tlen) ints[tid] = tw;
        for (int c = tid + RB; c < tlen; c += RB) ints[c] = tab[t0 + c];
      } else {
#pragma unroll 4
        for (int c = tid; c < nch; c += RB) *reinterpret_cast<v16_t *>(vals + VA * c) = *reinterpret_cast<const v16_t *>(val + start + VA * c);
        for (int c = tid; c < tlen; c += RB) ints[c] = tab[t0 + c];
      }
      if (VAL) for (int c = tid; c < tlen; c += RB) ints[c] = tab[t0 + c];
    } else {
#pragma unroll 4
      for (int c = tid; c < nch; c += RB) {
        const int k = start + VA * c;
        *reinterpret_cast<i16_t *>(ints + VA * c) = *reinterpret_cast<const i16_t *>(idx + k);
        *reinterpret_cast<v16_t *>(vals + VA * c) = *reinterpret_cast<const v16_t *>(val + k);
      }
    }
    __syncthreads();
    if (scan) coded_row_range(ints, 0, tlen, mypid, row < r1, wave_first, ga, ge);
    late_loads();
    if (row < r1 && ge > ga) {
      const int my_a = ga - start, my_e = ge - start, lim = nent - 1;
      if (coded) {
        const int ps = ints[mypid];
        const int last = my_e - my_a - 1;
        auto step = [&](const int k, const int j) {
          int oq[U]; double xv[U], vq[U];
#pragma unroll
          for (int q = 0; q < U; ++q) oq[q] = ints[ps + min(j + q, last)];   // past the row's end: the row's last index again
#pragma unroll
          for (int q = 0; q < U; ++q) {
            if (HALO && oq[q] >= CODE_HALO_LO) xv[q] = hv[row + (oq[q] - CODE_HALO)];
            else if (POST) {           // unconditional load (a column outside every aggregate reads entry 0 and is zeroed): no branch per gather
              const bool neg = oq[q] == CODE_NEG;
              const double g = x[neg ? 0 : base + oq[q]];
              xv[q] = neg ? 0.0 : g;
            } else xv[q] = x[base + oq[q]];
          }
#pragma unroll
          for (int q = 0; q < U; ++q) vq[q] = VAL ? vals[ps + min(j + q, last)] : vals[min(k + q, lim)];
#pragma unroll
          for (int q = 0; q < U; ++q) s += (k + q < my_e) ? vq[q] * xv[q] : 0.0;
        };
        // rows that all fit one step (7-point operators with U = 7, A·P with U = 5): straight-line code, so the loads issued behind
        // the barrier (e_c of the own aggregate) stay in flight beside the gathers instead of being drained at a loop header
        if constexpr (PK) {
          if (packed) {      // the same walk, every value through pk7_fetch (the packed slice starts at a multiple of 16 entries)
            const unsigned char *__restrict__ pvals = reinterpret_cast<const unsigned char *>(lds_raw);
            const int pk_sh = start - (lo & ~15);
            const unsigned pk_e0sh = (unsigned)pk_e << 20;
            auto step_pk = [&](const int k, const int j) {
              int oq[U]; double xv[U], vq[U];
#pragma unroll
              for (int q = 0; q < U; ++q) oq[q] = ints[ps + min(j + q, last)];
#pragma unroll
              for (int q = 0; q < U; ++q) {
                if (POST) {
                  const bool neg = oq[q] == CODE_NEG;
                  const double g = x[neg ? 0 : base + oq[q]];
                  xv[q] = neg ? 0.0 : g;
                } else xv[q] = x[base + oq[q]];
              }
#pragma unroll
              for (int q = 0; q < U; ++q) vq[q] = pk7_fetch(pvals, min(k + q, lim) + pk_sh, pk_e0sh);
#pragma unroll
              for (int q = 0; q < U; ++q) s += (k + q < my_e) ? vq[q] * xv[q] : 0.0;
            };
            if ((flags & 3) == 3) step_pk(my_a, 0);
            else for (int k = my_a, j = 0; k < my_e; k += U, j += U) step_pk(k, j);
            if (POST && dmode && dp != 255) di = omega * (1.0 / pk7_fetch(pvals, my_a + (int)dp + pk_sh, pk_e0sh));
          }
        }
        if (PK && packed) {}
        else if ((flags & 3) == 3) step(my_a, 0);
        else for (int k = my_a, j = 0; k < my_e; k += U, j += U) step(k, j);
        if (POST && dmode && dp != 255 && !(PK && packed)) di = omega * (1.0 / (VAL ? vals[ps + (int)dp] : vals[my_a + (int)dp]));
      } else {
        for (int k = my_a; k < my_e; k += U) {
          int cq[U]; double xv[U], vq[U];
#pragma unroll
          for (int q = 0; q < U; ++q) cq[q] = ints[min(k + q, lim)];
#pragma unroll
          for (int q = 0; q < U; ++q) {
            if (HALO && cq[q] >= split) xv[q] = hv[cq[q] - split];
            else if (POST) { const bool neg = cq[q] < 0; const double g = x[neg ? 0 : cq[q]]; xv[q] = neg ? 0.0 : g; }
            else xv[q] = x[cq[q]];
          }
#pragma unroll
          for (int q = 0; q < U; ++q) vq[q] = vals[min(k + q, lim)];
#pragma unroll
          for (int q = 0; q < U; ++q) s += (k + q < my_e) ? vq[q] * xv[q] : 0.0;
        }
        if (POST && dmode && dp != 255) di = omega * (1.0 / vals[my_a + (int)dp]);
      }
    }
  } else if (row < r1) {
    // heavier-than-budget block: lane t walks row t straight from global memory, same ascending order
    late_loads();
    for (int k = ga; k < ge; ++k) {
      const int c = idx[k];
      s += (double)val[k] * ((HALO && c >= split) ? hv[c - split] : ((POST && c < 0) ? 0.0 : x[c]));
    }
    if (POST && dmode && dp != 255) di = omega * (1.0 / val[ga + (int)dp]);
  }
  if (row < r1) {
    double v;
    if (OP == MGS_OP_SPMV) v = s;
    else if (OP == MGS_OP_RESIDUAL) v = bi - s;
    else if (OP == MGS_OP_JACOBI) v = xi + (omega * di) * (bi - s);
    else v = xin ? (di * xi + pei) + di * (bi - s) : pei + di * (bi - s);     // t-form: x = Pe + wd∘(t − A·Pe), t = b + r
    st_stream(out + row, v, capi < 0);                                              // capi < 0: streaming store (option nt_store)
    if (OP == MGS_OP_SPMV && dot_part) { bi = v * bi; di = v * v; }                // this row's terms of (y·w1, y·y); bi/di are free in this op
  }
  if (OP == MGS_OP_SPMV && dot_part) {      // launch-uniform: one partial pair per row block, summed in a fixed order
    double p1 = row < r1 ? bi : 0.0, p2 = row < r1 ? di : 0.0;
    for (int off = 32; off > 0; off >>= 1) { p1 += __shfl_down(p1, off); p2 += __shfl_down(p2, off); }
    __syncthreads();                                   // the staged values are done with: their LDS holds the 4 wave sums
    if ((tid & 63) == 0) { lds_raw[2 * (tid >> 6)] = p1; lds_raw[2 * (tid >> 6) + 1] = p2; }
    __syncthreads();
    if (tid == 0) {
      double t1 = 0.0, t2 = 0.0;
      for (int q = 0; q < RB / 64; ++q) { t1 += lds_raw[2 * q]; t2 += lds_raw[2 * q + 1]; }
      dot_part[blk] = t1; dot_part[dot_nb + blk] = t2;
    }
  }
}

#define CODED_PARAMS CODED_PARAMS_T(VT)
#define CODED_PARAMS_T(VT)                                                                                                              \
    int n, const int *__restrict__ rowptr, const int *__restrict__ idx, const VT *__restrict__ val,                                      \
    const unsigned char *__restrict__ pid, const int *__restrict__ tptr, const int *__restrict__ tab, const double *__restrict__ x,      \
    const double *__restrict__ b, const double *__restrict__ dinv, double omega, const double *__restrict__ xin,                         \
    const int *__restrict__ agg, double *__restrict__ out, int capv, int capi, BlockMap bm, const int *__restrict__ blkptr,               \
    const double *__restrict__ hv, int split, const double *__restrict__ vtab, const unsigned char *__restrict__ dpos,                   \
    const double *__restrict__ dot_w1, double *__restrict__ dot_part, int dot_nb, int flags
#define CODED_ARGS n, rowptr, idx, val, pid, tptr, tab, x, b, dinv, omega, xin, agg, out, capv, capi, blkptr, hv, split, vtab, dpos, dot_w1, dot_part, dot_nb, flags

template <int OP, int U, bool HALO, bool VAL, class VT = double>
__global__ __launch_bounds__(RB, OP == FUSE_POST_MAPPED ? 8 : 1) void csr_rowblock_coded_kernel(CODED_PARAMS) {
  const int vb = map_block(bm, blockIdx.x);
  if (vb < 0) return;
  coded_block_body<OP, U, HALO, VAL, VT>(block_of(bm, vb), CODED_ARGS);
}
// the packed form (option pack7): the same body with PK, and the packed copy behind the parameters of the form above
// (the post pass with U = 7 / 8 needs more than the 64 registers of eight waves per SIMD: unbounded there, instead of a bound that spills)
template <int OP, int U>
__global__ __launch_bounds__(RB, OP == FUSE_POST_MAPPED && U <= 5 ? 8 : 1) void csr_rowblock_coded_pk_kernel(CODED_PARAMS_T(double), const unsigned char *__restrict__ pk,
                                                                                                  const int *__restrict__ pk_e0) {
  const int vb = map_block(bm, blockIdx.x);
  if (vb < 0) return;
  coded_block_body<OP, U, false, false, double, true>(block_of(bm, vb), CODED_ARGS, pk, pk_e0);
}
// the same row blocks swept group by group (descriptors of the grouped pre pass, kernels_fused.hip: up to GRP_BLOCKS blocks per workgroup, one
// after the other) — experiment: does the post pass gain what the grouped pre pass gains from fewer, fatter workgroups?
template <int OP, int U, bool HALO, bool VAL, class VT = double>
__global__ __launch_bounds__(RB, OP == FUSE_POST_MAPPED ? 8 : 1) void csr_rowblock_coded_group_kernel(CODED_PARAMS, const int *__restrict__ gdesc) {
  const int g = map_block(bm, blockIdx.x);
  if (g < 0) return;
  const int4_t gb = *reinterpret_cast<const int4_t *>(gdesc + (size_t)32 * g);
#pragma unroll 1
  for (int h = 0; h < 4; ++h) {
    const int blk = h == 0 ? gb.x : (h == 1 ? gb.y : (h == 2 ? gb.z : gb.w));
    if (blk < 0) break;                               // group-uniform
    if (h) __syncthreads();                           // the previous block's LDS slice is done with
    coded_block_body<OP, U, HALO, VAL>(blk, CODED_ARGS);
  }
}

// the slice kernel (default path of operators without a usable pattern code; variant 1: cap < 0, every row block on the long-row path)
template <int OP, bool NT>
int launch_slice(const mgs_csr *A, int lanes, dim3 grid, const double *x, const double *b,
                 const double *dinv, double omega, double *out, int cap, BlockMap bm) {
  const size_t lds = (size_t)(cap > 0 ? cap + 2 : 2) * 12 + 16 + (size_t)A->ctx->opt_lds_pad;   // opt_lds_pad: occupancy experiments
  const int flags = kernel_flags(A->ctx, nt_store_on(A), false);
  with_lanes(lanes, [&](auto LN) {
    with_width<false>(gather_width(A), [&](auto U) {
      hipLaunchKernelGGL((csr_rowblock_slice_kernel<OP, NT, decltype(LN)::value, decltype(U)::value>), grid, dim3(RB), lds, A->ctx->stream,
                         A->rows, A->rowptr, A->col, A->val, x, b, dinv, omega, out, cap, bm, A->max_row_len <= 64 ? 1 : 0, blkptr_opt(A), flags);
    });
  });
  report_launch(A->ctx, 4, gather_width(A), flags, cap > 0 ? cap : 0, cap > 0 ? cap + 2 : 2);
  return MGS_OK;
}

}  // namespace

// The coded kernel on the view A (idx = its coded index array, c its code).  op ∈ {SPMV, RESIDUAL, JACOBI, FUSE_POST_MAPPED}; for the post
// pass: x = e_c, b = r, dinv = wd, xin = b, idx = agg[col].  hv/split: halo payload of a row shard.
// The value type follows A->val32 — the pre pass (RESIDUAL on Â) and the post pass (FUSE_POST_MAPPED on A·P) of an FP32 level run the same
// kernel instantiated for float values.  That form serves any unsharded operator with short rows — c may be NULL or code only a few blocks:
// the uncoded blocks stage their index slice — so a level switched to FP32 never falls back to a kernel that reads the FP64 values.
int launch_coded(const mgs_csr *A, const mgs_rowcode *c, int op, const int *idx, const double *x, const double *b, const double *dinv,
                 double omega, const double *xin, const int *agg, double *out, dim3 grid, BlockMap bm, const double *hv, int split) {
  mgs_ctx *ctx = A->ctx;
  const bool f32 = A->val32 != nullptr;
  const bool post = op != MGS_OP_SPMV && op != MGS_OP_RESIDUAL && op != MGS_OP_JACOBI;
  if (f32) {
    if (op != MGS_OP_RESIDUAL && op != FUSE_POST_MAPPED) return mgs_fail(ctx, MGS_ERR_INVALID, "FP32 operand values: op %d has no float form", op);
    if (hv) return mgs_fail(ctx, MGS_ERR_INVALID, "FP32 operand values: the coded kernel has no float form on a row shard");
    if (c && c->vtab) c = nullptr;      // value tuples are FP64: not this path (the setter refuses option valcode)
  }
  const coded_lds l = coded_budget(A, c, f32);
  const size_t lds = l.val_bytes + l.int_bytes + l.pad_bytes;
  const int u = post ? post_gather_width(A) : gather_width(A);
  const int flags = kernel_flags(ctx, A->max_row_len <= u, true);
  const double *vtab = c ? c->vtab : nullptr;
  const unsigned char *dpos = post && !f32 ? A->dpos : nullptr;      // t-form post pass (FP64 values): ω/a_ii from the streamed values
  if (dpos) omega = A->dpos_omega;
  // group sweep (views with A->sweep set; FP64 values, plain index codes, no halo): one workgroup per row-block group of the grouped pre pass
  const bool sweep = A->sweep && !f32 && !hv && !vtab && op == FUSE_POST_MAPPED;
  // option pack7: the view carries a packed copy of its FP64 values that is in step with them (pre pass on Â, post pass on A·P; unsharded, no value tuples)
  mgs_pack7 *pk = A->pk7;
  const bool packed = mgs_pack7_serves(pk, false) && ctx->opt_pack7 && c && !f32 && !hv && !vtab && !sweep && (op == MGS_OP_RESIDUAL || op == FUSE_POST_MAPPED);
  if (pk) pk->ran = packed ? 1 : 0;
  BlockMap gbm; dim3 ggrid(1);
  if (sweep) ggrid = plan_group_map(A, A->sweep, gbm);
  // the two wrappers share CODED_PARAMS; `more`: what the group wrapper takes behind them
  auto launch = [&](auto kernel, auto vals, dim3 g, const BlockMap &m, auto... more) {
    hipLaunchKernelGGL(kernel, g, dim3(RB), lds, ctx->stream, A->rows, A->rowptr, idx, vals, c ? c->pid : nullptr, c ? c->tptr : nullptr,
                       c ? c->tab : nullptr, x, b, dinv, omega, xin, agg, out, l.capv, nt_store_on(A) ? -l.capi : l.capi, m, A->blkptr, hv, split,
                       vtab, dpos, op == MGS_OP_SPMV ? A->dot_w1 : nullptr, op == MGS_OP_SPMV ? A->dot_part : nullptr, mgs_row_blocks(A), flags,
                       more...);
  };
  auto form = [&](auto O, auto H, auto V, auto vals) {
    constexpr int OP = decltype(O)::value;
    constexpr bool HALO = decltype(H)::value, VAL = decltype(V)::value;
    using VT = pointee_t<decltype(vals)>;
    with_width<OP == FUSE_POST_MAPPED>(u, [&](auto U) {
      constexpr int UU = decltype(U)::value;
      if constexpr (OP == FUSE_POST_MAPPED && !HALO && !VAL && std::is_same_v<VT, double>) {
        if (sweep) return launch(csr_rowblock_coded_group_kernel<OP, UU, false, false>, vals, ggrid, gbm, A->sweep->gdesc);
      }
      if constexpr ((OP == FUSE_POST_MAPPED || OP == MGS_OP_RESIDUAL) && !HALO && !VAL && std::is_same_v<VT, double>) {
        if (packed) return launch(csr_rowblock_coded_pk_kernel<OP, UU>, vals, grid, bm, (const unsigned char *)pk->data, (const int *)pk->e0);
      }
      launch(csr_rowblock_coded_kernel<OP, UU, HALO, VAL, VT>, vals, grid, bm);
    });
  };
  const std::false_type no{};
  if (f32) {      // the float forms: RESIDUAL and the post pass, never the halo or value-tuple forms
    if (post) form(int_c<FUSE_POST_MAPPED>{}, no, no, A->val32); else form(int_c<MGS_OP_RESIDUAL>{}, no, no, A->val32);
  } else {
    const double *val = A->val;
    with_bool(hv != nullptr, [&](auto H) {
      with_bool(vtab != nullptr, [&](auto V) {
        if (!with_csr_op(op, [&](auto O) { form(O, H, V, val); })) form(int_c<FUSE_POST_MAPPED>{}, H, V, val);
      });
    });
  }
  report_launch(ctx, f32 ? 2 : (sweep ? 3 : 1), u, flags, l.capv, l.capi, (f32 ? 1 : 0) | (packed ? 4 : 0), c ? c->tptr : nullptr);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

int mgs_spmv_dots(const mgs_csr *A, const double *x, double *y, const double *w1, double *out_host2) {
  mgs_ctx *ctx = A->ctx;
  const int nb = mgs_row_blocks(A);
  const bool fused = ctx->opt_fuse_dots && A->rows > 0 && ctx->opt_spmv_variant == 0 && !ctx->opt_nontemporal && use_rowcode(A, A->code) && A->lds_cap >= 8;
  if (!fused) {
    MGS_TRY(mgs_launch_csr_op(A, MGS_OP_SPMV, x, nullptr, nullptr, 0.0, y));
    return k_dot2(ctx, A->rows, y, w1, y, y, out_host2);
  }
  MGS_TRY(mgs_ensure_dot_part(ctx, 2 * (int64_t)nb));
  mgs_csr V = *A; V.owns = false; V.dot_w1 = w1; V.dot_part = ctx->dot_part;     // every row block of the launch writes its pair
  MGS_TRY(mgs_launch_csr_op(&V, MGS_OP_SPMV, x, nullptr, nullptr, 0.0, y));
  return k_dot2_finish(ctx, nb, ctx->dot_part, out_host2);
}

bool mgs_rowcode_usable(const mgs_csr *A, bool any) { return use_rowcode(A, A->code, any); }

// The coded kernel on the row blocks [blk_lo, blk_hi) of the view A (A->col = the coded index array, A->code its
// code); hv/split: halo payload of a row shard (nullptr / INT_MAX: none).  Caller checks mgs_rowcode_usable(A).
int mgs_launch_coded_range(const mgs_csr *A, int op, const double *x, const double *b, const double *dinv, double omega,
                           const double *xin, const int *agg, double *out, const double *hv, int split, int blk_lo, int blk_hi,
                           int gap_at, int gap_len) {
  if (A->rows == 0 || blk_hi <= blk_lo) return MGS_OK;
  if (!use_rowcode(A, A->code, hv != nullptr)) return MGS_ERR_STATE;
  BlockMap bm;
  const dim3 grid = plan_block_map(A, blk_lo, blk_hi, gap_at, gap_len, bm);
  return launch_coded(A, A->code, op, A->col, x, b, dinv, omega, xin, agg, out, grid, bm, hv, hv ? split : 0x7fffffff);
}

int mgs_launch_csr_op(const mgs_csr *A, int op, const double *x, const double *b, const double *dinv,
                      double omega, double *out) {
  return mgs_launch_csr_op_range(A, op, x, b, dinv, omega, out, 0, mgs_row_blocks(A));
}

// the same kernels on the row blocks [blk_lo, blk_hi) only (interior / boundary split of a row shard)
int mgs_launch_csr_op_range(const mgs_csr *A, int op, const double *x, const double *b, const double *dinv,
                            double omega, double *out, int blk_lo, int blk_hi, int gap_at, int gap_len) {
  mgs_ctx *ctx = A->ctx;
  if (A->rows == 0 || blk_hi <= blk_lo) return MGS_OK;
  if (gap_len > 0 && ctx->opt_spmv_variant != 0 && ctx->opt_spmv_variant != 5) {   // experimental variants: no gap support
    MGS_TRY(mgs_launch_csr_op_range(A, op, x, b, dinv, omega, out, blk_lo, gap_at, 0x7fffffff, 0));
    return mgs_launch_csr_op_range(A, op, x, b, dinv, omega, out, gap_at + gap_len, blk_hi + gap_len, 0x7fffffff, 0);
  }
  BlockMap bm;
  const dim3 grid = plan_block_map(A, blk_lo, blk_hi, gap_at, gap_len, bm);
  // FP32 level: pre pass on the float copy of Â's values, whatever the SpMV variant options say (the float forms take no ω)
  if (A->val32) return launch_coded(A, A->code, op, A->col, x, b, dinv, 0.0, nullptr, nullptr, out, grid, bm);
  // variants: 0 auto, 1 forced sub-wavefront rows, 2/3/4 = products-in-LDS with 1/2/4 entries per lane, 5 = slice-in-LDS, 6 = pipelined, 7 = one wave
  // per workgroup.  2–4, 6 and 7 are A/B-only forms (kernels_variants.hip); 6 and 7 fall through to the kernels below where their guards fail
  const int cap = ctx->opt_spmv_variant == 1 ? -1 : A->lds_cap;
  int rc = MGS_OK;
  if (launch_variant(A, op, x, b, dinv, omega, out, cap, grid, bm, &rc)) return rc;
  if (ctx->opt_spmv_variant == 0 && !ctx->opt_nontemporal && use_rowcode(A, A->code))
    return launch_coded(A, A->code, op, A->col, x, b, dinv, omega, nullptr, nullptr, out, grid, bm);
  if (A->pk7) A->pk7->ran = 0;      // the slice kernel reads no packed copy (mgs_hier_pack_info)
  const bool known = with_csr_op(op, [&](auto O) {
    with_bool(ctx->opt_nontemporal > 0, [&](auto NT) {
      launch_slice<decltype(O)::value, decltype(NT)::value>(A, long_row_lanes(A), grid, x, b, dinv, omega, out, cap, bm);
    });
  });
  if (!known) return mgs_fail(ctx, MGS_ERR_INVALID, "unknown csr op %d", op);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
