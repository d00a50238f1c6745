// kernels_fused.hip — the row-block kernels only the fused V-cycle runs (rowblock.hpp): the gather kernel of the fused passes
// (csr_rowblock_fused_kernel: pre and post pass of levels without a usable pattern code) and the grouped pre pass (row blocks paired along
// their aggregates, restriction inside the pass: two setup kernels, the one-block and the pair kernel, the stray kernel, the host grouping).
// The coded post pass is csr_rowblock_coded_kernel<FUSE_POST_MAPPED> of kernels_spmv.hip, reached through launch_coded.
#include "rowblock.hpp"

namespace {

// Fused V-cycle passes on the slice kernel (square, unsharded levels only):
//   FUSE_PRE : from x = 0 with ν1 = 1:  x1 = wd∘b,  r = b − A·x1   (gathers wd[c]·b[c]; one pass instead
//              of the (ωD⁻¹)b kernel + the residual kernel; bit-identical to the two-kernel form)
//   FUSE_POST: coarse-grid correction + one Jacobi sweep:  x'' = x1 + Pe + wd∘(r − A·Pe), Pe_j = ec[agg_j], x1 = wd∘b
//              recomputed from b (so the PRE pass need not store it)
//              (r = b − Ax is the residual already computed before restriction, so b − A(x+Pe) = r − A·Pe;
//              one pass instead of prolong-add + Jacobi; equal to the two-kernel form up to rounding)
// wd = ω·dinv precomputed per level.
template <int OP, bool STAGED>
__device__ __forceinline__ double fused_row_sum(const double *__restrict__ vsrc, const int *__restrict__ csrc, int a, int e,
                                                const double *__restrict__ wd, const double *__restrict__ bvec,
                                                const int *__restrict__ agg, const double *__restrict__ ec,
                                                int n_owned, const double *__restrict__ hv /*values of the halo columns (row shards)*/) {
  double s = 0.0;
  for (int k = a; k < e; k += 8) {
    double xv[8];
    const int rem = e - k;
    if (OP == FUSE_PRE) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (q < rem) { const int c = csrc[k + q]; xv[q] = wd[c] * (c < n_owned ? bvec[c] : hv[c - n_owned]); } else xv[q] = 0.0;   // row shards: wd covers the halo columns, hv = the peers' raw b
      }
    } else if (OP == FUSE_POST_MAPPED) {
      int av[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) av[q] = q < rem ? csrc[k + q] : -1;      // coarse column (−1: not aggregated)
#pragma unroll
      for (int q = 0; q < 8; ++q) xv[q] = av[q] >= 0 ? ec[av[q]] : 0.0;
    } else {
      int av[8], cv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) { cv[q] = q < rem ? csrc[k + q] : -1; av[q] = cv[q] >= 0 ? agg[cv[q]] : -1; }   // agg: coarse column of every local column (row shards: halo slots too)
#pragma unroll
      for (int q = 0; q < 8; ++q) xv[q] = av[q] >= 0 ? ec[av[q]] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) if (q < rem) s += vsrc[k + q] * xv[q];
  }
  return s;
}

template <int OP>
__global__ __launch_bounds__(RB) void csr_rowblock_fused_kernel(
    int n, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val,
    const double *__restrict__ wd, const double *__restrict__ bvec /*PRE: b, POST: r*/, const double *__restrict__ xin /*POST: b (x1 = wd∘b)*/,
    const int *__restrict__ agg, const double *__restrict__ ec, double *__restrict__ out /*PRE: r, POST: x''*/,
    double *__restrict__ out2 /*PRE: x1*/, int cap, BlockMap bm, const double *__restrict__ hv, const int *__restrict__ blkptr) {
  extern __shared__ double lds_raw[];
  const int vb = map_block(bm, blockIdx.x);
  if (vb < 0) return;
  const int blk = block_of(bm, vb);
  const int r0 = blk * RB;
  const int r1 = min(r0 + RB, n);
  const int tid = threadIdx.x;
  const int lo = blkptr ? blkptr[blk] : rowptr[r0];
  const int hi = blkptr ? blkptr[blk + 1] : rowptr[r1];
  double *__restrict__ vals = lds_raw;
  int *__restrict__ cols = reinterpret_cast<int *>(lds_raw + cap + 2);
  const int row = r0 + tid;
  const int start = lo & ~1;
  const bool staged = hi - lo <= cap;      // block-uniform; the few heavier blocks read their rows from global memory
  int ga = 0, ge = 0;
  double bi = 0.0, wi = 0.0, xi = 0.0, pei = 0.0;
  if (row < r1) {
    ga = rowptr[row]; ge = rowptr[row + 1];
    bi = bvec[row]; wi = wd[row];
    if (OP == FUSE_POST || OP == FUSE_POST_MAPPED) { xi = xin ? wi * xin[row] : 0.0; const int a = agg[row]; pei = a >= 0 ? ec[a] : 0.0; }   // x1 = wd∘b recomputed (xin = b; NULL: bvec holds t = b + r)
  }
  if (staged) {
    const int nch = (hi - start + 1) >> 1;
#pragma unroll 4
    for (int c = tid; c < nch; c += RB) {
      const int k = start + 2 * c;
      *reinterpret_cast<int2_t *>(cols + 2 * c) = *reinterpret_cast<const int2_t *>(col + k);
      *reinterpret_cast<double2_t *>(vals + 2 * c) = *reinterpret_cast<const double2_t *>(val + k);
    }
    __syncthreads();
  }
  if (row < r1) {
    const double s = staged ? fused_row_sum<OP, true>(vals, cols, ga - start, ge - start, wd, bvec, agg, ec, n, hv)
                            : fused_row_sum<OP, false>(val, col, ga, ge, wd, bvec, agg, ec, n, hv);
    if (OP == FUSE_PRE) { out[row] = bi - s; if (out2) out2[row] = wi * bi; }
    else out[row] = xin ? (xi + pei) + wi * (bi - s) : pei + wi * (bi - s);
  }
}

// ---------------------------------------------------------------------------------------------------------
// Grouped pre pass (DESIGN.md §4 "restriction inside the pre pass").  The V(1,1) cycle from x = 0 needs r = b − Â·b only
// for two things: its restriction r_c = Pᵀr and the post pass, which needs b + r.  Aggregates of the pairwise matching
// are 2–4 rows that sit in one row block or in two (a row and its neighbour one grid line further), so setup pairs such
// row blocks into GROUPS; one workgroup sweeps the blocks of a group with the coded row-block kernel's body, keeps the
// ≤ 512 residuals in LDS, writes t = b + r and restricts every aggregate whose members all lie in the group — same
// members, same ascending order as restrict_agg_kernel, so r_c has the same bits.  The r vector never travels through HBM
// (−8 B per row written, −8 B read back by the restriction, −4 B of member index, −8 B in the post pass, which reads t
// instead of r and b).  Aggregates that leave their group (odd shapes at domain boundaries) are "strays": their member rows
// also store r (bit mask), and a small trailing kernel restricts them from memory.
constexpr int GRP_MAX_MEMBERS = 6;     // 4 + 10 + 5·10 = 64 bits of the member code
constexpr int GRP_BLOCKS = 4;          // row blocks per group (residual buffer: up to 4·256 doubles of LDS)
constexpr int GRP_DESC = 32;           // ints per group descriptor (128 B: blocks, entry bounds lo/hi, aggregate ranges lo/hi)

// setup 1: aggregate ids must ascend with their first member (they do for the device matching: ids = rank of the leader);
// afirst[b] = first aggregate whose first member lies in row block >= b; votes: per row block up to GRP_SLOTS distinct
// other blocks its aggregates reach, with counts (the host pairs every block with its most frequent partner)
constexpr int GRP_SLOTS = 4;
__global__ void grp_scan_kernel(int nc, const int *__restrict__ cptr, const int *__restrict__ members, int nblocks,
                                int *__restrict__ vkey, int *__restrict__ vcnt, int *__restrict__ afirst, int *__restrict__ bad) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= nc) return;
  const int lo = cptr[a], hi = cptr[a + 1];
  if (hi <= lo) { atomicOr(bad, 1); return; }
  const int fm = members[lo], fb = fm / RB, lb = members[hi - 1] / RB;
  int pb = -1;
  if (a > 0) {
    const int plo = cptr[a - 1];
    if (lo <= plo) { atomicOr(bad, 1); return; }
    const int pfm = members[plo];
    if (pfm >= fm) { atomicOr(bad, 1); return; }
    pb = pfm / RB;
  }
  for (int q = pb + 1; q <= fb; ++q) afirst[q] = a;
  if (a == nc - 1) for (int q = fb + 1; q <= nblocks; ++q) afirst[q] = nc;
  if (lb != fb)
    for (int sl = 0; sl < GRP_SLOTS; ++sl) {
      const int old = atomicCAS(&vkey[fb * GRP_SLOTS + sl], -1, lb);
      if (old == -1 || old == lb) { atomicAdd(&vcnt[fb * GRP_SLOTS + sl], 1); break; }
    }
}
// setup 2: member positions inside the group's residual buffer (q-th block of the group: q·256 .. q·256+255), or stray
__global__ void grp_code_kernel(int nc, const int *__restrict__ cptr, const int *__restrict__ members, const int *__restrict__ blk2grp,
                                const int *__restrict__ gblk, unsigned long long *__restrict__ acode, unsigned *__restrict__ wmask,
                                int *__restrict__ stray, int stray_cap, int *__restrict__ nstray) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= nc) return;
  const int lo = cptr[a], cnt = cptr[a + 1] - lo;
  const int g = blk2grp[members[lo] / RB];
  int gb[GRP_BLOCKS];
#pragma unroll
  for (int q = 0; q < GRP_BLOCKS; ++q) gb[q] = gblk[GRP_BLOCKS * g + q];
  bool ok = cnt <= GRP_MAX_MEMBERS;
  unsigned long long code = (unsigned long long)cnt;
  int prev = 0, sh = 14;
  for (int k = 0; ok && k < cnt; ++k) {
    const int m = members[lo + k], blk = m / RB;
    int pos = -1;
#pragma unroll
    for (int q = 0; q < GRP_BLOCKS; ++q) if (blk == gb[q]) pos = q * RB + m - blk * RB;
    if (pos < 0) { ok = false; break; }
    if (k == 0) code |= (unsigned long long)pos << 4;
    else { const int d = pos - prev; if (d <= 0 || d >= 1024) { ok = false; break; } code |= (unsigned long long)d << sh; sh += 10; }
    prev = pos;
  }
  if (ok) { acode[a] = code; return; }
  acode[a] = 0ull;
  const int q = atomicAdd(nstray, 1);
  if (q < stray_cap) stray[q] = a;
  for (int k = 0; k < cnt; ++k) { const int m = members[lo + k]; atomicOr(&wmask[m >> 5], 1u << (m & 31)); }
}
__global__ void restrict_stray_kernel(int ns, const int *__restrict__ stray, const int *__restrict__ cptr, const int *__restrict__ members,
                                      const double *__restrict__ r, double *__restrict__ rc) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= ns) return;
  const int a = stray[q];
  double s = 0.0;
  for (int k = cptr[a], e = cptr[a + 1]; k < e; ++k) s += r[members[k]];
  rc[a] = s;
}

// the grouped pass itself: body of csr_rowblock_coded_kernel<RESIDUAL> per row block (coded table, uncoded index slice, or the
// unstaged walk — block-uniform choices), then the in-LDS restriction of the group's aggregates
// (six waves per SIMD: the halo variants of U = 7 / 8 came out at 82 / 89 registers — one wave less than the 80 of the others — and ran 6 % behind
// their share on a row shard)
// ND (option pre_nodiag; unsharded FP64 levels whose rows hold exactly one diagonal entry): Â's diagonal entry is fl(a_ii·fl(ω·fl(1/a_ii))), ω up to
// three roundings whatever the coefficients, so it is not streamed as a double.  A coded + staged block stages its slice of val_nd (Â's values
// without the diagonal entries: row i from rowptr[i] − i, block blk from lo − r0 to hi − r1) and walks the pattern as before; at the offset 0 the
// value is rebuilt from omega and the row's byte of nd_code (the distance of the stored entry from omega in units of the last place, taken on
// the bit patterns) and multiplies b_i — no LDS value, no gather — and behind it the value index is the pattern position minus one.  The rebuilt
// value IS the stored one, so the sum keeps its bits; the other branches read val as they always did.
// PK (option pack7; unsharded FP64 levels): a coded + staged block whose pk_e0 entry is not −1 stages its slice of the packed copy pk of the operand it
// streams (val_nd with ND, val otherwise) and fetches its values through pk7_fetch; see coded_block_body.
template <int U, bool HALO, class VT = double, bool ND = false, bool PK = false>
// (PK with U = 8 needs more than the 80 registers of six waves: five there, instead of a bound that spills)
__global__ __launch_bounds__(RB) __attribute__((amdgpu_waves_per_eu(PK && U == 8 ? 5 : 6))) void csr_group_pre_kernel(
    int n, const int *__restrict__ rowptr, const int *__restrict__ idx, const VT *__restrict__ val,
    const unsigned char *__restrict__ pid, const int *__restrict__ tptr, const int *__restrict__ tab,
    const double *__restrict__ x, const double *__restrict__ b, double *__restrict__ t_out, double *__restrict__ r_out,
    double *__restrict__ rc_out, const int *__restrict__ gdesc, const unsigned long long *__restrict__ acode,
    const unsigned *__restrict__ wmask, int capv, int capi, BlockMap bm, const double *__restrict__ hv, int split, int nts /*bit 0: streaming store of t; bit 1: slice staged by LDS-DMA, no loop; bit 2: option rowptr_scan*/,
    const int *__restrict__ gorder, int gper, const double *__restrict__ val_nd, const signed char *__restrict__ nd_code, double omega,
    const unsigned char *__restrict__ pk, const int *__restrict__ pk_e0) {
  extern __shared__ double lds_raw[];
  static_assert(!PK || (sizeof(VT) == 8 && !HALO), "packed values: unsharded FP64 levels only");
  constexpr int VA = val_traits<VT>::VA;
  typedef typename val_traits<VT>::v16 v16_t;
  typedef typename val_traits<VT>::i16 i16_t;
  static_assert(sizeof(VT) == 8 || !HALO, "float values: unsharded levels only");
  static_assert(!ND || (sizeof(VT) == 8 && !HALO), "no streamed diagonal: unsharded FP64 levels only");
  int g;
  if (gorder) {        // option group_order: workgroup (xcd, idx) → group, in the order of the one-block kernels' plane sweep
    const int idx = blockIdx.x >> 3;
    if (idx >= gper) return;
    g = gorder[(blockIdx.x & 7) * gper + idx];
  } else g = map_block(bm, blockIdx.x);
  if (g < 0) return;
  const int tid = threadIdx.x;
  VT *__restrict__ vals = reinterpret_cast<VT *>(lds_raw);                                // capv + 2 doubles (capv + 8 floats)
  int *__restrict__ ints = reinterpret_cast<int *>(lds_raw + val_region<VT>(capv));       // capi ints: the block's table, or its index slice
  double *__restrict__ rbuf = lds_raw + val_region<VT>(capv) + (capi + 1) / 2;            // residuals of the group's row blocks
  // group descriptor (one 128-byte record, no dependent loads behind it): blocks, their entry bounds, their aggregate ranges
  const int4_t *__restrict__ gd = reinterpret_cast<const int4_t *>(gdesc + (size_t)GRP_DESC * g);
  const int4_t gb = gd[0], glo = gd[1], ghi = gd[2], galo = gd[3], gahi = gd[4];
#define GSEL(v, h) ((h) == 0 ? (v).x : ((h) == 1 ? (v).y : ((h) == 2 ? (v).z : (v).w)))
  // member codes of this lane's first aggregate per block: in flight while the blocks are swept
  unsigned long long code0[GRP_BLOCKS];
#pragma unroll
  for (int h = 0; h < GRP_BLOCKS; ++h) { const int a = GSEL(galo, h) + tid; code0[h] = (GSEL(gb, h) >= 0 && a < GSEL(gahi, h)) ? acode[a] : 0ull; }
#pragma unroll
  for (int h = 0; h < GRP_BLOCKS; ++h) {
    const int blk = GSEL(gb, h);
    if (blk < 0) break;                                                   // group-uniform
    if (h) __syncthreads();                                               // the previous block's LDS slice is done with
    const int r0 = blk * RB, r1 = min(r0 + RB, n);
    const int lo = GSEL(glo, h), hi = GSEL(ghi, h);
    const int t0 = tptr ? tptr[blk] : 0, tlen = tptr ? tptr[blk + 1] - t0 : 0;
    const int row = r0 + tid, start = lo & ~(VA - 1), nent = hi - start;
    const bool coded = tlen > 0 && tlen <= capi;
    const bool staged = hi - lo <= capv && (coded || nent + VA - 1 <= capi);   // block-uniform
    int ga = 0, ge = 0;
    double bi = 0.0;
    unsigned wm = 0u;
    int mypid = 0;                                                        // loaded with the other per-row loads, not behind the barrier
    int dc = 0;                                                           // ND: the row's diagonal entry of Â, as its distance from omega
    const bool scan = coded && staged && (nts & 4);                       // block-uniform (coded_row_range)
    int wave_first = 0;
    if (scan) wave_first = rowptr[min(r0 + (tid & ~63), n)];
    if (row < r1) { if (!scan) { ga = rowptr[row]; ge = rowptr[row + 1]; } bi = b[row]; wm = wmask[row >> 5]; if (coded) mypid = pid[row]; if (ND && coded) dc = nd_code[row]; }
    double s = 0.0;
    // ND, coded block: its slice of val_nd (256 entries less; r1 − r0 less in the last block)
    const int nd_start = (lo - r0) & ~1, nd_nent = (hi - r1) - nd_start;
    // PK: the block's slice [pk_a, pk_b) of the packed operand, its records, and whether the block runs on them (block-uniform)
    int pk_a = 0, pk_nrec = 0, pk_e = -1, pk_sh = 0;
    bool packed = false;
    if constexpr (PK) {
      pk_a = ND ? lo - r0 : lo;
      pk_nrec = (((ND ? hi - r1 : hi) + 15) >> 4) - (pk_a >> 4);
      pk_e = pk_e0[blk];
      packed = coded && staged && pk_e >= 0 && 14 * pk_nrec <= val_region<VT>(capv);
      pk_sh = (ND ? nd_start : start) - (pk_a & ~15);      // the packed slice starts at a multiple of 16 entries
    }
    const unsigned char *__restrict__ pvals = reinterpret_cast<const unsigned char *>(lds_raw);
    const unsigned pk_e0sh = (unsigned)pk_e << 20;
    if (staged) {
      const int nch = (PK && packed) ? 7 * pk_nrec : ((ND && coded) ? (nd_nent + 1) >> 1 : (nent + VA - 1) >> (VA == 4 ? 2 : 1));      // 16-byte pieces of the value slice
      if (coded && nch <= 4 * RB && (nts & 2)) {          // no loop and no staging registers in front of the barrier (see coded_block_body)
        if (PK && packed) stage_pairs_dma(reinterpret_cast<const double *>(pk + (size_t)112 * (size_t)(pk_a >> 4)), reinterpret_cast<double *>(vals), nch, tid);
        else if (ND) stage_pairs_dma(val_nd + nd_start, reinterpret_cast<double *>(vals), nch, tid);
        else stage_pairs_dma(val + start, vals, nch, tid);
        int tw = 0;
        if (tid < tlen) tw = tab[t0 + tid];
        if (tid < tlen) ints[tid] = tw;
        for (int c = tid + RB; c < tlen; c += RB) ints[c] = tab[t0 + c];
        // LDS-DMA transfers are vector-memory operations of the issuing wave: the workgroup barrier's fence does not cover them, so every
        // wave drains its own before it arrives (spelled out; the compiler happens to place the same wait in front of s_barrier today)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      } else if (coded) {
        const VT *__restrict__ src = (PK && packed) ? reinterpret_cast<const VT *>(pk + (size_t)112 * (size_t)(pk_a >> 4))
                                                    : (ND ? reinterpret_cast<const VT *>(val_nd) + nd_start : val + start);
#pragma unroll 4
        for (int c = tid; c < nch; c += RB) *reinterpret_cast<v16_t *>(vals + VA * c) = *reinterpret_cast<const v16_t *>(src + VA * c);
        for (int c = tid; c < tlen; c += RB) ints[c] = tab[t0 + c];
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
      if (row < r1 && ge > ga) {
        const int my_a = ga - start, my_e = ge - start, lim = nent - 1;
        if (ND && coded) {
          const int ps = ints[mypid];
          const int last = ge - ga - 1;
          const int na = ga - row - nd_start, nlim = max(nd_nent - 1, 0);      // the row's first off-diagonal value in the staged slice
          int behind = 0;                                                       // 1 once the walk has passed the diagonal
          const double om = __longlong_as_double(__double_as_longlong(omega) + (long long)dc);      // Â_ii as val holds it
          if (PK && packed) {      // the same walk, every value through pk7_fetch
            for (int k = ga, j = 0; k < ge; k += U, j += U) {
              int oq[U], bq[U]; double xv[U], vq[U];
#pragma unroll
              for (int q = 0; q < U; ++q) oq[q] = ints[ps + min(j + q, last)];
#pragma unroll
              for (int q = 0; q < U; ++q) { bq[q] = behind; if (oq[q] == 0) behind = 1; }
#pragma unroll
              for (int q = 0; q < U; ++q) xv[q] = oq[q] == 0 ? bi : x[row + oq[q]];
#pragma unroll
              for (int q = 0; q < U; ++q) { const double v = pk7_fetch(pvals, min(na + j + q - bq[q], nlim) + pk_sh, pk_e0sh); vq[q] = oq[q] == 0 ? om : v; }
#pragma unroll
              for (int q = 0; q < U; ++q) s += (k + q < ge) ? vq[q] * xv[q] : 0.0;
            }
          } else
          for (int k = ga, j = 0; k < ge; k += U, j += U) {
            int oq[U], bq[U]; double xv[U], vq[U];
#pragma unroll
            for (int q = 0; q < U; ++q) oq[q] = ints[ps + min(j + q, last)];
#pragma unroll
            for (int q = 0; q < U; ++q) { bq[q] = behind; if (oq[q] == 0) behind = 1; }
#pragma unroll
            for (int q = 0; q < U; ++q) xv[q] = oq[q] == 0 ? bi : x[row + oq[q]];
#pragma unroll
            for (int q = 0; q < U; ++q) { const double v = reinterpret_cast<const double *>(vals)[min(na + j + q - bq[q], nlim)]; vq[q] = oq[q] == 0 ? om : v; }
#pragma unroll
            for (int q = 0; q < U; ++q) s += (k + q < ge) ? vq[q] * xv[q] : 0.0;
          }
        } else if (coded) {
          const int ps = ints[mypid];
          const int last = my_e - my_a - 1;
          if (PK && packed) {      // the same walk, every value through pk7_fetch (PK: no halo)
            for (int k = my_a, j = 0; k < my_e; k += U, j += U) {
              int oq[U]; double xv[U], vq[U];
#pragma unroll
              for (int q = 0; q < U; ++q) oq[q] = ints[ps + min(j + q, last)];
#pragma unroll
              for (int q = 0; q < U; ++q) xv[q] = x[row + oq[q]];
#pragma unroll
              for (int q = 0; q < U; ++q) vq[q] = pk7_fetch(pvals, min(k + q, lim) + pk_sh, pk_e0sh);
#pragma unroll
              for (int q = 0; q < U; ++q) s += (k + q < my_e) ? vq[q] * xv[q] : 0.0;
            }
          } else
          for (int k = my_a, j = 0; k < my_e; k += U, j += U) {
            int oq[U]; double xv[U], vq[U];
#pragma unroll
            for (int q = 0; q < U; ++q) oq[q] = ints[ps + min(j + q, last)];
#pragma unroll
            for (int q = 0; q < U; ++q) {
              if (HALO && oq[q] >= CODE_HALO_LO) xv[q] = hv[row + (oq[q] - CODE_HALO)];
              else xv[q] = x[row + oq[q]];
            }
#pragma unroll
            for (int q = 0; q < U; ++q) vq[q] = vals[min(k + q, lim)];
#pragma unroll
            for (int q = 0; q < U; ++q) s += (k + q < my_e) ? vq[q] * xv[q] : 0.0;
          }
        } else {
          for (int k = my_a; k < my_e; k += U) {
            int cq[U]; double xv[U], vq[U];
#pragma unroll
            for (int q = 0; q < U; ++q) cq[q] = ints[min(k + q, lim)];
#pragma unroll
            for (int q = 0; q < U; ++q) xv[q] = (HALO && cq[q] >= split) ? hv[cq[q] - split] : x[cq[q]];
#pragma unroll
            for (int q = 0; q < U; ++q) vq[q] = vals[min(k + q, lim)];
#pragma unroll
            for (int q = 0; q < U; ++q) s += (k + q < my_e) ? vq[q] * xv[q] : 0.0;
          }
        }
      }
    } else if (row < r1) {
      for (int k = ga; k < ge; ++k) { const int c = idx[k]; s += (double)val[k] * ((HALO && c >= split) ? hv[c - split] : x[c]); }
    }
    // members of stray aggregates also store r — the whole wave does when one of its rows must: 64 consecutive doubles are four full
    // cache lines, while lone 8-byte stores each cost a read-modify-write of an ECC word in HBM.  The vote is taken BEFORE the stores:
    // read after them, the mask (a loaded value) made the compiler wait for vmcnt(0) behind the t store, i.e. for the store itself to
    // complete, once per row block of the sweep.
    const bool stray_wave = __any((int)((wm >> (row & 31)) & 1u)) != 0;
    if (row < r1) {
      const double r = bi - s;
      st_stream(t_out + row, bi + r, (nts & 1) != 0);
      rbuf[h * RB + tid] = r;
      if (stray_wave) r_out[row] = r;
    }
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < GRP_BLOCKS; ++h) {
    if (GSEL(gb, h) < 0) break;
    const int a0 = GSEL(galo, h) + tid, ae = GSEL(gahi, h);
    for (int a = a0; a < ae; a += RB) {
      const unsigned long long code = a == a0 ? code0[h] : acode[a];
      const int cnt = (int)(code & 15ull);
      if (cnt == 0) continue;
      int pos = (int)((code >> 4) & 1023ull), sh = 14;
      double sum = 0.0;
      sum += rbuf[pos];
      for (int k = 1; k < cnt; ++k, sh += 10) { pos += (int)((code >> sh) & 1023ull); sum += rbuf[pos]; }
      rc_out[a] = sum;
    }
  }
#undef GSEL
}

// Concurrent form for groups of at most two row blocks: a 512-thread workgroup, each half sweeps one block of the pair at the same
// time (own value/table slices in LDS), one barrier later all 512 threads restrict the group's aggregates.  Same phase structure as the
// plain row-block kernel plus one barrier (the sequential form above pays a second staging phase per extra block), same occupancy
// (2 × slice + 4 KB of LDS per workgroup → 4 workgroups = 32 waves per CU).  Every barrier sits outside the per-block branches.
template <int U, bool HALO>
__global__ __launch_bounds__(2 * RB) void csr_group2_pre_kernel(
    int n, const int *__restrict__ rowptr, const int *__restrict__ idx, const double *__restrict__ val,
    const unsigned char *__restrict__ pid, const int *__restrict__ tptr, const int *__restrict__ tab,
    const double *__restrict__ x, const double *__restrict__ b, double *__restrict__ t_out, double *__restrict__ r_out,
    double *__restrict__ rc_out, const int *__restrict__ gdesc, const unsigned long long *__restrict__ acode,
    const unsigned *__restrict__ wmask, int capv, int capi, BlockMap bm, const double *__restrict__ hv, int split) {
  extern __shared__ double lds_raw[];
  const int g = map_block(bm, blockIdx.x);
  if (g < 0) return;
  const int half = threadIdx.x >> 8, tid = threadIdx.x & (RB - 1);
  const int half_doubles = capv + 2 + (capi + 1) / 2;
  double *__restrict__ vals = lds_raw + half * half_doubles;
  int *__restrict__ ints = reinterpret_cast<int *>(vals + capv + 2);
  double *__restrict__ rbuf = lds_raw + 2 * half_doubles;                 // 2·RB residuals: block 0 of the pair, then block 1
  const int4_t *__restrict__ gd = reinterpret_cast<const int4_t *>(gdesc + (size_t)GRP_DESC * g);
  const int4_t gb = gd[0], glo = gd[1], ghi = gd[2], galo = gd[3], gahi = gd[4];
  const int blk = half ? gb.y : gb.x;                                      // −1: a single-block group, this half only helps to restrict
  const int a0 = (half ? galo.y : galo.x) + tid, ae = half ? gahi.y : gahi.x;
  const unsigned long long code0 = (blk >= 0 && a0 < ae) ? acode[a0] : 0ull;
  const int r0 = blk * RB, r1 = blk >= 0 ? min(r0 + RB, n) : 0;
  const int lo = half ? glo.y : glo.x, hi = half ? ghi.y : ghi.x;
  const int t0 = (tptr && blk >= 0) ? tptr[blk] : 0, tlen = (tptr && blk >= 0) ? tptr[blk + 1] - t0 : 0;
  const int row = r0 + tid, start = lo & ~1, nent = hi - start;
  const bool coded = tlen > 0 && tlen <= capi;
  const bool staged = blk >= 0 && hi - lo <= capv && (coded || nent + 1 <= capi);   // uniform per half
  int ga = 0, ge = 0;
  double bi = 0.0;
  unsigned wm = 0u;
  if (blk >= 0 && row < r1) { ga = rowptr[row]; ge = rowptr[row + 1]; bi = b[row]; wm = wmask[row >> 5]; }
  if (staged) {
    const int nch = (nent + 1) >> 1;
    if (coded) {
#pragma unroll 4
      for (int c = tid; c < nch; c += RB) *reinterpret_cast<double2_t *>(vals + 2 * c) = *reinterpret_cast<const double2_t *>(val + start + 2 * c);
      for (int c = tid; c < tlen; c += RB) ints[c] = tab[t0 + c];
    } else {
#pragma unroll 4
      for (int c = tid; c < nch; c += RB) {
        const int k = start + 2 * c;
        *reinterpret_cast<int2_t *>(ints + 2 * c) = *reinterpret_cast<const int2_t *>(idx + k);
        *reinterpret_cast<double2_t *>(vals + 2 * c) = *reinterpret_cast<const double2_t *>(val + k);
      }
    }
  }
  __syncthreads();
  double s = 0.0;
  if (blk >= 0 && row < r1) {
    if (staged) {
      if (ge > ga) {
        const int my_a = ga - start, my_e = ge - start, lim = nent - 1;
        if (coded) {
          const int ps = ints[pid[row]];
          const int last = my_e - my_a - 1;
          for (int k = my_a, j = 0; k < my_e; k += U, j += U) {
            int oq[U]; double xv[U], vq[U];
#pragma unroll
            for (int q = 0; q < U; ++q) oq[q] = ints[ps + min(j + q, last)];
#pragma unroll
            for (int q = 0; q < U; ++q) {
              if (HALO && oq[q] >= CODE_HALO_LO) xv[q] = hv[row + (oq[q] - CODE_HALO)];
              else xv[q] = x[row + oq[q]];
            }
#pragma unroll
            for (int q = 0; q < U; ++q) vq[q] = vals[min(k + q, lim)];
#pragma unroll
            for (int q = 0; q < U; ++q) s += (k + q < my_e) ? vq[q] * xv[q] : 0.0;
          }
        } else {
          for (int k = my_a; k < my_e; k += U) {
            int cq[U]; double xv[U], vq[U];
#pragma unroll
            for (int q = 0; q < U; ++q) cq[q] = ints[min(k + q, lim)];
#pragma unroll
            for (int q = 0; q < U; ++q) xv[q] = (HALO && cq[q] >= split) ? hv[cq[q] - split] : x[cq[q]];
#pragma unroll
            for (int q = 0; q < U; ++q) vq[q] = vals[min(k + q, lim)];
#pragma unroll
            for (int q = 0; q < U; ++q) s += (k + q < my_e) ? vq[q] * xv[q] : 0.0;
          }
        }
      }
    } else {
      for (int k = ga; k < ge; ++k) { const int c = idx[k]; s += val[k] * ((HALO && c >= split) ? hv[c - split] : x[c]); }
    }
    const double r = bi - s;
    t_out[row] = bi + r;
    rbuf[half * RB + tid] = r;
  }
  if (__any((int)((wm >> (row & 31)) & 1u)) && blk >= 0 && row < r1) r_out[row] = bi - s;   // whole waves: see csr_group_pre_kernel
  __syncthreads();
  for (int a = a0; a < ae; a += RB) {                                      // this half's block's aggregates; positions span both halves
    const unsigned long long code = a == a0 ? code0 : acode[a];
    const int cnt = (int)(code & 15ull);
    if (cnt == 0) continue;
    int pos = (int)((code >> 4) & 1023ull), sh = 14;
    double sum = 0.0;
    sum += rbuf[pos];
    for (int k = 1; k < cnt; ++k, sh += 10) { pos += (int)((code >> sh) & 1023ull); sum += rbuf[pos]; }
    rc_out[a] = sum;
  }
}

// ------------------------------------------------------------------ host grouping: the steps of mgs_build_groups, each from plain vectors to plain vectors
struct GrpLink { int cnt, a, b; };      // cnt aggregates that start in row block a reach row block b > a

// 1. links from the votes (grp_scan_kernel's vkey / vcnt, GRP_SLOTS per row block): per block ascending in b, so the whole list is (a, b)-ascending
std::vector<GrpLink> grp_links(int nblocks, const std::vector<int> &vkey, const std::vector<int> &vcnt, int min_link) {
  std::vector<GrpLink> raw;
  for (int b = 0; b < nblocks; ++b) {
    GrpLink mine[GRP_SLOTS]; int nm = 0;
    for (int sl = 0; sl < GRP_SLOTS; ++sl) {
      const int k = vkey[(size_t)b * GRP_SLOTS + sl], c = vcnt[(size_t)b * GRP_SLOTS + sl];
      // option group_min_link: only links that carry a share of the block's aggregates (default 1 = every link; see mgs_internal.hpp)
      if (k > b && k < nblocks && c >= min_link) mine[nm++] = {c, b, k};
    }
    std::sort(mine, mine + nm, [](const GrpLink &p, const GrpLink &q) { return p.b < q.b; });
    for (int q = 0; q < nm; ++q) raw.push_back(mine[q]);
  }
  return raw;
}
// 2. counting sort and union: greedy union of row blocks along their most frequent links, groups of at most max_blocks blocks (deterministic:
// links sorted by count, then by block pair).  Returns the root of every block's group = the group's smallest block.
std::vector<int> grp_union(int nblocks, const std::vector<GrpLink> &raw, int max_blocks) {
  std::vector<GrpLink> links(raw.size());
  {   // order: count descending, then (a, b) ascending — raw is already (a, b)-ascending, so a stable counting sort by count does it
      // (a count is at most the 256 aggregates that can start in one row block; half a million blocks at 512³: no comparison sort)
    std::vector<size_t> start((size_t)RB + 2, 0);
    for (const GrpLink &l : raw) ++start[(size_t)(RB - std::min(l.cnt, RB)) + 1];
    for (size_t q = 1; q < start.size(); ++q) start[q] += start[q - 1];
    for (const GrpLink &l : raw) links[start[(size_t)(RB - std::min(l.cnt, RB))]++] = l;
  }
  std::vector<int> parent((size_t)nblocks), gsize((size_t)nblocks, 1);
  for (int b = 0; b < nblocks; ++b) parent[b] = b;
  auto find = [&](int v) { while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; } return v; };
  for (const GrpLink &l : links) {
    int ra = find(l.a), rb = find(l.b);
    if (ra == rb || gsize[ra] + gsize[rb] > max_blocks) continue;
    if (ra > rb) std::swap(ra, rb);
    parent[rb] = ra; gsize[ra] += gsize[rb];                              // root = smallest block of the group
  }
  std::vector<int> root((size_t)nblocks);
  for (int b = 0; b < nblocks; ++b) root[b] = find(b);
  return root;
}
// 3. group lists (GRP_BLOCKS slots per group, −1: none; groups in ascending order of their smallest block, blocks inside a group ascending) and
// every block's group (blk2grp) ...
std::vector<int> grp_lists(const std::vector<int> &root, std::vector<int> &blk2grp) {
  const int nblocks = (int)root.size();
  std::vector<int> gid((size_t)nblocks, -1);
  int ng = 0;
  for (int b = 0; b < nblocks; ++b) if (root[b] == b) gid[b] = ng++;
  std::vector<int> gblk((size_t)ng * GRP_BLOCKS, -1), fill((size_t)ng, 0);
  blk2grp.assign((size_t)nblocks, -1);
  for (int b = 0; b < nblocks; ++b) { const int g = gid[root[b]]; blk2grp[b] = g; gblk[(size_t)g * GRP_BLOCKS + fill[g]++] = b; }
  return gblk;
}
// ... and the plane distance: in groups, between a group and the one whose first block lies one far-band period (Db row blocks) further (middle of the matrix)
int grp_plane_distance(const std::vector<int> &gblk, int Db) {
  const int ng = (int)(gblk.size() / GRP_BLOCKS), gm = ng / 2, fb = gblk[(size_t)gm * GRP_BLOCKS];
  int lo_g = gm, hi_g = ng;
  while (lo_g < hi_g) { const int mid = (lo_g + hi_g) / 2; if (gblk[(size_t)mid * GRP_BLOCKS] < fb + Db) lo_g = mid + 1; else hi_g = mid; }
  return lo_g - gm;
}
// 4. descriptors: everything a workgroup needs about its blocks in one record of GRP_DESC ints — blocks, entry bounds lo / hi (blkptr), aggregate
// ranges lo / hi (afirst); *max_blocks: blocks of the largest group
std::vector<int> grp_descriptors(const std::vector<int> &gblk, const std::vector<int> &blkptr, const std::vector<int> &afirst, int *max_blocks) {
  const int ng = (int)(gblk.size() / GRP_BLOCKS);
  std::vector<int> desc((size_t)ng * GRP_DESC, -1);
  int maxb = 1;
  for (int g = 0; g < ng; ++g)
    for (int q = 0; q < GRP_BLOCKS; ++q) {
      const int b = gblk[(size_t)g * GRP_BLOCKS + q];
      int *d = &desc[(size_t)g * GRP_DESC];
      d[q] = b; d[4 + q] = b >= 0 ? blkptr[b] : 0; d[8 + q] = b >= 0 ? blkptr[b + 1] : 0; d[12 + q] = b >= 0 ? afirst[b] : 0; d[16 + q] = b >= 0 ? afirst[b + 1] : 0;
      if (b >= 0) maxb = std::max(maxb, q + 1);
    }
  *max_blocks = maxb;
  return desc;
}
// 5. order table (option group_order = S): the groups in the order in which the one-block kernels sweep their FIRST blocks — XCD-contiguous ranges of
// row blocks, inside a range strip-major: a strip of S row blocks followed through every plane (period Db blocks) of the range.  8 rows of *per_xcd
// groups, −1: none.
std::vector<int> grp_order(const std::vector<int> &gblk, int nblocks, int Db, int S, int *per_xcd) {
  const int ng = (int)(gblk.size() / GRP_BLOCKS), chunkB = (nblocks + 7) / 8;
  std::vector<std::vector<std::pair<long long, int>>> per(8);
  for (int g = 0; g < ng; ++g) {
    const int fb = gblk[(size_t)g * GRP_BLOCKS], xcd = std::min(fb / chunkB, 7), lb = fb - xcd * chunkB;
    const long long p = lb / Db, off = lb % Db, st = off / S, t = off % S;
    per[(size_t)xcd].push_back({(st * (long long)(chunkB / Db + 2) + p) * S + t, g});
  }
  size_t mx = 0;
  for (auto &v : per) { std::sort(v.begin(), v.end()); mx = std::max(mx, v.size()); }
  std::vector<int> order(8 * mx, -1);
  for (int x = 0; x < 8; ++x) for (size_t q = 0; q < per[(size_t)x].size(); ++q) order[(size_t)x * mx + q] = per[(size_t)x][q].second;
  *per_xcd = (int)mx;
  return order;
}
// the device scratch of mgs_build_groups: freed on every exit
struct GrpScratch {
  int *vkey = nullptr, *vcnt = nullptr, *flags = nullptr, *blk2grp = nullptr;
  ~GrpScratch() { if (vkey) mgs_hip_free(vkey); if (vcnt) mgs_hip_free(vcnt); if (flags) mgs_hip_free(flags); if (blk2grp) mgs_hip_free(blk2grp); }
};

}  // namespace

void mgs_free_groups(mgs_groups *g) {
  if (!g) return;
  if (g->gblk) mgs_hip_free(g->gblk); if (g->afirst) mgs_hip_free(g->afirst); if (g->acode) mgs_hip_free(g->acode); if (g->gdesc) mgs_hip_free(g->gdesc);
  if (g->wmask) mgs_hip_free(g->wmask); if (g->stray) mgs_hip_free(g->stray); if (g->gorder) mgs_hip_free(g->gorder);
  delete g;
}
// Pairs the row blocks of A along its aggregates (see csr_group_pre_kernel).  *out stays NULL when the level does not
// qualify: general P, aggregate ids not ascending with their first member, long rows, or more than opt_group_stray_pct % strays.
int mgs_build_groups(mgs_ctx *ctx, const mgs_csr *A, const mgs_xfer *T, mgs_groups **out) {
  *out = nullptr;
  const int n = A->rows, nc = T ? T->n_coarse : 0;
  if (!T || !T->aggregation || n <= 0 || nc <= 0 || A->max_row_len > 64 || !A->blkptr || A->lds_cap <= 0) return MGS_OK;
  const int nblocks = mgs_row_blocks(A);
  if (nblocks < ctx->opt_group_min_blocks) return MGS_OK;      // small levels: too few workgroups once blocks are grouped
  hipStream_t st = ctx->stream;
  mgs_groups *G = new mgs_groups();
  G->nblocks = nblocks;
  GrpScratch s;
  const size_t nv = (size_t)nblocks * GRP_SLOTS;
  int rc = mgs_dev_alloc(ctx, &s.vkey, nv);
  if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &s.vcnt, nv);
  if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &s.flags, 2);
  if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &G->afirst, (size_t)nblocks + 1);
  std::vector<int> hk(nv), hn(nv);
  int hflags[2] = {0, 0};
  if (rc == MGS_OK) {
    hipMemsetAsync(s.vkey, 0xff, sizeof(int) * nv, st);                  // −1: empty slot
    hipMemsetAsync(s.vcnt, 0, sizeof(int) * nv, st);
    hipMemsetAsync(s.flags, 0, 2 * sizeof(int), st);
    hipLaunchKernelGGL(grp_scan_kernel, dim3((nc + RB - 1) / RB), dim3(RB), 0, st, nc, T->cptr, T->members, nblocks, s.vkey, s.vcnt, G->afirst, s.flags);
    hipMemcpyAsync(hk.data(), s.vkey, sizeof(int) * nv, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(hn.data(), s.vcnt, sizeof(int) * nv, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(hflags, s.flags, sizeof hflags, hipMemcpyDeviceToHost, st);
    if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) rc = mgs_fail(ctx, MGS_ERR_HIP, "row-block grouping (scan) failed");
  }
  bool usable = rc == MGS_OK && hflags[0] == 0;
  if (usable) {
    const int Db = (A->far_band + RB - 1) / RB;
    std::vector<int> hb2g;
    const std::vector<int> hg = grp_lists(grp_union(nblocks, grp_links(nblocks, hk, hn, ctx->opt_group_min_link),
                                                    std::min(std::max(ctx->opt_group_blocks, 1), GRP_BLOCKS)), hb2g);
    G->ngroups = (int)(hg.size() / GRP_BLOCKS);
    G->plane_groups = grp_plane_distance(hg, Db);
    const int stray_cap = std::max((int)((int64_t)nc * std::min(std::max(ctx->opt_group_stray_pct, 0), 100) / 100), 1);
    rc = mgs_dev_alloc(ctx, &G->gblk, hg.size());
    if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &s.blk2grp, (size_t)nblocks);
    if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &G->acode, (size_t)nc);
    if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &G->wmask, (size_t)(n + 31) / 32 + 1);
    if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &G->stray, (size_t)stray_cap);
    if (rc == MGS_OK) {
      hipMemcpyAsync(G->gblk, hg.data(), sizeof(int) * hg.size(), hipMemcpyHostToDevice, st);
      hipMemcpyAsync(s.blk2grp, hb2g.data(), sizeof(int) * (size_t)nblocks, hipMemcpyHostToDevice, st);
      hipMemsetAsync(G->wmask, 0, sizeof(unsigned) * ((size_t)(n + 31) / 32 + 1), st);
      hipLaunchKernelGGL(grp_code_kernel, dim3((nc + RB - 1) / RB), dim3(RB), 0, st, nc, T->cptr, T->members, s.blk2grp, G->gblk, G->acode, G->wmask,
                         G->stray, stray_cap, s.flags + 1);
      hipMemcpyAsync(hflags, s.flags, sizeof hflags, hipMemcpyDeviceToHost, st);
      if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) rc = mgs_fail(ctx, MGS_ERR_HIP, "row-block grouping (codes) failed");
    }
    G->nstray = hflags[1];
    usable = rc == MGS_OK && G->nstray <= stray_cap;
    if (usable) {
      std::vector<int> hbp((size_t)nblocks + 1), haf((size_t)nblocks + 1);
      hipMemcpyAsync(hbp.data(), A->blkptr, sizeof(int) * ((size_t)nblocks + 1), hipMemcpyDeviceToHost, st);
      hipMemcpyAsync(haf.data(), G->afirst, sizeof(int) * ((size_t)nblocks + 1), hipMemcpyDeviceToHost, st);
      if (hipStreamSynchronize(st) != hipSuccess) rc = mgs_fail(ctx, MGS_ERR_HIP, "row-block grouping (descriptors) failed");
      std::vector<int> hd;
      if (rc == MGS_OK) hd = grp_descriptors(hg, hbp, haf, &G->max_blocks);
      const int S = ctx->opt_group_order;
      if (rc == MGS_OK && S > 0 && Db >= 512 && (nblocks + 7) / 8 >= 2 * Db) {
        const std::vector<int> ho = grp_order(hg, nblocks, Db, S, &G->gorder_per_xcd);
        rc = mgs_dev_alloc(ctx, &G->gorder, ho.size());
        if (rc == MGS_OK && hipMemcpy(G->gorder, ho.data(), sizeof(int) * ho.size(), hipMemcpyHostToDevice) != hipSuccess) rc = mgs_fail(ctx, MGS_ERR_HIP, "row-block grouping: order table upload failed");
      }
      if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &G->gdesc, hd.size());
      if (rc == MGS_OK && hipMemcpy(G->gdesc, hd.data(), sizeof(int) * hd.size(), hipMemcpyHostToDevice) != hipSuccess) rc = mgs_fail(ctx, MGS_ERR_HIP, "row-block grouping: descriptor upload failed");
      usable = rc == MGS_OK;
    }
  }
  if (getenv("MGS_DEBUG_GROUPS"))
    fprintf(stderr, "[mgs groups] n=%d nc=%d blocks=%d: ids ascending=%d groups=%d strays=%d (limit %d%%) -> %s\n", n, nc, nblocks, hflags[0] == 0,
            G->ngroups, G->nstray, ctx->opt_group_stray_pct, usable ? "grouped" : "separate kernels");
  if (!usable) { mgs_free_groups(G); return rc; }
  *out = G;
  return MGS_OK;
}

int mgs_launch_group_pre(const mgs_csr *A, const mgs_groups *G, const mgs_xfer *T, const double *x, const double *b,
                         double *t_out, double *r_out, double *rc_out, const double *hv, int split, const double *val_nd, const signed char *nd_code, double omega,
                         mgs_pack7 *pk) {
  mgs_ctx *ctx = A->ctx;
  if (A->rows == 0 || G->ngroups == 0) return MGS_OK;
  const mgs_rowcode *c = (use_rowcode(A, A->code, hv != nullptr) && !A->code->vtab) ? A->code : nullptr;
  const bool f32 = A->val32 != nullptr;      // FP32 level: the float form (unsharded levels only, the caller sees to that)
  if (f32 && hv) return mgs_fail(ctx, MGS_ERR_INVALID, "grouped pre pass: FP32 operand values on a row shard");
  if (val_nd && (f32 || hv || !nd_code)) return mgs_fail(ctx, MGS_ERR_INVALID, "grouped pre pass: the operand without diagonal serves unsharded FP64 levels only");
  if (f32) { nd_code = nullptr; omega = 0.0; }      // the float form knows no operand without diagonal
  // LDS: the coded kernels' two regions (the integer one rounded up to 8 bytes) and, behind them, the residuals of the group's row blocks
  const coded_lds l = coded_budget(A, c, f32);
  const size_t regions = l.val_bytes + ((l.int_bytes + 7) & ~(size_t)7);
  BlockMap bm;
  dim3 grid = plan_group_map(A, G, bm);
  const bool pairs = G->max_blocks <= 2 && ctx->opt_group_concurrent && !f32;     // 512 threads, both blocks of a pair at once (FP64 values only)
  const bool ordered = !pairs && G->gorder && ctx->opt_group_order > 0 && ctx->opt_xcd_remap;
  if (ordered) grid = dim3(8 * G->gorder_per_xcd);
  // option pack7: a packed copy of the operand the coded blocks stream (val_nd or Â's values), in step with it
  const bool packed = mgs_pack7_serves(pk, val_nd != nullptr) && ctx->opt_pack7 && c && !f32 && !hv && !pairs;
  if (pk) pk->ran = packed ? 1 : 0;
  // the pair kernel's parameters are the leading ones of the one-block kernel's; `more`: what the latter takes behind them
  auto launch = [&](auto kernel, auto vals, int threads, size_t lds, auto... more) {
    hipLaunchKernelGGL(kernel, grid, dim3(threads), lds + l.pad_bytes, ctx->stream, A->rows, A->rowptr, A->col, vals, c ? c->pid : nullptr,
                       c ? c->tptr : nullptr, c ? c->tab : nullptr, x, b, t_out, r_out, rc_out, G->gdesc, G->acode, G->wmask, l.capv, l.capi, bm, hv,
                       hv ? split : 0x7fffffff, more...);
  };
  with_width<false>(gather_width(A), [&](auto U) {
    constexpr int UU = decltype(U)::value;
    if (pairs) {
      with_bool(hv != nullptr, [&](auto H) { launch(csr_group2_pre_kernel<UU, decltype(H)::value>, (const double *)A->val, 2 * RB, 2 * regions + 2 * RB * 8); });
      report_launch(ctx, 7, UU, 0, l.capv, l.capi, 0, c ? c->tptr : nullptr);      // the pair kernel reads Â's FP64 values as they are: neither ND nor PK
      return;
    }
    auto form = [&](auto H, auto ND, auto PK, auto vals) {      // (HALO, ND) ∈ {(true, false), (false, true), (false, false)} for double, neither for float; PK without HALO, for double
      launch(csr_group_pre_kernel<UU, decltype(H)::value, pointee_t<decltype(vals)>, decltype(ND)::value, decltype(PK)::value>, vals, RB,
             regions + (size_t)G->max_blocks * RB * 8, kernel_flags(ctx, nt_store_on(A), true), ordered ? G->gorder : nullptr, G->gorder_per_xcd,
             val_nd, nd_code, omega, (const unsigned char *)(decltype(PK)::value ? pk->data : nullptr), (const int *)(decltype(PK)::value ? pk->e0 : nullptr));
    };
    const std::false_type no{};
    if (f32) form(no, no, no, A->val32);
    else if (hv) form(std::true_type{}, no, no, (const double *)A->val);
    else with_bool(val_nd != nullptr, [&](auto ND) { with_bool(packed, [&](auto PK) { form(no, ND, PK, (const double *)A->val); }); });
    report_launch(ctx, 6, UU, kernel_flags(ctx, nt_store_on(A), true), l.capv, l.capi, (f32 ? 1 : 0) | (val_nd ? 2 : 0) | (packed ? 4 : 0),
                  c ? c->tptr : nullptr);
  });
  MGS_HIP(ctx, hipGetLastError());
  if (G->nstray) {
    hipLaunchKernelGGL(restrict_stray_kernel, dim3((G->nstray + RB - 1) / RB), dim3(RB), 0, ctx->stream, G->nstray, G->stray, T->cptr, T->members, r_out, rc_out);
    MGS_HIP(ctx, hipGetLastError());
  }
  return MGS_OK;
}

// fused passes (see csr_rowblock_fused_kernel); returns MGS_ERR_STATE when the level cannot use them
int mgs_launch_fused(const mgs_csr *A, int which, const double *wd, const double *bvec, const double *xin, const int *agg,
                     const double *ec, double *out, double *out2) {
  return mgs_launch_fused_range(A, which, wd, bvec, xin, agg, ec, out, out2, nullptr, 0, mgs_row_blocks(A));
}
// row blocks [blk_lo, blk_hi); hv = values of the halo columns (nullptr for a square operator)
int mgs_launch_fused_range(const mgs_csr *A, int which, const double *wd, const double *bvec, const double *xin, const int *agg,
                           const double *ec, double *out, double *out2, const double *hv, int blk_lo, int blk_hi, int gap_at, int gap_len) {
  mgs_ctx *ctx = A->ctx;
  if (A->rows == 0 || blk_hi <= blk_lo) return MGS_OK;
  if (A->lds_cap <= 0 || (which == FUSE_PRE && A->rows != A->cols && !hv)) return MGS_ERR_STATE;   // (row shards: the pre pass reads its halo columns from the payload; the post passes gather e_c, halo room included)
  BlockMap bm;
  const dim3 grid = plan_block_map(A, blk_lo, blk_hi, gap_at, gap_len, bm);
  // FP32 level: post pass on the float copy of A·P's values (never the gather kernels, which read FP64 values)
  if (A->val32 && (which != FUSE_POST_MAPPED || hv)) return mgs_fail(ctx, MGS_ERR_INVALID, "FP32 operand values: fused pass %d has no float form", which);
  if (A->val32 || (which == FUSE_POST_MAPPED && use_rowcode(A, A->code)))      // A is the view whose col/code are the aggregate-mapped ones
    return launch_coded(A, A->code, FUSE_POST_MAPPED, A->col, ec, bvec, wd, 0.0, xin, agg, out, grid, bm);
  if (A->pk7) A->pk7->ran = 0;      // the gather kernel reads the FP64 values (mgs_hier_pack_info)
  const int cap = A->lds_cap;
  const size_t lds = (size_t)(cap + 2) * 12 + 16;
  with_fused_pass(which, [&](auto W) {
    hipLaunchKernelGGL((csr_rowblock_fused_kernel<decltype(W)::value>), grid, dim3(RB), lds, ctx->stream, A->rows, A->rowptr, A->col, A->val, wd, bvec,
                       xin, agg, ec, out, out2, cap, bm, hv, blkptr_opt(A));
  });
  report_launch(ctx, 0, 8, 0, cap, cap + 2);      // the gather kernel: steps of 8, index slice beside the values
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}
