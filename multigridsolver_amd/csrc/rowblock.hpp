// rowblock.hpp — what more than one unit of the row-block kernels needs: device helpers, the workgroup → row-block map, the pattern-code
// word format, the template fan-out and the host planners.  The units:
//   kernels_spmv.hip      what a SpMV, residual or Jacobi launch runs by default (slice kernel, pattern-coded kernel) and their launchers
//   kernels_variants.hip  the A/B-only forms of the same operators (option spmv_variant 2–4, 6, 7)
//   kernels_fused.hip     what only the fused cycle runs (gather kernel, grouped pre pass) and the host grouping
//   rowblock_setup.hip    what runs once per matrix (launch plan, pattern code)
//
// Design: AMG operators of PDE problems have 3..30 entries per row, so a
// wavefront-per-row kernel would idle ≥57 of 64 lanes.  One 256-thread workgroup owns 256
// consecutive rows ("row block") and stages the block's contiguous slice of val/col_idx in
// LDS with fully coalesced 16-/8-byte loads (every lane busy; plain loads — the non-temporal form
// measured 3 % slower here and stays an option).  Then lane t walks
// row t: the 64 lanes of a wave gather x[col] for 64 consecutive rows at once — contiguous
// runs of x for stencil-like operators — and add the products sequentially in ascending column
// order, the same order as Eigen's scalar loop
// (lib/Eigen/src/SparseCore/SparseDenseProduct.h:64-70), so the result is bit-identical to the
// CPU path; the epilogue (residual / damped Jacobi) is fused.  Row blocks whose slice does not
// fit the LDS budget (long rows) fall back, per block, to a sub-wavefront-per-row reduction with
// shuffles.  The workgroup→row-block map is XCD-contiguous (each of the 8 XCDs sweeps one eighth
// of the rows so re-read x planes stay in that XCD's 4 MiB L2), optionally strip-major.
// No MFMA: arithmetic intensity is 0.13 flop/B; the bound is HBM (≈8 TB/s peak).
//
// One definition: this header holds no __global__.  Every kernel template is defined and instantiated in exactly one .hip, because a second
// instantiation would be a second copy of the code in the library.  Everything here but BlockMap has internal linkage (each unit inlines its own
// copy, the library exports none of it); BlockMap is named in the signatures of the two launchers that cross unit boundaries (at the end).
#pragma once
#include "mgs_internal.hpp"

#include <algorithm>
#include <type_traits>

// Workgroup → row-block map.  (1) XCD-contiguous: workgroups are dealt round-robin over the 8
// XCDs, so XCD x = bid & 7 sweeps the x-th eighth of the row blocks.  (2) Optional strip-major
// sweep inside an XCD for operators with a far band at ±D row blocks (the e±N² planes of the
// 7-point stencil): instead of plane after plane, a strip of S row blocks is followed through all
// planes of the XCD's range, so x[e+N²] fetched for plane p is still in L2 when planes p+1 and
// p+2 need it as x[e] and x[e−N²].  Pure permutation: every row block is visited exactly once.
struct BlockMap { int nblocks, chunk, remap, D, S, P, base, gap_at = 0x7fffffff, gap_len = 0;
                  unsigned mps = 0, mS = 0; };   // ⌊2³²/(P·S)⌋+1 and ⌊2³²/S⌋+1: quotients by multiply-high — set by strip_map with D, S, P
// base: first row block of the launched range;
// row blocks >= gap_at are shifted by gap_len (one launch over the leading + trailing boundary blocks of a row shard)

namespace {

constexpr int RB = MGS_RB;      // rows per row block == threads per workgroup
constexpr int LDS_CAP_MAX = 5120;  // products (doubles) staged per block: 40 KiB → 4 blocks/CU

template <bool NT, class T>
__device__ __forceinline__ T ld_stream(const T *p) {
  if (NT) return __builtin_nontemporal_load(p);
  return *p;
}

// Streaming store of one output element per lane.  The builtin's hint does not survive here: both arms of `if (nt) nontemporal
// store else plain store` write the same value to the same address, the optimiser merges them into ONE plain store and the
// kernel never contained an `nt` store (seen in the ISA; the round-1/2 "nt_store is neutral" A/B compared identical code).  The
// instruction is spelled out instead.  Nothing in these kernels reads what it stored, so no wait count is owed.
__device__ __forceinline__ void st_stream(double *p, double v, bool nt) {
  if (nt) asm volatile("global_store_dwordx2 %0, %1, off nt" : : "v"(p), "v"(v) : "memory");
  else *p = v;
}

// Value slice of a row block straight from global memory into LDS (no VGPR in between, so nothing for the register allocator to
// keep alive or spill): piece p = 64 pairs = 1 KiB, wave w takes pieces w, w + 4, w + 8, w + 12; lane l of a piece moves pair 64p + l.
// Covers up to 1024 pairs (2048 doubles); the caller checks that.  The caller waits for its own transfers (s_waitcnt vmcnt(0), explicit)
// before the workgroup barrier that publishes the slice.
// VT = float (FP32 operand values): the same 16-byte transfers carry four floats each; `npairs` counts 16-byte pieces either way.
template <class VT>
__device__ __forceinline__ void stage_pairs_dma(const VT *__restrict__ src, VT *lds, int npairs, int tid) {
  constexpr int PER = 16 / (int)sizeof(VT);
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = wave + 4 * k;
    if (p * 64 + lane < npairs)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + PER * (p * 64 + lane)),
                                       (__attribute__((address_space(3))) void *)(lds + 64 * PER * p), 16, 0, 0);
  }
}

template <int OP>
__device__ __forceinline__ void epilogue(int row, double s, const double *__restrict__ x,
                                         const double *__restrict__ b, const double *__restrict__ dinv,
                                         double omega, double *__restrict__ out) {
  if (OP == MGS_OP_SPMV) out[row] = s;
  else if (OP == MGS_OP_RESIDUAL) out[row] = b[row] - s;
  else out[row] = x[row] + (omega * dinv[row]) * (b[row] - s);
}

// vector types for 16-byte wide streaming loads
typedef int int4_t __attribute__((ext_vector_type(4)));
typedef int int2_t __attribute__((ext_vector_type(2)));
typedef double double2_t __attribute__((ext_vector_type(2)));
typedef float float4_t __attribute__((ext_vector_type(4)));
// Value type of a matrix operand of the fused cycle passes (mgs_hier_set_operand_precision): double, or float for operands whose STORED
// values were rounded to FP32 at setup.  Only storage changes: a float value is widened before its product, every sum stays FP64 in the
// same order.  A 16-byte load carries VA values; the staged slice starts at an entry index that is a multiple of VA.
template <class VT> struct val_traits;
template <> struct val_traits<double> { typedef double2_t v16; typedef int2_t i16; static constexpr int VA = 2; };
template <> struct val_traits<float> { typedef float4_t v16; typedef int4_t i16; static constexpr int VA = 4; };
// doubles of LDS the value region of a row block takes: capv values + what the alignment of the slice's two ends adds
template <class VT> __host__ __device__ __forceinline__ int val_region(int capv) { return sizeof(VT) == 4 ? (capv + 8) >> 1 : capv + 2; }

// Option pack7: value e of a packed slice in LDS (112-byte records of sixteen entries: low dwords, 16-bit words of mantissa bits 32–47, bytes
// sign << 7 | (exponent − E0) << 4 | mantissa bits 48–51).  e0sh = E0 << 20.  Three LDS reads instead of one; the double is the stored one, bit for bit.
__device__ __forceinline__ double pk7_fetch(const unsigned char *__restrict__ lds, int e, unsigned e0sh) {
  const unsigned char *rec = lds + 112 * (e >> 4);
  const int i = e & 15;
  const unsigned lo = reinterpret_cast<const unsigned *>(rec)[i];
  const unsigned mid = reinterpret_cast<const unsigned short *>(rec + 64)[i];
  const unsigned b = rec[96 + i];
  return __hiloint2double((int)(((b & 0x80u) << 24) + ((b & 0x7fu) << 16) + e0sh + mid), (int)lo);
}

// the map itself (BlockMap, above)
__device__ __forceinline__ int block_of(const BlockMap &m, int vb) { const int b = m.base + vb; return b >= m.gap_at ? b + m.gap_len : b; }
__device__ __forceinline__ int map_block_xi(const BlockMap &m, int xcd, int idx);
__device__ __forceinline__ int map_block(const BlockMap &m, int bid) {
  if (!m.remap) return bid < m.nblocks ? bid : -1;
  return map_block_xi(m, bid & 7, bid >> 3);
}
__device__ __forceinline__ int map_block_xi(const BlockMap &m, int xcd, int idx) {
  int lb = idx;
  if (m.D > 0) {
    // Quotients by multiply-high (m.mps = ⌊2³²/(P·S)⌋+1, m.mS = ⌊2³²/S⌋+1; exact for idx·divisor < 2³², which the host checks — it
    // falls back to the plain XCD-contiguous map otherwise).  The two integer divisions this replaces compiled to ~65 dependent scalar
    // instructions at the head of EVERY wave, in front of its first load (and stayed there, if-converted, behind a run-time switch).
    const int ps = m.P * m.S;
    const int s = (int)__umulhi((unsigned)idx, m.mps), rem = idx - s * ps;
    const int p = (int)__umulhi((unsigned)rem, m.mS), t = rem - p * m.S;
    const int off = s * m.S + t;
    if (off >= m.D) return -1;
    lb = p * m.D + off;
  }
  if (lb >= m.chunk) return -1;
  const int vb = xcd * m.chunk + lb;
  return vb < m.nblocks ? vb : -1;
}

// ---------------------------------------------------------------------------------------------------------
// Pattern-coded rows (DESIGN.md §4 "pattern-coded index").  Operators of PDE problems repeat a handful of row
// shapes: the tuple (idx[k] − base(row))_k of a row — base(row) = row for the column array, agg[row] for the
// aggregate-mapped column array of the fused post pass — takes 3 distinct values in a 256-row block of the
// 7-point operator and a few dozen on the first Galerkin levels.  Setup dedupes the tuples per row block into a
// small table (`tab`: pstart[npat] then the tuples) and stores one byte per ROW (`pid`); the kernel then streams
// only the values (8 B per entry instead of 12) and rebuilds every index as base + tab[pstart[pid] + j] from LDS
// (lanes of a wave mostly read the same table word: LDS broadcast).  Same products in the same order → the results
// stay bit-identical to the CSR kernel.  Row blocks whose table would not pay (irregular rows) keep the index
// array (block-uniform branch), so any matrix is handled.
constexpr int CODE_NEG = (int)0x80000000;   // table word of a negative index (column not aggregated)
// Row shards: an index ≥ split addresses the halo payload hv[index − split].  Its table word is tagged and holds
// slot − row (constant along a plane boundary, where index − base is not): word = CODE_HALO + (slot − row).
constexpr int CODE_HALO = 0x60000000, CODE_HALO_LO = 0x50000000, CODE_OFF_MAX = 0x40000000;
// (a word outside the representable ranges makes the block uncodable: code_off of the setup returns CODE_BAD)
constexpr int CODE_BAD = 0x7fffffff;

// Inclusive prefix sum over the 64 lanes of a wave in six DPP adds (row_shr 1/2/4/8 inside the rows of 16 lanes, then row_bcast:15 into
// rows 1 and 3 and row_bcast:31 into rows 2 and 3 — the gfx9 scan; lanes without a source take the `old` operand, 0).  Every lane of
// the wave must be active.
__device__ __forceinline__ int wave_incl_scan(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
  return v;
}
// Entry range of a row of a CODED block without reading rowptr per row (option rowptr_scan): a pattern id fixes the row's length (the
// table holds the patterns back to back, ints[0] = their count), so a row starts at rowptr[first row of its wave] — one load per wave —
// plus the wave's prefix sum of lengths.  4 B per row less to stream.  Called by all lanes, behind the barrier that publishes the table.
__device__ __forceinline__ void coded_row_range(const int *__restrict__ ints, int tb, int tlen_blk, int mypid, bool valid, int wave_first, int &ga, int &ge) {
  int len = 0;
  if (valid) {
    const int np = ints[tb];
    const int p0 = ints[tb + mypid], p1 = (mypid + 1 < np) ? ints[tb + mypid + 1] : tlen_blk;
    len = p1 - p0;
  }
  const int incl = wave_incl_scan(len);
  ga = wave_first + incl - len; ge = wave_first + incl;
}

// ------------------------------------------------------------------ launch layer (host): what the units' launchers share; every launch decision is
// made in one function here or in one launcher of one unit
// Template fan-out: a run-time value reaches a kernel's template argument through one of these helpers, which calls f with the value as a
// std::integral_constant.  Each helper lists exactly the values its kernels are instantiated for.
template <int V> using int_c = std::integral_constant<int, V>;
template <class F> void with_bool(bool v, F f) { if (v) f(std::true_type{}); else f(std::false_type{}); }
// gather widths (gather_width below); FIVE: and the post pass's 5 (post_gather_width)
template <bool FIVE, class F> void with_width(int u, F f) {
  if constexpr (FIVE) { if (u == 5) return f(int_c<5>{}); }
  if (u == 4) f(int_c<4>{}); else if (u == 7) f(int_c<7>{}); else f(int_c<8>{});
}
// lanes per row of the long-row path
template <class F> void with_lanes(int n, F f) {
  if (n == 4) f(int_c<4>{}); else if (n == 8) f(int_c<8>{}); else if (n == 16) f(int_c<16>{}); else if (n == 32) f(int_c<32>{}); else f(int_c<64>{});
}
// the operator kernels' ops; false: op is none of them (f not called)
template <class F> bool with_csr_op(int op, F f) {
  if (op == MGS_OP_SPMV) f(int_c<MGS_OP_SPMV>{}); else if (op == MGS_OP_RESIDUAL) f(int_c<MGS_OP_RESIDUAL>{});
  else if (op == MGS_OP_JACOBI) f(int_c<MGS_OP_JACOBI>{}); else return false;
  return true;
}
// the gather kernel's passes
template <class F> void with_fused_pass(int which, F f) {
  if (which == FUSE_POST_MAPPED) f(int_c<FUSE_POST_MAPPED>{}); else if (which == FUSE_PRE) f(int_c<FUSE_PRE>{}); else f(int_c<FUSE_POST>{});
}
// value type of an operand's stored values from the pointer that carries them (A->val or A->val32)
template <class P> using pointee_t = std::remove_cv_t<std::remove_pointer_t<P>>;

inline double mean_row_len(const mgs_csr *A) { return A->rows ? (double)A->nnz / A->rows : 1.0; }
// U = gathers per step of the row walk: the typical row length (7-point stencils: exactly one step)
inline int gather_width(const mgs_csr *A) {
  const double mean_len = mean_row_len(A);
  return mean_len <= 4.5 ? 4 : (mean_len <= 7.5 && A->max_row_len <= 14 ? 7 : 8);
}
// post pass only: A·P of a 7-point operator with aggregates of four has 5 entries per row: one unrolled step of 5 instead of 7
inline int post_gather_width(const mgs_csr *A) {
  const double mean_len = mean_row_len(A);
  return mean_len > 4.5 && mean_len <= 5.5 && A->max_row_len <= 10 ? 5 : gather_width(A);
}
// lanes per row of the long-row path: next power of two ≥ mean row length, in [4,64]
inline int long_row_lanes(const mgs_csr *A) {
  const double mean = mean_row_len(A);
  int lanes = 4;
  while (lanes < 64 && lanes < mean) lanes <<= 1;
  return lanes;
}
// streaming stores of the output (option nt_store: operators with at least that many rows)
inline bool nt_store_on(const mgs_csr *A) { return A->ctx->opt_nt_store > 0 && A->rows >= A->ctx->opt_nt_store; }
// flags word of the row-block kernels.  bit 0 (`first`): the coded kernels (coded_block_body) — no row is longer than the gather width; the slice
// kernel and the grouped pre pass — streaming stores (nt_store_on).  bit 1: option stage_unroll.  bit 2: option rowptr_scan (the kernels that
// read a pattern code only: `coded`)
inline int kernel_flags(const mgs_ctx *ctx, bool first, bool coded) {
  return (first ? 1 : 0) | (ctx->opt_stage_unroll ? 2 : 0) | (coded && ctx->opt_rowptr_scan ? 4 : 0);
}
// row blocks of the slice kernel's launch take their bounds from the compact blkptr array (option blkptr; 0: from rowptr)
inline const int *blkptr_opt(const mgs_csr *A) { return A->ctx->opt_blkptr ? A->blkptr : nullptr; }

// strip-major sweep of period D (row blocks or groups) with strips of S: installs D, S, P and the multiply-high constants of
// map_block_xi and returns the workgroups per XCD — or leaves the plain XCD-contiguous map (returns bm.chunk) where a quotient would
// not be exact by multiply-high (idx·divisor ≥ 2³²: never at the sizes 288 GB hold, checked all the same)
inline int strip_map(BlockMap &bm, int D, int S) {
  const int P = (bm.chunk + D - 1) / D;
  const int per_xcd = ((D + S - 1) / S) * P * S;
  const unsigned long long ps = (unsigned long long)P * (unsigned long long)S;
  // (S < 2: ⌊2³²/1⌋+1 does not fit 32 bits — the multiply-high quotient would be 0 instead of the dividend; a strip of one block is
  // the plain plane-major order anyway, so the plain XCD-contiguous map serves)
  if (D <= 0 || S < 2 || ps < 2 || ((unsigned long long)per_xcd + 1) * ps >= (1ull << 32) || ps * (unsigned long long)S >= (1ull << 32)) { bm.D = bm.S = bm.P = 0; return bm.chunk; }
  bm.D = D; bm.S = S; bm.P = P;
  bm.mps = (unsigned)((1ull << 32) / ps) + 1u;
  bm.mS = (unsigned)((1ull << 32) / (unsigned long long)S) + 1u;
  return per_xcd;
}
// The one planner of a workgroup → unit map (units: row blocks, row-block groups, super blocks): `units` of them from `base` on, XCD-contiguous
// from 64 units up (option xcd_remap); returns the grid.  Strip-major sweep (option strip; strips of `strip` units) when three x planes
// (3·far·8 B) overflow an XCD's L2 share — a far band `D` units away, D >= d_min — and the XCD's range holds at least two planes.
// gap_at / gap_len stay as the caller set them.
inline dim3 plan_map(const mgs_ctx *ctx, BlockMap &bm, int base, int units, int D, int d_min, int strip) {
  bm.base = base; bm.nblocks = units;
  bm.remap = ctx->opt_xcd_remap && bm.nblocks >= 64;
  bm.chunk = (bm.nblocks + 7) / 8;
  bm.D = 0; bm.S = 0; bm.P = 0;
  int per_xcd = bm.chunk;
  if (bm.remap && ctx->opt_strip != 0 && D >= d_min && bm.chunk >= 2 * D) per_xcd = strip_map(bm, D, strip);
  return dim3(bm.remap ? per_xcd * 8 : bm.nblocks);
}
// workgroup → row-block map of a launch over the row blocks [blk_lo, blk_hi) with their gap (BlockMap): far band of at least 512 row blocks,
// strips of 64 by default
inline dim3 plan_block_map(const mgs_csr *A, int blk_lo, int blk_hi, int gap_at, int gap_len, BlockMap &bm) {
  const mgs_ctx *ctx = A->ctx;
  bm.gap_at = gap_at; bm.gap_len = gap_len;
  return plan_map(ctx, bm, blk_lo, blk_hi - blk_lo, (A->far_band + RB - 1) / RB, 512, ctx->opt_strip > 0 ? ctx->opt_strip : 64);
}
// workgroup → group map: XCD-contiguous, strip-major for far bands (distances in groups instead of row blocks)
inline dim3 plan_group_map(const mgs_csr *A, const mgs_groups *G, BlockMap &bm) {
  const mgs_ctx *ctx = A->ctx;
  const int Db = (A->far_band + RB - 1) / RB;
  const int D = Db >= 512 ? G->plane_groups : 0;          // groups from one far-band period to the next (setup: first blocks Db apart)
  // strip of 128 groups by default: 512³, same-process sweep 5.51 / 5.46 / 5.42 / 5.40 / 5.40 / 5.51 ms per cycle for 2 / 16 / 32 / 64 / 128 / 512 groups
  const int strip = ctx->opt_group_strip > 0 ? ctx->opt_group_strip : (ctx->opt_strip > 0 ? std::max(1, ctx->opt_strip / 2) : 128);
  return plan_map(ctx, bm, 0, G->ngroups, D, 64, strip);
}

// true when the coded kernel serves this operator (square or sharded; short rows; code present and worth it)
// (any = true: a row shard's operand passes — only this kernel knows the halo split, and on its uncoded blocks it is the
//  slice kernel: any code will do)
inline bool use_rowcode(const mgs_csr *A, const mgs_rowcode *c, bool any = false) {
  return c && A->ctx->opt_rowcode && A->blkptr && A->lds_cap > 0 && A->max_row_len <= 64 &&
         (any || (double)c->coded_blocks >= 0.5 * c->nblocks);
}
// LDS budget of one row block of the coded kernels (c may be NULL: nothing coded): capv values, capi ints, and the bytes of the two regions
struct coded_lds {
  int capv, capi;
  size_t val_bytes, int_bytes, pad_bytes;      // pad_bytes: what every launch adds behind the regions (alignment slack + option lds_pad)
};
inline coded_lds coded_budget(const mgs_csr *A, const mgs_rowcode *c, bool f32) {
  coded_lds l;
  // float values: capv a multiple of 4 (the integer region behind the values stays 16-byte aligned for the int4 stores of the uncoded
  // blocks), whose index slice may reach capv + 6 entries (both ends of the slice aligned to 4)
  l.capv = f32 ? (A->lds_cap + 3) & ~3 : A->lds_cap;
  // nearly everything coded: LDS holds values + tables only (8 B per entry → more workgroups per CU); otherwise
  // the integer region must also fit the index slice of the uncoded blocks
  const bool lean = c && (double)c->coded_blocks >= 0.985 * c->nblocks;
  l.capi = lean ? std::max(c->tab_cap, 64) : std::max(c ? c->tab_cap : 0, l.capv + (f32 ? 8 : 2));
  l.val_bytes = (size_t)(f32 ? val_region<float>(l.capv) : val_region<double>(l.capv)) * 8;
  l.int_bytes = (size_t)l.capi * 4;
  l.pad_bytes = 16 + (size_t)A->ctx->opt_lds_pad;      // opt_lds_pad: occupancy experiments
  return l;
}

}  // namespace

// ------------------------------------------------------------------ the two launchers that cross unit boundaries
// kernels_spmv.hip, called by kernels_fused.hip for the coded post pass: the coded kernel on the view A (see its definition)
int launch_coded(const mgs_csr *A, const mgs_rowcode *c, int op, const int *idx, const double *x, const double *b, const double *dinv,
                 double omega, const double *xin, const int *agg, double *out, dim3 grid, BlockMap bm,
                 const double *hv = nullptr, int split = 0x7fffffff);
// kernels_variants.hip, called by mgs_launch_csr_op_range: the A/B form that option spmv_variant names (2–4, 6, 7).  True: launched, or failed —
// *rc says which; false: the variant is none of them or its guard fails, and the caller goes on to the default kernels
bool launch_variant(const mgs_csr *A, int op, const double *x, const double *b, const double *dinv, double omega, double *out, int cap,
                    dim3 grid, const BlockMap &bm, int *rc);
