// blas1.hpp — what every BLAS-1 pass and deterministic reduction is built from (blas1.hip, the Krylov plans through krylov_plan.hpp, guess.hip, the block passes of blockvec.hip):
// the 16-byte lane type with its streaming store, the alignment and store-mode predicates of the launchers, and the folds that decide the bits
// of every sum — lanes → wave → workgroup partial, and partials → result.  Each fold is written here once; a kernel brings its own loop.
//
// Not here, on purpose: guess.hip's block_partials and fold kernels.  Its workgroup sum starts from the first wave's sum where these start from
// 0.0 (the results differ for a sum of −0.0), and its middle stage folds chunks of 256 partials, not 256 chunks; tests/guess_ref.py pins those
// bits.  mdot_partial_kernel (blas1.hip) keeps its own fold as well: there lane k sums row k's four wave sums, K ≤ 16 rows at once.
#pragma once
#include "mgs_internal.hpp"

namespace blas1 {
constexpr int TB = 256;                  // lanes per workgroup of every pass
typedef double vd2 __attribute__((ext_vector_type(2)));

// streaming store (the instruction spelled out: see st_stream in rowblock.hpp); nothing reads back what it stored
__device__ __forceinline__ void st2(vd2 *p, vd2 v, bool nt) {
  if (nt) asm volatile("global_store_dwordx4 %0, %1, off nt" : : "v"(p), "v"(v) : "memory");
  else *p = v;
}
inline bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int nts_of(const mgs_ctx *ctx, int64_t n) { return ctx->opt_nt_store > 0 && n >= ctx->opt_nt_store; }

// The end of every pass with two sums: the lanes' pair (s0, s1) folded over the wave (6 shuffle levels), then the workgroup's TB/64 wave sums added
// in wave order from 0.0, into the partials [2][gridDim.x] that k_dot2_finish folds.  Every lane of the workgroup comes here; sh: the kernel's
// __shared__ double [2][TB / 64].  BLAS1_FOLD1: one sum (sh: double [TB / 64]); pair != 0 writes the second partial as 0.0 so that the same
// staged fold serves.  Macros, not functions: as an inlined function the same statements were scheduled differently in five of the nine plan
// passes (profiles/r17_krylov_plan_base.md), and the passes are held to the instructions they had.
#define BLAS1_FOLD2(s0, s1, sh, part)                                                                                     \
  do {                                                                                                                    \
    for (int off = 32; off > 0; off >>= 1) { s0 += __shfl_down(s0, off); s1 += __shfl_down(s1, off); }                    \
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s0; sh[1][threadIdx.x >> 6] = s1; }                          \
    __syncthreads();                                                                                                      \
    if (threadIdx.x == 0) {                                                                                               \
      double t0 = 0.0, t1 = 0.0;                                                                                          \
      for (int q = 0; q < blas1::TB / 64; ++q) { t0 += sh[0][q]; t1 += sh[1][q]; }                                        \
      part[blockIdx.x] = t0; part[gridDim.x + blockIdx.x] = t1;                                                           \
    }                                                                                                                     \
  } while (0)
#define BLAS1_FOLD1(s, sh, part, pair)                                                                                    \
  do {                                                                                                                    \
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);                                                      \
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;                                                                \
    __syncthreads();                                                                                                      \
    if (threadIdx.x == 0) {                                                                                               \
      double t0 = 0.0;                                                                                                    \
      for (int q = 0; q < blas1::TB / 64; ++q) t0 += sh[q];                                                               \
      part[blockIdx.x] = t0; if (pair) part[gridDim.x + blockIdx.x] = 0.0;                                                \
    }                                                                                                                     \
  } while (0)

// The last stage, one workgroup: lane t adds part[t], part[t + TB], ... in index order, then a TB-wide tree in LDS (sh: __shared__ double [TB]).
// The sum comes back on lane 0 (0.0 elsewhere).  A caller that folds again with the same sh puts a __syncthreads() in between.
__device__ __forceinline__ double final_fold(int nb, const double *__restrict__ part, double *sh) {
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += TB) s += part[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = TB / 2; w > 0; w >>= 1) { if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
  return threadIdx.x == 0 ? sh[0] : 0.0;
}
}   // namespace blas1
