// reorder.hip — a device matrix renumbered and device matrices put together: C[i, j] = A[rperm[i], cperm[j]] for two bijections in device
// memory (mgs_csr_permute), C's values again through the kept source positions (mgs_csr_permute_numeric), C assembled from a br × bc grid
// of blocks (mgs_csr_bmat) and its values again (mgs_csr_bmat_numeric).  No reference counterpart: the reference reads its operators
// from files.
//
// The lists are the caller's device arrays.  Ingest rule (ingest.hip, extract.hip): no kernel uses a list entry as an address before it
// has compared it with its bounds as a 64-bit value.  A list is a bijection iff every entry is in range and none repeats an earlier one:
// pass 1 leaves in inv[v] the lowest position that holds v (32-bit atomicMin; a refused entry touches nothing), pass 2 finds the
// positions k with inv[perm[k]] != k.  The lowest offending position of either kind comes back through one 64-bit atomicMin word per
// list, so the message is deterministic; after a clean check inv is the inverse list, which for the columns is the map old → new.
//
// Values are moved as 64-bit words: −0.0 stays −0.0 and a NaN keeps its payload.
//
// Permute, phases: lists checked, rows narrowed (−1 = refused, passed over by everything later) → source row lengths → scan → fill.
//   (a) no column list: entry-parallel copy (output entry k finds its row by bisection in C's rowptr), stores coalesced;
//   (b) source row of at most 64 entries: one lane.  It writes the row's new columns, in source order, into its own slice of a scratch
//       array of nnz ints, then ranks every entry against that slice (len² reads of a slice that stays in the lane's cache lines);
//   (c) longer rows: one wave per row, four per workgroup.  The wave holds 64 entries of the row at a time and walks the whole row in
//       chunks of 64 beside them; a chunk's new columns go from lane to lane, nothing is staged, so a row may be of any length.
// The new columns of a row are distinct, so the rank (entries of the row with a smaller new column) is the place: computed from the row
// alone, no atomics on values or places, two calls give identical arrays (the list of wave rows is filled in any order — it only says
// which rows arm (c) serves).
//
// Bmat, phases: the grid checked on the host, the block table (rowptr, col, val, column offset of every position; row offsets of the
// block rows) written to device memory → one lane per output row sums its blocks' row lengths → scan → entry-parallel fill: an output
// entry finds its row by bisection in C's rowptr, its block row by bisection in the row offsets, its block by walking the row's
// per-block lengths, its source position from that block's rowptr.  The values-only pass is the same kernel without the column store.
//
// Transpose, values again (mgs_csr_transpose_numeric): one entry-parallel launch over A's entries, two bisections per entry, no kept map;
// places of distinct entries are distinct, so there are no atomics on values or places (the miss counter alone is one).
#include <cstring>
#include <vector>
#include "mgs_internal.hpp"

namespace {
typedef unsigned long long u64;
struct BmatBlock {            // one grid position in the device table; rp == NULL: a zero block
  const int *rp; const int *ci; const u64 *val;
  int coff, pad;
};
struct BmatRec { bool null; int rows, cols; int64_t nnz; };   // what mgs_csr_bmat_numeric compares the blocks it is given with
}  // namespace

struct mgs_reorder_plan {
  bool is_bmat = false;
  // mgs_csr_permute
  int *src = nullptr;           // keep_map: position in A's arrays of every entry of C (4 B per entry)
  bool keep = false;
  int64_t n_lane = 0, n_wave = 0;
  int a_rows = 0, a_cols = 0;   // the source as it was: mgs_csr_permute_numeric refuses another shape or entry count
  int64_t a_nnz = 0;
  // mgs_csr_bmat
  int br = 0, bc = 0, n_blocks = 0;
  void *table = nullptr;        // device: BmatBlock[br·bc], then int roff[br + 1]
  std::vector<BmatBlock> host_table;
  std::vector<BmatRec> rec;
};
void mgs_free_reorder(mgs_reorder_plan *p) {
  if (!p) return;
  if (p->src) mgs_hip_free(p->src);
  if (p->table) mgs_hip_free(p->table);
  delete p;
}

namespace {
constexpr int TB = 256;
constexpr int WAVE = 64;
constexpr int PERM_LANE_LEN = 64;     // source rows of at most this many entries: one lane per output row
constexpr u64 NO_ERR = ~0ull;
constexpr int NO_COL = 0x7fffffff;    // a lane without an entry: never below a new column
enum { ST_ROW = 0, ST_COL = 1, ST_WAVE = 2, ST_TOTAL = 3 };   // lowest bad position << 1 | kind of either list, rows listed for arm (c), entries (bmat)
enum { BAD_RANGE = 0, BAD_REPEAT = 1 };

struct DevBuf {  // RAII for temporaries
  void *p = nullptr;
  ~DevBuf() { if (p) mgs_hip_free(p); }
  template <class T> T *as() { return (T *)p; }
};
template <class T>
int dalloc(mgs_ctx *ctx, DevBuf &b, size_t count) { T *q = nullptr; MGS_TRY(mgs_dev_alloc(ctx, &q, count)); b.p = q; return MGS_OK; }

struct SyncUnlessDone {   // declared after a build's temporaries, so destroyed before them: an early error return waits for whatever is still
  hipStream_t s;          // enqueued before the temporaries are released
  bool done = false;
  ~SyncUnlessDone() { if (!done && hipStreamSynchronize(s) != hipSuccess) (void)hipGetLastError(); }
};
int finish(mgs_ctx *ctx, const char *who) {   // launch errors of everything enqueued so far + the stream's completion
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return mgs_fail(ctx, MGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  return MGS_OK;
}
long long fetch_index(const void *dev, long long at, int bits) {   // one element of an input list, for an error message
  long long v64 = 0; int v32 = 0;
  if (bits == 64) { if (hipMemcpy(&v64, (const long long *)dev + at, 8, hipMemcpyDeviceToHost) != hipSuccess) (void)hipGetLastError(); return v64; }
  if (hipMemcpy(&v32, (const int *)dev + at, 4, hipMemcpyDeviceToHost) != hipSuccess) (void)hipGetLastError();
  return v32;
}

// ------------------------------------------------------------------ the lists: bijection check, inverse, narrowed copy
// inv has n entries, all 0xffffffff before this kernel; narrow (may be NULL) receives the list as ints, −1 for a refused entry
template <class I>
__global__ void perm_mark_kernel(long long n, const I *__restrict__ in, unsigned *__restrict__ inv, int *__restrict__ narrow, u64 *__restrict__ slot) {
  const long long k = (long long)blockIdx.x * TB + threadIdx.x;
  if (k >= n) return;
  const long long v = (long long)in[k];
  const bool bad = v < 0 || v >= n;
  if (bad) atomicMin(slot, ((u64)k << 1) | BAD_RANGE);
  else atomicMin(&inv[v], (unsigned)k);
  if (narrow) narrow[k] = bad ? -1 : (int)v;
}
template <class I>
__global__ void perm_verify_kernel(long long n, const I *__restrict__ in, const unsigned *__restrict__ inv, u64 *__restrict__ slot) {
  const long long k = (long long)blockIdx.x * TB + threadIdx.x;
  if (k >= n) return;
  const long long v = (long long)in[k];
  if (v < 0 || v >= n) return;      // reported by pass 1
  if ((long long)inv[v] != k) atomicMin(slot, ((u64)k << 1) | BAD_REPEAT);      // an earlier position holds v
}
template <class I>
void perm_check_launch(hipStream_t s, long long n, const void *in, unsigned *inv, int *narrow, u64 *slot) {
  hipLaunchKernelGGL(perm_mark_kernel<I>, dim3(mgs_grid(n, TB)), dim3(TB), 0, s, n, (const I *)in, inv, narrow, slot);
  hipLaunchKernelGGL(perm_verify_kernel<I>, dim3(mgs_grid(n, TB)), dim3(TB), 0, s, n, (const I *)in, (const unsigned *)inv, slot);
}

// ------------------------------------------------------------------ permute: lengths, the three fill arms, values again
__global__ void perm_len_kernel(int nr, const int *__restrict__ rows, const int *__restrict__ arp, int *__restrict__ cnt, int ranked, int *__restrict__ wave_rows,
                                u64 *__restrict__ st) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= nr) return;
  const int r = rows ? rows[i] : i;
  const int n = r >= 0 ? arp[r + 1] - arp[r] : 0;
  cnt[i] = n;
  if (ranked && n > PERM_LANE_LEN) wave_rows[atomicAdd(&st[ST_WAVE], 1ull)] = i;      // at most nr rows are listed: wave_rows holds nr
}
__global__ void perm_rowcopy_kernel(long long nnz, int nr, const int *__restrict__ rows, const int *__restrict__ arp, const int *__restrict__ aci, const u64 *__restrict__ av,
                                    const int *__restrict__ crp, int *__restrict__ ccol, u64 *__restrict__ cval, int *__restrict__ src) {
  const long long k = (long long)blockIdx.x * TB + threadIdx.x;
  if (k >= nnz) return;
  int lo = 0, hi = nr;      // the entry's row: the last o with crp[o] ≤ k (empty rows share their successor's start and are passed over)
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((long long)crp[mid] <= k) lo = mid; else hi = mid;
  }
  const int r = rows ? rows[lo] : lo;
  if (r < 0) return;
  const int a0 = arp[r], off = (int)(k - crp[lo]);
  if (off >= arp[r + 1] - a0) return;      // cannot happen: crp is the scan of these lengths
  ccol[k] = aci[a0 + off];
  cval[k] = av[a0 + off];
  if (src) src[k] = a0 + off;
}
// t: nnz ints of scratch; row i's slice [crp[i], crp[i + 1]) is written and read by the row's own lane only
__global__ __launch_bounds__(TB) void perm_lane_kernel(int nr, const int *__restrict__ rows, const int *__restrict__ arp, const int *__restrict__ aci, const u64 *__restrict__ av,
                                                       const int *__restrict__ cmap, const int *__restrict__ crp, int *t, int *__restrict__ ccol, u64 *__restrict__ cval,
                                                       int *__restrict__ src) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= nr) return;
  const int r = rows ? rows[i] : i;
  if (r < 0) return;
  const int a0 = arp[r], len = arp[r + 1] - a0;
  if (len > PERM_LANE_LEN) return;             // arm (c)
  const int dst = crp[i];
  if (crp[i + 1] - dst != len) return;         // cannot happen: crp is the scan of these lengths
  for (int j = 0; j < len; ++j) t[dst + j] = cmap[aci[a0 + j]];
  for (int j = 0; j < len; ++j) {
    const int q = t[dst + j];
    int rank = 0;
    for (int j2 = 0; j2 < len; ++j2) rank += t[dst + j2] < q ? 1 : 0;      // rank < len whatever cmap holds: the stores stay inside the row
    ccol[dst + rank] = q; cval[dst + rank] = av[a0 + j];
    if (src) src[dst + rank] = a0 + j;
  }
}
__global__ __launch_bounds__(TB) void perm_wave_kernel(int n_wave, const int *__restrict__ wave_rows, const int *__restrict__ rows, const int *__restrict__ arp,
                                                       const int *__restrict__ aci, const u64 *__restrict__ av, const int *__restrict__ cmap, const int *__restrict__ crp,
                                                       int *__restrict__ ccol, u64 *__restrict__ cval, int *__restrict__ src) {
  const int w = blockIdx.x * (TB / WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= n_wave) return;                      // the whole wave leaves: the shuffles below see full waves only
  const int i = wave_rows[w];
  const int r = rows ? rows[i] : i;
  if (r < 0) return;                            // wave-uniform; cannot happen: only checked rows are listed
  const int a0 = arp[r], len = arp[r + 1] - a0;
  const int dst = crp[i], cap = crp[i + 1] - dst;
  for (int mine = 0; mine < len; mine += WAVE) {          // len is wave-uniform: every lane runs every trip of both loops
    const int p = mine + lane;
    const int q = p < len ? cmap[aci[a0 + p]] : NO_COL;
    int rank = 0;
    for (int base = 0; base < len; base += WAVE) {
      const int pc = base + lane;
      const int qc = pc < len ? cmap[aci[a0 + pc]] : NO_COL;
      for (int j = 0; j < WAVE; ++j) rank += __shfl(qc, j) < q ? 1 : 0;
    }
    if (p < len && rank < cap) {                // rank < cap always: the row's new columns are distinct
      ccol[dst + rank] = q; cval[dst + rank] = av[a0 + p];
      if (src) src[dst + rank] = a0 + p;
    }
  }
}
__global__ void perm_numeric_kernel(long long nnz, long long a_nnz, const int *__restrict__ src, const u64 *__restrict__ av, u64 *__restrict__ cval) {
  const long long k = (long long)blockIdx.x * TB + threadIdx.x;
  if (k >= nnz) return;
  const int p = src[k];
  if (p >= 0 && p < a_nnz) cval[k] = av[p];      // always: the map was written by the fill pass of a source with a_nnz entries
}

// ------------------------------------------------------------------ transpose: values again
// Entry k of A = (i, j, v): i by bisection in A's rowptr (the rule of scale_kernel), its place in At by bisection of i in At's columns of row
// j (mgs_csr_transpose leaves them ascending).  No place (another pattern): counted, nothing written.  Every index is compared with its
// bounds before it is an address; the only store is tval[p] with t_rp[j] ≤ p < t_rp[j + 1] ≤ nnz.
__global__ void transpose_numeric_kernel(long long nnz, int rows, int t_rows, const int *__restrict__ arp, const int *__restrict__ aci, const u64 *__restrict__ av,
                                         const int *__restrict__ trp, const int *__restrict__ tci, u64 *__restrict__ tval, u64 *__restrict__ miss) {
  const long long k = (long long)blockIdx.x * TB + threadIdx.x;
  if (k >= nnz) return;
  int lo = 0, hi = rows;      // the entry's row: the last i with arp[i] ≤ k (empty rows share their successor's start and are passed over)
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((long long)arp[mid] <= k) lo = mid; else hi = mid;
  }
  const int i = lo, j = aci[k];
  bool placed = false;
  if (j >= 0 && j < t_rows) {
    const int b = trp[j], e = trp[j + 1];
    if (b >= 0 && b <= e && (long long)e <= nnz) {      // always: At's rowptr is a scan over nnz entries
      int p = b, q = e;      // the first p in [b, e) with tci[p] ≥ i
      while (p < q) {
        const int mid = p + ((q - p) >> 1);
        if (tci[mid] < i) p = mid + 1; else q = mid;
      }
      if (p < e && tci[p] == i) { tval[p] = av[k]; placed = true; }
    }
  }
  if (!placed && miss) atomicAdd(miss, 1ull);
}

void perm_message(mgs_ctx *ctx, const char *who, const char *list, const char *kind, const void *dev, int bits, u64 word, int n, const unsigned *inv) {
  const long long k = (long long)(word >> 1), v = fetch_index(dev, k, bits);
  if ((word & 1ull) == BAD_RANGE) {
    mgs_fail(ctx, MGS_ERR_INVALID, "%s: %s index %lld at position %lld of the %s list is outside [0, %d)", who, kind, v, k, list, n);
    return;
  }
  unsigned first = 0;
  if (hipMemcpy(&first, inv + v, 4, hipMemcpyDeviceToHost) != hipSuccess) (void)hipGetLastError();      // v is in range: pass 2 reported it
  mgs_fail(ctx, MGS_ERR_INVALID, "%s: %s index %lld at position %lld of the %s list repeats the entry at position %u: the list is not a permutation", who, kind, v, k, list, first);
}

int permute_build(const mgs_csr *A, const void *rperm, const void *cperm, int bits, int keep_map, mgs_reorder_plan *pl, mgs_csr **out) {
  mgs_ctx *ctx = A->ctx;
  hipStream_t s = ctx->stream;
  const char *who = "mgs_csr_permute";
  const u64 *av = (const u64 *)A->val;
  const int nr = A->rows, nc = A->cols;
  DevBuf rows, rinv, cmap, cnt, wave, st, scratch;
  if (rperm) { MGS_TRY(dalloc<int>(ctx, rows, (size_t)nr)); MGS_TRY(dalloc<unsigned>(ctx, rinv, (size_t)nr)); }
  if (cperm) { MGS_TRY(dalloc<unsigned>(ctx, cmap, (size_t)nc)); MGS_TRY(dalloc<int>(ctx, wave, (size_t)nr)); MGS_TRY(dalloc<int>(ctx, scratch, (size_t)A->nnz)); }
  MGS_TRY(dalloc<int>(ctx, cnt, (size_t)nr + 1));
  MGS_TRY(dalloc<u64>(ctx, st, 4));
  SyncUnlessDone guard{s};
  const int *rl = rperm ? rows.as<int>() : nullptr;
  // 1. lists (the rows narrowed), 2. source row lengths and the rows of arm (c)
  u64 h[4] = {NO_ERR, NO_ERR, 0, 0};
  MGS_HIP(ctx, hipMemcpyAsync(st.p, h, sizeof h, hipMemcpyHostToDevice, s));
  MGS_HIP(ctx, hipMemsetAsync(cnt.p, 0, sizeof(int) * ((size_t)nr + 1), s));
  if (rperm && nr) {
    MGS_HIP(ctx, hipMemsetAsync(rinv.p, 0xff, sizeof(unsigned) * (size_t)nr, s));
    if (bits == 64) perm_check_launch<long long>(s, nr, rperm, rinv.as<unsigned>(), rows.as<int>(), st.as<u64>() + ST_ROW);
    else perm_check_launch<int>(s, nr, rperm, rinv.as<unsigned>(), rows.as<int>(), st.as<u64>() + ST_ROW);
  }
  if (cperm && nc) {
    MGS_HIP(ctx, hipMemsetAsync(cmap.p, 0xff, sizeof(unsigned) * (size_t)nc, s));
    if (bits == 64) perm_check_launch<long long>(s, nc, cperm, cmap.as<unsigned>(), nullptr, st.as<u64>() + ST_COL);
    else perm_check_launch<int>(s, nc, cperm, cmap.as<unsigned>(), nullptr, st.as<u64>() + ST_COL);
  }
  if (nr) hipLaunchKernelGGL(perm_len_kernel, dim3(mgs_grid(nr, TB)), dim3(TB), 0, s, nr, rl, A->rowptr, cnt.as<int>(), cperm ? 1 : 0, wave.as<int>(), st.as<u64>());
  MGS_HIP(ctx, hipMemcpyAsync(h, st.p, sizeof h, hipMemcpyDeviceToHost, s));
  MGS_TRY(finish(ctx, who));
  if (h[ST_ROW] != NO_ERR) { perm_message(ctx, who, "row", "row", rperm, bits, h[ST_ROW], nr, rinv.as<unsigned>()); return MGS_ERR_INVALID; }
  if (h[ST_COL] != NO_ERR) { perm_message(ctx, who, "column", "column", cperm, bits, h[ST_COL], nc, cmap.as<unsigned>()); return MGS_ERR_INVALID; }
  MGS_CHECK(ctx, h[ST_WAVE] <= (u64)nr, MGS_ERR_HIP, "%s: %llu long rows counted among %d rows", who, h[ST_WAVE], nr);
  const int n_wave = (int)h[ST_WAVE];
  // 3. scan, 4. columns, values, source positions
  const int64_t nnz = A->nnz;      // a bijection of the rows keeps every entry
  mgs_csr *C = nullptr;
  MGS_TRY(mgs_csr_alloc(ctx, nr, nc, nnz, &C));
  *out = C;      // the caller destroys it on failure
  int64_t total = -1;
  MGS_TRY(k_exclusive_scan_i32(ctx, cnt.as<int>(), C->rowptr, (int64_t)nr + 1, &total));
  MGS_CHECK(ctx, total == nnz, MGS_ERR_HIP, "%s: the permuted rows hold %lld entries, A holds %lld", who, (long long)total, (long long)nnz);
  if (keep_map) MGS_TRY(mgs_dev_alloc(ctx, &pl->src, (size_t)nnz));
  if (nr && nnz) {
    if (!cperm)
      hipLaunchKernelGGL(perm_rowcopy_kernel, dim3(mgs_grid(nnz, TB)), dim3(TB), 0, s, (long long)nnz, nr, rl, A->rowptr, A->col, av, C->rowptr, C->col, (u64 *)C->val, pl->src);
    else {
      const int *cm = (const int *)cmap.p;      // every entry below nc after the clean check
      if (nr > n_wave) hipLaunchKernelGGL(perm_lane_kernel, dim3(mgs_grid(nr, TB)), dim3(TB), 0, s, nr, rl, A->rowptr, A->col, av, cm, C->rowptr, scratch.as<int>(), C->col,
                                          (u64 *)C->val, pl->src);
      if (n_wave) hipLaunchKernelGGL(perm_wave_kernel, dim3(mgs_grid(n_wave, TB / WAVE)), dim3(TB), 0, s, n_wave, wave.as<int>(), rl, A->rowptr, A->col, av, cm, C->rowptr, C->col,
                                     (u64 *)C->val, pl->src);
    }
  }
  MGS_TRY(finish(ctx, who));
  guard.done = true;
  pl->keep = keep_map != 0;
  pl->n_lane = cperm ? (int64_t)nr - n_wave : 0; pl->n_wave = cperm ? n_wave : 0;
  pl->a_rows = A->rows; pl->a_cols = A->cols; pl->a_nnz = A->nnz;
  return mgs_plan_csr(C);
}

// ------------------------------------------------------------------ bmat: count, fill, values again
__device__ __forceinline__ int bmat_block_row(int br, const int *__restrict__ roff, int r) {      // the last I with roff[I] ≤ r: a block row that holds r, never an empty one
  int lo = 0, hi = br;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (roff[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}
__global__ void bmat_count_kernel(int rows, int br, int bc, const BmatBlock *__restrict__ tab, const int *__restrict__ roff, int *__restrict__ cnt, u64 *__restrict__ st) {
  const int r = blockIdx.x * TB + threadIdx.x;
  int n = 0;
  if (r < rows) {
    const int I = bmat_block_row(br, roff, r), i = r - roff[I];
    if (i < roff[I + 1] - roff[I])      // always
      for (int J = 0; J < bc; ++J) {
        const int *rp = tab[I * bc + J].rp;
        if (rp) n += rp[i + 1] - rp[i];
      }
    cnt[r] = n;
  }
  u64 sum = (u64)n;      // every lane of the wave is here
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&st[ST_TOTAL], sum);
}
template <bool VALUES_ONLY>
__global__ void bmat_fill_kernel(long long nnz, int rows, int br, int bc, const BmatBlock *__restrict__ tab, const int *__restrict__ roff, const int *__restrict__ crp,
                                 int *__restrict__ ccol, u64 *__restrict__ cval) {
  const long long k = (long long)blockIdx.x * TB + threadIdx.x;
  if (k >= nnz) return;
  int lo = 0, hi = rows;      // the entry's row: the last o with crp[o] ≤ k
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((long long)crp[mid] <= k) lo = mid; else hi = mid;
  }
  const int I = bmat_block_row(br, roff, lo), i = lo - roff[I];
  if (i >= roff[I + 1] - roff[I]) return;      // cannot happen
  int off = (int)(k - crp[lo]);
  for (int J = 0; J < bc; ++J) {
    const BmatBlock b = tab[I * bc + J];
    if (!b.rp) continue;
    const int a0 = b.rp[i], len = b.rp[i + 1] - a0;
    if (off < len) {
      if (!VALUES_ONLY) ccol[k] = b.ci[a0 + off] + b.coff;
      cval[k] = b.val[a0 + off];
      return;
    }
    off -= len;
  }
}

// the grid as the host sees it: sizes, offsets, table; every refusal of mgs_csr_bmat that needs no device
int bmat_layout(mgs_ctx *ctx, const char *who, int br, int bc, const mgs_csr *const *blocks, const int *row_sizes, const int *col_sizes, std::vector<int> &rs, std::vector<int> &cs) {
  rs.assign((size_t)br, -1); cs.assign((size_t)bc, -1);
  for (int I = 0; I < br; ++I)
    if (row_sizes) { MGS_CHECK(ctx, row_sizes[I] >= 0, MGS_ERR_INVALID, "%s: row_sizes[%d] = %d is negative", who, I, row_sizes[I]); rs[I] = row_sizes[I]; }
  for (int J = 0; J < bc; ++J)
    if (col_sizes) { MGS_CHECK(ctx, col_sizes[J] >= 0, MGS_ERR_INVALID, "%s: col_sizes[%d] = %d is negative", who, J, col_sizes[J]); cs[J] = col_sizes[J]; }
  for (int I = 0; I < br; ++I)
    for (int J = 0; J < bc; ++J) {
      const mgs_csr *B = blocks[I * bc + J];
      if (!B) continue;
      MGS_CHECK(ctx, B->ctx == ctx, MGS_ERR_INVALID, "%s: block (%d, %d) belongs to a different context", who, I, J);
      MGS_CHECK(ctx, !mgs_csr_is_shard(B), MGS_ERR_INVALID, "%s: block (%d, %d) is a row shard (%d rows, %d columns with halo columns): row shards are not supported", who, I, J,
                B->rows, B->cols);
      if (rs[I] < 0) rs[I] = B->rows;
      MGS_CHECK(ctx, rs[I] == B->rows, MGS_ERR_INVALID, "%s: block (%d, %d) has %d rows, block row %d has %d", who, I, J, B->rows, I, rs[I]);
      if (cs[J] < 0) cs[J] = B->cols;
      MGS_CHECK(ctx, cs[J] == B->cols, MGS_ERR_INVALID, "%s: block (%d, %d) has %d columns, block column %d has %d", who, I, J, B->cols, J, cs[J]);
    }
  for (int I = 0; I < br; ++I) MGS_CHECK(ctx, rs[I] >= 0, MGS_ERR_INVALID, "%s: block row %d holds only NULL blocks and row_sizes gives it no size", who, I);
  for (int J = 0; J < bc; ++J) MGS_CHECK(ctx, cs[J] >= 0, MGS_ERR_INVALID, "%s: block column %d holds only NULL blocks and col_sizes gives it no size", who, J);
  return MGS_OK;
}
void bmat_table(int br, int bc, const mgs_csr *const *blocks, const std::vector<int> &cs, std::vector<BmatBlock> &tab) {
  tab.assign((size_t)br * bc, BmatBlock{nullptr, nullptr, nullptr, 0, 0});
  for (int I = 0; I < br; ++I) {
    int coff = 0;
    for (int J = 0; J < bc; ++J) {
      const mgs_csr *B = blocks[I * bc + J];
      if (B) tab[(size_t)I * bc + J] = BmatBlock{B->rowptr, B->col, (const u64 *)B->val, coff, 0};
      coff += cs[J];
    }
  }
}

int bmat_build(mgs_ctx *ctx, int br, int bc, const mgs_csr *const *blocks, const int *row_sizes, const int *col_sizes, mgs_reorder_plan *pl, mgs_csr **out) {
  hipStream_t s = ctx->stream;
  const char *who = "mgs_csr_bmat";
  std::vector<int> rs, cs;
  MGS_TRY(bmat_layout(ctx, who, br, bc, blocks, row_sizes, col_sizes, rs, cs));
  const int nb = br * bc;
  std::vector<int> roff((size_t)br + 1, 0);
  long long rows = 0, cols = 0, nnz = 0;
  for (int I = 0; I < br; ++I) { rows += rs[I]; if (rows < 2147483647LL) roff[I + 1] = (int)rows; }
  for (int J = 0; J < bc; ++J) cols += cs[J];
  pl->rec.assign((size_t)nb, BmatRec{true, 0, 0, 0});
  for (int q = 0; q < nb; ++q)
    if (blocks[q]) { pl->rec[q] = BmatRec{false, blocks[q]->rows, blocks[q]->cols, blocks[q]->nnz}; nnz += blocks[q]->nnz; ++pl->n_blocks; }
  MGS_CHECK(ctx, rows < 2147483647LL && cols < 2147483647LL, MGS_ERR_INVALID, "%s: the result is %lld x %lld, 2^31 - 1 rows or columns or more", who, rows, cols);
  MGS_CHECK(ctx, nnz < 2147483647LL, MGS_ERR_INVALID, "%s: the blocks hold %lld entries, 2^31 - 1 or more", who, nnz);
  bmat_table(br, bc, blocks, cs, pl->host_table);
  const size_t tab_bytes = sizeof(BmatBlock) * (size_t)nb, roff_bytes = sizeof(int) * ((size_t)br + 1);
  char *table = nullptr;
  MGS_TRY(mgs_dev_alloc(ctx, &table, tab_bytes + roff_bytes));
  pl->table = table; pl->br = br; pl->bc = bc; pl->is_bmat = true;
  const BmatBlock *dtab = (const BmatBlock *)table;
  const int *droff = (const int *)(table + tab_bytes);
  DevBuf cnt, st;
  MGS_TRY(dalloc<int>(ctx, cnt, (size_t)rows + 1));
  MGS_TRY(dalloc<u64>(ctx, st, 4));
  SyncUnlessDone guard{s};      // also keeps roff and the host table alive until the copies below have run
  u64 h[4] = {NO_ERR, NO_ERR, 0, 0};
  MGS_HIP(ctx, hipMemcpyAsync(st.p, h, sizeof h, hipMemcpyHostToDevice, s));
  MGS_HIP(ctx, hipMemcpyAsync(table, pl->host_table.data(), tab_bytes, hipMemcpyHostToDevice, s));
  MGS_HIP(ctx, hipMemcpyAsync(table + tab_bytes, roff.data(), roff_bytes, hipMemcpyHostToDevice, s));
  MGS_HIP(ctx, hipMemsetAsync(cnt.p, 0, sizeof(int) * ((size_t)rows + 1), s));
  if (rows) hipLaunchKernelGGL(bmat_count_kernel, dim3(mgs_grid(rows, TB)), dim3(TB), 0, s, (int)rows, br, bc, dtab, droff, cnt.as<int>(), st.as<u64>());
  MGS_HIP(ctx, hipMemcpyAsync(h, st.p, sizeof h, hipMemcpyDeviceToHost, s));
  MGS_TRY(finish(ctx, who));
  MGS_CHECK(ctx, h[ST_TOTAL] == (u64)nnz, MGS_ERR_INVALID, "%s: the rows of the blocks hold %llu entries, the blocks record %lld", who, h[ST_TOTAL], nnz);
  mgs_csr *C = nullptr;
  MGS_TRY(mgs_csr_alloc(ctx, (int)rows, (int)cols, nnz, &C));
  *out = C;      // the caller destroys it on failure
  MGS_TRY(k_exclusive_scan_i32(ctx, cnt.as<int>(), C->rowptr, rows + 1, nullptr));
  if (rows && nnz)
    hipLaunchKernelGGL(bmat_fill_kernel<false>, dim3(mgs_grid(nnz, TB)), dim3(TB), 0, s, nnz, (int)rows, br, bc, dtab, droff, C->rowptr, C->col, (u64 *)C->val);
  MGS_TRY(finish(ctx, who));
  guard.done = true;
  return mgs_plan_csr(C);
}

}  // namespace

int k_csr_permute(const mgs_csr *A, const void *rperm_dev, const void *cperm_dev, int index_bits, int keep_map, mgs_csr **out) {
  const char *who = "mgs_csr_permute";
  MGS_CHECK(A ? A->ctx : nullptr, A && out, MGS_ERR_INVALID, "%s: NULL argument", who);
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, index_bits == 32 || index_bits == 64, MGS_ERR_INVALID, "%s: index_bits %d is neither 32 nor 64", who, index_bits);
  MGS_CHECK(ctx, !mgs_csr_is_shard(A), MGS_ERR_INVALID, "%s: A is a row shard (%d rows, %d columns with halo columns): reorderings of row shards are not supported", who, A->rows,
            A->cols);
  mgs_reorder_plan *pl = new mgs_reorder_plan();
  mgs_csr *C = nullptr;
  const int rc = permute_build(A, rperm_dev, cperm_dev, index_bits, keep_map, pl, &C);
  if (rc != MGS_OK) {
    hipStreamSynchronize(ctx->stream);
    mgs_csr_destroy(C); mgs_free_reorder(pl);
    return rc;
  }
  C->reop = pl;
  *out = C;
  return MGS_OK;
}

int k_csr_permute_numeric(const mgs_csr *A, mgs_csr *C) {
  const char *who = "mgs_csr_permute_numeric";
  MGS_CHECK(A ? A->ctx : (C ? C->ctx : nullptr), A && C, MGS_ERR_INVALID, "%s: NULL argument", who);
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, C->ctx == ctx, MGS_ERR_INVALID, "%s: C belongs to a different context", who);
  const mgs_reorder_plan *pl = C->reop;
  MGS_CHECK(ctx, pl && !pl->is_bmat && pl->keep, MGS_ERR_STATE, "%s: C keeps no source map (mgs_csr_permute with keep_map != 0 does)", who);
  MGS_CHECK(ctx, A->rows == pl->a_rows && A->cols == pl->a_cols && A->nnz == pl->a_nnz, MGS_ERR_INVALID, "%s: A is %d x %d with %lld entries, C was permuted from %d x %d with %lld", who,
            A->rows, A->cols, (long long)A->nnz, pl->a_rows, pl->a_cols, (long long)pl->a_nnz);
  MGS_CHECK(ctx, !(C->code && C->code->vtab), MGS_ERR_INVALID, "%s: C carries a value-carrying pattern code (option valcode): permute the matrix again instead", who);
  if (C->nnz) hipLaunchKernelGGL(perm_numeric_kernel, dim3(mgs_grid(C->nnz, TB)), dim3(TB), 0, ctx->stream, (long long)C->nnz, (long long)A->nnz, pl->src, (const u64 *)A->val, (u64 *)C->val);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

int k_csr_transpose_numeric(const mgs_csr *A, mgs_csr *At, int64_t *misses) {
  const char *who = "mgs_csr_transpose_numeric";
  MGS_CHECK(A ? A->ctx : (At ? At->ctx : nullptr), A && At, MGS_ERR_INVALID, "%s: NULL argument", who);
  mgs_ctx *ctx = A->ctx;
  MGS_CHECK(ctx, At->ctx == ctx, MGS_ERR_INVALID, "%s: At belongs to a different context", who);
  MGS_CHECK(ctx, At->rows == A->cols && At->cols == A->rows, MGS_ERR_INVALID, "%s: A is %d x %d, At is %d x %d, not %d x %d", who, A->rows, A->cols, At->rows, At->cols, A->cols,
            A->rows);
  MGS_CHECK(ctx, At->nnz == A->nnz, MGS_ERR_INVALID, "%s: A holds %lld entries, At holds %lld", who, (long long)A->nnz, (long long)At->nnz);
  MGS_CHECK(ctx, !(At->code && At->code->vtab), MGS_ERR_INVALID, "%s: At carries a value-carrying pattern code (option valcode): transpose the matrix again instead", who);
  if (misses) *misses = 0;
  if (!A->nnz || !A->rows) return MGS_OK;
  DevBuf miss;
  if (misses) {
    MGS_TRY(dalloc<u64>(ctx, miss, 1));
    MGS_HIP(ctx, hipMemsetAsync(miss.p, 0, sizeof(u64), ctx->stream));
  }
  SyncUnlessDone guard{ctx->stream};
  guard.done = !misses;      // nothing to release behind an enqueue-only call
  hipLaunchKernelGGL(transpose_numeric_kernel, dim3(mgs_grid(A->nnz, TB)), dim3(TB), 0, ctx->stream, (long long)A->nnz, A->rows, At->rows, A->rowptr, A->col, (const u64 *)A->val,
                     At->rowptr, At->col, (u64 *)At->val, miss.as<u64>());
  MGS_HIP(ctx, hipGetLastError());
  if (!misses) return MGS_OK;
  u64 h = 0;
  MGS_HIP(ctx, hipMemcpyAsync(&h, miss.p, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  MGS_TRY(finish(ctx, who));
  guard.done = true;
  *misses = (int64_t)h;
  MGS_CHECK(ctx, h == 0, MGS_ERR_STATE, "%s: %llu of A's %lld entries have no place in At: its pattern is not the transpose of A's (nothing was written for them)", who, h,
            (long long)A->nnz);
  return MGS_OK;
}

int k_csr_permute_info(const mgs_csr *C, int64_t out[4]) {
  MGS_CHECK(nullptr, C && out, MGS_ERR_INVALID, "mgs_csr_permute_info: NULL argument");
  out[0] = out[1] = out[2] = out[3] = 0;
  const mgs_reorder_plan *pl = C->reop;
  if (!pl || pl->is_bmat) return MGS_OK;
  out[0] = pl->n_lane; out[1] = pl->n_wave; out[2] = C->max_row_len; out[3] = pl->keep ? 4 * C->nnz : 0;
  return MGS_OK;
}

int k_csr_bmat(mgs_ctx *ctx, int br, int bc, const mgs_csr *const *blocks, const int *row_sizes, const int *col_sizes, mgs_csr **out) {
  const char *who = "mgs_csr_bmat";
  MGS_CHECK(ctx, ctx && blocks && out, MGS_ERR_INVALID, "%s: NULL argument", who);
  MGS_CHECK(ctx, br >= 1 && bc >= 1, MGS_ERR_INVALID, "%s: a grid of %d x %d blocks", who, br, bc);
  MGS_CHECK(ctx, (long long)br * bc <= MGS_BMAT_MAX_BLOCKS, MGS_ERR_INVALID, "%s: a grid of %d x %d = %lld blocks, more than MGS_BMAT_MAX_BLOCKS = %d", who, br, bc, (long long)br * bc,
            MGS_BMAT_MAX_BLOCKS);
  mgs_reorder_plan *pl = new mgs_reorder_plan();
  mgs_csr *C = nullptr;
  const int rc = bmat_build(ctx, br, bc, blocks, row_sizes, col_sizes, pl, &C);
  if (rc != MGS_OK) {
    hipStreamSynchronize(ctx->stream);
    mgs_csr_destroy(C); mgs_free_reorder(pl);
    return rc;
  }
  C->reop = pl;
  *out = C;
  return MGS_OK;
}

int k_csr_bmat_numeric(mgs_csr *C, const mgs_csr *const *blocks) {
  const char *who = "mgs_csr_bmat_numeric";
  MGS_CHECK(C ? C->ctx : nullptr, C && blocks, MGS_ERR_INVALID, "%s: NULL argument", who);
  mgs_ctx *ctx = C->ctx;
  mgs_reorder_plan *pl = C->reop;
  MGS_CHECK(ctx, pl && pl->is_bmat, MGS_ERR_INVALID, "%s: C was not built by mgs_csr_bmat", who);
  MGS_CHECK(ctx, !(C->code && C->code->vtab), MGS_ERR_INVALID, "%s: C carries a value-carrying pattern code (option valcode): assemble the matrix again instead", who);
  const int br = pl->br, bc = pl->bc, nb = br * bc;
  for (int I = 0; I < br; ++I)
    for (int J = 0; J < bc; ++J) {
      const mgs_csr *B = blocks[I * bc + J];
      const BmatRec &rec = pl->rec[(size_t)I * bc + J];
      MGS_CHECK(ctx, (B == nullptr) == rec.null, MGS_ERR_INVALID, "%s: block (%d, %d) is %s, it was %s when C was assembled", who, I, J, B ? "a matrix" : "NULL", rec.null ? "NULL" : "a matrix");
      if (!B) continue;
      MGS_CHECK(ctx, B->ctx == ctx, MGS_ERR_INVALID, "%s: block (%d, %d) belongs to a different context", who, I, J);
      MGS_CHECK(ctx, B->rows == rec.rows && B->cols == rec.cols && B->nnz == rec.nnz, MGS_ERR_INVALID,
                "%s: block (%d, %d) is %d x %d with %lld entries, it was %d x %d with %lld when C was assembled", who, I, J, B->rows, B->cols, (long long)B->nnz, rec.rows, rec.cols,
                (long long)rec.nnz);
    }
  // the table: the recorded column offsets stay (the shapes are the recorded ones), only the arrays may be other ones
  std::vector<BmatBlock> tab(pl->host_table);
  for (int q = 0; q < nb; ++q)
    if (blocks[q]) { tab[q].rp = blocks[q]->rowptr; tab[q].ci = blocks[q]->col; tab[q].val = (const u64 *)blocks[q]->val; }
  const size_t tab_bytes = sizeof(BmatBlock) * (size_t)nb;
  if (std::memcmp(tab.data(), pl->host_table.data(), tab_bytes) != 0) {      // other handles than the recorded ones: the table is rewritten once nothing reads it any more
    MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    MGS_HIP(ctx, hipMemcpy(pl->table, tab.data(), tab_bytes, hipMemcpyHostToDevice));
    pl->host_table.swap(tab);
  }
  if (C->rows && C->nnz)
    hipLaunchKernelGGL(bmat_fill_kernel<true>, dim3(mgs_grid(C->nnz, TB)), dim3(TB), 0, ctx->stream, (long long)C->nnz, C->rows, br, bc, (const BmatBlock *)pl->table,
                       (const int *)((const char *)pl->table + tab_bytes), C->rowptr, (int *)nullptr, (u64 *)C->val);
  MGS_HIP(ctx, hipGetLastError());
  return MGS_OK;
}

int k_csr_bmat_info(const mgs_csr *C, int64_t out[4]) {
  MGS_CHECK(nullptr, C && out, MGS_ERR_INVALID, "mgs_csr_bmat_info: NULL argument");
  out[0] = out[1] = out[2] = out[3] = 0;
  const mgs_reorder_plan *pl = C->reop;
  if (!pl || !pl->is_bmat) return MGS_OK;
  out[0] = pl->n_blocks; out[1] = pl->br; out[2] = pl->bc; out[3] = C->max_row_len;
  return MGS_OK;
}
