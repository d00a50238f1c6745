// rowblock_setup.hip — what the row-block kernels need once per matrix (rowblock.hpp): the launch plan (mgs_plan_csr: row-block bounds, LDS
// budget, far band, halo blocks) and the pattern code of an index array (mgs_build_rowcode: one byte per row + a small table per row block).
#include "rowblock.hpp"

namespace {

// table word of the index i of a row (a word outside the representable ranges makes the block uncodable: returns CODE_BAD)
__device__ __forceinline__ int code_off(int i, int base, int row, int split) {
  if (i < 0) return CODE_NEG;
  if (i >= split) { const int d = (i - split) - row; return (d > -0x10000000 && d < 0x10000000) ? CODE_HALO + d : CODE_BAD; }
  const int o = i - base;
  return (o > -CODE_OFF_MAX && o < CODE_OFF_MAX) ? o : CODE_BAD;
}
// setup pass 1: per row block, elect representatives (smallest row of each distinct tuple), give every row the
// rank of its representative (deterministic: order of first appearance), and size the block's table.  A block
// whose table would exceed half of its index slice is left uncoded (size 0).
__global__ __launch_bounds__(RB) void rowcode_assign_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ idx,
                                                            const int *__restrict__ base, int split, unsigned char *__restrict__ pid,
                                                            unsigned char *__restrict__ isrep, int *__restrict__ blk_ints,
                                                            const double *__restrict__ val /*non-null: tuples include the values*/) {
  __shared__ int s_rep, s_ints, s_np, s_bad;
  const int blk = blockIdx.x, r0 = blk * RB, r1 = min(r0 + RB, n), tid = threadIdx.x, row = r0 + tid;
  const bool valid = row < r1;
  int a = 0, len = 0, bs = 0;
  if (valid) { a = rowptr[row]; len = rowptr[row + 1] - a; bs = base ? base[row] : row; }
  // table budget: half of what the block streams otherwise (4 B per entry index-only, 12 B with values; a table entry
  // costs 4 resp. 12 B) → the same entry count either way
  const int budget = (rowptr[r1] - rowptr[r0]) / 2 - 64;
  bool assigned = !valid, rep = false, ok = true;
  int mypid = 0;
  if (tid == 0) { s_ints = 0; s_np = 0; s_bad = 0; }
  for (int p = 0; p < RB; ++p) {
    if (tid == 0) s_rep = 0x7fffffff;
    __syncthreads();
    if (!assigned) atomicMin(&s_rep, tid);
    __syncthreads();
    const int r = s_rep;
    if (r == 0x7fffffff) break;
    if (!assigned) {
      bool same = true;
      if (tid != r) {
        const int rr = r0 + r, ra = rowptr[rr], rl = rowptr[rr + 1] - ra, rb = base ? base[rr] : rr;
        same = rl == len;
        for (int j = 0; same && j < len; ++j) same = code_off(idx[a + j], bs, row, split) == code_off(idx[ra + j], rb, rr, split);
        if (val) for (int j = 0; same && j < len; ++j) same = __double_as_longlong(val[a + j]) == __double_as_longlong(val[ra + j]);   // same bits
      } else {
        rep = true; s_ints += len; s_np = p + 1;
        for (int j = 0; j < len; ++j) if (code_off(idx[a + j], bs, row, split) == CODE_BAD) s_bad = 1;
      }
      if (same) { assigned = true; mypid = p; }
    }
    __syncthreads();
    if (s_np + s_ints > budget || s_bad) { ok = false; break; }
  }
  if (valid) { pid[row] = ok ? (unsigned char)mypid : 0; isrep[row] = (ok && rep) ? 1 : 0; }
  if (tid == 0) blk_ints[blk] = ok ? s_np + s_ints : 0;
}
// setup pass 2: write the tables (pstart[npat], then the tuples in representative order)
__global__ __launch_bounds__(RB) void rowcode_fill_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ idx,
                                                          const int *__restrict__ base, int split, const unsigned char *__restrict__ pid,
                                                          const unsigned char *__restrict__ isrep, const int *__restrict__ tptr,
                                                          int *__restrict__ tab, const double *__restrict__ val, double *__restrict__ vtab) {
  __shared__ int plen[RB], pstart[RB];
  const int blk = blockIdx.x, r0 = blk * RB, r1 = min(r0 + RB, n), tid = threadIdx.x, row = r0 + tid;
  const int t0 = tptr[blk];
  if (tptr[blk + 1] == t0) return;
  const bool rep = row < r1 && isrep[row];
  int a = 0, len = 0, bs = 0, p = 0;
  if (rep) { a = rowptr[row]; len = rowptr[row + 1] - a; bs = base ? base[row] : row; p = pid[row]; plen[p] = len; }
  const int np = __syncthreads_count(rep);
  if (tid == 0) { int acc = np; for (int q = 0; q < np; ++q) { pstart[q] = acc; acc += plen[q]; } }
  __syncthreads();
  if (rep) {
    tab[t0 + p] = pstart[p];
    for (int j = 0; j < len; ++j) tab[t0 + pstart[p] + j] = code_off(idx[a + j], bs, row, split);
    if (vtab) for (int j = 0; j < len; ++j) vtab[t0 + pstart[p] + j] = val[a + j];     // same indexing as tab (header slots unused)
  }
}

// number of row blocks whose entry count exceeds each of 4 candidate LDS budgets
__global__ void plan_count_kernel(int n, const int *__restrict__ rowptr, int nblocks, int c0, int c1, int c2, int c3, int *__restrict__ out) {
  int vb = blockIdx.x * blockDim.x + threadIdx.x;
  if (vb >= nblocks) return;
  int r0 = vb * RB, r1 = min(r0 + RB, n);
  int cnt = rowptr[r1] - rowptr[r0];
  if (cnt > c0) atomicAdd(&out[0], 1);
  if (cnt > c1) atomicAdd(&out[1], 1);
  if (cnt > c2) atomicAdd(&out[2], 1);
  if (cnt > c3) atomicAdd(&out[3], 1);
}

__global__ void blkptr_kernel(int n, const int *__restrict__ rowptr, int nblocks, int *__restrict__ blkptr) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b <= nblocks) blkptr[b] = rowptr[min(b * RB, n)];
}

__global__ void plan_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col, int nblocks,
                            unsigned long long *__restrict__ farsum /* Σ_rows max |col−row| (owned columns) */, int *__restrict__ out /*[0]=max block nnz,[1]=max row len,[2]=max |col-row| over owned columns,
                                                    [3]=#row blocks touching halo columns,[4]=min block without halo,[5]=max block without halo*/) {
  int vb = blockIdx.x * blockDim.x + threadIdx.x;
  int mx = 0, mr = 0, far = 0;
  unsigned long long fsum = 0;
  if (vb < nblocks) {
    bool halo = false;
    int r0 = vb * RB, r1 = min(r0 + RB, n);
    mx = rowptr[r1] - rowptr[r0];
    for (int q = r0; q < r1; q += 64) atomicMax(&out[6], rowptr[min(q + 64, r1)] - rowptr[q]);
    for (int r = r0; r < r1; ++r) {
      const int a = rowptr[r], e = rowptr[r + 1];
      mr = max(mr, e - a);
      if (e > a) {   // sorted row: extremes are the first entry and the last owned entry
        int rf = max(0, r - col[a]);
        int k = e - 1;
        if (col[k] >= n) halo = true;
        while (k > a && col[k] >= n) --k;
        if (col[k] < n) rf = max(rf, col[k] - r);
        far = max(far, rf); fsum += (unsigned long long)rf;
      }
    }
    if (halo) atomicAdd(&out[3], 1);
    else { atomicMin(&out[4], vb); atomicMax(&out[5], vb); }
    atomicAdd(farsum, fsum);
  }
  for (int off = 32; off > 0; off >>= 1) { mx = max(mx, __shfl_down(mx, off)); mr = max(mr, __shfl_down(mr, off)); far = max(far, __shfl_down(far, off)); }
  if ((threadIdx.x & 63) == 0) { atomicMax(&out[0], mx); atomicMax(&out[1], mr); atomicMax(&out[2], far); }
}

}  // namespace

int mgs_plan_csr(mgs_csr *A) {
  mgs_ctx *ctx = A->ctx;
  A->max_row_len = 0;
  A->lds_cap = 0;
  if (A->rows == 0) return MGS_OK;
  int nblocks = mgs_row_blocks(A);
  if (A->blkptr) { mgs_hip_free(A->blkptr); A->blkptr = nullptr; }
  MGS_TRY(mgs_dev_alloc(ctx, &A->blkptr, (size_t)nblocks + 1));
  hipLaunchKernelGGL(blkptr_kernel, dim3((nblocks + 256) / 256), dim3(256), 0, ctx->stream, A->rows, A->rowptr, nblocks, A->blkptr);
  int *d = nullptr;
  MGS_TRY(mgs_dev_alloc(ctx, &d, 10));   // 7 ints + one 8-byte aligned 64-bit sum at d[8..9]
  const int init[10] = {0, 0, 0, 0, 0x7fffffff, -1, 0, 0, 0, 0};
  MGS_HIP(ctx, hipMemcpyAsync(d, init, sizeof init, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(plan_kernel, dim3((nblocks + 255) / 256), dim3(256), 0, ctx->stream, A->rows, A->rowptr, A->col, nblocks,
                     reinterpret_cast<unsigned long long *>(d + 8), d);
  int h[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  MGS_HIP(ctx, hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  MGS_HIP(ctx, mgs_hip_free(d));
  A->max_row_len = h[1];
  // typical far-band distance = mean over rows of the row's farthest owned column (the max is set by a few
  // odd-shaped boundary aggregates on coarse levels and would mis-size the strip-major sweep)
  unsigned long long fs; memcpy(&fs, &h[8], sizeof fs);
  A->far_band = A->rows ? (int)(fs / (unsigned long long)A->rows) : 0;
  A->far_band_max = h[2];
  // row blocks that read halo columns: usable for overlap when they form a prefix + suffix of the shard
  A->halo_lo_blocks = A->halo_hi_blocks = 0; A->halo_split_ok = false;
  if (A->cols > A->rows) {
    if (h[5] < 0) { A->halo_lo_blocks = nblocks; A->halo_split_ok = false; }          // every block touches the halo
    else {
      const int lo_cnt = h[4], hi_cnt = nblocks - 1 - h[5];
      A->halo_lo_blocks = lo_cnt; A->halo_hi_blocks = hi_cnt;
      A->halo_split_ok = (h[3] == lo_cnt + hi_cnt) && (nblocks - lo_cnt - hi_cnt) > 0;
    }
  }
  A->max_block_nnz = h[0];
  A->max_wave_nnz = h[6];
  A->lds_cap = h[0] < LDS_CAP_MAX ? h[0] : LDS_CAP_MAX;
  if (A->lds_cap < 64) A->lds_cap = 64;
  // LDS budget per workgroup sets the occupancy.  A handful of heavy row blocks (G0 fringes, irregular
  // aggregates on coarse levels) must not size it for everyone: take the smallest budget that still
  // stages ≥ 98.5 % of the row blocks; the rest run their rows from global memory (block-uniform branch).
  const double mean = (double)A->nnz / nblocks;
  if (nblocks >= 64 && (double)A->lds_cap > 1.12 * mean) {
    int cand[4] = {(int)(1.06 * mean) + 8, (int)(1.12 * mean) + 8, (int)(1.25 * mean) + 8, (int)(1.5 * mean) + 8};
    int *dc = nullptr;
    MGS_TRY(mgs_dev_alloc(ctx, &dc, 4));
    MGS_HIP(ctx, hipMemsetAsync(dc, 0, 4 * sizeof(int), ctx->stream));
    hipLaunchKernelGGL(plan_count_kernel, dim3((nblocks + 255) / 256), dim3(256), 0, ctx->stream, A->rows, A->rowptr, nblocks, cand[0], cand[1], cand[2], cand[3], dc);
    int over[4] = {0, 0, 0, 0};
    MGS_HIP(ctx, hipMemcpyAsync(over, dc, sizeof over, hipMemcpyDeviceToHost, ctx->stream));
    MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    MGS_HIP(ctx, mgs_hip_free(dc));
    for (int q = 0; q < 4; ++q)
      if (cand[q] < A->lds_cap && over[q] <= 0.015 * nblocks) { A->lds_cap = cand[q]; break; }
  }
  return MGS_OK;
}

// Builds the pattern code of the index array `idx` (CSR-shaped like rowptr; base = nullptr: offsets from the row;
// indices >= split address the halo payload of a row shard and are coded as slot − row).
int mgs_build_rowcode(mgs_ctx *ctx, int n, const int *rowptr, const int *idx, const int *base, int split, mgs_rowcode **out,
                      const double *val) {
  *out = nullptr;
  if (n <= 0) return MGS_OK;
  const int nblocks = (n + RB - 1) / RB;
  mgs_rowcode *c = new mgs_rowcode();
  c->nblocks = nblocks;
  unsigned char *isrep = nullptr;
  int *ints = nullptr;
  int rc = mgs_dev_alloc(ctx, &c->pid, (size_t)n);
  if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &isrep, (size_t)n);
  if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &ints, (size_t)nblocks + 1);
  if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &c->tptr, (size_t)nblocks + 1);
  std::vector<int> h((size_t)nblocks + 1, 0);
  if (rc == MGS_OK) {
    hipError_t e = hipMemsetAsync(ints, 0, sizeof(int) * ((size_t)nblocks + 1), ctx->stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(rowcode_assign_kernel, dim3(nblocks), dim3(RB), 0, ctx->stream, n, rowptr, idx, base, split, c->pid, isrep, ints, val);
      e = hipGetLastError();                       // launch errors (bad configuration) surface here, not at the later sync
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), ints, sizeof(int) * (size_t)nblocks, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = mgs_fail(ctx, MGS_ERR_HIP, "rowcode pass 1 failed: %s", hipGetErrorString(e));
  }
  if (rc == MGS_OK) {
    int64_t total = 0;
    std::vector<int> sizes;
    for (int q = 0; q < nblocks; ++q) { const int v = h[q]; h[q] = (int)total; total += v; if (v) { c->coded_blocks++; sizes.push_back(v); } }
    h[nblocks] = (int)total;
    c->tab_total = total;
    if (total >= 0x7fffffffLL) c->coded_blocks = 0;      // cannot index the table with 32 bits: leave the matrix uncoded
    if (c->coded_blocks) {
      // table budget in LDS: covers 98.5 % of the coded blocks (the rest walk their rows from global memory)
      std::sort(sizes.begin(), sizes.end());
      c->tab_max = sizes.back();
      c->tab_cap = sizes[(size_t)((sizes.size() - 1) * 0.985)];
      hipError_t e = hipMemcpyAsync(c->tptr, h.data(), sizeof(int) * ((size_t)nblocks + 1), hipMemcpyHostToDevice, ctx->stream);
      if (e != hipSuccess) rc = mgs_fail(ctx, MGS_ERR_HIP, "rowcode table offsets: %s", hipGetErrorString(e));
      if (rc == MGS_OK) rc = mgs_dev_alloc(ctx, &c->tab, (size_t)total + 4);
      if (rc == MGS_OK && val) rc = mgs_dev_alloc(ctx, &c->vtab, (size_t)total + 4);
      if (rc == MGS_OK) {
        hipLaunchKernelGGL(rowcode_fill_kernel, dim3(nblocks), dim3(RB), 0, ctx->stream, n, rowptr, idx, base, split, c->pid, isrep, c->tptr, c->tab, val, c->vtab);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = mgs_fail(ctx, MGS_ERR_HIP, "rowcode pass 2 failed: %s", hipGetErrorString(e));
      }
    }
  }
  if (isrep) mgs_hip_free(isrep);
  if (ints) mgs_hip_free(ints);
  if (rc != MGS_OK || !c->coded_blocks) { mgs_free_rowcode(c); c = nullptr; }
  *out = c;
  return rc;
}
void mgs_free_rowcode(mgs_rowcode *c) {
  if (!c) return;
  if (c->pid) mgs_hip_free(c->pid);
  if (c->tptr) mgs_hip_free(c->tptr);
  if (c->tab) mgs_hip_free(c->tab);
  if (c->vtab) mgs_hip_free(c->vtab);
  delete c;
}
