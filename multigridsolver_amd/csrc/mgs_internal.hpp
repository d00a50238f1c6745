// mgs_internal.hpp — private structures of libmgs.so (gfx950 only; no CPU fallback).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mgs.h"

// what the launcher of a fused pass decided (mgs_hier_post_pass and mgs_hier_pre_pass_info hand it to their callers): filled in by the launch
// path itself while mgs_ctx::report points at one, so a test can tell which arm of the kernels its case ran
struct mgs_launch_report {
  // 0 gather kernel (csr_rowblock_fused_kernel), 1 coded kernel FP64, 2 coded kernel FP32, 3 coded kernel swept group by group, 4 slice kernel
  // (csr_rowblock_slice_kernel), 5 aggregate-parallel pre pass (agg_pre_kernel), 6 grouped pre pass, sequential sweep (csr_group_pre_kernel),
  // 7 grouped pre pass, 512-thread pair kernel (csr_group2_pre_kernel)
  int kernel = -1;
  int u = 0, flags = 0, capv = 0, capi = 0;   // gather width, the kernel's flags word, LDS budgets (values / ints) of a row block
  int bits = 0;                // the launched instantiation: 1 FP32 values, 2 operand without diagonal (ND), 4 packed form (PK)
  const int *tptr = nullptr;   // device: table bounds of the pattern code the launch handed to its kernel (NULL: none, no block is coded)
};
constexpr int MGS_RED_VALS = 32;   // results one reduction can hand to the host (mgs_ctx::red_host)
// mgs_ctx::red_dev (blas1.hip): MGS_DOT_BLOCKS partial slots, then MGS_RED_VALS folded results, then MGS_RED_VALS device-only scalars
// (the first one: the mean of the last k_project_const)
constexpr int MGS_DOT_BLOCKS = 4096;
constexpr int MGS_RED_CAP = MGS_DOT_BLOCKS + 2 * MGS_RED_VALS;
constexpr int MGS_ABSMAX_SLOT = MGS_DOT_BLOCKS + MGS_RED_VALS + 8;   // a device-only scalar: the bits of max_i Σ_j |a_ij| while mgs_eig_lobpcg forms ‖A‖∞ (eig.hip)
static_assert(MGS_ABSMAX_SLOT > MGS_DOT_BLOCKS + MGS_RED_VALS && MGS_ABSMAX_SLOT < MGS_RED_CAP, "the ‖A‖∞ slot lies among the device-only scalars of mgs_ctx::red_dev, behind the mean of k_project_const");
constexpr int MGS_VECS_RING = 8;     // pinned staging slots for the coefficients of mgs_vecs_combine (blockvec.hip)
struct mgs_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  // scratch for reductions (device partials + pinned host landing zone)
  double *dot_part = nullptr; int64_t dot_part_cap = 0;   // per-row-block partials of the dots fused into the SpMV epilogue
  double *red_dev = nullptr;
  std::vector<struct mgs_vec *> ws_free;   // work vectors of the Krylov solvers, kept between solves (mgs_ctx_trim releases them)
  double *red_host = nullptr;       // 2·MGS_RED_VALS doubles, mapped + coherent: [0..MGS_RED_VALS) values, [MGS_RED_VALS] the ticket of the posted-result path
  double *red_host_dev = nullptr;   // the same buffer as the device sees it (NULL: not mappable, copy + synchronize)
  unsigned long long red_ticket = 0;
  int red_cap = 0;
  int n_cu = 256;
  // options
  int opt_xcd_remap = 1;
  int opt_nontemporal = 0;  // non-temporal loads of val/col (measured: no gain with the slice kernel)
  int opt_fuse = 1;         // fused V-cycle passes on square levels
  int opt_fuse_operands = 1; // precomputed operands Â = A·diag(wd), agg[col] for the fused passes (+12 B per entry of memory)
  int opt_spmv_variant = 0;  // 0 auto (stream), 1 force vector
  int opt_graph = 1;
  int opt_graph_split_rows = 1 << 20;   // K-cycle on an unsharded operator with at least this many rows: the fine level's two passes are launched eagerly and only the
                                        // levels below replay from ONE hipGraph that does not depend on (b, x) — its submission hides behind the fine level's pre pass (0: never)
  int opt_valcode = 0;   // pattern tuples include the VALUES (rows with equal index shape and equal values share a tuple): coded blocks stream no
                         // matrix entry at all.  Pays only where coefficients repeat (constant-coefficient / piecewise-constant operators): opt-in.
  int opt_nt_store = 1000000;  // streaming (`nt`) stores of the row-block kernels' outputs on operators with at least this many rows (0: never): SpMV −3.4 %, cycle −1.3 % at 512³
  int opt_split_min_rows = 400000;   // row shards: levels with fewer owned rows exchange first and launch once (no interior/boundary split)
  int opt_rowcode = 1;   // pattern-coded index (8 B per entry streamed instead of 12 where rows repeat their shape)
  int opt_blkptr = 1;    // row-block bounds from the compact blkptr array (0: from rowptr)
  int opt_lds_pad = 0;   // extra dynamic LDS bytes per workgroup (occupancy experiments only)
  int opt_strip = -1;  // strip-major sweep: -1 auto (32 row blocks), 0 off, >0 strip size in row blocks
  int opt_group_strip = 0;       // groups per strip of the grouped pre pass's strip-major sweep (0: from opt_strip)
  int opt_group_order = 0;       // > 0: the grouped pre pass visits its groups in the order of the ONE-BLOCK kernels' strip-major plane sweep, strips of this many
                                 // row blocks, through a table built with the groups (groups hold 1–4 blocks, so a period counted in groups drifts against the planes)
  int opt_merge_ap = 1;          // fused post pass on A·P (merged entries) instead of A with aggregate-mapped columns
  int opt_fuse_dots = 1;         // BiCGSTAB: r̃·v and (t·s, t·t) in the epilogue of the SpMV that produces v resp. t
  int opt_diag_from_values = 1;  // t-form post pass: ωD⁻¹ from the streamed diagonal entry (1 B per row of position) instead of the wd vector (8 B per row)
  int opt_fuse_restrict = 1;  // grouped pre pass: restriction inside the pre-smoothing/residual pass, post pass reads t = b + r
  int opt_group_min_blocks = 1024;  // ... levels with fewer row blocks keep the separate kernels
  int opt_group_sweep = 0;       // bit 0: the t-form post pass sweeps the grouped pre pass's row-block groups (one workgroup per group) instead of single blocks
  int opt_group_concurrent = 0;  // groups of ≤ 2 blocks: 512-thread workgroups sweep both blocks at once (csr_group2_pre_kernel; same bits; measured at 512³:
                                 // 6.59 ms per cycle against 6.50 for the sequential sweep of the same pairs and 6.13 for 4-block groups — kept for A/B)
  int opt_group_min_link = 1;   // ... aggregates two row blocks must share to be grouped (8: keeps a few odd boundary aggregates from pulling blocks of
                                // another plane into the group — 8 % less HBM traffic for that kernel, yet 2 % slower: fewer, fatter workgroups win)
  int opt_group_blocks = 4;    // ... row blocks per group (1..4); same-process A/B at 512³ (tools/studies_r1_r3/ab_group2.py): 4-block groups 6.21 ms per cycle,
                               // pairs 6.34 ms, separate kernels 6.64 ms
  int opt_group_stray_pct = 6; // ... unless more than this share of a level's aggregates leaves its row-block group
  int opt_post_results = 1;   // inner products reach the host through a mapped buffer + ticket the host polls (no copy engine, no interrupt)
  int opt_rowptr_scan = 1;    // coded row blocks take a row's entry range from its pattern's length (wave prefix sum, one rowptr load per wave) instead of
                              // two rowptr loads per row: 4 B per row less to stream (rowblock.hpp: coded_row_range)
  int opt_pre_nodiag = 1;     // grouped pre pass of an unsharded FP64 level: Â's diagonal entries (ω up to three roundings) are streamed as one byte per row,
                              // their distance from ω, instead of a double (7 B per row less, the same bits; 0: the kernels read val_wd as it is)
  int opt_pack7 = 1;          // fused passes of an unsharded FP64 level: coded + staged row blocks whose values span fewer than 8 binades stream a packed
                              // copy of the operand's values, 7 bytes per entry (sign, 3 exponent bits against a per-block base, 52 mantissa bits: the same
                              // bits; 0: every block reads the FP64 array)
  int opt_stage_unroll = 1;   // row-block kernels stage their value slice without a loop in front of the barrier (predicated 16-byte loads / LDS-DMA): −4 … −7 % per cycle
  int opt_blas1_pairs = 1;    // ... pairs per lane of those kernels: 1 = one-shot workgroups (0: capped persistent grid, k: k pairs per lane)
  int opt_blas1_vec = 1;      // axpby / axpbypcz / update+dots move 16 B per lane with four loads per stream in flight (same per-element bits)
  int opt_minres_nt = 0;      // k_minres_update stores w_prev (read again two passes later) with the `nt` hint where nt_store applies; x keeps plain stores.  Off: the gain
                              // is unmeasured (tools/ab_minres.py, profiles/r21_minres.md)
  int opt_aggpre_max_rows = 300000;  // levels with at most this many rows run pre pass + restriction as ONE aggregate-parallel kernel (launch-bound sizes; same bits)
  int opt_emu_split_self = 0;   // tools/emulate_rank.py only: a packed exchange with the rank itself goes out as two messages (a middle rank has two neighbours)
  int opt_kcycle_energy = 0;  // K-cycle coefficients from energy inner products (flexible-CG form; SPD operators) instead of the GCR form of the paper
  int opt_native_graph = 1;   // row shards on the native RCCL transport: capture the whole cycle (exchanges included) in a hipGraph
  int opt_native_overlap = 0; // ... and, inside that graph, run the interior row blocks on a second stream beside pack + exchange (measured on one GPU:
                              // a graph with cross-stream edges costs 0.48 ms of host time per launch and 1.219 vs 1.155 ms per cycle — off by default)
  hipStream_t comm_stream = nullptr;   // second stream of the captured native cycle (fork/join become graph edges)
  unsigned long long opt_epoch = 0;   // bumped by every mgs_ctx_set_option: captured cycles of an older epoch are dropped
  struct mgs_comm *ncomm = nullptr;   // native RCCL all-reduce of the inner products (takes precedence over the callback)
  mgs_allreduce_fn allreduce = nullptr;
  void *allreduce_user = nullptr;
  mgs_launch_report *report = nullptr;   // diagnostics (mgs_hier_post_pass, mgs_hier_pre_pass_info): the next fused-pass launch describes itself here; NULL in every cycle
  // block-vector passes (blockvec.hip): the device slot for a Gram matrix's folded entries and a combine's coefficients, allocated at the first call
  double *vecs_dev = nullptr;
  double *vecs_host = nullptr;                       // MGS_VECS_RING pinned slots: a combine copies the caller's coefficients here before it returns, the device copy reads the slot
  hipEvent_t vecs_ev[MGS_VECS_RING] = {};            // recorded behind each slot's device copy; waited for before the slot is written again
  int vecs_next = 0;
  int64_t vecs_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // mgs_vecs_info: launch decisions of the last mgs_vecs_gram / mgs_vecs_combine
  int64_t eig_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};    // mgs_eig_info: counters of the last mgs_eig_lobpcg (eig.hip)
  int64_t graph_captures = 0;                        // whole-cycle hipGraph captures made on this context (cycle.hip: capture_exec)
};
// the one statement that fills mgs_launch_report: what a fused-pass launcher launched (NULL in every cycle: nothing written)
static inline void report_launch(const mgs_ctx *ctx, int kernel, int u, int flags, int capv, int capi, int bits = 0, const int *tptr = nullptr) {
  if (ctx->report) *ctx->report = {kernel, u, flags, capv, capi, bits, tptr};
}

// pattern code of a CSR-shaped index array (format: rowblock.hpp; built by rowblock_setup.hip): one byte per row + a small table per row block
struct mgs_rowcode {
  unsigned char *pid = nullptr;  // n: the row's tuple within its row block's table
  int *tptr = nullptr;           // nblocks+1: table slice of each row block in tab (empty: block keeps its index array)
  int *tab = nullptr;            // per coded block: pstart[npat], then the offset tuples
  double *vtab = nullptr;        // option valcode: the tuples' values, indexed like tab (rows are one tuple only if index AND values repeat)
  int tab_max = 0, tab_cap = 0;  // largest table / LDS budget covering 98.5 % of the coded blocks (ints)
  int coded_blocks = 0, nblocks = 0;
  int64_t tab_total = 0;
};

// packed copy of an FP64 operand's values (option pack7; kernels_aux.hip: pack7_scan_kernel / pack7_fill_kernel)
struct mgs_pack7 {
  unsigned char *data = nullptr;   // 112-byte records of sixteen entries, padded to a whole record
  int *e0 = nullptr;               // nblocks: base exponent of each row block's slice, −1 = the block reads the FP64 array
  int64_t nent = 0;                // entries of the source array
  int nblocks = 0;
  bool nd = false;                 // the source is the operand without diagonal entries (val_nd)
  bool dirty = true;               // out of step with its source (the level's dirty bits, kept here because the launchers see the copy alone)
  int ran = -1;                    // the last launch that could have read it did (1) or did not (0); −1: none yet (mgs_hier_pack_info)
};
static inline bool mgs_pack7_serves(const mgs_pack7 *p, bool nd) { return p && !p->dirty && p->nd == nd; }      // a launch that streams val_nd (nd) or a whole operand may read this copy

// Field-wise constant null space (MGS_NULLSPACE_FIELDS, mgs_csr_set_nullspace_fields): the span of the indicators of up to 8 disjoint row sets.
// Owned by its matrix.  means: where the projection's sum pass leaves m_f = sum_f / n_f on the device (one set of slots per matrix, not per
// context: two matrices on one context do not collide).
struct mgs_nsfields {
  int nfields = 0;
  int64_t counts[MGS_NULLSPACE_MAX_FIELDS] = {0, 0, 0, 0, 0, 0, 0, 0};   // rows per field
  signed char *labels = nullptr;   // device, rows entries: the field of every row, −1 = in no field
  double *means = nullptr;         // device, MGS_NULLSPACE_MAX_FIELDS slots
};
struct mgs_csr {
  mgs_ctx *ctx = nullptr;
  int rows = 0, cols = 0;
  int64_t nnz = 0;
  int *rowptr = nullptr;  // rows+1
  int *blkptr = nullptr;  // rowptr sampled every 256 rows (row-block bounds), built by mgs_plan_csr
  int *col = nullptr;     // nnz (+pad)
  double *val = nullptr;  // nnz (+pad)
  bool owns = true;
  // launch plan of the row-block stream kernel (computed at upload)
  int max_row_len = 0;
  int far_band = 0;      // typical (mean over rows) farthest owned column distance
  int far_band_max = 0;  // max |col - row| over owned columns
  int halo_lo_blocks = 0, halo_hi_blocks = 0;  // leading / trailing row blocks that read halo columns
  bool halo_split_ok = false;                  // no other block does → interior rows can overlap the exchange
  int lds_cap = 0;  // entries staged per block
  int max_block_nnz = 0;
  int max_wave_nnz = 0;   // max entries of a 64-row group
  mgs_rowcode *code = nullptr;   // pattern code of col (mgs_csr_optimize; owned unless this is a view)
  bool code_tried = false;
  // views made by mgs_spmv_dots only: (y·w1, y·y) of the product y = A·x accumulated in the SpMV's epilogue (one partial pair per row block)
  const double *dot_w1 = nullptr; double *dot_part = nullptr;
  const struct mgs_groups *sweep = nullptr;   // views only: launch the coded kernel group by group over these row-block groups (option group_sweep)
  const unsigned char *dpos = nullptr;   // views of the t-form post pass only (not owned): position of the diagonal inside every row, so the
  double dpos_omega = 0.0;               // kernel takes ω/a_ii from the values it streams anyway instead of reading wd (8 B → 1 B per row)
  const float *val32 = nullptr;   // views of the fused passes on an FP32 level only (not owned): the values rounded to float; the kernels' float forms read
                                  // these instead of val (products widened to FP64 before they are added)
  mgs_pack7 *pk7 = nullptr;       // views of the fused passes on an unsharded FP64 level only (not owned): the packed copy of val (option pack7)
  int *origin = nullptr;   // coarse operators built by the device setup: the finest-level row each row descends from (its aggregate's
                           // leader, chained through the levels) — the index space the matching's tie-breaks work in; NULL = identity
  // matrices assembled from device triples (ingest.hip); the map is kept on request (keep_map) for mgs_csr_update_values_coo_dev
  bool coo_map = false;
  int *coo_src = nullptr;   // coo_ntrip: source position of every triple in (row, column, input order) order
  int *coo_run = nullptr;   // nnz + 1: first sorted triple of every entry; entry e sums coo_src[coo_run[e] .. coo_run[e + 1])
  int64_t coo_ntrip = 0;
  int coo_max_row = 0;      // most triples one row received
  int nullspace = MGS_NULLSPACE_NONE;   // mgs_csr_set_nullspace: what the caller declared (hierarchies and Krylov solvers act on it)
  mgs_nsfields *nsf = nullptr;          // nullspace == MGS_NULLSPACE_FIELDS: the labels, the counts and the means' device slots (owned)
  struct mgs_spgemm_plan *spg = nullptr;   // matrices built by mgs_csr_spgemm (spgemm.hip; owned): the row bins its numeric pass launches over
  struct mgs_add_plan *addp = nullptr;     // matrices built by mgs_csr_add (csr_algebra.hip; owned): the row bins mgs_csr_add_numeric launches over
  struct mgs_extract_plan *extp = nullptr; // matrices built by mgs_csr_extract (extract.hip; owned): the bins it counted and, with keep_map, the source position of every entry
  struct mgs_reorder_plan *reop = nullptr; // matrices built by mgs_csr_permute or mgs_csr_bmat (reorder.hip; owned): the kept source map, or the block table and what it recorded of the blocks
  bool halo_cols = false;   // generated as a row shard (mgs_csr_poisson3d on a plane range): the columns beyond the rows are halo columns
};
// a row shard as far as the library can tell: more columns than rows AND generated as a shard or living in a context that sums over ranks
// (a rectangular matrix of a single-process context is just a rectangular matrix)
static inline bool mgs_csr_is_shard(const mgs_csr *A) { return A->cols > A->rows && (A->halo_cols || A->ctx->allreduce || A->ctx->ncomm); }
constexpr int MGS_RB = 256;   // rows per row block of the row-block kernels (rowblock.hpp and its four units) == their threads per workgroup
static inline int mgs_row_blocks(const mgs_csr *A) { return (A->rows + MGS_RB - 1) / MGS_RB; }

struct mgs_vec {
  mgs_ctx *ctx = nullptr;
  int64_t n = 0;
  double *d = nullptr;
  bool owns = true;
};

struct mgs_xfer {
  mgs_ctx *ctx = nullptr;
  int n_fine = 0, n_coarse = 0;
  bool aggregation = false;
  // aggregation form
  int *agg = nullptr;      // n_fine, -1 = not aggregated (G0)
  int *cptr = nullptr;     // n_coarse+1: member list offsets (Pᵀ rowptr)
  int *members = nullptr;  // nnz(P): fine rows sorted by aggregate (Pᵀ col)
  int *corigin = nullptr;  // n_coarse: origin (see mgs_csr) of every aggregate, handed to the coarse operator
  int *halo_cmap = nullptr;   // row shards (mgs_galerkin_shard): coarse column (n_coarse + coarse halo slot, −1 = not aggregated) of every fine halo slot
  int n_halo_fine = 0, n_halo_coarse = 0;
  int64_t nnz = 0;
  // general form
  mgs_csr *P = nullptr, *Pt = nullptr;
};

// native RCCL transport (comm_rccl.hip)
struct mgs_comm;
struct mgs_xfer_op { const double *sptr; double *rptr; size_t count; int peer; };   // one ncclSend (sptr) or ncclRecv (rptr)
int mgs_comm_exchange_ops(mgs_comm *c, const mgs_xfer_op *ops, int nops);             // one group; ops of a peer are matched in order
int mgs_comm_allgather(mgs_comm *c, const double *send, double *recv, size_t count);
int mgs_comm_allreduce_sum(mgs_comm *c, double *buf, size_t count);
bool mgs_comm_capturable(const mgs_comm *c);   // false for the file-based stand-in of the tests (host-synchronous calls)
// peer-to-peer transport behind the same three operations (comm_p2p.hip): IPC-mapped windows, one kernel per exchange
struct mgs_p2p;
int mgs_p2p_create(mgs_ctx *ctx, int world, int rank, size_t slot_doubles, void *handle_out, mgs_p2p **out);
int mgs_p2p_connect(mgs_p2p *c, const void *handles);
void mgs_p2p_destroy(mgs_p2p *c);
int mgs_p2p_info(const mgs_p2p *c, long long out[6]);
int mgs_p2p_selftest(mgs_p2p *c, hipStream_t s, int rounds, long long *mismatches);
int mgs_p2p_exchange_ops(mgs_p2p *c, hipStream_t s, const mgs_xfer_op *ops, int nops);
int mgs_p2p_allgather(mgs_p2p *c, hipStream_t s, const double *send, double *recv, size_t count);
int mgs_p2p_allreduce_sum(mgs_p2p *c, hipStream_t s, double *buf, size_t count);
// halo plan of one sharded level for the native exchange
struct mgs_native_plan {
  mgs_comm *comm = nullptr;
  int *send_idx = nullptr;          // device: owned rows the peers need, peer after peer
  std::vector<int> scnt, rcnt;      // per peer
  int64_t ns = 0, nr = 0;
  double *sendbuf = nullptr;        // device, ns doubles
  // Pack-free form: a peer's send list that is a few contiguous row ranges (plane shards: one) is sent straight from the source
  // vector, one ncclSend per range, and the peer posts one ncclRecv per range — no pack kernel.  The ranges a rank sends are
  // its own decision (sseg, from send_idx); what it receives it is told by its peers (rseg, shipped by the host side at setup:
  // mgs_hier_native_send_segments → mgs_hier_set_native_recv_segments, which also switches this rank's sends to ranges).
  std::vector<std::vector<int>> sseg_start, sseg_len, rseg_len;   // per peer
  std::vector<std::vector<int>> pseg_len, prseg_len;              // per peer: message lengths of the packed form (one per peer; see emu_split_self)
  bool seg_ok = false;      // every peer's send list splits into at most MGS_MAX_SEG ranges
  bool use_seg = false;     // receive segmentation installed on this rank (collective call): sends go out as ranges
};
constexpr int MGS_MAX_SEG = 8;
struct mgs_hier;
// replicated coarse tail driven natively: all-gather of the right-hand side, tail cycle, own slice back
struct mgs_native_tail {
  mgs_comm *comm = nullptr;
  mgs_hier *tail = nullptr;         // not owned
  int maxn = 0, n_t = 0, my_off = 0, n_loc = 0;
  bool even = false;                // every rank holds maxn rows: the gathered buffer is the tail's right-hand side as it stands
  double *send = nullptr, *all = nullptr;   // maxn / world·maxn doubles
  int *gidx = nullptr;              // n_t: position of global tail row i in `all`
  mgs_vec *b = nullptr, *x = nullptr;
  int *halo_global = nullptr;       // device: global tail row of every halo slot of the last sharded level (mgs_hier_set_native_tail_halo)
  int n_halo_global = 0;
};

// Aggregate-complete row-block groups of a level (kernels_fused.hip, "grouped pre pass"): one workgroup sweeps the 1–2 row
// blocks of a group, keeps their residuals in LDS and restricts every aggregate that lies inside the group — the
// restriction kernel and the residual vector's trip through HBM disappear.  Aggregates that leave their group
// ("strays": odd shapes at domain boundaries) are restricted afterwards from the residuals their member rows also store.
struct mgs_groups {
  int ngroups = 0, nblocks = 0, nstray = 0, plane_groups = 0, max_blocks = 1;
  int *gdesc = nullptr;                 // 32 ints per group: blocks[4], entry bounds lo[4]/hi[4], aggregate ranges lo[4]/hi[4]
  int *gblk = nullptr;                  // 4 per group: its row blocks, ascending (−1: unused slot)
  int *afirst = nullptr;                // nblocks+1: first aggregate whose first member lies in row block b (ids ascend with it)
  unsigned long long *acode = nullptr;  // n_coarse: count | first position | position deltas (10 bits each) in the group's 1024-entry
                                        // residual buffer; 0 = stray
  unsigned *wmask = nullptr;            // (n+31)/32 bit mask: rows that also store r (members of stray aggregates)
  int *stray = nullptr;                 // stray aggregate ids
  int *gorder = nullptr; int gorder_per_xcd = 0;   // option group_order: group of workgroup (xcd, idx) at [xcd·per_xcd + idx], −1 = none
};
struct mgs_level {
  const mgs_csr *A = nullptr;
  bool own_A = false;
  mgs_xfer *T = nullptr;  // to next level
  int n = 0;              // owned rows
  int n_ext = 0;          // owned + halo
  mgs_vec *dinv = nullptr, *r = nullptr, *tmp = nullptr;
  mgs_vec *wd = nullptr;       // ω·dinv (fused passes); row shards: n_ext entries, the halo part holds the owners' values
  mgs_vec *hbuf = nullptr;     // halo payload of the fused pre pass (row shards): the peers' raw b of the rows this shard sees as halo
  bool halo_dinv = false;      // row shards: dinv's halo part has been fetched from the owners (one exchange at setup)
  int *cmap_ext = nullptr;     // row shards: coarse column of every local column (owned: agg, halo slot: T->halo_cmap), n_ext ints
  double *val_wd = nullptr;    // setup-time operand of the fused pre pass: a_ij·wd_j, so A·(wd∘b) = Â·b needs one gather
  int *col_agg = nullptr;      // setup-time operand of the fused post pass: agg[col_ij], so (A·Pe) gathers e_c directly
  mgs_rowcode *code_agg = nullptr;   // pattern code of col_agg (offsets from agg[row])
  mgs_csr *AP = nullptr;             // setup-time operand of the fused post pass, option merge_ap: A·P with the entries of a row that fall into one
  mgs_rowcode *code_ap = nullptr;    // aggregate summed (5 instead of 7 entries per row on the 7-point operator) and its pattern code (offsets from agg[row])
  mgs_rowcode *code_pre = nullptr;   // row shards: pattern code of col with tagged halo words (pre pass reads b + payload)
  mgs_rowcode *code_hat = nullptr;   // option valcode: pattern code of (col, val_wd) for the pre pass on Â
  // operand precision (mgs_hier_set_operand_precision): FP32 copies of the two setup-time operands' values, rounded to nearest from the
  // FP64 arrays above (which stay the source of truth and stay allocated: switching back is free and bit-identical)
  int op_bits = 64;                  // what the level was switched to; whether a cycle really runs on the copies: mgs_level_runs_f32 (hier_operands.hip)
  float *val_wd32 = nullptr;         // nnz + 8 floats
  float *ap_val32 = nullptr;         // nnz(A·P) + 8 floats
  unsigned char *dpos = nullptr;     // position of the diagonal entry inside each row (255: none / beyond 254), see mgs_csr::dpos
  mgs_groups *grp = nullptr;         // aggregate-complete row-block groups (grouped pre pass = pre pass + restriction in one kernel)
  bool grp_tried = false;
  // option pre_nodiag: Â's diagonal entry is ω after three roundings for every row, so the grouped pre pass streams val_wd without it
  double *val_nd = nullptr;          // nnz − rows + 8 doubles: val_wd in storage order, each row's diagonal entry left out (row i from rowptr[i] − i)
  signed char *nd_code = nullptr;    // rows bytes: bit pattern of Â_ii minus bit pattern of nd_omega (a few units of the last place)
  double nd_omega = 0.0;             // ω that nd_code counts from
  bool nd_tried = false, nd_ok = false;   // eligibility, decided once: grouped, unsharded, every row holds exactly one diagonal entry
  // option pack7: packed copies of the pre pass's operand (val_nd where the level streams it, val_wd otherwise) and of A·P's values
  mgs_pack7 *pk_hat = nullptr, *pk_ap = nullptr;
  mgs_vec *kc1 = nullptr, *kv1 = nullptr, *kc2 = nullptr, *kv2 = nullptr, *kr = nullptr;   // K-cycle work vectors
  double *kscal = nullptr;     // K-cycle scalars (device)
  unsigned dirty = ~0u;        // OPD_* bits: the derived operands that are out of step with their sources (or do not exist yet), see below
  mgs_vec *b = nullptr, *x = nullptr;  // coarse-level rhs / solution (levels >= 1)
  mgs_native_plan *nx = nullptr;       // native RCCL halo exchange of this level (row shards)
  signed char *ns_lab = nullptr;       // levels >= 1 under a fine operator with MGS_NULLSPACE_FIELDS: the field of every row (an aggregate takes its first member's), owned
};

// The derived operands of a level's fused passes and the ONE record of "this array is out of step with its source" (hier_operands.hip allocates, fills and frees them).
// The chain: wd = ω·D⁻¹ → val_wd = Â → val_nd + nd_code, val_wd32, the value-carrying codes; A → A·P → ap_val32; the packed copies follow val_nd / val_wd and A·P (their
// bit is mgs_pack7::dirty).  A bit is set by mgs_operands_mark (new ω, new values, a freed array) and cleared by the one fill of its array: clear = exists and in step.
enum : unsigned { OPD_WD = 1, OPD_HAT = 2, OPD_ND = 4, OPD_HAT32 = 8, OPD_CODES = 16, OPD_AP = 32, OPD_AP32 = 64, OPD_PACKS = 128 /* asks a fill for the packed copies */ };
static inline bool mgs_operand_in_step(const mgs_level &L, unsigned bit) { return !(L.dirty & bit); }
static inline bool mgs_level_nd_ready(const mgs_level &L) { return L.val_nd && L.nd_code && L.nd_ok && mgs_operand_in_step(L, OPD_ND); }      // the compact operand of the grouped pre pass can be streamed (and packed)

struct mgs_hier {
  mgs_ctx *ctx = nullptr;
  std::vector<mgs_level> lev;
  double omega = 0.5;
  int nu1 = 1, nu2 = 1;
  bool finalized = false;
  int bad_diag0 = 0;       // rows of the finest operator with a missing or zero diagonal: refused as soon as that level would be smoothed
  int kcycle_levels = 0;   // levels 1..kcycle_levels solve their coarse problem with 2 GCR steps (K-cycle)
  bool kcycle_entry = false;   // ... and so does level 0 when the hierarchy is entered from x = 0 (replicated tail of a row-sharded hierarchy whose
                               // K-cycle reaches the last sharded level: that level IS the tail's level 0)
  double corr_scale = 1.0; // over-correction: x ← x + σ·P e_c (σ = 1: the reference's form, bicg.cpp:48)
  bool additive = false;   // bicg.cpp:59: multigrid_solve(v) + M2(v) instead of the multiplicative form (M2 = ωD⁻¹)
  // coarsest direct solve
  int nc = 0;
  double *inv = nullptr;  // nc*nc dense inverse (row-major)
  int ns_nf = 0;                                       // MGS_NULLSPACE_FIELDS: fields and rows per field of the coarsest level (mgs_hier_finalize counts them,
  double ns_ccount[MGS_NULLSPACE_MAX_FIELDS] = {0};    // mgs_hier_refresh regularises with the same)
  int coarse_sweeps = 0;  // > 0: coarsening stalled above the dense limit → the coarsest level is smoothed, not solved
  mgs_halo_fn halo = nullptr;
  void *halo_user = nullptr;
  mgs_halo_fn halo_begin = nullptr, halo_end = nullptr;   // split-phase exchange (overlap with interior rows)
  mgs_halo_fused_fn halo_fused = nullptr;                  // payload exchange of the fused passes on row shards
  mgs_native_tail *ntail = nullptr;  // native form of the replicated tail (takes precedence over `coarse`)
  bool native = false;               // some level exchanges natively: sharded semantics even without callbacks
  mgs_coarse_fn coarse = nullptr;   // replaces the dense coarsest solve (replicated tail of a sharded hierarchy)
  void *coarse_user = nullptr;
  // hipGraph cache of one V-cycle
  // small cache of captured cycles keyed by (b, x, zero_guess)
  struct GraphSlot { hipGraphExec_t exec = nullptr; const double *b = nullptr; double *x = nullptr; int zero = -1; unsigned long long stamp = 0; };
  static constexpr int kGraphSlots = 16;   // BiCGSTAB alternates two (rhs, out) pairs; flexible GCR(m) cycles through m directions (restart 10: ten pairs)
  GraphSlot graphs[kGraphSlots];
  unsigned long long graph_clock = 0;
  unsigned long long graph_epoch = 0;   // ctx->opt_epoch the cached graphs were captured under
  // native transport under capture: the first cycles run eagerly (RCCL sets up its peer connections lazily, which a
  // capturing stream does not allow); a failed capture switches the hierarchy back to eager launches for good
  int native_eager_runs = 0;
  bool native_graph_failed = false;
  bool capturing = false;
  hipGraphExec_t coarse_exec = nullptr;  // split launch (opt_graph_split_rows): coarse_solve(level 1) on the level's own buffers, captured once
  bool coarse_launch = false;            // set around the eager fine-level passes: coarse_solve(h, 1, ..) replays coarse_exec
  // mgs_hier_refresh: counters of mgs_hier_refresh_info and the device flags one refresh reads back at its end
  int64_t refresh_count = 0, refresh_kept_graphs = 0, refresh_dev_levels = 0;
  int *nd_flag = nullptr;          // option pre_nodiag: rows whose diagonal entry of Â does not fit nd_code (device counter)
  int *refresh_flags = nullptr;   // [0] rows with a missing or zero diagonal (all levels), [1] entries outside the kept coarse patterns
  bool refresh_failed = false;    // the last refresh ended with MGS_ERR_NUMERIC: un-finalized until a later refresh succeeds
  std::vector<hipEvent_t> fork_events;   // fork/join events of the captured native cycle (two per overlapped exchange)
  size_t fork_used = 0;
};

// ------------------------------------------------------------------ device memory arena (mgs_api.hip)
// Every device allocation of the library goes through these two (never hipMalloc / hipFree directly: tests/test_abi.py greps for it).  With an arena (MGS_ARENA_GB = N, or mgs_arena_reserve) the library takes
// ONE hipMalloc of N GiB at its first allocation and places operators and vectors inside it (first fit, lowest address first, 2 MiB
// alignment for anything of 1 MiB or more, blocks coalesced on release); requests that do not fit fall through to hipMalloc.  Without
// one (default) they are hipMalloc / hipFree.  Why: DESIGN.md §5 "process to process".
hipError_t mgs_hip_malloc(void **p, size_t bytes);
hipError_t mgs_hip_free(void *p);
static inline void mgs_free_nsfields(mgs_nsfields *F) {      // the record of a field-wise null space with its two device arrays (NULL: nothing)
  if (!F) return;
  if (F->labels) mgs_hip_free(F->labels);
  if (F->means) mgs_hip_free(F->means);
  delete F;
}

// ------------------------------------------------------------------ error plumbing
extern thread_local std::string g_mgs_last_error;
int mgs_fail(mgs_ctx *ctx, int code, const char *fmt, ...);

#define MGS_HIP(ctx, call)                                                              \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess)                                                               \
      return mgs_fail((ctx), MGS_ERR_HIP, "%s failed: %s (%s:%d)", #call,               \
                      hipGetErrorString(e_), __FILE__, __LINE__);                       \
  } while (0)

#define MGS_CHECK(ctx, cond, code, ...)                                                 \
  do {                                                                                  \
    if (!(cond)) return mgs_fail((ctx), (code), __VA_ARGS__);                           \
  } while (0)

#define MGS_TRY(expr)                                                                   \
  do {                                                                                  \
    int rc_ = (expr);                                                                   \
    if (rc_ != MGS_OK) return rc_;                                                      \
  } while (0)

// ------------------------------------------------------------------ kernel launchers
// (kernels_spmv.hip; the fused passes and the grouped pre pass: kernels_fused.hip; plan and pattern code: rowblock_setup.hip)
enum { MGS_OP_SPMV = 0, MGS_OP_RESIDUAL = 1, MGS_OP_JACOBI = 2, FUSE_PRE = 3, FUSE_POST = 4,
       FUSE_POST_MAPPED = 5 /* FUSE_POST whose column array already holds agg[col] */ };
int mgs_launch_fused(const mgs_csr *A, int which, const double *wd, const double *bvec, const double *xin, const int *agg,
                     const double *ec, double *out, double *out2);
int mgs_launch_csr_op(const mgs_csr *A, int op, const double *x, const double *b,
                      const double *dinv, double omega, double *out);
// row blocks [blk_lo, blk_hi) of a virtual numbering in which the blocks >= gap_at are shifted by gap_len (one launch over
// the leading and trailing boundary blocks of a row shard: range [0, lo + nb − hi), gap_at = lo, gap_len = hi − lo)
int mgs_launch_csr_op_range(const mgs_csr *A, int op, const double *x, const double *b,
                            const double *dinv, double omega, double *out, int blk_lo, int blk_hi, int gap_at = 0x7fffffff, int gap_len = 0);
int mgs_launch_fused_range(const mgs_csr *A, int which, const double *wd, const double *bvec, const double *xin, const int *agg,
                           const double *ec, double *out, double *out2, const double *hv, int blk_lo, int blk_hi,
                           int gap_at = 0x7fffffff, int gap_len = 0);
int k_scale_vals(mgs_ctx *ctx, const mgs_csr *A, const double *wd, double *out);            // out_k = a_k·wd[col_k] (row shards: wd covers the halo columns too)
int k_diag_count(const mgs_csr *A, int *bad_count_host);                                       // rows that do not hold exactly one entry with col == row
int k_drop_diag_vals(mgs_ctx *ctx, const mgs_csr *A, const double *val, double omega, double *out, signed char *code, int *bad_dev);
                                                                                               // out: val without each row's diagonal entry (row i from rowptr[i] − i); code[i]: that entry's distance
                                                                                               // from omega in units of the last place; rows beyond ±127 are added to *bad_dev
int k_pack7(mgs_ctx *ctx, const int *blkptr, int nblocks, int nd_rows, const double *src, int *e0, unsigned char *out);   // packed copy of src (nd_rows >= 0: of the
                                                                                               // operand without diagonal entries of a matrix of nd_rows rows), e0 per row block
int k_map_cols(mgs_ctx *ctx, const mgs_csr *A, const int *cmap, int *out);                     // out_k = cmap[col_k]
int k_concat_i32(mgs_ctx *ctx, const int *a, int na, const int *b, int nb, int *out);
int k_tail_scatter(mgs_ctx *ctx, const double *xt, int my_off, int n_loc, const int *halo_global, int n_halo, double *x);   // x[0..n_loc) = xt[my_off..], x[n_loc+s] = xt[halo_global[s]]
int mgs_plan_csr(mgs_csr *A);
int mgs_build_rowcode(mgs_ctx *ctx, int n, const int *rowptr, const int *idx, const int *base, int split, mgs_rowcode **out,
                      const double *val = nullptr);
bool mgs_rowcode_usable(const mgs_csr *A, bool any = false);
int mgs_launch_coded_range(const mgs_csr *A, int op, const double *x, const double *b, const double *dinv, double omega,
                           const double *xin, const int *agg, double *out, const double *hv, int split, int blk_lo, int blk_hi,
                           int gap_at = 0x7fffffff, int gap_len = 0);
void mgs_free_rowcode(mgs_rowcode *c);
int mgs_build_groups(mgs_ctx *ctx, const mgs_csr *A, const mgs_xfer *T, mgs_groups **out);
void mgs_free_groups(mgs_groups *g);
// t = b + (b − Â·x) and r_c = Pᵀ(b − Â·x) in one pass over the groups of G; x = gather source (b itself, or with hv/split the
// halo payload of a row shard); strays' member rows also store r into r_out, restricted by the trailing small kernel
// val_nd, nd_code (option pre_nodiag, unsharded FP64 levels): Â's values without the diagonal entries, and each diagonal entry as its distance
// from omega (k_drop_diag_vals); coded + staged blocks then stream these instead of val — the same bits, 7 bytes per row less
int mgs_launch_group_pre(const mgs_csr *Ahat, const mgs_groups *G, const mgs_xfer *T, const double *x, const double *b,
                         double *t_out, double *r_out, double *rc_out, const double *hv, int split,
                         const double *val_nd = nullptr, const signed char *nd_code = nullptr, double omega = 0.0, mgs_pack7 *pk = nullptr);
                         // pk: packed copy of the operand the coded + staged blocks stream (val_nd if given, Ahat->val otherwise), or NULL
// (kernels_aux.hip; the BLAS-1 updates and reductions among these: blas1.hip)
int k_diag_inv(const mgs_csr *A, double *dinv, int *bad_count_host);
int k_diag_inv_async(const mgs_csr *A, double *dinv, int *bad_dev);   // no host round trip: bad rows are added to *bad_dev
int k_diag_pos(const mgs_csr *A, unsigned char *dpos);
int k_restrict_agg(mgs_ctx *ctx, int nc, const int *cptr, const int *members, const double *r, double *rc);
int k_agg_pre(const mgs_csr *A, const double *valhat, const double *b, const double *hv, const mgs_xfer *T, double *r_out, double *rc_out,
              const float *valhat32 = nullptr);   // small levels: pre pass + restriction, one dispatch (valhat32: the FP32 copy of valhat is read instead)
int k_round_vals(mgs_ctx *ctx, const double *in, float *out, int64_t n);   // out_k = (float)in_k, round to nearest: the FP32 operand copies
int k_prolong_agg(mgs_ctx *ctx, int n, const int *agg, const double *ec, double *x, int add);
int k_fill(mgs_ctx *ctx, double *d, int64_t n, double v);
int k_jacobi_zero(mgs_ctx *ctx, int n, double omega, const double *dinv, const double *b, double *x);   // x = (ωD⁻¹)b: the first sweep from x = 0
int k_rand(mgs_ctx *ctx, double *d, int64_t n, uint64_t seed, int64_t off);
int k_axpby(mgs_ctx *ctx, int64_t n, double a, const double *x, double b, double *y);
int k_axpbypcz(mgs_ctx *ctx, int64_t n, double a, const double *x, double b, const double *y, double c, double *z);
int k_dot(mgs_ctx *ctx, int64_t n, const double *x, const double *y, double *out_host);
// r = ax − θ·bx (t = fl(θ·bx_i), r_i = fl(ax_i − t)) with ‖r‖² = k_dot(r, r) bit for bit, one pass; r may be ax or bx; out_host = NULL: folded, not fetched
int k_eig_residual(mgs_ctx *ctx, int64_t n, const double *ax, const double *bx, double theta, double *r, double *out_host);
int k_dense_gemv(mgs_ctx *ctx, int n, const double *M, const double *b, double *x);
int k_dot_dev(mgs_ctx *ctx, int64_t n, const double *x, const double *y, double *out_dev);
int k_update_dot2(mgs_ctx *ctx, int64_t n, double a, const double *x, double b, const double *y, double *z, const double *w, double *out_host2);
int k_dot2(mgs_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w, double *out_host2);
// mgs_pcg's two passes: direction with the lagged x update (first != 0: p ← z, neither p read nor x touched; else x ← x + a·p, p ← z + beta·p)
// and the residual in place (r ← r − a·q, out_host2[0] = ‖r‖²)
int k_pcg_direction(mgs_ctx *ctx, int64_t n, int first, double a, double beta, double *x, double *p, const double *z);
int k_pcg_residual(mgs_ctx *ctx, int64_t n, double a, double *r, const double *q, double *out_host2);
// (minres.hip) mgs_minres's one pass of its own: the new search direction over the one before last, and the x update with it.  Per entry
// t = inv_g·z − a3·w_prev; t = t − a2·w; wn = t/a1; w_prev = wn; x = x + step·wn — every product, sum and quotient rounded on its own
// (tests/minres_ref.py: update_ref restates the bits).  48 B per row: read z, w_prev, w, x; write w_prev, x.
int k_minres_update(mgs_ctx *ctx, int64_t n, double inv_g, double a3, double a2, double a1, double step,
                    const double *z, double *w_prev /* in: w_{j−1}, out: w_{j+1} */, const double *w, double *x);
// Reductions that end in a host look (k_dot, k_dot2, k_dot2_finish, mgs_spmv_dots) take out_host = NULL as "enqueue and fold, do not fetch": the
// same launches, nothing posted, the folded values left in red_dev[MGS_DOT_BLOCKS ..] for the next kernel on the stream (mgs_pcg_plan).
int mgs_blas1_grid(const mgs_ctx *ctx, int64_t n2);          // workgroups of a 16-byte BLAS-1 launch over n2 pairs (grid_vec)
int mgs_blas1_grid_capped(const mgs_ctx *ctx, int64_t n);   // ... of an 8-byte grid-stride launch over n entries (grid_cap)
int mgs_ensure_dot_part(mgs_ctx *ctx, int64_t doubles);   // per-workgroup partial pairs of one-shot reduction launches
int k_dot2_finish(mgs_ctx *ctx, int nb, const double *part /*[2][nb]*/, double *out_host2);   // second stage + rank reduction + host copy
// y = A·x with (y·w1, y·y) from the same pass where the pattern-coded kernel serves A (else SpMV + k_dot2): BiCGSTAB's
// v = A·p̂ with r̃·v (bicg.cpp:107-108) and t = A·ŝ with (t·s, t·t) (bicg.cpp:117-118)
int mgs_spmv_dots(const mgs_csr *A, const double *x, double *y, const double *w1, double *out_host2);
int k_mdot(mgs_ctx *ctx, int64_t n, int K, const double *a, const double *const *b, double *out_dev, double *out_host);   // a·b_k, k < K ≤ 16, one pass
int k_maxpy_dot2(mgs_ctx *ctx, int64_t n, int K, const double *x, const double *const *w, const double *coef, double *z, const double *u, const double *u2, double *out_host2);
int k_kc_update_r(mgs_ctx *ctx, int n, const double *scal, const double *r, const double *v1, double *rp);
int k_kc_orth_dots(mgs_ctx *ctx, int n, bool energy, double *scal, const double *c1, const double *c2, const double *v1, const double *v2, const double *rp);
int k_kc_combine(mgs_ctx *ctx, int n, const double *scal, const double *c1, const double *c2, double *x);
// *inv_out != NULL on entry: written in place; reg 1: A + (max|a_ij|/n)·1·1ᵀ; reg 2: A + Σ_f (max|a_ij|/n_f)·z_f·z_fᵀ for the fields of lab (device, n entries) with fcount rows each
int k_dense_inverse(mgs_ctx *ctx, const mgs_csr *A, double **inv_out, int reg = 0, const signed char *lab = nullptr, const double *fcount = nullptr);
// field-wise constant null space on a hierarchy: coarse labels from the aggregation (an aggregate takes its first member's label), checked in the same launch.
// *bad_dev (the caller sets it to ~0): min over (row << 1 | kind), kind 0 = the row's label differs from its aggregate's first member's, 1 = a labelled row outside every aggregate
int k_coarse_labels(mgs_ctx *ctx, const mgs_xfer *T, const signed char *lab, signed char *clab, unsigned long long *bad_dev);
int k_label_indicator(mgs_ctx *ctx, int n, const signed char *lab, int f, double *out);   // out_i = 1.0 where lab_i == f, else 0.0
// constant null space (MGS_NULLSPACE_CONSTANT): v ← v − mean(v), two launches, the mean stays on the device; _nrm2: out_host2[0] = ‖v − mean‖² from the
// shift pass; k_const_dev_nrm2: the same norm of a vector that is only read (‖Πb‖ of the caller's right-hand side)
int k_project_const(mgs_ctx *ctx, int64_t n, double *v);
int k_project_const_nrm2(mgs_ctx *ctx, int64_t n, double *v, double *out_host2);
int k_const_dev_nrm2(mgs_ctx *ctx, int64_t n, const double *v, double *out_host2);
int k_project_const_nrm2_fold(mgs_ctx *ctx, int64_t n, double *v);         // ... the norm² stays in red_dev[MGS_DOT_BLOCKS]: enqueued only
int k_const_dev_nrm2_fold(mgs_ctx *ctx, int64_t n, const double *v);
int k_project_const_mean(mgs_ctx *ctx, double *mean_host);   // the mean the last projection subtracted (synchronises)
// field-wise constant null space (MGS_NULLSPACE_FIELDS): v_i ← v_i − m[label_i] for label_i ≥ 0, m_f = (Σ_{label_i = f} v_i)/n_f left in F->means.  store = false:
// v is only read (‖Πb‖).  nrm: ‖Πv‖² over all rows is folded into red_dev[MGS_DOT_BLOCKS] and, with out_host2, fetched (out_host2[1] = 0).  Enqueue-only without out_host2.
int k_project_fields(mgs_ctx *ctx, const mgs_nsfields *F, int64_t n, double *v, bool store, bool nrm, double *out_host2);
// the ONE dispatch on a matrix's null-space record (kind 1: k_project_const*, kind 2: k_project_fields; the matrix must carry one of them)
int k_ns_project(const mgs_csr *A, int64_t n, double *v);
int k_ns_project_nrm2(const mgs_csr *A, int64_t n, double *v, double *out_host2);       // out_host2 = NULL: the norm² stays on the device
int k_ns_dev_nrm2(const mgs_csr *A, int64_t n, const double *v, double *out_host2);      // v only read; out_host2 = NULL: the norm² stays on the device
// (ingest.hip) labels in device memory → checked int8 copy + rows per field; *bad_row >= 0: the lowest row whose label lies outside [−1, nfields), *bad_val its value
int k_labels_from_device(mgs_ctx *ctx, int64_t rows, const void *labels_dev, int index_bits, int nfields, signed char **lab_out, int64_t *counts, int64_t *bad_row, long long *bad_val);
int k_abs_inplace(mgs_ctx *ctx, int64_t n, double *v);
int k_absmax_dev(mgs_ctx *ctx, int64_t n, const double *v, unsigned long long *amax_bits_dev);
int k_poisson3d(mgs_ctx *ctx, int N, int plane_lo, int plane_hi, int local_cols, mgs_csr **out);
int k_poisson2d(mgs_ctx *ctx, int n, mgs_csr **out);
int k_gather(mgs_ctx *ctx, const double *x, const int *idx, int64_t n, double *out);
int k_xfer_from_csr(const mgs_csr *P, mgs_xfer **out);
int k_transpose(const mgs_csr *A, mgs_csr **out);
// (setup_agmg.hip)
int k_exclusive_scan_i32(mgs_ctx *ctx, const int *in, int *out, int64_t n, int64_t *total_host);
int k_galerkin_agg(const mgs_csr *A, const mgs_xfer *T, mgs_csr **out);
int k_build_ap(const mgs_csr *A, const mgs_xfer *T, const int *cmap_ext, int ncols, mgs_csr **out);   // cmap_ext = NULL: square level, T->agg
// values of C = PᵀAP (or A·P with cptr == NULL) for C's existing pattern, one launch, no host synchronisation (mgs_hier_refresh)
int k_galerkin_numeric(const mgs_csr *A, int nc, const int *cptr, const int *members, const int *colmap, mgs_csr *C, int *miss_dev);
int k_galerkin_agg_ext(const mgs_csr *A, const mgs_xfer *T, const int *halo_map_dev, int n_halo_c, mgs_csr **out);
int k_xfer_from_agg_host(mgs_ctx *ctx, int n_fine, int n_coarse, const int *agg_host, mgs_xfer **out);
int k_galerkin_general(const mgs_csr *A, const mgs_xfer *T, mgs_csr **out);
int k_pairwise_aggregate(const mgs_csr *A, double ktg, int npass, double tou, mgs_xfer **T_out, mgs_csr **Ac_out, const int *zone_dev = nullptr);
// (ingest.hip) matrices from device memory: checked CSR copy, COO assembly, re-assembly of the values through the kept map
int k_csr_from_device(mgs_ctx *ctx, int rows, int cols, int64_t nnz, const void *rowptr_dev, const void *col_dev, int index_bits, const void *val_dev, mgs_csr **out);
int k_csr_from_coo_device(mgs_ctx *ctx, int rows, int cols, int64_t ntrip, const void *row_dev, const void *col_dev, int index_bits, const void *val_dev, int keep_map,
                          mgs_csr **out);
int k_csr_update_values_coo(mgs_csr *A, const void *val_dev);
// (spgemm.hip) C = A·B on the device, its values again for an unchanged pattern, and the general Galerkin product through them
int k_spgemm(const mgs_csr *A, const mgs_csr *B, mgs_csr **out);
int k_spgemm_numeric(const mgs_csr *A, const mgs_csr *B, mgs_csr *C, int64_t *misses);
int k_spgemm_info(const mgs_csr *C, int64_t out[4]);
void mgs_free_spgemm(struct mgs_spgemm_plan *p);
// (csr_algebra.hip) C = α·A + β·B with the union pattern, its values again in place, diagonal scalings, the diagonal as a vector and back
int k_csr_add(double alpha, const mgs_csr *A, double beta, const mgs_csr *B, mgs_csr **out);
int k_csr_add_numeric(double alpha, const mgs_csr *A, double beta, const mgs_csr *B, mgs_csr *C, int64_t *misses);
int k_csr_add_info(const mgs_csr *C, int64_t out[4]);
int k_csr_scale(mgs_csr *A, const mgs_vec *dl, const mgs_vec *dr);
int k_csr_diag(const mgs_csr *A, mgs_vec *d);
int k_csr_from_diag(mgs_ctx *ctx, const mgs_vec *d, mgs_csr **out);
void mgs_free_add(struct mgs_add_plan *p);
// (extract.hip) S = A(rows, cols) from index lists in device memory, its values again through the kept map, gather / scatter of a vector by an index list
int k_csr_extract(const mgs_csr *A, const void *rows_dev, int64_t nr, const void *cols_dev, int64_t nc, int index_bits, int keep_map, mgs_csr **out);
int k_csr_extract_numeric(const mgs_csr *A, mgs_csr *S);
int k_csr_extract_info(const mgs_csr *S, int64_t out[4]);
int k_vec_gather(const mgs_vec *x, const void *idx_dev, int64_t n, int index_bits, mgs_vec *y, int64_t *bad);
int k_vec_scatter(const mgs_vec *y, const void *idx_dev, int64_t n, int index_bits, mgs_vec *x, int64_t *bad);
void mgs_free_extract(struct mgs_extract_plan *p);
// (reorder.hip) C[i, j] = A[rperm[i], cperm[j]] from permutations in device memory, its values again through the kept map; C assembled from a grid of blocks, its values again
int k_csr_permute(const mgs_csr *A, const void *rperm_dev, const void *cperm_dev, int index_bits, int keep_map, mgs_csr **out);
int k_csr_permute_numeric(const mgs_csr *A, mgs_csr *C);
int k_csr_permute_info(const mgs_csr *C, int64_t out[4]);
int k_csr_bmat(mgs_ctx *ctx, int br, int bc, const mgs_csr *const *blocks, const int *row_sizes, const int *col_sizes, mgs_csr **out);
int k_csr_bmat_numeric(mgs_csr *C, const mgs_csr *const *blocks);
int k_csr_transpose_numeric(const mgs_csr *A, mgs_csr *At, int64_t *misses);
int k_csr_bmat_info(const mgs_csr *C, int64_t out[4]);
void mgs_free_reorder(struct mgs_reorder_plan *p);

// helpers (mgs_api.hip)
int mgs_csr_alloc(mgs_ctx *ctx, int rows, int cols, int64_t nnz, mgs_csr **out);
void mgs_drop_graph(mgs_hier *h);        // the cached cycle graphs (whatever they recorded has changed)
bool mgs_hier_sharded(const mgs_hier *h);   // row-sharded: halo callbacks, native plans or tail, a replaced coarse solve, or a level with halo columns
int mgs_level_in_range(const mgs_hier *h, int level, const char *who);
int mgs_prepare_fused(mgs_hier *h);      // (hier_operands.hip, as the three below) operands, work vectors and codes a hierarchy's cycle needs, built outside any stream capture
bool mgs_level_runs_f32(const mgs_hier *h, int l);
void mgs_operands_mark(mgs_level &L, unsigned bits); void mgs_operands_free(mgs_level &L);      // mark: these operands and everything derived from them are out of step
int mgs_operands_fill(mgs_hier *h, int l, unsigned want);   // refills, in place, those of `want` that exist and are dirty
// (cycle.hip) halo slots dst of a level-l vector (or payload buffer) from the owners' src, complete on the stream, through the hierarchy's ONE transport rule
int mgs_halo_exchange(mgs_hier *h, int l, const double *src, double *dst, bool fused_pass = false);
// (krylov.hip) the context's pool of work vectors for the other translation units: a vector of n entries, written before
// it is read by whoever takes it; mgs_ws_put(NULL) does nothing — and the Krylov solvers' null-space rule
int mgs_krylov_nullspace(const mgs_csr *A, const mgs_hier *h, const char *who, bool *ns_out, bool serves_fields = false);
int mgs_ws_get(mgs_ctx *ctx, int64_t n, int64_t owned, mgs_vec **out);
void mgs_ws_put(mgs_ctx *ctx, mgs_vec *v);
// What the host-driven solvers share (krylov.hip, minres.hip).  Work vectors are taken from the pool in the order the solver asks and go back when the solve ends, first-taken-first
// or (reverse) last-taken-first: the next solve must find the same vectors in the same roles (graph slots are keyed by their addresses).
struct krylov_frame {
  mgs_ctx *ctx; mgs_hier *h; int n; bool ns, reverse;      // n: owned rows; ns: a null space is declared (constant, or field-wise on nsA)
  std::vector<mgs_vec *> taken;
  const mgs_csr *nsA = nullptr;                            // the matrix whose null-space record the projections dispatch on (NULL: the constant kind)
  ~krylov_frame() {
    hipStreamSynchronize(ctx->stream);
    if (reverse) std::reverse(taken.begin(), taken.end());
    for (mgs_vec *v : taken) mgs_ws_put(ctx, v);
  }
  int take(mgs_vec **q, int64_t len) { MGS_TRY(mgs_ws_get(ctx, len, n, q)); taken.push_back(*q); return MGS_OK; }
  mgs_vec view(const mgs_vec *full) const { mgs_vec v; v.ctx = ctx; v.n = n; v.d = full->d; v.owns = false; return v; }      // the owned part, so BLAS-1 sizes agree
  // halo of the level-0 vector w through the hierarchy's transport (no hierarchy: nothing to refresh); a failed exchange has always been MGS_ERR_STATE here
  int halo(mgs_vec *w) const { return !h || mgs_halo_exchange(h, 0, w->d, w->d + n) == MGS_OK ? MGS_OK : MGS_ERR_STATE; }
  // ‖b‖ (bicg.cpp:80), of a zero vector 1 (:85-86); constant null space: ‖Πb‖, b only read
  int norm_b(const mgs_vec &bv, double *normb) const {
    double d2[2];
    if (ns && nsA) { MGS_TRY(k_ns_dev_nrm2(nsA, n, bv.d, d2)); *normb = std::sqrt(d2[0]); }
    else if (ns) { MGS_TRY(k_const_dev_nrm2(ctx, n, bv.d, d2)); *normb = std::sqrt(d2[0]); }
    else MGS_TRY(mgs_nrm2(&bv, normb));
    if (*normb == 0.0) *normb = 1;
    return MGS_OK;
  }
};
// What the solvers that serve no row shard check first (the Krylov plans through krylov_plan.hpp, mgs_eig_lobpcg): a square matrix on a context that does not
// sum over ranks, and a finalized hierarchy of its size on the same context without halo columns, exchange callbacks, native plans or a tail.
static inline int mgs_check_unsharded(const mgs_csr *A, const mgs_hier *h, const char *who, const char *served_by) {
  mgs_ctx *c = A->ctx;
  MGS_CHECK(c, A->rows == A->cols && !c->ncomm && !c->allreduce, MGS_ERR_INVALID, "%s: the matrix is %d x %d%s (%s)", who, A->rows, A->cols,
            A->cols > A->rows ? ", halo columns: a row shard" : (A->rows == A->cols ? ", on a context that sums over ranks" : ", not square"), served_by);
  MGS_CHECK(c, A->rows > 0, MGS_ERR_INVALID, "%s: the matrix has no rows", who);
  if (h) {
    bool shard = h->halo || h->halo_begin || h->halo_end || h->halo_fused || h->coarse || h->native || h->ntail;
    for (const mgs_level &L : h->lev) shard = shard || L.nx || (L.A && L.A->cols > L.A->rows);
    MGS_CHECK(c, !shard, MGS_ERR_INVALID, "%s: the hierarchy has halo columns, exchange callbacks, native plans or a tail (%s)", who, served_by);
    MGS_CHECK(c, h->ctx == c && !h->lev.empty() && h->lev[0].n == A->rows, MGS_ERR_INVALID, "%s: the hierarchy's fine level has %d rows, A has %d", who,
              h->lev.empty() ? 0 : h->lev[0].n, A->rows);
    MGS_CHECK(c, h->finalized, MGS_ERR_STATE, "%s: call mgs_hier_finalize first", who);
  }
  return MGS_OK;
}
template <class T>
static inline int mgs_dev_alloc(mgs_ctx *ctx, T **p, size_t count) {
  *p = nullptr;
  hipError_t e = mgs_hip_malloc((void **)p, sizeof(T) * (count ? count : 1));
  if (e != hipSuccess) return mgs_fail(ctx, MGS_ERR_ALLOC, "hipMalloc(%zu bytes): %s", sizeof(T) * count, hipGetErrorString(e));
  return MGS_OK;
}
static inline int mgs_grid(int64_t work, int block) { return (int)((work + block - 1) / block); }
