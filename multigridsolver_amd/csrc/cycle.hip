// cycle.hip — the cycle's host side: the halo transport layer, the operands and launches of the fused passes, one function per cycle
// form, mgs_vcycle with its graph cache, and the single-pass entry points of the tests.  No kernel lives here; every numeric step is a
// launch on the context's stream.
#include "mgs_internal.hpp"

#include <algorithm>

// Halo exchange of level l through the native transport, on the context's stream: dst[slot] = src[row the owner of that slot was
// asked for] — src is a vector of the level (its owned entries), dst the halo slots (behind the owned entries of the same vector,
// or a payload buffer).  Where every peer's rows are a few contiguous ranges (plane shards) and the receive segmentation has been
// installed (mgs_hier_set_native_recv_segments), the ranges are sent straight from src: no pack kernel.
static int native_exchange(mgs_hier *h, int l, const double *src, double *dst) {
  mgs_native_plan *P = h->lev[l].nx;
  mgs_ctx *ctx = h->ctx;
  if (!P->ns && !P->nr) return MGS_OK;
  const int world = (int)P->scnt.size();
  std::vector<mgs_xfer_op> ops;
  const bool seg = P->use_seg && P->seg_ok;
  if (P->ns && !seg) MGS_TRY(k_gather(ctx, src, P->send_idx, P->ns, P->sendbuf));
  size_t so = 0, ro = 0;
  for (int p = 0; p < world; ++p) {
    if (seg) { for (size_t q = 0; q < P->sseg_len[p].size(); ++q) ops.push_back({src + P->sseg_start[p][q], nullptr, (size_t)P->sseg_len[p][q], p}); }
    else { size_t q0 = so; for (int len : P->pseg_len[p]) { ops.push_back({P->sendbuf + q0, nullptr, (size_t)len, p}); q0 += (size_t)len; } }      // packed: one message per peer
    if (P->use_seg) { size_t r = ro; for (int len : P->rseg_len[p]) { ops.push_back({nullptr, dst + r, (size_t)len, p}); r += (size_t)len; } }
    else { size_t r = ro; for (int len : P->prseg_len[p]) { ops.push_back({nullptr, dst + r, (size_t)len, p}); r += (size_t)len; } }
    so += (size_t)P->scnt[p]; ro += (size_t)P->rcnt[p];
  }
  return mgs_comm_exchange_ops(P->comm, ops.data(), (int)ops.size());
}

// Overlapped exchange inside a captured cycle (option native_overlap).  The RCCL calls stay on the stream the capture began on: RCCL forks to
// streams of its own inside a capture, and this HIP runtime only survives that on the ORIGIN stream (a forked stream that
// forks again ends in a cycle of the capture bookkeeping — hipStreamEndCapture recursed until the stack ran out).  What
// moves to the context's second stream is the kernel over the interior row blocks, which needs no halo value:
//   origin:  producer → [fork] → pack → RCCL group → [join] → boundary row blocks → …
//   second:             interior row blocks ──────────┘
// Under capture the two cross-stream dependencies are edges of the graph.
static int fork_side(mgs_hier *h, hipEvent_t *join) {
  mgs_ctx *ctx = h->ctx;
  while (h->fork_events.size() < h->fork_used + 2) {
    hipEvent_t e; MGS_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming)); h->fork_events.push_back(e);
  }
  hipEvent_t fork = h->fork_events[h->fork_used++]; *join = h->fork_events[h->fork_used++];
  MGS_HIP(ctx, hipEventRecord(fork, ctx->stream));
  MGS_HIP(ctx, hipStreamWaitEvent(ctx->comm_stream, fork, 0));
  return MGS_OK;
}
// runs `interior` (kernel launches on ctx->stream) on the second stream, then the exchange on the origin, then joins
template <class F>
static int overlapped_exchange(mgs_hier *h, int l, const double *src, double *out, F interior) {
  mgs_ctx *ctx = h->ctx;
  hipEvent_t join;
  MGS_TRY(fork_side(h, &join));
  hipStream_t origin = ctx->stream;
  ctx->stream = ctx->comm_stream;
  int rc = interior();
  ctx->stream = origin;
  MGS_TRY(rc);
  MGS_HIP(ctx, hipEventRecord(join, ctx->comm_stream));
  MGS_TRY(native_exchange(h, l, src, out));
  MGS_HIP(ctx, hipStreamWaitEvent(ctx->stream, join, 0));
  return MGS_OK;
}

// ------------------------------------------------------------------ halo transport: the ONE place that refreshes halo values
// dst (the halo slots of a level-l vector, or a payload buffer) receives the owners' src.  One precedence: the level's native plan, the
// plain callback, the split callbacks, the fused callback.  The first two callbacks work in place, so they serve dst == src + rows only;
// the fused callback serves any dst.  Two things a caller states because the forms of the cycle have always differed in them:
//   fused_pass  an exchange of the fused passes asks the fused callback (installed for them) before the in-place ones, and only such an
//               exchange runs beside its interior row blocks on the second stream of a captured native cycle (option native_overlap);
//   two_phase   the caller has interior row blocks to launch between begin and end: the split callbacks then go before the plain one.
// Installed callbacks are called on levels without halo columns too (the host side knows that it has nothing to send).
enum { HALO_NONE = 0, HALO_NATIVE, HALO_PLAIN, HALO_SPLIT, HALO_FUSED };
static int halo_transport(const mgs_hier *h, int l, const double *src, const double *dst, bool fused_pass, bool two_phase) {
  if (h->lev[l].nx) return HALO_NATIVE;
  const bool in_place = dst == src + h->lev[l].A->rows && !(fused_pass && h->halo_fused);
  if (in_place && h->halo_begin && (two_phase || !h->halo)) return HALO_SPLIT;
  if (in_place && h->halo) return HALO_PLAIN;
  return h->halo_fused ? HALO_FUSED : HALO_NONE;
}
// phase 0 starts the exchange, phase 1 completes it (the plain callback does both in phase 0); no transport: an error where there are halo columns
static int halo_phase(mgs_hier *h, int l, int via, const double *src, double *dst, int phase) {
  double *x = const_cast<double *>(src);
  int rc = 0;
  if (via == HALO_PLAIN) rc = phase ? 0 : h->halo(h->halo_user, l, x);
  else if (via == HALO_SPLIT) rc = phase ? h->halo_end(h->halo_user, l, x) : h->halo_begin(h->halo_user, l, x);
  else if (via == HALO_FUSED) rc = h->halo_fused(h->halo_user, l, 2, src, nullptr, dst, phase);
  else if (h->lev[l].A->cols > h->lev[l].A->rows) return mgs_fail(h->ctx, MGS_ERR_STATE, "level %d is a row shard but no halo exchange is installed", l);
  return rc ? mgs_fail(h->ctx, MGS_ERR_STATE, "halo exchange (%s) failed at level %d (%d)", phase ? "end" : "begin", l, rc) : MGS_OK;
}
// complete on the stream when it returns, nothing launched in between
int mgs_halo_exchange(mgs_hier *h, int l, const double *src, double *dst, bool fused_pass) {
  const int via = halo_transport(h, l, src, dst, fused_pass, false);
  if (via == HALO_NATIVE) return native_exchange(h, l, src, dst);
  MGS_TRY(halo_phase(h, l, via, src, dst, 0));
  return halo_phase(h, l, via, src, dst, 1);
}
// Below opt_split_min_rows owned rows a level's kernel is too short to hide an exchange behind its interior row blocks:
// exchange first, then one launch (one launch less per pass).
static bool halo_split(const mgs_hier *h, const mgs_csr *A) { return A->halo_split_ok && A->rows >= h->ctx->opt_split_min_rows; }
// The overlap form: launch(blk_lo, blk_hi, gap_at, gap_len) starts a kernel on a range of A's row blocks whose halo values come from level
// l's exchange src → dst (src NULL: nothing to exchange).  Where A's halo readers are its leading and trailing row blocks and the transport
// has two phases, the interior blocks run while the values are in flight and the boundary blocks follow in one launch; else one launch
// behind the exchange.
template <class F>
static int mgs_halo_exchange_around(mgs_hier *h, int l, const mgs_csr *A, const double *src, double *dst, bool fused_pass, F launch) {
  const int nb = mgs_row_blocks(A), lo = A->halo_lo_blocks, hi = nb - A->halo_hi_blocks;
  const bool split = src && halo_split(h, A);
  const int via = src ? halo_transport(h, l, src, dst, fused_pass, split) : HALO_NONE;
  const bool phases = via == HALO_NATIVE ? fused_pass && h->capturing && h->ctx->comm_stream : via == HALO_SPLIT || via == HALO_FUSED;
  if (!split || !phases) {
    if (src) MGS_TRY(mgs_halo_exchange(h, l, src, dst, fused_pass));
    return launch(0, nb, 0x7fffffff, 0);
  }
  if (via == HALO_NATIVE) MGS_TRY(overlapped_exchange(h, l, src, dst, [&]() { return launch(lo, hi, 0x7fffffff, 0); }));
  else {
    MGS_TRY(halo_phase(h, l, via, src, dst, 0));
    MGS_TRY(launch(lo, hi, 0x7fffffff, 0));
    MGS_TRY(halo_phase(h, l, via, src, dst, 1));
  }
  return launch(0, lo + nb - hi, lo, hi - lo);   // leading + trailing boundary blocks, one launch
}
// one SpMV-shaped kernel on level l with x's halo refreshed first
static int sharded_op(mgs_hier *h, int l, const mgs_csr *A, int op, double *x, const double *b, const double *dinv, double omega, double *out) {
  return mgs_halo_exchange_around(h, l, A, x, x + A->rows, false, [&](int b0, int b1, int ga, int gl) {
    return mgs_launch_csr_op_range(A, op, x, b, dinv, omega, out, b0, b1, ga, gl); });
}

// ------------------------------------------------------------------ the fused passes: operands, arms, launches
// The operands of level l's two fused passes under the options as they stand — the ONE place that chooses them (cycle_fused and
// mgs_hier_post_pass both ask here).  Setup-time operands: Â = A·diag(wd) makes the pre pass the plain residual kernel with x = b (one
// gather per entry); A·P (or col_agg = the coarse column of every entry) lets the post pass gather e_c directly.  On a shard the halo
// columns of Â read the payload buffer (the pattern-coded kernel knows that split); those of A·P read e_c's own halo.
struct fused_operands {
  mgs_csr Ahat, Amap;      // views: the pre pass's operand; the post pass's (meaningful only where `operands` holds)
  bool f32 = false;        // both passes read the FP32 copies of the stored values (float forms of the same kernels), or neither does
  bool operands = false;   // the passes run on the setup-time operands (false: the gather forms on A itself)
  int post_form = 0;       // post pass on: 0 A with the column-to-aggregate map (gather form), 1 aggregate-mapped A, 2 merged A·P
  bool grouped = false;    // the level qualifies for the grouped pre pass, whose post pass is the t-form (a row shard adds conditions of its own)
  const mgs_groups *sweep = nullptr;   // option group_sweep: the grouped level's post pass sweeps these row-block groups
};
static void level_fused_operands(const mgs_hier *h, int l, bool halo, fused_operands &o) {
  const mgs_ctx *ctx = h->ctx;
  const mgs_level &L = h->lev[l];
  mgs_csr &Ahat = o.Ahat, &Amap = o.Amap;
  // Â's code: its own when the tuples carry values or halo tags, A's index-only code otherwise
  Ahat = *L.A; Ahat.val = L.val_wd; Ahat.owns = false;
  Ahat.code = halo ? L.code_pre : ((L.A->code && L.A->code->vtab) || L.code_hat ? L.code_hat : L.A->code);
  Amap = *L.A; Amap.val = L.A->val; Amap.col = L.col_agg; Amap.code = L.code_agg; Amap.owns = false;
  if (ctx->opt_diag_from_values && L.dpos) { Amap.dpos = L.dpos; Amap.dpos_omega = h->omega; }   // t-form post pass: ω/a_ii from the streamed values
  const bool merged = ctx->opt_merge_ap && L.AP;
  if (merged) { Amap = *L.AP; Amap.code = L.code_ap; Amap.owns = false; }      // A·P, merged: fewer entries, wd read per row
  o.f32 = mgs_level_runs_f32(h, l) && !halo;
  if (o.f32) { Ahat.val32 = L.val_wd32; Amap.val32 = L.ap_val32; }
  // option pack7: packed copies of the two operands' FP64 values (unsharded FP64 levels; the launchers check that a copy serves their launch)
  if (!halo) { Ahat.pk7 = L.pk_hat; if (merged) Amap.pk7 = L.pk_ap; }
  o.operands = ctx->opt_fuse_operands && L.val_wd && (L.col_agg || merged) && (!halo || mgs_rowcode_usable(&Ahat, true));
  o.post_form = !o.operands ? 0 : (merged ? 2 : 1);
  o.grouped = ctx->opt_fuse_restrict && o.operands && L.grp && !(Ahat.code && Ahat.code->vtab);
  o.sweep = (o.grouped && (ctx->opt_group_sweep & 1)) ? L.grp : nullptr;
}
// Whether level l (not the coarsest) runs the fused form — aggregation P, V(1,1), multiplicative — from x = 0 under the options as they stand: the
// ONE place that decides it (cycle_level, mgs_hier_pre_pass_info and mgs_hier_post_pass all ask here).  Row shards also need the transport of the
// two payloads; a shard level without halo columns (single rank, isolated shard) behaves like a square level.
static bool level_fuses(const mgs_hier *h, int l) {
  const mgs_level &L = h->lev[l], &C = h->lev[l + 1];
  bool transport_ok = true;
  if (L.A->cols > L.A->rows) transport_ok = L.hbuf && L.halo_dinv && L.cmap_ext && (L.nx || h->halo_fused);
  if (C.A->cols > C.A->rows) transport_ok = transport_ok && (C.nx || h->halo_fused);
  return h->ctx->opt_fuse && !h->additive && h->nu1 == 1 && h->nu2 == 1 && L.wd && mgs_operand_in_step(L, OPD_WD) && L.T->aggregation && L.A->lds_cap > 0 && transport_ok;
}

// option pre_nodiag: the grouped pre pass of this level runs on val_nd (an eligible unsharded FP64 level whose compact operand is in step with val_wd)
static bool level_pre_nodiag(const mgs_hier *h, const mgs_level &L, bool halo, bool f32) {
  return h->ctx->opt_pre_nodiag && mgs_level_nd_ready(L) && !halo && !f32 && !h->ctx->opt_valcode;
}
// The arm of level l's fused pre pass under the options as they stand — the ONE place that chooses it (cycle_fused and
// mgs_hier_pre_pass_info both ask here).  shard_split: a row shard that launches its interior row blocks beside the halo exchange, uncaptured and
// without the native transport (the grouped form exchanges first and launches once, so it does not serve that case).
enum { PRE_ARM_GATHER = 0, PRE_ARM_RESIDUAL = 1, PRE_ARM_AGG = 2, PRE_ARM_GROUPED = 3 };
static int level_pre_arm(const mgs_hier *h, int l, const fused_operands &o, bool shard_split) {
  const mgs_ctx *ctx = h->ctx;
  const mgs_level &L = h->lev[l];
  if (o.grouped && !shard_split) return PRE_ARM_GROUPED;
  // small level (a dispatch costs what it costs, whatever it does): pre pass and restriction in one aggregate-parallel kernel
  if (ctx->opt_fuse_operands && L.val_wd && L.A->rows <= ctx->opt_aggpre_max_rows && L.A->max_row_len <= 64) return PRE_ARM_AGG;
  return o.operands ? PRE_ARM_RESIDUAL : PRE_ARM_GATHER;
}
// The launches of that arm where they need no exchange between them: every arm of an unsharded level (hv NULL), and the two one-kernel arms of
// a row shard once its halo values lie in hv.  Grouped: t_out = b + r, r_out the residuals of the stray waves' rows, rc_out = Pᵀr.
// The other arms: r_out = r on every row, rc_out = Pᵀr; t_out is not touched.
static int launch_pre_arm(const mgs_hier *h, int l, const fused_operands &o, int arm, const double *b, double *t_out, double *r_out, double *rc_out,
                          const double *hv) {
  mgs_ctx *ctx = h->ctx;
  const mgs_level &L = h->lev[l];
  if (arm == PRE_ARM_GROUPED) {
    // option pre_nodiag: an eligible FP64 level streams Â's diagonal as a byte per row (the same bits as from val_wd)
    const bool nodiag = level_pre_nodiag(h, L, hv != nullptr, o.f32);
    return mgs_launch_group_pre(&o.Ahat, L.grp, L.T, b, b, t_out, r_out, rc_out, hv, L.A->rows, nodiag ? L.val_nd : nullptr, L.nd_code, L.nd_omega, o.Ahat.pk7);
  }
  if (arm == PRE_ARM_AGG) return k_agg_pre(L.A, L.val_wd, b, hv, L.T, r_out, rc_out, o.f32 ? L.val_wd32 : nullptr);
  if (hv) return mgs_fail(ctx, MGS_ERR_STATE, "pre pass of level %d: a row shard launches this arm around its halo exchange", l);
  // r = b − A·x1 with x1 = wd∘b (never stored: the POST pass recomputes it from b)
  if (arm == PRE_ARM_RESIDUAL) MGS_TRY(mgs_launch_csr_op(&o.Ahat, MGS_OP_RESIDUAL, b, b, nullptr, 0.0, r_out));
  else MGS_TRY(mgs_launch_fused(L.A, FUSE_PRE, L.wd->d, b, nullptr, nullptr, nullptr, r_out, nullptr));
  return k_restrict_agg(ctx, L.T->n_coarse, L.T->cptr, L.T->members, r_out, rc_out);
}
// The post pass x = x1 + Pe + wd∘(r − A·Pe) on a range of row blocks — the ONE place that launches it: on the setup-time operand (A·P / aggregate-mapped
// A: the pattern-coded kernel where the code serves it, the gather kernel otherwise), or the gather form on A with the coarse column of every local
// column.  group_sweep: the launch follows the grouped pre pass (whole levels only), so option group_sweep applies.
static int launch_post_pass(const mgs_hier *h, int l, fused_operands &o, bool group_sweep, const double *bvec, const double *xin, const double *ec, double *x,
                            int b0, int b1, int ga, int gl) {
  const mgs_level &L = h->lev[l];
  o.Amap.sweep = group_sweep ? o.sweep : nullptr;
  if (o.operands) return mgs_launch_fused_range(&o.Amap, FUSE_POST_MAPPED, L.wd->d, bvec, xin, L.T->agg, ec, x, nullptr, nullptr, b0, b1, ga, gl);
  return mgs_launch_fused_range(L.A, FUSE_POST, L.wd->d, bvec, xin, L.cmap_ext ? L.cmap_ext : L.T->agg, ec, x, nullptr, nullptr, b0, b1, ga, gl);
}

// what mgs_hier_pre_pass_info and mgs_hier_post_pass ask of their level: a finalized hierarchy whose unsharded, index-coded level runs the fused form
static int fused_pass_level(mgs_hier *h, int level, const char *who) {
  mgs_ctx *ctx = h->ctx;
  MGS_CHECK(ctx, h->finalized, MGS_ERR_STATE, "%s: call mgs_hier_finalize first", who);
  MGS_CHECK(ctx, level >= 0 && level + 1 < (int)h->lev.size(), MGS_ERR_INVALID, "%s: level %d has no coarser level", who, level);
  MGS_TRY(mgs_prepare_fused(h));
  const mgs_level &L = h->lev[level], &C = h->lev[level + 1];
  MGS_CHECK(ctx, L.T && L.T->aggregation, MGS_ERR_STATE, "%s: level %d has a general P (the fused passes serve aggregation transfers only)", who, level);
  const bool plain = L.A->cols == L.A->rows && C.A->cols == C.A->rows && !L.nx && !L.cmap_ext && !ctx->opt_valcode && !(L.A->code && L.A->code->vtab) && !L.code_hat &&
                     !(L.code_agg && L.code_agg->vtab) && !(L.code_ap && L.code_ap->vtab);
  MGS_CHECK(ctx, plain, MGS_ERR_STATE, "%s: level %d is sharded or value-coded", who, level);
  MGS_CHECK(ctx, level_fuses(h, level), MGS_ERR_STATE, "%s: level %d does not run the fused passes (option fuse, V(1,1), multiplicative)", who, level);
  return MGS_OK;
}

// ------------------------------------------------------------------ the cycle
// The cycle body: pure kernel launches on ctx->stream (capturable into a hipGraph when no
// halo callback is installed).
//   ν1 × { x ← x + ωD⁻¹(b − Ax) };  r = b − Ax;  r_c = Pᵀr (bicg.cpp:48);  e_c = cycle(l+1, r_c) from 0
//   (coarsest: A_c⁻¹, bicg.cpp:35-36,48);  x ← x + P e_c (bicg.cpp:48);  ν2 × { x ← x + ωD⁻¹(b − Ax) }
// From x = 0 the first pre-sweep is x = (ωD⁻¹)b, the residual is b and x + P e_c is P e_c —
// bit-identical shortcuts that skip one SpMV-sized pass each.
static int cycle_level(mgs_hier *h, int l, const double *b, double *x, bool zero_guess);

// Approximate solve of the level-l problem A_l x = rhs from x = 0 for the level above.  V-cycle: one
// recursive cycle.  K-cycle (levels 1..kcycle_levels): two GCR steps preconditioned by that cycle
// (docs/AGMG_For_Convection_Diffusion.pdf §3.1; Fortran `nlvcyc`, src/CPU_Matlab/dagtwolev_mex.f90:59-61):
//   c1 = B rhs, v1 = A c1, r' = rhs − (α1/ρ1) v1;  c2 = B r', v2 = A c2, g = γ/ρ1;
//   x = (α1/ρ1) c1 + (α2/ρ2) (c2 − g c1),  ρ2 and α2 from the explicitly orthogonalised pair (c2 − g c1, v2 − g v1) — the paper's
//   ρ2 = β − γ²/ρ1 in exact arithmetic, without the difference of two nearly equal numbers.
static bool kcycle_here(const mgs_hier *h, int l) {
  const bool sharded = h->halo || h->halo_begin || h->native;
  // row shards: the five inner products are summed over the ranks — needs a reduction transport (native RCCL or the callback)
  return (l >= 1 ? l <= h->kcycle_levels : h->kcycle_entry) && l < (int)h->lev.size() - 1 && h->lev[l].kscal &&
         (!sharded || h->ctx->ncomm || h->ctx->allreduce);
}
// sum of `cnt` device scalars over the ranks of a row-sharded run (no-op on one GPU)
static int kc_allreduce(mgs_hier *h, double *dev, int cnt) {
  mgs_ctx *ctx = h->ctx;
  if (!(h->halo || h->halo_begin || h->native)) return MGS_OK;
  if (ctx->ncomm) return mgs_comm_allreduce_sum(ctx->ncomm, dev, (size_t)cnt);
  MGS_HIP(ctx, hipMemcpyAsync(ctx->red_host, dev, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, ctx->stream));
  MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->allreduce(ctx->allreduce_user, ctx->red_host, cnt)) return mgs_fail(ctx, MGS_ERR_STATE, "all-reduce callback failed");
  MGS_HIP(ctx, hipMemcpyAsync(dev, ctx->red_host, sizeof(double) * (size_t)cnt, hipMemcpyHostToDevice, ctx->stream));
  MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));     // red_host is reused by the next reduction
  return MGS_OK;
}
static int coarse_solve_inner(mgs_hier *h, int l, const double *rhs, double *x) {
  if (!kcycle_here(h, l)) return cycle_level(h, l, rhs, x, true);
  mgs_ctx *ctx = h->ctx;
  mgs_level &L = h->lev[l];
  const int n = L.n;
  double *sc = L.kscal;
  MGS_TRY(cycle_level(h, l, rhs, L.kc1->d, true));
  MGS_TRY(sharded_op(h, l, L.A, MGS_OP_SPMV, L.kc1->d, nullptr, nullptr, 0.0, L.kv1->d));      // halo of c1 refreshed on a row shard
  // GCR form (paper §3.1): inner products with v = A·c.  Energy form (option kcycle_energy, SPD operators; flexible-CG coefficients):
  // the same products with c as left factor — ρ1 = c1·Ac1, α1 = c1·rhs, γ = c2·Ac1; then, with the second direction orthogonalised
  // explicitly (c2' = c2 − (γ/ρ1)c1, v2' = v2 − (γ/ρ1)v1), ρ2 = d2'·v2' and α2 = d2'·r' (blas1.hip: kc_orth_dots_kernel).
  const bool energy = ctx->opt_kcycle_energy != 0;
  const double *d1 = energy ? L.kc1->d : L.kv1->d, *d2 = energy ? L.kc2->d : L.kv2->d;
  const double *two[2] = {L.kv1->d, rhs};
  MGS_TRY(k_mdot(ctx, n, 2, d1, two, sc + 0, nullptr));                      // ρ1, α1: d1 read once
  MGS_TRY(kc_allreduce(h, sc, 2));
  MGS_TRY(k_kc_update_r(ctx, n, sc, rhs, L.kv1->d, L.kr->d));
  MGS_TRY(cycle_level(h, l, L.kr->d, L.kc2->d, true));
  MGS_TRY(sharded_op(h, l, L.A, MGS_OP_SPMV, L.kc2->d, nullptr, nullptr, 0.0, L.kv2->d));
  MGS_TRY(k_dot_dev(ctx, n, d2, L.kv1->d, sc + 2));                          // γ
  MGS_TRY(kc_allreduce(h, sc + 2, 1));
  MGS_TRY(k_kc_orth_dots(ctx, n, energy, sc, L.kc1->d, L.kc2->d, L.kv1->d, L.kv2->d, L.kr->d));   // ρ2, α2
  MGS_TRY(kc_allreduce(h, sc + 3, 2));
  return k_kc_combine(ctx, n, sc, L.kc1->d, L.kc2->d, x);
}
// e_c for the level above; with an over-correction factor σ ≠ 1 (mgs_hier_set_correction_scale) it is scaled here, once, on the
// coarse vector (n_c entries), so every form of the level above — fused, grouped, unfused, K-cycle — sees σ·e_c
static int coarse_solve(mgs_hier *h, int l, const double *rhs, double *x) {
  if (l == 1 && h->coarse_launch && h->coarse_exec && rhs == h->lev[1].b->d && x == h->lev[1].x->d) {     // split launch (mgs_vcycle): everything below the fine level, one replay
    MGS_HIP(h->ctx, hipGraphLaunch(h->coarse_exec, h->ctx->stream));
    return MGS_OK;
  }
  MGS_TRY(coarse_solve_inner(h, l, rhs, x));
  if (h->corr_scale != 1.0) {
    // (the last sharded level's halo slots were filled from the replicated tail's solution together with the owned entries: scale them as well)
    const bool tail_halo = h->ntail && h->ntail->halo_global && l == (int)h->lev.size() - 1 && x == h->lev[l].x->d;
    MGS_TRY(k_axpby(h->ctx, tail_halo ? h->lev[l].n_ext : h->lev[l].n, h->corr_scale, x, 0.0, x));
  }
  return MGS_OK;
}

// replicated tail, native: all-gather the rhs, cycle, own slice back
static int cycle_native_tail(mgs_hier *h, mgs_level &L, const double *b, double *x) {
  mgs_ctx *ctx = h->ctx;
  mgs_native_tail *T = h->ntail;
  const double *tb = T->b->d;
  if (T->even) {        // equal shards: gather straight from b; the gathered buffer is already in the tail's row order (two dispatches less per cycle)
    MGS_TRY(mgs_comm_allgather(T->comm, b, T->all, (size_t)T->maxn));
    tb = T->all;
  } else {
    if (T->n_loc) MGS_HIP(ctx, hipMemcpyAsync(T->send, b, sizeof(double) * (size_t)T->n_loc, hipMemcpyDeviceToDevice, ctx->stream));
    MGS_TRY(mgs_comm_allgather(T->comm, T->send, T->all, (size_t)std::max(T->maxn, 1)));
    MGS_TRY(k_gather(ctx, T->all, T->gidx, T->n_t, T->b->d));
  }
  if (h->capturing) MGS_TRY(coarse_solve_inner(T->tail, 0, tb, T->x->d));   // part of the outer graph (mgs_prepare_fused ran before the capture); K iteration at the entry level if asked for
  else { mgs_vec bv; bv.ctx = ctx; bv.n = T->n_t; bv.d = const_cast<double *>(tb); bv.owns = false; MGS_TRY(mgs_vcycle(T->tail, &bv, T->x, 1)); }
  // own slice back; with the global rows of this level's halo slots known (mgs_hier_set_native_tail_halo) the same kernel fills the halo
  // slots from the replicated solution — the level above then needs no exchange for e_c
  if (T->halo_global && x == L.x->d) MGS_TRY(k_tail_scatter(ctx, T->x->d, T->my_off, T->n_loc, T->halo_global, T->n_halo_global, x));
  else if (T->n_loc) MGS_HIP(ctx, hipMemcpyAsync(x, T->x->d + T->my_off, sizeof(double) * (size_t)T->n_loc, hipMemcpyDeviceToDevice, ctx->stream));
  return MGS_OK;
}
// the coarsest level: native tail, coarse callback, smoothed (see mgs_hier_finalize), or the dense inverse
static int cycle_coarsest(mgs_hier *h, int l, const double *b, double *x) {
  mgs_ctx *ctx = h->ctx;
  mgs_level &L = h->lev[l];
  if (h->ntail) return cycle_native_tail(h, L, b, x);
  if (h->coarse) { int rc = h->coarse(h->coarse_user, b, x); return rc ? mgs_fail(ctx, MGS_ERR_STATE, "coarse solver callback failed (%d)", rc) : MGS_OK; }
  if (h->coarse_sweeps <= 0) return k_dense_gemv(ctx, h->nc, h->inv, b, x);
  double *cur = x, *alt = L.tmp->d;
  if (!(h->coarse_sweeps & 1)) std::swap(cur, alt);   // odd number of buffer flips ends in x
  MGS_TRY(k_jacobi_zero(ctx, L.n, h->omega, L.dinv->d, b, cur));
  for (int s = 1; s < h->coarse_sweeps; ++s) {
    MGS_TRY(mgs_halo_exchange(h, l, cur, cur + L.A->rows));
    MGS_TRY(mgs_launch_csr_op(L.A, MGS_OP_JACOBI, cur, b, L.dinv->d, h->omega, alt));
    std::swap(cur, alt);
  }
  if (cur != x) MGS_HIP(ctx, hipMemcpyAsync(x, cur, sizeof(double) * (size_t)L.n, hipMemcpyDeviceToDevice, ctx->stream));
  return MGS_OK;
}
// additive form of solve(), reference src/common/bicg.cpp:59 with M2 = ωD⁻¹, level by level (zero guess only):
//   x = P·cycle(l+1, Pᵀ b) + ωD⁻¹ b
static int cycle_additive(mgs_hier *h, int l, const double *b, double *x) {
  mgs_ctx *ctx = h->ctx;
  mgs_level &L = h->lev[l], &C = h->lev[l + 1];
  if (L.T->aggregation) MGS_TRY(k_restrict_agg(ctx, L.T->n_coarse, L.T->cptr, L.T->members, b, C.b->d));
  else MGS_TRY(mgs_launch_csr_op(L.T->Pt, MGS_OP_SPMV, b, nullptr, nullptr, 0.0, C.b->d));
  MGS_TRY(coarse_solve(h, l + 1, C.b->d, C.x->d));
  if (L.T->aggregation) MGS_TRY(k_prolong_agg(ctx, L.n, L.T->agg, C.x->d, x, 0));
  else MGS_TRY(mgs_launch_csr_op(L.T->P, MGS_OP_SPMV, C.x->d, nullptr, nullptr, 0.0, x));
  MGS_TRY(k_jacobi_zero(ctx, L.n, h->omega, L.dinv->d, b, L.tmp->d));
  return k_axpby(ctx, L.n, 1.0, L.tmp->d, 1.0, x);
}
// Fused form (level_fuses): two matrix passes, no separate (ωD⁻¹)b / prolong-add kernels — exchange, pre arm, coarse solve, post pass.
// Row shards: the only data of other ranks the two passes need are plain vector values — the peers' raw right-hand side of the
// rows this shard sees as halo (pre pass: Â's halo columns carry the owners' ωD⁻¹, fetched once at setup) and the coarse level's
// own halo of e_c (post pass: the halo columns of A·P are merged by REMOTE aggregate, i.e. they are the coarse level's halo
// columns).  Both are ordinary halo exchanges — contiguous ranges on plane shards, sent without a pack kernel.  The boundary row blocks
// of both passes are those of L.A that read halo columns (A·P has them in the same rows).
static int cycle_fused(mgs_hier *h, int l, const double *b, double *x) {
  mgs_ctx *ctx = h->ctx;
  mgs_level &L = h->lev[l], &C = h->lev[l + 1];
  const bool halo = L.A->cols > L.A->rows, chalo = C.A->cols > C.A->rows;
  const double *hv = halo ? L.hbuf->d : nullptr;
  fused_operands ops;
  level_fused_operands(h, l, halo, ops);
  const int arm = level_pre_arm(h, l, ops, halo && !L.nx && halo_split(h, L.A) && !h->capturing);
  const bool grouped = arm == PRE_ARM_GROUPED;
  if (grouped || arm == PRE_ARM_AGG || !halo) {
    // Grouped form: pre pass + restriction in one kernel (r stays in LDS; L.r receives t = b + r, L.tmp the residuals of the
    // few rows whose aggregate leaves its row-block group), post pass in its t-form.
    // On a row shard the right-hand side of the halo rows is exchanged first (no interior/boundary split in these forms).
    if (halo) MGS_TRY(mgs_halo_exchange(h, l, b, L.hbuf->d, true));
    MGS_TRY(launch_pre_arm(h, l, ops, arm, b, grouped ? L.r->d : nullptr, grouped ? L.tmp->d : L.r->d, C.b->d, hv));
  } else {
    // r = b − A·x1 with x1 = wd∘b (never stored: the POST pass recomputes it from b); a row shard launches around its exchange
    MGS_TRY(mgs_halo_exchange_around(h, l, L.A, b, L.hbuf->d, true, [&](int b0, int b1, int ga, int gl) {
      if (arm == PRE_ARM_RESIDUAL) return mgs_launch_coded_range(&ops.Ahat, MGS_OP_RESIDUAL, b, b, nullptr, 0.0, nullptr, nullptr, L.r->d, hv, L.A->rows, b0, b1, ga, gl);
      return mgs_launch_fused_range(L.A, FUSE_PRE, L.wd->d, b, nullptr, nullptr, nullptr, L.r->d, nullptr, hv, b0, b1, ga, gl); }));
    MGS_TRY(k_restrict_agg(ctx, L.T->n_coarse, L.T->cptr, L.T->members, L.r->d, C.b->d));
  }
  MGS_TRY(coarse_solve(h, l + 1, C.b->d, C.x->d));
  // e_c's halo: one exchange on the coarse level's plan — unless that level is the replicated tail's, whose solution already holds the
  // neighbours' entries (the kernel that hands over the own slice fills the halo slots too)
  const bool ec_exchange = chalo && !(l + 2 == (int)h->lev.size() && h->ntail && h->ntail->halo_global);
  double *ec = C.x->d;
  return mgs_halo_exchange_around(h, l + 1, L.A, ec_exchange ? ec : nullptr, ec + C.n, true, [&](int b0, int b1, int ga, int gl) {
    return launch_post_pass(h, l, ops, grouped, L.r->d, grouped ? nullptr : b, ec, x, b0, b1, ga, gl); });
}
// ν1 pre-sweeps, residual, restriction, coarse solve, correction, ν2 post-sweeps: one kernel per step
static int cycle_unfused(mgs_hier *h, int l, const double *b, double *x, bool zero_guess) {
  mgs_ctx *ctx = h->ctx;
  mgs_level &L = h->lev[l], &C = h->lev[l + 1];
  const int n = L.n;
  // number of out-of-place sweeps decides where the ping-pong ends; start so that it ends in x
  int swaps = h->nu2 + (zero_guess ? (h->nu1 > 0 ? h->nu1 - 1 : 0) : h->nu1);
  double *cur = x, *alt = L.tmp->d;
  if (zero_guess && (swaps & 1)) { cur = L.tmp->d; alt = x; }
  bool zero = zero_guess;
  for (int s = 0; s < h->nu1; ++s) {
    if (zero) { MGS_TRY(k_jacobi_zero(ctx, n, h->omega, L.dinv->d, b, cur)); zero = false; }
    else {
      MGS_TRY(sharded_op(h, l, L.A, MGS_OP_JACOBI, cur, b, L.dinv->d, h->omega, alt));
      std::swap(cur, alt);
    }
  }
  const double *r = L.r->d;
  if (zero) r = b;                                       // r = b − A·0
  else MGS_TRY(sharded_op(h, l, L.A, MGS_OP_RESIDUAL, cur, b, nullptr, 0.0, L.r->d));
  // restriction
  if (L.T->aggregation) MGS_TRY(k_restrict_agg(ctx, L.T->n_coarse, L.T->cptr, L.T->members, r, C.b->d));
  else MGS_TRY(mgs_launch_csr_op(L.T->Pt, MGS_OP_SPMV, r, nullptr, nullptr, 0.0, C.b->d));
  MGS_TRY(coarse_solve(h, l + 1, C.b->d, C.x->d));
  // prolongation / correction
  if (L.T->aggregation) MGS_TRY(k_prolong_agg(ctx, n, L.T->agg, C.x->d, cur, zero ? 0 : 1));
  else if (zero) MGS_TRY(mgs_launch_csr_op(L.T->P, MGS_OP_SPMV, C.x->d, nullptr, nullptr, 0.0, cur));
  else {
    MGS_TRY(mgs_launch_csr_op(L.T->P, MGS_OP_SPMV, C.x->d, nullptr, nullptr, 0.0, L.r->d));
    MGS_TRY(k_axpby(ctx, n, 1.0, L.r->d, 1.0, cur));
  }
  for (int s = 0; s < h->nu2; ++s) {
    MGS_TRY(sharded_op(h, l, L.A, MGS_OP_JACOBI, cur, b, L.dinv->d, h->omega, alt));
    std::swap(cur, alt);
  }
  if (cur != x) MGS_HIP(ctx, hipMemcpyAsync(x, cur, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
  return MGS_OK;
}
static int cycle_level(mgs_hier *h, int l, const double *b, double *x, bool zero_guess) {
  if (l == (int)h->lev.size() - 1) return cycle_coarsest(h, l, b, x);
  if (h->additive) return cycle_additive(h, l, b, x);
  if (zero_guess && level_fuses(h, l)) return cycle_fused(h, l, b, x);
  return cycle_unfused(h, l, b, x, zero_guess);
}

// One capture: `body` (launches on the context's stream) recorded and instantiated into *exec.  An error here means that the capture could not
// begin; past that point the caller gets the pair (*rc: what the body returned, *e: what HIP said) and *exec stays NULL unless both are clean.
template <class F>
static int capture_exec(mgs_hier *h, hipGraphExec_t *exec, int *rc, hipError_t *e, F body) {
  mgs_ctx *ctx = h->ctx;
  hipGraph_t g = nullptr;
  MGS_HIP(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
  h->capturing = true;
  ++ctx->graph_captures;
  *rc = body();
  h->capturing = false;
  *e = hipStreamEndCapture(ctx->stream, &g);
  if (*e == hipSuccess && *rc == MGS_OK) { *e = hipGraphInstantiate(exec, g, nullptr, nullptr, 0); if (*e != hipSuccess) *exec = nullptr; }
  if (g) hipGraphDestroy(g);
  return MGS_OK;
}

extern "C" {

int mgs_vcycle(mgs_hier *h, const mgs_vec *b, mgs_vec *x, int zero_guess) {
  mgs_ctx *ctx = h->ctx;
  MGS_CHECK(ctx, h->finalized, MGS_ERR_STATE, "mgs_vcycle: call mgs_hier_finalize first");
  MGS_TRY(mgs_prepare_fused(h));
  mgs_level &L0 = h->lev[0];
  MGS_CHECK(ctx, b->n >= L0.n && x->n >= L0.n, MGS_ERR_INVALID, "mgs_vcycle: vectors shorter than the operator (%d rows)", L0.n);
  MGS_CHECK(ctx, b->d != x->d, MGS_ERR_INVALID, "mgs_vcycle: x must not alias b");
  MGS_CHECK(ctx, !h->additive || zero_guess, MGS_ERR_INVALID, "mgs_vcycle: the additive form (bicg.cpp:59) is a preconditioner application from x = 0 only");
  if (h->lev.size() == 1 && !h->coarse_sweeps) return cycle_level(h, 0, b->d, x->d, true);
  auto entry = [&](const double *bb, double *xx, bool zg) -> int {      // kcycle_entry: two Krylov steps on level 0 itself (zero guess only)
    return (h->kcycle_entry && zg) ? coarse_solve_inner(h, 0, bb, xx) : cycle_level(h, 0, bb, xx, zg);
  };
  // sharded level 0 needs halo room behind the owned entries: work in the level's own buffer
  double *xw = x->d;
  const bool staged = x->n < L0.n_ext;
  if (staged) { xw = L0.x->d; if (!zero_guess) MGS_HIP(ctx, hipMemcpyAsync(xw, x->d, sizeof(double) * (size_t)L0.n, hipMemcpyDeviceToDevice, ctx->stream)); }
  // Native transport (RCCL send/recv groups and the tail all-gather are enqueued on this stream by the cycle itself):
  // capturable like any kernel launch once RCCL has set up its connections — two eager cycles first.
  const bool native = h->native || h->ntail;
  bool native_ok = false;
  if (native && ctx->opt_native_graph && !h->native_graph_failed) {
    // every exchange of the cycle must be native (installed callbacks are then never reached): each level with halo
    // columns has a plan, and the coarsest level is either square or handed to the native tail
    native_ok = h->ntail ? mgs_comm_capturable(h->ntail->comm) : (!h->coarse && h->lev.back().A->rows == h->lev.back().A->cols);
    for (auto &q : h->lev) if (q.nx ? !mgs_comm_capturable(q.nx->comm) : q.A->cols > q.A->rows) native_ok = false;
    if (native_ok && h->native_eager_runs < 2) { ++h->native_eager_runs; native_ok = false; }
  }
  const bool use_graph = ctx->opt_graph && (native ? native_ok : (!h->halo && !h->halo_begin && !h->coarse));
  if (h->graph_epoch != ctx->opt_epoch) mgs_drop_graph(h);
  h->graph_epoch = ctx->opt_epoch;
  // Split launch: a K-cycle's graph has hundreds of nodes (1.1 ms from hipGraphLaunch to its first kernel at 512³, and a cache keyed by
  // (b, x) that a flexible Krylov method with ten direction vectors overruns).  The fine level's passes go out eagerly instead, and the
  // levels below — which only touch their own buffers — replay from ONE graph whose submission hides behind the fine level's pre pass.
  const bool split_launch = use_graph && !native && zero_guess && h->kcycle_levels > 0 && !h->kcycle_entry && !h->additive && h->lev.size() > 2 &&
                            ctx->opt_graph_split_rows > 0 && L0.n >= ctx->opt_graph_split_rows && h->lev[1].b && h->lev[1].x;
  int rc = MGS_OK;
  hipError_t e = hipSuccess;
  if (split_launch) {
    if (!h->coarse_exec) {
      MGS_TRY(capture_exec(h, &h->coarse_exec, &rc, &e, [&]() { return coarse_solve(h, 1, h->lev[1].b->d, h->lev[1].x->d); }));
      if (rc != MGS_OK) return rc;
      if (e != hipSuccess) return mgs_fail(ctx, MGS_ERR_HIP, "coarse-level capture: %s", hipGetErrorString(e));
    }
    h->coarse_launch = true;
    rc = cycle_level(h, 0, b->d, xw, true);
    h->coarse_launch = false;
    MGS_TRY(rc);
  } else if (!use_graph) {
    MGS_TRY(entry(b->d, xw, zero_guess != 0));
  } else {
    const int zg = zero_guess != 0;
    mgs_hier::GraphSlot *slot = nullptr, *victim = &h->graphs[0];
    for (auto &g : h->graphs) {
      if (g.exec && g.b == b->d && g.x == xw && g.zero == zg) { slot = &g; break; }
      if (!g.exec) { if (victim->exec) victim = &g; }
      else if (victim->exec && g.stamp < victim->stamp) victim = &g;
    }
    if (!slot) {
      if (victim->exec) { hipGraphExecDestroy(victim->exec); *victim = mgs_hier::GraphSlot(); }
      if (h->ntail) MGS_TRY(mgs_prepare_fused(h->ntail->tail));      // allocations of the tail happen outside the capture
      if (native && ctx->opt_native_overlap && !ctx->comm_stream) MGS_HIP(ctx, hipStreamCreateWithFlags(&ctx->comm_stream, hipStreamNonBlocking));
      if (!ctx->opt_native_overlap && ctx->comm_stream) { hipStreamDestroy(ctx->comm_stream); ctx->comm_stream = nullptr; }
      h->fork_used = 0;
      MGS_TRY(capture_exec(h, &victim->exec, &rc, &e, [&]() { return entry(b->d, xw, zg != 0); }));
      if (rc != MGS_OK || e != hipSuccess) {
        if (!native) return rc != MGS_OK ? rc : mgs_fail(ctx, MGS_ERR_HIP, "cycle capture: %s", hipGetErrorString(e));
        // the transport could not be captured on this platform: eager launches from here on (same arithmetic)
        (void)hipGetLastError();
        h->native_graph_failed = true;
        ctx->err = std::string("native cycle not captured (") + (rc != MGS_OK ? ctx->err.c_str() : hipGetErrorString(e)) + "): eager launches";
        MGS_TRY(entry(b->d, xw, zg != 0));
        if (staged) MGS_HIP(ctx, hipMemcpyAsync(x->d, xw, sizeof(double) * (size_t)L0.n, hipMemcpyDeviceToDevice, ctx->stream));
        return MGS_OK;
      }
      victim->b = b->d; victim->x = xw; victim->zero = zg;
      slot = victim;
    }
    slot->stamp = ++h->graph_clock;
    MGS_HIP(ctx, hipGraphLaunch(slot->exec, ctx->stream));
  }
  if (staged) MGS_HIP(ctx, hipMemcpyAsync(x->d, xw, sizeof(double) * (size_t)L0.n, hipMemcpyDeviceToDevice, ctx->stream));
  return MGS_OK;
}

// ---- single passes of the cycle, launched alone (the exact-restatement tests)
int mgs_hier_pre_pass(mgs_hier *h, int level, const mgs_vec *b, mgs_vec *t, mgs_vec *r, mgs_vec *rc, int *nodiag) {
  MGS_CHECK(nullptr, h && b && t && r && rc, MGS_ERR_INVALID, "mgs_hier_pre_pass: NULL argument");
  mgs_ctx *ctx = h->ctx;
  MGS_CHECK(ctx, h->finalized, MGS_ERR_STATE, "mgs_hier_pre_pass: call mgs_hier_finalize first");
  MGS_CHECK(ctx, level >= 0 && level + 1 < (int)h->lev.size(), MGS_ERR_INVALID, "mgs_hier_pre_pass: level %d has no coarser level", level);
  MGS_TRY(mgs_prepare_fused(h));
  mgs_level &L = h->lev[level];
  const bool plain = L.A->cols == L.A->rows && !L.nx && !(L.A->code && L.A->code->vtab) && !L.code_hat;
  MGS_CHECK(ctx, ctx->opt_fuse_restrict && L.grp && L.val_wd && plain, MGS_ERR_STATE, "mgs_hier_pre_pass: level %d does not run the grouped pre pass (see mgs_hier_group_info), or is sharded / value-coded", level);
  MGS_CHECK(ctx, b->n >= L.n && t->n >= L.n && r->n >= L.n && rc->n >= L.T->n_coarse, MGS_ERR_INVALID, "mgs_hier_pre_pass: vectors shorter than the level (%d rows, %d aggregates)", L.n, L.T->n_coarse);
  fused_operands ops;
  level_fused_operands(h, level, false, ops);
  const bool nd = level_pre_nodiag(h, L, false, ops.f32);
  if (nodiag) *nodiag = nd ? 1 : 0;
  return launch_pre_arm(h, level, ops, PRE_ARM_GROUPED, b->d, t->d, r->d, rc->d, nullptr);
}
int mgs_hier_pre_pass_info(mgs_hier *h, int level, const mgs_vec *b, mgs_vec *t, mgs_vec *r, mgs_vec *rc, int64_t info[16]) {
  MGS_CHECK(nullptr, h && b && t && r && rc && info, MGS_ERR_INVALID, "mgs_hier_pre_pass_info: NULL argument");
  mgs_ctx *ctx = h->ctx;
  MGS_TRY(fused_pass_level(h, level, "mgs_hier_pre_pass_info"));
  mgs_level &L = h->lev[level];
  MGS_CHECK(ctx, b->n >= L.n && t->n >= L.n && r->n >= L.n && rc->n >= L.T->n_coarse, MGS_ERR_INVALID,
            "mgs_hier_pre_pass_info: vectors shorter than the level (%d rows, %d aggregates)", L.n, L.T->n_coarse);
  fused_operands ops;
  level_fused_operands(h, level, false, ops);
  const int arm = level_pre_arm(h, level, ops, false);
  mgs_launch_report rep;
  ctx->report = &rep;
  const int rcode = launch_pre_arm(h, level, ops, arm, b->d, t->d, r->d, rc->d, nullptr);
  ctx->report = nullptr;
  MGS_TRY(rcode);
  for (int q = 0; q < 16; ++q) info[q] = 0;
  const int nb = mgs_row_blocks(L.A);
  info[0] = arm; info[1] = rep.kernel; info[2] = rep.u; info[3] = rep.flags; info[4] = rep.capv; info[5] = rep.capi; info[6] = rep.bits;
  info[7] = info[8] = info[9] = -1;
  info[10] = arm == PRE_ARM_GROUPED ? L.grp->nstray : 0; info[11] = nb;
  // what every row block of the launch did, from the operand's block bounds, the table bounds the launch handed over and its LDS budgets — the
  // kernels' own block-uniform conditions (copies behind the launch; the host waits for them, the caller still synchronizes before it reads)
  const mgs_csr *op = arm == PRE_ARM_GATHER ? L.A : &ops.Ahat;
  if (op->blkptr && rep.kernel >= 0 && rep.kernel != 5) {
    std::vector<int> bp((size_t)nb + 1), tp;
    MGS_HIP(ctx, hipMemcpyAsync(bp.data(), op->blkptr, sizeof(int) * bp.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (rep.tptr) { tp.resize((size_t)nb + 1); MGS_HIP(ctx, hipMemcpyAsync(tp.data(), rep.tptr, sizeof(int) * tp.size(), hipMemcpyDeviceToHost, ctx->stream)); }
    MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int va = (rep.bits & 1) ? 4 : 2;      // values per 16-byte piece: the slice starts at a multiple of it
    int64_t ncoded = 0, nstaged = 0;
    for (int q = 0; q < nb; ++q) {
      const int lo = bp[q], hi = bp[q + 1], tlen = rep.tptr ? tp[q + 1] - tp[q] : 0;
      const bool coded = tlen > 0 && tlen <= rep.capi;
      const bool staged = hi - lo <= rep.capv && (coded || hi - (lo & ~(va - 1)) + va - 1 <= rep.capi);
      ncoded += coded && staged; nstaged += staged;
    }
    info[7] = ncoded; info[8] = nstaged; info[9] = nb - nstaged;
  }
  return MGS_OK;
}
int mgs_hier_post_pass(mgs_hier *h, int level, const mgs_vec *bvec, const mgs_vec *xin, const mgs_vec *ec, mgs_vec *x, const int range[4], int64_t info[8]) {
  MGS_CHECK(nullptr, h && bvec && ec && x && info, MGS_ERR_INVALID, "mgs_hier_post_pass: NULL argument");
  mgs_ctx *ctx = h->ctx;
  MGS_TRY(fused_pass_level(h, level, "mgs_hier_post_pass"));
  mgs_level &L = h->lev[level];
  MGS_CHECK(ctx, bvec->n >= L.n && (!xin || xin->n >= L.n) && x->n >= L.n && ec->n >= L.T->n_coarse, MGS_ERR_INVALID,
            "mgs_hier_post_pass: vectors shorter than the level (%d rows, %d aggregates)", L.n, L.T->n_coarse);
  const int nb = mgs_row_blocks(L.A);
  int b0 = 0, b1 = nb, ga = 0x7fffffff, gl = 0;
  if (range) {
    b0 = range[0]; b1 = range[1]; ga = range[2]; gl = range[3];
    const long long last = (long long)b1 - 1 + (b1 - 1 >= ga ? gl : 0);      // the highest row block the launch maps to
    MGS_CHECK(ctx, b0 >= 0 && b1 >= b0 && ga >= 0 && gl >= 0 && last < nb, MGS_ERR_INVALID, "mgs_hier_post_pass: row-block range {%d, %d, %d, %d} leaves the level's %d row blocks", b0, b1, ga, gl, nb);
  }
  fused_operands ops;
  level_fused_operands(h, level, false, ops);
  const mgs_csr *op = ops.operands ? &ops.Amap : L.A;
  mgs_launch_report rep;
  ctx->report = &rep;
  const int rc = launch_post_pass(h, level, ops, !range, bvec->d, xin ? xin->d : nullptr, ec->d, x->d, b0, b1, ga, gl);      // the group sweep launches whole levels only
  ctx->report = nullptr;
  MGS_TRY(rc);
  info[0] = ops.post_form; info[1] = rep.kernel; info[2] = rep.u; info[3] = rep.flags; info[4] = rep.capv; info[5] = rep.capi;
  // row blocks the kernel walks from global memory: entry counts from the operand's block bounds (a copy behind the launch; the host
  // waits for the copy, the caller still synchronizes before it reads x)
  int64_t over = -1;
  if (op->blkptr && rep.kernel >= 0) {
    std::vector<int> bp((size_t)nb + 1);
    MGS_HIP(ctx, hipMemcpyAsync(bp.data(), op->blkptr, sizeof(int) * bp.size(), hipMemcpyDeviceToHost, ctx->stream));
    MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    over = 0;
    for (int q = 0; q < nb; ++q) over += bp[q + 1] - bp[q] > rep.capv;
  }
  info[6] = over; info[7] = ops.grouped ? 1 : 0;
  return MGS_OK;
}
int mgs_hier_native_halo(mgs_hier *h, int level, void *x_dev) {
  MGS_CHECK(h->ctx, level >= 0 && level < (int)h->lev.size() && h->lev[level].nx, MGS_ERR_STATE, "mgs_hier_native_halo: level %d has no native plan", level);
  return native_exchange(h, level, (const double *)x_dev, (double *)x_dev + h->lev[level].A->rows);
}
int mgs_time_vcycle(mgs_hier *h, const mgs_vec *b, mgs_vec *x, int reps, double *ms) {
  mgs_ctx *ctx = h->ctx;
  MGS_CHECK(ctx, reps > 0 && ms, MGS_ERR_INVALID, "mgs_time_vcycle: bad arguments");
  hipEvent_t e0, e1;
  MGS_HIP(ctx, hipEventCreate(&e0)); MGS_HIP(ctx, hipEventCreate(&e1));
  MGS_HIP(ctx, hipEventRecord(e0, ctx->stream));
  for (int i = 0; i < reps; ++i) MGS_TRY(mgs_vcycle(h, b, x, 1));
  MGS_HIP(ctx, hipEventRecord(e1, ctx->stream));
  MGS_HIP(ctx, hipEventSynchronize(e1));
  float t = 0; MGS_HIP(ctx, hipEventElapsedTime(&t, e0, e1));
  hipEventDestroy(e0); hipEventDestroy(e1);
  *ms = (double)t / reps;
  return MGS_OK;
}

}  // extern "C"
