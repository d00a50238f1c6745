// hier_operands.hip — the derived operands of a level's two fused passes from allocation to free, host code only (the chain and its one record of staleness:
// mgs_level::dirty, mgs_internal.hpp; which operand a launch reads: cycle.hip).  mgs_prepare_fused allocates what a cycle under the options as they stand needs and fills
// what is dirty; mgs_hier_refresh marks all dirty and refills what exists.  mgs_drop_graph is called where a buffer a captured graph may know is allocated, freed or replaced.
#include "mgs_internal.hpp"
void mgs_operands_mark(mgs_level &L, unsigned bits) {
  if (bits & OPD_WD) bits |= OPD_HAT;
  if (bits & OPD_HAT) bits |= OPD_ND | OPD_HAT32 | OPD_CODES;
  if (bits & OPD_AP) bits |= OPD_AP32;
  L.dirty |= bits;
  if (L.pk_hat && (bits & (OPD_HAT | OPD_ND))) L.pk_hat->dirty = true;
  if (L.pk_ap && (bits & OPD_AP)) L.pk_ap->dirty = true;
}
// The ONE fill of every operand — the launch that computes it from its source, in place, enqueue-only — run where it is asked for (want), the array exists and is dirty,
// and its source is in step.  val_nd: a diagonal entry further from ω than a byte holds (1/a_ii under- or overflowed) is counted in h->nd_flag, which the caller zeroes before
// and reads after (its host synchronisation point).  A·P's numeric refill is asked for by mgs_hier_refresh alone, which owns the miss counter.
int mgs_operands_fill(mgs_hier *h, int l, unsigned want) {
  mgs_ctx *ctx = h->ctx; mgs_level &L = h->lev[l];
  auto due = [&](unsigned bit, unsigned src, const void *array) { return array && (want & L.dirty & bit) && !(L.dirty & src); };
  if (due(OPD_WD, 0, L.wd)) { MGS_TRY(k_axpby(ctx, L.n_ext, h->omega, L.dinv->d, 0.0, L.wd->d)); L.dirty &= ~OPD_WD; }
  if (due(OPD_HAT, OPD_WD, L.val_wd)) { MGS_TRY(k_scale_vals(ctx, L.A, L.wd->d, L.val_wd)); L.dirty &= ~OPD_HAT; }
  if (due(OPD_AP, 0, L.AP)) { MGS_TRY(k_galerkin_numeric(L.A, L.A->rows, nullptr, nullptr, L.T->agg, L.AP, h->refresh_flags + 1)); L.dirty &= ~OPD_AP; }
  if (due(OPD_HAT32, OPD_HAT, L.val_wd32)) { MGS_TRY(k_round_vals(ctx, L.val_wd, L.val_wd32, L.A->nnz)); L.dirty &= ~OPD_HAT32; }
  if (due(OPD_AP32, OPD_AP, L.ap_val32)) { MGS_TRY(k_round_vals(ctx, L.AP->val, L.ap_val32, L.AP->nnz)); L.dirty &= ~OPD_AP32; }
  if (due(OPD_ND, OPD_HAT, L.val_nd) && L.nd_ok) {
    MGS_TRY(k_drop_diag_vals(ctx, L.A, L.val_wd, h->omega, L.val_nd, L.nd_code, h->nd_flag));
    L.nd_omega = h->omega; L.dirty &= ~OPD_ND;
  }
  const bool nd = mgs_level_nd_ready(L);      // the pre pass's packed copy is of val_nd where the level streams that, of val_wd otherwise (pack7_alloc)
  const struct { mgs_pack7 *p; const mgs_csr *M; const double *src; bool nd; unsigned src_bit; } packs[2] = {
      {L.pk_hat, L.A, nd ? L.val_nd : L.val_wd, nd, nd ? OPD_ND : OPD_HAT}, {L.pk_ap, L.AP, L.AP ? L.AP->val : nullptr, false, OPD_AP}};
  for (auto &q : packs)
    if ((want & OPD_PACKS) && q.p && q.p->dirty && q.p->nd == q.nd && !(L.dirty & q.src_bit)) {
      MGS_TRY(k_pack7(ctx, q.M->blkptr, q.p->nblocks, q.nd ? q.M->rows : -1, q.src, q.p->e0, q.p->data));
      q.p->dirty = false;
    }
  return MGS_OK;
}
// ------------------------------------------------------------------ allocation and release
static void pack7_free(mgs_pack7 *&p) { if (p) { mgs_hip_free(p->data); mgs_hip_free(p->e0); delete p; p = nullptr; } }
static int pack7_alloc(mgs_hier *h, mgs_pack7 *&p, int nblocks, int64_t nent, bool nd) {      // option pack7: a (new, hence dirty) packed copy where there is none or one of another source or shape
  mgs_ctx *ctx = h->ctx;
  if (p && (p->nd != nd || p->nent != nent || p->nblocks != nblocks)) { pack7_free(p); mgs_drop_graph(h); }
  if (p) return MGS_OK;
  p = new mgs_pack7(); p->nd = nd; p->nent = nent; p->nblocks = nblocks;
  const size_t bytes = (size_t)112 * (size_t)((nent + 15) / 16) + 16;      // padded to a whole record
  MGS_TRY(mgs_dev_alloc(ctx, &p->data, bytes));
  MGS_HIP(ctx, hipMemsetAsync(p->data, 0, bytes, ctx->stream));
  MGS_TRY(mgs_dev_alloc(ctx, &p->e0, (size_t)nblocks));
  mgs_drop_graph(h); return MGS_OK;
}
static int f32_alloc(mgs_hier *h, mgs_level &L) {      // the FP32 copies of a level switched to 32 bits
  if (L.op_bits != 32 || !L.val_wd || !L.AP) return MGS_OK;
  if (!L.val_wd32) { MGS_TRY(mgs_dev_alloc(h->ctx, &L.val_wd32, (size_t)L.A->nnz + 8)); mgs_drop_graph(h); }
  if (!L.ap_val32) { MGS_TRY(mgs_dev_alloc(h->ctx, &L.ap_val32, (size_t)L.AP->nnz + 8)); mgs_drop_graph(h); }
  return MGS_OK;
}
void mgs_operands_free(mgs_level &L) {
  mgs_vec_destroy(L.wd); mgs_vec_destroy(L.hbuf);
  for (void *p : {(void *)L.val_wd, (void *)L.val_nd, (void *)L.nd_code, (void *)L.val_wd32, (void *)L.ap_val32, (void *)L.col_agg, (void *)L.cmap_ext, (void *)L.dpos}) mgs_hip_free(p);
  pack7_free(L.pk_hat); pack7_free(L.pk_ap);
  if (L.AP) mgs_csr_destroy(L.AP);
  for (mgs_rowcode *c : {L.code_agg, L.code_ap, L.code_pre, L.code_hat}) mgs_free_rowcode(c);
  mgs_free_groups(L.grp);
}
// wd = ω·dinv of every level that can run the fused passes and the operands derived from it; allocated and filled outside any stream capture
int mgs_prepare_fused(mgs_hier *h) {
  mgs_ctx *ctx = h->ctx;
  if (ctx->opt_rowcode)      // pattern codes of the level operators (a cache attached to the matrices)
    for (mgs_level &L : h->lev)
      if (!L.A->code_tried) { MGS_TRY(mgs_csr_optimize(const_cast<mgs_csr *>(L.A))); mgs_drop_graph(h); }
  for (int l = h->kcycle_entry ? 0 : 1; l <= h->kcycle_levels && l < (int)h->lev.size() - 1; ++l) {
    mgs_level &L = h->lev[l];
    if (L.kscal) continue;
    for (mgs_vec **q : {&L.kc1, &L.kv1, &L.kc2, &L.kv2, &L.kr}) MGS_TRY(mgs_vec_create(ctx, L.n_ext, q));
    MGS_TRY(mgs_dev_alloc(ctx, &L.kscal, 8));
    MGS_HIP(ctx, hipMemsetAsync(L.kscal, 0, 8 * sizeof(double), ctx->stream));      // defined before the first step (mgs_hier_kcycle_scalars)
    mgs_drop_graph(h);
  }
  const bool sharded = h->halo || h->halo_begin || h->native;
  if (!ctx->opt_fuse || h->nu1 != 1 || h->nu2 != 1 || (sharded && !h->halo_fused && !h->native)) return MGS_OK;
  for (size_t l = 0; l + 1 < h->lev.size(); ++l) {
    mgs_level &L = h->lev[l];
    if (!L.T || !L.T->aggregation) continue;
    if (L.A->rows != L.A->cols && !h->halo_fused && !L.nx) continue;
    const bool shard = L.A->cols > L.A->rows;
    if (!L.wd) { MGS_TRY(mgs_vec_create(ctx, L.n_ext, &L.wd)); mgs_drop_graph(h); }
    if (shard && !L.hbuf) MGS_TRY(mgs_vec_create(ctx, L.A->cols - L.A->rows, &L.hbuf));
    if (shard && !L.halo_dinv) {
      // one exchange at setup: the owners' D⁻¹ of the rows this shard sees as halo.  With it Â's halo columns are scaled like the
      // owned ones, and what the pre pass needs from the peers per cycle is their raw right-hand side (no packed product).
      // Collective: every rank prepares its hierarchy in its first cycle.
      MGS_TRY(mgs_halo_exchange(h, (int)l, L.dinv->d, L.dinv->d + L.A->rows));
      L.halo_dinv = true; mgs_operands_mark(L, OPD_WD); mgs_drop_graph(h);
    }
    if (shard && !L.cmap_ext && L.T->halo_cmap && L.T->n_halo_fine == L.A->cols - L.A->rows) {      // coarse column of every local column
      MGS_TRY(mgs_dev_alloc(ctx, &L.cmap_ext, (size_t)L.A->cols));
      MGS_TRY(k_concat_i32(ctx, L.T->agg, L.A->rows, L.T->halo_cmap, L.T->n_halo_fine, L.cmap_ext));
      mgs_drop_graph(h);
    }
    if (shard && !L.cmap_ext) continue;      // shard not built by mgs_galerkin_shard: one kernel per step on this level
    MGS_TRY(mgs_operands_fill(h, (int)l, OPD_WD));
    if (!ctx->opt_fuse_operands) continue;      // below: the derived CSR operands of the fused passes (same shape as A)
    if (!L.val_wd) { MGS_TRY(mgs_dev_alloc(ctx, &L.val_wd, (size_t)L.A->nnz + 4)); mgs_drop_graph(h); }
    MGS_TRY(mgs_operands_fill(h, (int)l, OPD_HAT));
    if (ctx->opt_merge_ap && !L.AP) {      // (the coarse level's local columns: its rows + its halo slots)
      MGS_TRY(k_build_ap(L.A, L.T, L.cmap_ext, h->lev[l + 1].A->cols, &L.AP)); mgs_drop_graph(h);
      L.dirty &= ~OPD_AP;      // the structural build computes the values too
      L.AP->far_band = L.A->far_band; L.AP->far_band_max = L.A->far_band_max;     // sweep order of the launch: the band of A (AP's columns are coarse ids)
      if (ctx->opt_rowcode)
        MGS_TRY(mgs_build_rowcode(ctx, L.AP->rows, L.AP->rowptr, L.AP->col, L.T->agg, 0x7fffffff, &L.code_ap, ctx->opt_valcode ? L.AP->val : nullptr));
    }
    if (!ctx->opt_merge_ap && !L.col_agg) {
      MGS_TRY(mgs_dev_alloc(ctx, &L.col_agg, (size_t)L.A->nnz + 4)); MGS_TRY(k_map_cols(ctx, L.A, L.cmap_ext ? L.cmap_ext : L.T->agg, L.col_agg)); mgs_drop_graph(h);
      if (ctx->opt_rowcode)
        MGS_TRY(mgs_build_rowcode(ctx, L.A->rows, L.A->rowptr, L.col_agg, L.T->agg, 0x7fffffff, &L.code_agg, ctx->opt_valcode ? L.A->val : nullptr));
    }
    if (ctx->opt_diag_from_values && !L.dpos && !ctx->opt_merge_ap) { MGS_TRY(mgs_dev_alloc(ctx, &L.dpos, (size_t)L.A->rows)); MGS_TRY(k_diag_pos(L.A, L.dpos)); mgs_drop_graph(h); }
    // row-block groups of the grouped pre pass (null: level does not qualify)
    if (ctx->opt_fuse_restrict && !L.grp_tried) { L.grp_tried = true; MGS_TRY(mgs_build_groups(ctx, L.A, L.T, &L.grp)); mgs_drop_graph(h); }
    // codes whose tuples depend on Â's values (or, on a shard, on the halo tags) follow val_wd, replaced, not refilled: whatever the options say NOW, a code built from
    // the old Â must not survive it.  On a shard the pre pass reads b (owned entries only) + the payload: halo columns need tagged table words
    if (L.dirty & OPD_CODES) {
      const bool build = ctx->opt_rowcode && (shard || ctx->opt_valcode);
      if (L.code_pre || L.code_hat || build) mgs_drop_graph(h);
      mgs_free_rowcode(L.code_pre); L.code_pre = nullptr; mgs_free_rowcode(L.code_hat); L.code_hat = nullptr;
      if (build && shard) MGS_TRY(mgs_build_rowcode(ctx, L.A->rows, L.A->rowptr, L.A->col, nullptr, L.A->rows, &L.code_pre, ctx->opt_valcode ? L.val_wd : nullptr));
      else if (build) MGS_TRY(mgs_build_rowcode(ctx, L.A->rows, L.A->rowptr, L.A->col, nullptr, 0x7fffffff, &L.code_hat, L.val_wd));
      L.dirty &= ~OPD_CODES;
    }
    MGS_TRY(f32_alloc(h, L));      // FP32 copies follow their FP64 operands (a new ω rescales Â)
    MGS_TRY(mgs_operands_fill(h, (int)l, OPD_HAT32 | OPD_AP32));
  }
  // Compact operand of the grouped pre pass (option pre_nodiag), allocated behind everything above: the other operands stay where the
  // arena places them without it.  Eligibility is decided once per level; the values follow val_wd.
  for (size_t l = 0; ctx->opt_fuse_operands && ctx->opt_pre_nodiag && l + 1 < h->lev.size(); ++l) {
    mgs_level &L = h->lev[l];
    if (!L.val_wd || !L.grp) continue;
    if (!L.nd_tried) {
      L.nd_tried = true; int bad = 1;
      if (L.A->cols == L.A->rows && !L.nx && L.A->max_row_len <= 64 && L.A->nnz >= L.A->rows) MGS_TRY(k_diag_count(L.A, &bad));
      L.nd_ok = bad == 0;
    }
    if (!L.nd_ok) continue;
    if (!L.val_nd) {
      const size_t m = (size_t)(L.A->nnz - L.A->rows);
      MGS_TRY(mgs_dev_alloc(ctx, &L.val_nd, m + 8));
      MGS_HIP(ctx, hipMemsetAsync(L.val_nd + m, 0, 8 * sizeof(double), ctx->stream));
      MGS_TRY(mgs_dev_alloc(ctx, &L.nd_code, (size_t)L.A->rows));
      if (!h->nd_flag) MGS_TRY(mgs_dev_alloc(ctx, &h->nd_flag, 1));
      mgs_drop_graph(h);
    }
    if (L.dirty & OPD_ND) {      // the flag is read per level here: an overflow ends the compact operand of this level only
      int bad = 0; MGS_HIP(ctx, hipMemsetAsync(h->nd_flag, 0, sizeof(int), ctx->stream));
      MGS_TRY(mgs_operands_fill(h, (int)l, OPD_ND));
      MGS_HIP(ctx, hipMemcpyAsync(&bad, h->nd_flag, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
      MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
      if (bad) { L.nd_ok = false; mgs_drop_graph(h); }
    }
  }
  // Packed copies of the operands' values (option pack7) on unsharded FP64 levels, allocated behind everything above for the same reason; the values follow their sources.
  for (size_t l = 0; ctx->opt_fuse_operands && ctx->opt_pack7 && !ctx->opt_valcode && l + 1 < h->lev.size(); ++l) {
    mgs_level &L = h->lev[l];
    if (!L.val_wd || !L.T || !L.T->aggregation || L.A->cols != L.A->rows || L.nx || !L.A->blkptr || L.op_bits != 64) continue;
    const bool nd = mgs_level_nd_ready(L);
    MGS_TRY(pack7_alloc(h, L.pk_hat, mgs_row_blocks(L.A), nd ? L.A->nnz - L.A->rows : L.A->nnz, nd));
    if (L.AP && L.AP->blkptr) MGS_TRY(pack7_alloc(h, L.pk_ap, mgs_row_blocks(L.AP), L.AP->nnz, false));
    MGS_TRY(mgs_operands_fill(h, (int)l, OPD_PACKS));
  }
  return MGS_OK;
}
// ------------------------------------------------------------------ operand precision (mgs_hier_set_operand_precision)
// A level can run its two fused passes on FP32 copies of Â's and A·P's values when both operands exist, the level is square (no halo
// columns) and both have short rows — then the float forms of the coded / grouped / aggregate-parallel kernels serve every row block.
static bool level_f32_eligible(const mgs_hier *h, int l) {
  if (l < 0 || l + 1 >= (int)h->lev.size()) return false;
  const mgs_level &L = h->lev[l]; const mgs_ctx *ctx = h->ctx;
  return ctx->opt_fuse && ctx->opt_fuse_operands && ctx->opt_merge_ap && !ctx->opt_valcode && L.T && L.T->aggregation && L.A->rows == L.A->cols &&
         L.val_wd && L.AP && L.A->blkptr && L.AP->blkptr && L.A->lds_cap > 0 && L.AP->lds_cap > 0 && L.A->max_row_len <= 64 && L.AP->max_row_len <= 64;
}
// ... and does so in the cycle the hierarchy would run NOW: only the fused zero-guess V(1,1) branch reads the operands at all
bool mgs_level_runs_f32(const mgs_hier *h, int l) {
  if (!level_f32_eligible(h, l)) return false;
  const mgs_level &L = h->lev[l];
  return L.op_bits == 32 && L.val_wd32 && L.ap_val32 && h->nu1 == 1 && h->nu2 == 1 && !h->additive;
}

extern "C" {
int mgs_hier_set_operand_precision(mgs_hier *h, int bits, int levels) {
  MGS_CHECK(nullptr, h, MGS_ERR_INVALID, "mgs_hier_set_operand_precision: NULL hierarchy");
  mgs_ctx *ctx = h->ctx;
  MGS_CHECK(ctx, bits == 64 || bits == 32, MGS_ERR_INVALID, "mgs_hier_set_operand_precision: bits must be 64 or 32 (got %d)", bits);
  MGS_CHECK(ctx, h->finalized, MGS_ERR_INVALID, "mgs_hier_set_operand_precision: call mgs_hier_finalize first");
  if (bits == 32) {
    MGS_CHECK(ctx, !ctx->opt_valcode, MGS_ERR_INVALID, "mgs_hier_set_operand_precision: option valcode is on (coded blocks stream no values: nothing to shrink)");
    MGS_CHECK(ctx, !mgs_hier_sharded(h), MGS_ERR_INVALID, "mgs_hier_set_operand_precision: row-sharded hierarchies (halo columns, native tail) keep FP64 operands");
    // the operands are prepared lazily, before a hierarchy's first cycle: do it now, so that the query answers right after this call
    MGS_TRY(mgs_prepare_fused(h));
  }
  const int nl = (int)h->lev.size(); int k = 0;      // k: the longest eligible prefix, at most `levels` long
  if (bits == 32) while (k < nl - 1 && (levels < 0 || k < levels) && level_f32_eligible(h, k)) ++k;
  for (int l = 0; l < nl; ++l) {
    mgs_level &L = h->lev[l];
    L.op_bits = l < k ? 32 : 64;
    if (L.op_bits == 32) { MGS_TRY(f32_alloc(h, L)); MGS_TRY(mgs_operands_fill(h, l, OPD_HAT32 | OPD_AP32)); }
    else if (L.val_wd32 || L.ap_val32) {      // the FP64 operands were kept: nothing to rebuild on the way back
      hipStreamSynchronize(ctx->stream); mgs_hip_free(L.val_wd32); mgs_hip_free(L.ap_val32);
      L.val_wd32 = nullptr; L.ap_val32 = nullptr; mgs_operands_mark(L, OPD_HAT32 | OPD_AP32);
    }
  }
  mgs_drop_graph(h); return MGS_OK;
}
int mgs_hier_operand_precision(const mgs_hier *h, int level, int *bits) {
  MGS_CHECK(nullptr, h && bits, MGS_ERR_INVALID, "mgs_hier_operand_precision: NULL argument");
  MGS_TRY(mgs_level_in_range(h, level, "mgs_hier_operand_precision"));
  *bits = mgs_level_runs_f32(h, level) ? 32 : 64; return MGS_OK;
}
int mgs_hier_fused_info(const mgs_hier *h, int level, int64_t out[6]) {
  MGS_TRY(mgs_level_in_range(h, level, "mgs_hier_fused_info"));
  const mgs_level &L = h->lev[level];
  auto coded = [](const mgs_rowcode *c) -> int64_t { return c ? c->coded_blocks : 0; };
  out[0] = mgs_row_blocks(L.A); out[1] = L.val_wd != nullptr; out[2] = L.col_agg != nullptr || L.AP != nullptr;
  out[3] = coded(L.A->code); out[4] = coded(L.code_pre); out[5] = coded(L.AP ? L.code_ap : L.code_agg);
  return MGS_OK;
}
int mgs_hier_pack_info(mgs_hier *h, int level, int64_t out[8]) {
  MGS_CHECK(nullptr, h && out, MGS_ERR_INVALID, "mgs_hier_pack_info: NULL argument");
  mgs_ctx *ctx = h->ctx;
  MGS_TRY(mgs_level_in_range(h, level, "mgs_hier_pack_info"));
  const mgs_level &L = h->lev[level];
  for (int q = 0; q < 8; ++q) out[q] = q == 3 || q == 6 ? -1 : 0;
  for (int w = 0; w < 2; ++w) {
    const mgs_pack7 *p = w ? L.pk_ap : L.pk_hat;
    if (!p) continue;
    std::vector<int> e0((size_t)p->nblocks);
    MGS_HIP(ctx, hipMemcpyAsync(e0.data(), p->e0, sizeof(int) * e0.size(), hipMemcpyDeviceToHost, ctx->stream));
    MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t packed = std::count_if(e0.begin(), e0.end(), [](int v) { return v >= 0; });
    const bool unused = p->dirty || L.op_bits != 64 || ctx->opt_valcode || !ctx->opt_pack7;      // no launch reads the copy as things stand
    out[w ? 4 : 0] = p->nblocks; out[w ? 5 : 1] = unused ? 0 : packed; out[w ? 6 : 3] = p->ran;
    if (!w) out[2] = p->nd ? 2 : 1;
    out[7] += (int64_t)112 * ((p->nent + 15) / 16) + 16 + (int64_t)sizeof(int) * p->nblocks;
  }
  return MGS_OK;
}
}  // extern "C"
