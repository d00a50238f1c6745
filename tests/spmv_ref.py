"""Host restatement of the standalone operator kernels (mgs_spmv, mgs_residual, mgs_jacobi: mgs_launch_csr_op_range and the kernels of
multigridsolver_amd/csrc/kernels_spmv.hip and, for the variants 2–4, 6 and 7, kernels_variants.hip), of the plan that picks their arm (mgs_plan_csr,
rowblock_setup.hip), their derived per-row error bar, and the
fixtures the CPU and GPU tests of these kernels share.  NumPy, FP64; no device, no oracle.

The operation.  For a CSR matrix A (stored order = ascending columns) and vectors x, b, dinv with  s_i = Σ_k v_ik·x[c_ik]:
    spmv      y_i = s_i
    residual  r_i = b_i − s_i
    jacobi    x'_i = x_i + (ω·dinv_i)·(b_i − s_i)          (the parenthesisation is part of the promise: `apply`)
The library is built with floating-point contraction off, so a product and the add that takes it are two roundings, and NumPy's float64
arithmetic — which never contracts — restates a kernel exactly once it takes the same operations in the same order.

Two summation orders exist.
  sequential  s = +0.0, then s += v_k·x[c_k] for k in stored order.  This is the order of the staged arm of every kernel (the slice kernel
              csr_rowblock_slice_kernel, the products-in-LDS kernel csr_rowblock_kernel, the pipelined and the one-wave kernels, the
              pattern-coded kernel) and of the slice and coded kernels' walk from global memory over a block heavier than the LDS budget
              whose matrix has no row longer than 64.  The gather steps of the slice and coded kernels that reach past a row's end
              add +0.0, which changes no bit of a sum that started at +0.0 (such a sum is never −0.0); what they gathered — another
              row's column, possibly a NaN or an infinity in x — is discarded by a select, not multiplied by zero.
  lanes(L)    L lanes share a row: lane l sums the entries a + l, a + l + L, … sequentially from +0.0; then for off = L/2 … 1 lane l
              adds lane l + off's value (__shfl_down); lane 0 holds the row's sum.  L is the smallest power of two in [4, 64] that
              is ≥ nnz/rows.  This is the order of a block heavier than the budget when the matrix has a row longer than 64 (slice
              kernel), of EVERY over-budget block of variants 2–4 (csr_rowblock_kernel has no sequential walk from global memory),
              and of every block of variant 1 when the matrix has a row longer than 64 (variant 1 stages nothing; with no such row
              its blocks take the sequential walk).

Which arm (`arm`).  cap = lds_cap of the plan (variant 1: −1).  A row block of cnt entries is STAGED when cnt ≤ cap.
    variants 0 and 5 (and 1)   slice kernel: staged, else sequential when max_row_len ≤ 64, else lanes(L)
    variants 2, 3, 4           csr_rowblock_kernel with 1, 2, 4 entries per lane and step: staged, else lanes(L)
    variant 6                  the pipelined kernel (`pipe`) for the whole matrix when max_block_nnz ≤ 2047 and max_block_nnz = lds_cap
                               (nothing over budget), else the slice kernel
    variant 7                  the one-wave kernel (`wave`) for the whole matrix when max_wave_nnz ≤ 4096, else the slice kernel
    variant 0 with a usable pattern code (mgs_csr_optimize; `coded=True`): the coded kernel — staged or the sequential walk.
The pipe bound (`pairs_needed`).  The pipelined kernel holds ITER·RB = 4·256 = 1024 sixteen-byte pairs (value pair + column pair) of a
row block in registers.  A block's slice starts at the even entry index lo & ~1, so a block [lo, hi) needs
(hi − (lo & ~1) + 1) >> 1 pairs: with cnt = hi − lo that is ⌈cnt/2⌉ for an even lo and ⌊cnt/2⌋ + 1 for an odd one — 1024 for
cnt = 2047 at either parity, 1024 for cnt = 2048 at an even lo, 1025 for cnt = 2048 at an odd lo, whose pair 1024 (the block's last
entry) would never be loaded.  Hence the bound 2047 of the guard; it was 2048 before this restatement was written.

The bar (`bar`), per row, derived (u = 2⁻⁵³, γ_m = m·u/(1 − m·u), L = stored length of the row, S_i = Σ_k |v_ik·x[c_ik]|).  Standard model
fl(a ∘ b) = (a ∘ b)(1 + δ), |δ| ≤ u, no underflow (the inputs lie in ±[0.5, 2] or are exact zeros):
  * ŝ_i.  Each product takes one rounding.  An addition one of whose operands is an exact zero (the +0.0 a chain starts from, the +0.0
    of a lane without entries, of a gather step past the row's end) is exact; strike those and either order is a binary tree over the
    row's L products, in which a product passes at most L − 1 rounded additions.  So |ŝ_i − s_i| ≤ γ_L·S_i for both orders, and
    γ_{L+1}·S_i — the figure used — leaves one u·S_i to spare, which pays for every second-order term below.
  * residual  r̂ = fl(b − ŝ): one further rounding, relative to the result:  |r̂ − r| ≤ γ_{L+1}·S + u·|b − s|.
  * jacobi    x̂' = fl(x + fl(ŵ·r̂)), ŵ = fl(ω·dinv): three further roundings.  ŵ·r̂ carries the error of r̂ scaled by |ω·dinv| and
    two δ of its own (ŵ, the product); the final sum one δ on the result:
        |x̂' − x'| ≤ |ω·dinv|·(γ_{L+1}·S + u·|b − s|) + 2u·|ω·dinv·(b − s)| + u·|x + ω·dinv·(b − s)|.
The exact values are taken in long double (64-bit mantissa) from the same FP64 inputs; their own error, (L + 3)·2⁻⁶⁴ relative to the same
magnitudes, is 2⁻¹¹ of the bar and is ignored.  `ratios` returns |x̂ − x| / bar per row; a row passes at ≤ 1 (a row whose bar is 0 — all
its terms are zeros — passes only with an error of exactly 0).

Inputs.  Values and vectors are drawn from ±[0.5, 2] as in the other *_ref modules: no term of a row is negligible beside the row's
sum, so a dropped or doubled entry or a neighbour's range moves the result by ≥ 0.25, and any change of the ORDER of three or more such
terms changes the low bits of most rows — which the planted defects of tests/test_spmv_ref_cpu.py show fixture by fixture."""
import numpy as np
import scipy.sparse as sps

from post_pass_ref import Guarded, SENT, signed  # noqa: F401  (re-exported: the output vectors of the GPU test)

U = 2.0 ** -53
RB = 256               # rows per row block (MGS_RB)
LDS_CAP_MAX = 5120     # entries staged per row block at the most
PIPE_PAIRS = 4 * RB    # sixteen-byte pairs of a row block the pipelined kernel holds in registers (ITER · RB)
WAVE_CAP = 4096        # entries of a 64-row group the one-wave kernel accepts


# ---- the plan (mgs_plan_csr) ----
def row_blocks(n_rows):
    return (n_rows + RB - 1) // RB


def plan(rowptr, col, n_rows, n_cols):
    """what mgs_plan_csr derives from the pattern; the keys of Csr.plan_info() plus lds_cap, max_wave_nnz, nblocks, rows, nnz, block_nnz
    (entries per row block) and block_lo (first entry index per row block)"""
    rp = np.asarray(rowptr, dtype=np.int64); col = np.asarray(col, dtype=np.int64)
    n = int(n_rows); nnz = int(rp[n]) if len(rp) else 0
    out = dict(max_block_nnz=0, max_row_len=0, far_band=0, lds_bytes=(0 + 2) * 12 + 16, halo_lo_blocks=0, halo_hi_blocks=0, halo_split_ok=0,
               has_long_row_blocks=0, lds_cap=0, max_wave_nnz=0, nblocks=0, rows=n, nnz=nnz, block_nnz=np.zeros(0, dtype=np.int64),
               block_lo=np.zeros(1, dtype=np.int64))
    if n == 0:
        return out
    nb = row_blocks(n)
    blo = rp[np.minimum(np.arange(nb + 1) * RB, n)]
    bnnz = np.diff(blo)
    wave = np.diff(rp[np.minimum(np.arange((n + 63) // 64 + 1) * 64, n)])          # row blocks are four 64-row groups: the same groups
    lens = np.diff(rp)
    rows = np.arange(n)
    # far band: per non-empty row max(0, row − first column, last OWNED column − row); integer mean over all rows
    ne = lens > 0
    first = np.zeros(n, dtype=np.int64); first[ne] = col[rp[:-1][ne]]
    owned = col < n
    rowid = np.repeat(rows, lens)
    last_owned = np.full(n, -1, dtype=np.int64)
    np.maximum.at(last_owned, rowid[owned], col[owned])
    rf = np.where(ne, np.maximum(0, rows - first), 0)
    rf = np.where(ne & (last_owned >= 0), np.maximum(rf, last_owned - rows), rf)
    out.update(max_block_nnz=int(bnnz.max()), max_row_len=int(lens.max()), far_band=int(rf.sum()) // n, max_wave_nnz=int(wave.max()),
               nblocks=nb, block_nnz=bnnz, block_lo=blo)
    # row blocks that read halo columns (col >= rows): usable for overlap when they form a prefix + suffix of the shard
    if n_cols > n:
        halo_blk = np.zeros(nb, dtype=bool)
        halo_blk[np.unique(rowid[~owned] // RB)] = True
        plain = np.flatnonzero(~halo_blk)
        if len(plain) == 0:
            out.update(halo_lo_blocks=nb)
        else:
            lo_cnt, hi_cnt = int(plain.min()), nb - 1 - int(plain.max())
            out.update(halo_lo_blocks=lo_cnt, halo_hi_blocks=hi_cnt,
                       halo_split_ok=int(int(halo_blk.sum()) == lo_cnt + hi_cnt and nb - lo_cnt - hi_cnt > 0))
    cap = max(64, min(out["max_block_nnz"], LDS_CAP_MAX))
    mean = nnz / nb
    if nb >= 64 and cap > 1.12 * mean:      # the budget step: the smallest candidate that still stages ≥ 98.5 % of the row blocks
        for f in (1.06, 1.12, 1.25, 1.5):
            cand = int(f * mean) + 8
            if cand < cap and int((bnnz > cand).sum()) <= 0.015 * nb:
                cap = cand
                break
    out.update(lds_cap=cap, lds_bytes=(cap + 2) * 12 + 16, has_long_row_blocks=int(out["max_block_nnz"] > cap))
    return out


PLAN_INFO_KEYS = ("max_block_nnz", "max_row_len", "far_band", "lds_bytes", "halo_lo_blocks", "halo_hi_blocks", "halo_split_ok", "has_long_row_blocks")


def plan_of(M):
    return plan(M.indptr, M.indices, M.shape[0], M.shape[1])


def plan_info(p):
    """the part of the plan Csr.plan_info() reports"""
    return {k: p[k] for k in PLAN_INFO_KEYS}


def lanes_of(p):
    """lanes per row of the lanes order: `while (lanes < 64 && lanes < mean) lanes <<= 1` from 4"""
    mean = p["nnz"] / p["rows"] if p["rows"] else 1.0
    lanes = 4
    while lanes < 64 and lanes < mean:
        lanes <<= 1
    return lanes


def gather_width(mean_len, max_row_len):
    """gathers per step of the slice kernel's row walk"""
    return 4 if mean_len <= 4.5 else (7 if mean_len <= 7.5 and max_row_len <= 14 else 8)


def gather_width_of(p):
    return gather_width(p["nnz"] / p["rows"] if p["rows"] else 1.0, p["max_row_len"])


def pairs_needed(lo, hi):
    """sixteen-byte pairs the slice [lo, hi) of a row block takes once it starts at the even index lo & ~1"""
    return (hi - (lo & ~1) + 1) >> 1


def pipe_admitted(p, bound=PIPE_PAIRS * 2 - 1):
    """the guard of variant 6 in mgs_launch_csr_op_range; bound: 2047 (2048 before the fix — kept for the CPU test's arithmetic)"""
    return p["max_block_nnz"] <= bound and p["max_block_nnz"] == p["lds_cap"]


def kernel(p, variant, coded=False):
    """the kernel that serves the whole launch: slice, rowblock (variants 2–4), pipe, wave, coded"""
    if variant == 6 and pipe_admitted(p):
        return "pipe"
    if variant == 7 and p["max_wave_nnz"] <= WAVE_CAP:
        return "wave"
    if variant == 0 and coded:
        return "coded"
    return "rowblock" if variant in (2, 3, 4) else "slice"


def arm(p, block, variant, coded=False):
    """the arm row block `block` takes: staged, sequential, lanes(L), pipe, wave"""
    k = kernel(p, variant, coded)
    if k in ("pipe", "wave"):
        return k
    cap = -1 if variant == 1 else p["lds_cap"]
    if int(p["block_nnz"][block]) <= cap:
        return "staged"
    if k == "coded" or (k == "slice" and p["max_row_len"] <= 64):
        return "sequential"
    return f"lanes({lanes_of(p)})"       # variants 2–4 have no sequential walk: every over-budget block, whatever its rows


# ---- the two summation orders ----
def _products(col, val, x, dtype):
    return np.asarray(val, dtype=dtype) * np.asarray(x, dtype=dtype)[np.asarray(col, dtype=np.int64)]


def row_sums_sequential(rowptr, col, val, x, dtype=np.float64):
    """s = +0.0, then s += val[k]·x[col[k]] in storage order; vectorised over the rows by entry position"""
    rp = np.asarray(rowptr, dtype=np.int64); n = len(rp) - 1
    p = _products(col, val, x, dtype)
    lens = np.diff(rp)
    s = np.zeros(n, dtype=dtype)
    for k in range(int(lens.max()) if n else 0):
        rows = np.flatnonzero(lens > k)
        s[rows] = s[rows] + p[rp[rows] + k]
    return s


def row_sums_lanes(rowptr, col, val, x, L, offsets=None, dtype=np.float64):
    """lane l sums the entries a + l, a + l + L, … sequentially from +0.0; then s[l] += s[l + off] for off = L/2 … 1 (offsets: another
    order of the tree's steps — a planted defect); lane 0's value"""
    rp = np.asarray(rowptr, dtype=np.int64); n = len(rp) - 1
    p = _products(col, val, x, dtype)
    lens = np.diff(rp)
    S = np.zeros((n, L), dtype=dtype)
    lane = np.arange(L)
    for j in range((int(lens.max()) + L - 1) // L if n else 0):
        r, l = np.nonzero(lens[:, None] > j * L + lane[None, :])
        S[r, l] = S[r, l] + p[rp[r] + j * L + l]
    if offsets is None:
        offsets = [L >> q for q in range(1, L.bit_length())]
    for off in offsets:
        S[:, :L - off] = S[:, :L - off] + S[:, off:]     # every lane with a lane l + off < L (the others feed lane 0 in neither order)
    return S[:, 0].copy()


def row_sums(p, variant, rowptr, col, val, x, coded=False):
    """every row's sum in the order of the arm its row block takes"""
    s = row_sums_sequential(rowptr, col, val, x)
    arms = [arm(p, blk, variant, coded) for blk in range(p["nblocks"])]
    if any(a.startswith("lanes") for a in arms):
        sl = row_sums_lanes(rowptr, col, val, x, lanes_of(p))
        for blk, a in enumerate(arms):
            if a.startswith("lanes"):
                s[blk * RB:(blk + 1) * RB] = sl[blk * RB:(blk + 1) * RB]
    return s


OPS = ("spmv", "residual", "jacobi")


def apply(op, s, x=None, b=None, dinv=None, omega=None):
    """the epilogues exactly as the kernels write them"""
    n = len(s)
    if op == "spmv":
        return s
    if op == "residual":
        return b[:n] - s
    return x[:n] + (omega * dinv[:n]) * (b[:n] - s)


# ---- exact values and the bar ----
def exact(op, rowptr, col, val, x, b=None, dinv=None, omega=None):
    """the operation in long double from the same FP64 inputs, and S_i = Σ|val·x| (long double)"""
    LD = np.longdouble
    rp = np.asarray(rowptr, dtype=np.int64); n = len(rp) - 1
    p = _products(col, val, x, LD)
    rowid = np.repeat(np.arange(n), np.diff(rp))
    s = np.zeros(n, dtype=LD); S = np.zeros(n, dtype=LD)
    np.add.at(s, rowid, p); np.add.at(S, rowid, np.abs(p))
    if op == "spmv":
        return s, S
    r = np.asarray(b, dtype=LD)[:n] - s
    if op == "residual":
        return r, S
    return np.asarray(x, dtype=LD)[:n] + (LD(omega) * np.asarray(dinv, dtype=LD)[:n]) * r, S


def bar(op, rowptr, col, val, x, b=None, dinv=None, omega=None):
    """the derived per-row bar of the module docstring (long double)"""
    LD = np.longdouble
    rp = np.asarray(rowptr, dtype=np.int64); n = len(rp) - 1
    m = (np.diff(rp) + 1).astype(LD) * LD(U)
    s, S = exact("spmv", rowptr, col, val, x)
    bs = m / (1 - m) * S
    if op == "spmv":
        return bs
    r = np.asarray(b, dtype=LD)[:n] - s
    br = bs + LD(U) * np.abs(r)
    if op == "residual":
        return br
    w = LD(omega) * np.asarray(dinv, dtype=LD)[:n]
    return np.abs(w) * br + 2 * LD(U) * np.abs(w * r) + LD(U) * np.abs(np.asarray(x, dtype=LD)[:n] + w * r)


def ratios(xhat, xref, bar_):
    """|x̂ − x| / bar per row; a row passes at ≤ 1; a zero bar passes only a zero error"""
    err = np.abs(np.asarray(xhat, dtype=np.longdouble) - xref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bar_ > 0, err / np.where(bar_ > 0, bar_, 1), np.where(err == 0, 0.0, np.inf))
    return np.asarray(q, dtype=np.float64)


# ---- the pattern code of mgs_csr_optimize: which row blocks it codes (rowcode_assign_kernel) ----
def coded_blocks(rowptr, col, n_rows):
    """row blocks whose table — one word per distinct (length, col − row) tuple plus the tuples — fits half the block's entries less 64"""
    rp = np.asarray(rowptr, dtype=np.int64); col = np.asarray(col, dtype=np.int64)
    count = 0
    for blk in range(row_blocks(n_rows)):
        r0, r1 = blk * RB, min(blk * RB + RB, n_rows)
        pats = {tuple(col[rp[r]:rp[r + 1]] - r) for r in range(r0, r1)}
        ints = len(pats) + sum(map(len, pats))
        if 0 < ints <= (rp[r1] - rp[r0]) // 2 - 64:
            count += 1
    return count


def code_usable(p, ncoded):
    """use_rowcode: at least half of the row blocks coded and no row longer than 64"""
    return ncoded > 0 and p["max_row_len"] <= 64 and ncoded >= 0.5 * p["nblocks"]


# ---- case builders: scipy CSR with sorted indices, values from ±[0.5, 2] ----
def banded(lengths, n_cols, rng, pattern="random", reserve=0):
    """row i holds lengths[i] entries at c0_i + j·step_i.  random: c0 and step ∈ {1, 2, 3} drawn per row; stencil: step 1 around the
    diagonal, so rows of one length repeat their shape (what the pattern code needs).  reserve: trailing columns left unreferenced"""
    lengths = np.asarray(lengths, dtype=np.int64); n = len(lengths); w = n_cols - reserve
    assert int(lengths.max(initial=0)) <= w
    rp = np.r_[0, np.cumsum(lengths)].astype(np.int64)
    rows = np.repeat(np.arange(n), lengths); pos = np.arange(rp[-1]) - rp[rows]
    if pattern == "stencil":
        step = np.ones(n, dtype=np.int64)
        c0 = np.clip(np.arange(n) - lengths // 2, 0, w - lengths)
    else:
        step = np.maximum(1, np.minimum(rng.integers(1, 4, n), (w - 1) // np.maximum(lengths - 1, 1)))
        c0 = (rng.random(n) * (w - (lengths - 1).clip(0) * step)).astype(np.int64)
    colv = c0[rows] + pos * step[rows]
    M = sps.csr_matrix((signed(rng, int(rp[-1])), colv.astype(np.int32), rp.astype(np.int32)), shape=(n, n_cols))
    M.has_sorted_indices = True
    return M


def with_entries(M, rows, cols, rng):
    """M with one more entry per (row, col) — columns M leaves unreferenced, behind each row's last column"""
    E = sps.csr_matrix((signed(rng, len(rows)), (np.asarray(rows), np.asarray(cols))), shape=M.shape)
    assert not (M.multiply(E)).nnz
    R = (M + E).tocsr(); R.sort_indices()
    return R


def vectors(M, seed):
    """x (columns), b, dinv (rows of max(shape): Jacobi reads x[row]) from ±[0.5, 2], and ω"""
    rng = np.random.default_rng(seed)
    k = max(M.shape)
    return signed(rng, k), signed(rng, k), signed(rng, k), 0.7


def edge_case(n, pattern="random"):
    """row counts around the block size: lengths cycle through 3, 0, 1, 5, 2, 8, 4 (cut at n columns)"""
    rng = np.random.default_rng(1000 + n)
    lengths = np.minimum(np.array([3, 0, 1, 5, 2, 8, 4])[np.arange(n) % 7], n)
    return banded(lengths, n, rng, pattern)


def wide_case():
    """600 × 700: the columns from 600 on are halo columns in the plan's eyes; row block 0 references none, row blocks 1 and 2 do"""
    rng = np.random.default_rng(1700)
    lengths = np.array([3, 0, 1, 5, 2, 8, 4])[np.arange(600) % 7]
    top = banded(lengths[:RB], 700, rng, reserve=100)
    low = banded(lengths[RB:], 700, rng)
    M = sps.vstack([top, low], format="csr"); M.sort_indices()
    return M


def empty_rows_case(n=300):
    """rows without a single entry"""
    return sps.csr_matrix((n, n))


GATHER_CYCLE = {4: (0, 1, 3, 4, 5, 8, 9), 7: (0, 1, 6, 7, 8, 14), 8: (0, 1, 7, 8, 9, 16, 17)}     # 0, 1, U − 1, U, U + 1, 2U(, 2U + 1: U = 7 must stay ≤ 14)
GATHER_N = 600
LONELY_ROWS = (15, 260)       # rows of length 1 that get one of the two columns nobody else references (columns n − 2, n − 1)


def gather_case(u, long_row=False, pattern="stencil"):
    """600 rows whose mean length puts the gather width at u, lengths cycling through GATHER_CYCLE[u]; the second row block starts at an
    odd entry index (its staged slice begins with the first block's last entry); the last row's length u + 1 is no multiple of u; columns
    n − 2 and n − 1 are referenced by exactly one row each (the poisoned x entries).  long_row: a row of 15 entries (u = 7 → width 8)"""
    rng = np.random.default_rng(2000 + u + 100 * long_row)
    n = GATHER_N
    cyc = np.array(GATHER_CYCLE[u])
    lengths = cyc[np.arange(n) % len(cyc)].copy()
    for r in LONELY_ROWS:
        lengths[r] = 1
    lengths[LONELY_ROWS[0] - 2] = cyc[-1]; lengths[LONELY_ROWS[0] - 1] = 0       # the row two above pads its last step with the lonely entry
    lengths[LONELY_ROWS[1] - 2] = cyc[-1]; lengths[LONELY_ROWS[1] - 1] = 0
    lengths[n - 1] = u + 1
    if long_row:
        lengths[530] = 15
    if (int(lengths[:RB].sum()) + 1) % 2 == 0:                                   # + 1: the lonely entry of row 15
        lengths[0] = 1 - lengths[0] if lengths[0] in (0, 1) else lengths[0] + 1
    M = banded(lengths, n, rng, pattern, reserve=2)
    M = with_entries(M, LONELY_ROWS, (n - 2, n - 1), rng)
    assert M.indptr[RB] % 2 == 1
    return M


def signed_zero_case():
    """the u = 8 gather matrix with −0.0 among its values, and x such that some rows' products are all −0.0"""
    M = gather_case(8).copy()
    x, b, dinv, omega = vectors(M, 77)
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    x[::11] = -0.0
    x[5::13] = 0.0
    M.data[3::17] = -0.0
    allneg = (rows % 5 == 2)
    M.data[allneg] = np.copysign(0.0, -np.copysign(1.0, x[M.indices[allneg]]))      # (−0)·(+x), (+0)·(−x): every product −0.0
    return M, (x, b, dinv, omega), np.unique(rows[allneg])


BUDGET_BLOCKS = 68
BUDGET_HEAVY = 34


def budget_case(heavy=40, long_row=0, pattern="stencil", base=3):
    """68 row blocks of `base` entries per row, row block 34 with `heavy` per row (0: none heavier), long_row: one row of that many entries
    inside it"""
    rng = np.random.default_rng(3000 + heavy + long_row)
    n = BUDGET_BLOCKS * RB
    lengths = np.full(n, base, dtype=np.int64)
    if heavy:
        lengths[BUDGET_HEAVY * RB:(BUDGET_HEAVY + 1) * RB] = heavy
    if long_row:
        lengths[BUDGET_HEAVY * RB + 77] = long_row
    return banded(lengths, n, rng, pattern)


def over_cap_case(long_row=0):
    """512 rows: five entries per row in block 0, twenty-one in block 1 (5376 > 5120); long_row: one row of block 1 that long"""
    rng = np.random.default_rng(4000 + long_row)
    lengths = np.r_[np.full(RB, 5), np.full(RB, 21)]
    if long_row:
        lengths[RB + 100] = long_row
    return banded(lengths, 512, rng)


LANES_MEAN = {4: 3, 8: 6, 16: 12, 32: 24, 64: 40}


def lanes_case(L, long_row=True):
    """600 rows (two full row blocks and one of 88) of mean length LANES_MEAN[L]; the lengths 0, 1, L − 1, L, L + 1, 3L + 2 and one row of
    70 entries sit in the first block and again in the last, partial one.  long_row=False: no row longer than 64 (L = 4 only)"""
    rng = np.random.default_rng(5000 + L + 100 * long_row)
    n = 600
    t = LANES_MEAN[L]
    lengths = t + (np.arange(n) % 3 - 1)
    special = [0, 1, L - 1, L, L + 1, 3 * L + 2, 70 if long_row else 14]
    assert long_row or max(special) <= 64
    for base in (9, 2 * RB + 31):
        lengths[base:base + 2 * len(special):2] = special
    return banded(lengths, n, rng)


def chunk_case(r):
    """4·256 + 88 rows: the row blocks 1, 2, 3 start at entry indices ≡ 1, 2, 3 (mod 4) and the matrix ends at an index ≡ r (mod 4): the
    widened 16-byte loads of variants 3 and 4 reach before a block's first and behind the matrix's last entry"""
    rng = np.random.default_rng(6000 + r)
    n = 4 * RB + 88
    lengths = rng.integers(0, 10, n)
    for blk in range(3):                                  # blocks 0, 1, 2 hold ≡ 1 (mod 4) entries each
        rows = slice(blk * RB, (blk + 1) * RB)
        lengths[(blk + 1) * RB - 1] += (1 - int(lengths[rows].sum())) % 4
    lengths[n - 1] += (r - int(lengths.sum())) % 4
    M = banded(lengths, n, rng)
    assert [int(M.indptr[k * RB]) % 4 for k in range(4)] == [0, 1, 2, 3] and M.nnz % 4 == r
    return M


def wave_case(n):
    """rows 128–191 (the third 64-row group of row block 0) without entries where n reaches them"""
    rng = np.random.default_rng(7000 + n)
    lengths = np.array([3, 0, 1, 5, 2, 8, 4, 11])[np.arange(n) % 8]
    lengths[128:192] = 0
    return banded(lengths, n, rng)


def wave_over_case():
    """one 64-row group of 65 entries per row: max_wave_nnz = 4160 > 4096, the row block still within the staging budget"""
    rng = np.random.default_rng(7999)
    lengths = np.full(RB, 2); lengths[64:128] = 65
    return banded(lengths, 300, rng)


def pipe_case(n):
    """five entries per row on average; n = 200, 1024, 1100, 1900: 1, 4, 5 (a last super block of one partial block) and 8 row blocks"""
    rng = np.random.default_rng(8000 + n)
    return banded(np.array([5, 3, 7, 0, 9, 6])[np.arange(n) % 6], n, rng)


def pipe_boundary_case(cnt, lo_odd):
    """two row blocks: block 1 holds exactly cnt entries (2047 or 2048) from an entry index lo of the given parity; block 0 is lighter"""
    rng = np.random.default_rng(9000 + cnt + lo_odd)
    l0 = np.full(RB, 5); l0[0] += int(lo_odd)
    l1 = np.full(RB, cnt // RB); l1[:cnt % RB] += 1
    M = banded(np.r_[l0, l1], 2 * RB, rng)
    assert M.indptr[RB] % 2 == int(lo_odd) and M.indptr[2 * RB] - M.indptr[RB] == cnt
    return M
