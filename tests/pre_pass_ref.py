"""Host restatement of the cycle's fused pre pass (mgs_hier_pre_pass_info), its derived per-row and per-aggregate error bars, and the helpers
the CPU and GPU tests of that pass share.  Vectors, stencils and aggregate generators come from post_pass_ref.

The pass.  For a level with operator A (CSR, stored order), aggregate map agg (−1: the row lies outside every aggregate), ω and a right-hand
side b, with d_k = fl(ω·fl(1/a_kk)) (post_pass_ref.dvec):
    Â_ik = fl(a_ik·d_k)                          (scale_vals_kernel: one product per stored entry; k_axpby with b = 0 makes d)
    s_i  = Σ_k Â_ik·b_k                          form "hat": the residual kernels, the aggregate-parallel and the grouped kernel
    s_i  = Σ_k a_ik·fl(d_k·b_k)                  form "wd":  the gather form on A itself (FUSE_PRE of csr_rowblock_fused_kernel)
    r_i  = fl(b_i − s_i),   t_i = fl(b_i + r_i)
    r_c[a] = Σ_{j ∈ members(a)} r_j              members in ascending row order
An FP32 level reads float32(Â_ik) (round to nearest, k_round_vals), widened to FP64 before the product.

Two evaluations.  (a) `evaluate(..., np.float64)`: the kernels' own association.  s starts at +0.0 and takes the products one by one in stored
order, one rounding per product and per sum, no FMA (the library is built with -ffp-contract=off; numpy never contracts); the padded gather
steps of the row-block kernels add +0.0, which changes no bit of a sum that started at +0.0.  r_c starts at 0.0 and takes the members'
residuals in ascending member order (restrict_agg_kernel, the in-LDS restriction of the grouped kernels, restrict_stray_kernel, lane 0 of
agg_pre_kernel).  Where the order is a promise — no row of the level longer than 64 — (a) is what the device must return BIT FOR BIT, in
every arm.  (b) `evaluate(..., np.longdouble)`: the same formula from the same FP64 (or FP32) operand values Â (form "wd": from a and d) in
64-bit-mantissa arithmetic; its own error is 2⁻¹¹ of the bars below and is ignored.

The bars, derived (u = 2⁻⁵³; m_i = stored length of row i, plus 1 for form "wd" whose products carry two roundings; S_i = Σ_k |Â_ik|·|b_k|, for
form "wd" Σ_k |a_ik|·|d_k|·|b_k|).  Standard model fl(x ∘ y) = (x ∘ y)(1 + δ), |δ| ≤ u, no underflow (every input lies in [0.5, 2] in
magnitude).  The operand values are inputs: Â is compared as stored, so its own rounding is not part of the error.
  * ŝ_i: each product carries one δ (two for "wd": d·b, then a·(d·b)) and at most m_i − 1 effective additions (the first, 0.0 + p, is exact):
    |ŝ_i − s_i| ≤ γ_{m_i}·S_i, with m_i as defined above, to first order m_i·u·S_i.
  * r̂_i = fl(b_i − ŝ_i): one more δ on |b_i| + S_i:   |r̂_i − r_i| ≤ (m_i + 1)·u·(|b_i| + S_i) to first order; one further u covers the
    second-order terms:                                  |r̂_i − r_i| ≤ (m_i + 2)·u·(|b_i| + S_i).
  * t̂_i = fl(b_i + r̂_i): |t_i| ≤ 2|b_i| + S_i; the error of r̂ passes through, the sum adds one δ on |b_i| + |r̂_i| ≤ 2(|b_i| + S_i), i.e.
    two more u on (|b_i| + S_i):                        |t̂_i − t_i| ≤ (m_i + 4)·u·(|b_i| + S_i).
  * r̂_c[a] over k_a members: the error of every r̂_j passes through, and r̂_j sits in at most k_a − 1 additions (k_a counted, which also
    covers the second order), each a δ on a partial sum bounded by the members' Σ(|b_j| + S_j):
                                                         |r̂_c[a] − r_c[a]| ≤ Σ_j (m_j + 2 + k_a)·u·(|b_j| + S_j).
None of these depends on the order of a row's entries or of an aggregate's members, so they also serve rows longer than 64, where the
kernels split a row among lanes and promise no order.

Inputs.  Values and b come from ±[0.5, 2]: no term of a row is negligible beside the row's sum, so a dropped term, a b of the wrong row or a
member of the wrong aggregate moves the result by ≥ 0.25·0.3 — thirteen orders of magnitude above the bars."""
import numpy as np
import scipy.sparse as sps

import post_pass_ref as R
from post_pass_ref import Guarded, SENT, U, agg_P, randomize, random_aggregates, renumber, signed  # noqa: F401  (shared with the tests)


def hat_values(A, omega, f32=False):
    """Â's stored values fl(a_ik·d_k) in A's stored order (FP32 level: rounded to float, kept as float32)"""
    A = A.tocsr()
    v = A.data * R.dvec(A, omega)[A.indices]
    return v.astype(np.float32) if f32 else v


def hat_matrix(A, omega):
    A = A.tocsr()
    return sps.csr_matrix((hat_values(A, omega), A.indices.copy(), A.indptr.copy()), shape=A.shape)


def members_of(agg, nc):
    """member lists in ascending row order: (cptr, members)"""
    agg = np.asarray(agg)
    rows = np.flatnonzero(agg >= 0)
    order = np.argsort(agg[rows], kind="stable")
    cptr = np.zeros(nc + 1, dtype=np.int64)
    np.add.at(cptr, agg[rows] + 1, 1)
    return np.cumsum(cptr), rows[order]


def renumber_by_first_member(agg):
    """aggregate ids ascending with their first (lowest) member — the numbering the device matching produces and the only one under which
    row-block groups form (grp_scan_kernel)"""
    agg = np.asarray(agg).copy()
    ok = agg >= 0
    ids, first = np.unique(agg[ok], return_index=True)          # first occurrence in ascending row order
    new = np.empty(int(ids.max()) + 1 if len(ids) else 0, dtype=np.int64)
    new[ids[np.argsort(first, kind="stable")]] = np.arange(len(ids))
    agg[ok] = new[agg[ok]]
    return agg.astype(np.int32)


def _products(A, omega, b, dtype, form, f32):
    """per stored entry: the product the kernels add, and |value|·|b| in long double"""
    A = A.tocsr(); T = dtype; L = np.longdouble
    bb = np.asarray(b, dtype=np.float64)
    if form == "hat":
        v = hat_values(A, omega, f32)
        p = v.astype(T) * bb.astype(T)[A.indices]
        mag = np.abs(v.astype(L)) * np.abs(bb.astype(L))[A.indices]
    elif form == "wd":
        assert not f32, "the gather form reads A's FP64 values"
        d = R.dvec(A, omega)
        p = A.data.astype(T) * (d.astype(T) * bb.astype(T))[A.indices]
        mag = np.abs(A.data.astype(L)) * (np.abs(d.astype(L)) * np.abs(bb.astype(L)))[A.indices]
    else:
        raise ValueError(form)
    return p, mag


def row_sums(rowptr, p, dtype, reverse=False, skip=None):
    """s_i from +0.0 in stored order (reverse: last entry first), vectorised by entry position within the row"""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = len(rowptr) - 1
    ln = np.diff(rowptr)
    if skip is not None:
        p = p.copy(); p[np.asarray(skip)] = 0
    s = np.zeros(n, dtype=dtype)
    for k in range(int(ln.max()) if n else 0):
        rows = np.flatnonzero(ln > k)
        e = rowptr[rows + 1] - 1 - k if reverse else rowptr[rows] + k
        s[rows] = s[rows] + p[e]
    return s


def restrict(r, agg, nc, dtype, reverse=False):
    """r_c[a] from 0.0 over the members in ascending order (reverse: descending), vectorised by member position"""
    cptr, mem = members_of(agg, nc)
    cnt = np.diff(cptr)
    rc = np.zeros(nc, dtype=dtype)
    r = np.asarray(r, dtype=dtype)
    for k in range(int(cnt.max()) if nc else 0):
        a = np.flatnonzero(cnt > k)
        m = mem[cptr[a + 1] - 1 - k] if reverse else mem[cptr[a] + k]
        rc[a] = rc[a] + r[m]
    return rc


def evaluate(A, omega, agg, nc, b, dtype=np.float64, form="hat", f32=False, reverse=False, skip=None, bdiag=None):
    """(t, r, r_c) of the pre pass in `dtype` with the kernels' association.  Mutations for the CPU test: reverse (entries of every row visited
    last to first), skip (stored entries left out), bdiag (the b the rows subtract from and add to, instead of their own)."""
    A = A.tocsr()
    p, _ = _products(A, omega, b, dtype, form, f32)
    s = row_sums(A.indptr, p, dtype, reverse, skip)
    bi = np.asarray(b if bdiag is None else bdiag, dtype=dtype)
    r = bi - s
    t = bi + r
    return t, r, restrict(r, agg, nc, dtype)


def bars(A, omega, agg, nc, b, form="hat", f32=False):
    """(bar_t, bar_r, bar_rc) of the module docstring, long double"""
    A = A.tocsr(); L = np.longdouble
    _, mag = _products(A, omega, b, L, form, f32)
    n = A.shape[0]
    S = np.zeros(n, dtype=L)
    np.add.at(S, np.repeat(np.arange(n), np.diff(A.indptr)), mag)
    m = np.diff(A.indptr).astype(L) + (1 if form == "wd" else 0)
    w = np.abs(np.asarray(b, dtype=L)) + S
    agg = np.asarray(agg); ok = agg >= 0
    ka = np.bincount(agg[ok], minlength=nc).astype(L)
    brc = np.zeros(nc, dtype=L)
    np.add.at(brc, agg[ok], ((m[ok] + 2 + ka[agg[ok]]) * w[ok]))
    return (m + 4) * w * L(U), (m + 2) * w * L(U), brc * L(U)


def ratios(xhat, xref, bar_):
    """|x̂ − x| / bar; passes at ≤ 1 (an empty aggregate list cannot occur: every id below nc has a member)"""
    return np.asarray(np.abs(np.asarray(xhat, dtype=np.longdouble) - xref) / bar_, dtype=np.float64)


def aggregates_1_to_9(n, rng, g0=0.05):
    """shuffled aggregates of 1–9 members (more than four: the second shuffle round of the aggregate-parallel kernel, the loop of the
    restriction kernel; more than six: strays of the grouped kernel by size) with a share of rows outside every aggregate"""
    return random_aggregates(n, rng, sizes=tuple(range(1, 10)), g0=g0)


def with_row_lengths(n, lengths, rng):
    """an operator whose row i holds lengths[i % len(lengths)] entries, the diagonal among them, the others at random columns"""
    rows, cols = [], []
    for i in range(n):
        k = min(lengths[i % len(lengths)], n) - 1
        c = rng.choice(n - 1, k, replace=False) if k > 0 else np.zeros(0, dtype=np.int64)
        c = c + (c >= i)                                         # skip the diagonal: randomize adds it
        rows.append(np.full(k, i)); cols.append(c)
    return sps.csr_matrix((np.ones(sum(map(len, rows))), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
