"""Option pre_nodiag (default 1): the grouped pre pass of an eligible level does not stream Â's diagonal entries as doubles.  Â = A·diag(ωD⁻¹)
holds fl(a_ii·fl(ω·fl(1/a_ii))) there — ω up to three roundings — and the kernel rebuilds that entry from ω and one byte per row (its distance
from ω in units of the last place), multiplies it with the b_i it already holds and adds the product in its place in the ascending-column
sum.  The rebuilt entry is the stored one, so every comparison below could ask for equal bits; the bars are the ones the issue set:
  * option on against off: ≤ 1e-13 relative in the 2-norm (the project's bar for two roundings of one cycle, tests/test_gpu_parity.py);
  * option on, one level in two forms (pattern code on/off, 512-thread pairs / sequential sweep, a second run, a refreshed hierarchy and
    its twin, a new ω and a hierarchy built with it): the same bits;
  * against the oracle's cycle on the downloaded hierarchy: ≤ 1e-10, the bar of every cycle test here;
  * FP32 operand levels and levels that do not qualify: the same bits as with the option off.
The pre pass alone (mgs_hier_pre_pass) is held to a host restatement: a row's sum has at most 11 terms of one sign pattern each bounded by
|Â||b|, so 1e-13 relative in the 2-norm leaves two orders of magnitude above 11·2⁻⁵³ ≈ 1.2e-15.  That host product does not have the kernel's
summation order, so the pass is ALSO held, bit for bit, to the exact restatement of tests/pre_pass_ref.py (every operator here has rows of at
most 64 entries, where the order is a promise): t, r_c and the written entries of r."""
import numpy as np
import pytest
import scipy.sparse as sps

import pre_pass_ref as Q

pytestmark = pytest.mark.gpu

SENT = -1.2345e30      # what the guard zones and the unwritten entries hold
GUARD = 64


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


DEFAULTS = (("pre_nodiag", 1), ("rowcode", 1), ("fuse_restrict", 1), ("group_stray_pct", 6), ("group_min_blocks", 1024), ("group_blocks", 4),
            ("group_concurrent", 0))


def restore(ctx):
    for k, v in DEFAULTS:
        ctx.set_option(k, v)


def small_levels_group(ctx, stray_pct=60):
    ctx.set_option("group_stray_pct", stray_pct); ctx.set_option("group_min_blocks", 1)


def oracle_cycle(orc, h, b_np, omega=0.6):
    """the oracle's cycle on the downloaded hierarchy (aggregation transfers)"""
    As, Ps = [], []
    for l in range(h.nlev):
        rp, ci, v = h.level_A(l).download(); r = h.level_shape(l)[0]
        As.append(orc.Csr.from_arrays(r, r, rp, ci, v))
        if l < h.nlev - 1:
            T = h.level_P(l); a = T.agg(); nf, nc = T.shape; rows = np.nonzero(a >= 0)[0]
            Ps.append(orc.Csr.from_scipy(sps.csr_matrix((np.ones(rows.size), (rows, a[rows])), shape=(nf, nc))))
    return orc.Hier(As[0], Ps, omega=omega, nu1=1, nu2=1, As=As).vcycle(b_np)


class Guarded:
    """a device vector of n entries with GUARD sentinels on either side"""
    def __init__(self, ctx, mg, n):
        self.n = n
        self.buf = ctx.vec(np.full(n + 2 * GUARD, SENT))
        self.v = mg.Vec.wrap(ctx, self.buf.ptr + 8 * GUARD, n)

    def check(self, what):
        a = self.buf.numpy()
        assert np.all(a[:GUARD] == SENT) and np.all(a[GUARD + self.n:] == SENT), what
        return a[GUARD:GUARD + self.n]


def pre_pass_against_host(ctx, mg, h, b, omega, want_nodiag):
    """level 0's grouped pre pass alone, into guarded vectors, against t = b + r, r = b − Â·b, r_c = Pᵀr computed on the host"""
    rp, ci, v = h.level_A(0).download(); n = h.level_shape(0)[0]; nc = h.level_shape(1)[0]
    A = sps.csr_matrix((v, ci, rp), shape=(n, n))
    b_np = b.numpy()
    r_ref = b_np - (A @ sps.diags(omega * (1.0 / A.diagonal()))) @ b_np
    g = h.level_P(0).agg(); ok = g >= 0
    rc_ref = np.bincount(g[ok], weights=r_ref[ok], minlength=nc)
    t, r, rc = Guarded(ctx, mg, n), Guarded(ctx, mg, n), Guarded(ctx, mg, nc)
    assert h.pre_pass(0, b, t.v, r.v, rc.v) == want_nodiag
    t_np, r_np, rc_np = t.check("t"), r.check("r"), rc.check("r_c")
    assert rel(t_np, b_np + r_ref) <= 1e-13 and rel(rc_np, rc_ref) <= 1e-13, (rel(t_np, b_np + r_ref), rel(rc_np, rc_ref))
    w = r_np != SENT                                       # r: the rows of stray aggregates only
    assert np.linalg.norm(r_np[w] - r_ref[w]) <= 1e-13 * np.linalg.norm(r_ref)
    # the exact restatement: the kernel's own order, equal bits
    assert np.diff(rp).max() <= 64
    t_x, r_x, rc_x = Q.evaluate(A, omega, g, nc, b_np, np.float64, "hat")
    assert np.array_equal(t_np, t_x), ("t: bits", np.flatnonzero(t_np != t_x)[:8])
    assert np.array_equal(rc_np, rc_x), ("r_c: bits", np.flatnonzero(rc_np != rc_x)[:8])
    assert np.array_equal(r_np[w], r_x[w]), ("r: bits", np.flatnonzero(w)[r_np[w] != r_x[w]][:8])
    return t_np, rc_np


def compare_all(ctx, mg, orc, A, stray_pct=60):
    """what the module's docstring lists, for one operator"""
    n = A.shape[0]
    try:
        small_levels_group(ctx, stray_pct)
        h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 200, 32).finalize()
        b = ctx.vec(n).rand(seed=3)
        x = Guarded(ctx, mg, n)
        h.vcycle(b, x.v); x1 = x.check("x").copy()
        info = h.group_info(0)
        assert info["groups"] > 0, info                                        # level 0 ran grouped ...
        t1, rc1 = pre_pass_against_host(ctx, mg, h, b, 0.6, True)             # ... and without Â's diagonal
        assert np.array_equal(h.vcycle(b).numpy(), x1)                         # a second run
        ctx.set_option("rowcode", 0); xp = h.vcycle(b).numpy(); tp, rcp = pre_pass_against_host(ctx, mg, h, b, 0.6, True); ctx.set_option("rowcode", 1)
        assert np.array_equal(xp, x1) and np.array_equal(tp, t1) and np.array_equal(rcp, rc1)      # index slices instead of the pattern code
        ctx.set_option("pre_nodiag", 0); x0 = h.vcycle(b).numpy(); t0, rc0 = pre_pass_against_host(ctx, mg, h, b, 0.6, False); ctx.set_option("pre_nodiag", 1)
        print(f"n={n} groups={info['groups']} strays={info['stray_aggregates']}: on vs off {rel(x1, x0):.3e}")
        assert rel(x1, x0) <= 1e-13, rel(x1, x0)
        assert np.array_equal(x1, x0) and np.array_equal(t1, t0) and np.array_equal(rc1, rc0)      # the rebuilt diagonal entry is the stored one
        assert np.array_equal(h.vcycle(b).numpy(), x1)                         # back on: the compact operand is still in step
        e = rel(x1, oracle_cycle(orc, h, b.numpy()))
        print(f"  vs oracle {e:.3e}")
        assert e <= 1e-10, e
        # pairs of row blocks: the 512-thread form against the sequential sweep over the same pairs (groups are built once per hierarchy)
        ctx.set_option("group_blocks", 2); ctx.set_option("group_concurrent", 1)
        h2 = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 200, 32).finalize()
        x2 = h2.vcycle(b).numpy(); t2, rc2 = pre_pass_against_host(ctx, mg, h2, b, 0.6, True)
        assert h2.group_info(0)["groups"] > 0 and rel(x2, x1) <= 1e-13, (rel(x2, x1), h2.group_info(0))
        ctx.set_option("group_concurrent", 0)
        assert np.array_equal(h2.vcycle(b).numpy(), x2)
        t3, rc3 = pre_pass_against_host(ctx, mg, h2, b, 0.6, True)
        assert np.array_equal(t3, t2) and np.array_equal(rc3, rc2)
    finally:
        restore(ctx)


@pytest.mark.parametrize("kind", ["poisson3d_33", "poisson3d_64", "poisson2d_130", "CSky3d30", "CSky2d100", "random_graph"])
def test_option_on_against_off(ctx, mg, orc, inputs, kind):
    """a. ragged last block and x-lines off the 256-row grid (33³), a plain grid (64³), 2-D rows of 3–5 entries, the bundled nonsymmetric
    variable-coefficient operators, and a random graph's shifted Laplacian (uncoded blocks, many strays)"""
    if kind.startswith("poisson3d"):
        A = ctx.poisson3d(int(kind.split("_")[1]))
    elif kind.startswith("poisson2d"):
        A = ctx.poisson2d(int(kind.split("_")[1]))
    elif kind == "random_graph":
        rng = np.random.default_rng(12)
        m = 30000
        i = np.concatenate([np.arange(m - 1), rng.integers(0, m, 2 * m), rng.integers(0, m, m // 20)])
        j = np.concatenate([np.arange(1, m), np.clip(i[m - 1:3 * m - 1] + rng.integers(-40, 41, 2 * m), 0, m - 1), rng.integers(0, m, m // 20)])
        keep = i != j
        W = sps.coo_matrix((rng.uniform(0.5, 1.5, keep.sum()), (i[keep], j[keep])), shape=(m, m)).tocsr()
        W = W + W.T
        M = (sps.diags(np.asarray(W.sum(axis=1)).ravel() + 0.02) - W).tocsr(); M.sort_indices()
        A = ctx.csr(m, m, M.indptr, M.indices, M.data)
    else:
        A = mg.Csr.from_mtx(ctx, inputs[kind])
    compare_all(ctx, mg, orc, A, 100 if kind == "random_graph" else 60)


def banded700():
    """n = 700: three row blocks, the last partial.  Row 0 holds its diagonal only (compact length 0); the diagonal comes first in rows 1–99,
    last in rows 100–199 and 400–698 (even), in the middle elsewhere; rows 300–399 hold 9–11 entries with the diagonal at position 8 or 9,
    i.e. behind the first gather step of every unroll factor (4, 7, 8).  Off-diagonals negative, rows strictly diagonally dominant."""
    n = 700
    rng = np.random.default_rng(7)
    rows, cols = [], []
    for i in range(n):
        if i == 0:
            offs = []
        elif i < 100:
            offs = [1, 2]
        elif i < 200:
            offs = [-2, -1]
        elif i < 300:
            offs = [-1, 1] + ([5] if i % 3 == 0 else [])
        elif i < 400:
            offs = list(range(-8, 0)) if i % 3 == 0 else (list(range(-8, 0)) + [1] if i % 3 == 1 else list(range(-9, 0)) + [1])
        else:
            offs = [-1] if i % 2 == 0 else [-3, -1, 1, 3]
        for o in offs:
            if 0 <= i + o < n:
                rows.append(i); cols.append(i + o)
    off = sps.coo_matrix((-(1.0 + 0.3 * rng.random(len(rows))), (rows, cols)), shape=(n, n)).tocsr()
    M = (off + sps.diags(-np.asarray(off.sum(axis=1)).ravel() + 0.5 + rng.random(n))).tocsr()
    M.sort_indices()
    lens = np.diff(M.indptr)
    assert lens[0] == 1 and lens[1:].min() == 2 and lens.max() == 11 and set(lens[300:400]) == {9, 10, 11}
    return M


def test_diagonal_at_the_edges_of_rows_and_slices(ctx, mg, orc):
    """b. the compact operand's index arithmetic where it can go wrong: an empty compact row at the start of a slice, the diagonal first / last
    in a row, the diagonal in a later gather step, a partial last block; guard zones around t, r_c and x stay untouched"""
    M = banded700()
    A = ctx.csr(700, 700, M.indptr, M.indices, M.data)
    compare_all(ctx, mg, orc, A, 100)


def test_level_with_a_general_P_keeps_its_path(ctx, mg, orc):
    """c. a two-level hierarchy whose P is no aggregation (rows of two entries): no row-block groups, the option changes no bit"""
    N = 40; n = N * N; nc = n // 2
    A = ctx.poisson2d(N)
    i = np.arange(n)
    P = sps.coo_matrix((np.r_[np.ones(n), np.full(n, 0.25)], (np.r_[i, i], np.r_[i // 2, np.minimum(i // 2 + 1, nc - 1)])), shape=(n, nc)).tocsr()
    P.sort_indices()
    try:
        small_levels_group(ctx)
        h = mg.Hierarchy(A, 0.6, 1, 1)
        h.push_P(ctx.csr(n, nc, P.indptr, P.indices, P.data)); h.finalize()
        assert h.nlev == 2 and not h.level_P(0).is_aggregation
        b = ctx.vec(n).rand(seed=5)
        x1 = h.vcycle(b).numpy()
        assert h.group_info(0)["groups"] == 0
        ctx.set_option("pre_nodiag", 0); x0 = h.vcycle(b).numpy(); ctx.set_option("pre_nodiag", 1)
        assert np.array_equal(x1, x0)
        As = []
        for l in range(2):
            rp, ci, v = h.level_A(l).download(); r = h.level_shape(l)[0]
            As.append(orc.Csr.from_arrays(r, r, rp, ci, v))
        ho = orc.Hier(As[0], [orc.Csr.from_scipy(P)], omega=0.6, nu1=1, nu2=1, As=As)
        e = rel(x1, ho.vcycle(b.numpy()))
        print(f"general P vs oracle {e:.3e}")
        assert e <= 1e-10, e
    finally:
        restore(ctx)


def agg_P(g, nc):
    ok = g >= 0
    return sps.csr_matrix((np.ones(int(ok.sum())), (np.flatnonzero(ok), g[ok])), shape=(len(g), nc))


@pytest.mark.parametrize("npass", [1, 2])
def test_refresh_keeps_the_compact_operand_in_step(ctx, mg, npass):
    """d. new values on the same pattern + mgs_hier_refresh against a twin built from scratch on the new values with the same aggregates.
    npass = 1: the same bits.  npass = 2: the twin's Galerkin operators are chained products of pushed 0/1 transfers (DESIGN.md §4's caveat),
    so 1e-13."""
    N = 40; n = N ** 3
    rp, ci, v = ctx.poisson3d(N).download()
    rng = np.random.default_rng(3)
    s = 1.0 + 0.2 * rng.random(n)
    v2 = v * s[np.repeat(np.arange(n), np.diff(rp))] * s[ci] * 1.25        # a symmetric rescaling: every value moves, diagonals differ row to row
    try:
        small_levels_group(ctx)
        A = ctx.csr(n, n, rp, ci, v)
        h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, npass, 8.0, 200, 32).finalize()
        b = ctx.vec(n).rand(seed=11)
        x_old = h.vcycle(b).numpy()
        assert h.group_info(0)["groups"] > 0
        A.update_values(v2); h.refresh()
        x = h.vcycle(b).numpy()
        assert not np.array_equal(x, x_old)
        A2 = ctx.csr(n, n, rp, ci, v2)
        h2 = mg.Hierarchy(A2, 0.6, 1, 1)
        for l in range(h.nlev - 1):
            P = agg_P(h.level_P(l).agg(), h.level_shape(l + 1)[0])
            h2.push_P(ctx.csr(P.shape[0], P.shape[1], P.indptr, P.indices, P.data))
        h2.finalize()
        x2 = h2.vcycle(b).numpy()
        assert h2.group_info(0)["groups"] > 0
        t, r, rc = ctx.vec(n), ctx.vec(n), ctx.vec(h.level_shape(1)[0])
        assert h.pre_pass(0, b, t, r, rc) and h2.pre_pass(0, b, t, r, rc)
        print(f"npass={npass}: refreshed vs twin {rel(x, x2):.3e}")
        if npass == 1:
            assert np.array_equal(x, x2), rel(x, x2)
        else:
            assert rel(x, x2) <= 1e-13, rel(x, x2)
    finally:
        restore(ctx)


def test_new_omega_rescales_the_compact_operand(ctx, mg):
    """d. set_smoother(0.8) on a hierarchy that has run at ω = 0.6 against one built at 0.8: the same bits (a stale val_nd, or bytes counted from 0.6, would show)"""
    N = 40; n = N ** 3
    try:
        small_levels_group(ctx)
        A = ctx.poisson3d(N)
        b = ctx.vec(n).rand(seed=2)
        h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 200, 32).finalize()
        x6 = h.vcycle(b).numpy()
        h.set_smoother(0.8, 1, 1)
        x = h.vcycle(b).numpy()
        h8 = mg.Hierarchy(A, 0.8, 1, 1).coarsen(10.0, 2, 8.0, 200, 32).finalize()
        x8 = h8.vcycle(b).numpy()
        t, r, rc = ctx.vec(n), ctx.vec(n), ctx.vec(h.level_shape(1)[0])
        assert h.pre_pass(0, b, t, r, rc) and h8.pre_pass(0, b, t, r, rc)
        assert not np.array_equal(x, x6)
        assert np.array_equal(x, x8), rel(x, x8)
    finally:
        restore(ctx)


def test_fp32_operand_levels_do_not_move(ctx, mg):
    """e. levels switched to FP32 operands run the float form of the kernel, which streams its diagonal as before"""
    N = 48; n = N ** 3
    try:
        small_levels_group(ctx)
        A = ctx.poisson3d(N)
        h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 200, 32).finalize()
        b = ctx.vec(n).rand(seed=4)
        x64 = h.vcycle(b).numpy()
        h.set_operand_precision(32)
        assert h.operand_precision(0) == 32 and h.group_info(0)["groups"] > 0
        x1 = h.vcycle(b).numpy()
        t, r, rc = ctx.vec(n), ctx.vec(n), ctx.vec(h.level_shape(1)[0])
        assert not h.pre_pass(0, b, t, r, rc)
        ctx.set_option("pre_nodiag", 0); x0 = h.vcycle(b).numpy(); ctx.set_option("pre_nodiag", 1)
        assert not np.array_equal(x1, x64)
        assert np.array_equal(x1, x0)
    finally:
        restore(ctx)
