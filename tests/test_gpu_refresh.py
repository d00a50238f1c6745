"""mgs_hier_refresh: a hierarchy whose fine operator got new values on the same pattern (mgs_csr_update_values) is held BIT FOR BIT to a
twin built from scratch on a second upload of the new matrix with the same aggregates (every level's aggregation downloaded and pushed
as a 0/1 CSR P).  Same operands, same kernels' sums in the same order: no tolerance anywhere in this file."""
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sps

from galerkin_ref import galerkin_restated

pytestmark = pytest.mark.gpu

OK, INVALID, NUMERIC, STATE = 0, -1, -5, -6
TOL = 1e-10


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


def csky(N, velocity):
    from multigridsolver_amd import synthetic
    return synthetic.csky3d(N, velocity=velocity, rowsum_floor=synthetic.CSKY_ROWSUM_MARGIN)


@pytest.fixture(scope="module")
def pair24():
    """A1 = csky3d(24) at velocity 1000, A2 = the same at velocity 800: one pattern, two sets of values"""
    rp1, ci1, v1 = csky(24, 1000.0)
    rp2, ci2, v2 = csky(24, 800.0)
    assert np.array_equal(rp1, rp2) and np.array_equal(ci1, ci2)
    assert not np.array_equal(v1, v2)
    return 24 ** 3, rp1, ci1, v1, v2


def agg_P(g, nc):
    ok = g >= 0
    return sps.csr_matrix((np.ones(int(ok.sum())), (np.flatnonzero(ok), g[ok])), shape=(len(g), nc))


def twin_of(ctx, mg, h, n, rp, ci, v, omega=0.6):
    """a hierarchy built from scratch on a fresh upload of (rp, ci, v) with h's aggregates, level by level"""
    A2 = ctx.csr(n, n, rp, ci, v)
    h2 = mg.Hierarchy(A2, omega, 1, 1)
    for l in range(h.nlev - 1):
        g = h.level_P(l).agg()
        P = agg_P(g, h.level_shape(l + 1)[0])
        h2.push_P(ctx.csr(P.shape[0], P.shape[1], P.indptr, P.indices, P.data))
    assert h2.nlev == h.nlev
    return A2, h2.finalize()


def assert_same_bits(h, h2, b, what=""):
    for l in range(h.nlev):
        (rp, ci, v), (rp2, ci2, v2) = h.level_A(l).download(), h2.level_A(l).download()
        assert np.array_equal(rp, rp2) and np.array_equal(ci, ci2), (what, l)
        assert np.array_equal(v, v2), (what, l, float(np.abs(v - v2).max()))
    x, x2 = h.vcycle(b).numpy(), h2.vcycle(b).numpy()
    assert np.isfinite(x).all() and np.linalg.norm(x) > 0
    assert np.array_equal(x, x2), (what, float(np.abs(x - x2).max()))
    return x


def built(ctx, mg, n, rp, ci, v, omega=0.6):
    """hierarchy by device aggregation on an upload of (rp, ci, v), one cycle run so that operands and graphs exist"""
    A = ctx.csr(n, n, rp, ci, v)
    h = mg.Hierarchy(A, omega, 1, 1).coarsen(10.0, 2, 8.0).finalize()
    assert h.nlev >= 3
    b = ctx.vec(n).rand(seed=11)
    h.vcycle(b)
    return A, h, b


def test_refresh_is_the_twin_bit_for_bit(ctx, mg, pair24):
    n, rp, ci, v1, v2 = pair24
    A, h, b = built(ctx, mg, n, rp, ci, v1)
    x1 = h.vcycle(b).numpy()
    assert A.update_values(v2) is A
    assert h.refresh() is h
    info = h.refresh_info()
    assert info["refreshes"] == 1 and info["device_levels"] == h.nlev - 1, info
    A2, h2 = twin_of(ctx, mg, h, n, rp, ci, v2)
    x2 = assert_same_bits(h, h2, b, "velocity 800")
    assert not np.array_equal(x1, x2)
    # the refreshed level-1 values against the scipy restatement of the summation order
    g = h.level_P(0).agg()
    M = galerkin_restated(rp, ci, v2, g, h.level_shape(1)[0])
    rp1, ci1, val1 = h.level_A(1).download()
    assert np.array_equal(rp1, M.indptr) and np.array_equal(ci1, M.indices)
    assert np.array_equal(val1, M.data), float(np.abs(val1 - M.data).max())
    # a second refresh back to A1's values, against a twin on A1
    A.update_values(v1); h.refresh()
    assert h.refresh_info()["refreshes"] == 2
    A1t, h1t = twin_of(ctx, mg, h, n, rp, ci, v1)
    assert_same_bits(h, h1t, b, "back to velocity 1000")


def test_refresh_device_values_form(ctx, mg, pair24):
    """update_values from a device vector (the D2D form) and from a raw device pointer + length"""
    n, rp, ci, v1, v2 = pair24
    A, h, b = built(ctx, mg, n, rp, ci, v1)
    dv = ctx.vec(v2)
    assert len(dv) == A.nnz
    A.update_values(dv); h.refresh()
    A2, h2 = twin_of(ctx, mg, h, n, rp, ci, v2)
    assert_same_bits(h, h2, b, "device vector")
    dv1 = ctx.vec(v1)
    A.update_values(dv1.ptr, len(dv1)); h.refresh()
    A1t, h1t = twin_of(ctx, mg, h, n, rp, ci, v1)
    assert_same_bits(h, h1t, b, "device pointer")


def test_refresh_fp32_operands_follow(ctx, mg, pair24):
    n, rp, ci, v1, v2 = pair24
    A, h, b = built(ctx, mg, n, rp, ci, v1)
    h.set_operand_precision(32)
    assert h.operand_precision(0) == 32
    x32_old = h.vcycle(b).numpy()
    A.update_values(v2); h.refresh()
    assert h.operand_precision(0) == 32
    A2, h2 = twin_of(ctx, mg, h, n, rp, ci, v2)
    x64 = h2.vcycle(b).numpy()
    h2.set_operand_precision(32)
    x32 = assert_same_bits(h, h2, b, "FP32 operands")
    assert not np.array_equal(x32, x64) and not np.array_equal(x32, x32_old)


def test_refresh_kcycle(ctx, mg, pair24):
    n, rp, ci, v1, v2 = pair24
    A, h, b = built(ctx, mg, n, rp, ci, v1)
    h.set_kcycle(2)
    h.vcycle(b)
    A.update_values(v2); h.refresh()
    A2, h2 = twin_of(ctx, mg, h, n, rp, ci, v2)
    h2.set_kcycle(2)
    assert_same_bits(h, h2, b, "K-cycle")


def test_refresh_after_new_smoother(ctx, mg, pair24):
    """set_smoother between update_values and refresh: the refreshed operands carry the new ω"""
    n, rp, ci, v1, v2 = pair24
    A, h, b = built(ctx, mg, n, rp, ci, v1)
    A.update_values(v2)
    h.set_smoother(0.8, 1, 1)
    h.refresh()
    A2, h2 = twin_of(ctx, mg, h, n, rp, ci, v2, omega=0.8)
    assert_same_bits(h, h2, b, "omega 0.8")


def test_refresh_before_first_cycle(ctx, mg, pair24):
    """operands not built yet are left to the next cycle's setup, which sees the new values"""
    n, rp, ci, v1, v2 = pair24
    A = ctx.csr(n, n, rp, ci, v1)
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0).finalize()
    A.update_values(v2); h.refresh()
    A2, h2 = twin_of(ctx, mg, h, n, rp, ci, v2)
    assert_same_bits(h, h2, ctx.vec(n).rand(seed=3), "no cycle before the refresh")


def test_refresh_keeps_the_cached_graphs(ctx, mg, pair24):
    n, rp, ci, v1, v2 = pair24
    A, h, b = built(ctx, mg, n, rp, ci, v1)
    x = ctx.vec(n)
    h.vcycle(b, x); h.vcycle(b, x)
    before = h.graph_info()["captured_cycles"]
    assert before >= 1
    A.update_values(v2); h.refresh()
    assert h.graph_info()["captured_cycles"] == before
    assert h.refresh_info()["kept_graphs"] == 1
    h.vcycle(b, x)                                            # a replay of the graph captured before the refresh
    assert h.graph_info()["captured_cycles"] == before
    A2, h2 = twin_of(ctx, mg, h, n, rp, ci, v2)
    assert np.array_equal(x.numpy(), h2.vcycle(b).numpy())   # ... which sees the new values


def true_res(A, x, b):
    return A.residual(x, b).nrm2() / b.nrm2()


def test_bicgstab_on_the_refreshed_hierarchy(ctx, mg, pair24):
    n, rp, ci, v1, v2 = pair24
    A, h, _ = built(ctx, mg, n, rp, ci, v1)
    A.update_values(v2); h.refresh()
    A2, h2 = twin_of(ctx, mg, h, n, rp, ci, v2)
    b = ctx.vec(n).rand(seed=5)
    x, x2, x3 = ctx.vec(n), ctx.vec(n), ctx.vec(n)
    st, it, tol = mg.bicgstab(A, x, b, h, 500, TOL)
    st2, it2, tol2 = mg.bicgstab(A2, x2, b, h2, 500, TOL)
    A3 = ctx.csr(n, n, rp, ci, v2)
    h3 = mg.Hierarchy(A3, 0.6, 1, 1).coarsen(10.0, 2, 8.0).finalize()
    st3, it3, _ = mg.bicgstab(A3, x3, b, h3, 500, TOL)
    res = true_res(A, x, b)
    print(f"BiCGSTAB csky3d(24) velocity 1000 -> 800: refreshed {it} it (true residual {res:.3e}), twin {it2} it, rebuilt by coarsen {it3} it (status {st3})")
    assert st == 0 and st2 == 0, (st, st2)
    assert it == it2, (it, it2)
    assert res < TOL, res
    assert np.array_equal(x.numpy(), x2.numpy())


def test_pcg_on_a_refreshed_spd_pair(ctx, mg):
    """device Poisson 48³ and the same scaled symmetrically, a_ij·d_i·d_j with d in [√0.5, √2]"""
    N = 48; n = N ** 3
    A = ctx.poisson3d(N)
    rp, ci, v1 = A.download()
    d = np.sqrt(np.random.default_rng(7).uniform(0.5, 2.0, n))
    rows = np.repeat(np.arange(n), np.diff(rp))
    v2 = v1 * d[rows] * d[ci]
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0).finalize()
    b = ctx.vec(n).rand(seed=9)
    h.vcycle(b)
    A.update_values(v2); h.refresh()
    A2, h2 = twin_of(ctx, mg, h, n, rp, ci, v2)
    assert_same_bits(h, h2, b, "scaled Poisson")
    x, x2, x3 = ctx.vec(n), ctx.vec(n), ctx.vec(n)
    st, it, _ = mg.pcg(A, x, b, h, 500, TOL)
    st2, it2, _ = mg.pcg(A2, x2, b, h2, 500, TOL)
    A3 = ctx.csr(n, n, rp, ci, v2)
    h3 = mg.Hierarchy(A3, 0.6, 1, 1).coarsen(10.0, 2, 8.0).finalize()
    st3, it3, _ = mg.pcg(A3, x3, b, h3, 500, TOL)
    res = true_res(A, x, b)
    print(f"PCG Poisson 48^3 scaled: refreshed {it} it (true residual {res:.3e}), twin {it2} it, rebuilt by coarsen {it3} it (status {st3})")
    assert st == 0 and st2 == 0, (st, st2)
    assert it == it2, (it, it2)
    assert res < TOL, res


def code_of(fn):
    import multigridsolver_amd as m
    with pytest.raises(m.MgsError) as e:
        fn()
    return e.value.code


def test_errors(ctx, mg, orc, pair24):
    n, rp, ci, v1, v2 = pair24
    A = ctx.csr(n, n, rp, ci, v1)
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0)
    assert code_of(h.refresh) == STATE                                   # before finalize
    h.finalize()
    b = ctx.vec(n).rand(seed=2)
    h.vcycle(b)
    assert code_of(lambda: A.update_values(v2[:-1])) == INVALID          # wrong length
    assert code_of(lambda: A.update_values(ctx.vec(A.nnz + 1))) == INVALID
    ctx.set_option("valcode", 1)
    try:
        assert code_of(h.refresh) == INVALID
    finally:
        ctx.set_option("valcode", 0)
    # a general-P level
    Ao = orc.poisson2d(20)
    m = Ao.shape[0]; mc = m // 4
    rows = np.repeat(np.arange(m), 2)
    cols = np.stack([np.arange(m) // 4, (np.arange(m) // 4 + 1) % mc], 1).ravel()
    Pg = sps.csr_matrix((np.tile([0.75, 0.25], m), (rows, cols)), shape=(m, mc))
    Ag = ctx.csr(m, m, Ao.rowptr, Ao.col, Ao.val)
    hg = mg.Hierarchy(Ag, 0.6, 1, 1).push_P(ctx.csr(m, mc, Pg.indptr, Pg.indices, Pg.data)).finalize()
    assert code_of(hg.refresh) == INVALID
    # a zero on the diagonal: numeric error, and no cycle until a later refresh succeeds
    bad = v2.copy()
    row = 5
    k = rp[row] + int(np.flatnonzero(ci[rp[row]:rp[row + 1]] == row)[0])
    bad[k] = 0.0
    A.update_values(bad)
    assert code_of(h.refresh) == NUMERIC
    assert code_of(lambda: h.vcycle(b)) == STATE
    assert h.graph_info()["captured_cycles"] == 0
    A.update_values(v2); h.refresh()
    A2, h2 = twin_of(ctx, mg, h, n, rp, ci, v2)
    assert_same_bits(h, h2, b, "restored after the numeric error")


def test_refresh_leaves_the_bytes_in_use_unchanged():
    """in a process of its own (the arena is per process): from the second refresh on, mgs_arena_info's bytes in use do not move"""
    from conftest import REPO
    code = r'''
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import multigridsolver_amd as mg
L = mg.lib()
assert L.mgs_arena_reserve(C.c_size_t(256 << 20)) == 0
def used():
    out = (C.c_size_t * 3)(); assert L.mgs_arena_info(out) == 0; return int(out[1])
ctx = mg.Context(0)
A = ctx.poisson3d(48); n = 48 ** 3
rp, ci, v = A.download()
h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0).finalize()
b = ctx.vec(n).rand(seed=4); x = ctx.vec(n)
h.vcycle(b, x)
seen = []
for k in range(3):
    vk = v * (1.0 + 0.1 * (k + 1))
    A.update_values(vk)
    before = used(); h.refresh(); after = used()
    seen.append((before, after))
    h.vcycle(b, x); ctx.sync()
assert used() > 0
assert seen[1][0] == seen[1][1] and seen[2][0] == seen[2][1], seen
assert h.refresh_info()["refreshes"] == 3
assert seen[0][1] - seen[0][0] >= h.refresh_info()["extra_bytes"] > 0, (seen, h.refresh_info())
ctx.close()
print("REFRESH_BYTES", seen)
''' % REPO
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0 and "REFRESH_BYTES" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
