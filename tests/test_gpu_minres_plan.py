"""mgs_minres_plan on the device against mgs_minres on the same device: the plan promises mgs_minres's contract and mgs_minres's BITS, for
every `ahead`, and an enqueue-only form that never waits for the device.  Every comparison below is exact ((status, iterations, resid)
equal, np.array_equal on x) except where a true residual is recomputed with scipy, which is held to 1.5·tol, the margin of
tests/test_gpu_minres.py.

Fixtures: tests/minres_ref.py's saddle(N) with the explicit two-P hierarchy of tests/test_gpu_minres.py, ω = 0.6, V(1,1), b = saddle_rhs.
saddle(7) has 515 rows — odd, so the tail element of the 16-byte arms runs — and P's of (515, 71) and (71, 9).  On the CPU
(tests/test_minres_plan_ref_cpu.py) it makes true-residual checks at iterations 37 and 39 (refused) and 40 at tol 1e-6, and at 60
(refused) and 61 at 1e-10, so ahead = 1, 2 and 7 all enqueue iterations past a refused check and the recalibration runs.  The device's
own counts may differ in the last place: the tests compare with mgs_minres and assert info[5] >= 1, not an iteration number."""
import time

import numpy as np
import pytest
import scipy.sparse as sps

from minres_ref import banded_sym, saddle, saddle_rhs
from test_gpu_minres import Saddle, dev, to_scipy, true_resid

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -6
AHEADS = (0, 1, 2, 7, 10000)


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


class Sys:
    """a saddle system on the device: K, b, one hierarchy for mgs_minres (the reference side) whose results are computed once and shared"""

    def __init__(self, mg, ctx, orc, N):
        self.mg, self.ctx = mg, ctx
        self.s = Saddle(orc, N)
        self.rows = self.s.rows
        self.K = dev(ctx, self.s.K)
        self.b = ctx.vec(self.s.b)
        self.h_ref = self.s.hierarchy(mg, ctx)
        self._ref = {}

    def hierarchy(self):
        return self.s.hierarchy(self.mg, self.ctx)

    def minres(self, tol, max_iter=500):
        key = (tol, max_iter)
        if key not in self._ref:
            x = self.ctx.vec(self.rows)
            r = self.mg.minres(self.K, x, self.b, self.h_ref, max_iter, tol)
            self._ref[key] = (r, x.numpy())
        return self._ref[key]


_made = {}


@pytest.fixture
def sys7(mg, ctx, orc):
    if 7 not in _made:
        _made[7] = Sys(mg, ctx, orc, 7)
        assert _made[7].rows == 515 and [P.shape for P in _made[7].s.Ps] == [(515, 71), (71, 9)]
    return _made[7]


@pytest.fixture
def sys5(mg, ctx, orc):
    if 5 not in _made:
        _made[5] = Sys(mg, ctx, orc, 5)
        assert _made[5].rows == 188
    return _made[5]


@pytest.fixture(scope="module", autouse=True)
def _release(ctx):
    yield
    _made.clear()      # before the context closes


def same(got, x, want, xw, label=""):
    assert got == want, (label, got, want)
    assert np.array_equal(x, xw), (label, "x differs")


# ------------------------------------------------------------------------------------------------------ 1. same bits as mgs_minres
@pytest.mark.parametrize("tol", [1e-6, 1e-10])
def test_same_bits_as_mgs_minres(ctx, mg, sys7, tol):
    want, xw = sys7.minres(tol)
    assert want[0] == 0 and 10 < want[1] < 200
    h = sys7.hierarchy()
    plan = mg.MinresPlan(sys7.K, h)
    for ahead in AHEADS:
        x = ctx.vec(sys7.rows)
        got = plan.solve(x, sys7.b, 500, tol, ahead)
        info = plan.info()
        print(f"tol {tol:g} ahead {ahead}: {got}, info {info}")
        same(got, x.numpy(), want, xw, f"ahead {ahead}")
        assert info[2] - info[3] == want[1] and info[5] >= 1
        if ahead == 0:
            assert info[3] == 0
    assert h.graph_info()["captured_cycles"] == 2          # the plan's (v[k], z̃[k]) pairs never move
    # x and b 8 bytes off a 16-byte boundary: the 8-byte arm of the update pass, against mgs_minres on the same views
    n = sys7.rows
    xb, bb = ctx.vec(n + 2), ctx.vec(n + 2)
    xo, bo = mg.Vec.wrap(ctx, xb.ptr + 8, n), mg.Vec.wrap(ctx, bb.ptr + 8, n)
    assert xo.ptr % 16 == 8 and bo.ptr % 16 == 8
    bo.upload(sys7.s.b)
    want8 = mg.minres(sys7.K, xo, bo, sys7.h_ref, 500, tol); xw8 = xo.numpy()
    assert want8[0] == 0 and np.array_equal(xw8, xw)
    for ahead in AHEADS:
        xo.fill(0.0)
        got8 = plan.solve(xo, bo, 500, tol, ahead)
        same(got8, xo.numpy(), want8, xw8, f"8-byte views, ahead {ahead}")
        assert plan.info()[5] >= 1
    del xo, bo


def test_same_bits_without_a_hierarchy(ctx, mg, sys5):
    """h = NULL on saddle(5)'s K, cut at max_iter = 40: the copy arm, and status 1 with the true residual"""
    n = sys5.rows
    x = ctx.vec(n); want = mg.minres(sys5.K, x, sys5.b, None, 40, 1e-10); xw = x.numpy()
    assert want[:2] == (1, 40)
    tr = true_resid(sys5.s.K, xw, sys5.s.b)
    assert abs(want[2] - tr) <= 1e-10 * tr
    plan = mg.MinresPlan(sys5.K)
    for ahead in AHEADS:
        y = ctx.vec(n); got = plan.solve(y, sys5.b, 40, 1e-10, ahead)
        same(got, y.numpy(), want, xw, f"h = None, ahead {ahead}")
        assert plan.info()[2] == 40 and plan.info()[3] == 0


# ------------------------------------------------------------------------------------------------------------------ 2. every status
def test_every_status(ctx, mg, sys5, sys7):
    i32 = np.int32
    n = sys7.rows
    h = sys7.hierarchy()
    plan = mg.MinresPlan(sys7.K, h)
    # 0 at iteration 0: b = 0, and x0 = a converged x
    z = ctx.vec(n)
    for ahead in (0, 3):
        y = ctx.vec(n); got = plan.solve(y, z, 500, 1e-6, ahead)
        assert got == (0, 0, 0.0) == mg.minres(sys7.K, ctx.vec(n), z, sys7.h_ref, 500, 1e-6) and not y.numpy().any()
    _, xs = sys7.minres(1e-10)
    x = ctx.vec(xs); want = mg.minres(sys7.K, x, sys7.b, sys7.h_ref, 500, 1e-6)
    for ahead in (0, 3):
        y = ctx.vec(xs); got = plan.solve(y, sys7.b, 500, 1e-6, ahead)
        same(got, y.numpy(), want, xs, "converged x0")
        assert got[:2] == (0, 0)
    # 1 with max_iter 3 and 0
    for max_iter in (3, 0):
        want, xw = sys7.minres(1e-10, max_iter)
        assert want[:2] == (1, max_iter)
        for ahead in (0, 1, 5):
            y = ctx.vec(n); got = plan.solve(y, sys7.b, max_iter, 1e-10, ahead)
            same(got, y.numpy(), want, xw, f"max_iter {max_iter} ahead {ahead}")
            assert plan.info()[2] == max_iter
    # 2 at the start: a one-level hierarchy on −L, whose dense coarse solve is (−L)⁻¹
    Ls = sys5.s.sd["L"]; m = Ls.shape[0]
    hn = mg.Hierarchy(dev(ctx, -Ls), 0.6, 1, 1).finalize()
    assert hn.nlev == 1
    Ld, bl = dev(ctx, Ls), ctx.vec(saddle_rhs(m))
    x = ctx.vec(m); want = mg.minres(Ld, x, bl, hn, 50, 1e-8)
    assert want == (2, 0, 1.0)
    pn = mg.MinresPlan(Ld, hn)
    for ahead in (0, 2):
        y = ctx.vec(m); got = pn.solve(y, bl, 50, 1e-8, ahead)
        same(got, y.numpy(), want, np.zeros(m), "negative definite preconditioner")
    y = ctx.vec(m)
    assert pn.enqueue(y, bl, 4, 1e-8).result() == (2, 0, 1.0) and not y.numpy().any()
    # 3 with the 2×2 singular cases (x untouched), and the two-iteration 2×2 cases
    two = [
        ((np.array([0, 1, 1], i32), np.array([0], i32), np.array([1.0])), np.array([0.0, 1.0]), np.zeros(2), (3, 1)),
        ((np.array([0, 1, 1], i32), np.array([0], i32), np.array([1.0])), np.array([0.25, 1.0]), np.array([0.25, -0.5]), (3, 1)),
        ((np.array([0, 1, 2], i32), np.array([1, 0], i32), np.array([1.0, 1.0])), np.array([1.0, 0.0]), np.zeros(2), (0, 2)),
        ((np.array([0, 1, 2], i32), np.array([0, 1], i32), np.array([1.0, -1.0])), np.array([1.0, 1.0]), np.zeros(2), (0, 2)),
    ]
    for (rp, ci, v), b2, x0, st_it in two:
        A = ctx.csr(2, 2, rp, ci, v)
        bv = ctx.vec(b2)
        x = ctx.vec(x0); want = mg.minres(A, x, bv, None, 10, 1e-12)
        assert want[:2] == st_it
        p2 = mg.MinresPlan(A)
        for ahead in (0, 1, 4):
            y = ctx.vec(x0); got = p2.solve(y, bv, 10, 1e-12, ahead)
            same(got, y.numpy(), want, x.numpy(), f"2x2 {st_it} ahead {ahead}")
        if st_it[0] == 3:
            assert np.array_equal(x.numpy(), x0)
        y = ctx.vec(x0)
        st, done, res = p2.enqueue(y, bv, 10, 1e-12).result()
        assert (st, done, res) == want and np.array_equal(y.numpy(), x.numpy())
    # operators of 1, 2 and 3 rows: 12 fixed steps
    for k in (1, 2, 3):
        A = ctx.csr(k, k, *banded_sym(k, seed=200).csr())
        bv = ctx.vec(np.array([1.0, -0.5, 0.25][:k]))
        x = ctx.vec(k); want = mg.minres(A, x, bv, None, 12, 1e-300)
        pk = mg.MinresPlan(A)
        for ahead in (0, 2):
            y = ctx.vec(k); got = pk.solve(y, bv, 12, 1e-300, ahead)
            same(got, y.numpy(), want, x.numpy(), f"{k} rows ahead {ahead}")


# ---------------------------------------------------------------------------------------------------------- 3. allowed hierarchies
@pytest.mark.parametrize("tweak", ["additive", "scale"])
def test_allowed_hierarchies(ctx, mg, sys7, tweak):
    def make():
        h = sys7.hierarchy()
        return h.set_additive(True) if tweak == "additive" else h.set_correction_scale(1.1)
    n = sys7.rows
    x = ctx.vec(n); want = mg.minres(sys7.K, x, sys7.b, make(), 500, 1e-6); xw = x.numpy()
    assert want[0] == 0
    plan = mg.MinresPlan(sys7.K, make())
    for ahead in (0, 1, 7):
        y = ctx.vec(n); got = plan.solve(y, sys7.b, 500, 1e-6, ahead)
        same(got, y.numpy(), want, xw, f"{tweak}, ahead {ahead}")


# ---------------------------------------------------------------------------------------------------------------- 4. enqueue only
def test_enqueue_only(ctx, mg, sys7):
    n, tol = sys7.rows, 1e-6
    want, xw = sys7.minres(tol)
    iters = want[1] + 5
    h = sys7.hierarchy()
    plan = mg.MinresPlan(sys7.K, h)
    x = ctx.vec(n)
    plan.enqueue(x, sys7.b, iters, tol)
    st, done, res, est = plan.result(recursive=True)
    info = plan.info()
    print(f"enqueue({iters}): {(st, done, res, est)}, mgs_minres {want}, info {info}")
    assert st == 1 and done < iters and est < tol <= res      # the estimate ran ahead of the 2-norm
    cut, xc = sys7.minres(0.0, done)
    assert cut == (1, done, res) and np.array_equal(x.numpy(), xc)
    assert info[2] == iters and info[3] == iters - done and info[4] == 0
    # again from that x: κ is measured afresh
    st2, done2, res2 = plan.enqueue(x, sys7.b, iters, tol).result()
    tr = true_resid(sys7.s.K, x.numpy(), sys7.s.b)
    print(f"again from x: {(st2, done2, res2)}, recomputed {tr:.4e}")
    assert st2 == 0 and res2 < tol and tr < 1.5 * tol and abs(res2 - tr) <= 1e-6 * tr
    # tol = 0 runs exactly `iters` iterations
    cut5, x5w = sys7.minres(0.0, 5)
    x5 = ctx.vec(n)
    assert plan.enqueue(x5, sys7.b, 5, 0.0).result() == cut5 == (1, 5, cut5[2]) and np.array_equal(x5.numpy(), x5w)
    assert plan.info()[3] == 0
    # two enqueues with different (x, b) before one result
    b2_np = saddle_rhs(n, seed=5); b2 = ctx.vec(b2_np)
    x2w = ctx.vec(n); want2 = mg.minres(sys7.K, x2w, b2, sys7.h_ref, 7, 0.0)
    xa, xb = ctx.vec(n), ctx.vec(n)
    plan.enqueue(xa, sys7.b, 5, 0.0)
    plan.enqueue(xb, b2, 7, 0.0)
    assert plan.result() == want2
    assert np.array_equal(xa.numpy(), x5w) and np.array_equal(xb.numpy(), x2w.numpy())
    assert h.graph_info()["captured_cycles"] == 2


# ------------------------------------------------------------------------------------------------------ 5. enqueue does not wait
def test_enqueue_does_not_wait(mg, orc):
    """a busy kernel of about 0.3 s in front on the same stream: enqueue returns while it still runs"""
    import torch
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        c = mg.Context(0, stream.cuda_stream)
        plan = h = None
        try:
            s = Saddle(orc, 7); n = s.rows
            K = dev(c, s.K)
            h = s.hierarchy(mg, c)
            b = c.vec(s.b)
            plan = mg.MinresPlan(K, h)
            xw = c.vec(n); want = plan.solve(xw, b, 500, 1e-6, 0)          # warm-up, and the counts of the two extremes of `ahead`
            it = want[1]
            assert want[0] == 0 and plan.info()[4] >= it
            x = c.vec(n); got = plan.solve(x, b, 500, 1e-6, 10000)
            assert got == want and plan.info()[4] <= 2 * (plan.info()[5] + 1)
            x5w = c.vec(n); plan.enqueue(x5w, b, 5, 1e-6).result()
            # the busy kernel: torch's spin kernel, else a chain of the library's own SpMV launches; calibrated once with two events
            if hasattr(torch.cuda, "_sleep"):
                unit, busy = 50_000_000, lambda k: torch.cuda._sleep(int(k))
            else:
                u, v = c.vec(n), c.vec(n)
                unit, busy = 500, lambda k: [K.spmv(u, v) for _ in range(int(k))]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); busy(unit); e1.record(stream); e1.synchronize()
            ms = e0.elapsed_time(e1)
            x5 = c.vec(n)
            stream.synchronize()
            busy(unit * 300.0 / max(ms, 1e-3))
            ev = torch.cuda.Event(); ev.record(stream)
            t0 = time.perf_counter()
            plan.enqueue(x5, b, 5, 1e-6)
            dt = time.perf_counter() - t0
            still_busy = not ev.query()
            st, done, res = plan.result()
            print(f"busy kernel calibrated {ms:.1f} ms per {unit} units; enqueue(5) returned after {dt * 1e3:.2f} ms, busy kernel still running: {still_busy}")
            assert still_busy
            assert (st, done) == (1, 5) and plan.info()[4] == 0
            assert np.array_equal(x5.numpy(), x5w.numpy())
        finally:
            stream.synchronize()
            del plan, h
            c.close()


# ------------------------------------------------------------------------------------------------------------------- 6. refusals
def refused(mg, code, word, fn):
    with pytest.raises(mg.MgsError) as e:
        fn()
    assert e.value.code == code and word in str(e.value) and "mgs_minres_plan" in str(e.value), str(e.value)


def test_refusals(ctx, mg, sys5):
    s = sys5
    n = s.rows
    K = s.K
    x, b = ctx.vec(n), ctx.vec(s.s.b)
    refused(mg, INVALID, "nu1 == nu2", lambda: mg.MinresPlan(K, s.s.hierarchy(mg, ctx, 2, 1)))
    refused(mg, INVALID, "K-cycle", lambda: mg.MinresPlan(K, s.hierarchy().set_kcycle(1)))
    refused(mg, INVALID, "K-cycle", lambda: mg.MinresPlan(K, s.hierarchy().set_kcycle_entry(True)))
    refused(mg, INVALID, "null space", lambda: mg.MinresPlan(dev(ctx, s.s.K).set_nullspace("constant")))
    from multigridsolver_amd.synthetic import neumann3d
    neu = ctx.csr(512, 512, *neumann3d(8)).set_nullspace("constant")             # declared on the hierarchy's fine operator only
    hn = mg.Hierarchy(neu, 0.6, 1, 1).coarsen(coarse_rows=60).finalize()
    refused(mg, INVALID, "null space", lambda: mg.MinresPlan(ctx.csr(512, 512, *neumann3d(8)), hn))
    refused(mg, INVALID, "not square", lambda: mg.MinresPlan(dev(ctx, s.s.K[:, :-1])))
    shard = ctx.poisson3d(16, 4, 8, local_cols=True)
    refused(mg, INVALID, "row shard", lambda: mg.MinresPlan(shard))
    twin = ctx.poisson3d(8)
    hc = mg.Hierarchy(twin, 0.6, 1, 1).coarsen(coarse_rows=60).finalize()
    refused(mg, INVALID, "rows", lambda: mg.MinresPlan(K, hc))                   # a hierarchy of another size
    hc.set_halo_exchange(lambda level, ptr: None)
    refused(mg, INVALID, "callbacks", lambda: mg.MinresPlan(twin, hc))
    refused(mg, STATE, "finalize", lambda: mg.MinresPlan(twin, mg.Hierarchy(twin, 0.6, 1, 1)))
    try:
        empty = ctx.csr(0, 0, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    except mg.MgsError:
        empty = None
    if empty is not None:
        refused(mg, INVALID, "no rows", lambda: mg.MinresPlan(empty))
    plan = mg.MinresPlan(K)
    refused(mg, STATE, "nothing", lambda: plan.result())
    refused(mg, INVALID, "rows", lambda: plan.solve(ctx.vec(n - 1), b))
    refused(mg, INVALID, "rows", lambda: plan.solve(x, ctx.vec(n - 1)))
    refused(mg, INVALID, "rows", lambda: plan.enqueue(x, ctx.vec(n - 1), 3, 1e-6))
    refused(mg, INVALID, "alias", lambda: plan.solve(b, b))
    refused(mg, INVALID, "alias", lambda: plan.enqueue(b, b, 3, 1e-6))
    refused(mg, INVALID, "ahead", lambda: plan.solve(x, b, ahead=-1))
    refused(mg, INVALID, "iters", lambda: plan.enqueue(x, b, -1, 1e-6))
    L = mg.lib()
    assert L.mgs_minres_plan_create(None, None, None) == INVALID
    assert L.mgs_minres_plan_create(K.h, None, None) == INVALID and "mgs_minres_plan_create" in L.mgs_last_error(ctx.h).decode()
    assert L.mgs_minres_plan_solve(None, x.h, b.h, 0, None, None, None) == INVALID
    assert L.mgs_minres_plan_solve(plan.h, x.h, b.h, 0, None, None, None) == INVALID and "mgs_minres_plan_solve" in L.mgs_last_error(ctx.h).decode()
    assert L.mgs_minres_plan_enqueue(plan.h, None, b.h, 1, 1e-6) == INVALID and "mgs_minres_plan_enqueue" in L.mgs_last_error(ctx.h).decode()
    assert L.mgs_minres_plan_result(None, None, None, None, None) == INVALID
    assert L.mgs_minres_plan_info(plan.h, None) == INVALID and "mgs_minres_plan_info" in L.mgs_last_error(ctx.h).decode()
    assert L.mgs_minres_plan_destroy(None) == 0
    assert not x.numpy().any() and np.array_equal(b.numpy(), s.s.b)
    c2 = mg.Context(0)
    try:
        c2.set_allreduce(lambda a: None)
        A2c = c2.poisson3d(8)
        refused(mg, INVALID, "sums over ranks", lambda: mg.MinresPlan(A2c))
        del A2c
    finally:
        c2.close()


# --------------------------------------------------------------------------------------------------------------------- 7. repeat
def test_repeat(ctx, mg, sys7):
    """two solves and two enqueues give the same bits; mgs_arena_info's bytes in use (0 without an arena: MGS_ARENA_GB) and info[0] stay as
    create left them"""
    import ctypes as C
    L = mg.lib()

    def used():
        out = (C.c_size_t * 3)(); assert L.mgs_arena_info(out) == 0; return int(out[1])
    n = sys7.rows
    h = sys7.hierarchy()
    x = ctx.vec(n)
    plan = mg.MinresPlan(sys7.K, h)
    bytes0, used0 = plan.info()[0], used()
    assert bytes0 >= 7 * 8 * n
    runs = []
    for _ in range(2):
        x.fill(0.0); r = plan.solve(x, sys7.b, 500, 1e-10, 2)
        runs.append((r, x.numpy(), plan.info()[2:6]))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    runs = []
    for _ in range(2):
        x.fill(0.0); r = plan.enqueue(x, sys7.b, 30, 1e-10).result(recursive=True)
        runs.append((r, x.numpy(), plan.info()[2:4]))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    assert plan.info()[0] == bytes0 and used() == used0
    assert h.graph_info()["captured_cycles"] == 2
    plan.close(); plan.close()
    assert not plan.h


# ------------------------------------------------------------------------------------------------- 8. the time step, end to end
def assemble(mg, ctx, Ls, Ds, m):
    """the README's saddle-point recipe on the device → every handle the refresh chain needs"""
    o = {}
    o["L"], o["D"] = dev(ctx, Ls), dev(ctx, Ds)
    o["C"] = mg.Csr.from_diag(ctx, ctx.vec(np.full(m, 1e-2)))
    o["Cm"] = mg.Csr.from_diag(ctx, ctx.vec(np.full(m, -1e-2)))
    o["Dt"] = o["D"].transpose()
    o["Dts"] = o["D"].transpose().scale(left=o["L"].diag_inv())      # diag(L)⁻¹·Dᵀ
    o["G"] = o["D"] @ o["Dts"]
    o["S"] = o["C"] + o["G"]                                           # C + D·diag(L)⁻¹·Dᵀ
    o["K"] = mg.Csr.bmat(ctx, [[o["L"], o["Dt"]], [o["D"], o["Cm"]]])
    o["B"] = mg.Csr.block_diag(ctx, [o["L"], o["S"]])
    return o


def bits(A):
    return tuple(a.tobytes() for a in A.download())


def test_the_time_step_end_to_end(ctx, mg):
    sd = saddle(8)
    n, m, tol = sd["n"], sd["m"], 1e-8
    b_np = saddle_rhs(n + m); b = ctx.vec(b_np)
    o = assemble(mg, ctx, sd["L"], sd["D"], m)
    h = mg.Hierarchy(o["B"], 0.6, 1, 1).coarsen(10.0, 2, 8.0, 50).finalize()
    plan = mg.MinresPlan(o["K"], h)
    x = ctx.vec(n + m)
    first = plan.enqueue(x, b, 200, tol).result()
    assert first[0] in (0, 1) and true_resid(sd["K"], x.numpy(), b_np) < 1e-4
    assert h.graph_info()["captured_cycles"] == 2
    # new values on the same patterns: L's diagonal 6 → 6.5, D's k-th stored value times (1 + 0.25·cos k)
    L2 = sd["L"].copy(); L2.setdiag(6.5); L2 = L2.tocsr(); L2.sort_indices()
    D2 = sd["D"].copy(); D2.data = D2.data * (1.0 + 0.25 * np.cos(np.arange(D2.nnz)))
    assert np.array_equal(L2.indices, sd["L"].indices) and np.array_equal(D2.indices, sd["D"].indices)
    ptrs = o["K"].device_ptrs(), o["S"].device_ptrs()
    # the chain: every step values-only, in place
    o["L"].update_values(L2.data); o["D"].update_values(D2.data)
    o["Dt"].transpose_update(o["D"]); o["Dts"].transpose_update(o["D"])
    o["Dts"].scale(left=o["L"].diag_inv())                            # the refill brought unscaled values
    o["G"].matmul_update(o["D"], o["Dts"])
    o["S"].add_update(o["C"], o["G"])
    o["K"].bmat_update([[o["L"], o["Dt"]], [o["D"], o["Cm"]]])
    o["B"].bmat_update([[o["L"], None], [None, o["S"]]])
    h.refresh()
    x.fill(0.0)
    st, done, res = plan.enqueue(x, b, 200, tol).result()
    assert (o["K"].device_ptrs(), o["S"].device_ptrs()) == ptrs
    # K and S: the bits of a fresh assembly from the new values
    f = assemble(mg, ctx, L2, D2, m)
    assert bits(o["K"]) == bits(f["K"]) and bits(o["S"]) == bits(f["S"]) and bits(o["B"]) == bits(f["B"])
    K2 = sps.bmat([[L2, D2.T], [D2, -1e-2 * sps.eye(m)]], format="csr")
    assert abs(to_scipy(o["K"]) - K2).max() == 0.0
    assert h.graph_info()["captured_cycles"] == 2 and h.refresh_info()["refreshes"] == 1 and h.refresh_info()["kept_graphs"] == 1
    tr = true_resid(K2, x.numpy(), b_np)
    print(f"time step: first solve {first}; after the refresh chain enqueue(200) → {(st, done, res)}, recomputed {tr:.4e}")
    assert st in (0, 1) and abs(res - tr) <= 1e-6 * tr
    # through solve: the bits of mgs_minres on the refreshed hierarchy
    y = ctx.vec(n + m); got = plan.solve(y, b, 500, tol)
    assert h.graph_info()["captured_cycles"] == 2
    z = ctx.vec(n + m); want = mg.minres(o["K"], z, b, h, 500, tol)
    same(got, y.numpy(), want, z.numpy(), "after the refresh chain")
    tr = true_resid(K2, y.numpy(), b_np)
    print(f"  solve: {got}, recomputed {tr:.4e}")
    assert got[0] == 0 and tr < 1.5 * tol
