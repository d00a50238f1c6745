"""mgs_fgcr_plan on the device against mgs_fgcr on the same device: the plan promises mgs_fgcr's contract and mgs_fgcr's BITS, for every `ahead`,
and an enqueue-only form that never waits for the device.  Every comparison below is exact ((status, iterations, resid) equal, np.array_equal on
x) except the true residual of the enqueue-only form, which is held against the oracle's recomputation of ‖b − A·x‖/‖b‖ on mgs_fgcr's x at 1e-12
relative (mgs_residual has the oracle's summation order; only the fold of the norm differs).  Shapes are the smallest on which each path can go
wrong: csky3d(31) is nonsymmetric, has an odd number of rows (the tail element of the 16-byte arms) and 117 row blocks; the exits of mgs_fgcr
are reached with block-diagonal copies of the small operators of tests/test_fgcr_plan_ref_cpu.py, whose dyadic values keep every sum exact in any
order; the restart from the true residual runs on the 2-D Poisson operator 30² at a tolerance the recursion reaches before the true residual."""
import time

import numpy as np
import pytest

from krylov_ref import banded

pytestmark = pytest.mark.gpu

INVALID = -1      # MGS_ERR_INVALID
STATE = -6        # MGS_ERR_STATE
AHEADS = (0, 1, 2, 7, 10000)


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


def dev(ctx, o):
    return ctx.csr(o.shape[0], o.shape[1], o.rowptr, o.col, o.val)


def explicit_levels(Ao, nlev):
    Ps, A = [], Ao
    for _ in range(nlev - 1):
        P = A.agmg(10.0, 2, 8.0, strict=False)
        Ps.append(P)
        A = A.galerkin(P)
    return Ps


def push_all(mg, ctx, A, Ps, omega, nu1=1, nu2=1):
    h = mg.Hierarchy(A, omega, nu1, nu2)
    for P in Ps:
        h.push_P(dev(ctx, P))
    return h.finalize()


class C31:
    """csky3d(31), three levels of explicit P, ω = 0.6: hierarchies for mgs_fgcr (the reference side; V(1,1) and K-cycle) and fresh ones for the
    plans, so that the plans' captured cycles can be counted; the mgs_fgcr results are computed once and shared"""

    def __init__(self, mg, ctx, orc):
        from multigridsolver_amd.synthetic import csky3d
        n = 31 ** 3
        self.Ao = orc.Csr.from_arrays(n, n, *csky3d(31)); self.n = n
        assert self.n % 2 == 1
        self.Ps = explicit_levels(self.Ao, 3)
        self.A = dev(ctx, self.Ao)
        self.h_ref = push_all(mg, ctx, self.A, self.Ps, 0.6)
        self.hk_ref = push_all(mg, ctx, self.A, self.Ps, 0.6).set_kcycle(1)
        self.b_np = orc.rand_rhs(self.n); self.b = ctx.vec(self.b_np)
        self.ref = {}
        self.mg, self.ctx = mg, ctx

    def fgcr(self, restart=10, max_iter=80, tol=1e-10, kcycle=False):
        key = (restart, max_iter, tol, kcycle)
        if key not in self.ref:
            x = self.ctx.vec(self.n)
            r = self.mg.fgcr(self.A, x, self.b, self.hk_ref if kcycle else self.h_ref, restart, max_iter, tol)
            self.ref[key] = (r, x.numpy())
        return self.ref[key]


_c31 = {}


@pytest.fixture
def c31(mg, ctx, orc):
    if "p" not in _c31:
        _c31["p"] = C31(mg, ctx, orc)
    return _c31["p"]


@pytest.fixture(scope="module", autouse=True)
def _release(ctx):
    yield
    _c31.clear()      # before the context closes


def same(got, x, want, xw, label=""):
    assert got[:2] == want[:2] and (got[2] == want[2] or (np.isnan(got[2]) and np.isnan(want[2]))), (label, got, want)
    assert np.array_equal(x, xw, equal_nan=True), (label, "x differs", rel(x, xw))


@pytest.mark.parametrize("restart", [1, 3, 10, 16])
def test_same_bits_as_mgs_fgcr(ctx, mg, c31, restart):
    """1. (status, iterations, resid) and every bit of x, for ahead in {0, 1, 2, 7, 10000}; info; captured cycles; max_iter at and around a window"""
    want, xw = c31.fgcr(restart)
    print(f"mgs_fgcr({restart}) on csky3d(31): {want}")
    h = push_all(mg, ctx, c31.A, c31.Ps, 0.6)
    plan = mg.FgcrPlan(c31.A, h, restart)
    captured = h.graph_info()["captured_cycles"]
    assert captured == restart                                 # one cycle r → C[k] per window slot
    for ahead in AHEADS:
        x = ctx.vec(c31.n)
        got = plan.solve(x, c31.b, 80, 1e-10, ahead)
        info = plan.info()
        print(f"restart {restart}, ahead {ahead}: {got}, info {info}")
        same(got, x.numpy(), want, xw, f"restart {restart}, ahead {ahead}")
        assert info[2] == min(80, want[1] + min(ahead, 1022)) and info[3] == info[2] - want[1]
    # max_iter in {0, 1, 3, restart, restart + 1} at tol 1e-12: status 1 with mgs_fgcr's x
    for max_iter in sorted({0, 1, 3, restart, restart + 1}):
        wm, xm = c31.fgcr(restart, max_iter, 1e-12)
        for ahead in (0, 5):
            y = ctx.vec(c31.n); got = plan.solve(y, c31.b, max_iter, 1e-12, ahead)
            same(got, y.numpy(), wm, xm, f"restart {restart}, max_iter {max_iter}, ahead {ahead}")
            assert got[:2] == (1, max_iter) and plan.info()[2] == max_iter
    if restart <= 10:
        assert h.graph_info()["captured_cycles"] == captured    # the plan's r and C[k] never move
    plan.close()


def test_same_bits_on_views_8_bytes_off(ctx, mg, c31):
    """1. x and b 8 bytes off a 16-byte boundary: the 8-byte arm of the x-pass, against mgs_fgcr on the same views"""
    n = c31.n
    h = push_all(mg, ctx, c31.A, c31.Ps, 0.6)
    plan = mg.FgcrPlan(c31.A, h, 10)
    xb, bb = ctx.vec(n + 2), ctx.vec(n + 2)
    xo, bo = mg.Vec.wrap(ctx, xb.ptr + 8, n), mg.Vec.wrap(ctx, bb.ptr + 8, n)
    assert xo.ptr % 16 == 8
    bo.upload(c31.b_np)
    want8 = mg.fgcr(c31.A, xo, bo, c31.h_ref, 10, 200, 1e-10); xw8 = xo.numpy()
    assert want8[0] == 0
    for ahead in (0, 1, 4):
        xo.fill(0.0)
        got8 = plan.solve(xo, bo, 200, 1e-10, ahead)
        same(got8, xo.numpy(), want8, xw8, f"8-byte views, ahead {ahead}")
    xo.fill(0.0)
    st, done, res = plan.enqueue(xo, bo, want8[1] + 2, 1e-10).result()
    assert done == want8[1] and np.array_equal(xo.numpy(), xw8)
    assert h.graph_info()["captured_cycles"] == 10
    plan.close()


def test_same_bits_with_a_kcycle(ctx, mg, c31):
    """1. restart 10 with set_kcycle(1): first two mgs_fgcr runs agree bit for bit themselves, then the plan agrees with them"""
    want, xw = c31.fgcr(10, kcycle=True)
    x2 = ctx.vec(c31.n); again = mg.fgcr(c31.A, x2, c31.b, c31.hk_ref, 10, 80, 1e-10)
    print(f"mgs_fgcr(10) + K-cycle on csky3d(31): {want}")
    assert again == want and np.array_equal(x2.numpy(), xw)
    h = push_all(mg, ctx, c31.A, c31.Ps, 0.6).set_kcycle(1)
    plan = mg.FgcrPlan(c31.A, h, 10)
    captured = h.graph_info()["captured_cycles"]
    for ahead in AHEADS:
        x = ctx.vec(c31.n)
        got = plan.solve(x, c31.b, 80, 1e-10, ahead)
        info = plan.info()
        print(f"K-cycle, ahead {ahead}: {got}, info {info}")
        same(got, x.numpy(), want, xw, f"K-cycle, ahead {ahead}")
        assert info[2] == min(80, want[1] + min(ahead, 1022)) and info[3] == info[2] - want[1]
    assert h.graph_info()["captured_cycles"] == captured
    plan.close()


def test_same_bits_without_hierarchy(ctx, mg):
    """2. h = NULL on krylov_ref.banded(513): a random x0, a converged x0, b = 0"""
    n = 513
    A = ctx.csr(n, n, *banded(n).csr())
    b = ctx.vec(np.random.default_rng(7).standard_normal(n))
    for restart in (3, 10):
        x = ctx.vec(n); want = mg.fgcr(A, x, b, None, restart, 200, 1e-10); xw = x.numpy()
        assert want[0] == 0 and want[1] >= 5
        plan = mg.FgcrPlan(A, None, restart)
        for ahead in AHEADS:
            y = ctx.vec(n); got = plan.solve(y, b, 200, 1e-10, ahead)
            same(got, y.numpy(), want, xw, f"banded, restart {restart}, ahead {ahead}")
            assert plan.info()[2] == min(200, want[1] + min(ahead, 1022)) and plan.info()[3] == plan.info()[2] - want[1]
        x0 = np.random.default_rng(3).standard_normal(n)
        x = ctx.vec(x0); want0 = mg.fgcr(A, x, b, None, restart, 200, 1e-10)
        y = ctx.vec(x0); got = plan.solve(y, b, 200, 1e-10, 2)
        same(got, y.numpy(), want0, x.numpy(), "random x0")
        # an x0 that already solves the system: (0, 0), x untouched
        xs = ctx.vec(n); mg.fgcr(A, xs, b, None, restart, 400, 1e-13); xs = xs.numpy()
        x = ctx.vec(xs); wants = mg.fgcr(A, x, b, None, restart, 80, 1e-10)
        y = ctx.vec(xs); got = plan.solve(y, b, 80, 1e-10, 3)
        same(got, y.numpy(), wants, xs, "converged x0")
        assert got[:2] == (0, 0) and plan.info()[2:4] == [3, 3]
        # b = 0
        z = ctx.vec(n)
        y = ctx.vec(n); got = plan.solve(y, z, 80, 1e-10)
        assert got == (0, 0, 0.0) and np.array_equal(y.numpy(), np.zeros(n))
        assert got == mg.fgcr(A, ctx.vec(n), z, None, restart, 80, 1e-10)
        plan.close()


def test_same_bits_in_the_8_byte_arm(mg, orc):
    """1. option blas1_vec = 0 in a context of its own: the 8-byte form of the residual pass, its grid and its partial layout (k_update_dot2's other arm)"""
    from multigridsolver_amd.synthetic import csky3d
    c = mg.Context(0)
    plan = h = h_ref = None
    try:
        c.set_option("blas1_vec", 0)
        n = 31 ** 3
        Ao = orc.Csr.from_arrays(n, n, *csky3d(31))
        Ps = explicit_levels(Ao, 3)
        A = dev(c, Ao)
        h_ref = push_all(mg, c, A, Ps, 0.6)
        b = c.vec(orc.rand_rhs(n))
        x = c.vec(n); want = mg.fgcr(A, x, b, h_ref, 10, 200, 1e-10); xw = x.numpy()
        assert want[0] == 0
        h = push_all(mg, c, A, Ps, 0.6)
        plan = mg.FgcrPlan(A, h, 10)
        for ahead in (0, 2, 10000):
            y = c.vec(n); got = plan.solve(y, b, 200, 1e-10, ahead)
            same(got, y.numpy(), want, xw, f"blas1_vec 0, ahead {ahead}")
        y = c.vec(n)
        st, done, res = plan.enqueue(y, b, want[1] + 3, 1e-10).result()
        assert (st, done) == (0, want[1]) and res == want[2] and np.array_equal(y.numpy(), xw)
        assert h.graph_info()["captured_cycles"] == 10
        # h = NULL, 513 rows: three workgroups of the 8-byte sum pass
        B = c.csr(513, 513, *banded(513).csr())
        bb = c.vec(np.random.default_rng(7).standard_normal(513))
        x = c.vec(513); want = mg.fgcr(B, x, bb, None, 3, 200, 1e-10)
        y = c.vec(513); got = mg.FgcrPlan(B, None, 3).solve(y, bb, 200, 1e-10, 1)
        same(got, y.numpy(), want, x.numpy(), "blas1_vec 0, banded")
    finally:
        if plan is not None:
            plan.close()
        del plan, h, h_ref
        c.close()


# the operators of tests/test_fgcr_plan_ref_cpu.py: (name, entries of a block (an empty row carries one explicit zero on its diagonal), block size,
# right-hand side of a block, copies, expected status, expected iterations by restart, expected x of a block)
EXITS = [("converged mid-window", [(0, 0, 2.0), (1, 1, 2.0)], 2, [3.0, -5.0], 257, 0, {2: 1, 10: 1}, [1.5, -2.5]),
         ("breakdown at k = 0", [(0, 1, 1.0), (1, 1, 0.0)], 2, [1.0, 0.0], 257, 2, {2: 1, 10: 1}, [0.0, 0.0]),
         ("breakdown behind an orthogonalisation", [(0, 0, 1.0), (1, 2, 1.0), (2, 2, 0.0)], 3, [1.0, 0.0, 1.0], 171, 2, {2: 4, 10: 3}, [1.0, 1.0, 0.0])]


@pytest.mark.parametrize("restart", [2, 10])
@pytest.mark.parametrize("name,entries,m,rhs,copies,status,its,xblock", EXITS, ids=[e[0] for e in EXITS])
def test_every_exit(ctx, mg, name, entries, m, rhs, copies, status, its, xblock, restart):
    """3. first mgs_fgcr itself returns the expected status and x, then the plan equals it in tuple and bits; the same exit through enqueue + result"""
    n = m * copies
    rows = [[] for _ in range(m)]
    for i, j, v in entries:
        rows[i].append((j, v))
    rp, ci, va = [0], [], []
    for c in range(copies):
        for i in range(m):
            for j, v in sorted(rows[i]):
                ci.append(c * m + j); va.append(v)
            rp.append(len(ci))
    A = ctx.csr(n, n, np.array(rp, dtype=np.int32), np.array(ci, dtype=np.int32), np.array(va))
    b_np = np.tile(np.array(rhs), copies); b = ctx.vec(b_np)
    x = ctx.vec(n); want = mg.fgcr(A, x, b, None, restart, 50, 1e-10); xw = x.numpy()
    print(f"{name}, restart {restart}: mgs_fgcr {want}, x[:3] = {xw[:3]}")
    assert want[:2] == (status, its[restart]) and np.array_equal(xw, np.tile(np.array(xblock), copies))
    if name == "converged mid-window":
        assert want[2] == 0.0
    if name == "breakdown at k = 0":
        assert want[2] == 1.0
    if name == "breakdown behind an orthogonalisation":
        assert abs(want[2] - 1.0 / np.sqrt(2.0)) <= 4 * np.finfo(float).eps
    plan = mg.FgcrPlan(A, None, restart)
    for ahead in (0, 3):
        y = ctx.vec(n); got = plan.solve(y, b, 50, 1e-10, ahead)
        print(f"{name}: plan, ahead {ahead}: {got}, info {plan.info()}")
        same(got, y.numpy(), want, xw, f"{name}, ahead {ahead}")
        assert plan.info()[3] == plan.info()[2] - want[1] and plan.info()[5] == 0
    y = ctx.vec(n)
    st, done, tr, rec = plan.enqueue(y, b, 50, 1e-10).result(recursive=True)
    assert (st, done) == (status, want[1]) and tr == want[2] and np.array_equal(y.numpy(), xw)
    assert plan.info()[3] == 50 - want[1] and plan.info()[4] == 0
    plan.close()


@pytest.mark.parametrize("ahead", [0, 3])
def test_drift(ctx, mg, orc, ahead):
    """4. 2-D Poisson 30² at tol 1e-14, restart 10, no hierarchy: the recursion says converged before the true residual does, and the host
    restarts the window from the true residual; the path must have run, its count is not pinned"""
    Ao = orc.poisson2d(30)
    n = Ao.shape[0]
    assert n == 900
    A = dev(ctx, Ao)
    b = ctx.vec(np.random.default_rng(0).random(n))
    x = ctx.vec(n); want = mg.fgcr(A, x, b, None, 10, 3000, 1e-14); xw = x.numpy()
    plan = mg.FgcrPlan(A, None, 10)
    y = ctx.vec(n); got = plan.solve(y, b, 3000, 1e-14, ahead)
    info = plan.info()
    print(f"drift, ahead {ahead}: mgs_fgcr {want}, plan {got}, info {info}")
    same(got, y.numpy(), want, xw, f"drift, ahead {ahead}")
    assert info[5] >= 1
    plan.close()


def test_enqueue_only(ctx, mg, orc, c31):
    """5."""
    n = c31.n
    want, xw = c31.fgcr(10, 200)          # FGCR(10) + V(1,1) needs more than 80 iterations at 1e-10
    it = want[1]
    assert want[0] == 0 and it < 195
    h = push_all(mg, ctx, c31.A, c31.Ps, 0.6)
    plan = mg.FgcrPlan(c31.A, h, 10)
    x = ctx.vec(n)
    plan.enqueue(x, c31.b, it + 5, 1e-10)
    st, done, res, rec = plan.result(recursive=True)
    info = plan.info()
    tr = np.linalg.norm(c31.Ao.residual(xw, c31.b_np)) / np.linalg.norm(c31.b_np)
    print(f"enqueue(it + 5): {(st, done, res, rec)}, mgs_fgcr {want}, oracle's true residual {tr!r}, info {info}")
    assert done == it
    assert np.array_equal(x.numpy(), xw)
    assert abs(res - tr) <= 1e-12 * tr
    assert st == (0 if res < 1e-10 else 1)
    assert info[2] == it + 5 and info[3] == 5 and info[4] == 0
    # iters = 3: status 1, mgs_fgcr(max_iter = 3)'s x; a second enqueue continues from that x and converges
    want3, xw3 = c31.fgcr(10, 3, 1e-10)
    x3 = ctx.vec(n)
    st, done, res, rec = plan.enqueue(x3, c31.b, 3, 1e-10).result(recursive=True)
    assert (st, done) == (1, 3) and np.array_equal(x3.numpy(), xw3)
    tr3 = np.linalg.norm(c31.Ao.residual(xw3, c31.b_np)) / np.linalg.norm(c31.b_np)
    print(f"enqueue(3): true residual {res!r}, oracle {tr3!r}, mgs_fgcr {want3}")
    assert abs(res - tr3) <= 1e-12 * tr3
    assert plan.info()[3] == 0
    st, done, res = plan.enqueue(x3, c31.b, 200, 1e-10).result()
    print(f"second enqueue from that x: {(st, done, res)}")
    assert st == 0 and done < 200 and res < 1e-10
    assert np.linalg.norm(c31.Ao.residual(x3.numpy(), c31.b_np)) / np.linalg.norm(c31.b_np) < 1e-10
    assert h.graph_info()["captured_cycles"] == 10


def test_enqueue_does_not_wait(mg, orc):
    """6. a busy kernel of about 0.3 s in front on the same stream: enqueue returns while it still runs (size, bar and reasoning of
    test_enqueue_does_not_wait in tests/test_gpu_bicgstab_plan.py: the busy kernel is calibrated with two events, and `still running` is asked of
    an event recorded behind it, so the bar does not depend on how fast the host or the device is)"""
    import torch
    from multigridsolver_amd.synthetic import csky3d
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        c = mg.Context(0, stream.cuda_stream)
        plan = h = None
        try:
            n = 31 ** 3
            Ao = orc.Csr.from_arrays(n, n, *csky3d(31))
            A = dev(c, Ao)
            h = push_all(mg, c, A, explicit_levels(Ao, 3), 0.6)
            b = c.vec(orc.rand_rhs(n))
            plan = mg.FgcrPlan(A, h, 10)
            xw = c.vec(n); want = plan.solve(xw, b, 200, 1e-10, 0)         # warm-up, and the counts of the two extremes of `ahead`
            it = want[1]
            assert want[0] == 0 and plan.info()[4] >= it
            x = c.vec(n); got = plan.solve(x, b, 200, 1e-10, 10000)
            assert got == want and plan.info()[4] <= 4
            x5w = c.vec(n); plan.enqueue(x5w, b, 5, 1e-10).result()
            # the busy kernel: torch's spin kernel, else a chain of the library's own SpMV launches; calibrated once with two events
            if hasattr(torch.cuda, "_sleep"):
                unit, busy = 50_000_000, lambda k: torch.cuda._sleep(int(k))
            else:
                u, v = c.vec(n), c.vec(n)
                unit, busy = 500, lambda k: [A.spmv(u, v) for _ in range(int(k))]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); busy(unit); e1.record(stream); e1.synchronize()
            ms = e0.elapsed_time(e1)
            x5 = c.vec(n)
            stream.synchronize()
            busy(unit * 300.0 / max(ms, 1e-3))
            ev = torch.cuda.Event(); ev.record(stream)
            t0 = time.perf_counter()
            plan.enqueue(x5, b, 5, 1e-10)
            dt = time.perf_counter() - t0
            still_busy = not ev.query()
            st, done, res = plan.result()
            total = time.perf_counter() - t0
            print(f"busy kernel calibrated {ms:.1f} ms per {unit} units; enqueue(5) returned after {dt * 1e3:.2f} ms, busy kernel still running: {still_busy}; "
                  f"result returned after {total * 1e3:.2f} ms")
            assert still_busy
            assert dt < total
            assert (st, done) == (1, 5) and plan.info()[4] == 0
            assert np.array_equal(x5.numpy(), x5w.numpy())
        finally:
            stream.synchronize()
            if plan is not None:
                plan.close()
            del plan, h
            c.close()


def test_nullspace(ctx, mg):
    """7. the pure-Neumann operator and right-hand side of tests/test_gpu_nullspace.py at its smallest size (neumann3d(9), 729 rows), declared
    constant, with hierarchy: mgs_fgcr's bits and a zero-mean x; a hierarchy built for the undeclared twin is refused"""
    import nullspace_ref as ns
    from multigridsolver_amd.synthetic import neumann3d
    N = 9; n = N ** 3
    A = ctx.csr(n, n, *neumann3d(N)).set_nullspace("constant")
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(coarse_rows=60).finalize()
    b_np = ns.project(np.random.default_rng(len("neumann3d_9")).standard_normal(n)); b = ctx.vec(b_np)
    x = ctx.vec(n); want = mg.fgcr(A, x, b, h, 10, 200, 1e-10); xw = x.numpy()
    print(f"null space: mgs_fgcr {want}")
    assert want[0] == 0
    plan = mg.FgcrPlan(A, h, 10)
    for ahead in (0, 1, 4):
        y = ctx.vec(n); got = plan.solve(y, b, 200, 1e-10, ahead)
        same(got, y.numpy(), want, xw, f"null space, ahead {ahead}")
        assert abs(y.numpy().mean()) <= 1e-12 * abs(y.numpy()).max()
    # a guess with a constant component: it is projected out; status 1 at and around a window boundary
    x0 = np.random.default_rng(3).standard_normal(n) + 5.0
    for max_iter, tol in ((200, 1e-10), (0, 1e-12), (3, 1e-12), (10, 1e-12), (11, 1e-12)):
        x = ctx.vec(x0); wantm = mg.fgcr(A, x, b, h, 10, max_iter, tol)
        for ahead in (0, 3):
            y = ctx.vec(x0); got = plan.solve(y, b, max_iter, tol, ahead)
            same(got, y.numpy(), wantm, x.numpy(), f"null space, x0 with a mean, max_iter {max_iter}, ahead {ahead}")
            assert abs(y.numpy().mean()) <= 1e-12 * abs(y.numpy()).max()
    y = ctx.vec(n)
    st, done, res = plan.enqueue(y, b, want[1] + 2, 1e-10).result()
    assert (st, done) == (0, want[1]) and plan.info()[3] == 2
    assert np.array_equal(y.numpy(), xw)
    twin = ctx.csr(n, n, *neumann3d(N))
    refused(mg, INVALID, "null-space", lambda: mg.FgcrPlan(twin, h, 10))
    plan.close()


def refused(mg, code, word, fn):
    with pytest.raises(mg.MgsError) as e:
        fn()
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_refusals(ctx, mg, c31):
    """8. each with a message"""
    shard = ctx.poisson3d(16, 4, 8, local_cols=True)
    refused(mg, INVALID, "row shard", lambda: mg.FgcrPlan(shard))
    n = c31.n
    for restart in (0, 17, -1, 64):
        refused(mg, INVALID, "restart", lambda: mg.FgcrPlan(c31.A, None, restart))
    plan = mg.FgcrPlan(c31.A)
    x, b = ctx.vec(n), ctx.vec(n)
    refused(mg, INVALID, "rows", lambda: plan.solve(ctx.vec(n - 1), b))
    refused(mg, INVALID, "rows", lambda: plan.solve(x, ctx.vec(n - 1)))
    refused(mg, INVALID, "rows", lambda: plan.enqueue(x, ctx.vec(n - 1), 3, 1e-6))
    refused(mg, INVALID, "alias", lambda: plan.solve(x, x))
    refused(mg, INVALID, "alias", lambda: plan.enqueue(x, x, 3, 1e-6))
    refused(mg, INVALID, "ahead", lambda: plan.solve(x, b, ahead=-1))
    refused(mg, INVALID, "iters", lambda: plan.enqueue(x, b, -1, 1e-6))
    # a hierarchy built for the undeclared twin of a declared matrix (the declaration is not verified: any operator serves), and the reverse
    twin = ctx.poisson3d(8)
    h = mg.Hierarchy(twin, 0.6, 1, 1).coarsen(coarse_rows=60).finalize()
    declared = ctx.poisson3d(8).set_nullspace("constant")
    refused(mg, INVALID, "null-space", lambda: mg.FgcrPlan(declared, h))
    from multigridsolver_amd.synthetic import neumann3d
    m = 8 ** 3
    neu = ctx.csr(m, m, *neumann3d(8)).set_nullspace("constant")
    hn = mg.Hierarchy(neu, 0.6, 1, 1).coarsen(coarse_rows=60).finalize()
    refused(mg, INVALID, "null-space", lambda: mg.FgcrPlan(ctx.csr(m, m, *neumann3d(8)), hn))
    # a hierarchy with an exchange callback
    hc = mg.Hierarchy(twin, 0.6, 1, 1).coarsen(coarse_rows=60).finalize()
    hc.set_halo_exchange(lambda level, ptr: None)
    refused(mg, INVALID, "callbacks", lambda: mg.FgcrPlan(twin, hc))
    # a hierarchy of another size; an unfinalized hierarchy (MGS_ERR_STATE)
    refused(mg, INVALID, "rows", lambda: mg.FgcrPlan(c31.A, h))
    refused(mg, STATE, "finalize", lambda: mg.FgcrPlan(twin, mg.Hierarchy(twin, 0.6, 1, 1)))
    # NULL arguments
    L = mg.lib()
    assert L.mgs_fgcr_plan_create(None, None, 10, None) == INVALID
    assert L.mgs_fgcr_plan_create(c31.A.h, None, 10, None) == INVALID
    assert L.mgs_fgcr_plan_solve(None, x.h, b.h, 0, None, None, None) == INVALID
    assert L.mgs_fgcr_plan_solve(plan.h, x.h, b.h, 0, None, None, None) == INVALID
    assert L.mgs_fgcr_plan_enqueue(plan.h, None, b.h, 1, 1e-6) == INVALID
    assert L.mgs_fgcr_plan_result(None, None, None, None, None) == INVALID
    assert L.mgs_fgcr_plan_info(plan.h, None) == INVALID
    assert L.mgs_fgcr_plan_destroy(None) == 0
    # a matrix without rows (where the upload accepts one)
    try:
        empty = ctx.csr(0, 0, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    except mg.MgsError:
        empty = None
    if empty is not None:
        refused(mg, INVALID, "no rows", lambda: mg.FgcrPlan(empty))
    # result before anything was solved or enqueued
    refused(mg, STATE, "nothing", lambda: plan.result())
    # a context that sums over ranks
    c2 = mg.Context(0)
    try:
        c2.set_allreduce(lambda a: None)
        A2c = c2.poisson3d(8)
        refused(mg, INVALID, "sums over ranks", lambda: mg.FgcrPlan(A2c))
        del A2c
    finally:
        c2.close()


def test_refused_while_the_stream_is_captured(mg):
    """8. MGS_ERR_STATE from solve and enqueue while the context's stream is being captured; nothing is launched, and the plan serves afterwards"""
    import torch
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        c = mg.Context(0, stream.cuda_stream)
        plan = None
        try:
            n = 513
            A = c.csr(n, n, *banded(n).csr())
            b = c.vec(np.random.default_rng(7).standard_normal(n))
            x = c.vec(n)
            plan = mg.FgcrPlan(A)
            want = plan.solve(x, b, 200, 1e-10)
            xw = x.numpy()
            t = torch.zeros(64, device="cuda")
            stream.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
                t.add_(1.0)
                refused(mg, STATE, "captured", lambda: plan.solve(x, b, 200, 1e-10))
                refused(mg, STATE, "captured", lambda: plan.enqueue(x, b, 3, 1e-10))
            stream.synchronize()
            y = c.vec(n)
            assert plan.solve(y, b, 200, 1e-10) == want and np.array_equal(y.numpy(), xw)
        finally:
            stream.synchronize()
            if plan is not None:
                plan.close()
            del plan
            c.close()


def test_determinism(ctx, mg, c31):
    """9. two identical solves and two identical enqueues: identical bits, identical result and identical info()[2:4]"""
    n = c31.n
    h = push_all(mg, ctx, c31.A, c31.Ps, 0.6)
    plan = mg.FgcrPlan(c31.A, h, 10)
    runs = []
    for _ in range(2):
        x = ctx.vec(n); r = plan.solve(x, c31.b, 80, 1e-10, 2)
        runs.append((r, x.numpy(), plan.info()[2:4], plan.result(recursive=True)))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2] and runs[0][3] == runs[1][3]
    assert runs[0][3][:3] == runs[0][0]                     # after a solve, result returns what that solve returned
    runs = []
    for _ in range(2):
        x = ctx.vec(n); r = plan.enqueue(x, c31.b, 30, 1e-10).result(recursive=True)
        runs.append((r, x.numpy(), plan.info()[2:4]))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
