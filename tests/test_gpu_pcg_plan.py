"""mgs_pcg_plan on the device against mgs_pcg on the same device: the plan promises mgs_pcg's contract and mgs_pcg's BITS, for every
`ahead`, and an enqueue-only form that never waits for the device.  Every comparison below is exact ((status, iterations, resid) equal,
np.array_equal on x) except where the enqueue-only form reports the true residual, which is held against the oracle's recomputation.
Shapes are the smallest on which each path can go wrong: poisson3d(31) has an odd number of rows (the tail element of the 16-byte forms)
and 117 row blocks; poisson2d(30) without preconditioner reaches the restart branch (tests/test_pcg_plan_ref_cpu.py probes it on the CPU)."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID = -1      # MGS_ERR_INVALID


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


class P31:
    """poisson3d(31), three levels of explicit P, ω = 0.6: one hierarchy for mgs_pcg (the reference side) and one for the plans, so that the
    plans' captured cycles can be counted; the mgs_pcg results are computed once and shared"""

    def __init__(self, mg, ctx, orc):
        self.Ao = orc.poisson3d(31); self.n = self.Ao.shape[0]
        assert self.n % 2 == 1
        self.Ps = explicit_levels(self.Ao, 3)
        self.A = dev(ctx, self.Ao)
        self.h_ref = push_all(mg, ctx, self.A, self.Ps, 0.6)
        self.b_np = orc.rand_rhs(self.n); self.b = ctx.vec(self.b_np)
        self.ref = {}
        self.mg, self.ctx = mg, ctx

    def pcg(self, flexible=False, max_iter=60, tol=1e-10, x0=None, b=None):
        key = (flexible, max_iter, tol, None if x0 is None else x0.tobytes()[:64], id(b))
        if key not in self.ref:
            x = self.ctx.vec(self.n if x0 is None else x0)
            r = self.mg.pcg(self.A, x, self.b if b is None else b, self.h_ref, max_iter, tol, flexible)
            self.ref[key] = (r, x.numpy())
        return self.ref[key]


_p31 = {}


@pytest.fixture
def p31(mg, ctx, orc):
    if "p" not in _p31:
        _p31["p"] = P31(mg, ctx, orc)
    return _p31["p"]


@pytest.fixture(scope="module", autouse=True)
def _release(ctx):
    yield
    _p31.clear()      # before the context closes


def same(got, x, want, xw, label=""):
    assert got == want, (label, got, want)
    assert np.array_equal(x, xw), (label, "x differs", rel(x, xw))


@pytest.mark.parametrize("flexible", [False, True])
def test_same_bits_as_mgs_pcg(ctx, mg, p31, flexible):
    """1. (status, iterations, resid) and every bit of x, for ahead in {0, 1, 2, 7, 10000}; one captured cycle; the 8-byte forms"""
    want, xw = p31.pcg(flexible)
    assert want[0] == 0 and 5 < want[1] < 60
    h = push_all(mg, ctx, p31.A, p31.Ps, 0.6)
    plan = mg.PcgPlan(p31.A, h, flexible)
    for ahead in (0, 1, 2, 7, 10000):
        x = ctx.vec(p31.n)
        got = plan.solve(x, p31.b, 60, 1e-10, ahead)
        info = plan.info()
        print(f"flexible {int(flexible)} ahead {ahead}: {got}, info {info}")
        same(got, x.numpy(), want, xw, f"ahead {ahead}")
        assert info[2] == min(60, want[1] + min(ahead, 1022)) and info[3] == info[2] - want[1] and info[5] == 0
    assert h.graph_info()["captured_cycles"] == 1          # the plan's r and z never move
    # x and b 8 bytes off a 16-byte boundary: the 8-byte forms of direction and flush, against mgs_pcg on the same views
    n = p31.n
    xb, bb = ctx.vec(n + 2), ctx.vec(n + 2)
    xo, bo = mg.Vec.wrap(ctx, xb.ptr + 8, n), mg.Vec.wrap(ctx, bb.ptr + 8, n)
    assert xo.ptr % 16 == 8
    bo.upload(p31.b_np)
    want8 = mg.pcg(p31.A, xo, bo, p31.h_ref, 60, 1e-10, flexible); xw8 = xo.numpy()
    xo.fill(0.0)
    got8 = plan.solve(xo, bo, 60, 1e-10, 1)
    same(got8, xo.numpy(), want8, xw8, "8-byte views")
    assert want8[0] == 0


def test_every_status(ctx, mg, orc, p31):
    """2. each against mgs_pcg with equal bits"""
    Po = orc.poisson2d(30); n = Po.shape[0]
    No = orc.Csr.from_scipy(-Po.to_scipy())
    Nd = dev(ctx, No)
    b = ctx.vec(orc.rand_rhs(n))
    for ahead in (0, 2):
        x = ctx.vec(n); want = mg.pcg(Nd, x, b, None, 50, 1e-8)
        y = ctx.vec(n); got = mg.PcgPlan(Nd).solve(y, b, 50, 1e-8, ahead)
        same(got, y.numpy(), want, x.numpy(), "negated operator")
        assert got[:2] == (3, 1) and np.array_equal(y.numpy(), np.zeros(n))
        Pagg = Po.agmg(10.0, 2, 8.0)
        h = push_all(mg, ctx, Nd, [Pagg], 0.6)
        x = ctx.vec(n); want = mg.pcg(Nd, x, b, h, 50, 1e-8)
        y = ctx.vec(n); got = mg.PcgPlan(Nd, h).solve(y, b, 50, 1e-8, ahead)
        same(got, y.numpy(), want, x.numpy(), "negative definite preconditioner")
        assert got[:2] == (2, 1)
    h = push_all(mg, ctx, p31.A, p31.Ps, 0.6)
    n = p31.n
    for flexible in (False, True):
        plan = mg.PcgPlan(p31.A, h, flexible)
        for max_iter in (3, 4):
            want, xw = p31.pcg(flexible, max_iter, 1e-12)
            for ahead in (0, 1, 5):
                y = ctx.vec(n); got = plan.solve(y, p31.b, max_iter, 1e-12, ahead)
                same(got, y.numpy(), want, xw, f"max_iter {max_iter} flexible {flexible} ahead {ahead}")
                assert got[:2] == (1, max_iter) and plan.info()[2] == max_iter
    plan = mg.PcgPlan(p31.A, h)
    x0 = orc.rand_rhs(n, seed=3)
    want, xw = p31.pcg(False, 60, 1e-10, x0=x0)
    y = ctx.vec(x0); got = plan.solve(y, p31.b, 60, 1e-10)
    same(got, y.numpy(), want, xw, "random x0")
    assert got[0] == 0
    # a converged x0: (0, 0), x untouched
    xs = y.numpy()
    x = ctx.vec(xs); want = mg.pcg(p31.A, x, p31.b, p31.h_ref, 60, 1e-10)
    got = plan.solve(y, p31.b, 60, 1e-10, 3)
    same(got, y.numpy(), want, xs, "converged x0")
    assert got[:2] == (0, 0)
    # b = 0
    z = ctx.vec(n)
    y = ctx.vec(n); got = plan.solve(y, z, 60, 1e-10)
    assert got == (0, 0, 0.0) and np.array_equal(y.numpy(), np.zeros(n))
    assert got == mg.pcg(p31.A, ctx.vec(n), z, p31.h_ref, 60, 1e-10)


@pytest.mark.parametrize("tol", [1e-14, 1e-15])
def test_restart_branch(ctx, mg, orc, tol):
    """3. the recursion says converged, the true residual does not: restart from it, as mgs_pcg does"""
    Ao = orc.poisson2d(30); n = Ao.shape[0]
    A = dev(ctx, Ao)
    b = ctx.vec(orc.rand_rhs(n))
    x = ctx.vec(n); want = mg.pcg(A, x, b, None, 400, tol); xw = x.numpy()
    plan = mg.PcgPlan(A)
    for ahead in (0, 3):
        y = ctx.vec(n); got = plan.solve(y, b, 400, tol, ahead)
        info = plan.info()
        print(f"tol {tol:g} ahead {ahead}: {got}, info {info}")
        same(got, y.numpy(), want, xw, f"ahead {ahead}")
        assert info[5] >= 1


def test_enqueue_only(ctx, mg, orc, p31):
    """4."""
    n = p31.n
    want, xw = p31.pcg(False)
    it = want[1]
    h = push_all(mg, ctx, p31.A, p31.Ps, 0.6)
    plan = mg.PcgPlan(p31.A, h)
    x = ctx.vec(n)
    plan.enqueue(x, p31.b, it + 5, 1e-10)
    st, done, res = plan.result()
    info = plan.info()
    print(f"enqueue(it + 5): {(st, done, res)}, mgs_pcg {want}, info {info}")
    assert (st, done) == (0, it) and res < 1e-10
    assert np.array_equal(x.numpy(), xw)
    assert info[2] == it + 5 and info[3] == 5 and info[4] == 0
    # iters = 3: status 1, mgs_pcg(max_iter = 3)'s x, the true residual
    want3, xw3 = p31.pcg(False, 3, 1e-10)
    x3 = ctx.vec(n)
    st, done, res = plan.enqueue(x3, p31.b, 3, 1e-10).result()
    assert (st, done) == (1, 3) and np.array_equal(x3.numpy(), xw3)
    tr = np.linalg.norm(p31.Ao.residual(xw3, p31.b_np)) / np.linalg.norm(p31.b_np)
    assert abs(res - tr) <= 1e-8 * tr
    assert plan.info()[3] == 0
    # two enqueues with different (x, b) before one result
    b2_np = orc.rand_rhs(n, seed=5); b2 = ctx.vec(b2_np)
    x2w = ctx.vec(n); want2 = mg.pcg(p31.A, x2w, b2, p31.h_ref, 60, 1e-10)
    xa, xb = ctx.vec(n), ctx.vec(n)
    plan.enqueue(xa, p31.b, it + 1, 1e-10)
    plan.enqueue(xb, b2, want2[1], 1e-10)
    st, done, res = plan.result()
    assert (st, done) == (0, want2[1])
    assert np.array_equal(xa.numpy(), xw) and np.array_equal(xb.numpy(), x2w.numpy())
    assert h.graph_info()["captured_cycles"] == 1


def test_enqueue_does_not_wait(mg, orc):
    """5. a busy kernel of about 0.3 s in front on the same stream: enqueue returns while it still runs"""
    import torch
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        c = mg.Context(0, stream.cuda_stream)
        plan = h = None
        try:
            Ao = orc.poisson3d(31); n = Ao.shape[0]
            A = dev(c, Ao)
            h = push_all(mg, c, A, explicit_levels(Ao, 3), 0.6)
            b = c.vec(orc.rand_rhs(n))
            plan = mg.PcgPlan(A, h)
            xw = c.vec(n); want = plan.solve(xw, b, 60, 1e-10, 0)          # warm-up, and the counts of the two extremes of `ahead`
            it = want[1]
            assert want[0] == 0 and plan.info()[4] >= it
            x = c.vec(n); got = plan.solve(x, b, 60, 1e-10, 10000)
            assert got == want and plan.info()[4] <= plan.info()[5] + 2
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
            print(f"busy kernel calibrated {ms:.1f} ms per {unit} units; enqueue(5) returned after {dt * 1e3:.2f} ms, busy kernel still running: {still_busy}")
            assert still_busy
            assert (st, done) == (1, 5) and plan.info()[4] == 0
            assert np.array_equal(x5.numpy(), x5w.numpy())
        finally:
            stream.synchronize()
            del plan, h
            c.close()


def test_nullspace(ctx, mg):
    """6. neumann3d(12) declared constant, device-built hierarchy"""
    from multigridsolver_amd.synthetic import neumann3d
    N = 12; n = N ** 3
    A = ctx.csr(n, n, *neumann3d(N)).set_nullspace("constant")
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(coarse_rows=60).finalize()
    b = ctx.vec(np.random.default_rng(12).standard_normal(n))
    x = ctx.vec(n); want = mg.pcg(A, x, b, h, 200, 1e-10); xw = x.numpy()
    assert want[0] == 0
    plan = mg.PcgPlan(A, h)
    for ahead in (0, 1, 4):
        y = ctx.vec(n); got = plan.solve(y, b, 200, 1e-10, ahead)
        same(got, y.numpy(), want, xw, f"null space, ahead {ahead}")
        assert abs(y.numpy().mean()) <= 1e-12 * abs(y.numpy()).max()
    y = ctx.vec(n)
    st, done, res = plan.enqueue(y, b, want[1] + 2, 1e-10).result()
    assert (st, done) == (0, want[1]) and res < 1e-10 and plan.info()[3] == 2
    assert np.array_equal(y.numpy(), xw)
    assert abs(y.numpy().mean()) <= 1e-12 * abs(y.numpy()).max()
    # a random x0 carries a mean: it is projected out
    x0 = np.random.default_rng(3).standard_normal(n) + 5.0
    x = ctx.vec(x0); want = mg.pcg(A, x, b, h, 200, 1e-10)
    y = ctx.vec(x0); got = plan.solve(y, b, 200, 1e-10)
    same(got, y.numpy(), want, x.numpy(), "null space, x0 with a mean")


def test_kcycle(ctx, mg, orc):
    """7. poisson3d(32), four levels, K-cycle on levels 1..2 with energy coefficients"""
    Ao = orc.poisson3d(32); n = Ao.shape[0]
    A = dev(ctx, Ao)
    Ps = explicit_levels(Ao, 4)
    b = ctx.vec(orc.rand_rhs(n))
    hk = push_all(mg, ctx, A, Ps, 0.6).set_kcycle(2)
    ctx.set_option("kcycle_energy", 1)
    try:
        with pytest.raises(mg.MgsError) as e:
            mg.PcgPlan(A, hk, False)
        assert e.value.code == INVALID and "flexible" in str(e.value)
        x = ctx.vec(n); want = mg.pcg(A, x, b, hk, 100, 1e-10, True)
        assert want[0] == 0
        plan = mg.PcgPlan(A, hk, True)
        for ahead in (0, 2):
            y = ctx.vec(n); got = plan.solve(y, b, 100, 1e-10, ahead)
            same(got, y.numpy(), want, x.numpy(), f"K-cycle, ahead {ahead}")
    finally:
        ctx.set_option("kcycle_energy", 0)


def test_refusals(ctx, mg, p31):
    """8. each with a message"""
    def refused(code, word, fn):
        with pytest.raises(mg.MgsError) as e:
            fn()
        assert e.value.code == code and word in str(e.value), str(e.value)
    shard = ctx.poisson3d(16, 4, 8, local_cols=True)
    refused(INVALID, "row shard", lambda: mg.PcgPlan(shard))
    n = p31.n
    plan = mg.PcgPlan(p31.A)
    x, b = ctx.vec(n), ctx.vec(n)
    refused(INVALID, "rows", lambda: plan.solve(ctx.vec(n - 1), b))
    refused(INVALID, "rows", lambda: plan.enqueue(x, ctx.vec(n - 1), 3, 1e-6))
    refused(INVALID, "alias", lambda: plan.solve(x, x))
    refused(INVALID, "alias", lambda: plan.enqueue(x, x, 3, 1e-6))
    refused(INVALID, "ahead", lambda: plan.solve(x, b, ahead=-1))
    refused(INVALID, "iters", lambda: plan.enqueue(x, b, -1, 1e-6))
    # a hierarchy built for the undeclared twin of a declared matrix (the declaration is not verified: any operator serves), and the reverse
    twin = ctx.poisson3d(8)
    h = mg.Hierarchy(twin, 0.6, 1, 1).coarsen(coarse_rows=60).finalize()
    declared = ctx.poisson3d(8).set_nullspace("constant")
    refused(INVALID, "null-space", lambda: mg.PcgPlan(declared, h))
    from multigridsolver_amd.synthetic import neumann3d
    m = 8 ** 3
    neu = ctx.csr(m, m, *neumann3d(8)).set_nullspace("constant")
    hn = mg.Hierarchy(neu, 0.6, 1, 1).coarsen(coarse_rows=60).finalize()
    refused(INVALID, "null-space", lambda: mg.PcgPlan(ctx.csr(m, m, *neumann3d(8)), hn))
    # an unfinalized hierarchy (MGS_ERR_STATE)
    refused(-6, "finalize", lambda: mg.PcgPlan(twin, mg.Hierarchy(twin, 0.6, 1, 1)))
    assert mg.lib().mgs_pcg_plan_create(None, None, 0, None) == INVALID


def test_determinism(ctx, mg, p31):
    """9. two identical solves and two identical enqueues: identical bits and identical info()[2:4]"""
    n = p31.n
    h = push_all(mg, ctx, p31.A, p31.Ps, 0.6)
    plan = mg.PcgPlan(p31.A, h)
    runs = []
    for _ in range(2):
        x = ctx.vec(n); r = plan.solve(x, p31.b, 60, 1e-10, 2)
        runs.append((r, x.numpy(), plan.info()[2:4]))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    runs = []
    for _ in range(2):
        x = ctx.vec(n); r = plan.enqueue(x, p31.b, 30, 1e-10).result()
        runs.append((r, x.numpy(), plan.info()[2:4]))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]


def test_close(ctx, mg):
    """10. close() twice, then letting the object go, raises nothing; a fresh plan on the same matrix solves to the same bits as before"""
    A = ctx.poisson3d(8); n = 8 ** 3
    b = ctx.vec(n).rand(seed=0)
    plan = mg.PcgPlan(A)
    x = ctx.vec(n); want = plan.solve(x, b, 200, 1e-10); xw = x.numpy()
    assert want[0] == 0 and want[1] > 1
    plan.close()
    plan.close()
    assert not plan.h
    del plan
    fresh = mg.PcgPlan(A)
    y = ctx.vec(n); got = fresh.solve(y, b, 200, 1e-10)
    same(got, y.numpy(), want, xw, "fresh plan")
    fresh.close()
