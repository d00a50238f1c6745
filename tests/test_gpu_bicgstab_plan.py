"""mgs_bicgstab_plan on the device against mgs_bicgstab on the same device: the plan promises mgs_bicgstab's contract and mgs_bicgstab's BITS,
for every `ahead`, and an enqueue-only form that never waits for the device.  Every comparison below is exact ((status, iterations, resid)
equal, np.array_equal on x) except where the enqueue-only form reports the true residual, which is held against the oracle's recomputation.
Shapes are the smallest on which each path can go wrong: csky3d(31) is nonsymmetric, has an odd number of rows (the tail element of the
16-byte forms) and 117 row blocks; the exits of bicg.cpp:74-136 are reached with block-diagonal copies of the small operators of
tests/test_bicgstab_plan_ref_cpu.py, whose dyadic values keep every sum exact in any order."""
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
    """csky3d(31), three levels of explicit P, ω = 0.6: one hierarchy for mgs_bicgstab (the reference side) and fresh ones for the plans, so
    that the plans' captured cycles can be counted; the mgs_bicgstab results are computed once and shared"""

    def __init__(self, mg, ctx, orc):
        from multigridsolver_amd.synthetic import csky3d
        n = 31 ** 3
        self.Ao = orc.Csr.from_arrays(n, n, *csky3d(31)); self.n = n
        assert self.n % 2 == 1
        self.Ps = explicit_levels(self.Ao, 3)
        self.A = dev(ctx, self.Ao)
        self.h_ref = push_all(mg, ctx, self.A, self.Ps, 0.6)
        self.b_np = orc.rand_rhs(self.n); self.b = ctx.vec(self.b_np)
        self.ref = {}
        self.mg, self.ctx = mg, ctx

    def bicgstab(self, max_iter=80, tol=1e-10):
        key = (max_iter, tol)
        if key not in self.ref:
            x = self.ctx.vec(self.n)
            r = self.mg.bicgstab(self.A, x, self.b, self.h_ref, max_iter, tol)
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


def test_same_bits_as_mgs_bicgstab(ctx, mg, c31):
    """1. (status, iterations, resid) and every bit of x, for ahead in {0, 1, 2, 7, 10000}; info; two captured cycles; views 8 bytes off"""
    want, xw = c31.bicgstab()
    print(f"mgs_bicgstab on csky3d(31): {want}")
    assert want[0] == 0 and 5 < want[1] < 80
    h = push_all(mg, ctx, c31.A, c31.Ps, 0.6)
    plan = mg.BicgstabPlan(c31.A, h)
    assert h.graph_info()["captured_cycles"] == 2
    for ahead in AHEADS:
        x = ctx.vec(c31.n)
        got = plan.solve(x, c31.b, 80, 1e-10, ahead)
        info = plan.info()
        print(f"ahead {ahead}: {got}, info {info}")
        same(got, x.numpy(), want, xw, f"ahead {ahead}")
        assert info[2] == min(80, want[1] + min(ahead, 1022)) and info[3] == info[2] - want[1] and info[5] == 0
    assert h.graph_info()["captured_cycles"] == 2          # the plan's p, p̂, s, ŝ never move
    # x and b 8 bytes off a 16-byte boundary: the 8-byte form of the x-pass, against mgs_bicgstab on the same views
    n = c31.n
    xb, bb = ctx.vec(n + 2), ctx.vec(n + 2)
    xo, bo = mg.Vec.wrap(ctx, xb.ptr + 8, n), mg.Vec.wrap(ctx, bb.ptr + 8, n)
    assert xo.ptr % 16 == 8
    bo.upload(c31.b_np)
    want8 = mg.bicgstab(c31.A, xo, bo, c31.h_ref, 80, 1e-10); xw8 = xo.numpy()
    xo.fill(0.0)
    got8 = plan.solve(xo, bo, 80, 1e-10, 1)
    same(got8, xo.numpy(), want8, xw8, "8-byte views")
    assert want8[0] == 0
    assert h.graph_info()["captured_cycles"] == 2
    # max_iter in {0, 1, 3}: status 1, *max_iter as given
    for max_iter in (0, 1, 3):
        wm, xm = c31.bicgstab(max_iter, 1e-12)
        for ahead in (0, 5):
            y = ctx.vec(n); got = plan.solve(y, c31.b, max_iter, 1e-12, ahead)
            same(got, y.numpy(), wm, xm, f"max_iter {max_iter} ahead {ahead}")
            assert got[:2] == (1, max_iter) and plan.info()[2] == max_iter
    plan.close()


def test_same_bits_without_hierarchy(ctx, mg):
    """1. h = NULL on krylov_ref.banded(513): a random x0, a converged x0, b = 0"""
    n = 513
    A = ctx.csr(n, n, *banded(n).csr())
    b = ctx.vec(np.random.default_rng(7).standard_normal(n))
    x = ctx.vec(n); want = mg.bicgstab(A, x, b, None, 80, 1e-10); xw = x.numpy()
    assert want[0] == 0 and 5 <= want[1] <= 60
    plan = mg.BicgstabPlan(A)
    for ahead in AHEADS:
        y = ctx.vec(n); got = plan.solve(y, b, 80, 1e-10, ahead)
        same(got, y.numpy(), want, xw, f"banded, ahead {ahead}")
        assert plan.info()[2] == min(80, want[1] + min(ahead, 1022)) and plan.info()[3] == plan.info()[2] - want[1]
    x0 = np.random.default_rng(3).standard_normal(n)
    x = ctx.vec(x0); want0 = mg.bicgstab(A, x, b, None, 80, 1e-10)
    y = ctx.vec(x0); got = plan.solve(y, b, 80, 1e-10, 2)
    same(got, y.numpy(), want0, x.numpy(), "random x0")
    # an x0 that already solves the system: (0, 0), x untouched
    xs = ctx.vec(n); mg.bicgstab(A, xs, b, None, 200, 1e-12); xs = xs.numpy()
    x = ctx.vec(xs); wants = mg.bicgstab(A, x, b, None, 80, 1e-10)
    y = ctx.vec(xs); got = plan.solve(y, b, 80, 1e-10, 3)
    same(got, y.numpy(), wants, xs, "converged x0")
    assert got[:2] == (0, 0) and plan.info()[2:4] == [3, 3]
    # b = 0
    z = ctx.vec(n)
    y = ctx.vec(n); got = plan.solve(y, z, 80, 1e-10)
    assert got == (0, 0, 0.0) and np.array_equal(y.numpy(), np.zeros(n))
    assert got == mg.bicgstab(A, ctx.vec(n), z, None, 80, 1e-10)


def test_same_bits_in_the_8_byte_arm(mg, orc):
    """1. option blas1_vec = 0 in a context of its own: the 8-byte forms of every pass, their grids and their partial layout"""
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
        x = c.vec(n); want = mg.bicgstab(A, x, b, h_ref, 80, 1e-10); xw = x.numpy()
        assert want[0] == 0
        h = push_all(mg, c, A, Ps, 0.6)
        plan = mg.BicgstabPlan(A, h)
        for ahead in (0, 2, 10000):
            y = c.vec(n); got = plan.solve(y, b, 80, 1e-10, ahead)
            same(got, y.numpy(), want, xw, f"blas1_vec 0, ahead {ahead}")
        assert h.graph_info()["captured_cycles"] == 2
        # h = NULL, 513 rows: three workgroups of the 8-byte sum passes
        B = c.csr(513, 513, *banded(513).csr())
        bb = c.vec(np.random.default_rng(7).standard_normal(513))
        x = c.vec(513); want = mg.bicgstab(B, x, bb, None, 80, 1e-10)
        y = c.vec(513); got = mg.BicgstabPlan(B).solve(y, bb, 80, 1e-10, 1)
        same(got, y.numpy(), want, x.numpy(), "blas1_vec 0, banded")
    finally:
        if plan is not None:
            plan.close()
        del plan, h, h_ref
        c.close()


# the operators of tests/test_bicgstab_plan_ref_cpu.py: (name, block, right-hand side of a block, copies, expected status, expected iterations or None)
I2 = [[2.0, 0.0], [0.0, 2.0]]
A2 = [[-2.0, -2.0], [-2.0, 0.0]]
A3 = [[-2.0, -2.0, -2.0], [-2.0, -2.0, -1.0], [-2.0, -1.0, -2.0]]
A3D = [[-2.0, -2.0, -2.0], [-2.0, -2.0, -2.0], [-2.0, 2.0, 0.0]]
EXITS = [("half step", I2, [3.0, -5.0], 257, 0, 1),
         ("status 3", A2, [1.0, 0.0], 257, 3, None),
         ("NaN", A2, [0.0, 1.0], 257, 1, None),
         ("status 2 or 3", A3, [2.0, 1.0, 1.0], 171, (2, 3), None),
         ("status 2", A3D, [0.0, 1.0, 0.0], 171, 2, None)]
# "status 2 or 3": α = −0.2 is not dyadic, so which zero the rounded arithmetic meets depends on the order of the sums — exactly, t·s = 0 at
# iteration 1 (ω = 0, status 3); numpy's dot leaves t·s = 1.3e-17 and meets ρ = 0 two iterations later (status 2,
# tests/test_bicgstab_plan_ref_cpu.py); the device's folds give t·s = 0.  Either way x = (−0.4, −0.2, −0.2) and resid = 0.2·√2, and the plan has
# to take the exit mgs_bicgstab takes.  "status 2" (α = −1/2, ω = 1/2, r = (−1, 0, 0) ⟂ r̃ at iteration 2) is dyadic throughout: ρ = 0 in any order.


@pytest.mark.parametrize("name,block,rhs,copies,status,its", EXITS, ids=[e[0] for e in EXITS])
def test_every_exit(ctx, mg, name, block, rhs, copies, status, its):
    """2. first mgs_bicgstab itself returns the expected status, then the plan equals it in tuple and bits, *max_iter untouched on 2 and 3"""
    import scipy.sparse as sp
    M = sp.kron(sp.identity(copies), sp.csr_matrix(np.array(block)), format="csr")
    M.eliminate_zeros(); M.sort_indices()
    n = M.shape[0]
    A = ctx.csr(n, n, M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data)
    b_np = np.tile(np.array(rhs), copies); b = ctx.vec(b_np)
    max_iter = 6 if name == "NaN" else 50
    x = ctx.vec(n); want = mg.bicgstab(A, x, b, None, max_iter, 1e-10); xw = x.numpy()
    print(f"{name}: mgs_bicgstab {want}, x[:3] = {xw[:3]}")
    assert want[0] == status or (isinstance(status, tuple) and want[0] in status), (name, want)
    status = want[0]
    if its is not None:
        assert want[1] == its
    if status in (2, 3):
        assert want[1] == max_iter                      # *max_iter untouched
    if name == "half step":
        assert want[2] == 0.0 and np.array_equal(xw, 0.5 * b_np)
    if name == "status 3":
        assert want[2] == 1.0 and np.array_equal(xw, np.tile([-0.5, 0.0], copies))
    if name == "NaN":
        assert np.isnan(want[2]) and np.isnan(xw).all()
    if name == "status 2 or 3":
        assert np.allclose(xw, np.tile([-0.4, -0.2, -0.2], copies), rtol=1e-14, atol=0) and abs(want[2] - 0.2 * np.sqrt(2.0)) < 1e-14
    if name == "status 2":
        assert want[2] == 1.0 and np.array_equal(xw, np.tile([-0.5, -0.5, 0.5], copies))
    plan = mg.BicgstabPlan(A)
    for ahead in (0, 3):
        y = ctx.vec(n); got = plan.solve(y, b, max_iter, 1e-10, ahead)
        print(f"{name}: plan, ahead {ahead}: {got}, info {plan.info()}")
        same(got, y.numpy(), want, xw, f"{name}, ahead {ahead}")
    # the same exit through enqueue + result
    y = ctx.vec(n)
    st, done, tr, rec = plan.enqueue(y, b, max_iter, 1e-10).result(recursive=True)
    assert st == status and np.array_equal(y.numpy(), xw, equal_nan=True)
    assert rec == want[2] or (np.isnan(rec) and np.isnan(want[2]))
    if status == 0:
        assert done == want[1]
    if name == "status 2":
        assert done == 2
    if name == "status 3":
        assert done == 1


def test_enqueue_only(ctx, mg, orc, c31):
    """3."""
    n = c31.n
    want, xw = c31.bicgstab()
    it = want[1]
    h = push_all(mg, ctx, c31.A, c31.Ps, 0.6)
    plan = mg.BicgstabPlan(c31.A, h)
    x = ctx.vec(n)
    plan.enqueue(x, c31.b, it + 5, 1e-10)
    st, done, res, rec = plan.result(recursive=True)
    info = plan.info()
    tr = np.linalg.norm(c31.Ao.residual(xw, c31.b_np)) / np.linalg.norm(c31.b_np)
    print(f"enqueue(it + 5): {(st, done, res, rec)}, mgs_bicgstab {want}, oracle's true residual {tr!r}, info {info}")
    assert done == it and rec == want[2]
    assert np.array_equal(x.numpy(), xw)
    assert abs(res - tr) <= 1e-12 * tr
    assert st == (0 if res < 1e-10 else 1)
    assert info[2] == it + 5 and info[3] == 5 and info[4] == 0
    # iters = 3: status 1, mgs_bicgstab(max_iter = 3)'s x; a second enqueue continues from that x and converges
    want3, xw3 = c31.bicgstab(3, 1e-10)
    x3 = ctx.vec(n)
    st, done, res, rec = plan.enqueue(x3, c31.b, 3, 1e-10).result(recursive=True)
    assert (st, done) == (1, 3) and rec == want3[2] and np.array_equal(x3.numpy(), xw3)
    tr3 = np.linalg.norm(c31.Ao.residual(xw3, c31.b_np)) / np.linalg.norm(c31.b_np)
    print(f"enqueue(3): true residual {res!r}, oracle {tr3!r}")
    assert abs(res - tr3) <= 1e-12 * tr3
    assert plan.info()[3] == 0
    st, done, res = plan.enqueue(x3, c31.b, 80, 1e-10).result()
    print(f"second enqueue from that x: {(st, done, res)}")
    assert st == 0 and done < 80 and res < 1e-10
    assert np.linalg.norm(c31.Ao.residual(x3.numpy(), c31.b_np)) / np.linalg.norm(c31.b_np) < 1e-10
    assert h.graph_info()["captured_cycles"] == 2


def test_enqueue_does_not_wait(mg, orc):
    """4. a busy kernel of about 0.3 s in front on the same stream: enqueue returns while it still runs (size, bar and reasoning of
    test_enqueue_does_not_wait in tests/test_gpu_pcg_plan.py: the busy kernel is calibrated with two events, and `still running` is asked of an
    event recorded behind it, so the bar does not depend on how fast the host or the device is)"""
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
            plan = mg.BicgstabPlan(A, h)
            xw = c.vec(n); want = plan.solve(xw, b, 80, 1e-10, 0)          # warm-up, and the counts of the two extremes of `ahead`
            it = want[1]
            assert want[0] == 0 and plan.info()[4] >= it
            x = c.vec(n); got = plan.solve(x, b, 80, 1e-10, 10000)
            assert got == want and plan.info()[4] <= 2
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
    """5. neumann3d(16) plus eps·(S − Sᵀ), S the cyclic shift: nonsymmetric, every row and column still sums to zero; declared constant"""
    import scipy.sparse as sp
    from multigridsolver_amd.synthetic import neumann3d
    N = 16; n = N ** 3
    rp, ci, v = neumann3d(N)
    L = sp.csr_matrix((v, ci, rp), shape=(n, n))
    i = np.arange(n)
    S = sp.csr_matrix((np.ones(n), (i, (i + 1) % n)), shape=(n, n))
    M = (L + 0.25 * (S - S.T)).tocsr()
    M.sum_duplicates(); M.sort_indices()
    assert abs(M @ np.ones(n)).max() == 0.0 and abs(M.T @ np.ones(n)).max() == 0.0 and abs(M - M.T).max() > 0
    A = ctx.csr(n, n, M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data).set_nullspace("constant")
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(coarse_rows=60).finalize()
    b = ctx.vec(np.random.default_rng(12).standard_normal(n))
    x = ctx.vec(n); want = mg.bicgstab(A, x, b, h, 200, 1e-10); xw = x.numpy()
    print(f"null space: mgs_bicgstab {want}")
    assert want[0] == 0
    plan = mg.BicgstabPlan(A, h)
    for ahead in (0, 1, 4):
        y = ctx.vec(n); got = plan.solve(y, b, 200, 1e-10, ahead)
        same(got, y.numpy(), want, xw, f"null space, ahead {ahead}")
        assert abs(y.numpy().mean()) <= 1e-12 * abs(y.numpy()).max()
    y = ctx.vec(n)
    st, done, res, rec = plan.enqueue(y, b, want[1] + 2, 1e-10).result(recursive=True)
    assert done == want[1] and rec == want[2] and plan.info()[3] == 2
    assert np.array_equal(y.numpy(), xw)
    assert abs(y.numpy().mean()) <= 1e-12 * abs(y.numpy()).max()
    # a random x0 carries a mean: it is projected out
    x0 = np.random.default_rng(3).standard_normal(n) + 5.0
    x = ctx.vec(x0); want = mg.bicgstab(A, x, b, h, 200, 1e-10)
    y = ctx.vec(x0); got = plan.solve(y, b, 200, 1e-10)
    same(got, y.numpy(), want, x.numpy(), "null space, x0 with a mean")
    assert abs(y.numpy().mean()) <= 1e-12 * abs(y.numpy()).max()


def refused(mg, code, word, fn):
    with pytest.raises(mg.MgsError) as e:
        fn()
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_refusals(ctx, mg, c31):
    """6. each with a message"""
    shard = ctx.poisson3d(16, 4, 8, local_cols=True)
    refused(mg, INVALID, "row shard", lambda: mg.BicgstabPlan(shard))
    n = c31.n
    plan = mg.BicgstabPlan(c31.A)
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
    refused(mg, INVALID, "null-space", lambda: mg.BicgstabPlan(declared, h))
    from multigridsolver_amd.synthetic import neumann3d
    m = 8 ** 3
    neu = ctx.csr(m, m, *neumann3d(8)).set_nullspace("constant")
    hn = mg.Hierarchy(neu, 0.6, 1, 1).coarsen(coarse_rows=60).finalize()
    refused(mg, INVALID, "null-space", lambda: mg.BicgstabPlan(ctx.csr(m, m, *neumann3d(8)), hn))
    # a hierarchy with an exchange callback
    hc = mg.Hierarchy(twin, 0.6, 1, 1).coarsen(coarse_rows=60).finalize()
    hc.set_halo_exchange(lambda level, ptr: None)
    refused(mg, INVALID, "callbacks", lambda: mg.BicgstabPlan(twin, hc))
    # a hierarchy of another size; an unfinalized hierarchy (MGS_ERR_STATE)
    refused(mg, INVALID, "rows", lambda: mg.BicgstabPlan(c31.A, h))
    refused(mg, STATE, "finalize", lambda: mg.BicgstabPlan(twin, mg.Hierarchy(twin, 0.6, 1, 1)))
    # NULL arguments
    L = mg.lib()
    assert L.mgs_bicgstab_plan_create(None, None, None) == INVALID
    assert L.mgs_bicgstab_plan_solve(None, x.h, b.h, 0, None, None, None) == INVALID
    assert L.mgs_bicgstab_plan_solve(plan.h, x.h, b.h, 0, None, None, None) == INVALID
    assert L.mgs_bicgstab_plan_enqueue(plan.h, None, b.h, 1, 1e-6) == INVALID
    assert L.mgs_bicgstab_plan_result(None, None, None, None, None) == INVALID
    assert L.mgs_bicgstab_plan_info(plan.h, None) == INVALID
    assert L.mgs_bicgstab_plan_destroy(None) == 0
    # a matrix without rows (where the upload accepts one)
    try:
        empty = ctx.csr(0, 0, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    except mg.MgsError:
        empty = None
    if empty is not None:
        refused(mg, INVALID, "no rows", lambda: mg.BicgstabPlan(empty))
    # result before anything was solved or enqueued
    refused(mg, STATE, "nothing", lambda: plan.result())
    # a context that sums over ranks
    c2 = mg.Context(0)
    try:
        c2.set_allreduce(lambda a: None)
        A2c = c2.poisson3d(8)
        refused(mg, INVALID, "sums over ranks", lambda: mg.BicgstabPlan(A2c))
        del A2c
    finally:
        c2.close()


def test_refused_while_the_stream_is_captured(mg):
    """6. MGS_ERR_STATE from solve and enqueue while the context's stream is being captured; nothing is launched, and the plan serves afterwards"""
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
            plan = mg.BicgstabPlan(A)
            want = plan.solve(x, b, 80, 1e-10)
            xw = x.numpy()
            t = torch.zeros(64, device="cuda")
            stream.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
                t.add_(1.0)
                refused(mg, STATE, "captured", lambda: plan.solve(x, b, 80, 1e-10))
                refused(mg, STATE, "captured", lambda: plan.enqueue(x, b, 3, 1e-10))
            stream.synchronize()
            y = c.vec(n)
            assert plan.solve(y, b, 80, 1e-10) == want and np.array_equal(y.numpy(), xw)
        finally:
            stream.synchronize()
            if plan is not None:
                plan.close()
            del plan
            c.close()


def test_determinism(ctx, mg, c31):
    """6. two identical solves and two identical enqueues: identical bits and identical info()[2:4]"""
    n = c31.n
    h = push_all(mg, ctx, c31.A, c31.Ps, 0.6)
    plan = mg.BicgstabPlan(c31.A, h)
    runs = []
    for _ in range(2):
        x = ctx.vec(n); r = plan.solve(x, c31.b, 80, 1e-10, 2)
        runs.append((r, x.numpy(), plan.info()[2:4]))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    runs = []
    for _ in range(2):
        x = ctx.vec(n); r = plan.enqueue(x, c31.b, 30, 1e-10).result(recursive=True)
        runs.append((r, x.numpy(), plan.info()[2:4]))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
