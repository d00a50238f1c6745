"""Matrices declared MGS_NULLSPACE_CONSTANT on the device (include/mgs.h: mgs_csr_set_nullspace): the regularised coarsest solve, the
projection kernels and the projected Krylov solvers against tests/nullspace_ref.py run on the device's OWN hierarchy (level operators
and aggregates downloaded).  Operators: neumann3d(12) (1728 rows: full and ragged row blocks of 256), neumann3d(9) (729 rows, odd:
aggregates of one and three rows at the faces), a 20×20 grid graph Laplacian with random weights in [0.5, 2] (non-constant
coefficients) and a 50-row weighted Laplacian solved by a one-level hierarchy.  Hierarchies use coarse_rows = 60.

Bars (tol = 1e-10, max_iter = 200 as a cap that catches stagnation):
  * the relative residual recomputed in numpy against Πb is at most tol·(1 + 1e-3);
  * |mean(x)| <= n·ε·max|x_i|, the worst case of any summation order;
  * x and x_ref both have zero mean and residuals of at most tol·‖Πb‖, so ‖x − x_ref‖ <= 2·tol·‖Πb‖/λ_min⁺ (λ_min⁺: np.linalg.eigvalsh);
  * iteration counts: tests/test_gpu_pcg.py's, |it − it_ref| <= max(2, it_ref // 6) for PCG against the restatement on the same
    hierarchy, it <= it_ref + max(4, it_ref // 4) for BiCGSTAB and FGCR."""
import ctypes as C

import numpy as np
import pytest

import agmg_ref
import nullspace_ref as ns

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TOL = 1e-10
INVALID, NUMERIC = -1, -5


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


def grid_laplacian(nx, ny, seed):
    """weighted graph Laplacian of the nx × ny grid graph, weights uniform in [0.5, 2] from a fixed seed → scipy CSR, sorted columns"""
    import scipy.sparse as sps
    rng = np.random.default_rng(seed)
    idx = np.arange(nx * ny).reshape(nx, ny)
    e = np.r_[np.c_[idx[:-1].ravel(), idx[1:].ravel()], np.c_[idx[:, :-1].ravel(), idx[:, 1:].ravel()]]
    w = rng.uniform(0.5, 2.0, len(e))
    W = sps.coo_matrix((np.r_[w, w], (np.r_[e[:, 0], e[:, 1]], np.r_[e[:, 1], e[:, 0]])), shape=(nx * ny, nx * ny)).tocsr()
    A = (sps.diags(np.asarray(W.sum(axis=1)).ravel()) - W).tocsr()
    A.sort_indices()
    return A


def host_operator(name):
    from multigridsolver_amd.synthetic import neumann3d
    if name.startswith("neumann3d_"):
        N = int(name.split("_")[1])
        return agmg_ref.csr(N ** 3, N ** 3, *neumann3d(N))
    return {"grid20": lambda: grid_laplacian(20, 20, 5), "onelevel50": lambda: grid_laplacian(5, 10, 9)}[name]()


def upload(mg, ctx, S):
    return mg.Csr.upload(ctx, S.shape[0], S.shape[1], S.indptr, S.indices, S.data)


def device_cycle(h, omega=0.6):
    """nullspace_ref.Cycle over the device's own hierarchy"""
    As, aggs = [], []
    for l in range(h.nlev):
        rows = h.level_shape(l)[0]
        As.append(agmg_ref.csr(rows, rows, *h.level_A(l).download()))
        if l + 1 < h.nlev:
            aggs.append(h.level_P(l).agg().astype(np.int64))
    return ns.Cycle(As, aggs, omega)


_lam = {}      # λ_min⁺ per operator, computed once


class Problem:
    def __init__(self, mg, ctx, name):
        self.name = name
        self.S = host_operator(name); self.n = self.S.shape[0]
        self.A = upload(mg, ctx, self.S).set_nullspace("constant")
        self.h = mg.Hierarchy(self.A, 0.6, 1, 1)
        if name != "onelevel50":
            self.h.coarsen(coarse_rows=60)
        self.h.finalize()
        self.cycle = device_cycle(self.h)
        if name not in _lam:
            lam = np.linalg.eigvalsh(self.S.toarray())
            assert abs(lam[0]) <= self.n * EPS * lam[-1]
            _lam[name] = lam[1]
        self.lam = _lam[name]
        self.b = ns.project(np.random.default_rng(len(name)).standard_normal(self.n))      # consistent to rounding
        self.ref = {}

    def reference(self, solver):
        if solver not in self.ref:
            run = {"pcg": lambda: ns.pcg(self.S, self.b, self.cycle.vcycle, tol=TOL, max_iter=200),
                   "pcg_flexible": lambda: ns.pcg(self.S, self.b, self.cycle.vcycle, tol=TOL, max_iter=200, flexible=True),
                   "bicgstab": lambda: ns.bicgstab(self.S, self.b, self.cycle.vcycle, tol=TOL, max_iter=200),
                   "fgcr": lambda: ns.fgcr(self.S, self.b, self.cycle.vcycle, restart=10, tol=TOL, max_iter=200)}[solver]
            self.ref[solver] = run()
            assert self.ref[solver][0] == 0
        return self.ref[solver]


_problems = {}


@pytest.fixture
def problem(mg, ctx):
    def get(name):
        if name not in _problems:
            _problems[name] = Problem(mg, ctx, name)
        return _problems[name]
    yield get


@pytest.fixture(scope="module", autouse=True)
def _release_problems(ctx):
    yield
    _problems.clear()      # before the context closes


def check_solution(p, x, b_given, label, x_ref, scale=1.0):
    """the bars of the module docstring for a device solution x of A·x = Π·b_given; x_ref: the solution it is held against"""
    pb = ns.project(b_given)
    true = np.linalg.norm(ns.project(b_given - scale * (p.S @ x))) / np.linalg.norm(pb)
    mean, dist = abs(x.mean()), np.linalg.norm(x - x_ref)
    bound = 2 * TOL * np.linalg.norm(pb) / (scale * p.lam)
    print(f"{label}: true residual {true:.4e}, |mean(x)| {mean:.3e} (bar {p.n * EPS * np.abs(x).max():.3e}), ‖x − x_ref‖ {dist:.3e} (bar {bound:.3e})")
    assert true <= TOL * (1 + 1e-3)
    assert mean <= p.n * EPS * np.abs(x).max()
    assert dist <= bound


# ---------------------------------------------------------------------------------------------------------------- (1) refusal kept
def test_refusal_kept_without_the_declaration(mg, ctx):
    S = host_operator("neumann3d_12")
    A = upload(mg, ctx, S)
    assert A.nullspace() is None
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(coarse_rows=60)
    assert h.nlev >= 3
    with pytest.raises(mg.MgsError) as e:
        h.finalize()
    assert e.value.code == NUMERIC and "singular" in str(e.value)
    A.set_nullspace("constant")
    assert A.nullspace() == "constant"
    h.finalize()
    d = A.nullspace_defect()
    print(f"neumann3d(12): {h.nlev} levels, defects {d}")
    assert d == (0.0, 0.0)                      # integer entries: A·1 is exact
    # the net catches a matrix that does not carry the null space: the Dirichlet operator's corner rows sum to 3, its interior rows to 12 in modulus
    assert ctx.poisson3d(12).nullspace_defect() == (0.25, 0.25)
    # what mgs_csr_set_nullspace refuses
    with pytest.raises(mg.MgsError) as e:
        ctx.poisson3d(8, 2, 6, local_cols=True).set_nullspace("constant")        # a row shard: halo columns
    assert e.value.code == INVALID
    assert mg.lib().mgs_csr_set_nullspace(A.h, 2) == INVALID and A.nullspace() == "constant"


# ---------------------------------------------------------------------------------------------------------------- (2) PCG
@pytest.mark.parametrize("name", ["neumann3d_12", "neumann3d_9", "grid20", "onelevel50"])
def test_pcg(mg, ctx, problem, name):
    p = problem(name)
    assert p.h.nlev >= 3 or name == "onelevel50"
    st_r, it_r, res_r, x_r = p.reference("pcg")
    x = ctx.vec(p.n)
    st, it, res = mg.pcg(p.A, x, ctx.vec(p.b), p.h, 200, TOL)
    print(f"{name}: {p.h.nlev} levels, device status {st}, {it} iterations, reported {res:.4e}; restatement {it_r} iterations, {res_r:.4e}")
    assert st == 0 and res < TOL
    assert abs(it - it_r) <= max(2, it_r // 6), (it, it_r)
    check_solution(p, x.numpy(), p.b, name, x_r)
    # h = NULL: z = Πr
    if name == "onelevel50":
        st_n, it_n, _, x_n = ns.pcg(p.S, p.b, None, tol=TOL, max_iter=200)
        x = ctx.vec(p.n); st, it, res = mg.pcg(p.A, x, ctx.vec(p.b), None, 200, TOL)
        assert st == 0 == st_n and abs(it - it_n) <= max(2, it_n // 6), (it, it_n)
        check_solution(p, x.numpy(), p.b, name + " unpreconditioned", x_n)


# ---------------------------------------------------------------------------------------------------------------- (3) inconsistent b
def test_inconsistent_rhs(mg, ctx, problem):
    p = problem("neumann3d_12")
    _, it_r, _, x_r = p.reference("pcg")
    b3 = p.b + 3.0
    bd = ctx.vec(b3)
    x = ctx.vec(p.n)
    st, it, res = mg.pcg(p.A, x, bd, p.h, 200, TOL)
    assert st == 0 and abs(it - it_r) <= max(2, it_r // 6)
    assert np.array_equal(bd.numpy(), b3)                      # the caller's b is only read
    xd = x.numpy()
    check_solution(p, xd, b3, "b + 3·1", x_r)
    # *tol is relative to ‖Πb‖, not to ‖b‖ (three times larger here)
    rel_pb = np.linalg.norm(ns.project(b3 - p.S @ xd)) / np.linalg.norm(ns.project(b3))
    assert abs(res - rel_pb) <= 1e-3 * rel_pb
    assert np.linalg.norm(b3) > 3 * np.linalg.norm(ns.project(b3))
    # b = c·1: Πb = 0, normb = 1, nothing to do
    x = ctx.vec(p.n); st, it, res = mg.pcg(p.A, x, ctx.vec(np.full(p.n, 2.0)), p.h, 200, TOL)
    assert (st, it) == (0, 0) and res <= p.n * EPS * 2.0 and np.array_equal(x.numpy(), np.zeros(p.n))


# ---------------------------------------------------------------------------------------------------------------- (4) initial guess
def test_initial_guess_with_a_mean(mg, ctx, problem):
    p = problem("neumann3d_9")
    _, _, _, x_r = p.reference("pcg")
    x0 = np.random.default_rng(4).standard_normal(p.n); x0 += 5.0 - x0.mean()
    x = ctx.vec(x0)
    st, it, res = mg.pcg(p.A, x, ctx.vec(p.b), p.h, 200, TOL)
    assert st == 0
    check_solution(p, x.numpy(), p.b, "guess with mean 5", x_r)
    # a converged, zero-mean guess: nothing to do
    st, it, res = mg.pcg(p.A, x, ctx.vec(p.b), p.h, 200, TOL)
    assert (st, it) == (0, 0)
    check_solution(p, x.numpy(), p.b, "converged guess", x_r)


# ---------------------------------------------------------------------------------------------------------------- (5) BiCGSTAB, FGCR
@pytest.mark.parametrize("solver", ["bicgstab", "fgcr"])
def test_bicgstab_and_fgcr(mg, ctx, problem, solver):
    p = problem("neumann3d_12")
    st_r, it_r, res_r, x_r = p.reference(solver)
    x = ctx.vec(np.full(p.n, 5.0)) if solver == "fgcr" else ctx.vec(p.n)      # FGCR from a guess with a constant component
    b = ctx.vec(p.b)
    if solver == "bicgstab":
        st, it, res = mg.bicgstab(p.A, x, b, p.h, 200, TOL)
    else:
        st, it, res = mg.fgcr(p.A, x, b, p.h, 10, 200, TOL)
    print(f"{solver}: device status {st}, {it} iterations, reported {res:.4e}; restatement {it_r} iterations, {res_r:.4e}")
    assert st == 0 and res < TOL
    assert it <= it_r + max(4, it_r // 4), (it, it_r)
    check_solution(p, x.numpy(), p.b, solver, x_r)


# ---------------------------------------------------------------------------------------------------------------- (6) K-cycle
def test_kcycle_flexible_pcg(mg, ctx, problem):
    p = problem("neumann3d_12")
    _, _, _, x_r = p.reference("pcg")
    hk = mg.Hierarchy(p.A, 0.6, 1, 1).coarsen(coarse_rows=60).finalize().set_kcycle(2)
    with pytest.raises(mg.MgsError) as e:
        mg.pcg(p.A, ctx.vec(p.n), ctx.vec(p.b), hk, 200, TOL, False)
    assert e.value.code == INVALID and "flexible" in str(e.value)          # the acceptance rule of flexible = 0 is unchanged
    x = ctx.vec(p.n)
    st, it, res = mg.pcg(p.A, x, ctx.vec(p.b), hk, 200, TOL, True)
    print(f"K-cycle(2) + flexible PCG: status {st}, {it} iterations, reported {res:.4e}")
    assert st == 0
    check_solution(p, x.numpy(), p.b, "K-cycle(2)", x_r)


# ---------------------------------------------------------------------------------------------------------------- (7) coarsest solve alone
def test_coarsest_solve_alone(mg, ctx, problem):
    p = problem("onelevel50")
    assert p.h.nlev == 1
    M = ns.regularised(p.S)
    cond = np.linalg.cond(M)
    b = ns.project(np.random.default_rng(2).standard_normal(p.n))
    x = p.h.vcycle(ctx.vec(b)).numpy()
    xs = np.linalg.solve(M, b)
    err = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    print(f"one level, {p.n} rows: cond {cond:.1f}, rel diff to np.linalg.solve {err:.3e} (bar {8 * p.n * EPS * cond:.3e})")
    assert err <= 8 * p.n * EPS * cond
    # mgs_vcycle is not projected: on 1 the regularised inverse answers 1/s
    s = np.abs(p.S.data).max()
    x1 = p.h.vcycle(ctx.vec(np.ones(p.n))).numpy()
    assert np.linalg.norm(x1 - 1.0 / s) <= 8 * p.n * EPS * cond * np.linalg.norm(x1)


# ---------------------------------------------------------------------------------------------------------------- (8) refresh
def test_refresh_with_doubled_values(mg, ctx):
    p = Problem(mg, ctx, "neumann3d_12")          # its own copy: the values change
    x = ctx.vec(p.n); b = ctx.vec(p.b)
    st, it, res = mg.pcg(p.A, x, b, p.h, 200, TOL)
    assert st == 0
    x1 = x.numpy()
    p.A.update_values(2.0 * p.S.data)
    p.h.refresh()
    assert p.h.refresh_info()["kept_graphs"] == 1
    x = ctx.vec(p.n)
    st2, it2, res2 = mg.pcg(p.A, x, b, p.h, 200, TOL)
    print(f"refresh with 2·A: {it} iterations before, {it2} after")
    assert st2 == 0 and abs(it2 - it) <= 1
    # x2 and x1/2 have zero mean and residuals of at most tol·‖Πb‖ for the operator 2·A, whose λ_min⁺ is twice A's
    check_solution(p, x.numpy(), p.b, "2·A", 0.5 * x1, scale=2.0)
    # taking the declaration back makes the next refresh refuse the singular coarsest operator again
    p.A.set_nullspace(None)
    with pytest.raises(mg.MgsError) as e:
        p.h.refresh()
    assert e.value.code == NUMERIC
    p.A.set_nullspace("constant")
    p.h.refresh()
    x = ctx.vec(p.n); st3, it3, _ = mg.pcg(p.A, x, b, p.h, 200, TOL)
    assert st3 == 0 and abs(it3 - it) <= 1


# ---------------------------------------------------------------------------------------------------------------- (9) flag off again
def test_flag_set_and_cleared_is_the_unflagged_path(mg, ctx):
    def solve(c, toggle):
        A = c.poisson3d(12)
        if toggle:
            A.set_nullspace("constant"); A.set_nullspace(None)
        assert A.nullspace() is None
        h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(coarse_rows=60).finalize()
        x = c.vec(12 ** 3)
        r = mg.pcg(A, x, c.vec(12 ** 3).rand(seed=3), h, 200, TOL)
        return r, x.numpy()
    r1, x1 = solve(ctx, True)
    c2 = mg.Context(0)
    try:
        r2, x2 = solve(c2, False)
    finally:
        c2.close()
    assert r1[0] == 0 and r1 == r2 and np.array_equal(x1, x2)


def test_kind_mismatch_between_matrix_and_hierarchy(mg, ctx, problem):
    p = problem("neumann3d_9")
    twin = upload(mg, ctx, p.S)                     # same values, no declaration
    for run in (lambda: mg.pcg(twin, ctx.vec(p.n), ctx.vec(p.b), p.h, 10, TOL),
                lambda: mg.bicgstab(twin, ctx.vec(p.n), ctx.vec(p.b), p.h, 10, TOL),
                lambda: mg.fgcr(twin, ctx.vec(p.n), ctx.vec(p.b), p.h, 10, 10, TOL)):
        with pytest.raises(mg.MgsError) as e:
            run()
        assert e.value.code == INVALID and "kind" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- (10) projection kernel
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, (1 << 16) + 3])
@pytest.mark.parametrize("offset", [0, 8])
def test_projection_kernel(mg, ctx, n, offset):
    """offset 8: a view that starts 8 bytes off 16-byte alignment (the scalar path); offset 0 takes the 16-byte path"""
    v = np.random.default_rng(n).standard_normal(n) + 3.0
    base = ctx.vec(n + 1)
    assert base.ptr % 16 == 0
    w = mg.Vec.wrap(ctx, base.ptr + offset, n)
    runs = []
    for _ in range(2):
        w.upload(v)
        m = w.project_const()
        runs.append((m, w.numpy()))
    (m, out), (m2, out2) = runs
    assert abs(m - v.mean()) <= n * EPS * np.abs(v).max()
    assert np.array_equal(out, v - m)                            # each entry is fl(v_i − m) for the device's own m
    assert m == m2 and np.array_equal(out, out2)                 # bit-reproducible
    # the variant that also returns ‖v − m‖ from the shift pass: same m, same entries; the sum of n squares carries at most n·ε relative
    w.upload(v)
    m3, nrm = w.project_const(nrm2=True)
    assert m3 == m and np.array_equal(w.numpy(), out)
    assert abs(nrm - np.linalg.norm(out)) <= n * EPS * np.linalg.norm(out)
    if offset:
        assert base.numpy()[0] == 0.0                            # the entry in front of the view is untouched
    else:
        assert base.numpy()[n] == 0.0                            # ... and the one behind it


def test_projection_kernel_large(mg, ctx):
    """n = 2²¹ + 5: 4097 one-shot workgroups, so the partials leave the context's own scratch (more than 2048), the fold takes its
    chunk stage (more than 4096), and the shift pass stores with the `nt` hint (option nt_store: 10⁶ rows on) — the branches every
    large solve takes.  Same checks as above, and the scalar form (option blas1_vec = 0) against the same bars."""
    n = (1 << 21) + 5
    v = np.random.default_rng(21).standard_normal(n) + 3.0
    w = ctx.vec(n)
    runs = []
    for _ in range(2):
        w.upload(v)
        m, nrm = w.project_const(nrm2=True)
        runs.append((m, nrm, w.numpy()))
    (m, nrm, out), (m2, nrm2, out2) = runs
    assert abs(m - v.mean()) <= n * EPS * np.abs(v).max()
    assert np.array_equal(out, v - m)
    assert m == m2 and nrm == nrm2 and np.array_equal(out, out2)
    assert abs(nrm - np.linalg.norm(out)) <= n * EPS * np.linalg.norm(out)
    w.upload(v)
    assert w.project_const() == m and np.array_equal(w.numpy(), out)          # without the norm: the same mean, the same entries
    ctx.set_option("blas1_vec", 0)
    try:
        w.upload(v)
        ms, nrms = w.project_const(nrm2=True)
        outs = w.numpy()
    finally:
        ctx.set_option("blas1_vec", 1)
    assert abs(ms - v.mean()) <= n * EPS * np.abs(v).max() and np.array_equal(outs, v - ms)
    assert abs(nrms - np.linalg.norm(outs)) <= n * EPS * np.linalg.norm(outs)


# ---------------------------------------------------------------------------------------------------------------- (11) structural refusals
def test_structural_refusals(mg, ctx):
    import scipy.sparse as sps
    lib = mg.lib()
    S = grid_laplacian(4, 6, 1); n = S.shape[0]
    # a general P: one entry of 0.5
    A = upload(mg, ctx, S).set_nullspace("constant")
    i = np.arange(n)
    P = sps.coo_matrix((np.r_[np.ones(n), 0.5], (np.r_[i, 0], np.r_[i // 2, 1])), shape=(n, n // 2)).tocsr()
    P.sort_indices()
    h = mg.Hierarchy(A, 0.6, 1, 1).push_P(upload(mg, ctx, P))
    assert not h.level_P(0).is_aggregation
    with pytest.raises(mg.MgsError) as e:
        h.finalize()
    assert e.value.code == INVALID and "level 0" in str(e.value) and "general P" in str(e.value)
    assert b"general P" in lib.mgs_last_error(ctx.h)
    # an aggregate array that leaves row 5 outside every aggregate
    A2 = upload(mg, ctx, S).set_nullspace("constant")
    agg = (i // 2).astype(np.int32); agg[5] = -1
    T = C.c_void_p()
    assert lib.mgs_xfer_from_agg(ctx.h, n, n // 2, agg.ctypes.data_as(C.POINTER(C.c_int)), C.byref(T)) == 0
    Ac = C.c_void_p()
    assert lib.mgs_csr_galerkin(A2.h, T, C.byref(Ac)) == 0
    h2 = mg.Hierarchy(A2, 0.6, 1, 1)
    assert lib.mgs_hier_push_level(h2.h, T, Ac) == 0             # the hierarchy owns both now
    with pytest.raises(mg.MgsError) as e:
        h2.finalize()
    assert e.value.code == INVALID and "level 0" in str(e.value) and "1 rows outside every aggregate" in str(e.value)
    assert b"outside every aggregate" in lib.mgs_last_error(ctx.h)
    # without the declaration the same hierarchy is what it always was (row 5 left out, the coarse operator is regular): accepted
    A2.set_nullspace(None)
    h2.finalize()
    ctx.sync()                                                   # nothing faulted: the refusals are argument checks made before any launch
