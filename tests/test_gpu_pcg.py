"""mgs_pcg on the device against its numpy restatement (tests/pcg_ref.py) with the CPU oracle's cycle as preconditioner.
Bars: status equal; iterations within max(2, it/6) of the restatement and, at tol 1e-10, x within 1e-8 relative — what the
project already asks of BiCGSTAB against the reference's own run; the true residual recomputed by the oracle below 1.5·tol."""
import numpy as np
import pytest

from pcg_ref import pcg_ref

pytestmark = pytest.mark.gpu


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


def true_resid(Ao, x, b):
    return np.linalg.norm(Ao.residual(x, b)) / np.linalg.norm(b)


def explicit_levels(Ao, nlev):
    """the reference aggregation ("10 2 8") + Galerkin product per level on the CPU oracle: nlev − 1 prolongations"""
    Ps, A = [], Ao
    for _ in range(nlev - 1):
        P = A.agmg(10.0, 2, 8.0, strict=False)
        Ps.append(P)
        A = A.galerkin(P)
    return Ps


def diffusion3d_jumps(orc, N=32, block=8, seed=7):
    """7-point diffusion operator on N³ nodes, Dirichlet boundary, coefficient 1 or 10³ per block³ of nodes (seeded), face
    coefficients by harmonic mean: symmetric positive definite M-matrix"""
    import scipy.sparse as sps
    rng = np.random.default_rng(seed)
    nb = N // block
    kb = 10.0 ** (3 * rng.integers(0, 2, size=(nb, nb, nb)))
    k = np.kron(kb, np.ones((block, block, block)))
    idx = np.arange(N ** 3).reshape(N, N, N)
    diag = np.zeros((N, N, N))
    rows, cols, vals = [], [], []
    for ax in range(3):
        lo = [slice(None)] * 3; hi = [slice(None)] * 3
        lo[ax] = slice(0, N - 1); hi[ax] = slice(1, N)
        lo, hi = tuple(lo), tuple(hi)
        w = 2.0 * k[lo] * k[hi] / (k[lo] + k[hi])
        diag[lo] += w; diag[hi] += w
        rows += [idx[lo].ravel(), idx[hi].ravel()]; cols += [idx[hi].ravel(), idx[lo].ravel()]; vals += [-w.ravel(), -w.ravel()]
        first = [slice(None)] * 3; last = [slice(None)] * 3
        first[ax] = 0; last[ax] = N - 1
        diag[tuple(first)] += k[tuple(first)]; diag[tuple(last)] += k[tuple(last)]
    rows.append(idx.ravel()); cols.append(idx.ravel()); vals.append(diag.ravel())
    A = sps.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N ** 3, N ** 3))
    A.sort_indices()
    return orc.Csr.from_scipy(A)


def push_all(mg, ctx, A, Ps, omega, nu1=1, nu2=1):
    h = mg.Hierarchy(A, omega, nu1, nu2)
    for P in Ps:
        h.push_P(dev(ctx, P))
    return h.finalize()


def check_parity(mg, ctx, orc, Ao, A, h, ho, b_np, tol, flexible=False, x0=None, label=""):
    """device solve against the restatement: the bars of the module docstring; returns the device's count"""
    st_r, it_r, res_r, x_r = pcg_ref(Ao, b_np, ho.vcycle, tol=tol, max_iter=500, flexible=flexible, x0=x0)
    x = ctx.vec(Ao.shape[0] if x0 is None else x0)
    st, it, res = mg.pcg(A, x, ctx.vec(b_np), h, 500, tol, flexible)
    xd = x.numpy()
    tr = true_resid(Ao, xd, b_np)
    print(f"{label} tol {tol:g} flexible {int(flexible)}: device status {st}, {it} iterations, reported {res:.4e}, true {tr:.4e}; "
          f"restatement status {st_r}, {it_r} iterations, {res_r:.4e}; x rel diff {rel(xd, x_r):.3e}")
    assert st == 0 and st_r == 0
    assert abs(it - it_r) <= max(2, it_r // 6), (it, it_r)
    assert tr < 1.5 * tol
    if tol <= 1e-10:
        assert rel(xd, x_r) <= 1e-8
    return it


@pytest.mark.parametrize("tol", [1e-6, 1e-10])
def test_parity_pinned_input(ctx, mg, orc, inputs, tol):
    """poisson2d(100) + the reference's P (poisson10000promatrix.mtx), ω = 0.5, V(1,1): the input tests/test_pcg_restatement_cpu.py pins"""
    Ao = orc.poisson2d(100); Po = orc.Csr.read(inputs["poisson10000promatrix"])
    A = dev(ctx, Ao)
    h = push_all(mg, ctx, A, [Po], 0.5)
    ho = orc.Hier(Ao, [Po], omega=0.5, nu1=1, nu2=1)
    check_parity(mg, ctx, orc, Ao, A, h, ho, orc.rand_rhs(Ao.shape[0]), tol, label="poisson2d(100)+refP")


def _operator(orc, kind):
    return orc.poisson3d(48) if kind == "poisson3d_48" else diffusion3d_jumps(orc)


@pytest.mark.parametrize("kind", ["poisson3d_48", "diffusion3d_32_jumps"])
def test_multilevel_explicit_and_device_hierarchy(ctx, mg, orc, kind):
    """five levels, the same explicit P's on both sides; then the device-built hierarchy on the same operator, its count held to the
    margin test_device_agmg_hierarchy grants a device-built hierarchy against explicit P's"""
    Ao = _operator(orc, kind); n = Ao.shape[0]
    Ps = explicit_levels(Ao, 5)
    A = dev(ctx, Ao)
    h = push_all(mg, ctx, A, Ps, 0.6)
    assert h.nlev == 5
    ho = orc.Hier(Ao, Ps, omega=0.6, nu1=1, nu2=1)
    b_np = orc.rand_rhs(n)
    for tol in (1e-6, 1e-10):
        it_ref = check_parity(mg, ctx, orc, Ao, A, h, ho, b_np, tol, label=kind)
        hd = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0).finalize()
        x = ctx.vec(n); st, it_dev, res = mg.pcg(A, x, ctx.vec(b_np), hd, 500, tol)
        tr = true_resid(Ao, x.numpy(), b_np)
        print(f"{kind} tol {tol:g}: device-built hierarchy ({hd.nlev} levels) {it_dev} iterations, true residual {tr:.4e}; explicit P's {it_ref}")
        assert st == 0 and tr < 1.5 * tol
        assert it_dev <= it_ref + max(4, it_ref // 4), (it_dev, it_ref)


@pytest.mark.parametrize("kind,nlev", [("poisson2d_100", 4), ("poisson3d_32", 4), ("poisson3d_48", 5)])
def test_flexible_form(ctx, mg, orc, kind, nlev):
    """V(2,1) and the K-cycle are not fixed symmetric operators: flexible=False is refused with MGS_ERR_INVALID, flexible=True
    converges; for V(2,1) the count follows the flexible restatement with the same P's"""
    Ao = {"poisson2d_100": lambda: orc.poisson2d(100), "poisson3d_32": lambda: orc.poisson3d(32), "poisson3d_48": lambda: orc.poisson3d(48)}[kind]()
    n = Ao.shape[0]
    Ps = explicit_levels(Ao, nlev)
    A = dev(ctx, Ao)
    b_np = orc.rand_rhs(n); b = ctx.vec(b_np)
    tol = 1e-10
    h = push_all(mg, ctx, A, Ps, 0.6, 2, 1)
    ho = orc.Hier(Ao, Ps, omega=0.6, nu1=2, nu2=1)
    with pytest.raises(mg.MgsError) as e:
        mg.pcg(A, ctx.vec(n), b, h, 500, tol, False)
    assert e.value.code == -1 and "flexible" in str(e.value)
    check_parity(mg, ctx, orc, Ao, A, h, ho, b_np, tol, flexible=True, label=kind + " V(2,1)")
    # K-cycle on levels 1..2 with energy coefficients
    hk = push_all(mg, ctx, A, Ps, 0.6, 1, 1).set_kcycle(2)
    ctx.set_option("kcycle_energy", 1)
    try:
        with pytest.raises(mg.MgsError) as e:
            mg.pcg(A, ctx.vec(n), b, hk, 500, tol, False)
        assert e.value.code == -1 and "flexible" in str(e.value)
        x = ctx.vec(n); st, it, res = mg.pcg(A, x, b, hk, 500, tol, True)
        tr = true_resid(Ao, x.numpy(), b_np)
        print(f"{kind} K-cycle(2, energy) flexible: status {st}, {it} iterations, true residual {tr:.4e}")
        assert st == 0 and tr < 1.5 * tol
    finally:
        ctx.set_option("kcycle_energy", 0)


def test_contract_cases(ctx, mg, orc):
    # A negative definite, no preconditioner: r·r > 0, p·A·p < 0 in the first iteration
    Po = orc.poisson2d(30); n = Po.shape[0]
    No = orc.Csr.from_scipy(-Po.to_scipy())
    Nd = dev(ctx, No)
    b_np = orc.rand_rhs(n); b = ctx.vec(b_np)
    st_r, it_r, _, _ = pcg_ref(No, b_np, None, tol=1e-8, max_iter=50)
    x = ctx.vec(n); st, it, res = mg.pcg(Nd, x, b, None, 50, 1e-8)
    assert (st, it) == (3, 1) == (st_r, it_r)
    assert np.array_equal(x.numpy(), np.zeros(n))          # no completed update
    # ... with a two-level hierarchy (aggregation of +A, pushed: the device setup never sees the sign) ωD⁻¹ and the coarse
    # inverse are negative definite: r·z < 0 in the first iteration
    Pagg = Po.agmg(10.0, 2, 8.0)
    h = push_all(mg, ctx, Nd, [Pagg], 0.6)
    ho = orc.Hier(No, [Pagg], omega=0.6, nu1=1, nu2=1)
    st_r, it_r, _, _ = pcg_ref(No, b_np, ho.vcycle, tol=1e-8, max_iter=50)
    x = ctx.vec(n); st, it, res = mg.pcg(Nd, x, b, h, 50, 1e-8)
    assert (st, it) == (2, 1) == (st_r, it_r)

    # max_iter = 3, n = 29 791 odd: the lagged x update is flushed before the return, the tail element is updated
    Ao = orc.poisson3d(31); n = Ao.shape[0]
    assert n % 2 == 1
    Ps = explicit_levels(Ao, 3)
    A = dev(ctx, Ao)
    h = push_all(mg, ctx, A, Ps, 0.6)
    ho = orc.Hier(Ao, Ps, omega=0.6, nu1=1, nu2=1)
    b_np = orc.rand_rhs(n); b = ctx.vec(b_np)
    st_r, it_r, res_r, x_r = pcg_ref(Ao, b_np, ho.vcycle, tol=1e-12, max_iter=3)
    x = ctx.vec(n); st, it, res = mg.pcg(A, x, b, h, 3, 1e-12)
    print(f"max_iter 3: device ({st}, {it}, {res:.6e}), restatement ({st_r}, {it_r}, {res_r:.6e}), x rel diff {rel(x.numpy(), x_r):.3e}")
    assert (st, it) == (1, 3) == (st_r, it_r)
    assert rel(x.numpy(), x_r) <= 1e-10 and abs(res - res_r) <= 1e-8 * res_r
    assert abs(true_resid(Ao, x.numpy(), b_np) - res) <= 1e-8 * res      # x really holds all three updates
    for flexible in (False, True):                                        # the flexible form's lagged update as well
        st_r, it_r, res_r, x_r = pcg_ref(Ao, b_np, ho.vcycle, tol=1e-12, max_iter=4, flexible=flexible)
        x = ctx.vec(n); st, it, res = mg.pcg(A, x, b, h, 4, 1e-12, flexible)
        assert (st, it) == (1, 4) == (st_r, it_r) and rel(x.numpy(), x_r) <= 1e-10

    # a random initial guess: the restatement's result from the same x0
    x0 = orc.rand_rhs(n, seed=3)
    check_parity(mg, ctx, orc, Ao, A, h, ho, b_np, 1e-10, x0=x0, label="poisson3d(31) random x0")
    # x0 = a converged solution: nothing to do
    x = ctx.vec(n); st, it, res = mg.pcg(A, x, b, h, 500, 1e-10)
    assert st == 0 and it > 0
    xs = x.numpy()
    st, it, res2 = mg.pcg(A, x, b, h, 500, 1e-10)
    assert (st, it) == (0, 0) and res2 < 1e-10 and np.array_equal(x.numpy(), xs)
    # b = 0, x0 = 0
    x = ctx.vec(n); st, it, res = mg.pcg(A, x, ctx.vec(n), h, 500, 1e-10)
    assert (st, it, res) == (0, 0, 0.0) and np.array_equal(x.numpy(), np.zeros(n))


def test_determinism_scalar_forms_and_graph_reuse(ctx, mg, orc):
    Ao = orc.poisson3d(31); n = Ao.shape[0]
    Ps = explicit_levels(Ao, 3)
    A = dev(ctx, Ao)
    h = push_all(mg, ctx, A, Ps, 0.6)
    b = ctx.vec(orc.rand_rhs(n))
    ctx.trim()
    runs = []
    for flexible in (False, True):
        x1 = ctx.vec(n); r1 = mg.pcg(A, x1, b, h, 500, 1e-10, flexible)
        g1 = h.graph_info()["captured_cycles"]
        x2 = ctx.vec(n); r2 = mg.pcg(A, x2, b, h, 500, 1e-10, flexible)
        g2 = h.graph_info()["captured_cycles"]
        assert r1[0] == 0 and r1 == r2 and np.array_equal(x1.numpy(), x2.numpy())
        # r and z keep their addresses within a solve and across solves: the cycle replays from the slot the first solve captured
        assert g2 == g1, (g1, g2)
        runs.append((r1, x1.numpy(), g1))
    assert runs[0][2] == runs[1][2] == 1, [r[2] for r in runs]
    # the 8-byte forms of the two passes (option blas1_vec = 0)
    ctx.set_option("blas1_vec", 0)
    try:
        for flexible, (r1, x1, _) in zip((False, True), runs):
            x = ctx.vec(n); r = mg.pcg(A, x, b, h, 500, 1e-10, flexible)
            assert r[0] == 0 and rel(x.numpy(), x1) <= 1e-10
    finally:
        ctx.set_option("blas1_vec", 1)


def test_full_size_512(ctx, mg):
    """mgs_pcg + V(1,1) on the device-built 512³ hierarchy to 1e-10; the count is recorded, not asserted"""
    N = 512; n = N ** 3
    A = ctx.poisson3d(N)
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 1024, 32).finalize()
    b = ctx.vec(n).rand(seed=11)
    x = ctx.vec(n)
    st, it, res = mg.pcg(A, x, b, h, 1000, 1e-10)
    true = A.residual(x, b).nrm2() / b.nrm2()
    print(f"512^3: PCG + V(1,1) status {st}, {it} iterations, reported {res:.4e}, true residual {true:.4e}")
    assert st == 0
    assert true <= 1e-10
