"""Properties of the restatement of mgs_guess (tests/guess_ref.py) that hold for the method itself, whatever the device does; the device is
then held to the restatement (tests/test_gpu_guess.py).  Operators: 3-D Poisson 8³ (energy and residual kind) and the reference's
nonsymmetric family csky3d(8) (residual kind); solutions of random right-hand sides from a sparse LU."""
import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spl

import guess_ref as G
from pcg_ref import pcg_ref

CAP = 8
U = 2.0 ** -53


def csky(N):
    from multigridsolver_amd.synthetic import csky3d
    rp, ci, v = csky3d(N)
    return sps.csr_matrix((v, ci, rp), shape=(N ** 3, N ** 3))


@pytest.fixture(scope="module")
def problems(orc):
    out = {}
    for name, A, kind in [("poisson8-energy", orc.poisson3d(8).to_scipy(), G.ENERGY), ("poisson8-residual", orc.poisson3d(8).to_scipy(), G.RESIDUAL),
                          ("csky8-residual", csky(8), G.RESIDUAL)]:
        A = A.tocsr()
        out[name] = (A, kind, spl.splu(A.tocsc()))
    return out


NAMES = ["poisson8-energy", "poisson8-residual", "csky8-residual"]


def filled(A, kind, lu, m, seed=1, dtype=np.float64):
    rng = np.random.default_rng(seed)
    g = G.GuessRef(A, kind, CAP, dtype=dtype)
    bs, xs = [], []
    for _ in range(m):
        b = rng.standard_normal(A.shape[0]); x = lu.solve(b)
        assert g.update(x)
        bs.append(b); xs.append(x)
    return g, bs, xs


def changed(A, kind):
    """same pattern, other values; the energy kind needs the result symmetric positive definite: D·A·D"""
    n = A.shape[0]
    if kind == G.ENERGY:
        D = sps.diags(1 + 0.05 * np.sin(np.arange(n)))
        return (D @ A @ D).tocsr()
    B = A.copy(); B.data = B.data * (1 + 0.05 * np.sin(np.arange(B.nnz)))
    return B


@pytest.mark.parametrize("name", NAMES)
def test_gram_is_the_identity_after_capacity_updates_and_after_a_rebase(problems, name):
    """Orthonormality defect max|G − I| in float64.  Measured on these three problems: 4.4e-16, 2.2e-16, 3.3e-16 after eight updates and
    2.2e-16, 2.2e-16, 4.4e-16 after the rebase (long double: 1.1e-19 … 2.2e-19).  Bar: 8 × the largest measured defect = 8 × 4.4e-16 =
    3.6e-15 — the margin 8 covers other seeds and BLAS summation orders; twice-applied Gram-Schmidt keeps the defect at a small multiple of
    u whatever the conditioning, so the bar does not grow with the problem."""
    A, kind, lu = problems[name]
    g, _, _ = filled(A, kind, lu, CAP)
    d = np.abs(g.gram() - np.eye(CAP)).max()
    g.rebase(changed(A, kind))
    assert g.size == CAP and g.refused == 0
    d2 = np.abs(g.gram() - np.eye(CAP)).max()
    A2 = changed(A, kind)
    for k in range(CAP):                                                       # every ỹ was recomputed with the new values
        assert np.linalg.norm(g.Y[k] - A2 @ g.X[k]) <= 64 * U * np.linalg.norm(g.Y[k]) * np.sqrt(CAP)
    gl, _, _ = filled(A, kind, lu, CAP, dtype=np.longdouble)
    dl = np.abs(gl.gram() - np.eye(CAP)).max()
    print(f"{name}: defect {d:.2e}, after rebase {d2:.2e}, long double {float(dl):.2e}")
    assert d <= 8 * 4.4e-16 and d2 <= 8 * 4.4e-16
    assert dl <= 8 * 4.4e-16 * 2.0 ** -11                                     # the same bar in units of the long double's rounding


@pytest.mark.parametrize("name", NAMES)
def test_projection_never_loses(problems, name):
    """residual kind: ‖b − A·x0‖ <= ‖b‖; energy kind: ‖x − x0‖_A <= ‖x‖_A — for an arbitrary b (x0 is the best approximation from the span in
    that norm, and 0 lies in the span); a rounding allowance of 1e-12 relative"""
    A, kind, lu = problems[name]
    g, _, _ = filled(A, kind, lu, 5)
    rng = np.random.default_rng(9)
    for _ in range(4):
        b = rng.standard_normal(A.shape[0])
        x0, alpha, rel = g.apply(b)
        if kind == G.RESIDUAL:
            assert np.linalg.norm(b - A @ x0) <= np.linalg.norm(b) * (1 + 1e-12)
            assert abs(rel - np.linalg.norm(b - A @ x0) / np.linalg.norm(b)) <= 1e-12
        else:
            x = lu.solve(b); e = x - x0
            assert e @ (A @ e) <= (x @ (A @ x)) * (1 + 1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_exact_recovery_in_the_span(problems, name):
    """b = Σ c_i·b_i of earlier right-hand sides: x0 solves the system to rounding.  Bar 1e-9 on ‖b − A·x0‖/‖b‖ (the bar of the device test)."""
    A, kind, lu = problems[name]
    g, bs, xs = filled(A, kind, lu, 6)
    c = np.random.default_rng(3).standard_normal(6)
    b = sum(ci * bi for ci, bi in zip(c, bs))
    x0, _, rel = g.apply(b)
    print(f"{name}: rel_resid {rel:.2e}")
    assert rel < 1e-9 and np.linalg.norm(b - A @ x0) / np.linalg.norm(b) < 1e-9


@pytest.mark.parametrize("name", NAMES)
def test_duplicate_candidate_is_refused(problems, name):
    A, kind, lu = problems[name]
    g, bs, xs = filled(A, kind, lu, 4)
    X = [v.copy() for v in g.X]
    assert not g.update(xs[2])
    assert not g.update(xs[0] - 2.0 * xs[3])
    assert g.size == 4 and g.refused == 2 and all(np.array_equal(a, b) for a, b in zip(X, g.X))
    assert g.last["nu2"] <= G.FLOOR2 * g.last["nu0"] or g.last["nu2"] < G.ETA2 * g.last["nu1"]
    if kind == G.ENERGY:                       # A not positive along x: refused whatever the basis holds
        h = G.GuessRef(-A, kind, CAP)
        assert not h.update(xs[0]) and h.last["nu0"] < 0 and h.refused == 1
    assert not G.GuessRef(A, kind, CAP).update(np.zeros(A.shape[0]))


@pytest.mark.parametrize("name", NAMES)
def test_restart_keeps_the_latest_solution(problems, name):
    A, kind, lu = problems[name]
    g, bs, xs = filled(A, kind, lu, CAP)
    rng = np.random.default_rng(11)
    b = rng.standard_normal(A.shape[0]); x = lu.solve(b)
    assert g.update(x)
    assert g.size == 1 and g.restarts == 1 and g.last["restart"] and g.last["K"] == 0
    x0, _, rel = g.apply(2.5 * b)                   # the span is the latest solution alone: its right-hand side is recovered, an older one is not
    assert rel < 1e-12 and np.linalg.norm(x0 - 2.5 * x) <= 1e-12 * np.linalg.norm(x)
    assert g.apply(bs[0])[2] > 0.5
    assert g.update(xs[0]) and g.size == 2


def test_constant_null_space(problems):
    """pure-Neumann operator: candidates are made zero-mean, so is every x0; the constant is refused with ν0² = 0 exactly"""
    from multigridsolver_amd.synthetic import neumann3d
    N = 6; n = N ** 3
    rp, ci, v = neumann3d(N)
    A = sps.csr_matrix((v, ci, rp), shape=(n, n))
    g = G.GuessRef(A, G.ENERGY, CAP, nullspace=True)
    assert not g.update(np.ones(n)) and g.last["nu0"] == 0.0
    rng = np.random.default_rng(2)
    for _ in range(3):
        assert g.update(rng.standard_normal(n) + 7.0)
    b = rng.standard_normal(n)
    x0 = g.apply(b - b.mean())[0]
    assert abs(x0.mean()) <= 8 * U * np.abs(x0).max()


def test_projected_guess_beats_the_previous_solution_on_the_probe_sequence(orc):
    """Poisson 12³, CG without preconditioner (tests/pcg_ref.py) to 1e-8, nine steps of guess_ref.probe_rhs, capacity 8.  Recorded counts:
    zero guess 43 43 43 43 43 43 44 44 44; previous solution 43 40 40 40 40 40 41 41 41 (steps 3..8: 243); projected 43 40 38 35 33 28 23 21 18
    (steps 3..8: 158)."""
    Ao = orc.poisson3d(12); As = Ao.to_scipy()
    rhs = [G.probe_rhs(12, s) for s in range(9)]

    def solve(b, x0):
        st, it, res, x = pcg_ref(Ao, b, None, tol=1e-8, max_iter=500, x0=x0)
        assert st == 0
        return it, x
    prev = G.run_sequence(solve, rhs, "previous")
    proj = G.run_sequence(solve, rhs, "projected", lambda: G.GuessRef(As, G.ENERGY, CAP))
    print("previous", prev, sum(prev[3:9]), "projected", proj, sum(proj[3:9]))
    assert sum(proj[3:9]) < sum(prev[3:9])
