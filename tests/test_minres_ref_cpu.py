"""CPU-only: the numpy restatement of mgs_minres (tests/minres_ref.py) against scipy.sparse.linalg.minres on three saddle-point systems,
its exits on hand-made 2×2 cases, the recalibration of its stopping rule, the per-entry update against a scalar loop, and the spectrum
of the banded indefinite operator the GPU tests run on.

Bar on x against scipy at equal iteration counts: 1e-13 relative.  Measured: 4.7e-16 … 5.6e-16 (printed by the test), so the bar is about
200 times that — room for another BLAS's summation order, while one wrong rotation moves x in its leading digits."""
import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

import krylov_ref as kr
from minres_ref import banded_sym, exact_block_precond, minres_ref, saddle, saddle_rhs, update_ref

X_BAR = 1e-13


@pytest.fixture(scope="module")
def systems():
    made = {}

    def get(N):
        if N not in made:
            sd = saddle(N)
            made[N] = (sd, exact_block_precond(sd), saddle_rhs(sd["n"] + sd["m"]))
        return made[N]
    return get


def scipy_minres(K, b, M, maxiter):
    """scipy's MINRES for exactly `maxiter` iterations: a tolerance it does not reach first"""
    rows = K.shape[0]
    Mop = spla.LinearOperator((rows, rows), matvec=M, dtype=np.float64)
    try:
        x, info = spla.minres(K, b, M=Mop, rtol=1e-300, maxiter=maxiter)
    except TypeError:                                   # older scipy spells the tolerance `tol`
        x, info = spla.minres(K, b, M=Mop, tol=1e-300, maxiter=maxiter)
    return x


@pytest.mark.parametrize("N", [6, 8, 12])
def test_restatement_against_scipy(systems, N):
    sd, M, b = systems(N)
    K = sd["K"]
    assert abs(K - K.T).max() == 0.0
    if N == 6:
        ev = np.linalg.eigvalsh(K.toarray())
        print(f"N=6: eigenvalues of K in [{ev.min():.3f}, {ev.max():.3f}], {int((ev < 0).sum())} negative, {int((ev > 0).sum())} positive")
        assert ev.min() < 0 < ev.max() and (ev < 0).sum() == sd["m"] and (ev > 0).sum() == sd["n"]
    st, it, resid, x = minres_ref(lambda u: K @ u, b, M, tol=1e-10, max_iter=500)
    true = np.linalg.norm(b - K @ x) / np.linalg.norm(b)
    assert st == 0 and true < 1e-10 and resid == pytest.approx(true, rel=1e-12)
    xs = scipy_minres(K, b, M, it)
    d = kr.rel(x, xs)
    print(f"N={N} ({K.shape[0]} rows): {it} iterations, true residual {true:.3e}; restatement vs scipy.sparse.linalg.minres x {d:.3e} (bar {X_BAR:.0e})")
    assert d <= X_BAR


def test_exits(systems):
    tol = 1e-12
    # diag(1, −1), b = (1, 1): two distinct eigenvalues, two iterations
    st, it, resid, x = minres_ref(lambda u: np.array([u[0], -u[1]]), np.array([1.0, 1.0]), tol=tol, max_iter=10)
    assert (st, it) == (0, 2) and resid < tol and np.allclose(x, [1.0, -1.0], rtol=0, atol=1e-15)
    # [[0, 1], [1, 0]], b = (1, 0): zero diagonal, δ = 0 in both iterations
    st, it, resid, x = minres_ref(lambda u: np.array([u[1], u[0]]), np.array([1.0, 0.0]), tol=tol, max_iter=10)
    assert (st, it) == (0, 2) and resid == 0.0 and np.array_equal(x, [0.0, 1.0])
    # [[1, 0], [0, 0]], b = (0, 1): b lies in the null space — singular and inconsistent; dyadic throughout
    x0 = np.array([0.25, -0.5])
    st, it, resid, x = minres_ref(lambda u: np.array([u[0], 0.0]), np.array([0.0, 1.0]), tol=tol, max_iter=10)
    assert (st, it) == (3, 1) and resid == 1.0 and not x.any()
    st, it, resid, x = minres_ref(lambda u: np.array([u[0], 0.0]), np.array([0.25, 1.0]), tol=tol, max_iter=10, x0=x0)
    assert (st, it) == (3, 1) and resid == 1.0 / np.sqrt(0.0625 + 1.0) and np.array_equal(x, x0)
    # a negative definite "preconditioner"
    sd, M, b = systems(6)
    K = sd["K"]
    st, it, resid, x = minres_ref(lambda u: K @ u, b, lambda u: -u, tol=tol, max_iter=10)
    assert (st, it) == (2, 0) and resid == 1.0 and not x.any()
    # out of iterations: the reported residual is the true one
    st, it, resid, x = minres_ref(lambda u: K @ u, b, M, tol=tol, max_iter=3)
    true = np.linalg.norm(b - K @ x) / np.linalg.norm(b)
    print(f"max_iter 3 on 6³: resid {resid:.6e}, recomputed {true:.6e}")
    assert (st, it) == (1, 3) and resid > tol and abs(resid - true) <= 1e-12 * true
    # max_iter 0: nothing done, the start's residual
    st, it, resid, x = minres_ref(lambda u: K @ u, b, M, tol=tol, max_iter=0)
    assert (st, it) == (1, 0) and resid == 1.0 and not x.any()


def test_recalibration(systems):
    """|η| is the residual in the M⁻¹ norm: the first estimate κ·|η| falls below tol before the 2-norm does; the true residual refuses, κ is
    recalibrated from it and the recurrence goes on — status 0 is reported on a true residual below tol"""
    sd, M, b = systems(8)
    K = sd["K"]
    checks = []
    st, it, resid, x = minres_ref(lambda u: K @ u, b, M, tol=1e-10, max_iter=500, checks=checks)
    true = np.linalg.norm(b - K @ x) / np.linalg.norm(b)
    print(f"8³ tol 1e-10: {it} iterations, {len(checks)} true-residual checks {[(j, f'{e:.2e}', f'{r:.2e}') for j, e, r in checks]}")
    assert st == 0 and true < 1e-10
    assert len(checks) >= 2 and all(r >= 1e-10 for _, _, r in checks[:-1]) and checks[-1][2] < 1e-10 and checks[-1][0] == it
    assert all(e < 1e-10 for _, e, _ in checks)
    # the same x as a run that is simply cut at that count: the checks do not disturb the recurrence
    st2, it2, _, x2 = minres_ref(lambda u: K @ u, b, M, tol=1e-300, max_iter=it)
    assert (st2, it2) == (1, it) and np.array_equal(x, x2)


def test_update_ref_is_the_scalar_loop():
    rng = np.random.default_rng(5)
    z, wp, w, x = (rng.standard_normal(7) for _ in range(4))
    inv_g, a3, a2, a1, step = 0.7, -0.3, 1.9, 2.3, -0.45
    wn, xn = update_ref(inv_g, a3, a2, a1, step, z, wp, w, x)
    for i in range(7):
        t = float(inv_g * z[i]) - float(a3 * wp[i])
        t = t - float(a2 * w[i])
        t = t / a1
        assert wn[i] == t and xn[i] == x[i] + float(step * t)


@pytest.mark.parametrize("n", [2, 3, 513, 1500])
def test_banded_sym_is_symmetric_indefinite_and_well_conditioned(n):
    op = banded_sym(n, seed=3)
    rp, ci, v = op.csr()
    A = sps.csr_matrix((v, ci, rp), shape=(n, n))
    assert abs(A - A.T).max() == 0.0
    d = A.diagonal()
    assert (d > 0).any() and (d < 0).any()
    ev = np.linalg.eigvalsh(A.toarray())
    print(f"n={n}: spectrum [{ev.min():.3f}, {ev.max():.3f}], smallest |λ| {np.abs(ev).min():.3f}, condition {np.abs(ev).max() / np.abs(ev).min():.2f}")
    assert ev.min() < 0 < ev.max() and np.abs(ev).min() >= 0.5 and np.abs(ev).max() <= 9.5
    xr = np.random.default_rng(n).standard_normal(n)
    assert kr.rel(op.apply(xr), A @ xr) <= 1e-15


def test_long_double_run_agrees_with_float64():
    """the dtype switch: the same statements in np.longdouble, 12 fixed steps on the banded operator"""
    op = banded_sym(513, seed=3)
    b = np.random.default_rng(513).standard_normal(513)
    r64 = minres_ref(op.apply, b, None, tol=1e-300, max_iter=12)
    rld = minres_ref(op.apply, b, None, tol=1e-300, max_iter=12, dtype=np.longdouble)
    assert r64[0] == rld[0] == 1 and r64[1] == rld[1] == 12 and rld[3].dtype == np.longdouble
    d = kr.rel(r64[3], rld[3])
    print(f"float64 vs long double after 12 steps: x {d:.3e}, resid {r64[2]:.6e} vs {float(rld[2]):.6e}")
    assert d <= 2e-15 and abs(r64[2] - float(rld[2])) <= 1e-10 * float(rld[2])
