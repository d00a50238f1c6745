"""CPU-only: the restatement of mgs_eig_lobpcg_gen (tests/eig_gen_ref.py) against scipy.linalg.eigh(A, B), against eig_ref.lobpcg for B = I, and
the fixture of the residual pass: inputs on which fl(ax − fl(θ·bx)) differs from the exactly rounded and from the fused result.

Bars: |Δθ| ≤ 1e-8·θ (a residual of 1e-6 relative to ‖A‖∞ + θ‖B‖∞ bounds the eigenvalue error by its square over the gap, which is far below;
1e-8 leaves room for the gap 0.057 of (poisson8d, 7)); ‖XᵀBX − I‖ ≤ 1e-12 (a few hundred roundings of a Gram entry of unit columns)."""
import math
from fractions import Fraction

import numpy as np
import pytest
import scipy.linalg

import blas1_ref as b1
import eig_gen_ref as G
import eig_ref as E

TOL = 1e-6
_HOST = {}


def host(name):
    if name not in _HOST:
        A, _ = E.fixture(name)
        B = G.mass(name)
        w = scipy.linalg.eigh(A, B, eigvals_only=True)
        _HOST[name] = (A, B, w, E.dense_inverse(A, None))
    return _HOST[name]


def test_the_mass_matrix_is_symmetric_and_strictly_diagonally_dominant():
    for name in ("poisson6", "poisson8d"):
        A, B, w, _ = host(name)
        assert np.array_equal(B, B.T) and np.array_equal(A, A.T)
        d = np.diag(B)
        assert np.all(d > np.abs(B).sum(axis=1) - d) and np.all(d > 0)
        assert np.abs(A @ B - B @ A).max() > 1e-3      # B is no polynomial in A: the two do not commute


@pytest.mark.parametrize("pk", ["none", "inverse"])
@pytest.mark.parametrize("name,m", G.CASES)
def test_restatement_against_scipy(name, m, pk):
    A, B, w, Ainv = host(name)
    r = G.lobpcg_gen(A, B, E.start_block(A.shape[0], m), None if pk == "none" else Ainv, tol=TOL, max_iter=200)
    X, th = r["X"], r["theta"]
    orth = np.abs(X.T @ B @ X - np.eye(m)).max()
    print(f"{name} m={m} {pk}: iterations {r['iterations']}, max|dtheta| {np.abs(th - w[:m]).max():.2e}, |XtBX-I| {orth:.2e}, restarts {r['restarts']}, spmv {r['spmv']}/{r['spmv_b']}")
    assert r["status"] == 0 and (r["resid"] < TOL).all()
    assert r["iterations"] == G.ITERATIONS[(name, m, pk)]
    assert np.all(np.diff(th) >= 0)
    assert np.all(np.abs(th - w[:m]) <= 1e-8 * w[:m]), (th, w[:m])
    assert orth <= 1e-12
    anorm, bnorm = np.abs(A).sum(axis=1).max(), np.abs(B).sum(axis=1).max()
    true = np.linalg.norm(A @ X - (B @ X) * th, axis=0) / (anorm + np.abs(th) * bnorm)
    assert np.all(np.abs(r["resid"] - true) <= 1e-12)
    assert r["restarts"] == 0
    assert r["spmv"] == 2 * r["spmv_b"]      # every block goes through A and through B once


def test_smallest_relative_gap_of_the_cases():
    gaps = {}
    for name, m in G.CASES:
        w = host(name)[2]
        gaps[(name, m)] = (w[m] - w[m - 1]) / w[m - 1]
    print(gaps)
    assert abs(min(gaps.values()) - 0.057) < 1e-3 and min(gaps, key=gaps.get) == ("poisson8d", 7)


@pytest.mark.parametrize("name,want", [("poisson6", 41), ("poisson8d", 45)])
def test_identity_mass_gives_the_standard_solver(name, want):
    A, _ = E.fixture(name)
    n = A.shape[0]
    r = G.lobpcg_gen(A, np.eye(n), E.start_block(n, 4), None, tol=TOL)
    r0 = E.lobpcg(A, E.start_block(n, 4), None, None, tol=TOL)
    assert r["iterations"] == r0["iterations"] == E.ITERATIONS[(name, 4, "none")] == want
    assert np.abs(r["theta"] - r0["theta"]).max() <= 1e-14


def test_statuses_of_the_restatement():
    A, B, w, _ = host("poisson6")
    X0 = E.start_block(216, 4)
    assert G.lobpcg_gen(A, -np.eye(216), X0)["status"] == 2
    r = G.lobpcg_gen(A, B, X0, max_iter=2)
    assert r["status"] == 1 and r["iterations"] == 2
    X1 = X0.copy(); X1[:, 2] = X1[:, 0]
    r = G.lobpcg_gen(A, B, X1)
    assert r["status"] == 2 and np.array_equal(r["X"], X1)


# ------------------------------------------------------------------------------------------------------------- the residual pass
def test_residual_fixture_tells_the_three_roundings_apart():
    ax, bx, th = G.residual_fixture(513)
    r, s = G.residual(ax, bx, th)
    exact = np.array([float(Fraction(float(a)) - Fraction(th) * Fraction(float(b))) for a, b in zip(ax, bx)])
    assert (r != exact).sum() > 50                                        # two roundings against one
    # and no further apart than the three roundings allow: the product's, the difference's, and that of the exact value itself
    assert np.all(np.abs(r - exact) <= (np.abs(th * bx) + np.abs(r) + np.abs(exact)) * 2.0 ** -53 * (1 + 2.0 ** -50))
    if hasattr(math, "fma"):
        f, sf = G.residual(ax, bx, th, defect="fused")
        assert np.array_equal(f, exact)                                   # the fused result is the exactly rounded one …
        assert sf != s                                                    # … and the norm tells
    # the expression, entry by entry, in Python floats
    assert all(float(x) == float(a) - th * float(b) for x, a, b in zip(r, ax, bx))


def test_residual_norm_is_dot_of_r_under_dot_launch():
    for n in (1, 2, 3, 511, 512, 513, 5000):
        ax, bx, th = G.residual_fixture(n)
        for launch in (dict(aligned=True), dict(aligned=False), dict(aligned=True, blas1_vec=0)):
            r, s = G.residual(ax, bx, th, **launch)
            assert s == b1.dot(r, r, **launch)
            vec, nb = b1.dot_launch(n, **launch)
            assert s == b1.reduce_terms(r * r, nb, vec)
    # the two arms associate differently: on some length the bits differ
    diff = 0
    for n in (511, 512, 513, 5000):
        ax, bx, th = G.residual_fixture(n)
        diff += G.residual(ax, bx, th, aligned=True)[1] != G.residual(ax, bx, th, aligned=False)[1]
    assert diff > 0
