"""CPU checks of tests/eig_ref.py, the NumPy restatement the GPU tests of the block passes and of mgs_eig_lobpcg compare with.

1. The restated Gram and combine equal exact rational arithmetic (fractions) rounded after every operation in the kernels' order.
2. On a fixture built for it they differ from U.T @ V, from S @ C, from another summation order and from the fused-multiply-add forms, so the
   bit-for-bit GPU comparison notices a wrong order or a contraction.
3. The restated solver reaches tol 1e-6 on every fixture with no preconditioner and with the dense inverse (regularised as mgs_hier_finalize
   does for the singular ones), in the iterations recorded in eig_ref.ITERATIONS (the GPU test reads them).
4. Its θ_j meet |θ_j − λ_j| <= resid_j·‖A‖∞ + n·ε·‖A‖∞: the residual theorem for a symmetric matrix and a unit vector, plus the backward error of
   the reference eigenvalues (numpy.linalg.eigvalsh).
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import blas1_ref as b1
import eig_ref as E

EPS = np.finfo(np.float64).eps


def fl(x):
    """a Fraction rounded to the nearest double (ties to even: float() of a Fraction is correctly rounded)"""
    return float(x)


def _exact_reduce(p, nb, vec):
    """blas1_ref.reduce_terms on the already rounded terms p, every addition through exact rationals rounded once"""
    add = lambda a, b: fl(Fraction(a) + Fraction(b))
    n, TB = len(p), b1.TB
    lanes = [0.0] * (nb * TB)
    if vec:
        n2 = n // 2
        for i in range(n2):
            t = i % (nb * TB)
            lanes[t] = add(lanes[t], p[2 * i]); lanes[t] = add(lanes[t], p[2 * i + 1])
        if n & 1:
            lanes[0] = add(lanes[0], p[n - 1])
    else:
        for i in range(n):
            lanes[i % (nb * TB)] = add(lanes[i % (nb * TB)], p[i])
    part = []
    for w in range(nb):
        s = 0.0
        for q in range(TB // 64):
            v = lanes[w * TB + q * 64:w * TB + (q + 1) * 64]
            off = 32
            while off:
                v = [add(v[l], v[l + off]) if l + off < 2 * off else v[l] for l in range(len(v))]
                off >>= 1
            s = add(s, v[0])
        part.append(s)
    sh = [0.0] * TB
    for i, v in enumerate(part):
        sh[i % TB] = add(sh[i % TB], v)
    w = TB // 2
    while w:
        for t in range(w):
            sh[t] = add(sh[t], sh[t + w])
        w >>= 1
    return sh[0]


@pytest.mark.parametrize("n,vec", [(1, False), (63, True), (63, False), (1030, True), (1031, True), (1031, False)])
def test_gram_equals_exact_rationals(n, vec):
    rng = np.random.default_rng(n + vec)
    U, V = [rng.standard_normal(n) for _ in range(2)], [rng.standard_normal(n) for _ in range(3)]
    nb = E.gram_launch(n, aligned=vec)[1]
    G = E.gram(U, V, nb, vec)
    for a in range(2):
        for b in range(3):
            p = [fl(Fraction(float(U[a][i])) * Fraction(float(V[b][i]))) for i in range(n)]
            assert G[a, b] == _exact_reduce(p, nb, vec), (a, b)


def test_combine_equals_exact_rationals():
    rng = np.random.default_rng(4)
    S, Cm = [rng.standard_normal(37) for _ in range(5)], rng.standard_normal((5, 3))
    Y = E.combine(S, Cm)
    for j in range(3):
        for i in range(37):
            y = fl(Fraction(float(Cm[0, j])) * Fraction(float(S[0][i])))
            for a in range(1, 5):
                y = fl(Fraction(y) + Fraction(fl(Fraction(float(Cm[a, j])) * Fraction(float(S[a][i])))))
            assert Y[j][i] == y


def test_gram_symmetric_route_is_symmetric_and_mirrors():
    rng = np.random.default_rng(8)
    U = [rng.standard_normal(300) for _ in range(10)]
    G = E.gram(U, U, 1, True, same=True)
    assert np.array_equal(G, G.T)
    full = E.gram(U, U, 1, True, same=False)
    assert np.array_equal(G, full)      # products commute bit for bit and every entry adds them in the same order


def test_restatement_differs_from_blas_and_fma():
    """the fixture: Gaussian data over a few binades, so that order and contraction change the last bits"""
    rng = np.random.default_rng(21)
    n = 1031
    U = [rng.standard_normal(n) * np.exp2(rng.integers(-2, 3, n)) for _ in range(3)]
    vec, nb = E.gram_launch(n)
    G = E.gram(U, U, nb, vec, same=True)
    assert not np.array_equal(G, np.array(U) @ np.array(U).T)
    assert not np.array_equal(G, E.gram(U, U, nb, not vec, same=True))      # the 8-byte form is another order
    assert not np.array_equal(G, E.gram(U, U, 1, vec, same=True))           # and so is another grid
    # the odd last element is added after the lane's pairs: on 32 blocks of three elements the other order changes some result
    tails = [(E.gram([U[0][i:i + 3]], [U[1][i:i + 3]], 1, True)[0, 0], E.gram([U[0][i:i + 3]], [U[1][i:i + 3]], 1, True, defect="tail_first")[0, 0]) for i in range(0, 96, 3)]
    assert any(a != b for a, b in tails)
    Cm = rng.standard_normal((3, 2))
    Y = E.combine(U, Cm)
    assert not np.array_equal(np.array(Y).T, np.array(U).T @ Cm)
    assert not np.array_equal(np.array(Y), np.array(E.combine(U, Cm, defect="descending")))
    if hasattr(math, "fma"):
        fused = [math.fma(Cm[1, 0], U[1][i], Cm[0, 0] * U[0][i]) for i in range(n)]
        fused = [math.fma(Cm[2, 0], U[2][i], fused[i]) for i in range(n)]
        assert not np.array_equal(Y[0], np.array(fused))
        # a Gram entry of n = 2 on the 16-byte path is lane 0's two products added in turn: contracted, the second would be fused into the sum
        a, b = U[0][:2], U[1][:2]
        contracted = [math.fma(x[1], y[1], x[0] * y[0]) for x, y in ((U[0][i:i + 2], U[1][i:i + 2]) for i in range(0, 64, 2))]
        plain = [E.gram([U[0][i:i + 2]], [U[1][i:i + 2]], 1, True)[0, 0] for i in range(0, 64, 2)]
        assert E.gram([a], [b], 1, True)[0, 0] == a[0] * b[0] + a[1] * b[1]
        assert contracted != plain


@pytest.fixture(scope="module")
def solved():
    out = {}
    for name, m in E.CASES:
        A, lab = E.fixture(name)
        for pk in ("none", "inverse"):
            M = None if pk == "none" else E.dense_inverse(A, lab)
            out[(name, m, pk)] = (A, lab, E.lobpcg(A, E.start_block(A.shape[0], m), M, E.projector(lab), tol=1e-6, max_iter=200))
    return out


@pytest.mark.parametrize("pk", ["none", "inverse"])
@pytest.mark.parametrize("name,m", E.CASES)
def test_solver_converges_within_the_bound(solved, name, m, pk):
    A, lab, r = solved[(name, m, pk)]
    n = A.shape[0]
    anorm = np.abs(A).sum(axis=1).max()
    assert r["status"] == 0 and (r["resid"] < 1e-6).all()
    # BLAS may round A @ X differently from one machine to the next, which can move the last iteration: one iteration of slack, no more
    assert abs(r["iterations"] - E.ITERATIONS[(name, m, pk)]) <= 1, (r["iterations"], E.ITERATIONS[(name, m, pk)])
    lam = E.complement_eigs(A, lab)[0][:m]
    X, th = r["X"], r["theta"]
    true = np.linalg.norm(A @ X - X * th, axis=0) / anorm
    assert np.all(np.abs(th - lam) <= true * anorm + n * EPS * anorm), (th, lam)
    assert np.abs(X.T @ X - np.eye(m)).max() <= 64 * m * EPS
    if lab is not None:
        for f in range(int(lab.max()) + 1):
            z = (lab == f).astype(np.float64)
            assert np.abs(z @ X).max() / np.sqrt(z.sum()) <= n * EPS
        assert th[0] > 0.1      # the null vectors are not returned


def test_preconditioner_pays_and_status_paths():
    A, lab = E.fixture("poisson8d")
    assert E.ITERATIONS[("poisson8d", 4, "inverse")] < E.ITERATIONS[("poisson8d", 4, "none")]
    X0 = E.start_block(512, 4)
    r = E.lobpcg(A, X0, None, None, tol=1e-6, max_iter=2)
    assert r["status"] == 1 and r["iterations"] == 2 and np.all(np.diff(r["theta"]) >= 0)
    assert np.abs(r["X"].T @ r["X"] - np.eye(4)).max() <= 64 * 4 * EPS
    X0[:, 2] = X0[:, 0]
    r = E.lobpcg(A, X0, None, None)
    assert r["status"] == 2 and r["iterations"] == 0 and np.array_equal(r["X"], X0)
