"""The host dense algebra of mgs_eig_lobpcg (multigridsolver_amd/csrc/eig_dense.hpp) in a stand-alone CPU program (tests/cpp_eig/eig_dense_main.cpp,
its own main, g++ -Wall with no warning, no HIP header, no libmgs): the cyclic Jacobi eigensolver against numpy.linalg.eigh, the generalised
problem G_A·v = θ·G_B·v with κ(G_B) up to 1e8, and the pivot rule's refusals.

Bars.  `sweeps` Jacobi sweeps are at most n²·sweeps/2 rotations, each a backward error of a few ε·‖G‖_F to first order: eigenvalues agree with
eigh's within n²·sweeps·ε·‖G‖_F.  The generalised problem: ‖VᵀG_AV − Θ‖ within the same bound times κ(G_B), with G = G_A: n²·sweeps·ε·‖G_A‖_F·κ(G_B);
‖VᵀG_BV − I‖ within n²·sweeps·ε·‖G_B‖_F·κ(G_B).  θ_j against the NumPy reference has a bar of its own, because the eigenvalues of the pencil reach
‖G_A‖·‖G_B⁻¹‖, far above ‖G_A‖_F, and both the routine and the reference (which goes through the same Cholesky reduction) carry a RELATIVE error of
κ(G_B)·ε on each of them: |θ_j − ref_j| <= n²·sweeps·ε·κ(G_B)·max(|ref_j|, ‖G_A‖_F) — for eigenvalues up to ‖G_A‖_F that is the bar above."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

EPS = np.finfo(np.float64).eps
SRC = os.path.join(REPO, "tests", "cpp_eig", "eig_dense_main.cpp")
INC = os.path.join(REPO, "multigridsolver_amd", "csrc")


def _compile(out, extra=()):
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O1", "-Wall", *extra, "-I", INC, "-o", out, SRC], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in r.stderr, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("eig_dense") / "eig_dense"))


def _run(exe, tmp, mode, GA, GB=None, m_rule=8):
    n = GA.shape[0]
    parts = [np.array([mode, n, m_rule], dtype=np.float64), np.ascontiguousarray(GA, dtype=np.float64).ravel()]
    if GB is not None:
        parts.append(np.ascontiguousarray(GB, dtype=np.float64).ravel())
    fin, fout = os.path.join(str(tmp), "in.f64"), os.path.join(str(tmp), "out.f64")
    np.concatenate(parts).tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    o = np.fromfile(fout)
    return int(o[0]), o[1:1 + n], o[1 + n:].reshape(n, n)


def _sym(n, seed):
    B = np.random.default_rng(seed).standard_normal((n, n))
    return 0.5 * (B + B.T)


def _check_jacobi(exe, tmp, G):
    n = G.shape[0]
    sweeps, w, V = _run(exe, tmp, 0, G)
    assert sweeps >= 1
    bar = n * n * sweeps * EPS * max(np.linalg.norm(G), np.finfo(np.float64).tiny)
    ref = np.linalg.eigvalsh(G)
    print(f"n={n} sweeps={sweeps} max|w-ref|={np.abs(w - ref).max():.3e} bar={bar:.3e}")
    assert np.all(np.diff(w) >= 0)
    assert np.abs(w - ref).max() <= bar
    assert np.abs(V.T @ V - np.eye(n)).max() <= n * n * sweeps * EPS * np.sqrt(n)
    assert np.abs(V.T @ G @ V - np.diag(w)).max() <= bar


@pytest.mark.parametrize("n", [1, 2, 3, 12, 24])
def test_jacobi_random_symmetric(exe, tmp_path, n):
    _check_jacobi(exe, tmp_path, _sym(n, 100 + n))


def test_jacobi_diagonal_and_repeated(exe, tmp_path):
    _check_jacobi(exe, tmp_path, np.diag([3.0, -1.0, 2.0, 2.0, 0.0, 7.5]))
    Q = np.linalg.qr(np.random.default_rng(3).standard_normal((9, 9)))[0]
    _check_jacobi(exe, tmp_path, Q @ np.diag([1.0, 1.0, 1.0, 2.0, 2.0, 5.0, 5.0, 5.0, 9.0]) @ Q.T)      # repeated eigenvalues


@pytest.mark.parametrize("n,kappa", [(3, 1e0), (12, 1e4), (24, 1e8), (24, 1e2)])
def test_generalized(exe, tmp_path, n, kappa):
    rng = np.random.default_rng(int(n + np.log10(kappa)))
    GA = _sym(n, 7 * n)
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    GB = Q @ np.diag(np.logspace(0, -np.log10(kappa), n)) @ Q.T
    GB = 0.5 * (GB + GB.T)
    sweeps, th, V = _run(exe, tmp_path, 1, GA, GB, m_rule=min(n, 8))
    assert sweeps >= 1
    L = np.linalg.cholesky(GB)
    Li = np.linalg.inv(L)
    M = Li @ GA @ Li.T
    ref = np.linalg.eigvalsh(0.5 * (M + M.T))
    kb = np.linalg.cond(GB)
    unit = n * n * sweeps * EPS * kb
    bar_a, bar_b = unit * np.linalg.norm(GA), unit * np.linalg.norm(GB)
    bar_th = unit * np.maximum(np.abs(ref), np.linalg.norm(GA))
    err_a, err_b = np.abs(V.T @ GA @ V - np.diag(th)).max(), np.abs(V.T @ GB @ V - np.eye(n)).max()
    print(f"n={n} kappa={kb:.2e} sweeps={sweeps} |VtAV-Th|={err_a:.3e} (bar {bar_a:.3e}) |VtBV-I|={err_b:.3e} (bar {bar_b:.3e}) "
          f"max |th-ref|/bar_j={np.max(np.abs(th - ref) / bar_th):.3e}")
    assert np.all(np.diff(th) >= 0)
    assert err_a <= bar_a
    assert err_b <= bar_b
    assert np.all(np.abs(th - ref) <= bar_th)


def test_pivot_rule_refuses(exe, tmp_path):
    GA = _sym(4, 1)
    B = np.random.default_rng(2).standard_normal((4, 3))
    singular = np.zeros((4, 4)); singular[:3, :3] = np.eye(3)      # an exactly singular G_B: a zero pivot
    assert _run(exe, tmp_path, 1, GA, singular)[0] == 0
    twice = np.ones((2, 2))                                         # two identical columns: the second pivot is exactly 0
    assert _run(exe, tmp_path, 1, _sym(2, 5), twice)[0] == 0
    nan = B @ B.T + np.eye(4); nan[2, 1] = nan[1, 2] = np.nan
    assert _run(exe, tmp_path, 1, GA, nan)[0] == 0
    good = B @ B.T + np.eye(4)
    assert _run(exe, tmp_path, 1, GA, good)[0] >= 1
    GAn = GA.copy(); GAn[0, 0] = np.inf
    assert _run(exe, tmp_path, 1, GAn, good)[0] == -1


def test_zero_diagonal_and_sweep_count(exe, tmp_path):
    """a matrix with a zero diagonal (the relative rotation bar is 0 there): converges, and the count returned is that of the sweeps done"""
    G = np.array([[0.0, 1.0, 0.5], [1.0, 0.0, -2.0], [0.5, -2.0, 0.0]])
    _check_jacobi(exe, tmp_path, G)
    sweeps, w, _ = _run(exe, tmp_path, 0, np.diag([2.0, 1.0]))
    assert sweeps == 1 and np.array_equal(w, [1.0, 2.0])      # one sweep, which made no rotation


def test_under_sanitizers(tmp_path):
    """the same program with -fsanitize=address,undefined, run once on the largest case: host code with its own main"""
    exe = _compile(str(tmp_path / "eig_dense_san"), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    n = 24
    B = np.random.default_rng(9).standard_normal((n, n))
    sweeps, th, V = _run(exe, tmp_path, 1, _sym(n, 4), B @ B.T + np.eye(n))
    assert sweeps >= 1 and np.isfinite(th).all() and np.isfinite(V).all()
