"""CPU tests of tests/nullspace_ref.py (the numpy restatement the GPU tests of the constant null space are held against) on the 6³ and
9³ Neumann operators, hierarchy by tests/agmg_ref.py's restatement of the device aggregation with coarse_rows = 60."""
import numpy as np
import pytest

import agmg_ref
import nullspace_ref as ns
from multigridsolver_amd.synthetic import neumann3d

EPS = np.finfo(np.float64).eps
TOL = 1e-10


@pytest.fixture(scope="module", params=[6, 9])
def problem(request):
    N = request.param; n = N ** 3
    A = agmg_ref.csr(n, n, *neumann3d(N))
    As, aggs = ns.build_hierarchy(A, 60)
    assert len(As) >= 2 and As[-1].shape[0] <= 60
    b = np.random.default_rng(N).standard_normal(n) + 3.0          # not consistent: the solvers see Πb
    return dict(N=N, n=n, A=A, As=As, aggs=aggs, b=b, dense=A.toarray())


def test_generator_has_the_constant_null_space(problem):
    A, N = problem["A"], problem["N"]
    assert abs(A - A.T).nnz == 0
    assert np.array_equal(A @ np.ones(problem["n"]), np.zeros(problem["n"]))
    assert np.array_equal(A.diagonal(), -(A - __import__("scipy.sparse").sparse.diags(A.diagonal())).sum(axis=1).A1)
    assert A.diagonal().min() == 3 and A.diagonal().max() == 6 and A.nnz == 7 * N ** 3 - 6 * N ** 2
    assert all(np.all(np.diff(A.indices[A.indptr[i]:A.indptr[i + 1]]) > 0) for i in range(problem["n"]))
    for Ac in problem["As"][1:]:                                     # every level inherits it: P·1_c = 1
        assert np.abs(Ac @ np.ones(Ac.shape[0])).max() <= 8 * EPS * np.abs(Ac.data).max()


def test_pcg_reaches_tol_and_matches_the_pseudo_inverse(problem):
    A, b = problem["A"], problem["b"]
    pb = ns.project(b)
    cyc = ns.Cycle(problem["As"], problem["aggs"], 0.6)
    st, it, resid, x = ns.pcg(A, b, cyc.vcycle, tol=TOL, max_iter=200)
    true = np.linalg.norm(ns.project(b - A @ x)) / np.linalg.norm(pb)
    print(f"N {problem['N']}: {len(problem['As'])} levels, PCG status {st}, {it} iterations, reported {resid:.3e}, true {true:.3e}, mean(x) {x.mean():.2e}")
    assert st == 0 and resid < TOL and true <= TOL * (1 + 1e-3)
    assert abs(x.mean()) <= problem["n"] * EPS * np.abs(x).max()
    # x and x* = A⁺Πb both have zero mean, so x − x* = −A⁺r with ‖r‖ <= tol·‖Πb‖: ‖x − x*‖ <= tol·‖Πb‖/λ_min⁺; the factor 2 covers pinv's own residual
    lam = np.linalg.eigvalsh(problem["dense"])
    assert abs(lam[0]) <= problem["n"] * EPS * lam[-1] and lam[1] > 1e-3
    xs = np.linalg.pinv(problem["dense"]) @ pb
    assert np.linalg.norm(x - xs) <= 2 * TOL * np.linalg.norm(pb) / lam[1]
    # the other two projected loops land on the same solution, from a guess with a constant component
    x0 = np.full(problem["n"], 5.0)
    for name, run in (("bicgstab", lambda: ns.bicgstab(A, b, cyc.vcycle, tol=TOL, max_iter=200, x0=x0)),
                      ("fgcr", lambda: ns.fgcr(A, b, cyc.vcycle, restart=10, tol=TOL, max_iter=200, x0=x0))):
        st2, it2, resid2, x2 = run()
        print(f"   {name}: status {st2}, {it2} iterations, {resid2:.3e}")
        assert st2 == 0 and abs(x2.mean()) <= problem["n"] * EPS * np.abs(x2).max()
        assert np.linalg.norm(x2 - xs) <= 2 * TOL * np.linalg.norm(pb) / lam[1]


def test_regularised_inverse_is_the_pseudo_inverse_on_the_complement(problem):
    Ac = problem["As"][-1]; n = Ac.shape[0]
    M = ns.regularised(Ac)
    cond = np.linalg.cond(M)
    plain = np.linalg.cond(Ac.toarray())
    b = ns.project(np.random.default_rng(1).standard_normal(n))
    x = np.linalg.solve(M, b)
    xs = np.linalg.pinv(Ac.toarray()) @ b
    err = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    print(f"N {problem['N']}: coarsest {n} rows, cond regularised {cond:.1f} (plain {plain:.2e}), rel diff to pinv {err:.2e}")
    assert cond < 1e3 < plain
    assert err <= 8 * n * EPS * cond
    # its eigenvalue on 1 is s = max|a_ij|
    s = np.abs(Ac.data).max()
    assert np.linalg.norm(M @ np.ones(n) - s * np.ones(n)) <= 8 * n * EPS * s * np.sqrt(n)
