"""Pins the yardstick of the PCG tests: the numpy restatement tests/pcg_ref.py (flexible=False) is the method
scipy.sparse.linalg.cg implements — same iteration count and the same x with the same preconditioner — on the pinned input
poisson2d(100) + the reference's poisson10000promatrix.mtx, ω = 0.5, V(1,1).  The true-residual confirmation, which scipy does
not have, passes at its first attempt there, so it does not alter the comparison."""
import numpy as np
import pytest

from pcg_ref import pcg_ref


@pytest.mark.parametrize("tol,its", [(1e-6, 28), (1e-10, 44)])
def test_pcg_ref_equals_scipy_cg(orc, inputs, tol, its):
    import scipy.sparse.linalg as spla
    A = orc.poisson2d(100)
    P = orc.Csr.read(inputs["poisson10000promatrix"])
    H = orc.Hier(A, [P], omega=0.5, nu1=1, nu2=1)
    n = A.shape[0]
    b = orc.rand_rhs(n)
    st, it, resid, x = pcg_ref(A, b, H.vcycle, tol=tol, max_iter=500)
    count = [0]
    M = spla.LinearOperator((n, n), matvec=lambda v: H.vcycle(np.ascontiguousarray(v, dtype=np.float64).ravel()), dtype=np.float64)
    xs, info = spla.cg(A.to_scipy(), b, rtol=tol, atol=0.0, maxiter=500, M=M, callback=lambda _x: count.__setitem__(0, count[0] + 1))
    print(f"tol {tol:g}: pcg_ref {it} iterations (status {st}, resid {resid:.4e}); scipy cg {count[0]} iterations (info {info}); "
          f"x rel diff {np.linalg.norm(x - xs) / np.linalg.norm(xs):.3e}")
    assert st == 0 and info == 0
    assert it == count[0] == its
    assert np.linalg.norm(x - xs) <= 1e-12 * np.linalg.norm(xs)
    assert np.linalg.norm(b - A.spmv(x)) / np.linalg.norm(b) < tol
    # the flexible β (equal to the classical one in exact arithmetic for a fixed symmetric operator) reaches the same tolerance
    stf, itf, _, xf = pcg_ref(A, b, H.vcycle, tol=tol, max_iter=500, flexible=True)
    print(f"tol {tol:g}: flexible pcg_ref {itf} iterations")
    assert stf == 0 and np.linalg.norm(b - A.spmv(xf)) / np.linalg.norm(b) < tol
