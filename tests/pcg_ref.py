"""numpy restatement of mgs_pcg (include/mgs.h), statement by statement — the oracle side of the PCG tests.  `A` is an
oracle_py.Csr (or a callable v -> A·v), `precond` a callable v -> B·v (orc.Hier(...).vcycle) or None for the identity.  With
flexible=False it is the textbook method scipy.sparse.linalg.cg implements (tests/test_pcg_restatement_cpu.py pins that); the
additions are the true-residual confirmation before status 0 and the two positivity checks.

dtype = np.float64 (default) keeps every operation and every bit of the earlier float64-only version.  Any other dtype
(np.longdouble: the extended-precision yardstick of tests/krylov_ref.py) runs the same statements in that type, with the inner
products summed pairwise (np.sum) instead of through BLAS, which numpy does not have for it."""
import numpy as np


def _dot(a, b):
    return float(a @ b) if a.dtype == np.float64 else (a * b).sum()


def _norm(a):
    return np.linalg.norm(a) if a.dtype == np.float64 else np.sqrt((a * a).sum())


def pcg_ref(A, b, precond=None, tol=1e-6, max_iter=10000, flexible=False, x0=None, dtype=np.float64):
    """→ (status, iterations, resid, x); status 0 converged / 1 max_iter / 2 r·z not positive / 3 p·A·p not positive"""
    spmv = A if callable(A) else A.spmv
    b = np.ascontiguousarray(b, dtype=dtype)
    x = np.zeros(b.shape[0], dtype=dtype) if x0 is None else np.array(x0, dtype=dtype)
    normb = _norm(b)
    if normb == 0.0:
        normb = 1.0
    r = b - spmv(x)
    resid = _norm(r) / normb
    if resid <= tol:
        return 0, 0, resid, x
    p = q = None
    alpha = rho_prev = 0.0
    restart = True
    for i in range(1, max_iter + 1):
        z = np.array(r, copy=True) if precond is None else precond(r)
        rho = _dot(r, z)
        zq = _dot(z, q) if (flexible and not restart) else 0.0
        if not rho > 0:
            return 2, i, resid, x
        if restart:
            p = z.copy()
            restart = False
        else:
            beta = -alpha * zq / rho_prev if flexible else rho / rho_prev
            p = z + beta * p
        q = spmv(p)
        pq = _dot(p, q)
        if not pq > 0:
            return 3, i, resid, x
        alpha = rho / pq
        x = x + alpha * p
        r = r - alpha * q
        resid = _norm(r) / normb
        rho_prev = rho
        if resid < tol:
            r = b - spmv(x)
            resid = _norm(r) / normb
            if resid < tol:
                return 0, i, resid, x
            restart = True
    return 1, max_iter, resid, x
