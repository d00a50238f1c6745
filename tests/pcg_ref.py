"""numpy restatement of mgs_pcg (include/mgs.h), statement by statement — the oracle side of the PCG tests.  `A` is an
oracle_py.Csr, `precond` a callable v -> B·v (orc.Hier(...).vcycle) or None for the identity.  With flexible=False it is the
textbook method scipy.sparse.linalg.cg implements (tests/test_pcg_restatement_cpu.py pins that); the additions are the
true-residual confirmation before status 0 and the two positivity checks."""
import numpy as np


def pcg_ref(A, b, precond=None, tol=1e-6, max_iter=10000, flexible=False, x0=None):
    """→ (status, iterations, resid, x); status 0 converged / 1 max_iter / 2 r·z not positive / 3 p·A·p not positive"""
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.zeros(A.shape[0]) if x0 is None else np.array(x0, dtype=np.float64)
    normb = np.linalg.norm(b)
    if normb == 0.0:
        normb = 1.0
    r = b - A.spmv(x)
    resid = np.linalg.norm(r) / normb
    if resid <= tol:
        return 0, 0, resid, x
    p = q = None
    alpha = rho_prev = 0.0
    restart = True
    for i in range(1, max_iter + 1):
        z = np.array(r, copy=True) if precond is None else precond(r)
        rho = float(r @ z)
        zq = float(z @ q) if (flexible and not restart) else 0.0
        if not rho > 0:
            return 2, i, resid, x
        if restart:
            p = z.copy()
            restart = False
        else:
            beta = -alpha * zq / rho_prev if flexible else rho / rho_prev
            p = z + beta * p
        q = A.spmv(p)
        pq = float(p @ q)
        if not pq > 0:
            return 3, i, resid, x
        alpha = rho / pq
        x = x + alpha * p
        r = r - alpha * q
        resid = np.linalg.norm(r) / normb
        rho_prev = rho
        if resid < tol:
            r = b - A.spmv(x)
            resid = np.linalg.norm(r) / normb
            if resid < tol:
                return 0, i, resid, x
            restart = True
    return 1, max_iter, resid, x
