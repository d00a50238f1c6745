"""numpy restatement of what the library does for a matrix declared MGS_NULLSPACE_CONSTANT (include/mgs.h: mgs_csr_set_nullspace) — the
oracle side of tests/test_gpu_nullspace.py, pinned by tests/test_nullspace_ref_cpu.py.  No GPU.

  * project(v) = v − sum(v)/n: the projection Π = I − 1·1ᵀ/n (k_project_const);
  * Cycle: the V(1,1) cycle from a zero guess over a hierarchy given as lists of CSR operators (scipy) and aggregate arrays, the
    coarsest solve np.linalg.solve(A_c + (s/n_c)·1·1ᵀ, ·) with s = max|a_ij| of A_c — what mgs_hier_finalize inverts;
  * pcg / bicgstab / fgcr: the projected loops of mgs_pcg, mgs_bicgstab and mgs_fgcr in the style of tests/pcg_ref.py and
    tests/krylov_ref.py; `precond` is a callable v -> M·v (Cycle(...).vcycle) or None for the identity.  They solve A·x = Πb, every true
    residual is Π(b − A·x), *tol is relative to ‖Πb‖, and the x returned has zero mean;
  * build_hierarchy: mgs_hier_coarsen's loop on tests/agmg_ref.py's restatement of the device aggregation (CPU tests; the GPU tests
    hand Cycle the device's own level operators and aggregates)."""
import numpy as np


def project(v):
    return v - v.sum() / v.size


def regularised(Ac):
    """dense A_c + (s/n_c)·1·1ᵀ, s = max|a_ij| over the stored entries of the scipy CSR matrix Ac"""
    n = Ac.shape[0]
    s = np.abs(Ac.data).max() if Ac.nnz else 0.0
    return Ac.toarray() + s / n


def build_hierarchy(A, coarse_rows, ktg=10.0, npass=2, tou=8.0, max_levels=32):
    """→ (As, aggs): level operators (scipy CSR) and the aggregate array of every level but the last"""
    import agmg_ref
    As, aggs, origin = [A], [], None
    while len(As) < max_levels and As[-1].shape[0] > coarse_rows:
        R = agmg_ref.aggregate(As[-1], ktg, npass, tou, origin=origin)
        if R.A_coarse.shape[0] == 0 or R.A_coarse.shape[0] > int(0.9 * As[-1].shape[0]):
            break
        aggs.append(np.asarray(R.agg, dtype=np.int64)); As.append(R.A_coarse.tocsr()); origin = R.origin
    return As, aggs


class Cycle:
    """V(1,1) with damped Jacobi (ω) from a zero guess: x = ωD⁻¹b, r = b − A·x, x += P·cycle(Pᵀr), x += ωD⁻¹(b − A·x); every row must lie in
    an aggregate (the condition mgs_hier_finalize checks for a declared null space).  nullspace=False: the plain coarsest solve."""

    def __init__(self, As, aggs, omega=0.6, nullspace=True):
        assert len(aggs) == len(As) - 1 and all((a >= 0).all() for a in aggs)
        self.As, self.aggs = As, [np.asarray(a, dtype=np.int64) for a in aggs]
        self.wd = [omega / A.diagonal() for A in As[:-1]]
        self.Mc = regularised(As[-1]) if nullspace else As[-1].toarray()

    def vcycle(self, b, l=0):
        if l == len(self.As) - 1:
            return np.linalg.solve(self.Mc, b)
        A, agg, wd = self.As[l], self.aggs[l], self.wd[l]
        x = wd * b
        r = b - A @ x
        ec = self.vcycle(np.bincount(agg, weights=r, minlength=self.As[l + 1].shape[0]), l + 1)
        x = x + ec[agg]
        return x + wd * (b - A @ x)


def _normb(b):
    nb = np.linalg.norm(project(b))
    return nb if nb != 0.0 else 1.0


def pcg(A, b, precond=None, tol=1e-6, max_iter=10000, flexible=False, x0=None):
    """→ (status, iterations, resid, x): tests/pcg_ref.py with z ← Πz after every preconditioner application, Π on every true residual
    and x ← Πx after the last update"""
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros(b.size) if x0 is None else np.array(x0, dtype=np.float64)
    normb = _normb(b)
    r = project(b - A @ x)
    resid = np.linalg.norm(r) / normb
    if resid <= tol:
        return 0, 0, resid, project(x)
    p = q = None
    alpha = rho_prev = 0.0
    restart = True
    for i in range(1, max_iter + 1):
        z = project(r.copy() if precond is None else precond(r))
        rho = float(r @ z)
        zq = float(z @ q) if (flexible and not restart) else 0.0
        if not rho > 0:
            return 2, i, resid, project(x)
        if restart:
            p = z.copy(); restart = False
        else:
            p = z + (-alpha * zq / rho_prev if flexible else rho / rho_prev) * p
        q = A @ p
        pq = float(p @ q)
        if not pq > 0:
            return 3, i, resid, project(x)
        alpha = rho / pq
        x = x + alpha * p
        r = r - alpha * q
        resid = np.linalg.norm(r) / normb
        rho_prev = rho
        if resid < tol:
            x = project(x)
            r = project(b - A @ x)
            resid = np.linalg.norm(r) / normb
            if resid < tol:
                return 0, i, resid, x
            restart = True
    return 1, max_iter, resid, project(x)


def bicgstab(A, b, precond=None, tol=1e-6, max_iter=10000, x0=None):
    """→ (status, iterations, resid, x): BiCGSTABiml (mgs_bicgstab) with both preconditioned vectors of an iteration projected, r₀ = Π(b − A·x₀)
    and x ← Πx before every return"""
    M = (lambda v: v.copy()) if precond is None else precond
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros(b.size) if x0 is None else np.array(x0, dtype=np.float64)
    normb = _normb(b)
    r = project(b - A @ x)
    rt = r.copy()
    rho_1 = float(rt @ r)
    resid = np.linalg.norm(r) / normb
    if resid <= tol:
        return 0, 0, resid, project(x)
    rho_2 = alpha = omega = 0.0
    p = v = None
    for i in range(1, max_iter + 1):
        if rho_1 == 0:
            return 2, i, resid, project(x)
        p = r.copy() if i == 1 else r + (-(rho_1 / rho_2) * (alpha / omega) * omega) * v + ((rho_1 / rho_2) * (alpha / omega)) * p
        phat = project(M(p))
        v = A @ phat
        alpha = rho_1 / float(rt @ v)
        s = r - alpha * v
        resid = np.linalg.norm(s) / normb
        if resid < tol:
            return 0, i, resid, project(x + alpha * phat)
        shat = project(M(s))
        t = A @ shat
        omega = float(t @ s) / float(t @ t)
        x = x + alpha * phat + omega * shat
        r = s - omega * t
        rho_2 = rho_1
        rho_1 = float(rt @ r)
        resid = np.linalg.norm(r) / normb
        if resid < tol:
            return 0, i, resid, project(x)
        if omega == 0:
            return 3, i, resid, project(x)
    return 1, max_iter, resid, project(x)


def fgcr(A, b, precond=None, restart=10, tol=1e-6, max_iter=1000, x0=None):
    """→ (status, iterations, resid, x): restarted flexible GCR (mgs_fgcr) with c_k ← Πc_k before v_k = A·c_k; at every window closure
    x ← Πx and the true residual Π(b − A·x) replaces the recurrence's; status 0 only on the true residual.  Directions and their images
    are orthogonalised together (tests/krylov_ref.py: the same x in exact arithmetic as the library's triangular solve)."""
    M = (lambda v: v.copy()) if precond is None else precond
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros(b.size) if x0 is None else np.array(x0, dtype=np.float64)
    normb = _normb(b)

    def true_residual(x):
        x = project(x)
        r = project(b - A @ x)
        return x, r, np.linalg.norm(r) / normb

    x, r, resid = true_residual(x)
    if resid <= tol:
        return 0, 0, resid, x
    it = 0
    while it < max_iter:
        Cs, Vs, rh = [], [], []
        for _ in range(restart):
            c = project(M(r)); v = A @ c
            hs = [float(vj @ v) / rj for vj, rj in zip(Vs, rh)]
            for hj, cj, vj in zip(hs, Cs, Vs):
                v = v - hj * vj; c = c - hj * cj
            rho = float(v @ v); it += 1
            if rho == 0.0:
                x, r, resid = true_residual(x)
                return (0 if resid < tol else 2), it, resid, x
            al = float(v @ r) / rho
            x = x + al * c; r = r - al * v
            Cs.append(c); Vs.append(v); rh.append(rho)
            resid = np.linalg.norm(r) / normb
            if resid < tol or it >= max_iter:
                break
        x, r, resid = true_residual(x)
        if resid < tol:
            return 0, it, resid, x
    return 1, it, resid, x
