"""numpy restatement of what the library does for a matrix declared MGS_NULLSPACE_FIELDS (include/mgs.h: mgs_csr_set_nullspace_fields) — the
oracle side of tests/test_gpu_nullspace_fields.py, pinned by tests/test_nullspace_fields_ref_cpu.py.  No GPU.

  * project(v, labels): Π = I − Σ_f z_f·z_fᵀ/n_f — every labelled entry minus the mean of its field, rows labelled −1 untouched;
  * coarse_labels(labels, agg, nc): an aggregate takes the label of its first member; mixed aggregates and labelled rows outside every
    aggregate raise ValueError naming the lowest offending row (the refusals of mgs_hier_finalize);
  * regularised(Ac, labels): dense A_c + Σ_f (s/n_cf)·z_cf·z_cfᵀ with s = max|a_ij| of A_c;
  * Cycle: the V(1,1) cycle of tests/nullspace_ref.py that allows agg == −1 (such a row is smoothed and receives no coarse correction);
  * minres: the projected loop of mgs_minres on tests/minres_ref.py's statements — K·x = Πb, normb = ‖Πb‖ (1 if 0), x ← Πx before every
    true residual, every true residual Π(b − K·x), z̃ ← Π(M·v) after every preconditioner application;
  * pcg: tests/nullspace_ref.py's projected loop with this projection;
  * build_hierarchy: mgs_hier_coarsen's loop on tests/agmg_ref.py's restatement of the device aggregation (CPU tests; the GPU tests hand
    Cycle the device's own level operators and aggregates);
  * enclosed_stokes(N): the test system as scipy matrices (K, B = block_diag(L, S), labels) from multigridsolver_amd.synthetic's blocks."""
import numpy as np

import minres_ref as mr
import nullspace_ref as ns


def project(v, labels):
    v = np.array(v, dtype=np.float64, copy=True)
    labels = np.asarray(labels)
    for f in range(int(labels.max()) + 1 if labels.size else 0):
        sel = labels == f
        if sel.any():
            v[sel] = v[sel] - v[sel].sum() / sel.sum()
    return v


def coarse_labels(labels, agg, nc):
    labels = np.asarray(labels, dtype=np.int64); agg = np.asarray(agg, dtype=np.int64)
    first = np.full(nc, -1, dtype=np.int64)
    inside = np.nonzero(agg >= 0)[0]
    first[agg[inside][::-1]] = inside[::-1]            # lowest member of every aggregate
    clab = np.where(first >= 0, labels[np.maximum(first, 0)], -1)
    bad_out = (agg < 0) & (labels >= 0)
    bad_mix = np.zeros(labels.size, dtype=bool)
    bad_mix[inside] = labels[inside] != clab[agg[inside]]
    bad = bad_out | bad_mix
    if bad.any():
        row = int(np.nonzero(bad)[0][0])
        raise ValueError(f"row {row}: " + ("labelled and outside every aggregate" if bad_out[row] else "shares an aggregate with another label"))
    return clab


def regularised(Ac, labels):
    M = Ac.toarray()
    s = np.abs(Ac.data).max() if Ac.nnz else 0.0
    labels = np.asarray(labels)
    for f in range(int(labels.max()) + 1 if labels.size else 0):
        z = (labels == f).astype(np.float64)
        if z.any():
            M = M + (s / z.sum()) * np.outer(z, z)
    return M


def build_hierarchy(A, coarse_rows, ktg=10.0, npass=2, tou=8.0, max_levels=32):
    """nullspace_ref.build_hierarchy (which does not look at the aggregates' coverage)"""
    return ns.build_hierarchy(A, coarse_rows, ktg, npass, tou, max_levels)


class Cycle:
    """V(1,1) with damped Jacobi (ω) from a zero guess over level operators As (scipy CSR) and aggregate arrays aggs with −1 allowed:
    x = ωD⁻¹b, r = b − A·x, x[agg >= 0] += cycle(Pᵀr)[agg], x += ωD⁻¹(b − A·x).  labels: the fine labels (coarse ones follow the
    aggregation) for the regularised coarsest solve; None: the plain one (np.linalg.solve raises on an exactly singular matrix)."""

    def __init__(self, As, aggs, omega=0.6, labels=None):
        assert len(aggs) == len(As) - 1
        self.As, self.aggs = As, [np.asarray(a, dtype=np.int64) for a in aggs]
        self.wd = [omega / A.diagonal() for A in As[:-1]]
        self.labels = None
        if labels is None:
            self.Mc = As[-1].toarray()
        else:
            self.labels = [np.asarray(labels, dtype=np.int64)]
            for l, a in enumerate(self.aggs):
                self.labels.append(coarse_labels(self.labels[-1], a, As[l + 1].shape[0]))
            self.Mc = regularised(As[-1], self.labels[-1])

    def vcycle(self, b, l=0):
        if l == len(self.As) - 1:
            return np.linalg.solve(self.Mc, b)
        A, agg, wd = self.As[l], self.aggs[l], self.wd[l]
        ins = agg >= 0
        x = wd * b
        r = b - A @ x
        ec = self.vcycle(np.bincount(agg[ins], weights=r[ins], minlength=self.As[l + 1].shape[0]), l + 1)
        x = x.copy(); x[ins] = x[ins] + ec[agg[ins]]
        return x + wd * (b - A @ x)


def minres(A, b, labels, precond=None, tol=1e-6, max_iter=10000, x0=None, projected=True):
    """→ (status, iterations, resid, x): tests/minres_ref.py's loop with the projections of mgs_minres for MGS_NULLSPACE_FIELDS.
    projected=False: the same loop with Π = I (what runs without the declaration)."""
    Pi = (lambda v: project(v, labels)) if projected else (lambda v: np.array(v, dtype=np.float64, copy=True))
    spmv = A if callable(A) else (lambda v: A @ v)
    dot, norm = mr._dot, mr._norm
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.zeros(b.shape[0]) if x0 is None else np.array(x0, dtype=np.float64)
    M = (lambda u: Pi(u)) if precond is None else (lambda u: Pi(precond(u)))
    state = {"x": x}

    def true_residual():
        state["x"] = Pi(state["x"])
        r = Pi(b - spmv(state["x"]))
        return r, norm(r) / normb
    normb = norm(Pi(b))
    if normb == 0.0:
        normb = 1.0
    v, resid = true_residual()
    if resid <= tol:
        return 0, 0, resid, state["x"]
    zt = M(v)
    g2 = dot(zt, v)
    if not g2 > 0:
        return 2, 0, resid, state["x"]
    gam = np.sqrt(g2); gam_prev = 1.0; eta = gam
    kappa = resid * normb / gam
    s0 = s1 = 0.0; c0 = c1 = 1.0
    w_prev = np.zeros_like(x); w = np.zeros_like(x); v_prev = np.zeros_like(x)
    for j in range(1, max_iter + 1):
        q = spmv(zt)
        delta = dot(q, zt) / (gam * gam)
        v_new = (1 / gam) * q + (-(delta / gam)) * v + (-(gam / gam_prev)) * v_prev
        zt_new = M(v_new)
        gn2 = dot(zt_new, v_new)
        if not gn2 >= 0:
            return 2, j, true_residual()[1], state["x"]
        gamn = np.sqrt(gn2)
        a0 = c1 * delta - c0 * s1 * gam
        a1 = np.sqrt(a0 * a0 + gn2)
        a2 = s1 * delta + c0 * c1 * gam
        a3 = s0 * gam
        if a1 == 0:
            return 3, j, true_residual()[1], state["x"]
        cn = a0 / a1; sn = gamn / a1
        w_new, state["x"] = mr.update_ref(1 / gam, a3, a2, a1, cn * eta, zt, w_prev, w, state["x"])
        eta = -sn * eta
        v_prev, v = v, v_new
        zt = zt_new
        w_prev, w = w, w_new
        s0, s1 = s1, sn
        c0, c1 = c1, cn
        gam_prev, gam = gam, gamn
        est = kappa * abs(eta) / normb
        fresh = False
        if est < tol or gamn == 0:
            resid = true_residual()[1]; fresh = True
            if resid < tol:
                return 0, j, resid, state["x"]
            if gamn == 0:
                return 3, j, resid, state["x"]
            kappa = resid * normb / abs(eta)
        if j == max_iter and not fresh:
            resid = true_residual()[1]
    return 1, max(max_iter, 0), resid, state["x"]


def pcg(A, b, labels, precond=None, tol=1e-6, max_iter=10000, x0=None):
    """→ (status, iterations, resid, x): nullspace_ref.pcg with the field-wise projection in the place of the global mean"""
    Pi = lambda v: project(v, labels)      # noqa: E731
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros(b.size) if x0 is None else np.array(x0, dtype=np.float64)
    normb = np.linalg.norm(Pi(b))
    if normb == 0.0:
        normb = 1.0
    r = Pi(b - A @ x)
    resid = np.linalg.norm(r) / normb
    if resid <= tol:
        return 0, 0, resid, Pi(x)
    p = None
    alpha = rho_prev = 0.0
    restart = True
    for i in range(1, max_iter + 1):
        z = Pi(r.copy() if precond is None else precond(r))
        rho = float(r @ z)
        if not rho > 0:
            return 2, i, resid, Pi(x)
        if restart:
            p = z.copy(); restart = False
        else:
            p = z + (rho / rho_prev) * p
        q = A @ p
        pq = float(p @ q)
        if not pq > 0:
            return 3, i, resid, Pi(x)
        alpha = rho / pq
        x = x + alpha * p
        r = r - alpha * q
        resid = np.linalg.norm(r) / normb
        rho_prev = rho
        if resid < tol:
            x = Pi(x)
            r = Pi(b - A @ x)
            resid = np.linalg.norm(r) / normb
            if resid < tol:
                return 0, i, resid, x
            restart = True
    return 1, max_iter, resid, Pi(x)


def _sp(t, rows, cols):
    import scipy.sparse as sps
    rp, ci, v = t
    return sps.csr_matrix((v, ci, rp), shape=(rows, cols))


def enclosed_stokes(N):
    """→ dict: scipy CSR L, D, K = [[L, Dᵀ], [D, 0]], S = D·diag(L)⁻¹·Dᵀ, B = block_diag(L, S), labels, m, n (synthetic.enclosed_stokes)"""
    import scipy.sparse as sps
    from multigridsolver_amd.synthetic import enclosed_stokes as gen
    g = gen(N)
    m = g["m"]
    L = _sp(g["L"], 3 * m, 3 * m); D = _sp(g["D"], m, 3 * m)
    K = sps.bmat([[L, D.T], [D, None]], format="csr")
    S = (D @ sps.diags(1.0 / L.diagonal()) @ D.T).tocsr()
    B = sps.block_diag([L, S], format="csr")
    for X in (L, D, K, S, B):
        X.sum_duplicates(); X.sort_indices()
    return {"L": L, "D": D, "K": K, "S": S, "B": B, "labels": g["labels"], "m": m, "n": 4 * m}
