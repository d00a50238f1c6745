"""numpy restatement of mgs_minres (include/mgs.h; multigridsolver_amd/csrc/minres.hip), statement by statement — the oracle side of the
MINRES tests.  `A` is an oracle_py.Csr (or a callable v -> A·v), `precond` a callable v -> M·v with M symmetric positive definite
(orc.Hier(...).vcycle, an exact block solve) or None for the identity.  The method is preconditioned MINRES in the form of Elman,
Silvester and Wathen, Alg. 4.1 (Paige-Saunders), with v and z̃ = M·v stored unnormalised; tests/test_minres_ref_cpu.py pins it against
scipy.sparse.linalg.minres.  The additions are the stopping rule on the true residual (κ recalibrated, no restart) and the exits.

dtype = np.float64 (default) or any other numpy float type (np.longdouble: the extended-precision yardstick of tests/krylov_ref.py); the
same statements run in that type.  Inner products are Σ aᵢ·bᵢ with every product rounded on its own (np.sum, pairwise), in every type: the
device's sums hold no fused multiply-add either.

Also here: update_ref, the per-entry arithmetic of k_minres_update; banded_sym, a symmetric indefinite banded operator in slice and CSR
form after krylov_ref.banded; saddle, the saddle-point systems [[L, Dᵀ], [D, −C]] the CPU and the GPU tests share."""
import numpy as np

import krylov_ref as kr


def _dot(a, b):
    s = (a * b).sum()
    return float(s) if a.dtype == np.float64 else s


def _norm(a):
    return np.sqrt(_dot(a, a))


def update_ref(inv_g, a3, a2, a1, step, z, w_prev, w, x):
    """k_minres_update per entry → (w_new, x_new): every product, sum and quotient rounded on its own, the quotient a true division"""
    t = inv_g * z - a3 * w_prev
    t = t - a2 * w
    wn = t / a1
    return wn, x + step * wn


def minres_ref(A, b, precond=None, tol=1e-6, max_iter=10000, x0=None, dtype=np.float64, checks=None):
    """→ (status, iterations, resid, x); status 0 converged on the true residual / 1 max_iter / 2 z̃·v negative or not a number /
    3 Krylov space exhausted above the tolerance.  resid is the true relative residual whatever the status.
    checks: a list that receives (iteration, est, true residual) of every true-residual check the stopping rule made"""
    spmv = A if callable(A) else A.spmv
    T = np.dtype(dtype).type
    b = np.ascontiguousarray(b, dtype=dtype)
    x = np.zeros(b.shape[0], dtype=dtype) if x0 is None else np.array(x0, dtype=dtype)
    M = (lambda u: np.array(u, copy=True)) if precond is None else precond

    def true_resid():
        return _norm(b - spmv(x)) / normb
    normb = _norm(b)
    if normb == 0.0:
        normb = T(1)
    v = b - spmv(x)
    resid = _norm(v) / normb
    if resid <= tol:
        return 0, 0, resid, x
    zt = M(v)
    g2 = _dot(zt, v)
    if not g2 > 0:
        return 2, 0, resid, x
    gam = np.sqrt(g2); gam_prev = T(1); eta = gam
    kappa = resid * normb / gam
    s0 = s1 = T(0); c0 = c1 = T(1)
    w_prev = np.zeros_like(x); w = np.zeros_like(x); v_prev = np.zeros_like(x)
    for j in range(1, max_iter + 1):
        q = spmv(zt)
        delta = _dot(q, zt) / (gam * gam)
        v_new = (1 / gam) * q + (-(delta / gam)) * v + (-(gam / gam_prev)) * v_prev        # k_axpbypcz: a·x + b·y + c·z, left to right
        zt_new = M(v_new)
        gn2 = _dot(zt_new, v_new)
        if not gn2 >= 0:
            return 2, j, true_resid(), x
        gamn = np.sqrt(gn2)
        a0 = c1 * delta - c0 * s1 * gam
        a1 = np.sqrt(a0 * a0 + gn2)
        a2 = s1 * delta + c0 * c1 * gam
        a3 = s0 * gam
        if a1 == 0:
            return 3, j, true_resid(), x
        cn = a0 / a1; sn = gamn / a1
        w_new, x = update_ref(1 / gam, a3, a2, a1, cn * eta, zt, w_prev, w, x)
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
            resid = true_resid(); fresh = True
            if checks is not None:
                checks.append((j, float(est), float(resid)))
            if resid < tol:
                return 0, j, resid, x
            if gamn == 0:
                return 3, j, resid, x
            kappa = resid * normb / abs(eta)
        if j == max_iter and not fresh:
            resid = true_resid()
    return 1, max(max_iter, 0), resid, x


# --------------------------------------------------------------------------------------- a symmetric indefinite banded operator
def banded_sym(n, seed=0):
    """krylov_ref.Banded with the offsets (−B, −1, 0, +1, +B): the off-diagonals in −[0.2, 1], the upper two mirroring the lower two, and a
    diagonal of magnitude [4.5, 5.5] whose sign alternates in runs of seeded random length (both signs from n = 2 on).  Every row is strictly
    dominant (off-diagonal row sum <= 4 < 4.5), so by Gershgorin the spectrum lies in [−9.5, −0.5] ∪ [0.5, 9.5]: symmetric, indefinite,
    condition number below 19 (tests/test_minres_ref_cpu.py checks it with eigvalsh)."""
    rng = np.random.default_rng(seed)
    B = kr.BAND
    lB, l1 = (-rng.uniform(0.2, 1.0, n) for _ in range(2))
    d = rng.uniform(4.5, 5.5, n)
    sign = np.where(np.cumsum(rng.integers(0, 2, n)) % 2 == 0, 1.0, -1.0)
    if n >= 2:
        sign[0], sign[1] = 1.0, -1.0
    d = d * sign
    lB[:min(B, n)] = 0.0; l1[:1] = 0.0
    u1 = np.zeros(n); uB = np.zeros(n)
    u1[:-1] = l1[1:]
    if B < n:
        uB[:-B] = lB[B:]
    return kr.Banded(n, [lB, l1, d, u1, uB])


# ----------------------------------------------------------------------------------------------------- the saddle-point systems
def saddle(N):
    """→ dict of scipy CSR matrices: L the 3-D 7-point Laplacian on N³ points (Dirichlet; diagonal 6), D every second row of I − shift
    (shift: ones on the first superdiagonal), C = 1e-2·I, K = [[L, Dᵀ], [D, −C]] (symmetric indefinite), S = C + D·diag(L)⁻¹·Dᵀ (the
    Schur complement with L replaced by its diagonal: symmetric positive definite), and n, m = rows of L and of D"""
    import scipy.sparse as sps
    e = sps.eye(N, format="csr")
    t = sps.diags([-np.ones(N - 1), 2.0 * np.ones(N), -np.ones(N - 1)], [-1, 0, 1], format="csr")
    L = (sps.kron(sps.kron(t, e), e) + sps.kron(sps.kron(e, t), e) + sps.kron(sps.kron(e, e), t)).tocsr()
    n = N ** 3
    D = (sps.eye(n, format="csr") - sps.eye(n, k=1, format="csr")).tocsr()[::2, :].tocsr()
    m = D.shape[0]
    Cm = (1e-2 * sps.eye(m, format="csr")).tocsr()
    K = sps.bmat([[L, D.T], [D, -Cm]], format="csr")
    S = (Cm + D @ sps.diags(1.0 / L.diagonal()) @ D.T).tocsr()
    for X in (L, D, Cm, K, S):
        X.sum_duplicates(); X.sort_indices()
    return {"L": L, "D": D, "C": Cm, "K": K, "S": S, "n": n, "m": m}


def saddle_rhs(rows, seed=0):
    """entries uniform in [0, 1), as the reference draws its right-hand side (src/common/bicg.cpp:159-162)"""
    return np.random.default_rng(seed).uniform(0.0, 1.0, rows)


def exact_block_precond(sd):
    """v -> block_diag(L, S)⁻¹·v through two sparse LU factorisations"""
    from scipy.sparse.linalg import splu
    luL, luS = splu(sd["L"].tocsc()), splu(sd["S"].tocsc())
    n = sd["n"]
    return lambda v: np.concatenate([luL.solve(v[:n]), luS.solve(v[n:])])
