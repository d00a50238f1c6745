"""NumPy restatement of mgs_eig_lobpcg_gen (multigridsolver_amd/csrc/eig.hip) and of its fused residual pass mgs_eig_residual (csrc/blas1.hip).

The solver loop is the library's method statement by statement, on dense arrays, with numpy.linalg for the dense steps: its iterates agree with
the library's to rounding, not to the bit.  The residual pass is restated with the kernel's own expression and association: t = fl(θ·bx_i),
r_i = fl(ax_i − t), and Σ fl(r_i·r_i) through the folds of blas1_ref under k_dot's launch decisions, so the GPU test compares bit for bit.
"""
import numpy as np

import blas1_ref as b1
import eig_ref as E
from eig_ref import _chol_rule, _qr_factor, fixture, start_block  # noqa: F401  (the fixtures and the start block are eig_ref's)

# (fixture, m): the blocks the generalised solver is held to; none of them cuts a multiple eigenvalue of the pencil (A, B)
CASES = [(name, m) for name in ("poisson6", "poisson8d") for m in (1, 4, 7)]


# ------------------------------------------------------------------------------------------------------------------ the fixtures
def mass_parts(name):
    """→ (ρ, L): B = diag(ρ) + L/24 with L the Dirichlet Poisson matrix of the fixture's grid, ρ = default_rng(7).uniform(0.75, 1.25, n).
    B is strictly diagonally dominant (the diagonal is ρ_i + 0.25 ≥ 1, the off-diagonal row sum at most 6/24), hence SPD, and no polynomial in A."""
    from multigridsolver_amd import synthetic
    N = {"poisson6": 6, "poisson8d": 8}[name]
    L = E._dense(*synthetic._poisson3d_dirichlet(N))
    rho = np.random.default_rng(7).uniform(0.75, 1.25, N ** 3)
    return rho, L


def mass(name):
    rho, L = mass_parts(name)
    return np.diag(rho) + L / 24.0


# --------------------------------------------------------------------------------------------------------------- the residual pass
def residual(ax, bx, theta, defect=None, **launch):
    """mgs_eig_residual → (r, ‖r‖² as folded).  r_i = fl(ax_i − fl(θ·bx_i)); the norm is blas1_ref.dot(r, r) under dot_launch.
    launch: aligned, blas1_vec, blas1_pairs, n_cu.  defect "fused": ax_i − θ·bx_i rounded once (what a contracted multiply-add gives),
    for the test that shows the fixture can tell."""
    ax, bx = np.asarray(ax, dtype=np.float64), np.asarray(bx, dtype=np.float64)
    th = np.float64(theta)
    if defect == "fused":
        import math
        r = np.array([math.fma(-float(th), float(b), float(a)) for a, b in zip(ax, bx)])
    else:
        t = th * bx
        r = ax - t
    return r, b1.dot(r, r, **launch)


def residual_fixture(n, seed=3):
    """(ax, bx, θ) on which the three ways of rounding ax_i − θ·bx_i differ: θ and bx carry full mantissas, so θ·bx_i is inexact, and ax_i lies
    close to θ·bx_i, so the rounding error of the product survives the cancellation"""
    rng = np.random.default_rng(seed)
    bx = rng.uniform(0.5, 2.0, n)
    theta = 0.7310585786300049
    ax = theta * bx * (1.0 + rng.uniform(-1, 1, n) * 2.0 ** -30)
    ax[::7] = rng.standard_normal(len(ax[::7]))      # and entries without cancellation, of either sign
    return ax, bx, theta


# ---------------------------------------------------------------------------------------------------------------- the solver loop
def _sym(G):
    return 0.5 * (G + G.T)


def lobpcg_gen(A, B, X0, M=None, tol=1e-6, max_iter=200):
    """mgs_eig_lobpcg_gen on dense arrays.  A, B: (n, n) symmetric, B positive definite; X0: (n, m); M: (n, n) preconditioner or None.
    → dict(status, iterations, theta, resid, X, restarts, spmv, spmv_b)"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    n, m = X0.shape
    anorm = np.abs(A).sum(axis=1).max() or 1.0
    bnorm = np.abs(B).sum(axis=1).max() or 1.0
    X = np.array(X0, dtype=np.float64)
    theta, resid = np.zeros(m), np.zeros(m)
    cnt = dict(spmv=0, spmv_b=0)

    def mulA(V):
        cnt["spmv"] += V.shape[1]
        return A @ V

    def mulB(V):
        cnt["spmv"] += V.shape[1]; cnt["spmv_b"] += V.shape[1]
        return B @ V

    def out(status, it, X_):
        return dict(status=status, iterations=it, theta=theta, resid=resid, X=X_, restarts=restarts, **cnt)

    def resid_of(AX_, BX_):
        return np.linalg.norm(AX_ - BX_ * theta, axis=0) / (anorm + np.abs(theta) * bnorm)
    restarts = 0
    BX = mulB(X)
    L = _chol_rule(_sym(X.T @ BX), m)
    if L is None:
        return out(2, 0, np.array(X0))
    Ci = np.linalg.inv(L).T
    X, BX = X @ Ci, BX @ Ci
    AX = mulA(X)
    theta, Z = np.linalg.eigh(_sym(X.T @ AX))
    X, AX, BX = X @ Z, AX @ Z, BX @ Z
    P = AP = BP = None
    fresh, it = True, 0
    while True:
        R = AX - BX * theta
        resid = np.linalg.norm(R, axis=0) / (anorm + np.abs(theta) * bnorm)
        if not np.isfinite(resid).all():
            return out(3, it, X)
        act = [j for j in range(m) if not resid[j] < tol] if it < max_iter else []
        if not act:
            if not fresh:
                AX, BX = mulA(X), mulB(X); fresh = True
                if it < max_iter:
                    continue
                resid = resid_of(AX, BX)
            return out(0 if (resid < tol).all() else 1, it, X)
        W = R[:, act]
        if M is not None:
            W = M @ W
        W = W - X @ (BX.T @ W)
        BW = mulB(W)
        Cw = _qr_factor(_sym(W.T @ BW), m)
        if Cw is None:
            return out(3, it, X)
        W, BW = W @ Cw, BW @ Cw
        AW = mulA(W)
        useP = P is not None
        if useP:
            Pa, APa, BPa = P[:, act], AP[:, act], BP[:, act]
            Cq = _qr_factor(_sym(Pa.T @ BPa), m)
            if Cq is None:
                useP = False; restarts += 1
            else:
                Pa, APa, BPa = Pa @ Cq, APa @ Cq, BPa @ Cq
        while True:
            S = np.concatenate([X, W] + ([Pa] if useP else []), axis=1)
            AS = np.concatenate([AX, AW] + ([APa] if useP else []), axis=1)
            BS = np.concatenate([BX, BW] + ([BPa] if useP else []), axis=1)
            GA, GB = S.T @ AS, _sym(S.T @ BS)
            L = _chol_rule(GB, m)
            if L is None or not np.isfinite(GA).all():
                if not useP or L is not None:
                    return out(3, it, X)
                useP = False; restarts += 1
                continue
            Li = np.linalg.inv(L)
            ev, Y = np.linalg.eigh(Li @ _sym(GA) @ Li.T)
            Cz = (Li.T @ Y)[:, :m]
            Cp = np.array(Cz); Cp[:m] = 0.0
            X, P = S @ Cz, S @ Cp
            AX, AP = AS @ Cz, AS @ Cp
            BX, BP = BS @ Cz, BS @ Cp
            theta = ev[:m]
            break
        fresh = False; it += 1


# iterations of lobpcg_gen above from start_block(n, m), tol 1e-6, B = mass(fixture), per (fixture, m, preconditioner): "none" = h NULL,
# "inverse" = eig_ref.dense_inverse(A).  tests/test_eig_gen_ref_cpu.py holds the restatement to them; tests/test_gpu_eig_gen.py compares the
# library's counts with them.
ITERATIONS = {
    ("poisson6", 1, "none"): 50, ("poisson6", 1, "inverse"): 10, ("poisson6", 4, "none"): 37, ("poisson6", 4, "inverse"): 12,
    ("poisson6", 7, "none"): 40, ("poisson6", 7, "inverse"): 16, ("poisson8d", 1, "none"): 47, ("poisson8d", 1, "inverse"): 12,
    ("poisson8d", 4, "none"): 44, ("poisson8d", 4, "inverse"): 14, ("poisson8d", 7, "none"): 53, ("poisson8d", 7, "inverse"): 18,
}
