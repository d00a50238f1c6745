"""NumPy restatement of the block-vector passes (multigridsolver_amd/csrc/blockvec.hip) and of mgs_eig_lobpcg (csrc/eig.hip).

Gram and combine are restated with the kernels' own association, so the GPU tests compare bit for bit: an entry of G is one reduction of
the products u_a[i]·v_b[i] through the folds of blas1_ref (lanes → wave → workgroup → last stage), the workgroup count and the 16-byte
decision are arguments, and a combine adds fl(C[a][j]·S_a[i]) in ascending a.  The solver loop is the library's method statement by
statement with numpy.linalg for the dense steps; its iterates agree with the library's to rounding, not to the bit.
"""
import numpy as np

import blas1_ref as b1

TB = b1.TB
GT = 8                  # a Gram tile is at most GT × GT
GRAM_BLOCKS = 2048      # most workgroups of a Gram pass
VECS_MAX = 24
EIG_MAX_BLOCK = 8


# ------------------------------------------------------------------------------------------------------------- the block passes
def gram_launch(n, aligned=True, blas1_vec=1):
    """mgs_vecs_gram → (16-byte form?, workgroups): one pair (or element) per lane, at most GRAM_BLOCKS workgroups"""
    vec = bool(blas1_vec) and aligned and n >= 2
    work = n // 2 if vec else n
    return vec, min(max(b1.cdiv(work, TB), 1), GRAM_BLOCKS)


def combine_launch(n, aligned=True, blas1_vec=1):
    vec = bool(blas1_vec) and aligned and n >= 2
    work = n // 2 if vec else n
    return vec, min(max(b1.cdiv(work, TB), 1), 1 << 20)


def gram(U, V, nb, vec, same=False, tile=GT, defect=None):
    """G[a, b] = Σ_i U[a][i]·V[b][i] as the kernels add it.  U, V: lists of equally long arrays; nb workgroups; vec: the 16-byte form.
    same: the same list on both sides — tiles on and above the diagonal are computed, the ones below are their mirror images."""
    p, q = len(U), len(V)
    G = np.zeros((p, q))
    for a in range(p):
        for b in range(q):
            if same and b // tile < a // tile:
                continue
            G[a, b] = b1.reduce_terms(np.asarray(U[a], dtype=np.float64) * np.asarray(V[b], dtype=np.float64), nb, vec, defect)
    if same:
        for a in range(p):
            for b in range(a):
                if b // tile < a // tile:
                    G[a, b] = G[b, a]
    return G


def combine(S, Cm, defect=None):
    """Y_j = fl(…fl(fl(C[0][j]·S_0) + fl(C[1][j]·S_1)) + …) → list of q arrays.  defect "descending": the sum taken from the last input down"""
    Cm = np.asarray(Cm, dtype=np.float64)
    k, q = Cm.shape
    order = list(range(k))[::-1] if defect == "descending" else list(range(k))
    out = []
    for j in range(q):
        y = Cm[order[0], j] * np.asarray(S[order[0]], dtype=np.float64)
        for a in order[1:]:
            y = y + Cm[a, j] * np.asarray(S[a], dtype=np.float64)
        out.append(y)
    return out


# ------------------------------------------------------------------------------------------------------------------ the fixtures
def _dense(rp, ci, v):
    n = len(rp) - 1
    A = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(rp))
    np.add.at(A, (rows, ci), v)
    return A


def fixture(name):
    """→ (dense A, labels or None): labels[i] = the field of row i of a declared null space (all 0: the constant kind), None: regular"""
    from multigridsolver_amd import synthetic
    if name == "poisson6":
        return _dense(*synthetic._poisson3d_dirichlet(6)), None
    if name == "poisson8d":
        A = _dense(*synthetic._poisson3d_dirichlet(8))
        return A + np.diag(np.random.default_rng(5).uniform(0, 1, 512)), None
    if name == "neumann6":
        return _dense(*synthetic.neumann3d(6)), np.zeros(216, dtype=np.int64)
    if name == "neumann45":
        A4, A5 = _dense(*synthetic.neumann3d(4)), _dense(*synthetic.neumann3d(5))
        A = np.zeros((64 + 125, 64 + 125)); A[:64, :64] = A4; A[64:, 64:] = A5
        return A, np.concatenate([np.zeros(64, dtype=np.int64), np.ones(125, dtype=np.int64)])
    raise KeyError(name)


# (fixture, m): the blocks the issue names; none of them cuts a multiple eigenvalue
CASES = [("poisson6", 1), ("poisson6", 4), ("poisson6", 7), ("poisson8d", 4), ("neumann6", 3), ("neumann6", 6), ("neumann45", 3)]


def start_block(n, m, seed=11):
    """the Gaussian start vectors both the restatement and the GPU tests use: m columns of length n"""
    return np.random.default_rng(seed).standard_normal((n, m))


def projector(labels):
    """Π = I − Σ_f z_f·z_fᵀ/n_f as a function on (n, q) blocks (None: no declaration)"""
    if labels is None:
        return None
    fields = [labels == f for f in range(int(labels.max()) + 1)]

    def proj(Vb):
        Vb = np.array(Vb, dtype=np.float64)
        for msk in fields:
            Vb[msk] -= Vb[msk].mean(axis=0)
        return Vb
    return proj


def dense_inverse(A, labels):
    """the one-level hierarchy's coarse solve: inv(A), regularised as mgs_hier_finalize does for a declared null space:
    A + Σ_f (max|a_ij|/n_f)·z_f·z_fᵀ"""
    R = np.array(A)
    if labels is not None:
        s = np.abs(A).max()
        for f in range(int(labels.max()) + 1):
            z = (labels == f).astype(np.float64)
            R += (s / z.sum()) * np.outer(z, z)
    return np.linalg.inv(R)


def complement_eigs(A, labels):
    """eigenvalues of A on the complement of the declared null space, ascending, with eigenvectors"""
    n = A.shape[0]
    if labels is None:
        return np.linalg.eigh(A)
    Z = np.stack([(labels == f) / np.sqrt((labels == f).sum()) for f in range(int(labels.max()) + 1)], axis=1)
    Q = np.linalg.qr(np.concatenate([Z, np.eye(n)], axis=1))[0][:, Z.shape[1]:n]
    w, Y = np.linalg.eigh(Q.T @ A @ Q)
    return w, Q @ Y


# ---------------------------------------------------------------------------------------------------------------- the solver loop
def _chol_rule(G, m):
    """Cholesky by the pivot rule of eig_dense.hpp: a pivot not greater than 8·m·ε·max diag refuses → L or None"""
    n = G.shape[0]
    dmax = np.max(np.diag(G))
    if not (dmax > 0) or not np.isfinite(G).all():
        return None
    bar = 8.0 * m * np.finfo(np.float64).eps * dmax
    L = np.zeros((n, n))
    for j in range(n):
        d = G[j, j] - L[j, :j] @ L[j, :j]
        if not (d > bar):
            return None
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (G[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _qr_factor(G, m):
    """eig_dense::qr_factor: the pivot rule on the Gram matrix of the normalised columns, D·G·D = L·Lᵀ; → C = D·L⁻ᵀ (B·C is orthonormal) or None"""
    g = np.diag(G)
    if not (np.isfinite(g).all() and (g > 0).all()):
        return None
    d = 1.0 / np.sqrt(g)
    L = _chol_rule(G * d[:, None] * d[None, :], m)
    return None if L is None else d[:, None] * np.linalg.inv(L).T


def lobpcg(A, X0, M=None, proj=None, tol=1e-6, max_iter=200):
    """mgs_eig_lobpcg on dense arrays.  A: (n, n) symmetric; X0: (n, m); M: (n, n) preconditioner or None; proj: projector(labels) or None.
    → dict(status, iterations, theta, resid, X, restarts)"""
    A = np.asarray(A, dtype=np.float64)
    n, m = X0.shape
    anorm = np.abs(A).sum(axis=1).max() or 1.0
    X = np.array(X0, dtype=np.float64)
    if proj:
        X = proj(X)
    theta, resid = np.zeros(m), np.zeros(m)
    L = _chol_rule(X.T @ X, m)
    if L is None:
        return dict(status=2, iterations=0, theta=theta, resid=resid, X=np.array(X0), restarts=0)
    X = X @ np.linalg.inv(L).T
    AX = A @ X
    G = X.T @ AX
    theta, Z = np.linalg.eigh(0.5 * (G + G.T))
    X, AX = X @ Z, AX @ Z
    P = AP = None
    fresh, it, restarts = True, 0, 0
    while True:
        R = AX - X * theta
        resid = np.linalg.norm(R, axis=0) / anorm
        if not np.isfinite(resid).all():
            return dict(status=3, iterations=it, theta=theta, resid=resid, X=X, restarts=restarts)
        act = [j for j in range(m) if not resid[j] < tol] if it < max_iter else []
        if not act:
            if not fresh:
                AX = A @ X; fresh = True
                if it < max_iter:
                    continue
                resid = np.linalg.norm(AX - X * theta, axis=0) / anorm
            return dict(status=0 if (resid < tol).all() else 1, iterations=it, theta=theta, resid=resid, X=X, restarts=restarts)
        W = R[:, act]
        if M is not None:
            W = M @ W
        if proj:
            W = proj(W)
        W = W - X @ (X.T @ W)
        Cw = _qr_factor(W.T @ W, m)
        if Cw is None:
            return dict(status=3, iterations=it, theta=theta, resid=resid, X=X, restarts=restarts)
        W = W @ Cw
        AW = A @ W
        useP = P is not None
        if useP:
            Pa, APa = P[:, act], AP[:, act]
            Cq = _qr_factor(Pa.T @ Pa, m)
            if Cq is None:
                useP = False; restarts += 1
            else:
                Pa, APa = Pa @ Cq, APa @ Cq
        while True:
            S = np.concatenate([X, W] + ([Pa] if useP else []), axis=1)
            AS = np.concatenate([AX, AW] + ([APa] if useP else []), axis=1)
            GA, GB = S.T @ AS, S.T @ S
            L = _chol_rule(GB, m)
            if L is None or not np.isfinite(GA).all():
                if not useP or L is not None:
                    return dict(status=3, iterations=it, theta=theta, resid=resid, X=X, restarts=restarts)
                useP = False; restarts += 1
                continue
            Li = np.linalg.inv(L)
            ev, Y = np.linalg.eigh(Li @ (0.5 * (GA + GA.T)) @ Li.T)
            Cz = (Li.T @ Y)[:, :m]
            Cp = np.array(Cz); Cp[:m] = 0.0
            X, P = S @ Cz, S @ Cp
            AX, AP = AS @ Cz, AS @ Cp
            theta = ev[:m]
            break
        fresh = False; it += 1


# iterations of lobpcg above from start_block(n, m), tol 1e-6, per (fixture, m, preconditioner): "none" = h NULL, "inverse" = dense_inverse.
# tests/test_eig_ref_cpu.py holds the restatement to them; tests/test_gpu_eig.py compares the library's counts with them.
ITERATIONS = {
    ("poisson6", 1, "none"): 43, ("poisson6", 1, "inverse"): 9, ("poisson6", 4, "none"): 41, ("poisson6", 4, "inverse"): 12,
    ("poisson6", 7, "none"): 46, ("poisson6", 7, "inverse"): 16, ("poisson8d", 4, "none"): 45, ("poisson8d", 4, "inverse"): 13,
    ("neumann6", 3, "none"): 54, ("neumann6", 3, "inverse"): 8, ("neumann6", 6, "none"): 40, ("neumann6", 6, "inverse"): 10,
    ("neumann45", 3, "none"): 82, ("neumann45", 3, "inverse"): 11,
}
