"""numpy restatement of mgs_guess (include/mgs.h; kernels in multigridsolver_amd/csrc/guess.hip) — the oracle side of the guess tests.

Elementwise results are formed exactly as the kernels form them: Σ_k c_k·v_k is ((c_0·v_0 + c_1·v_1) + c_2·v_2) + …, the sum starting
from the first product, one rounding per product and per sum; x' = x − Σ, x̃ = s·x''.  In float64 and FED THE DEVICE'S COEFFICIENT BITS
(`alpha=` of apply, `coef=` of update) x0, x', w' and the stored pairs therefore equal the device's bit for bit.  Left to itself the
restatement computes its own inner products (BLAS in float64, pairwise sums in any other dtype: np.longdouble is the extended-precision
yardstick) — those agree with the device's to rounding only, since the order of the sums differs.

A: a scipy.sparse matrix, an oracle_py.Csr or a callable v -> A·v."""
import math

import numpy as np

ENERGY, RESIDUAL = "energy", "residual"
ETA2 = 0.5          # DGKS with η = 1/√2, on the squares: accept when ν2² >= ν1²/2
FLOOR2 = 2.0 ** -94  # … and ν2 > 32·2⁻⁵²·ν0: what is left of a candidate inside the span is rounding noise, which the second pass barely shortens


def _dot(a, b):
    return float(a @ b) if a.dtype == np.float64 else (a * b).sum()


def combine(c, V, like):
    """Σ_k c_k·V_k in the kernels' order; an empty sum is 0"""
    if len(V) == 0:
        return np.zeros_like(like)
    t = c[0] * V[0]
    for k in range(1, len(V)):
        t = t + c[k] * V[k]
    return t


class GuessRef:
    def __init__(self, A, kind=ENERGY, capacity=8, nullspace=False, dtype=np.float64):
        assert kind in (ENERGY, RESIDUAL) and 1 <= capacity <= 16
        self.kind, self.capacity, self.nullspace, self.dtype = kind, capacity, nullspace, dtype
        self.set_operator(A)
        self.X, self.Y = [], []
        self.restarts = self.refused = 0
        self.last = {}

    def set_operator(self, A):
        if callable(A):
            self.spmv = A
        elif hasattr(A, "spmv"):
            self.spmv = A.spmv
        elif self.dtype == np.float64:
            self.spmv = lambda v: A @ v
        else:                                   # scipy has no extended-precision product: row sums in the working type
            coo = A.tocoo(); r, c, v = coo.row, coo.col, coo.data.astype(self.dtype)
            def mv(x):
                out = np.zeros(A.shape[0], dtype=self.dtype); np.add.at(out, r, v * x[c]); return out
            self.spmv = mv

    @property
    def size(self):
        return len(self.X)

    def Q(self):
        return self.X if self.kind == ENERGY else self.Y

    # ---- apply
    def apply(self, b, alpha=None):
        """→ (x0, α, ‖b − Σ α_k·ỹ_k‖/‖b‖); alpha: the device's α bits instead of the restatement's own"""
        b = np.asarray(b, dtype=self.dtype)
        if alpha is None:
            alpha = np.array([_dot(q, b) for q in self.Q()], dtype=self.dtype)
        x0 = combine(alpha, self.X, b)
        if self.size == 0:
            return x0, alpha, 1.0
        r0 = b - combine(alpha, self.Y, b)
        nb = math.sqrt(float(_dot(b, b))); nr = math.sqrt(float(_dot(r0, r0)))
        return x0, alpha, (nr / nb if nb > 0 else (math.inf if nr > 0 else 0.0))

    # ---- update
    def update(self, x, coef=None, w=None):
        """offer x → added.  coef: dict of the device's bits (c1, c2, s, flag) to follow instead of the restatement's own inner products
        and decision; w: the device's A·x where the operator's own product is not reproducible on the host.  self.last keeps every
        intermediate (c1, c2, nu0, nu1, nu2, s, flag, xp = x', wp = w', K, restart)."""
        x = np.asarray(x, dtype=self.dtype)
        if self.nullspace:
            x = x - x.sum() / self.dtype(x.size)
        restart = self.size == self.capacity
        X, Y = ([], []) if restart else (self.X, self.Y)
        Qs = X if self.kind == ENERGY else Y
        K = len(X)
        w = self.spmv(x) if w is None else np.asarray(w, dtype=self.dtype)
        c1 = np.array([_dot(q, w) for q in Qs], dtype=self.dtype)
        nu0 = _dot(x if self.kind == ENERGY else w, w)
        L = dict(K=K, restart=restart, nu0=nu0)
        if K:
            if coef is not None:
                c1 = np.asarray(coef["c1"], dtype=self.dtype)
            xp = x - combine(c1, X, x); wp = w - combine(c1, Y, w)
            c2 = np.array([_dot(q, wp) for q in Qs], dtype=self.dtype)
            nu1 = _dot(xp if self.kind == ENERGY else wp, wp)
            if coef is not None:
                c2 = np.asarray(coef["c2"], dtype=self.dtype)
            xpp = xp - combine(c2, X, xp); wpp = wp - combine(c2, Y, wp)
            nu2 = _dot(xpp if self.kind == ENERGY else wpp, wpp)
            L.update(c1=c1, c2=c2, xp=xp, wp=wp)
        else:
            xpp, wpp, nu1, nu2 = x, w, nu0, nu0
            L.update(c1=c1[:0], c2=c1[:0], xp=x, wp=w)
        ok = bool(np.isfinite(nu2) and nu2 > 0 and nu2 >= ETA2 * nu1 and nu0 > 0 and nu2 > FLOOR2 * nu0)
        s = self.dtype(1.0) / np.sqrt(self.dtype(nu2)) if ok else self.dtype(0.0)
        if coef is not None:
            ok, s = bool(coef["flag"]), self.dtype(coef["s"])
        L.update(nu1=nu1, nu2=nu2, s=s, flag=ok)
        self.last = L
        if not ok:
            self.refused += 1
            return False
        if restart:
            self.X, self.Y = [], []
            self.restarts += 1
        self.X.append(s * xpp); self.Y.append(s * wpp)
        return True

    def rebase(self, A=None):
        """A's values changed: reset, then update(x̃_k) from the oldest to the newest"""
        if A is not None:
            self.set_operator(A)
        old = self.X
        self.X, self.Y = [], []
        for xk in old:
            self.update(xk)

    def reset(self):
        self.X, self.Y = [], []

    def gram(self):
        Qs = self.Q()
        return np.array([[_dot(Qs[j], self.Y[k]) for k in range(self.size)] for j in range(self.size)], dtype=self.dtype).reshape(self.size, self.size)


# ---------------------------------------------------------------------------------------------------------------- the probe's sequence
def probe_rhs(N, step, dim=3):
    """right-hand side number `step` of the sequence the feature was probed with (multigridsolver_amd.synthetic.moving_blob_rhs, dt = 0.05)"""
    from multigridsolver_amd.synthetic import moving_blob_rhs
    return moving_blob_rhs(N, step, dim)


def run_sequence(solve, rhs, mode, make_guess=None):
    """iteration counts of solving rhs[0], rhs[1], … in turn.  solve(b, x0) -> (iterations, x); mode "zero" | "previous" | "projected"
    (make_guess() -> an object with apply(b) -> (x0, …) and update(x))"""
    counts, xprev, g = [], None, (make_guess() if mode == "projected" else None)
    for b in rhs:
        if mode == "zero" or xprev is None:
            x0 = np.zeros_like(b)
        elif mode == "previous":
            x0 = xprev
        else:
            x0 = np.asarray(g.apply(b)[0], dtype=np.float64)
        it, x = solve(b, x0)
        counts.append(it)
        xprev = x
        if g is not None:
            g.update(x)
    return counts
