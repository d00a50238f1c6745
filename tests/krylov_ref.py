"""Extended-precision yardsticks of the Krylov solvers' scalars: restatements of mgs_bicgstab, mgs_pcg and mgs_fgcr
(multigridsolver_amd/csrc/krylov.hip) for a FIXED number of steps, in any numpy float type (np.longdouble: the reference;
np.float64: the distance a correct FP64 implementation may have from it), plus a banded test operator whose product is a few
shifted numpy slices, so that applying it in long double needs no sparse library.

Every restatement takes (apply_A, b, x0, steps, ...) and returns (x, resid) with resid the solver's reported relative residual:
the recurrence residual for BiCGSTAB and PCG, the true residual recomputed at the last window closure for FGCR (what mgs_fgcr
reports).  Inner products are summed pairwise (np.sum), so the long-double reference carries an error of a few 2^-64.

tests/test_krylov_ref_cpu.py pins these restatements (against the oracle's bicgstab and against themselves across types)."""
import numpy as np

from pcg_ref import pcg_ref

BAND = 300


def dot(a, b):
    return (a * b).sum()


def rel(a, b):
    """‖a − b‖/‖b‖ evaluated in the wider of the two types"""
    a = np.asarray(a); b = np.asarray(b)
    t = np.result_type(a.dtype, b.dtype)
    d = a.astype(t) - b.astype(t)
    nb = np.sqrt(dot(b.astype(t), b.astype(t)))
    return float(np.sqrt(dot(d, d)) / (nb if nb > 0 else 1))


# ---------------------------------------------------------------------------------------------------------------- the solvers
def bicgstab_fixed(apply_A, b, x0, steps, dtype=np.longdouble, snapshots=None):
    """BiCGSTABiml as mgs_bicgstab runs it without a preconditioner (p̂ = p, ŝ = s), tol = 0: exactly `steps` iterations unless a
    breakdown (ρ = 0 or ω = 0) ends it.  snapshots: a dict whose keys are step counts < steps; filled with (x, resid) after those steps,
    i.e. with what the shorter runs return."""
    b = np.asarray(b, dtype=dtype); x = np.array(x0, dtype=dtype)
    normb = np.sqrt(dot(b, b))
    if normb == 0:
        normb = dtype(1)
    r = b - apply_A(x)
    rt = r.copy()
    rho_1 = dot(rt, r)
    resid = np.sqrt(dot(r, r)) / normb
    rho_2 = alpha = omega = dtype(0)
    p = v = None
    for i in range(1, steps + 1):
        if rho_1 == 0:
            break
        if i == 1:
            p = r.copy()
        else:
            beta = (rho_1 / rho_2) * (alpha / omega)
            p = r + (-beta * omega) * v + beta * p
        v = apply_A(p)
        alpha = rho_1 / dot(rt, v)
        s = r + (-alpha) * v
        t = apply_A(s)
        omega = dot(t, s) / dot(t, t)
        x = alpha * p + omega * s + x
        r = s + (-omega) * t
        rho_2 = rho_1
        rho_1 = dot(rt, r)
        resid = np.sqrt(dot(r, r)) / normb
        if snapshots is not None and i in snapshots:
            snapshots[i] = (x.copy(), resid)
        if omega == 0:
            break
    return x, resid


def pcg_fixed(apply_A, b, x0, steps, flexible=False, dtype=np.longdouble):
    """mgs_pcg without a preconditioner for `steps` iterations: tests/pcg_ref.py run in `dtype` with tol = 0"""
    st, it, resid, x = pcg_ref(apply_A, b, None, tol=0.0, max_iter=steps, flexible=flexible, x0=x0, dtype=dtype)
    assert st == 1 and it == steps, (st, it)
    return x, resid


def fgcr_fixed(apply_A, b, x0, steps, restart, dtype=np.longdouble):
    """restarted flexible GCR(restart) without a preconditioner: classical Gram-Schmidt of v_k = A·c_k against the window's v_j (every
    coefficient from the not yet updated v_k), r ← r − α v; when a window closes (full, or out of steps) the true residual b − A·x
    replaces the recurrence's.  mgs_fgcr leaves the c_k un-orthogonalised and solves the triangular coefficient system instead — the
    same x in exact arithmetic."""
    b = np.asarray(b, dtype=dtype); x = np.array(x0, dtype=dtype)
    normb = np.sqrt(dot(b, b))
    if normb == 0:
        normb = dtype(1)
    r = b - apply_A(x)
    it = 0
    while it < steps:
        Cs, Vs, rh = [], [], []
        for _ in range(restart):
            c = r.copy(); v = apply_A(c)
            hs = [dot(vj, v) / rj for vj, rj in zip(Vs, rh)]
            for hj, cj, vj in zip(hs, Cs, Vs):
                v = v - hj * vj; c = c - hj * cj
            rho = dot(v, v); al = dot(v, r) / rho
            x = x + al * c; r = r - al * v
            Cs.append(c); Vs.append(v); rh.append(rho); it += 1
            if it >= steps:
                break
        r = b - apply_A(x)
    return x, np.sqrt(dot(r, r)) / normb


# ------------------------------------------------------------------------------------------------------- the banded operator
class Banded:
    """n × n operator with the offsets (−B, −1, 0, +1, +B): diag[k][i] is the entry (i, i + off[k]), zero where that column does not exist"""
    OFFS = (-BAND, -1, 0, 1, BAND)

    def __init__(self, n, diags):
        self.n = n
        self.diags = [np.ascontiguousarray(d, dtype=np.float64) for d in diags]
        self._cast = {}

    def _d(self, dtype):
        dtype = np.dtype(dtype)
        if dtype not in self._cast:
            self._cast[dtype] = [d.astype(dtype) for d in self.diags]
        return self._cast[dtype]

    def apply(self, x):
        """A·x in x's own type, as shifted slices"""
        n = self.n
        d = self._d(x.dtype)
        y = d[2] * x
        for k, off in enumerate(self.OFFS):
            if off < 0 and -off < n:
                y[-off:] += d[k][-off:] * x[:off]
            elif off > 0 and off < n:
                y[:-off] += d[k][:-off] * x[off:]
        return y

    def csr(self):
        """→ (rowptr, col, val) with sorted columns, for upload"""
        n = self.n
        i = np.arange(n, dtype=np.int64)
        cols = np.stack([i + off for off in self.OFFS], axis=1)
        vals = np.stack(self.diags, axis=1)
        keep = (cols >= 0) & (cols < n)
        rowptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(keep.sum(axis=1), out=rowptr[1:])
        return rowptr.astype(np.int32), cols[keep].astype(np.int32), vals[keep]


def banded(n, seed=0, spd=False):
    """nonsymmetric: four independent off-diagonals in −[0.2, 1], diagonal in [4.5, 5.5] (strictly row dominant).
    spd = True: the two upper diagonals mirror the lower ones — symmetric and strictly dominant with a positive diagonal, hence SPD."""
    rng = np.random.default_rng(seed)
    B = BAND
    lB, l1, u1, uB = (-rng.uniform(0.2, 1.0, n) for _ in range(4))
    d = rng.uniform(4.5, 5.5, n)
    if spd:
        u1 = np.zeros(n); uB = np.zeros(n)
        u1[:-1] = l1[1:]
        if B < n:
            uB[:-B] = lB[B:]
    lB[:min(B, n)] = 0.0; l1[:1] = 0.0; u1[-1:] = 0.0; uB[max(n - B, 0):] = 0.0
    return Banded(n, [lB, l1, d, u1, uB])


def csr_apply(rowptr, col, val, x):
    """A·x from CSR arrays in x's type, row-wise with np.add.reduceat (empty rows give 0)"""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    y = np.zeros(len(rowptr) - 1, dtype=x.dtype)
    if len(col) == 0:
        return y
    prod = np.asarray(val).astype(x.dtype) * x[np.asarray(col)]
    nonempty = rowptr[1:] > rowptr[:-1]
    y[nonempty] = np.add.reduceat(prod, rowptr[:-1][nonempty])
    return y
