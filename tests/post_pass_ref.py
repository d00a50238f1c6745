"""Host restatement of the cycle's fused post pass (mgs_hier_post_pass), its derived per-row error bar, and the helpers the CPU and GPU
tests of that pass share.

The pass.  For a level with operator A (CSR, stored order), aggregate map agg (−1: the row lies outside every aggregate), ω, a coarse
vector e_c and per-row inputs, with  s_i = Σ_k v_ik·e_c[c_ik]  over row i of the level's post-pass OPERAND,  pe_i = e_c[agg_i] (0 for
agg_i < 0)  and  d_i = fl(ω·fl(1/a_ii)):
    t-form      (bvec = t = b + r)      x_i = pe_i + d_i·(t_i − s_i)
    (r, b)-form (bvec = r, xin = b)     x_i = (d_i·b_i + pe_i) + d_i·(r_i − s_i)
The operand is one of three, each in the order the library documents:
    "gather" / "mapped"   A itself in stored order, every column j replaced by agg[j] (an entry whose column lies outside every aggregate
                          stays in its place and contributes nothing); the gather form maps at run time, the mapped form at setup — the
                          same products in the same order;
    "merged"              A·P: per row the entries that fall into one aggregate summed in ascending column order (the first is stored,
                          the later ones are added, one rounding each), the entries of unaggregated columns dropped, the aggregates in
                          ascending order (k_build_ap, setup_agmg.hip);
and its FP32 copy holds np.float32(v) (round to nearest); the kernels widen it to FP64 before the product.

Two evaluations.  (a) `evaluate(..., np.float64)`: the kernels' own association — s starts at 0.0 and takes the products one by one in
stored order, one rounding per product and per sum, no FMA (the library is built with contraction off; numpy never contracts); the
padded gather steps of the coded kernel add +0.0, which changes no bit of a sum that started at +0.0.  Where the documented order is a
promise (the operand has no row longer than 64, so the coded kernel or the gather kernel walks it front to back), (a) is what the device
must return BIT FOR BIT.  (b) `evaluate(..., np.longdouble)`: the same formula from the same FP64 (or FP32) operand values and the same
d in 64-bit-mantissa arithmetic; its own error, (m + 4)·2⁻⁶⁴ relative to the same magnitudes, is 2⁻¹¹ of the bar below and is ignored.

The bar, per row, derived (u = 2⁻⁵³, m = stored length of the operand's row, S_i = Σ_k |v_ik|·|e_c[c_ik]|).  Standard model
fl(a ∘ b) = (a ∘ b)(1 + δ), |δ| ≤ u, no underflow (every input here lies in [0.5, 2] in magnitude, or is a sum of such):
  * ŝ_i: m products (one δ each) and m additions of which the first, 0.0 + p, is exact: every product carries at most m factors
    (1 + δ), so |ŝ_i − s_i| ≤ γ_m·S_i with γ_m = m·u/(1 − m·u) = m·u + O(u²).
  * t-form: x̂ = fl(pe + fl(d·fl(t − ŝ))).  t − ŝ adds one δ to |t| + S, the product with d a second, the final sum a third, which
    also falls on pe.  First order:  |x̂ − x| ≤ u·(|pe| + 3·|d|·|t| + (m + 3)·|d|·S) ≤ (m + 3)·u·(|pe| + |d|·(|t| + S)).
  * (r, b)-form: x̂ = fl(fl(fl(d·b) + pe) + fl(d·fl(r − ŝ))).  d·b carries three δ (product, inner sum, final sum), pe two, d·r three,
    d·S m + 3:  |x̂ − x| ≤ (m + 3)·u·(|d·b| + |pe| + |d|·(|r| + S)) to first order; the issue states m + 4 for this form and this
    module keeps the issue's figure (it is the larger one).
  * One further u in each form covers the second-order terms ((m + 3)²u² ≪ u for m < 2²⁶):
        t-form       |x̂_i − x_i| ≤ (m + 4)·u·(|pe_i| + |d_i|·(|t_i| + S_i))
        (r, b)-form  |x̂_i − x_i| ≤ (m + 5)·u·(|d_i·b_i| + |pe_i| + |d_i|·(|r_i| + S_i))
  * Merged against unmerged: a value of A·P is a sum of up to L entries of A with L − 1 roundings, so an evaluation on the merged operand
    compared with the exact sum over the UNMERGED operand gets (longest merged run)·u more on the S term, S taken over the unmerged row
    (`bar(..., extra=L)`).
x_i is the value from (b); the comparator `ratios` returns |x̂ − x| / bar per row, and a row passes at ≤ 1.

Inputs.  The tests draw operand values and vectors from [0.5, 2] with random signs: no term of a row is negligible beside the row's sum,
so a dropped or doubled term, an e_c of the neighbouring aggregate or a d of the neighbouring row moves x_i by at least
|d|·0.25 ≈ 0.07 — fourteen orders of magnitude above the bar — and the comparator cannot miss it."""
import numpy as np
import scipy.sparse as sps

U = 2.0 ** -53
SENT = -1.2345e30      # what the guard zones and the unwritten entries hold
GUARD = 64
INT_MAX = 0x7fffffff


class Guarded:
    """a device vector of n entries with GUARD sentinels on either side, sentinel-filled (the class of tests/test_gpu_pre_nodiag.py)"""
    def __init__(self, ctx, mg, n):
        self.n = n
        self.buf = ctx.vec(np.full(n + 2 * GUARD, SENT))
        self.v = mg.Vec.wrap(ctx, self.buf.ptr + 8 * GUARD, n)

    def check(self, what):
        a = self.buf.numpy()
        assert np.all(a[:GUARD] == SENT) and np.all(a[GUARD + self.n:] == SENT), what
        return a[GUARD:GUARD + self.n].copy()


def signed(rng, size):
    """[0.5, 2] in magnitude, random sign"""
    return rng.uniform(0.5, 2.0, size) * rng.choice([-1.0, 1.0], size)


def randomize(pattern, rng, quantum=None, diag_shift=0.0):
    """a CSR matrix on `pattern` (diagonal added) with off-diagonal values from ±[0.5, 2] and diagonal values from +[0.5, 2]; quantum: values
    rounded to multiples of it (2⁻¹⁰: every A·P sum is then exact in FP64 and in FP32-rounded form independent of the summation order);
    diag_shift: added to the diagonal (quantized values can cancel exactly in a Galerkin sum: a shift of 4 keeps every coarse diagonal
    of a hierarchy built on the operator away from zero)"""
    P = (sps.csr_matrix(pattern) + sps.identity(pattern.shape[0], format="csr")).tocsr()
    P.sum_duplicates(); P.sort_indices()
    v = signed(rng, P.nnz)
    rows = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
    v[rows == P.indices] = np.abs(v[rows == P.indices]) + diag_shift
    if quantum:
        v = np.round(v / quantum) * quantum
    return sps.csr_matrix((v, P.indices.copy(), P.indptr.copy()), shape=P.shape)


class Operand:
    """rows of (coarse column, value) pairs in stored order; col < 0: the entry contributes nothing"""
    def __init__(self, rowptr, col, val, kind):
        self.rowptr = np.asarray(rowptr, dtype=np.int64); self.col = np.asarray(col, dtype=np.int64); self.val = val; self.kind = kind
        self.n = len(self.rowptr) - 1
        self.len = np.diff(self.rowptr)

    @property
    def max_len(self):
        return int(self.len.max()) if self.n else 0

    @property
    def mean_len(self):
        return len(self.col) / max(self.n, 1)

    def f32(self):
        return Operand(self.rowptr, self.col, self.val.astype(np.float32), self.kind + "32")

    def block_nnz(self):
        return np.diff(self.rowptr[np.minimum(np.arange(0, self.n + 256, 256), self.n)])


def operand_mapped(A, agg):
    """A in stored order with col_agg[k] = agg[col[k]]"""
    A = A.tocsr()
    return Operand(A.indptr, np.asarray(agg, dtype=np.int64)[A.indices], A.data.copy(), "mapped")


def operand_merged(A, agg):
    """A·P as k_build_ap builds it; returns the operand and the longest merged run"""
    A = A.tocsr(); agg = np.asarray(agg, dtype=np.int64)
    n = A.shape[0]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr))
    ca = agg[A.indices]
    keep = ca >= 0
    rows, ca, v = rows[keep], ca[keep], A.data[keep]
    order = np.lexsort((np.arange(len(ca)), ca, rows))          # by row, aggregate, then stored (= ascending column) order
    rows, ca, v = rows[order], ca[order], v[order]
    first = np.ones(len(ca), dtype=bool)
    first[1:] = (rows[1:] != rows[:-1]) | (ca[1:] != ca[:-1])
    run = np.cumsum(first) - 1                                   # output entry of every input entry
    nout = int(run[-1]) + 1 if len(run) else 0
    pos = np.arange(len(ca)) - np.flatnonzero(first)[run]        # position inside its run
    out = np.zeros(nout)
    for p in range(int(pos.max()) + 1 if len(pos) else 0):       # the first entry is stored, the later ones are added in order
        m = pos == p
        out[run[m]] = v[m] if p == 0 else out[run[m]] + v[m]
    rp = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rp, rows[first] + 1, 1)
    return Operand(np.cumsum(rp), ca[first], out, "merged"), (int(pos.max()) + 1 if len(pos) else 0)


def dvec(A, omega):
    """d_i = fl(ω·fl(1/a_ii))"""
    return omega * (1.0 / A.diagonal())


def _gathered(op, ec, dtype):
    ok = op.col >= 0
    e = np.where(ok, np.asarray(ec, dtype=dtype)[np.where(ok, op.col, 0)], dtype(0))
    return op.val.astype(dtype), e, ok


def row_sums(op, ec, dtype=np.float64, skip=None):
    """s_i, sequentially from 0.0 in stored order; skip: entry indices left out (the mutations of the CPU test)"""
    v, e, _ = _gathered(op, ec, dtype)
    p = v * e
    if skip is not None:
        p[np.asarray(skip)] = 0
    s = np.zeros(op.n, dtype=dtype)
    for k in range(op.max_len):
        rows = np.flatnonzero(op.len > k)
        s[rows] = s[rows] + p[op.rowptr[rows] + k]
    return s


def abs_sums(op, ec):
    v, e, _ = _gathered(op, ec, np.longdouble)
    s = np.zeros(op.n, dtype=np.longdouble)
    np.add.at(s, np.repeat(np.arange(op.n), op.len), np.abs(v) * np.abs(e))
    return s


def pe_of(agg, ec, dtype=np.float64):
    agg = np.asarray(agg)
    return np.where(agg >= 0, np.asarray(ec, dtype=dtype)[np.where(agg >= 0, agg, 0)], dtype(0))


def evaluate(op, d, agg, ec, bvec, xin=None, dtype=np.float64, s=None, pe=None):
    """the post pass in `dtype` with the kernels' association; s / pe: substitutes (mutations)"""
    T = dtype
    s = row_sums(op, ec, T) if s is None else s
    pe = pe_of(agg, ec, T) if pe is None else pe
    d = np.asarray(d, dtype=T); bvec = np.asarray(bvec, dtype=T)
    if xin is None:
        return pe + d * (bvec - s)
    return (d * np.asarray(xin, dtype=T) + pe) + d * (bvec - s)


def bar(op, d, agg, ec, bvec, xin=None, extra=0, S=None):
    """the derived per-row bar (module docstring); extra: longest merged run when a merged evaluation is held to the unmerged sum, S then
    being the unmerged operand's Σ|v||e|"""
    L = np.longdouble
    S = abs_sums(op, ec) if S is None else S
    pe = np.abs(pe_of(agg, ec, L)); d = np.abs(np.asarray(d, dtype=L)); m = op.len.astype(L)
    if xin is None:
        return ((m + 4) * (pe + d * (np.abs(np.asarray(bvec, dtype=L)) + S)) + extra * d * S) * L(U)
    return ((m + 5) * (d * np.abs(np.asarray(xin, dtype=L)) + pe + d * (np.abs(np.asarray(bvec, dtype=L)) + S)) + extra * d * S) * L(U)


def ratios(xhat, xref, bar_):
    """|x̂ − x| / bar per row; a row passes at ≤ 1"""
    return np.asarray(np.abs(np.asarray(xhat, dtype=np.longdouble) - xref) / bar_, dtype=np.float64)


def pre_pass_host(A, d, agg, nc, b):
    """the host pre pass of tests/test_gpu_pre_nodiag.py: r = b − Â·b with Â = A·diag(d), t = b + r, r_c = Pᵀr"""
    r = b - (A @ sps.diags(d)) @ b
    ok = np.asarray(agg) >= 0
    return b + r, r, np.bincount(np.asarray(agg)[ok], weights=r[ok], minlength=nc)


# ---- operator families (patterns; values come from `randomize`) ----
def stencil_1d2d(n):
    """mean row length ≤ 4.5: a 1-D three-point line with a second coupling at distance 16 on every other row"""
    i = np.arange(n)
    r = np.r_[i[:-1], i[1:], i[:-16:2], i[16::2]]; c = np.r_[i[1:], i[:-1], i[16::2], i[:-16:2]]
    return sps.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))


def stencil_5pt(n, w=16):
    """the 2-D five-point pattern on rows of w points, cut at n rows"""
    i = np.arange(n)
    e = i[(i % w) != w - 1]; e = e[e + 1 < n]
    s = i[i + w < n]
    r = np.r_[e, e + 1, s, s + w]; c = np.r_[e + 1, e, s + w, s]
    return sps.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))


def stencil_27pt(n, w=6):
    """the 3-D 27-point pattern on w × w planes, cut at n rows (a Galerkin-like operator: rows of up to 27 entries)"""
    i = np.arange(n)
    x, y, z = i % w, (i // w) % w, i // (w * w)
    r, c = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == dy == dz == 0:
                    continue
                ok = (x + dx >= 0) & (x + dx < w) & (y + dy >= 0) & (y + dy < w) & (z + dz >= 0)
                j = i + dx + w * dy + w * w * dz
                ok &= j < n
                r.append(i[ok]); c.append(j[ok])
    return sps.csr_matrix((np.ones(sum(map(len, r))), (np.concatenate(r), np.concatenate(c))), shape=(n, n))


def random_graph(n, deg, rng, symmetric=True):
    """the graph of test_random_aggregations_and_graph_laplacians: deg random neighbours per row plus a ring"""
    rows = np.repeat(np.arange(n), deg); cols = rng.integers(0, n, size=n * deg)
    ring = np.arange(n)
    W = sps.csr_matrix((np.ones(n * deg), (rows, cols)), shape=(n, n)) + sps.csr_matrix((np.ones(n), (ring, (ring + 1) % n)), shape=(n, n))
    if symmetric:
        W = W + W.T
    W = W.tolil(); W.setdiag(0); W = W.tocsr(); W.eliminate_zeros()
    return W


def unaggregated_case(n, rng, run=(768, 1068), singles=(0, 255, 256, 700)):
    """five-point operator with pairs as aggregates, except: single rows outside every aggregate (first / last row of a row block, one in a
    block's middle — their neighbours keep some unaggregated columns), and a run of consecutive rows, decoupled from the rest and all
    outside every aggregate: the operand has empty rows and one entirely empty row block"""
    Pn = stencil_5pt(n).tocoo()
    inside = (Pn.row >= run[0]) & (Pn.row < run[1])
    keep = inside == ((Pn.col >= run[0]) & (Pn.col < run[1]))
    Pn = sps.csr_matrix((Pn.data[keep], (Pn.row[keep], Pn.col[keep])), shape=(n, n))
    g = pairs(n).copy(); g[list(singles)] = -1; g[run[0]:run[1]] = -1
    return randomize(Pn, rng), renumber(g)


def pairs(n):
    return (np.arange(n) // 2).astype(np.int32)


def random_aggregates(n, rng, sizes=(1, 2, 3, 8, 16), g0=0.05):
    """aggregates of the given sizes with shuffled membership and a share of rows outside every aggregate (the generator of
    test_random_aggregations_and_graph_laplacians, sizes drawn from `sizes`)"""
    sz = []
    while sum(sz) < n:
        sz.append(int(rng.choice(sizes)))
    agg = np.repeat(np.arange(len(sz)), sz)[:n]
    agg = agg[rng.permutation(n)]
    agg[rng.random(n) < g0] = -1
    _, inv = np.unique(agg[agg >= 0], return_inverse=True); agg[agg >= 0] = inv
    return agg.astype(np.int32)


def renumber(agg):
    agg = np.asarray(agg).copy()
    _, inv = np.unique(agg[agg >= 0], return_inverse=True); agg[agg >= 0] = inv
    return agg.astype(np.int32)


def agg_P(agg, nc):
    ok = np.asarray(agg) >= 0
    return sps.csr_matrix((np.ones(int(ok.sum())), (np.flatnonzero(ok), np.asarray(agg)[ok])), shape=(len(agg), nc))


class Case:
    """one level under test: operator, aggregates, ω, the three operands, d and random vectors"""
    def __init__(self, A, agg, omega=0.6, seed=1):
        self.A = A.tocsr(); self.A.sort_indices()
        self.agg = np.asarray(agg, dtype=np.int32); self.n = A.shape[0]; self.nc = int(self.agg.max()) + 1
        self.omega = omega
        self.d = dvec(self.A, omega)
        self.mapped = operand_mapped(self.A, self.agg)
        self.merged, self.longest_run = operand_merged(self.A, self.agg)
        rng = np.random.default_rng(seed)
        self.t, self.r, self.b, self.ec = signed(rng, self.n), signed(rng, self.n), signed(rng, self.n), signed(rng, self.nc)

    def operand(self, kind):
        return {"mapped": self.mapped, "gather": self.mapped, "merged": self.merged, "merged32": self.merged.f32()}[kind]

    def forms(self):
        """(name, bvec, xin) of the two forms"""
        return (("t", self.t, None), ("rb", self.r, self.b))
