"""Host restatement of ONE ROW SHARD's cycle (cycle_fused, cycle_unfused, coarse_solve_inner and halo_transport of
multigridsolver_amd/csrc/cycle.hip; the operands of hier_operands.hip), numpy only: no device, no oracle, no second process.  It is composed
from the restatements the unsharded steps already have — pre_pass_ref, post_pass_ref, spmv_ref, kcycle_ref, galerkin_ref — and adds what
exists on a shard only.

The shard.  `cut(G, r0, r1)` takes rows [r0, r1) of a global CSR matrix into LOCAL column numbering: owned columns first (global column
− r0), then one halo slot per distinct off-shard column in ascending global order; every row sorted by local column.  A level is the
n × (n + n_halo) operator A, the aggregate of every owned row (agg, −1: none), the coarse column of every halo slot (halo_cmap, −1: none,
else in [nc, nc + n_halo_coarse)) and ω.  Its coarse operator is galerkin_ref's product on the extended column map agg ⧺ halo_cmap.

The extended operands (`Level.deliver`), from the D⁻¹ of the halo rows the owners delivered at setup (one exchange per level):
    wd_ext   fl(ω·fl(1/a_jj)) on owned rows, fl(ω·dinv_halo) on halo slots           (k_axpby over n_ext entries)
    Â        fl(a_ik·wd_ext_k) per stored entry                                       (scale_vals_kernel)
    cmap_ext agg ⧺ halo_cmap;  aggregate-mapped A and merged A·P over [0, nc + n_halo_coarse): post_pass_ref's operands on cmap_ext.

The steps.  Every row sum starts at +0.0 and takes its products in stored order, one rounding per product and per sum (no FMA).
    pre pass on [b; payload]   "residual", "agg", "grouped": s_i = Σ Â_ik·bx_k;  "gather": s_i = Σ a_ik·fl(wd_ext_k·bx_k);
                               r = b − s, t = b + r, r_c = Pᵀr over the members in ascending order
    post pass on [e_c; halo]   (r, b)-form x = (d·b + pe) + d·(r − s), or the t-form x = pe + d·(t − s) behind the grouped arm; s over the
                               mapped operand (forms 0 and 1: the same products) or the merged one (form 2)
    one kernel per step        x = (ω·dinv)·b from zero; Jacobi, residual and SpMV of the n × (n + n_halo) operator on [x; halo of x];
                               restrict_agg, prolong_agg; cycle_unfused's sweep counts from a zero and a non-zero guess
    coarsest "solve"           x_c = fl(0.5·fl(dinv_c·r_c)): elementwise, hence the same on a shard and on the whole operator
    σ                          e_c = fl(σ·e_c) on the owned entries, before its halo is exchanged
    K step                     kcycle_ref's reductions and updates; the peers' parts are added (one rounding) to (ρ1, α1), to γ and to
                               (ρ2, α2) where kc_allreduce runs.

The driver.  `Run(levels, cfg, log).cycle(b, x0)` walks the cycle and, wherever the library asks its transport for values, takes the next entry
of the LOG the device run produced (tests/test_gpu_shard_cycle.py) — or that `Peers` produces on the host (tests/test_shard_ref_cpu.py).  An
entry is a dict: kind ("plain", "begin", "end", "fused", "coarse", "allreduce"), level, phase, in_place, src (the owned entries of the vector
the library handed over) and, on phase 0, answer (what the peers returned).  The driver asserts kind, level, phase and in_place — which is
halo_transport's precedence restated: native plan (never here), then for an in-place exchange outside the fused passes the split pair (when
the caller has interior blocks to launch, or no plain callback exists), the plain callback, and last the fused callback — compares src with
its own vector BIT FOR BIT (a difference is recorded under the step's name in `Run.mismatch`), and goes on with the logged answer.  `finish()`
fails unless the log was used up exactly.

Twin and bars.  The chain itself runs in FP64 only.  Every matrix pass is evaluated a second time in long double from the SAME FP64 inputs
(operand values as stored, vectors as the FP64 chain produced them), and held to the bar its own module derives: pre_pass_ref's (m + 2)·u
·(|b| + S) for r, post_pass_ref.bar for x, spmv_ref's γ_{L+1} bars for Jacobi, residual and SpMV — all with the row taken over the owned
and the halo columns.  `Run.ratio[step]` keeps the largest |FP64 − twin| / bar of every step, `Run.last` the twin and bar of the pass that
wrote the cycle's result x."""
import numpy as np
import scipy.sparse as sps

import galerkin_ref as G
import kcycle_ref as K
import post_pass_ref as Q
import pre_pass_ref as P
import spmv_ref as S

U = Q.U
LD = np.longdouble
ARMS = ("gather", "residual", "agg", "grouped")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def cut(Gm, r0, r1):
    """(A_loc, halo_rows): rows [r0, r1) of the global CSR Gm in local column numbering, and the global row of every halo slot"""
    Gm = Gm.tocsr(); Gm.sort_indices()
    n = r1 - r0
    lo, hi = int(Gm.indptr[r0]), int(Gm.indptr[r1])
    ci = Gm.indices[lo:hi].astype(np.int64)
    off = (ci < r0) | (ci >= r1)
    halo_rows = np.unique(ci[off])
    loc = np.where(off, n + np.searchsorted(halo_rows, ci), ci - r0)
    A = sps.csr_matrix((Gm.data[lo:hi].copy(), loc, Gm.indptr[r0:r1 + 1] - lo), shape=(n, n + len(halo_rows)))
    A.sort_indices()
    return A, halo_rows


class Level:
    """one level of a shard: A (n × (n + nh)), and — unless it is the coarsest — agg, nc, halo_cmap, nhc"""

    def __init__(self, A, omega, agg=None, nc=0, halo_cmap=None, nhc=0):
        self.A = A.tocsr(); self.A.sort_indices()
        self.n, cols = self.A.shape
        self.nh = cols - self.n
        self.omega = omega
        self.dinv = 1.0 / self.A.diagonal()
        self.coarsest = agg is None
        if not self.coarsest:
            self.agg = np.asarray(agg, dtype=np.int32); self.nc = int(nc)
            self.halo_cmap = np.asarray(halo_cmap, dtype=np.int32); self.nhc = int(nhc)
            assert len(self.agg) == self.n and len(self.halo_cmap) == self.nh
            self.cmap_ext = np.r_[self.agg, self.halo_cmap].astype(np.int32)
        self.wd_ext = None

    def galerkin(self):
        """the shard's coarse operator nc × (nc + nhc) (k_galerkin_agg_ext)"""
        cptr, mem = G.member_lists(self.agg, self.nc)
        rp, ci, v, _ = G.galerkin_agg_fast(self.A.indptr, self.A.indices, self.A.data, self.cmap_ext, mem, cptr, self.nc + self.nhc)
        return sps.csr_matrix((v, ci, rp), shape=(self.nc, self.nc + self.nhc))

    def deliver(self, dinv_halo, wd_slot=None, cmap_ext=None, diag_first=False):
        """the extended operands from the delivered D⁻¹.  Planted defects: wd_slot — the halo slots take this OWNED row's wd; cmap_ext —
        another extended column map; diag_first — every row holds (and therefore sums) its diagonal entry first instead of at its column's place"""
        assert len(dinv_halo) == self.nh
        if diag_first:
            self.A = _diag_first(self.A)
        self.wd_ext = self.omega * np.r_[self.dinv, np.asarray(dinv_halo, dtype=np.float64)]
        if wd_slot is not None:
            self.wd_ext[self.n:] = self.wd_ext[wd_slot]
        self.hat = self.A.data * self.wd_ext[self.A.indices]
        cm = self.cmap_ext if cmap_ext is None else np.asarray(cmap_ext, dtype=np.int32)
        self.mapped = Q.operand_mapped(self.A, cm)
        self.merged, self.longest = Q.operand_merged(self.A, cm)
        return self


def _diag_first(A):
    """the same matrix with every row's diagonal entry moved to the front of the row (the other entries keep their order)"""
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    k = np.lexsort((np.arange(A.nnz), A.indices != rows, rows))
    B = sps.csr_matrix(A.shape)
    B.indptr, B.indices, B.data = A.indptr.copy(), A.indices[k].copy(), A.data[k].copy()
    return B


def hierarchy(A0, omega, specs):
    """levels of a shard from its finest operator and, per coarsening, (agg, nc, halo_cmap, nhc); the last level is the coarsest"""
    levels, A = [], A0
    for agg, nc, hm, nhc in specs:
        levels.append(Level(A, omega, agg, nc, hm, nhc))
        A = levels[-1].galerkin()
    levels.append(Level(A, omega))
    return levels


# ------------------------------------------------------------------ the passes, each in a dtype
def _ext_row_abs(L, val, xext):
    """S_i = Σ_k |v_ik|·|x_k| over owned and halo columns, long double"""
    mag = np.abs(np.asarray(val, dtype=LD)) * np.abs(np.asarray(xext, dtype=LD))[L.A.indices]
    s = np.zeros(L.n, dtype=LD)
    np.add.at(s, np.repeat(np.arange(L.n), np.diff(L.A.indptr)), mag)
    return s


def pre_pass(L, b, payload, arm, T=np.float64):
    """(t, r, r_c) on [b; payload] in the association of `arm`"""
    bx = np.r_[b, payload].astype(T)
    if arm == "gather":
        p = L.A.data.astype(T) * (L.wd_ext.astype(T) * bx)[L.A.indices]
    else:
        p = L.hat.astype(T) * bx[L.A.indices]
    s = P.row_sums(L.A.indptr, p, T)
    bi = np.asarray(b, dtype=T)
    r = bi - s
    return bi + r, r, P.restrict(r, L.agg, L.nc, T)


def pre_bars(L, b, payload, arm):
    """(bar_t, bar_r, bar_rc) of pre_pass_ref, rows taken over owned and halo columns"""
    bx = np.r_[b, payload]
    if arm == "gather":
        Sabs = _ext_row_abs(L, L.A.data, np.abs(L.wd_ext.astype(LD)) * np.abs(bx.astype(LD)))
    else:
        Sabs = _ext_row_abs(L, L.hat, bx)
    m = np.diff(L.A.indptr).astype(LD) + (1 if arm == "gather" else 0)
    w = np.abs(np.asarray(b, dtype=LD)) + Sabs
    ok = L.agg >= 0
    ka = np.bincount(L.agg[ok], minlength=L.nc).astype(LD)
    brc = np.zeros(L.nc, dtype=LD)
    np.add.at(brc, L.agg[ok], (m[ok] + 2 + ka[L.agg[ok]]) * w[ok])
    return (m + 4) * w * LD(U), (m + 2) * w * LD(U), brc * LD(U)


def post_operand(L, form):
    return L.merged if form == 2 else L.mapped


def post_pass(L, ec_ext, bvec, xin, form, T=np.float64):
    """x of the post pass on [e_c; halo of e_c]: xin None = t-form (bvec = t), else bvec = r and xin = b"""
    return Q.evaluate(post_operand(L, form), L.wd_ext[:L.n], L.agg, ec_ext, bvec, xin, dtype=T)


def post_bar(L, ec_ext, bvec, xin, form):
    return Q.bar(post_operand(L, form), L.wd_ext[:L.n], L.agg, ec_ext, bvec, xin)


def op(L, kind, xext, b=None, T=np.float64):
    """spmv / residual / jacobi of the n × (n + nh) operator on xext = [x; halo of x]"""
    s = S.row_sums_sequential(L.A.indptr, L.A.indices, L.A.data, xext, T)
    if kind == "spmv":
        return s
    r = np.asarray(b, dtype=T) - s
    if kind == "residual":
        return r
    return np.asarray(xext[:L.n], dtype=T) + (T(L.omega) * L.dinv.astype(T)) * r


def op_bar(L, kind, xext, b=None):
    return S.bar(kind, L.A.indptr, L.A.indices, L.A.data, xext, b, L.dinv, L.omega)


def jacobi_zero(L, b, T=np.float64):
    return (T(L.omega) * L.dinv.astype(T)) * np.asarray(b, dtype=T)


def prolong(L, ec, T=np.float64):
    return Q.pe_of(L.agg, ec, T)


def coarsest_solve(L, b, T=np.float64):
    """the test's coarsest "solve": x_c = fl(0.5·fl(dinv_c·b))"""
    return T(0.5) * (L.dinv.astype(T) * np.asarray(b, dtype=T))


# ------------------------------------------------------------------ the cycle's shape under the options, and the driver
class Config:
    """what decides the cycle's form: smoother, σ, K levels and form, the installed callbacks, and per level (not the coarsest) the arm of the
    pre pass, the post pass's operand and whether the level splits its launches around an exchange (halo_split)"""

    def __init__(self, installed=("fused",), nu=(1, 1), sigma=1.0, kcycle=0, energy=False, allreduce=False, fuse=True, forms=None):
        self.installed = frozenset(installed); self.nu = tuple(nu); self.sigma = float(sigma)
        self.kcycle = int(kcycle); self.energy = bool(energy); self.allreduce = bool(allreduce); self.fuse = bool(fuse)
        self.forms = forms or {}
        assert self.installed <= {"plain", "split", "fused"}

    @property
    def sharded(self):      # h->halo || h->halo_begin
        return bool(self.installed & {"plain", "split"})

    def fuses(self):
        return self.fuse and self.nu == (1, 1) and "fused" in self.installed

    def form(self, l):
        return self.forms.get(l, dict(arm="agg", post=2, split=False))


def pre_arm(fuse_operands, has_val_wd, operands, grouped, shard_split, rows, max_row_len, aggpre_max_rows):
    """level_pre_arm restated"""
    if grouped and not shard_split:
        return "grouped"
    if fuse_operands and has_val_wd and rows <= aggpre_max_rows and max_row_len <= 64:
        return "agg"
    return "residual" if operands else "gather"


def transport(installed, in_place, fused_pass, two_phase):
    """halo_transport restated (no native plan): "plain", "split", "fused" or None"""
    in_place = in_place and not (fused_pass and "fused" in installed)
    if in_place and "split" in installed and (two_phase or "plain" not in installed):
        return "split"
    if in_place and "plain" in installed:
        return "plain"
    return "fused" if "fused" in installed else None


CALLS = {"plain": (("plain", 0),), "split": (("begin", 0), ("end", 1)), "fused": (("fused", 0), ("fused", 1))}


class Run:
    def __init__(self, levels, cfg, log, twin=True, first=True):
        """first: this is the hierarchy's first cycle that can fuse — the one whose preparation fetches the owners' D⁻¹"""
        self.levels, self.cfg, self.log, self.pos, self.twin, self.first = levels, cfg, list(log), 0, twin, first
        self.mismatch, self.ratio, self.scalars, self.last, self.calls = [], {}, {}, None, []
        self.swap = False
        self.defects = {}      # level -> keyword arguments of Level.deliver (the planted defects of the CPU test)

    # ---- the log
    def take(self, what, **want):
        assert self.pos < len(self.log), f"the log ends before: {what} {want}"
        e = self.log[self.pos]
        for k, v in want.items():
            assert e.get(k) == v, f"log entry {self.pos} ({what}): {k} = {e.get(k)!r}, the cycle's form asks for {v!r}; entry {_brief(e)}"
        self.pos += 1
        self.calls.append(_brief(e))
        return e

    def compare(self, what, logged, mine):
        if not same_bits(logged, mine):
            bad = np.flatnonzero(bits(logged) != bits(mine)) if np.shape(logged) == np.shape(mine) else np.zeros(0, int)
            self.mismatch.append((what, int(len(bad)), bad[:4].tolist(), np.asarray(logged)[bad[:4]].tolist(), np.asarray(mine)[bad[:4]].tolist()))

    def finish(self):
        assert self.pos == len(self.log), f"{len(self.log) - self.pos} log entries were not used, first {_brief(self.log[self.pos])}"
        return self

    def exchange(self, l, src, what, in_place, fused_pass, two_phase):
        """the halo values of a level-l vector whose owned entries are src"""
        via = transport(self.cfg.installed, in_place, fused_pass, two_phase)
        assert via, f"{what}: level {l} is a row shard but no callback serves this exchange"
        ans = None
        for kind, phase in CALLS[via]:
            e = self.take(what, kind=kind, level=l, phase=phase, in_place=in_place)
            self.compare(f"{what} ({kind}, phase {phase})", e["src"], src)
            if phase == 0:
                ans = np.asarray(e["answer"], dtype=np.float64)
        assert ans.shape == (self.levels[l].nh,), (what, ans.shape)
        return ans

    def allreduce(self, vals, what):
        if not self.cfg.sharded:
            return list(vals)
        e = self.take(what, kind="allreduce", count=len(vals))
        self.compare(what, e["src"], np.asarray(vals, dtype=np.float64))
        return [np.float64(v) + np.float64(p) for v, p in zip(vals, e["answer"])]

    def step(self, name, fn, bar, final):
        """fn(T) in FP64; its long-double twin from the same inputs and the largest error/bar ratio"""
        out = fn(np.float64)
        if self.twin:
            ref, b = fn(LD), bar()
            first = lambda v: v[1] if isinstance(v, tuple) else v      # noqa: E731  (pre pass: (t, r, r_c) — r is what the bar is of)
            q = S.ratios(first(out), first(ref), b)
            self.ratio[name] = max(self.ratio.get(name, 0.0), float(q.max()) if len(q) else 0.0)
            if final:
                self.last = (first(ref), b)
        return out

    # ---- setup: one D⁻¹ exchange per level that can run the fused passes (mgs_prepare_fused), in place, outside the fused passes
    def setup(self):
        if self.first and self.cfg.fuses():
            for l, L in enumerate(self.levels[:-1]):
                L.deliver(self.exchange(l, L.dinv, f"D^-1 of level {l}", True, False, False), **self.defects.get(l, {}))
        return self

    # ---- the cycle
    def cycle(self, b, x0=None):
        self.setup()
        return self.level(0, np.asarray(b, dtype=np.float64), None if x0 is None else np.asarray(x0, dtype=np.float64), x0 is None)

    def level(self, l, b, x, zero):
        if l == len(self.levels) - 1:
            e = self.take(f"coarsest solve (level {l})", kind="coarse")
            self.compare(f"right-hand side of the coarsest solve (level {l})", e["src"], b)
            return coarsest_solve(self.levels[l], b)
        if zero and self.cfg.fuses():
            return self.fused(l, b)
        return self.unfused(l, b, x, zero)

    def coarse_solve(self, l, rhs):
        k_here = 1 <= l <= self.cfg.kcycle and l < len(self.levels) - 1 and (not self.cfg.sharded or self.cfg.allreduce)
        x = self.kstep(l, rhs) if k_here else self.level(l, rhs, None, True)
        return x if self.cfg.sigma == 1.0 else np.float64(self.cfg.sigma) * x

    def fused(self, l, b):
        L, f = self.levels[l], self.cfg.form(l)
        arm, top = f["arm"], l == 0
        payload = self.exchange(l, b, f"right-hand side of level {l} (payload of the pre pass)", False, True, f["split"] and arm in ("gather", "residual"))
        got = payload
        if self.swap and top:      # planted: the pre pass reads e_c's halo room (zeros before its first exchange) ...
            payload = np.zeros(L.nh)
        t, r, rc = self.step(f"pre pass of level {l} ({arm})", lambda T: pre_pass(L, b, payload, arm, T), lambda: pre_bars(L, b, payload, arm)[1], False)
        ec = self.coarse_solve(l + 1, rc)
        ech = self.exchange(l + 1, ec, f"e_c of level {l + 1}", True, True, f["split"])
        if self.swap and top:      # ... and the post pass the payload buffer
            ech = np.resize(got, len(ech))
        ece = np.r_[ec, ech]
        bvec, xin = (t, None) if arm == "grouped" else (r, b)
        return self.step(f"post pass of level {l} (operand {f['post']}, {'t' if xin is None else 'r,b'}-form)",
                         lambda T: post_pass(L, ece, bvec, xin, f["post"], T), lambda: post_bar(L, ece, bvec, xin, f["post"]), top)

    def sharded_op(self, l, kind, x, b, what, final=False):
        L = self.levels[l]
        xe = np.r_[x, self.exchange(l, x, f"{what} of level {l}", True, False, self.cfg.form(l)["split"])]
        return self.step(f"{kind} of level {l}", lambda T: op(L, kind, xe, b, T), lambda: op_bar(L, kind, xe, b), final)

    def unfused(self, l, b, x, zero):
        L, (nu1, nu2), top = self.levels[l], self.cfg.nu, l == 0
        cur, z = x, zero
        for s in range(nu1):
            if z:
                cur, z = jacobi_zero(L, b), False
            else:
                cur = self.sharded_op(l, "jacobi", cur, b, f"x before pre-sweep {s}")
        r = b if z else self.sharded_op(l, "residual", cur, b, "x before the residual")
        ec = self.coarse_solve(l + 1, P.restrict(r, L.agg, L.nc, np.float64))
        cur = prolong(L, ec) if z else cur + prolong(L, ec)
        for s in range(nu2):
            cur = self.sharded_op(l, "jacobi", cur, b, f"x before post-sweep {s}", final=top and s == nu2 - 1)
        return cur

    def kstep(self, l, rhs):
        """coarse_solve_inner with the peers' parts added where kc_allreduce runs"""
        en = self.cfg.energy
        c1 = self.level(l, rhs, None, True)
        v1 = self.sharded_op(l, "spmv", c1, None, "c1 of the K step")
        rho1, alpha1 = self.allreduce(K.first_scalars(c1, v1, rhs, en, True), f"rho1, alpha1 of level {l}")
        rp = K.update_r(rho1, alpha1, rhs, v1)
        c2 = self.level(l, rp, None, True)
        v2 = self.sharded_op(l, "spmv", c2, None, "c2 of the K step")
        (gamma,) = self.allreduce([K.dot_dev(c2 if en else v2, v1)], f"gamma of level {l}")
        rho2, alpha2 = self.allreduce(K.orth_dots(K.quotient(gamma, rho1), c1, c2, v1, v2, rp, en), f"rho2, alpha2 of level {l}")
        scal = [rho1, alpha1, gamma, rho2, alpha2]
        self.scalars[l] = [float(v) for v in scal]
        return K.combine(scal, c1, c2)


def _brief(e):
    return (e.get("kind"), e.get("level"), e.get("phase"), e.get("in_place"))


def cycle(levels, script, b, x0=None, cfg=None, twin=True, first=True, defects=None, swap=False):
    """(x, run) of one cycle of the shard that consumes `script` in order; fails if the script is not used up exactly.  defects, swap: planted
    defects (swap: the pre pass of level 0 reads e_c's halo answer as its payload and the post pass the payload's, where both have one length)"""
    run = Run(levels, cfg or Config(), script, twin, first)
    run.defects = defects or {}
    run.swap = swap
    x = run.cycle(b, x0)
    run.finish()
    return x, run


# ------------------------------------------------------------------ a host transport that produces a log (the CPU tests; the GPU test has its own)
class Peers:
    """plays the peers on the host: answer(level, what, src) returns the halo values of an exchange, reduce(what, vals) the peers' parts of a
    reduction; `record(levels, cfg, b, x0)` walks the cycle once and returns the log the driver then replays"""

    def __init__(self, answer, reduce=None):
        self.answer, self.reduce = answer, reduce

    def record(self, levels, cfg, b, x0=None, first=True):
        peers, log = self, []

        class Recorder(Run):
            def exchange(self, l, src, what, in_place, fused_pass, two_phase):
                via = transport(self.cfg.installed, in_place, fused_pass, two_phase)
                ans = np.asarray(peers.answer(l, what, np.asarray(src, dtype=np.float64)), dtype=np.float64)
                for kind, phase in CALLS[via]:
                    e = dict(kind=kind, level=l, phase=phase, in_place=in_place, src=np.array(src, dtype=np.float64))
                    if phase == 0:
                        e["answer"] = ans
                    log.append(e)
                return ans

            def allreduce(self, vals, what):
                if not self.cfg.sharded:
                    return list(vals)
                part = np.asarray(peers.reduce(what, np.asarray(vals, dtype=np.float64)), dtype=np.float64)
                log.append(dict(kind="allreduce", count=len(vals), src=np.asarray(vals, dtype=np.float64), answer=part))
                return [np.float64(v) + np.float64(p) for v, p in zip(vals, part)]

            def level(self, l, b_, x, zero):
                if l == len(self.levels) - 1:
                    log.append(dict(kind="coarse", src=np.array(b_, dtype=np.float64)))
                    return coarsest_solve(self.levels[l], b_)
                return Run.level(self, l, b_, x, zero)

        Recorder(levels, cfg, [], twin=False, first=first).cycle(b, x0)
        return log


# ------------------------------------------------------------------ fixtures the CPU and the GPU test share
OMEGA = 0.6


def grid7(nx, ny, nz):
    """the 7-point pattern on an nx × ny × nz grid, x fastest (no diagonal)"""
    i = np.arange(nx * ny * nz)
    x, y, z = i % nx, (i // nx) % ny, i // (nx * ny)
    r, c = [], []
    for ok, step in ((x + 1 < nx, 1), (y + 1 < ny, nx), (z + 1 < nz, nx * ny)):
        r += [i[ok], i[ok] + step]; c += [i[ok] + step, i[ok]]
    return sps.csr_matrix((np.ones(sum(map(len, r))), (np.concatenate(r), np.concatenate(c))), shape=(len(i), len(i)))


def vc7(nx, ny, nz, seed):
    """variable-coefficient, nonsymmetric 7-point operator: off-diagonal values from ±[0.5, 2], diagonal from [4.5, 6] (post_pass_ref.randomize
    with a shift of 4: no Galerkin diagonal of two pairwise coarsenings comes near zero)"""
    return Q.randomize(grid7(nx, ny, nz), np.random.default_rng(seed), diag_shift=4.0)


def poisson7(nx, ny, nz):
    """6 on the diagonal, −1 beside it: mgs_csr_poisson3d's values"""
    Pn = grid7(nx, ny, nz)
    return (sps.identity(Pn.shape[0], format="csr") * 6.0 - Pn).tocsr()


def couple(A, rows, slots, rng):
    """A plus one entry per (row, halo slot) pair, values from ±[0.5, 2]"""
    n = A.shape[0]
    E = sps.csr_matrix((Q.signed(rng, len(rows)), (np.asarray(rows), n + np.asarray(slots))), shape=A.shape)
    B = (A + E).tocsr(); B.sort_indices()
    return B


def pair_spec(n, nh, rng, outside=(), unmapped=5, spare=8):
    """(agg, nc, halo_cmap, nhc): pairs of consecutive rows (pairs along x on a grid whose lines hold an even number of points), the rows of
    `outside` and four random ones outside every aggregate, ids ascending with their first member; halo slots in pairs on one coarse halo column,
    `unmapped` of them on none, and `spare` coarse halo columns more than are used"""
    agg = np.arange(n) // 2
    agg[np.r_[np.asarray(outside, dtype=np.int64), rng.choice(n, 4, replace=False)]] = -1
    agg = P.renumber_by_first_member(agg)
    nc = int(agg.max()) + 1
    hm = nc + np.arange(nh) // 2
    hm[rng.choice(nh, unmapped, replace=False)] = -1
    return agg.astype(np.int32), nc, hm.astype(np.int32), (nh + 1) // 2 + spare


def three_levels(A0, seed):
    """a shard's three levels from its finest operator: two pairwise coarsenings with every irregularity of pair_spec on both"""
    rng = np.random.default_rng(seed)
    n, cols = A0.shape
    s0 = pair_spec(n, cols - n, rng, outside=(0, 255, 256, n - 1))
    s1 = pair_spec(s0[1], s0[3], rng, outside=(1, s0[1] - 2), unmapped=3, spare=4)
    return hierarchy(A0, OMEGA, [s0, s1])


def operator_a(seed=11):
    """planes 3..9 of a 12 × 12 × 14 variable-coefficient grid: 1008 rows (four row blocks, the last partial), 144 + 144 halo slots"""
    return cut(vc7(12, 12, 14, seed), 3 * 144, 10 * 144)[0]


def operator_b():
    """poisson3d(16, 4, 12, local_cols=True): 2048 rows in eight exact row blocks"""
    return cut(poisson7(16, 16, 16), 4 * 256, 12 * 256)[0]


def operator_c(blocks=(1, 2), seed=11):
    """operator (a) plus three rows in each of the given row blocks coupled to halo slots"""
    rng = np.random.default_rng(seed + 1)
    rows = np.concatenate([256 * k + np.array([3, 100, 250]) for k in blocks])
    return couple(operator_a(seed), rows, rng.choice(288, len(rows), replace=False), rng)
