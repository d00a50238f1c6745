"""One row shard's cycle on the device, in ONE process, against the exact host restatement tests/shard_ref.py: the test plays every peer.

A hierarchy takes its halo values, its coarsest solve and its reductions from callbacks.  The harness builds a three-level shard with explicit
aggregates (mgs_xfer_from_agg, mgs_galerkin_shard with a test-chosen coarse halo map, mgs_hier_push_level; levels 0 and 1 have halo columns,
level 2 is "solved" by the coarse callback: x_c = fl(0.5·fl(dinv_c·b)) on the host) and installs a SCRIPTED TRANSPORT as the plain, the split
and / or the fused callback.  On every call the transport downloads and logs the owned entries of the vector it is handed (with level, callback
kind, phase, and whether the destination is that vector's own halo room), answers with seeded values from ±[0.5, 2] (positive for the one D⁻¹
exchange per level at setup), and in a two-phase exchange writes NaN into the destination in phase 0 and the values only in phase 1 — a row
block launched as interior that reads a halo column turns its rows into NaN.  shard_ref.cycle then walks the same cycle on the host and
consumes that log in order.

Asserted in every case: x has the restatement's bits (no row of any level is longer than 64: the kernels promise their order); every logged
source vector — D⁻¹, right-hand sides, e_c, the sweeps' x, the coarsest solve's input, the K step's local scalars — has the restated bits,
named by step; the log is exactly the call sequence of the cycle's form (kinds by halo_transport's precedence) and is used up; the guard zones
of b and x are untouched and b is unchanged; every row of x lies within the derived bar of the long-double twin of the pass that wrote it; the
form the case was built for is the one that ran (arm and operand from mgs_hier_fused_info / mgs_hier_group_info under the options: halo-tagged
coded blocks > 0, or groups > 0); the coarse operators of levels 1 and 2 have the restated Galerkin bits.

Operators: (a) planes 3..9 of a 12 × 12 × 14 variable-coefficient nonsymmetric 7-point grid (1008 rows, four row blocks, the last partial,
144 + 144 halo slots read by blocks 0 and 3); (b) poisson3d(16, 4, 12, local_cols=True) (2048 rows, eight exact blocks); (c) operator (a) with
three rows each of blocks 1 AND 2 coupled to halo slots: no interior block is left and the plan reports halo_split_ok = 0; (c1) the same with
rows of block 1 alone — by the plan's rule (halo readers form a prefix and a suffix) that level still splits, with a two-block prefix, so it is
kept as a fourth operator: its block 1 must be launched behind the exchange, its block 2 beside it.  Aggregates on both coarsenings: pairs
along x, rows outside every aggregate (first and last row of a row block among them), halo slots without a coarse column, two slots on one
coarse halo column, more coarse halo columns than are used.

Measured on an MI355X: every comparison of bits held — x, every logged source vector, the K step's five scalars, the Galerkin operators of
levels 1 and 2.  Largest |x − twin| / bar per case, operators (a) / (b) / (c) [/ (c1)], as the tests print it (both levels ran the arm named):
    fused form      gather, operand 0      0.130 / 0.149 / 0.126
                    residual on Â          operand 2: 0.174 / 0.157 / 0.174      operand 1: 0.177 / 0.140 / 0.177
                    aggregate-parallel     operand 2: 0.174 / 0.157 / 0.174      operand 1: 0.177 / 0.140 / 0.177
                    grouped, t-form        operand 2: 0.174 / 0.158 / 0.218      operand 1: 0.141 / 0.136 / 0.197
    split_min_rows=1 (same bits as the default, no NaN)   residual 0.174 / 0.157 / 0.174 / 0.174; gather 0.130 / 0.149 / 0.126 / 0.126;
                    aggregate-parallel 0.174 / 0.157 / 0.174 / 0.174; split callbacks alone, one kernel per step: V(1,1) 0.298 / 0.314 / 0.298 /
                    0.298, V(2,1) 0.255 / 0.302 / 0.243 / 0.244
    plain callback alone, (a) / (b), zero guess | non-zero guess:   V(1,1) 0.298 / 0.314 | 0.270 / 0.252;   V(2,1) 0.255 / 0.302 | 0.264 / 0.270;
                    V(0,2) 0.326 / 0.293 | 0.224 / 0.311;   V(3,2) 0.248 / 0.264 | 0.242 / 0.277
    K step on level 1, (a) / (b):   GCR form 0.158 / 0.168;   energy form 0.161 / 0.137
    σ = 1.1, (a) / (b):   0.163 / 0.142
    every callback installed, (a) / (b):   zero guess 0.174 / 0.157;   non-zero guess 0.287 / 0.285
The largest ratio of an intermediate pass of the fused cases (pre passes, post pass of level 1) was 0.221.
Call sequences (kind, level; every two-phase exchange is a phase-0 call followed by a phase-1 call):
    fused V(1,1), fused callback alone   D⁻¹ 0, D⁻¹ 1 (in place) | b of 0, b of 1 into the payload buffers | coarsest solve | e_c of 2, e_c of 1
                                         (in place): 13 calls, FUSED_V11 below; the same with split_min_rows=1 and with σ = 1.1
    plain callback alone                 V(ν1,ν2) from zero: per level max(ν1 − 1, 0) + (1 unless ν1 = 0) + ν2 calls, level 0 from a guess ν1 + 1 + ν2,
                                         and the coarsest solve: 5 | 6 calls for V(1,1), 7 | 8 for V(2,1), 5 | 6 for V(0,2), 11 | 12 for V(3,2)
    split callbacks alone                begin → end per exchange: 9 calls for V(1,1), 13 for V(2,1)
    K step (split + fused)               D⁻¹ through begin/end; per inner cycle the fused calls of level 1, then c's halo through begin/end; three
                                         reductions of 2, 1 and 2 scalars; two coarsest solves
    every callback, zero guess           plain, plain (D⁻¹) then the fused calls; non-zero guess: plain ×2 | level 1's fused calls | plain, and with
                                         split_min_rows=1 begin → end in the place of each plain call"""
import ctypes as C

import numpy as np
import pytest

import post_pass_ref as Q
import shard_ref as R

pytestmark = pytest.mark.gpu

DEFAULTS = dict(fuse_operands=1, merge_ap=1, aggpre_max_rows=300000, fuse_restrict=1, group_min_blocks=1024, group_stray_pct=6, split_min_rows=400000,
                kcycle_energy=0)
GROUPING = dict(group_min_blocks=1, group_stray_pct=60, split_min_rows=100000000)      # as test_grouped_pre_pass_on_row_shards forces it
ARM_OPTIONS = {"agg": {}, "residual": dict(aggpre_max_rows=0, fuse_restrict=0), "gather": dict(fuse_operands=0), "grouped": GROUPING}
OPERATORS = {"a": R.operator_a, "b": R.operator_b, "c": R.operator_c, "c1": lambda: R.operator_c((1,))}
SEED_LEVELS, SEED_B, SEED_PEERS = 5, 6, 7


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


def int_ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


class Transport:
    """the scripted peers: log, seeded answers, NaN until phase 1"""

    def __init__(self, ctx, mg, shapes, seed, dinv_levels):
        self.ctx, self.mg, self.shapes = ctx, mg, shapes
        self.rng = np.random.default_rng(seed)
        self.log, self.errors, self.pending = [], [], {}
        self.dinv_levels = list(dinv_levels)      # the setup exchanges still to come, in order: their answers are positive

    def guarded(self, fn):
        def wrapped(*args):
            try:
                return fn(*args)
            except BaseException as e:  # noqa: BLE001  (kept for the test; the library sees a failed callback)
                self.errors.append(e)
                raise
        return wrapped

    def serve(self, level, kind, phase, src_ptr, dst_ptr):
        n, nh = self.shapes[level]
        wrap = self.mg.Vec.wrap
        src = wrap(self.ctx, src_ptr, n).numpy()                    # waits for the stream: what the library handed over
        e = dict(kind=kind, level=level, phase=phase, in_place=dst_ptr == src_ptr + 8 * n, src=src)
        dst = wrap(self.ctx, dst_ptr, nh)
        if phase == 0:
            ans = Q.signed(self.rng, nh)
            if self.dinv_levels and self.dinv_levels[0] == level and e["in_place"]:
                self.dinv_levels.pop(0); ans = np.abs(ans)
            e["answer"] = ans
            if kind == "plain":
                dst.upload(ans)
            else:
                assert (level, dst_ptr) not in self.pending
                self.pending[(level, dst_ptr)] = ans
                dst.upload(np.full(nh, np.nan))
        else:
            dst.upload(self.pending.pop((level, dst_ptr)))         # behind everything launched since phase 0
        self.log.append(e)

    def install(self, h, installed):
        if "plain" in installed:
            h.set_halo_exchange(self.guarded(lambda level, p: self.serve(level, "plain", 0, p, p + 8 * self.shapes[level][0])))
        if "split" in installed:
            h.set_halo_exchange_split(self.guarded(lambda level, p: self.serve(level, "begin", 0, p, p + 8 * self.shapes[level][0])),
                                      self.guarded(lambda level, p: self.serve(level, "end", 1, p, p + 8 * self.shapes[level][0])))
        if "fused" in installed:
            def fused(level, kind, a, b, out, phase):
                assert kind == 2 and not b
                self.serve(level, "fused", phase, a, out)
            h.set_halo_exchange_fused(self.guarded(fused))

    def coarse_solver(self, h, L):
        def cb(_u, b_ptr, x_ptr):
            try:
                b = self.mg.Vec.wrap(self.ctx, b_ptr, L.n).numpy()
                self.log.append(dict(kind="coarse", src=b))
                self.mg.Vec.wrap(self.ctx, x_ptr, L.n).upload(R.coarsest_solve(L, b))
                return 0
            except BaseException as e:  # noqa: BLE001
                self.errors.append(e)
                return 1
        from multigridsolver_amd._lib import COARSE_FN
        self._coarse = COARSE_FN(cb)
        assert self.mg.lib().mgs_hier_set_coarse_solver(h.h, self._coarse, None) == 0

    def allreduce(self, a):
        part = a * self.rng.uniform(0.5, 2.0, len(a))              # the peers' parts: logged, then added
        self.log.append(dict(kind="allreduce", count=len(a), src=a.copy(), answer=part))
        a[:] = a + part


def build(ctx, mg, name, levels):
    """the device hierarchy of `levels` with explicit aggregates; the coarse operators must come out with the restated bits"""
    lib = mg.lib()
    L0 = levels[0]
    if name == "b":
        A = ctx.poisson3d(16, 4, 12, local_cols=True)
        rp, ci, v = A.download()
        assert A.shape == L0.A.shape and np.array_equal(rp, L0.A.indptr) and np.array_equal(ci, L0.A.indices) and R.same_bits(v, L0.A.data)
    else:
        A = ctx.csr(L0.n, L0.n + L0.nh, L0.A.indptr, L0.A.indices, L0.A.data)
    h = mg.Hierarchy(A, R.OMEGA, 1, 1)      # (keeps A referenced)
    for l, L in enumerate(levels[:-1]):
        T, Ac = C.c_void_p(), C.c_void_p()
        agg = np.ascontiguousarray(L.agg, dtype=np.int32); hm = np.ascontiguousarray(L.halo_cmap, dtype=np.int32)
        assert lib.mgs_xfer_from_agg(ctx.h, L.n, L.nc, int_ptr(agg), C.byref(T)) == 0
        assert lib.mgs_galerkin_shard(h.level_A(l).h, T, int_ptr(hm), L.nhc, C.byref(Ac)) == 0, lib.mgs_last_error(ctx.h)
        assert lib.mgs_hier_push_level(h.h, T, Ac) == 0, lib.mgs_last_error(ctx.h)      # ownership of both moves into the hierarchy
        M, want = h.level_A(l + 1), levels[l + 1].A
        rp, ci, v = M.download()
        assert M.shape == want.shape and np.array_equal(rp, want.indptr) and np.array_equal(ci, want.indices), f"pattern of the level-{l + 1} operator"
        assert R.same_bits(v, want.data), f"Galerkin values of level {l + 1}"
    return h


def forms_of(ctx, h, levels, opts):
    """arm, post operand and split of every level under the options, from the library's own report (level_fused_operands / level_pre_arm restated)"""
    out = {}
    for l, L in enumerate(levels[:-1]):
        fi, gi, plan = h.fused_info(l), h.group_info(l), h.level_A(l).plan_info()
        operands = bool(opts["fuse_operands"] and fi["has_val_wd"] and fi["has_col_agg"] and fi["coded_col_halo"] > 0)
        grouped = bool(opts["fuse_restrict"] and operands and gi["groups"] > 0)
        split = bool(plan["halo_split_ok"] and L.n >= opts["split_min_rows"])
        arm = R.pre_arm(opts["fuse_operands"], fi["has_val_wd"], operands, grouped, split, L.n, plan["max_row_len"], opts["aggpre_max_rows"])
        out[l] = dict(arm=arm, post=0 if not operands else (2 if opts["merge_ap"] else 1), split=split, info=(fi, gi, plan))
    return out


def run_case(ctx, mg, name, options=None, installed=("fused",), nu=(1, 1), sigma=1.0, kcycle=0, guesses=(False,), seed=SEED_PEERS):
    """build, cycle on the device with the scripted transport, restate from its log; returns one dict per cycle (one cycle per guess)"""
    opts = dict(DEFAULTS, **(options or {}))
    levels = R.three_levels(OPERATORS[name](), SEED_LEVELS)
    n, nh = levels[0].n, levels[0].nh
    rng = np.random.default_rng(SEED_B)
    b_np = Q.signed(rng, n)
    out = []
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        h = build(ctx, mg, name, levels)
        h.set_smoother(R.OMEGA, *nu)
        if sigma != 1.0:
            h.set_correction_scale(sigma)
        cfg = R.Config(installed=installed, nu=nu, sigma=sigma, kcycle=kcycle, energy=bool(opts["kcycle_energy"]), allreduce=kcycle > 0)
        tr = Transport(ctx, mg, [(L.n, L.nh) for L in levels], seed, [0, 1] if cfg.fuses() else [])
        tr.install(h, installed)
        tr.coarse_solver(h, levels[-1])
        if kcycle:
            ctx.set_allreduce(tr.allreduce)
            h.set_kcycle(kcycle)
        for i, guess in enumerate(guesses):
            bg, xg = Q.Guarded(ctx, mg, n), Q.Guarded(ctx, mg, n + nh)
            bg.v.upload(b_np)
            x0 = Q.signed(rng, n) if guess else None
            if guess:
                xg.v.upload(x0)
            tr.log = []
            try:
                h.vcycle(bg.v, xg.v, zero_guess=not guess)
                ctx.sync()
            except Exception:
                if tr.errors:
                    raise tr.errors[0]
                raise
            assert not tr.errors and not tr.pending
            xfull = xg.check(f"{name}: guard zones of x")
            x = xfull[:n]
            assert R.same_bits(bg.check(f"{name}: guard zones of b"), b_np), "b was written"
            cfg.forms = forms_of(ctx, h, levels, opts)
            xr, run = R.cycle(levels, tr.log, b_np, x0, cfg=cfg, first=i == 0)
            scal = h.kcycle_scalars(1) if kcycle else None
            out.append(dict(x=x, xr=xr, run=run, log=tr.log, forms=cfg.forms, scalars=scal, levels=levels, h=h, xhalo=xfull[n:]))
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)
    return out


def check(res, what):
    """the assertions every case makes; returns the largest error/bar ratio of x against the long-double twin"""
    x, xr, run = res["x"], res["xr"], res["run"]
    assert np.isfinite(x).all(), f"{what}: {int((~np.isfinite(x)).sum())} rows of x are not finite (a halo value read before its exchange completed)"
    assert not run.mismatch, f"{what}: logged source vectors differ from the restatement: {run.mismatch}"
    bad = np.flatnonzero(R.bits(x) != R.bits(xr))
    assert len(bad) == 0, f"{what}: {len(bad)} rows of x differ from the restatement, first {bad[:5]}: {x[bad[:5]]} against {xr[bad[:5]]}; forms {[(f['arm'], f['post'], f['split']) for f in res['forms'].values()]}"
    q = Q.ratios(x, *run.last)
    assert q.max() <= 1.0 and max(run.ratio.values()) <= 1.0, (what, q.max(), run.ratio)
    return float(q.max())


def fused_calls(level, in_place):
    return [("fused", level, phase, in_place) for phase in (0, 1)]


FUSED_V11 = (fused_calls(0, True) + fused_calls(1, True) +                      # setup: D⁻¹ of levels 0 and 1, in place
             fused_calls(0, False) + fused_calls(1, False) +                    # right-hand sides into the payload buffers
             [("coarse", None, None, None)] + fused_calls(2, True) + fused_calls(1, True))      # coarsest solve; e_c of levels 2 and 1 into their own halo room


# ------------------------------------------------------------------ 1. the fused form, one case per pre arm and post operand
@pytest.mark.parametrize("arm,post", [(a, p) for a in R.ARMS for p in ((0,) if a == "gather" else (2, 1))])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fused_form_per_arm_and_operand(ctx, mg, name, arm, post):
    options = dict(ARM_OPTIONS[arm], merge_ap=1 if post == 2 else 0)
    res = run_case(ctx, mg, name, options)[0]
    f0, f1 = res["forms"][0], res["forms"][1]
    fi, gi, _ = f0["info"]
    assert (f0["arm"], f0["post"]) == (arm, post), f"level 0 runs {f0['arm']} / operand {f0['post']}: {fi} {gi}"
    if arm == "grouped":
        assert gi["groups"] > 0
    elif arm != "gather":
        assert fi["coded_col_halo"] > 0 and fi["has_val_wd"] and fi["has_col_agg"]
    else:
        assert not fi["has_val_wd"]
    assert res["run"].calls == FUSED_V11, res["run"].calls
    assert np.all(res["xhalo"] == Q.SENT), "the fused form wrote into x's halo room: no exchange of x belongs to it"
    q = check(res, f"({name}) {arm} / operand {post}")
    print(f"({name}) level 0 {arm}/{post}, level 1 {f1['arm']}/{f1['post']}: largest |x - twin| / bar = {q:.3f}; per step {({k: round(v, 3) for k, v in res['run'].ratio.items()})}")


# ------------------------------------------------------------------ 2. interior / boundary split against the default
@pytest.mark.parametrize("arm", ["residual", "gather", "agg"])
@pytest.mark.parametrize("name", ["a", "b", "c", "c1"])
def test_split_launches_have_the_default_bits(ctx, mg, name, arm):
    base = run_case(ctx, mg, name, ARM_OPTIONS[arm])[0]
    split = run_case(ctx, mg, name, dict(ARM_OPTIONS[arm], split_min_rows=1))[0]
    plan = split["forms"][0]["info"][2]
    want = {"a": (1, 1, 1), "b": (1, 1, 1), "c": (4, 0, 0), "c1": (2, 1, 1)}[name]
    assert (plan["halo_lo_blocks"], plan["halo_hi_blocks"], plan["halo_split_ok"]) == want, plan
    assert split["forms"][0]["split"] == (name != "c") and not base["forms"][0]["split"]
    assert split["forms"][0]["arm"] == arm and base["forms"][0]["arm"] == arm
    q = check(split, f"({name}) {arm}, split_min_rows=1")
    check(base, f"({name}) {arm}")
    assert R.same_bits(split["x"], base["x"]), "the split launches change bits of x"
    assert split["run"].calls == base["run"].calls == FUSED_V11      # begin → end around the interior launch: the same calls, NaN in between
    print(f"({name}) {arm} split: largest |x - twin| / bar = {q:.3f}")


@pytest.mark.parametrize("nu", [(1, 1), (2, 1)])
@pytest.mark.parametrize("name", ["a", "b", "c", "c1"])
def test_split_callbacks_one_kernel_per_step(ctx, mg, name, nu):
    base = run_case(ctx, mg, name, None, installed=("split",), nu=nu)[0]
    split = run_case(ctx, mg, name, dict(split_min_rows=1), installed=("split",), nu=nu)[0]
    assert split["forms"][0]["split"] == (name != "c")
    q = check(split, f"({name}) V{nu} through the split callbacks, split_min_rows=1")
    check(base, f"({name}) V{nu} through the split callbacks")
    assert R.same_bits(split["x"], base["x"])
    calls = split["run"].calls
    assert calls == base["run"].calls and all(c[0] in ("begin", "end", "coarse") for c in calls)
    halo = [c for c in calls if c[0] != "coarse"]
    assert all(a[0] == "begin" and b[0] == "end" and a[1] == b[1] for a, b in zip(halo[0::2], halo[1::2]))
    print(f"({name}) V{nu} split callbacks: largest |x - twin| / bar = {q:.3f}; calls {len(calls)}")


# ------------------------------------------------------------------ 3. no fused callback: one kernel per step
@pytest.mark.parametrize("nu", [(1, 1), (2, 1), (0, 2), (3, 2)])
@pytest.mark.parametrize("name", ["a", "b"])
def test_unfused_sweep_counts_zero_and_nonzero_guess(ctx, mg, name, nu):
    zero, guess = run_case(ctx, mg, name, None, installed=("plain",), nu=nu, guesses=(False, True))
    for res, what in ((zero, "zero guess"), (guess, "non-zero guess")):
        q = check(res, f"({name}) V{nu} {what}")
        calls = res["run"].calls
        assert all(c[0] in ("plain", "coarse") and (c[0] == "coarse" or c[3]) for c in calls)
        nz = what == "zero guess"
        per_level = lambda z: nu[1] + (0 if nu[0] == 0 and z else 1) + (max(nu[0] - 1, 0) if z else nu[0])      # noqa: E731  sweeps + residual
        assert len(calls) == 1 + per_level(nz) + per_level(True), (what, calls)      # level 1 always starts from zero
        print(f"({name}) V{nu} {what}: largest |x - twin| / bar = {q:.3f}; {len(calls)} calls")
    assert not R.same_bits(zero["x"], guess["x"])


# ------------------------------------------------------------------ 4. K step on level 1
@pytest.mark.parametrize("energy", [0, 1])
@pytest.mark.parametrize("name", ["a", "b"])
def test_k_step_on_level_1_with_peer_parts(mg, name, energy):
    c = mg.Context(0)      # a context of its own: the all-reduce callback stays with it
    try:
        res = run_case(c, mg, name, dict(kcycle_energy=energy), installed=("split", "fused"), kcycle=1)[0]
        q = check(res, f"({name}) K step, energy={energy}")
        want, got = res["run"].scalars[1], res["scalars"]
        assert R.same_bits(got, want), f"K-step scalars [rho1, alpha1, gamma, rho2, alpha2]: device {got}, restated {want}"
        kinds = [k[0] for k in res["run"].calls]
        assert kinds.count("allreduce") == 3 and kinds.count("coarse") == 2 and kinds.count("begin") == 4      # D⁻¹ of two levels, c1, c2
        assert [e["count"] for e in res["log"] if e["kind"] == "allreduce"] == [2, 1, 2]
        print(f"({name}) K step energy={energy}: largest |x - twin| / bar = {q:.3f}; scalars {got}")
    finally:
        for k, v in DEFAULTS.items():
            c.set_option(k, v)
        c.close()


# ------------------------------------------------------------------ 5. over-correction: e_c is scaled before its halo is exchanged
@pytest.mark.parametrize("name", ["a", "b"])
def test_correction_scale(ctx, mg, name):
    res = run_case(ctx, mg, name, None, sigma=1.1)[0]
    plain = run_case(ctx, mg, name, None)[0]
    q = check(res, f"({name}) sigma = 1.1")
    assert res["run"].calls == FUSED_V11 and not R.same_bits(res["x"], plain["x"])
    ec2 = [e for e in res["log"] if e["kind"] == "fused" and e["level"] == 2 and e["phase"] == 0][0]["src"]
    ec2_plain = [e for e in plain["log"] if e["kind"] == "fused" and e["level"] == 2 and e["phase"] == 0][0]["src"]
    assert R.same_bits(ec2, 1.1 * ec2_plain)
    print(f"({name}) sigma=1.1: largest |x - twin| / bar = {q:.3f}")


# ------------------------------------------------------------------ 6. halo_transport's precedence with every callback installed
@pytest.mark.parametrize("name", ["a", "b"])
def test_transport_precedence_with_every_callback_installed(ctx, mg, name):
    """plain, split and fused callbacks together: the setup exchange and an in-place exchange with nothing to overlap take the plain callback, one
    with interior blocks to launch the split pair, the fused passes their own — from a zero guess (fused) and a non-zero one (level 0 unfused)"""
    every = ("plain", "split", "fused")
    base = run_case(ctx, mg, name, None, installed=every, guesses=(False, True))
    split = run_case(ctx, mg, name, dict(split_min_rows=1), installed=every, guesses=(False, True))
    kinds = lambda res: [c[0] for c in res["run"].calls]      # noqa: E731
    for rb, rs, what in zip(base, split, ("zero guess", "non-zero guess")):
        q = check(rs, f"({name}) every callback, split_min_rows=1, {what}")
        check(rb, f"({name}) every callback, {what}")
        assert R.same_bits(rb["x"], rs["x"])
        print(f"({name}) every callback, {what}: largest |x - twin| / bar = {q:.3f}; default {kinds(rb)}; split {kinds(rs)}")
    fused_part = ["fused"] * 4 + ["coarse"] + ["fused"] * 4
    assert kinds(base[0]) == kinds(split[0]) == ["plain", "plain"] + fused_part                       # D⁻¹ of both levels: in place, nothing to overlap
    level1 = ["fused"] * 2 + ["coarse"] + ["fused"] * 2                                               # level 1 from zero: fused
    assert kinds(base[1]) == ["plain"] * 2 + level1 + ["plain"]                                       # pre-sweep, residual | post-sweep
    assert kinds(split[1]) == ["begin", "end"] * 2 + level1 + ["begin", "end"]
