"""tests/shard_ref.py — the host restatement of a row shard's cycle — checked without a GPU.

Anchor.  A global variable-coefficient 7-point operator on 12 × 12 × 9 points, one pairwise aggregation that straddles no shard (rows outside
every aggregate included) and the elementwise coarsest "solve" x_c = fl(0.5·fl(dinv_c·r_c)).  The operator is cut into three shards of three
planes; every shard gets its true neighbours' values (D⁻¹, b, e_c) through shard_ref.Peers and runs shard_ref's FP64 two-level cycle in every arm
of the pre pass against every operand of the post pass.  Assembled over the shards, x must agree with the LONG-DOUBLE restatement of the unsharded
cycle (pre_pass_ref.evaluate, post_pass_ref.evaluate on the whole operator) within a bound derived from the existing bars, to first order:
    post_pass_ref.bar of the row (extra = the longest merged run where the shard reads the merged operand: its values are rounded sums)
  + d_i·bar_r_i (bar_t_i behind the grouped arm)                                   the error carried in r (pre_pass_ref.bars)
  + δe_c[agg_i] + d_i·Σ_k |a_ik|·δe_c[c_ik]                                        the error carried in e_c, with
    δe_c[a] = 0.5·dinv_c[a]·bar_rc[a] + 3u·|e_c[a]|                                (two products of the solve, and the twin's own dinv_c in FP64)
The payload and the delivered D⁻¹ are copies, so they carry nothing.  Measured: the largest |x − twin| / bound over all rows, arms and operands
is 0.055 (printed by the test, per arm and operand); the bound is first order and holds with that room.

Defects.  Each of four planted mistakes — halo slots scaled by an owned row's wd, a halo slot on the wrong coarse column, payload and e_c halo
swapped, every row's diagonal summed first — changes the bits of x on the fixtures the GPU test uses, in every form it touches: the comparison
of tests/test_gpu_shard_cycle.py can fail.  The driver's own checks (call sequence, source vectors, an unused or missing log entry) are shown to
fire as well."""
import numpy as np
import pytest

import galerkin_ref as G
import post_pass_ref as Q
import pre_pass_ref as P
import shard_ref as R

LD = np.longdouble
FORMS = [(arm, post) for arm in R.ARMS for post in ((0,) if arm == "gather" else (1, 2))]


# ------------------------------------------------------------------ the anchor
@pytest.fixture(scope="module")
def world():
    nx = ny = 12; nz = 9; planes = 3
    Gm = R.vc7(nx, ny, nz, seed=3)
    n = Gm.shape[0]
    rng = np.random.default_rng(4)
    agg = np.arange(n) // 2                                           # pairs along x: no pair crosses a plane
    agg[rng.choice(n, 40, replace=False)] = -1
    agg = P.renumber_by_first_member(agg)
    nc = int(agg.max()) + 1
    b = Q.signed(rng, n)
    bounds = [(p * planes * nx * ny, (p + 1) * planes * nx * ny) for p in range(nz // planes)]
    shards = []
    for r0, r1 in bounds:
        A, hrows = R.cut(Gm, r0, r1)
        own = agg[r0:r1]
        c0 = int(own[own >= 0].min())
        loc = np.where(own >= 0, own - c0, -1)
        ncl = int(loc.max()) + 1
        assert np.array_equal(np.unique(loc[loc >= 0]), np.arange(ncl))               # the shard's aggregates are a contiguous id range
        need = np.unique(agg[hrows][agg[hrows] >= 0])
        hm = np.where(agg[hrows] >= 0, ncl + np.searchsorted(need, agg[hrows]), -1)
        shards.append(dict(r0=r0, r1=r1, c0=c0, hrows=hrows, need=need, levels=R.hierarchy(A, R.OMEGA, [(loc, ncl, hm, len(need))])))
    return dict(G=Gm, agg=agg, nc=nc, b=b, shards=shards)


def test_cut_and_the_shard_galerkin_product_are_rows_of_the_global_ones(world):
    Gm, agg, nc = world["G"], world["agg"], world["nc"]
    Ac = G.galerkin_restated(Gm.indptr, Gm.indices, Gm.data, agg, nc)
    for s in world["shards"]:
        L0, L1 = s["levels"]
        n = s["r1"] - s["r0"]
        gcol = np.r_[np.arange(s["r0"], s["r1"]), s["hrows"]]
        back = Q.sps.csr_matrix((L0.A.data, gcol[L0.A.indices], L0.A.indptr), shape=(n, Gm.shape[0]))
        assert (back != Gm[s["r0"]:s["r1"]]).nnz == 0
        assert np.all(np.diff(s["hrows"]) > 0) and L0.A.has_sorted_indices
        owned_first = np.all(L0.A.indices[L0.A.indices < n] == gcol[L0.A.indices[L0.A.indices < n]] - s["r0"])
        assert owned_first
        # coarse operator: the global product's rows, bit for bit (no coarse column mixes owned and halo entries)
        ccol = np.r_[s["c0"] + np.arange(L1.n), s["need"]]
        rows = Ac[s["c0"]:s["c0"] + L1.n].tocsr(); rows.sort_indices()
        mine = Q.sps.csr_matrix((L1.A.data, ccol[L1.A.indices], L1.A.indptr), shape=rows.shape); mine.sort_indices()
        assert np.array_equal(mine.indptr, rows.indptr) and np.array_equal(mine.indices, rows.indices)
        assert R.same_bits(mine.data, rows.data)


def run_world(world, arm, post):
    """the assembled FP64 x of the three shards; every shard is recorded and replayed through the driver"""
    Gm, agg, nc, b = world["G"], world["agg"], world["nc"], world["b"]
    dinv_g = 1.0 / Gm.diagonal()
    cfg = R.Config(forms={0: dict(arm=arm, post=post, split=False)})
    ec_g = np.zeros(nc)
    for rnd in range(2):                    # round 0 finds every shard's own e_c (its halo plays no part in that), round 1 hands them round
        x = np.zeros(Gm.shape[0])
        for s in world["shards"]:
            def answer(level, what, src, s=s):
                if what.startswith("D^-1"):
                    return dinv_g[s["hrows"]]
                if what.startswith("right-hand side"):
                    return b[s["hrows"]]
                assert what.startswith("e_c of level 1") and level == 1
                ec_g[s["c0"]:s["c0"] + len(src)] = src
                return ec_g[s["need"]]
            bl = b[s["r0"]:s["r1"]]
            log = R.Peers(answer).record(s["levels"], cfg, bl)
            xs, run = R.cycle(s["levels"], log, bl, cfg=cfg)
            assert not run.mismatch and max(run.ratio.values()) <= 1.0, (run.mismatch, run.ratio)
            x[s["r0"]:s["r1"]] = xs
    return x


def twin_and_bound(world, arm, post):
    Gm, agg, nc, b = world["G"], world["agg"], world["nc"], world["b"]
    form = "wd" if arm == "gather" else "hat"
    t, r, rc = P.evaluate(Gm, R.OMEGA, agg, nc, b, LD, form)
    bt, br, brc = P.bars(Gm, R.OMEGA, agg, nc, b, form)
    Ac = G.galerkin_restated(Gm.indptr, Gm.indices, Gm.data, agg, nc)
    dinv_c = 1.0 / Ac.diagonal()
    ec = LD(0.5) * (dinv_c.astype(LD) * rc)
    c = Q.Case(Gm, agg, R.OMEGA)
    bvec, xin, bcarry = (t, None, bt) if arm == "grouped" else (r, b, br)
    x = Q.evaluate(c.mapped, c.d, agg, ec, bvec, xin, LD)
    dec = LD(0.5) * np.abs(dinv_c.astype(LD)) * brc + 3 * LD(Q.U) * np.abs(ec)
    d = np.abs(c.d.astype(LD))
    own = Q.bar(c.mapped, c.d, agg, ec, bvec, xin, extra=c.longest_run if post == 2 else 0, S=Q.abs_sums(c.mapped, ec))
    return x, own + d * bcarry + Q.pe_of(agg, dec, LD) + d * Q.abs_sums(c.mapped, dec)


@pytest.mark.parametrize("arm,post", FORMS)
def test_anchor_three_shards_against_the_unsharded_long_double_cycle(world, arm, post):
    x = run_world(world, arm, post)
    ref, bound = twin_and_bound(world, arm, post)
    q = Q.ratios(x, ref, bound)
    print(f"anchor {arm} / operand {post}: largest |x - twin| / bound = {q.max():.3f}")
    assert q.max() <= 1.0, (arm, post, q.max(), int(q.argmax()))
    assert np.abs(x).min() > 0 and q.max() > 1e-4              # a comparison of something with something


def test_the_anchor_tells_the_arms_apart(world):
    """gather against residual (two roundings per product), t-form against (r, b)-form, merged against mapped: different bits of x"""
    xs = {f: run_world(world, *f) for f in (("gather", 0), ("residual", 1), ("residual", 2), ("grouped", 1), ("agg", 1))}
    assert not R.same_bits(xs["gather", 0], xs["residual", 1])
    assert not R.same_bits(xs["residual", 1], xs["grouped", 1])
    assert not R.same_bits(xs["residual", 1], xs["residual", 2])
    assert R.same_bits(xs["residual", 1], xs["agg", 1])                      # the aggregate-parallel arm promises the residual arm's bits


# ------------------------------------------------------------------ the GPU test's fixtures: defects, driver
def random_peers(seed):
    rng = np.random.default_rng(seed)
    return R.Peers(lambda level, what, src: (np.abs if what.startswith("D^-1") else (lambda v: v))(Q.signed(rng, NH[level])),
                   lambda what, vals: vals * rng.uniform(0.5, 2.0, len(vals)))


NH = {}


@pytest.fixture(scope="module", params=["a", "b", "c"])
def shard(request):
    A = {"a": R.operator_a, "b": R.operator_b, "c": R.operator_c}[request.param]()
    levels = R.three_levels(A, seed=5)
    NH.clear(); NH.update({l: L.nh for l, L in enumerate(levels)})
    b = Q.signed(np.random.default_rng(6), levels[0].n)
    return request.param, levels, b


def forms_cfg(arm, post, **kw):
    return R.Config(forms={0: dict(arm=arm, post=post, split=False), 1: dict(arm=arm, post=post, split=False)}, **kw)


@pytest.mark.parametrize("arm,post", FORMS)
def test_planted_defects_change_the_bits(shard, arm, post):
    name, levels, b = shard
    cfg = forms_cfg(arm, post)
    log = random_peers(7).record(levels, cfg, b)
    x, run = R.cycle(levels, log, b, cfg=cfg)
    assert not run.mismatch and max(run.ratio.values()) <= 1.0, run.ratio
    L0 = levels[0]
    wrong = L0.cmap_ext.copy()
    slot = L0.n + int(np.flatnonzero(L0.halo_cmap >= 0)[0])
    wrong[slot] = wrong[slot] + 1 if wrong[slot] + 1 < L0.nc + L0.nhc else wrong[slot] - 1
    planted = dict(owned_wd=dict(defects={0: dict(wd_slot=np.arange(L0.nh) % L0.n)}), wrong_coarse_column=dict(defects={0: dict(cmap_ext=wrong)}),
                   swapped=dict(swap=True), diagonal_first=dict(defects={0: dict(diag_first=True)}))
    for what, kw in planted.items():
        fresh = R.three_levels(L0.A if what != "diagonal_first" else L0.A.copy(), seed=5)
        xd, rd = R.cycle(fresh, log, b, cfg=cfg, twin=False, **kw)
        nbad = int((R.bits(xd) != R.bits(x)).sum())
        assert nbad > 0, (name, what)
        if what in ("owned_wd", "swapped", "diagonal_first"):      # these reach the pre pass: the coarse right-hand side differs as well
            assert any(m[0].startswith("right-hand side of the coarsest") or m[0].startswith("right-hand side of level 1") for m in rd.mismatch), (what, rd.mismatch)


CYCLES = [dict(installed=("plain",), nu=nu) for nu in ((1, 1), (2, 1), (0, 2), (3, 2))] + [
    dict(installed=("split",), nu=(2, 1)), dict(installed=("split", "fused"), kcycle=1, allreduce=True),
    dict(installed=("plain", "fused"), kcycle=1, allreduce=True, energy=True), dict(installed=("fused",), sigma=1.1)]


@pytest.mark.parametrize("kw", CYCLES, ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
@pytest.mark.parametrize("guess", [False, True])
def test_driver_replays_its_own_log_and_names_what_differs(shard, kw, guess):
    name, levels, b = shard
    if name == "c":
        return
    cfg = forms_cfg("agg", 2, **kw)
    x0 = Q.signed(np.random.default_rng(9), levels[0].n) if guess else None
    log = random_peers(10).record(levels, cfg, b, x0)
    x, run = R.cycle(levels, log, b, x0, cfg=cfg)
    assert not run.mismatch and np.isfinite(x).all() and max(run.ratio.values()) <= 1.0, (run.mismatch, run.ratio)
    assert run.last is not None and Q.ratios(x, *run.last).max() <= 1.0
    kinds = [e["kind"] for e in log]
    assert kinds.count("coarse") == (2 if kw.get("kcycle") else 1)
    assert kinds.count("allreduce") == (3 if kw.get("kcycle") else 0)
    if kw.get("kcycle"):
        assert len(run.scalars[1]) == 5 and run.scalars[1][0] != 0
    # the callback kinds follow halo_transport's precedence
    inst = set(kw["installed"])
    for e in log:
        if e["kind"] in ("plain", "begin", "end"):
            assert e["in_place"] and (e["kind"] == "plain") == ("plain" in inst)
        if e["kind"] == "fused" and inst & {"plain", "split"} and e["in_place"]:
            assert e["level"] >= 1                                   # e_c's halo: an exchange of the fused passes goes to the fused callback
    # a vector that differs is named; a log that is too long or too short fails
    k = next(i for i, e in enumerate(log) if e["kind"] not in ("allreduce",) and len(e["src"]) > 3)
    bent = [dict(e) for e in log]; bent[k]["src"] = bent[k]["src"].copy(); bent[k]["src"][3] = np.nextafter(bent[k]["src"][3], np.inf)
    _, r2 = R.cycle(levels, bent, b, x0, cfg=cfg, twin=False)
    assert len(r2.mismatch) == 1 and r2.mismatch[0][1] == 1 and r2.mismatch[0][2] == [3], r2.mismatch
    with pytest.raises(AssertionError, match="not used"):
        R.cycle(levels, log + [log[-1]], b, x0, cfg=cfg, twin=False)
    with pytest.raises(AssertionError, match="the log ends|asks for"):
        R.cycle(levels, log[:-1], b, x0, cfg=cfg, twin=False)
    with pytest.raises(AssertionError, match="asks for"):
        other = ({"plain", "split"} - inst) | (inst & {"fused"}) if inst & {"plain", "split"} else {"plain", "fused"}      # another transport: other callback kinds
        R.cycle(levels, log, b, x0, cfg=forms_cfg("agg", 2, **dict(kw, installed=tuple(other), allreduce=True)), twin=False)


def test_transport_precedence_and_pre_arm_tables():
    T = R.transport
    all3 = {"plain", "split", "fused"}
    assert T(all3, True, False, False) == "plain" and T(all3, True, False, True) == "split"        # interior blocks to launch: the split pair first
    assert T(all3, True, True, True) == "fused" and T(all3, False, True, False) == "fused"        # the fused passes ask their own callback
    assert T({"split", "fused"}, True, False, False) == "split"                                   # no plain callback
    assert T({"fused"}, True, False, False) == "fused" and T({"plain"}, False, True, False) is None
    assert T({"plain", "split"}, True, True, False) == "plain" and T(set(), True, False, False) is None
    arm = R.pre_arm
    assert arm(1, 1, True, True, False, 1000, 7, 300000) == "grouped" and arm(1, 1, True, True, True, 1000, 7, 300000) == "agg"
    assert arm(1, 1, True, False, False, 1000, 7, 0) == "residual" and arm(0, 0, False, False, False, 1000, 7, 300000) == "gather"
    assert arm(1, 1, False, False, False, 1000, 65, 300000) == "gather"


def test_fixture_plans():
    """operator (a): halo readers in row blocks 0 and 3; (b): eight exact blocks; a few rows of block 1 alone make a two-block prefix, which the
    plan still splits (halo_split_ok = 1); rows of blocks 1 AND 2 leave no interior block: halo_split_ok = 0"""
    import spmv_ref as S
    pa, pb = S.plan_of(R.operator_a()), S.plan_of(R.operator_b())
    assert (pa["nblocks"], pa["halo_lo_blocks"], pa["halo_hi_blocks"], pa["halo_split_ok"]) == (4, 1, 1, 1) and R.operator_a().shape == (1008, 1296)
    assert (pb["nblocks"], pb["halo_lo_blocks"], pb["halo_hi_blocks"], pb["halo_split_ok"]) == (8, 1, 1, 1) and R.operator_b().shape == (2048, 2560)
    p1, pc = S.plan_of(R.operator_c((1,))), S.plan_of(R.operator_c())
    assert (p1["halo_lo_blocks"], p1["halo_hi_blocks"], p1["halo_split_ok"]) == (2, 1, 1)
    assert pc["halo_split_ok"] == 0 and R.operator_c().shape == (1008, 1296)
    for A in (R.operator_a(), R.operator_b(), R.operator_c()):
        lv = R.three_levels(A, 5)
        assert all(np.diff(L.A.indptr).max() <= 64 for L in lv) and all(L.nh > 0 for L in lv)
        L0 = lv[0]
        assert (L0.agg < 0).sum() >= 4 and (L0.halo_cmap < 0).sum() >= 3
        used = np.unique(L0.halo_cmap[L0.halo_cmap >= 0])
        assert len(used) < L0.nhc and np.bincount(L0.halo_cmap[L0.halo_cmap >= 0] - L0.nc).max() == 2
