"""The device pairwise matching (multigridsolver_amd/csrc/setup_agmg.hip) against its exact host restatement tests/agmg_ref.py.

Every comparison is np.array_equal of the downloaded aggregate ids with the restatement's: the library is built with -ffp-contract=off,
halving is exact and FP64 division is IEEE on both sides, so the device takes the same decisions, not similar ones.  Multi-level cases go
level by level: the level's operator and origins are downloaded from the device and that level alone is restated, so a difference names its
level.  agmg_ref.check_matching (every pair is an admissible coupling, no admissible coupling is left between two singletons, ids are the
ranks of the smallest members, no aggregate spans two zones — on ALL couplings) runs beside it and alone where the restatement's round
loop would take too long (the 4 194 305-row chain).  Round counts and branch counters come from the restatement: they are properties of
the inputs, printed per case.

Not exercised: the forced last round (round 95).  No small input is known that survives the 71 hash-only rounds before it."""
import ctypes as C

import numpy as np
import pytest

import agmg_ref as R

pytestmark = pytest.mark.gpu

KTG = 10.0
INVALID = -1


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


def up(ctx, A):
    return ctx.csr(A.shape[0], A.shape[1], A.indptr, A.indices, A.data)


def down(M):
    rp, ci, v = M.download()
    return R.csr(M.shape[0], M.shape[1], rp, ci, v)


def report(tag, Rr):
    for s, p in enumerate(Rr.passes):
        pairs, singles, g0 = R.pass_counts(p["agg"])
        print(f"{tag} pass {s + 1}: {p['A'].shape[0]} rows, rounds {p['rounds']}, pairs {pairs}, singletons {singles}, G0 {g0}, branches {p['branches']}")


def levels_equal(ctx, mg, A_sp, npass, tag, tou=8.0, coarse_rows=20, max_levels=32, origin=None):
    """coarsen on the device, then restate every level from what the device holds there: aggregate ids, the next operator (pattern and
    values, bit for bit: same sums in the same order) and its origins are equal; the coarsening stopped where the rule says"""
    A = up(ctx, A_sp)
    if origin is not None:
        A.set_origin(origin)
    h = mg.Hierarchy(A, 0.5, 1, 1).coarsen(KTG, npass, tou, coarse_rows=coarse_rows, max_levels=max_levels)
    out = []
    for l in range(h.nlev - 1):
        Al, org = down(h.level_A(l)), h.level_A(l).origin()
        Rr = R.aggregate(Al, KTG, npass, tou, org)
        report(f"{tag} level {l}", Rr)
        assert all(p["rounds"] < R.MAX_ROUNDS for p in Rr.passes)
        agg = h.level_P(l).agg()
        assert np.array_equal(agg, Rr.agg), (tag, l, int(np.sum(agg != Rr.agg)))
        R.check_matching(Al, agg, KTG, npass=len(Rr.passes))
        R.check_passes(Rr, KTG)
        rp, ci, v = h.level_A(l + 1).download()
        assert np.array_equal(rp, Rr.A_coarse.indptr) and np.array_equal(ci, Rr.A_coarse.indices)
        assert np.array_equal(v, Rr.A_coarse.data), (tag, l, float(np.max(np.abs(v - Rr.A_coarse.data))))
        assert np.array_equal(h.level_A(l + 1).origin(), Rr.origin)
        out.append(Rr)
    last = h.level_A(h.nlev - 1)
    if last.shape[0] > coarse_rows and h.nlev < max_levels:      # stopped early: only because the next step stalls (mgs_hier_coarsen)
        Rr = R.aggregate(down(last), KTG, npass, tou, last.origin())
        assert Rr.nc == 0 or Rr.nc > int(0.9 * last.shape[0])
    assert h.nlev >= 2
    return h, out


def one_pass(ctx, mg, A_sp, origin=None):
    A = up(ctx, A_sp)
    if origin is not None:
        A.set_origin(origin)
    h = mg.Hierarchy(A, 0.5, 1, 1).coarsen(KTG, 1, 8.0, coarse_rows=0, max_levels=2)
    assert h.nlev == 2
    return h.level_P(0).agg()


# ------------------------------------------------------------------------------------------------------------------------- scan edges
@pytest.mark.parametrize("n", [2047, 2048, 2049, 4095, 4097])
def test_scan_edges_uniform_chain(ctx, mg, n):
    """the leader-flag scan has n + 1 entries: one full tile of 2048, one tile + 1, two tiles − 1 / + 1"""
    A = R.chain(n)
    agg_ref, rounds, br = R.pairwise_pass(A, KTG, 1)
    cf = R.chain_closed_form(n)
    assert np.array_equal(agg_ref, cf)                         # the closed form is the restatement's (also pinned on the CPU)
    agg = one_pass(ctx, mg, A)
    print(f"chain n = {n}: rounds {rounds}, pairs/singletons/G0 {R.pass_counts(agg_ref)}, branches {br}")
    assert np.array_equal(agg, agg_ref) and np.array_equal(agg, cf)
    R.check_matching(A, agg, KTG)


def test_scan_three_levels_deep(ctx, mg):
    """n + 1 = 4 194 306 > 2048²: the smallest chain whose flag scan recurses three deep (tile sums of tile sums); closed form and
    check_matching only"""
    n = 4194305
    rp = np.r_[0, 2, 2 + 3 * np.arange(1, n - 1, dtype=np.int64), 3 * n - 2].astype(np.int32)
    i = np.arange(n, dtype=np.int64)
    col = np.stack([i - 1, i, i + 1], axis=1).ravel()[1:-1].astype(np.int32)
    val = np.tile(np.array([-1.0, 2.0, -1.0]), n)[1:-1]
    A = R.csr(n, n, rp, col, val)
    agg = one_pass(ctx, mg, A)
    assert np.array_equal(agg, R.chain_closed_form(n))
    print("chain n = 4194305:", R.check_matching(A, agg, KTG))


# -------------------------------------------------------------------------------------------------------------------- ties everywhere
@pytest.mark.parametrize("npass", [1, 2, 3])
@pytest.mark.parametrize("family", ["poisson2d_33", "poisson3d_9", "poisson3d_17"])
def test_ties_all_levels(ctx, mg, family, npass):
    """integer coefficients: every μ of a level ties with many others and the Galerkin sums are exact in any order, so the whole chain of
    operators is equal bit for bit and every decision is a tie-break in origin space"""
    A = {"poisson2d_33": lambda: R.poisson2d(33), "poisson3d_9": lambda: R.poisson3d(9), "poisson3d_17": lambda: R.poisson3d(17)}[family]()
    h, levels = levels_equal(ctx, mg, A, npass, f"{family} npass {npass}", coarse_rows=20)
    assert h.nlev >= 3 and len(levels[0].passes) == npass


# ------------------------------------------------------------------------------------------------------------------- distinct weights
def test_distinct_weights_random_nonsymmetric(ctx, mg):
    h, levels = levels_equal(ctx, mg, R.random_nonsymmetric(), 2, "random_nonsymmetric", coarse_rows=20)
    assert levels[0].passes[0]["rounds"] > 2


def test_distinct_weights_csky3d(ctx, mg):
    from multigridsolver_amd import synthetic
    N = 12
    rp, ci, v = synthetic.csky3d(N)
    levels_equal(ctx, mg, R.csr(N ** 3, N ** 3, rp, ci, v), 2, "csky3d 12", coarse_rows=20)


def test_every_inadmissibility_branch(ctx, mg):
    A, (above, below) = R.branchy()
    agg_ref, rounds, br = R.pairwise_pass(A, KTG, 1)
    print(f"branchy: rounds {rounds}, pairs/singletons/G0 {R.pass_counts(agg_ref)}, branches {br}")
    for name in ("g0", "okay_neg", "zero", "mu_nonpos", "mu_gt_ktg"):       # properties of the input
        assert br[name] > 0, name
    mu_a, mu_b = R.mu_of(A, KTG, *above), R.mu_of(A, KTG, *below)
    print(f"μ{above} = {mu_a!r}, μ{below} = {mu_b!r}")
    assert KTG < mu_a <= KTG * (1 + 4e-16 * 8) and KTG * (1 - 4e-16 * 8) <= mu_b <= KTG    # within a few ulps of ktg on either side
    agg = one_pass(ctx, mg, A)
    assert np.array_equal(agg, agg_ref)
    assert agg[above[0]] != agg[above[1]]
    R.check_matching(A, agg, KTG)
    levels_equal(ctx, mg, A, 2, "branchy", coarse_rows=20)


# ------------------------------------------------------------------------------------------------------------------- hash-only rounds
def test_hash_only_rounds(ctx, mg):
    A = R.hash_chain()
    agg_ref, rounds, br = R.pairwise_pass(A, KTG, 1)
    print(f"hash chain: rounds {rounds}, pairs/singletons/G0 {R.pass_counts(agg_ref)}")
    assert R.MU_ROUNDS < rounds < R.MAX_ROUNDS
    agg = one_pass(ctx, mg, A)
    assert np.array_equal(agg, agg_ref)
    R.check_matching(A, agg, KTG)


# ----------------------------------------------------------------------------------------------------------------- one-sided couplings
@pytest.mark.parametrize("family", ["one_sided_random", "forward_chain", "one_sided_zeros"])
def test_one_sided_couplings(ctx, mg, family):
    """a coupling stored (or non-zero) on one side only is a candidate like any other: the matching runs on the union of the patterns of A
    and Aᵀ, and {i,j} counts when a_ij != 0 or a_ji != 0"""
    A = getattr(R, family)()
    agg_ref, rounds, br = R.pairwise_pass(A, KTG, 1)
    print(f"{family}: asymmetric pattern {R._Pattern(A).asymmetric}, rounds {rounds}, pairs/singletons/G0 {R.pass_counts(agg_ref)}, branches {br}")
    assert rounds < R.MAX_ROUNDS
    agg = one_pass(ctx, mg, A)
    assert np.array_equal(agg, agg_ref), int(np.sum(agg != agg_ref))
    R.check_matching(A, agg, KTG)                               # in particular: no admissible coupling left between two singletons
    levels_equal(ctx, mg, A, 2, family, coarse_rows=20)


# ---------------------------------------------------------------------------------------------------------------------- row-shard form
@pytest.mark.parametrize("npass", [1, 2])
@pytest.mark.parametrize("zoned", [False, True])
def test_row_shard(ctx, mg, zoned, npass):
    """planes 4..7 of a 12³ Poisson grid with local columns (rows < cols): halo columns enter s_i and the G0 test and never pair; with
    zones (first owned plane 1, last owned plane 2, interior 0) no aggregate spans two zones, after pass 2 either"""
    from multigridsolver_amd._lib import check, lib
    N = 12
    A = ctx.poisson3d(N, 4, 8, local_cols=True)
    rows, cols = A.shape
    assert rows == 4 * N * N and cols == rows + 2 * N * N
    A_sp = down(A)
    host, host_zone = R.poisson3d_shard(N, 4, 8)                # the shard the CPU file pins the yardstick on
    assert np.array_equal(A_sp.indptr, host.indptr) and np.array_equal(A_sp.indices, host.indices) and np.array_equal(A_sp.data, host.data)
    zone = None
    if zoned:
        zone = np.zeros(rows, dtype=np.int32); zone[:N * N] = 1; zone[-N * N:] = 2
        assert np.array_equal(zone, host_zone)
        has_halo = np.diff(A_sp.indptr) > np.diff((A_sp[:, :rows]).tocsr().indptr)
        assert np.array_equal(has_halo, zone > 0)               # the zones are the exported planes
    T = C.c_void_p()
    check(lib().mgs_aggregate_shard_zoned(A.h, KTG, npass, 8.0, zone.ctypes.data_as(C.c_void_p) if zoned else None, C.byref(T)), ctx.h)
    agg = mg.core.Xfer(ctx, T).agg()
    Rr = R.aggregate(A_sp, KTG, npass, 8.0, A.origin(), zone)
    report(f"shard zoned {zoned} npass {npass}", Rr)
    assert len(Rr.passes) == npass and Rr.passes[0]["branches"]["halo"] == 2 * N * N and (Rr.passes[0]["branches"]["zone"] > 0) == zoned
    assert np.array_equal(agg, Rr.agg)
    R.check_matching(A_sp, agg, KTG, npass=npass, zone=zone)
    R.check_passes(Rr, KTG)


# --------------------------------------------------------------------------------------------------------------------------- tou stop
def test_tou_stop(ctx, mg):
    A = R.poisson2d(33)
    first = R.aggregate(A, KTG, 1, 8.0)
    ratio = A.nnz / first.A_coarse.nnz
    for tou, passes in ((ratio * (1 - 1e-9), 1), (ratio * (1 + 1e-9), 2)):
        Rr = R.aggregate(A, KTG, 2, tou)
        assert len(Rr.passes) == passes
        h, _ = levels_equal(ctx, mg, A, 2, f"tou {tou!r}", tou=tou, coarse_rows=0, max_levels=2)
        sizes = np.bincount(h.level_P(0).agg()[Rr.agg >= 0])
        assert sizes.max() == 2 ** passes


# --------------------------------------------------------------------------------------------------------------- caller-given origin
def test_caller_given_origin(ctx, mg):
    n = 16
    A = R.poisson2d(n)
    rng = np.random.default_rng(8)
    perm = rng.permutation(n * n)
    ident = R.aggregate(A, KTG, 2, 8.0).agg
    for tag, org in (("permutation", perm), ("shifted permutation", 3 * perm + 100000)):      # origins may exceed the row count
        assert not np.array_equal(R.aggregate(A, KTG, 2, 8.0, org).agg, ident)                 # the tie-breaks do depend on it
        levels_equal(ctx, mg, A, 2, tag, coarse_rows=20, origin=org)


def test_origin_refusals(ctx, mg):
    n = 8
    A = up(ctx, R.poisson2d(n))
    good = np.arange(n * n, dtype=np.int32)[::-1].copy()
    A.set_origin(good)
    for bad in (np.r_[good[:-1], good[0]], np.r_[-1, good[1:]], np.zeros(n * n, dtype=np.int32)):
        with pytest.raises(mg.MgsError) as e:
            A.set_origin(bad)
        assert e.value.code == INVALID
        assert np.array_equal(A.origin(), good)                 # refused before anything changed
    h = mg.Hierarchy(A, 0.5, 1, 1).coarsen(KTG, 1, 8.0, coarse_rows=0, max_levels=2)
    agg = h.level_P(0).agg()
    assert np.array_equal(agg, R.pairwise_pass(R.poisson2d(n), KTG, 1, good)[0])


def test_level_views_keep_their_hierarchy_alive(ctx, mg):
    """level_A / level_P are views into the hierarchy: read from a temporary hierarchy they must not outlive it"""
    A = up(ctx, R.poisson2d(16))
    h = mg.Hierarchy(A, 0.5, 1, 1).coarsen(KTG, 2, 8.0, coarse_rows=20)
    P0 = mg.Hierarchy(A, 0.5, 1, 1).coarsen(KTG, 2, 8.0, coarse_rows=20).level_P(0)
    A1 = mg.Hierarchy(A, 0.5, 1, 1).coarsen(KTG, 2, 8.0, coarse_rows=20).level_A(1)
    assert P0._hier is not h and P0._hier.h and A1._hier.h       # the temporaries are still there, held by their views
    assert np.array_equal(P0.agg(), h.level_P(0).agg())
    assert all(np.array_equal(a, b) for a, b in zip(A1.download(), h.level_A(1).download()))
