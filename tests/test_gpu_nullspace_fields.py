"""Matrices declared MGS_NULLSPACE_FIELDS on the device (include/mgs.h: mgs_csr_set_nullspace_fields): the label ingest, the projection
kernels, the coarse labels and the regularised coarsest solve, and the projected mgs_minres / mgs_minres_plan / mgs_pcg against
tests/nullspace_fields_ref.py run on the device's OWN hierarchy (level operators and aggregates downloaded).

The test system is enclosed_stokes(N) (multigridsolver_amd/synthetic.py): K = [[L, Dᵀ], [D, 0]] with exactly one null vector, the pressure
constant, assembled on the device with bmat / transpose / scale / @ as in the README; the preconditioner is the hierarchy of
block_diag(L, S), S = D·diag(L)⁻¹·Dᵀ, coarse_rows = 50, ω = 0.6, V(1,1).  Without the declaration its coarsest operator is singular and
finalize() refuses it — on the parent commit too, where the declaration does not exist: the solves below cannot pass there.

Bars:
  * the reported residual equals ‖Π(b − K·x)‖/‖Πb‖ recomputed in numpy within 1e-3 relative;
  * |mean(x_f)| <= n_f·ε·max|x_i| for every field, the worst case of any summation order;
  * x and the restatement's x both lie in the range and both residuals are at most tol·‖Πb‖, so ‖x − x_ref‖ <= 2·tol·‖Πb‖/σ_min⁺ (σ_min⁺:
    the smallest non-zero |eigenvalue| of the dense symmetric matrix, np.linalg.eigvalsh);
  * iteration counts: tests/test_gpu_nullspace.py's bar, |it − it_ref| <= max(2, it_ref // 6);
  * nullspace_defect <= 16·ε: a row of S holds 7 entries and takes 6 additions, each off by at most one rounding;
  * projection: every labelled entry is fl(v_i − m_f) for the device's own m_f, |m_f − mean_f| <= n_f·ε·max|v|, two identical calls give
    identical bits, unlabelled entries and the guard entries around the view keep their bits, nrm2 within n·ε relative."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sps

import nullspace_fields_ref as nf
import nullspace_ref as ns
from test_gpu_minres import dev, to_scipy
from test_gpu_nullspace import grid_laplacian

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
INVALID, NUMERIC = -1, -5


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


def dev_labels(ctx, lab, dtype):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(lab, dtype=dtype)).to(f"cuda:{ctx.device}")
    torch.cuda.synchronize(ctx.device)
    return t


def identity(mg, ctx, n):
    return mg.Csr.from_diag(ctx, ctx.vec(np.ones(n)))


def refused(mg, code, words, fn):
    with pytest.raises(mg.MgsError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    for w in ([words] if isinstance(words, str) else words):
        assert w in str(e.value), str(e.value)


# ================================================================================================================ projection kernel
def check_projection(ctx, mg, n, offset, nfields, seed):
    rng = np.random.default_rng(seed)
    lab = rng.integers(-1, nfields, n)
    k = min(nfields, n)
    lab[:k] = np.arange(k)                                  # every field receives at least one row
    nfl = int(lab.max()) + 1                                # (n < nfields: the fields that exist)
    A = identity(mg, ctx, n).set_nullspace_fields(lab, nfl)
    assert A.nullspace() == "fields" and A.nullspace_fields() == (nfl, [int((lab == f).sum()) for f in range(nfl)])
    base = ctx.vec(n + 4)
    assert base.ptr % 16 == 0
    lo = 2 if offset == 0 else 1                            # view at 16 or at 8 bytes: entry lo − 1 in front and entry lo + n behind are guards
    view = mg.Vec.wrap(ctx, base.ptr + 8 * lo, n)
    assert view.ptr % 16 == offset
    v = rng.standard_normal(n) * 3.0 + 1.5
    full = np.full(n + 4, 7.25); full[lo:lo + n] = v
    outs = []
    for _ in range(2):
        base.upload(full)
        m, nrm = view.project_fields(A, nrm2=True)
        outs.append((m.copy(), nrm, base.numpy()))
    (m, nrm, got), (m2, nrm2, got2) = outs
    assert np.array_equal(m, m2) and nrm == nrm2 and np.array_equal(got, got2)                # identical calls, identical bits
    out = got[lo:lo + n]
    assert np.array_equal(got[:lo], full[:lo]) and np.array_equal(got[lo + n:], full[lo + n:])   # guards
    assert np.array_equal(out[lab < 0].view(np.int64), v[lab < 0].view(np.int64))             # unlabelled: bit-unchanged
    for f in range(nfl):
        sel = lab == f
        mean = math.fsum(v[sel]) / sel.sum()
        assert abs(m[f] - mean) <= sel.sum() * EPS * np.abs(v).max(), (n, offset, nfields, f)
        assert np.array_equal(out[sel], v[sel] - m[f]), (n, offset, nfields, f)
    assert abs(nrm - np.linalg.norm(out)) <= n * EPS * np.linalg.norm(out)
    base.upload(full)
    assert np.array_equal(view.project_fields(A), m) and np.array_equal(base.numpy(), got)    # without the norm: the same means, the same entries
    del view
    return A


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 65539])
def test_projection_kernel(ctx, mg, n):
    for offset in (0, 8):
        for nfields in (1, 3, 8):
            check_projection(ctx, mg, n, offset, nfields, seed=n + offset + nfields)
    ctx.sync()


@pytest.mark.parametrize("vec", [1, 0])
def test_projection_kernel_large(ctx, mg, vec):
    """n = 2²¹ + 5: 4097 workgroups of the 16-byte arm (the chunk stage of the fold) and the `nt` store hint (nt_store = 10⁶ rows)"""
    n = 2 ** 21 + 5
    ctx.set_option("blas1_vec", vec)
    try:
        for offset in (0, 8):
            check_projection(ctx, mg, n, offset, 2, seed=77 + offset)
    finally:
        ctx.set_option("blas1_vec", 1)
    ctx.sync()


def test_two_matrices_on_one_context_do_not_collide(ctx, mg):
    n = 300
    A = identity(mg, ctx, n).set_nullspace_fields(np.zeros(n, dtype=np.int64))
    B = identity(mg, ctx, n).set_nullspace_fields(np.r_[np.zeros(100), np.ones(200)].astype(np.int32), 2)
    a, b = ctx.vec(np.full(n, 2.0)), ctx.vec(np.r_[np.full(100, 1.0), np.full(200, -3.0)])
    ma = a.project_fields(A); mb = b.project_fields(B)
    assert ma.tolist() == [2.0] and mb.tolist() == [1.0, -3.0]
    assert not a.numpy().any() and not b.numpy().any()
    a.fill(4.0)
    assert a.project_fields(A).tolist() == [4.0] and b.project_fields(B).tolist() == [0.0, 0.0]


# ================================================================================================================== ingest refusals
def test_ingest_refusals(ctx, mg):
    n = 700
    good = np.r_[np.zeros(300), np.ones(300), -np.ones(100)].astype(np.int64)
    A = identity(mg, ctx, n).set_nullspace_fields(good, 2)
    before = (A.nullspace(), A.nullspace_fields())
    assert before == ("fields", (2, [300, 300]))

    def bad(lab, nfields, words, dtype=np.int64):
        t = dev_labels(ctx, lab, dtype)
        refused(mg, INVALID, words, lambda: A.set_nullspace_fields(t, nfields))
        assert (A.nullspace(), A.nullspace_fields()) == before           # the declaration it had
        ctx.sync()
    lab = good.copy(); lab[[650, 411]] = 2
    bad(lab, 2, ["row 411", "label 2"])                                      # a label equal to nfields: the lowest row is named
    bad(lab, 2, ["row 411", "label 2"], np.int32)
    lab = good.copy(); lab[[699, 5]] = -2
    bad(lab, 2, ["row 5", "label -2"])
    lab = good.copy(); lab[123] = 2 ** 32
    bad(lab, 2, ["row 123", str(2 ** 32)])                                   # compared as a 64-bit value: it does not alias 0
    lab = good.copy(); lab[lab == 1] = 2
    bad(lab, 3, "field 1 has no rows")
    for nfields, bits_words in ((0, "nfields"), (9, "nfields")):
        bad(good, nfields, bits_words)
    assert mg.lib().mgs_csr_set_nullspace(A.h, 2) == INVALID and b"unknown kind" in mg.lib().mgs_last_error(ctx.h)   # entered through the new call only
    assert (A.nullspace(), A.nullspace_fields()) == before
    # a row shard
    shard = ctx.poisson3d(8, 2, 6, local_cols=True)
    t = dev_labels(ctx, np.zeros(shard.shape[0]), np.int32)
    refused(mg, INVALID, "row shard", lambda: shard.set_nullspace_fields(t, 1))
    assert shard.nullspace() is None
    with pytest.raises(ValueError):
        A.set_nullspace_fields(good[:-1])                                    # the length is checked in Python
    # taking the declaration back frees the labels; a constant declaration replaces it
    assert A.set_nullspace(None).nullspace() is None and A.nullspace_fields() == (0, [])
    refused(mg, INVALID, "MGS_NULLSPACE_FIELDS", lambda: ctx.vec(n).project_fields(A))
    assert A.set_nullspace_fields(good).set_nullspace("constant").nullspace() == "constant"
    ctx.sync()


# =============================================================================================================== enclosed Stokes flow
def device_cycle(h, labels, omega=0.6):
    """nullspace_fields_ref.Cycle over the device's own hierarchy"""
    As, aggs = [], []
    for l in range(h.nlev):
        As.append(to_scipy(h.level_A(l)))
        if l + 1 < h.nlev:
            aggs.append(h.level_P(l).agg().astype(np.int64))
    return nf.Cycle(As, aggs, omega, labels=labels), aggs


class Stokes:
    """enclosed_stokes(N) on the device with every handle the values-only chain needs, its hierarchy, and what the checks share"""

    def __init__(self, mg, ctx, N, declare=True):
        self.mg, self.ctx = mg, ctx
        self.sd = sd = nf.enclosed_stokes(N)
        self.n, self.m, self.lab = sd["n"], sd["m"], sd["labels"]
        self.L, self.D = dev(ctx, sd["L"]), dev(ctx, sd["D"])
        self.Dt = self.D.transpose()
        self.Dts = self.D.transpose().scale(left=self.L.diag_inv())
        self.S = self.D @ self.Dts
        self.K = mg.Csr.bmat(ctx, [[self.L, self.Dt], [self.D, None]])
        self.B = mg.Csr.block_diag(ctx, [self.L, self.S])
        assert self.K.shape == (self.n, self.n) and abs(to_scipy(self.K) - sd["K"]).max() == 0.0
        if declare:
            self.K.set_nullspace_fields(self.lab)                                       # numpy, nfields = max + 1
            self.B.set_nullspace_fields(dev_labels(ctx, self.lab, np.int32), 1)         # a device tensor
        self.h = None
        self._smin = None
        self.b_np = np.random.default_rng(N).uniform(0.0, 1.0, self.n)                  # non-zero pressure mean
        self.b = ctx.vec(self.b_np)
        self.ref = {}

    def hierarchy(self):
        return self.mg.Hierarchy(self.B, 0.6, 1, 1).coarsen(coarse_rows=50).finalize()

    def prepare(self):
        if self.h is None:
            self.h = self.hierarchy()
            self.cycle, self.aggs = device_cycle(self.h, self.lab)
        return self

    @property
    def smin(self):
        if self._smin is None:
            ev = np.sort(np.abs(np.linalg.eigvalsh(self.sd["K"].toarray())))
            assert ev[0] <= self.n * EPS * ev[-1] and ev[1] > 0.1                       # exactly one null vector
            self._smin = ev[1]
        return self._smin

    def reference(self, tol, x0=None, key=None):
        key = (tol, key)
        if key not in self.ref:
            self.ref[key] = nf.minres(self.sd["K"], self.b_np, self.lab, self.cycle.vcycle, tol=tol, max_iter=500, x0=x0)
            assert self.ref[key][0] == 0
        return self.ref[key]

    def check(self, got, x, tol, ref, label, K=None, scale=1.0):
        K = self.sd["K"] if K is None else K
        st, it, resid = got
        pb = nf.project(self.b_np, self.lab)
        true = np.linalg.norm(nf.project(self.b_np - K @ x, self.lab)) / np.linalg.norm(pb)
        xp = x[self.lab == 0]
        print(f"{label}: {got}, recomputed {true:.4e}, |mean(x_p)| {abs(xp.mean()):.3e} (bar {self.m * EPS * np.abs(x).max():.3e})")
        assert st == 0 and resid < tol
        assert abs(resid - true) <= 1e-3 * true
        assert abs(xp.mean()) <= self.m * EPS * np.abs(x).max()
        if ref is not None:
            _, it_r, _, x_r = ref
            dist, bar = np.linalg.norm(x - x_r / scale), 2 * tol * np.linalg.norm(pb) / (scale * self.smin)
            print(f"   ‖x − x_ref‖ {dist:.3e} (bar {bar:.3e}), iterations {it} against {it_r}")
            assert dist <= bar
            assert abs(it - it_r) <= max(2, it_r // 6)


_stokes = {}


@pytest.fixture
def stokes(mg, ctx):
    def get(N):
        if N not in _stokes:
            _stokes[N] = Stokes(mg, ctx, N)
        return _stokes[N].prepare()
    yield get


@pytest.fixture(scope="module", autouse=True)
def _release(ctx):
    yield
    _stokes.clear()      # before the context closes


def test_enclosed_stokes_fails_without_and_works_with_the_declaration(ctx, mg, stokes):
    tol = 1e-8
    plain = Stokes(mg, ctx, 6, declare=False)
    assert plain.n == 864
    refused(mg, NUMERIC, "singular", plain.hierarchy)                      # today's behaviour, kept
    refused(mg, INVALID, "null-space kind", lambda: mg.minres(plain.K, ctx.vec(plain.n), plain.b, stokes(6).h, 10, tol))   # K undeclared, h declared
    s = stokes(6)
    assert s.h.nlev >= 3
    shapes = [s.h.level_shape(l)[0] for l in range(s.h.nlev)]
    outside = [(a < 0).sum() for a in s.aggs]
    print(f"levels {shapes}, rows outside every aggregate {outside}")
    assert outside[0] > 0 and (s.aggs[0][s.lab >= 0] >= 0).all()           # all three row classes occur on level 0
    for M, name in ((s.K, "K"), (s.B, "B")):
        d = M.nullspace_defect()
        print(f"nullspace_defect({name}) = {d}")
        assert max(d) <= 16 * EPS
    bits = s.b.numpy().tobytes()
    x = ctx.vec(s.n)
    got = mg.minres(s.K, x, s.b, s.h, 500, tol)
    assert s.b.numpy().tobytes() == bits                                   # the caller's b is only read
    s.check(got, x.numpy(), tol, s.reference(tol), "enclosed_stokes(6) to 1e-8")
    # deterministic: the same call again gives the same bits
    y = ctx.vec(s.n)
    assert mg.minres(s.K, y, s.b, s.h, 500, tol) == got and np.array_equal(x.numpy(), y.numpy())
    # without a hierarchy the projections alone make the system solvable (slowly): the loop stays in the range
    z = ctx.vec(s.n)
    st, it, res = mg.minres(s.K, z, s.b, None, 3000, 1e-6)
    print(f"no preconditioner: {(st, it, res)}")
    assert st == 0 and abs(z.numpy()[s.lab == 0].mean()) <= s.m * EPS * np.abs(z.numpy()).max()


def test_enclosed_stokes_8(ctx, mg, stokes):
    tol = 1e-6
    s = stokes(8)
    assert s.n == 2048
    x = ctx.vec(s.n)
    got = mg.minres(s.K, x, s.b, s.h, 500, tol)
    s.check(got, x.numpy(), tol, s.reference(tol), "enclosed_stokes(8) to 1e-6")


def test_initial_guess_and_zero_right_hand_side(ctx, mg, stokes):
    tol = 1e-8
    s = stokes(6)
    x0 = np.random.default_rng(9).standard_normal(s.n); x0[s.lab == 0] += 5.0 - x0[s.lab == 0].mean()      # pressure mean 5
    x = ctx.vec(x0)
    got = mg.minres(s.K, x, s.b, s.h, 500, tol)
    s.check(got, x.numpy(), tol, s.reference(tol, x0=x0, key="x0"), "initial guess of pressure mean 5")
    # Πb = 0 and an x0 inside the null space: nothing to do, x = Πx0
    b0 = ctx.vec(np.r_[np.zeros(3 * s.m), np.full(s.m, 0.75)])
    g0 = np.r_[np.zeros(3 * s.m), np.full(s.m, 3.0)]
    x = ctx.vec(g0); w = ctx.vec(g0)
    got = mg.minres(s.K, x, b0, s.h, 500, tol)
    w.project_fields(s.K)
    print(f"Πb = 0: {got}")
    assert got[:2] == (0, 0) and got[2] == 0.0 and np.array_equal(x.numpy(), w.numpy()) and not x.numpy().any()


def test_plan_has_minres_bits(ctx, mg, stokes):
    tol = 1e-8
    s = stokes(6)
    xw = ctx.vec(s.n)
    want = mg.minres(s.K, xw, s.b, s.h, 500, tol)
    assert want[0] == 0
    h = s.hierarchy()
    plan = mg.MinresPlan(s.K, h)
    for ahead in (0, 1, 10000):
        x = ctx.vec(s.n)
        got = plan.solve(x, s.b, 500, tol, ahead)
        info = plan.info()
        print(f"ahead {ahead}: {got}, info {info}")
        assert got == want and np.array_equal(x.numpy(), xw.numpy()), f"ahead {ahead}"
        assert info[0] > 7 * 8 * s.n and info[1] >= 1 and info[2] - info[3] == want[1] and info[3] >= 0 and info[4] >= 1 and info[5] >= 0
        if ahead == 0:
            assert info[3] == 0
    assert h.graph_info()["captured_cycles"] == 2
    # enqueue + result: no host wait; status 0 on the true residual, or 1 with its documented meaning (the estimate ran ahead)
    x = ctx.vec(s.n)
    st, done, res = plan.enqueue(x, s.b, want[1] + 5, tol).result()
    assert plan.info()[4] == 0
    true = np.linalg.norm(nf.project(s.b_np - s.sd["K"] @ x.numpy(), s.lab)) / np.linalg.norm(nf.project(s.b_np, s.lab))
    print(f"enqueue({want[1] + 5}): {(st, done, res)}, recomputed {true:.4e}")
    assert abs(res - true) <= 1e-3 * true
    assert (st == 0 and true <= tol * (1 + 1e-3)) or (st == 1 and done <= want[1] + 5 and res >= tol)
    assert abs(x.numpy()[s.lab == 0].mean()) <= s.m * EPS * np.abs(x.numpy()).max()
    # the constant kind is still refused, and a hierarchy of other counts
    refused(mg, INVALID, "constant null space", lambda: mg.MinresPlan(dev(ctx, s.sd["K"]).set_nullspace("constant")))


def test_refresh_keeps_labels_and_graphs(ctx, mg):
    tol = 1e-8
    s = Stokes(mg, ctx, 6)
    h = s.hierarchy()
    plan = mg.MinresPlan(s.K, h)
    x = ctx.vec(s.n)
    first = plan.solve(x, s.b, 500, tol)
    assert first[0] == 0 and h.graph_info()["captured_cycles"] == 2
    # doubled L and D values on the same patterns; S follows through the values-only chain
    s.L.update_values(2.0 * s.sd["L"].data); s.D.update_values(2.0 * s.sd["D"].data)
    s.Dt.transpose_update(s.D); s.Dts.transpose_update(s.D).scale(left=s.L.diag_inv())
    s.S.matmul_update(s.D, s.Dts)
    s.K.bmat_update([[s.L, s.Dt], [s.D, None]]); s.B.bmat_update([[s.L, None], [None, s.S]])
    h.refresh()
    assert h.refresh_info()["refreshes"] == 1 and h.refresh_info()["kept_graphs"] == 1 and h.graph_info()["captured_cycles"] == 2
    assert s.K.nullspace() == "fields" and s.B.nullspace_fields() == (1, [s.m])
    y = ctx.vec(s.n)
    got = plan.solve(y, s.b, 500, tol)
    s.check(got, y.numpy(), tol, None, "after refresh (values doubled)", K=2.0 * s.sd["K"])
    assert np.linalg.norm(y.numpy() - 0.5 * x.numpy()) <= 2 * tol * np.linalg.norm(s.b_np) / (2.0 * s.smin)
    assert h.graph_info()["captured_cycles"] == 2
    z = ctx.vec(s.n)
    assert mg.minres(s.K, z, s.b, h, 500, tol) == got and np.array_equal(z.numpy(), y.numpy())


# ============================================================================================================== PCG with two fields
def two_field_system():
    from multigridsolver_amd.synthetic import neumann3d
    import agmg_ref
    G = grid_laplacian(6, 5, 3)                                                        # 30 rows, Neumann: one constant
    e = sps.eye(4, format="csr"); t = sps.diags([-np.ones(3), 2.0 * np.ones(4), -np.ones(3)], [-1, 0, 1], format="csr")
    Pd = (sps.kron(sps.kron(t, e), e) + sps.kron(sps.kron(e, t), e) + sps.kron(sps.kron(e, e), t)).tocsr()      # Poisson 4³, Dirichlet: regular
    Nm = agmg_ref.csr(125, 125, *neumann3d(5))                                         # one more constant
    A = sps.block_diag([G, Pd, Nm], format="csr"); A.sort_indices()
    lab = np.r_[np.zeros(30), -np.ones(64), np.ones(125)].astype(np.int64)
    return A, lab


def run_pcg(mg, ctx, S, lab, b_np, tol, label, lam):
    A = dev(ctx, S).set_nullspace_fields(lab)
    assert A.nullspace_fields() == (2, [30, 125])
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(coarse_rows=20).finalize()
    assert h.nlev >= 2
    cycle, _ = device_cycle(h, lab)
    ref = nf.pcg(S, b_np, lab, cycle.vcycle, tol=tol, max_iter=200)
    assert ref[0] == 0
    x = ctx.vec(S.shape[0]); b = ctx.vec(b_np)
    st, it, resid = mg.pcg(A, x, b, h, 200, tol)
    xs = x.numpy()
    pb = nf.project(b_np, lab)
    true = np.linalg.norm(nf.project(b_np - S @ xs, lab)) / np.linalg.norm(pb)
    dist, bar = np.linalg.norm(xs - ref[3]), 2 * tol * np.linalg.norm(pb) / lam
    print(f"{label}: {(st, it, resid)}, recomputed {true:.4e}, reference {ref[1]} iterations, ‖x − x_ref‖ {dist:.3e} (bar {bar:.3e})")
    assert st == 0 and true <= tol * (1 + 1e-3) and b.numpy().tobytes() == b_np.tobytes()
    for f in (0, 1):
        sel = lab == f
        assert abs(xs[sel].mean()) <= sel.sum() * EPS * np.abs(xs).max()
    assert dist <= bar and abs(it - ref[1]) <= max(2, ref[1] // 6)
    return it, ref[1]


def test_pcg_two_fields(ctx, mg):
    tol = 1e-10
    S, lab = two_field_system()
    n = S.shape[0]
    lam = np.linalg.eigvalsh(S.toarray())
    assert abs(lam[1]) <= n * EPS * lam[-1] and lam[2] > 1e-3                          # two null vectors
    b_np = np.random.default_rng(11).standard_normal(n)                                # inconsistent: Π makes it consistent
    it, it_r = run_pcg(mg, ctx, S, lab, b_np, tol, "block order", lam[2])
    # the rows of the two Neumann blocks interleaved: the same permutation on matrix, labels and right-hand side
    order = np.argsort(np.r_[np.arange(30) * 4.0, 1000.0 + np.arange(64), np.arange(125) + 0.5], kind="stable")
    Sp = S[order][:, order].tocsr(); Sp.sort_indices()
    assert (np.diff(lab[order][:60]) != 0).sum() > 20                                  # interleaved indeed
    # on the device through permute, held against the host permutation
    import torch
    p = torch.from_numpy(order.astype(np.int64)).to(f"cuda:{ctx.device}"); torch.cuda.synchronize(ctx.device)
    assert abs(to_scipy(dev(ctx, S).permute(p, p)) - Sp).max() == 0.0
    it_p, it_pr = run_pcg(mg, ctx, Sp, lab[order], b_np[order], tol, "interleaved", lam[2])
    assert abs(it_p - it) <= max(2, it_r // 6)


# ============================================================================================================== structural refusals
def push_agg(mg, ctx, A, agg, nc):
    lib = mg.lib()
    agg = np.ascontiguousarray(agg, dtype=np.int32)
    T, Ac = C.c_void_p(), C.c_void_p()
    assert lib.mgs_xfer_from_agg(ctx.h, len(agg), nc, agg.ctypes.data_as(C.POINTER(C.c_int)), C.byref(T)) == 0
    assert lib.mgs_csr_galerkin(A.h, T, C.byref(Ac)) == 0
    h = mg.Hierarchy(A, 0.6, 1, 1)
    assert lib.mgs_hier_push_level(h.h, T, Ac) == 0             # the hierarchy owns both now
    return h


def test_structural_refusals(ctx, mg):
    S = grid_laplacian(4, 6, 1); n = S.shape[0]                # (the declarations below are not verified: they exercise the checks)
    i = np.arange(n)
    lab = (i >= 12).astype(np.int64)
    # an aggregate that mixes two labels: rows 11 (label 0) and 12 (label 1)
    A = dev(ctx, S).set_nullspace_fields(lab)
    h = push_agg(mg, ctx, A, (i + 1) // 2, 13)
    refused(mg, INVALID, ["level 0", "row 12", "another label"], h.finalize)
    ctx.sync()
    # a labelled row outside every aggregate
    agg = i // 2; agg[5] = -1
    h = push_agg(mg, ctx, A, agg, 12)
    refused(mg, INVALID, ["level 0", "row 5", "outside every aggregate"], h.finalize)
    ctx.sync()
    # ... which is fine for an unlabelled row
    lab5 = lab.copy(); lab5[5] = -1
    A5 = dev(ctx, S).set_nullspace_fields(lab5)
    h5 = push_agg(mg, ctx, A5, agg, 12)
    try:
        h5.finalize()                                           # structurally accepted; numerically S is not singular on these fields
    except mg.MgsError as e:
        assert e.code == NUMERIC
    # a general P
    P = sps.coo_matrix((np.r_[np.ones(n), 0.5], (np.r_[i, 0], np.r_[i // 2, 1])), shape=(n, n // 2)).tocsr(); P.sort_indices()
    hp = mg.Hierarchy(A, 0.6, 1, 1).push_P(dev(ctx, P))
    refused(mg, INVALID, ["level 0", "general P"], hp.finalize)
    # the solvers that do not serve the kind name what does
    x, b = ctx.vec(n), ctx.vec(np.ones(n))
    served = "mgs_minres / mgs_pcg"
    refused(mg, INVALID, served, lambda: mg.bicgstab(A, x, b, None, 10, 1e-6))
    refused(mg, INVALID, served, lambda: mg.fgcr(A, x, b, None, 10, 10, 1e-6))
    refused(mg, INVALID, served, lambda: mg.PcgPlan(A))
    refused(mg, INVALID, served, lambda: mg.BicgstabPlan(A))
    refused(mg, INVALID, served, lambda: mg.FgcrPlan(A))
    refused(mg, INVALID, served, lambda: mg.Guess(A, "energy", 4))
    # minres still refuses the constant kind
    Ac = dev(ctx, S).set_nullspace("constant")
    refused(mg, INVALID, "constant null space", lambda: mg.minres(Ac, x, b, None, 10, 1e-6))
    # a hierarchy whose field counts differ from A's; one of another kind
    lab2 = (i >= 10).astype(np.int64)
    B2 = dev(ctx, S).set_nullspace_fields(lab2)
    h2 = push_agg(mg, ctx, B2, i // 2, 12).finalize()
    refused(mg, INVALID, ["field 0", "12", "10"], lambda: mg.pcg(A, x, b, h2, 10, 1e-6))
    refused(mg, INVALID, ["field 0", "12", "10"], lambda: mg.minres(A, x, b, h2, 10, 1e-6))
    refused(mg, INVALID, ["field 0", "12", "10"], lambda: mg.MinresPlan(A, h2))
    B3 = dev(ctx, S).set_nullspace_fields(np.zeros(n, dtype=np.int64))
    h3 = push_agg(mg, ctx, B3, i // 2, 12).finalize()
    refused(mg, INVALID, "fields", lambda: mg.pcg(A, x, b, h3, 10, 1e-6))
    hc = mg.Hierarchy(Ac, 0.6, 1, 1).finalize()
    refused(mg, INVALID, "null-space kind", lambda: mg.pcg(A, x, b, hc, 10, 1e-6))
    ctx.sync()                                                  # nothing faulted: argument checks, or the check kernel's word


# ======================================================================================================== kinds 0 and 1 are untouched
def test_constant_kind_through_the_dispatch(ctx, mg):
    """mgs_pcg's projections go through one dispatch on the matrix's record: with max_iter = 0 the solve is x ← Πx0 alone, which must be
    Vec.project_const's bits for a constant matrix and Vec.project_fields's for a fields matrix; a full solve keeps its iteration count"""
    S = grid_laplacian(20, 20, 5); n = S.shape[0]
    rng = np.random.default_rng(2)
    x0, b_np = rng.standard_normal(n) + 3.0, ns.project(rng.standard_normal(n))
    A1 = dev(ctx, S).set_nullspace("constant")
    x, w, b = ctx.vec(x0), ctx.vec(x0), ctx.vec(b_np)
    st, it, _ = mg.pcg(A1, x, b, None, 0, 1e-10)
    w.project_const()
    assert (st, it) == (1, 0) and np.array_equal(x.numpy(), w.numpy())
    A2 = dev(ctx, S).set_nullspace_fields(np.zeros(n, dtype=np.int64))
    x, w = ctx.vec(x0), ctx.vec(x0)
    st, it, _ = mg.pcg(A2, x, b, None, 0, 1e-10)
    w.project_fields(A2)
    assert (st, it) == (1, 0) and np.array_equal(x.numpy(), w.numpy())
    # the full solves: the constant kind against tests/nullspace_ref.py as before, the one-field twin beside it
    h1 = mg.Hierarchy(A1, 0.6, 1, 1).coarsen(coarse_rows=60).finalize()
    h2 = mg.Hierarchy(A2, 0.6, 1, 1).coarsen(coarse_rows=60).finalize()
    As = [to_scipy(h1.level_A(l)) for l in range(h1.nlev)]
    aggs = [h1.level_P(l).agg().astype(np.int64) for l in range(h1.nlev - 1)]
    ref = ns.pcg(S, b_np, ns.Cycle(As, aggs, 0.6).vcycle, tol=1e-10, max_iter=200)
    x1, x2 = ctx.vec(n), ctx.vec(n)
    r1 = mg.pcg(A1, x1, b, h1, 200, 1e-10); r2 = mg.pcg(A2, x2, b, h2, 200, 1e-10)
    print(f"constant {r1}, one field {r2}, reference {ref[:3]}")
    assert r1[0] == 0 and r2[0] == 0 and abs(r1[1] - ref[1]) <= max(2, ref[1] // 6) and abs(r2[1] - r1[1]) <= max(2, ref[1] // 6)
    y1 = ctx.vec(n)
    assert mg.pcg(A1, y1, b, h1, 200, 1e-10) == r1 and np.array_equal(x1.numpy(), y1.numpy())
    # an undeclared matrix takes no projection at all
    A0 = dev(ctx, S + sps.eye(n, format="csr")); x = ctx.vec(x0)
    assert mg.pcg(A0, x, b, None, 0, 1e-10)[:2] == (1, 0) and np.array_equal(x.numpy(), x0)
