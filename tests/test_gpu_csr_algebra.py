"""mgs_csr_add / mgs_csr_add_numeric / mgs_csr_scale / mgs_csr_diag / mgs_csr_from_diag on the device against the host restatement of
their arithmetic (tests/csr_algebra_ref.py): rowptr and col with np.array_equal, val bit for bit (view(np.int64)).
tests/test_csr_algebra_ref_cpu.py shows that every value fixture compared here is sensitive to the specified roundings, so equal bits
mean the operations of include/mgs.h, each rounded on its own."""
import ctypes as C

import numpy as np
import pytest

import csr_algebra_ref as ref
import spgemm_ref

pytestmark = pytest.mark.gpu

OK, INVALID, STATE = 0, -1, -6
NOT_A_SUM = {"lane_rows": 0, "wave_rows": 0, "max_row_len": 0, "common_entries": 0}


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


def up(ctx, M):
    return ctx.csr(*M)


def assert_bits(Cd, want, what=""):
    rp, ci, v = Cd.download()
    assert Cd.shape == (want[0], want[1]), what
    assert np.array_equal(rp, want[2]) and np.array_equal(ci, want[3]), what
    same = v.view(np.int64) == want[4].view(np.int64)
    assert same.all(), (what, int((~same).sum()), float(np.abs(v - want[4]).max()))
    return rp, ci, v


def total(fx, ctx):
    alpha, A, beta, B = fx
    dA, dB = up(ctx, A), up(ctx, B)
    return dA, dB, dA.add(dB, alpha, beta)


def test_poisson8_plus_a_random_pattern_runs_on_the_lane_path(ctx):
    fx = ref.fx_lane()
    dA, dB, Cd = total(fx, ctx)
    rp, ci, v = assert_bits(Cd, ref.add(*fx), "poisson 8^3 + 5 per row")
    info = Cd.add_info()
    assert info == ref.add_info(fx[1], fx[3]) and info["lane_rows"] == 512 and info["wave_rows"] == 0 and info["common_entries"] >= 1024, info
    assert dA.add_info() == NOT_A_SUM and ctx.poisson2d(4).add_info() == NOT_A_SUM
    # an ordinary matrix: launch plan, pattern code, SpMV
    assert Cd.plan_info()["max_row_len"] == info["max_row_len"] == int(np.diff(rp).max())
    x = np.random.default_rng(1).standard_normal(512)
    y = Cd.optimize().spmv(ctx.vec(x)).numpy()
    yr = ref.to_scipy(ref.add(*fx)) @ x
    assert np.linalg.norm(y - yr) <= 1e-12 * np.linalg.norm(yr)
    # the operator forms: alpha = beta = 1 and alpha = 1, beta = −1
    assert_bits(dA + dB, ref.add(1.0, fx[1], 1.0, fx[3]), "A + B")
    assert_bits(dA - dB, ref.add(1.0, fx[1], -1.0, fx[3]), "A - B")


def test_rectangular_with_empty_rows(ctx):
    fx = ref.fx_rect()
    dA, dB, Cd = total(fx, ctx)
    rp, ci, v = assert_bits(Cd, ref.add(*fx), "37 x 53")
    lens = np.diff(rp)
    assert lens[20] == 0 and lens[3] == np.diff(fx[3][2])[3] and lens[11] == np.diff(fx[1][2])[11] and Cd.shape == (37, 53)
    assert Cd.add_info() == ref.add_info(fx[1], fx[3])


def test_the_bin_boundary(ctx):
    fx = ref.fx_boundary()
    dA, dB, Cd = total(fx, ctx)
    assert_bits(Cd, ref.add(*fx), "64 | 65 entries")
    info = Cd.add_info()
    assert info["lane_rows"] == 1 and info["wave_rows"] == 1 and info == ref.add_info(fx[1], fx[3]), info


def test_the_wave_path_over_several_chunks_and_determinism(ctx):
    fx = ref.fx_wave()
    dA, dB, Cd = total(fx, ctx)
    rp, ci, v = assert_bits(Cd, ref.add(*fx), "several chunks")
    info = Cd.add_info()
    assert info["wave_rows"] == 5 and info["lane_rows"] == 2 and info == ref.add_info(fx[1], fx[3]), info
    assert np.diff(rp).tolist() == [150 + 131 - 40, 100, 180, 108, 110, 4, 0]
    again = dA.add(dB, fx[0], fx[2]).download()
    assert all(a.tobytes() == b.tobytes() for a, b in zip((rp, ci, v), again))
    assert_bits(dB.add(dA, fx[2], fx[0]), ref.add(fx[2], fx[3], fx[0], fx[1]), "the operands exchanged")


def test_a_long_row(ctx):
    fx = ref.fx_long()
    dA, dB, Cd = total(fx, ctx)
    rp, ci, v = assert_bits(Cd, ref.add(*fx), "(5000, 4000) in 3 x 20000")
    assert np.diff(rp).tolist() == [2, 8000, 0]
    assert Cd.add_info() == {"lane_rows": 2, "wave_rows": 1, "max_row_len": 8000, "common_entries": 1001}


def test_special_values_and_scalars(ctx):
    alpha, A, beta, B = ref.fx_special()
    dA, dB, Cd = total((alpha, A, beta, B), ctx)
    rp, ci, v = assert_bits(Cd, ref.add(alpha, A, beta, B), "zeros")
    assert rp.tolist() == [0, 2, 4] and ci.tolist() == [0, 1, 0, 2]
    assert v[0] == 0.0 and not np.signbit(v[0]) and v[3] == 0.0 and not np.signbit(v[3])      # equal values cancel and stay entries
    assert v[1] == 0.0 and np.signbit(v[1]) and v[2] == 0.0 and np.signbit(v[2])              # a lone −0.0 stays −0.0
    # the same handle on either side, on both paths
    for fx in (ref.fx_lane(), ref.fx_wave()):
        M = fx[1]
        dM = up(ctx, M)
        Sd = dM.add(dM, ref.ALPHA, ref.BETA)
        assert_bits(Sd, ref.add(ref.ALPHA, M, ref.BETA, M), "A == B")
        assert Sd.add_info()["common_entries"] == len(M[3]) == Sd.nnz
        assert not (dM - dM).download()[2].view(np.int64).any()      # every entry +0.0, none dropped
    # a sum is an operand of another sum and a factor of a product
    S2 = Cd.add(dA, 2.0, 1.0)
    assert_bits(S2, ref.add(2.0, ref.add(alpha, A, beta, B), 1.0, A), "a sum of a sum")


def test_numeric_update_in_place(ctx, mg):
    fx0, fx1 = ref.fx_numeric(0), ref.fx_numeric(1)
    dA, dB, Cd = total(fx0, ctx)
    assert_bits(Cd, ref.add(*fx0), "first values")
    ptrs = Cd.device_ptrs()
    dA.update_values(fx1[1][4]); dB.update_values(fx1[3][4])
    assert Cd.add_update(dA, dB, fx1[0], fx1[2]) is Cd           # enqueued only
    assert Cd.device_ptrs() == ptrs
    assert_bits(Cd, ref.add(*fx1), "second values and scalars, in place")
    dA.update_values(fx0[1][4]); dB.update_values(fx0[3][4])
    assert Cd.add_update(dA, dB, fx0[0], fx0[2], check=True) is Cd      # misses == 0
    misses = C.c_int64(-1)
    assert mg.lib().mgs_csr_add_numeric(fx0[0], dA.h, fx0[2], dB.h, Cd.h, C.byref(misses)) == OK and misses.value == 0
    assert_bits(Cd, ref.add(*fx0), "first values again")
    fresh = up(ctx, fx0[1]).add(up(ctx, fx0[3]), fx0[0], fx0[2])
    assert all(np.array_equal(p, q) for p, q in zip(Cd.download(), fresh.download()))
    assert Cd.device_ptrs() == ptrs
    # a B of another pattern: row 5 (a lane row) holds column 8 instead of 7, row 4 (a wave row) column 499 instead of its last
    B = fx0[3]
    ci = B[3].copy()
    assert ci[B[2][6] - 1] == 7 and ci[B[2][5] - 1] < 499
    ci[B[2][6] - 1] = 8; ci[B[2][5] - 1] = 499
    dBp = up(ctx, (B[0], B[1], B[2], ci, B[4]))
    with pytest.raises(mg.MgsError) as e:
        Cd.add_update(dA, dBp, fx0[0], fx0[2], check=True)
    assert e.value.code == STATE and e.value.misses == 3, (e.value, e.value.misses)
    assert Cd.add_update(dA, dB, fx0[0], fx0[2], check=True) is Cd
    assert_bits(Cd, ref.add(*fx0), "after the refused update")
    # a C that no sum built; shapes that do not fit C
    with pytest.raises(mg.MgsError) as e:
        dA.add_update(dA, dB)
    assert e.value.code == INVALID and "not built by mgs_csr_add" in str(e.value)
    rA, rB = up(ctx, ref.fx_rect()[1]), up(ctx, ref.fx_rect()[3])
    with pytest.raises(mg.MgsError) as e:
        Cd.add_update(rA, rB)
    assert e.value.code == INVALID and "C is 7 x 1000" in str(e.value)
    assert mg.lib().mgs_csr_add_numeric(1.0, None, 1.0, dB.h, Cd.h, None) == INVALID


def test_scale_diag_from_diag(ctx, mg):
    A, dl, dr = ref.fx_scale()
    vl, vr = ctx.vec(dl), ctx.vec(dr)
    for l, r, hl, hr in ((vl, None, dl, None), (None, vr, None, dr), (vl, vr, dl, dr), (None, None, None, None)):
        dA = up(ctx, A)
        ptrs = dA.device_ptrs()
        assert dA.scale(left=l, right=r) is dA and dA.device_ptrs() == ptrs
        assert_bits(dA, ref.scale(A, hl, hr), f"left {l is not None} right {r is not None}")
    # the diagonal of a matrix with missing diagonal entries, a tall one (row 2 stores a 0.0 on it)
    M = ref.fx_missing_diag()
    dM = up(ctx, M)
    d = dM.diagonal()
    assert len(d) == 4
    got = d.numpy()
    assert got.tobytes() == ref.diag(M).tobytes() and got[0] != 0.0 and not got[1:].view(np.int64).any()      # +0.0 where none is stored
    assert ctx.poisson3d(8).diagonal().numpy().tolist() == [6.0] * 512
    wide_d = up(ctx, ref.fx_rect()[1]).diagonal()                         # 37 x 53
    assert wide_d.numpy().tobytes() == ref.diag(ref.fx_rect()[1]).tobytes()
    # a vector as a diagonal matrix, zeros included
    w = np.array([1.5, 0.0, -0.0, -2.25, 7.0])
    D = mg.Csr.from_diag(ctx, ctx.vec(w))
    rp, ci, v = D.download()
    assert D.shape == (5, 5) and rp.tolist() == [0, 1, 2, 3, 4, 5] and ci.tolist() == [0, 1, 2, 3, 4] and v.tobytes() == w.tobytes()
    assert D.diagonal().numpy().tobytes() == w.tobytes() and D.add_info() == NOT_A_SUM
    assert D.spmv(ctx.vec(np.ones(5))).numpy().tolist() == [1.5, 0.0, 0.0, -2.25, 7.0]
    # refusals: short vectors, a row shard, a value-carrying pattern code
    L = mg.lib()
    dA = up(ctx, A)
    before = dA.download()[2].copy()
    assert L.mgs_csr_scale(dA.h, ctx.vec(36).h, None) == INVALID and "36 entries" in L.mgs_last_error(ctx.h).decode()
    assert L.mgs_csr_scale(dA.h, None, ctx.vec(52).h) == INVALID and "52 entries" in L.mgs_last_error(ctx.h).decode()
    assert L.mgs_csr_diag(dA.h, ctx.vec(36).h) == INVALID and "36 entries" in L.mgs_last_error(ctx.h).decode()
    shard = ctx.poisson3d(8, 2, 5, local_cols=True)
    assert L.mgs_csr_scale(shard.h, None, ctx.vec(320).h) == INVALID and "row shard" in L.mgs_last_error(ctx.h).decode()
    assert dA.download()[2].tobytes() == before.tobytes()
    c2 = mg.Context(0)
    try:
        c2.set_option("valcode", 1)
        P = c2.poisson3d(8).optimize()
        assert P.rowcode_info()["coded_blocks"] > 0
        with pytest.raises(mg.MgsError) as e:
            P.scale(left=c2.vec(np.ones(512)))
        assert e.value.code == INVALID and "valcode" in str(e.value)
        del P
    finally:
        c2.close()


def test_composition_with_the_product(ctx):
    B, d = ref.fx_compose()
    dinv = 1.0 / d
    dB = up(ctx, B)
    Bt = dB.transpose()
    S = dB.scale(right=ctx.vec(dinv)) @ Bt                                # (B·D⁻¹)·Bᵀ
    want = spgemm_ref.spgemm(ref.scale(B, None, dinv), spgemm_ref.csr(spgemm_ref.to_scipy(B).T))
    assert_bits(S, want, "B D^-1 B^T")
    assert S.shape == (40, 40)


def host_residual(A, x, b):
    rp, ci, v = A.download()
    n = len(rp) - 1
    r = b - ref.to_scipy((n, n, rp, ci, v)) @ x
    return np.linalg.norm(r) / np.linalg.norm(b)


def test_the_implicit_time_step_loop(ctx, mg):
    """A = M/Δt + K built on the device, a hierarchy on it, a solve; a new Δt through add_update, refresh, a solve — no host assembly.
    The residual is relative to ‖b‖, as the solver's; the 1e-9 margin is 10× the solver's tolerance, for the host's different summation
    order."""
    n = 512
    K = ctx.poisson3d(8)
    mass = 0.5 + np.random.default_rng(77).random(n)
    M = mg.Csr.from_diag(ctx, ctx.vec(mass))
    rpK, ciK, vK = K.download()
    Kh = (n, n, rpK, ciK, vK)
    Mh = (n, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), mass)
    dt = 1.7      # M/Δt ≤ 0.89: the interior rows stay far from diagonal dominance, so the pairwise matching coarsens them
    A = M.add(K, 1.0 / dt, 1.0)
    assert_bits(A, ref.add(1.0 / dt, Mh, 1.0, Kh), "M/dt + K")
    assert A.nnz == K.nnz and A.add_info()["common_entries"] == n
    ptrs = A.device_ptrs()
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, coarse_rows=60).finalize()
    assert h.nlev >= 2
    bh = np.random.default_rng(78).standard_normal(n)
    b = ctx.vec(bh); x = ctx.vec(n)
    st, it, tol = mg.pcg(A, x, b, h, 200, 1e-10)
    assert st == 0 and tol <= 1e-10, (st, it, tol)
    assert host_residual(A, x.numpy(), bh) < 1e-9
    dt2 = 0.3
    assert A.add_update(M, K, 1.0 / dt2, 1.0) is A
    fresh = M.add(K, 1.0 / dt2, 1.0)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(A.download(), fresh.download()))
    assert_bits(A, ref.add(1.0 / dt2, Mh, 1.0, Kh), "M/dt2 + K, in place")
    assert A.device_ptrs() == ptrs
    h.refresh()
    x2 = ctx.vec(n)
    st, it2, tol = mg.pcg(A, x2, b, h, 200, 1e-10)
    assert st == 0 and tol <= 1e-10, (st, it2, tol)
    assert host_residual(A, x2.numpy(), bh) < 1e-9
    assert not np.array_equal(x.numpy(), x2.numpy())


def test_refusals(ctx, mg):
    L = mg.lib()
    _, A, _, B = ref.fx_rect()
    dA, dB = up(ctx, A), up(ctx, B)

    def refused(a, b, word):
        out = C.c_void_p(0x1234)
        assert L.mgs_csr_add(1.0, a, 1.0, b, C.byref(out)) == INVALID
        msg = L.mgs_last_error(ctx.h).decode()
        assert word in msg and out.value == 0x1234, msg
    At = dA.transpose()
    refused(dA.h, At.h, "A is 37 x 53, B is 53 x 37")           # shape mismatch: the message gives both
    refused(None, dB.h, "NULL"); refused(dA.h, None, "NULL")
    assert L.mgs_csr_add(1.0, dA.h, 1.0, dB.h, None) == INVALID
    other = mg.Context(0)
    try:
        oB = up(other, B)
        refused(dA.h, oB.h, "different contexts")
        del oB
    finally:
        other.close()
    local = ctx.poisson3d(8, 2, 5, local_cols=True)             # 192 x 320: owned columns, then two halo planes
    X = ref.rows_to_csr([np.array([0, 100])] + [ref.EMPTY] * 191, 320, np.random.default_rng(2))
    dX = up(ctx, X)
    refused(local.h, dX.h, "row shard"); refused(dX.h, local.h, "row shard")
    refused(local.h, local.h, "row shard")
    assert_bits(dA.add(dB, 2.0, 3.0), ref.add(2.0, A, 3.0, B), "the context still works")
