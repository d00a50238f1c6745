"""mgs_csr_spgemm / mgs_csr_spgemm_numeric on the device against the host restatement of their arithmetic (tests/spgemm_ref.py): rowptr
and col with np.array_equal, val bit for bit (view(np.int64)).  tests/test_spgemm_ref_cpu.py shows that every fixture compared here
is sensitive to the order of its sums, so equal bits mean the order of include/mgs.h."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import spgemm_ref as ref

pytestmark = pytest.mark.gpu

OK, INVALID, STATE = 0, -1, -6


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


def product(ctx, fx):
    A, B = fx
    dA, dB = up(ctx, A), up(ctx, B)
    return dA, dB, dA.matmul(dB)


def test_poisson8_times_itself_runs_on_the_lane_path(ctx):
    fx = ref.fx_poisson8()
    dA, dB, Cd = product(ctx, fx)
    want = ref.spgemm(*fx)
    rp, ci, v = assert_bits(Cd, want, "poisson 8^3")
    info = Cd.spgemm_info()
    assert info == {"lane_rows": 512, "workgroup_rows": 0, "max_row_len": int(np.diff(rp).max()), "max_row_products": 49}, info
    # an ordinary matrix: launch plan, pattern code, SpMV
    assert Cd.plan_info()["max_row_len"] == info["max_row_len"]
    x = np.random.default_rng(1).standard_normal(512)
    y = Cd.optimize().spmv(ctx.vec(x)).numpy()
    yr = ref.to_scipy(want) @ x
    assert np.linalg.norm(y - yr) <= 1e-12 * np.linalg.norm(yr)
    assert ctx.poisson2d(4).spgemm_info() == {"lane_rows": 0, "workgroup_rows": 0, "max_row_len": 0, "max_row_products": 0}


def test_rectangular_with_empty_rows(ctx):
    fx = ref.fx_rect()
    dA, dB, Cd = product(ctx, fx)
    rp, ci, v = assert_bits(Cd, ref.spgemm(*fx), "37 x 53 times 53 x 29")
    lens = np.diff(rp)
    assert lens[3] == 0 and lens[11] == 0 and lens[7] == 0 and Cd.shape == (37, 29)
    assert (dA @ dB).nnz == Cd.nnz                       # the operator form


def test_the_bin_boundary(ctx):
    fx = ref.fx_boundary()
    dA, dB, Cd = product(ctx, fx)
    rp, ci, v = assert_bits(Cd, ref.spgemm(*fx), "64 | 65 products")
    info = Cd.spgemm_info()
    assert info["lane_rows"] == 1 and info["workgroup_rows"] == 1 and info["max_row_products"] == 65, info
    assert np.diff(rp)[1] < 64


def test_the_workgroup_path_over_several_steps_and_determinism(ctx):
    fx = ref.fx_wide()
    dA, dB, Cd = product(ctx, fx)
    want = ref.spgemm(*fx)
    rp, ci, v = assert_bits(Cd, want, "five steps")
    info = Cd.spgemm_info()
    assert info["workgroup_rows"] == 2 and info["lane_rows"] == 1 and info["max_row_products"] == 4000 and info["max_row_len"] == rp[1], info
    again = dA.matmul(dB).download()
    assert all(a.tobytes() == b.tobytes() for a, b in zip((rp, ci, v), again))


def test_the_row_limit(ctx, mg):
    fx = ref.fx_limit(ref.MAX_ROW)
    dA, dB, Cd = product(ctx, fx)
    assert_bits(Cd, ref.spgemm(*fx), "8192 columns")
    assert Cd.spgemm_info()["max_row_len"] == ref.MAX_ROW
    L = mg.lib()
    for fx, row in ((ref.fx_limit(ref.MAX_ROW + 1), 0), (ref.fx_limit_row3(), 3)):
        dA, dB = up(ctx, fx[0]), up(ctx, fx[1])
        out = C.c_void_p(0x1234)
        assert L.mgs_csr_spgemm(dA.h, dB.h, C.byref(out)) == INVALID
        msg = L.mgs_last_error(ctx.h).decode()
        assert f"row {row} " in msg and "MGS_SPGEMM_MAX_ROW" in msg, msg
        assert out.value == 0x1234                       # *C untouched
    # the context still works
    assert_bits(product(ctx, ref.fx_zeros())[2], ref.spgemm(*ref.fx_zeros()))


def test_structural_zeros_stay_entries(ctx):
    fx = ref.fx_zeros()
    rp, ci, v = assert_bits(product(ctx, fx)[2], ref.spgemm(*fx), "zeros")
    assert rp.tolist() == [0, 2, 4] and ci.tolist() == [0, 1, 0, 1]
    assert v[0] == 0.0 and not np.signbit(v[0])          # a·b + (−a)·b stays an entry
    assert v[3] == 0.0 and np.signbit(v[3])              # a lone −0.0 stays −0.0


def agg_P(g, nc):
    ok = g >= 0
    return sps.csr_matrix((np.ones(int(ok.sum())), (np.flatnonzero(ok), g[ok])), shape=(len(g), nc))


def test_numeric_recomputes_in_place_and_the_hierarchy_refreshes(ctx, mg):
    (A1, B1), (A2, B2) = ref.fx_numeric(0), ref.fx_numeric(1)
    n = A1[0]
    dA, dB, Cd = product(ctx, (A1, B1))
    assert_bits(Cd, ref.spgemm(A1, B1), "first values")
    ptrs = Cd.device_ptrs()
    h = mg.Hierarchy(Cd, 0.6, 1, 1).coarsen(10.0, 2, 8.0, coarse_rows=40).finalize()
    assert h.nlev >= 2
    b = ctx.vec(n).rand(seed=11); x = ctx.vec(n)
    h.vcycle(b, x); h.vcycle(b, x)
    x1 = x.numpy()
    dA.update_values(A2[4]); dB.update_values(B2[4])
    assert Cd.matmul_update(dA, dB) is Cd
    assert Cd.device_ptrs() == ptrs
    assert_bits(Cd, ref.spgemm(A2, B2), "second values, in place")
    assert Cd.matmul_update(dA, dB, check=True) is Cd    # no product outside the pattern
    assert_bits(Cd, ref.spgemm(A2, B2), "second values again")
    h.refresh()
    assert h.refresh_info()["kept_graphs"] == 1, h.refresh_info()
    h.vcycle(b, x)
    fresh = up(ctx, A2).matmul(up(ctx, B2))
    assert all(np.array_equal(p, q) for p, q in zip(Cd.download(), fresh.download()))
    h2 = mg.Hierarchy(fresh, 0.6, 1, 1)
    for l in range(h.nlev - 1):
        P = agg_P(h.level_P(l).agg(), h.level_shape(l + 1)[0])
        h2.push_P(ctx.csr(P.shape[0], P.shape[1], P.indptr, P.indices, P.data))
    h2.finalize()
    x2 = h2.vcycle(b).numpy()
    assert np.isfinite(x2).all() and np.linalg.norm(x2) > 0 and not np.array_equal(x1, x2)
    assert np.array_equal(x.numpy(), x2)


def test_numeric_counts_products_outside_the_pattern(ctx, mg):
    rng = np.random.default_rng(5)
    A = ref.rows_to_csr([np.array([0, 1])], 2, rng)
    B = ref.rows_to_csr([np.array([0, 1]), np.array([2])], 3, rng)
    keep = np.array([True, False, True])                 # B′ = B without its entry (0, 1)
    Bp = (2, 3, np.array([0, 1, 2], dtype=np.int32), B[3][keep], B[4][keep])
    dA, dB, dBp = up(ctx, A), up(ctx, B), up(ctx, Bp)
    Cp = dA.matmul(dBp)
    assert Cp.download()[1].tolist() == [0, 2]
    with pytest.raises(mg.MgsError) as e:
        Cp.matmul_update(dA, dB, check=True)
    assert e.value.code == STATE and e.value.misses == 1, (e.value, e.value.misses)
    assert Cp.matmul_update(dA, dBp, check=True) is Cp
    assert_bits(Cp, ref.spgemm(A, Bp))


def test_refusals(ctx, mg):
    L = mg.lib()
    A, B = ref.fx_rect()
    dA, dB = up(ctx, A), up(ctx, B)

    def refused(a, b, word):
        out = C.c_void_p(0x1234)
        assert L.mgs_csr_spgemm(a, b, C.byref(out)) == INVALID
        msg = L.mgs_last_error(ctx.h).decode()
        assert word in msg and out.value == 0x1234, msg
    refused(dA.h, dA.h, "37 x 53")                       # shape mismatch
    refused(None, dB.h, "NULL"); refused(dA.h, None, "NULL")
    assert L.mgs_csr_spgemm(dA.h, dB.h, None) == INVALID
    other = mg.Context(0)
    try:
        oB = up(other, B)
        refused(dA.h, oB.h, "different contexts")
        del oB
    finally:
        other.close()
    shard = ctx.poisson3d(8, 2, 5)                       # rows of planes 2..4 of the 8^3 operator: 192 x 512
    full = ctx.poisson3d(8)
    refused(shard.h, full.h, "row shard")
    local = ctx.poisson3d(8, 2, 5, local_cols=True)      # 192 x 320: owned columns, then two halo planes
    X = ref.rows_to_csr([np.array([0, 100]), np.array([191])], 192, np.random.default_rng(2))
    dX = up(ctx, X)
    refused(dX.h, local.h, "row shard")
    # _numeric: shapes that do not fit C, a C that no product built
    Cd = dA.matmul(dB)
    with pytest.raises(mg.MgsError) as e:
        Cd.matmul_update(dB, dB)
    assert e.value.code == INVALID
    with pytest.raises(mg.MgsError) as e:
        bA, bB = (up(ctx, M) for M in ref.fx_boundary())
        Cd.matmul_update(bA, bB)
    assert e.value.code == INVALID and "C is 37 x 29" in str(e.value)
    with pytest.raises(mg.MgsError) as e:
        dA.matmul_update(dA, dB)
    assert e.value.code == INVALID
    assert L.mgs_csr_spgemm_numeric(None, dB.h, Cd.h, None) == INVALID
    assert_bits(Cd, ref.spgemm(A, B), "untouched by the refused calls")


def test_a_context_that_sums_over_ranks_refuses_matrices_with_more_columns_than_rows(mg):
    c = mg.Context(0)
    try:
        c.set_allreduce(lambda a: None)
        A, B = ref.fx_rect()
        with pytest.raises(mg.MgsError) as e:
            up(c, A).matmul(up(c, B))
        assert e.value.code == INVALID and "row shard" in str(e.value)
    finally:
        c.close()


def test_general_galerkin_is_two_device_products(ctx, mg, orc):
    Ao = orc.poisson2d(20)
    n = Ao.shape[0]; nc = n // 4
    P = ref.general_P(n, nc)
    A = (n, n, np.asarray(Ao.rowptr, dtype=np.int32), np.asarray(Ao.col, dtype=np.int32), np.asarray(Ao.val, dtype=np.float64))
    dA, dP = up(ctx, A), up(ctx, P)
    T = mg.Xfer.from_csr(dP)
    assert not T.is_aggregation
    assert_bits(dA.galerkin(T), ref.galerkin(A, P), "(Pt A) P, Poisson 2-D n = 20")
    # the same patterns with values whose sums show their order (test_spgemm_ref_cpu.py)
    rng = np.random.default_rng(2020)
    Aw, Pw = ref.with_values(A, ref.wide(rng, len(A[3]))), ref.with_values(P, ref.wide(rng, len(P[3])))
    dPw = up(ctx, Pw)
    assert_bits(up(ctx, Aw).galerkin(mg.Xfer.from_csr(dPw)), ref.galerkin(Aw, Pw), "(Pt A) P, wide values")
    # the hierarchy on it, as test_gpu_parity.py::test_general_P_fallback demands
    Po = orc.Csr.from_scipy(ref.to_scipy(P))
    r_np = orc.rand_rhs(n)
    h = mg.Hierarchy(dA, 0.6, 1, 1).push_P(dP).finalize()
    ho = orc.Hier(Ao, [Po], omega=0.6, nu1=1, nu2=1)
    want = ho.vcycle(r_np)
    assert np.linalg.norm(h.vcycle(ctx.vec(r_np)).numpy() - want) <= 1e-10 * np.linalg.norm(want)
