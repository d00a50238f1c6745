"""mgs_csr_extract / mgs_csr_extract_numeric / mgs_csr_extract_info / mgs_vec_gather / mgs_vec_scatter on the device against the host
restatement of their contract (tests/extract_ref.py): rowptr and col with np.array_equal, val bit for bit (view(np.int64)).
tests/test_extract_ref_cpu.py shows that the restatement is scipy's A[rows][:, cols] and that every fixture has the property its test here
relies on (the 64 | 65 boundary, the empty and the full chunk of the long row, −0.0 and NaN, repeated and descending rows).  Index lists
are placed with torch and made visible with torch.cuda.synchronize()."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla
import torch

import csr_algebra_ref
import extract_ref as ref
import spgemm_ref

pytestmark = pytest.mark.gpu

OK, INVALID, STATE = 0, -1, -6
NOT_A_BLOCK = {"lane_rows": 0, "wave_rows": 0, "max_row_len": 0, "map_bytes": 0}


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


def dev(a, dtype=np.int32):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to("cuda:0")
    torch.cuda.synchronize()
    return t


def up(ctx, M):
    return ctx.csr(*M)


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def assert_bits(Sd, want, what=""):
    rp, ci, v = Sd.download()
    assert Sd.shape == (want[0], want[1]), what
    assert np.array_equal(rp, want[2]) and np.array_equal(ci, want[3]), what
    same = bits(v) == bits(want[4])
    assert same.all(), (what, int((~same).sum()))
    return rp, ci, v


def block(ctx, dA, A, rows, cols, dtype=np.int32, keep_map=False, what=""):
    """the block on the device, held to the restatement: arrays and info"""
    Sd = dA.extract(dev(rows, dtype), dev(cols, dtype), keep_map=keep_map)
    want = ref.extract(A, rows, cols)
    assert_bits(Sd, want, what)
    assert Sd.extract_info() == ref.info(A, rows, cols, keep_map), (what, Sd.extract_info())
    return Sd, want


# ------------------------------------------------------------------ 1. Poisson 8³, one plane fixed
def test_poisson8_blocks_run_on_the_lane_path(ctx):
    A, fixed, free = ref.fx_poisson8()
    dA = ctx.poisson3d(8)
    assert_bits(dA, A, "the fixture is mgs_csr_poisson3d's operator")
    for name, rows, cols in (("ff", free, free), ("fc", free, fixed), ("cf", fixed, free), ("cc", fixed, fixed)):
        Sd, want = block(ctx, dA, A, rows, cols, what=name)
        info = Sd.extract_info()
        assert info["lane_rows"] == len(rows) and info["wave_rows"] == 0, (name, info)
        assert Sd.plan_info()["max_row_len"] == info["max_row_len"]
    assert dA.extract_info() == NOT_A_BLOCK
    # an ordinary matrix: pattern code, SpMV
    Aff = dA.extract(dev(free), dev(free))
    x = np.random.default_rng(1).standard_normal(448)
    y = Aff.optimize().spmv(ctx.vec(x)).numpy()
    yr = ref.to_scipy(ref.matrix(ref.extract(A, free, free))) @ x
    assert np.linalg.norm(y - yr) <= 1e-12 * np.linalg.norm(yr)


# ------------------------------------------------------------------ 2. rectangular, empty rows, the None forms, empty lists
def test_rectangular_with_empty_rows(ctx):
    A, rows, cols = ref.fx_rect()
    dA = up(ctx, A)
    Sd, want = block(ctx, dA, A, rows, None, what="descending rows with repeats, every column")
    info = Sd.extract_info()
    assert info["lane_rows"] == 0 and info["wave_rows"] == 0 and Sd.shape == (len(rows), 53)
    assert np.diff(want[2])[[0, 4, 5, 7, 8]].tolist() == [0] * 5            # rows 36, 20, 20, 3, 3 of A are empty
    Sd, want = block(ctx, dA, A, None, cols, what="every row, a column list")
    assert Sd.shape == (37, len(cols)) and Sd.extract_info()["lane_rows"] == 37
    block(ctx, dA, A, rows, cols, what="both lists")
    Sd, want = block(ctx, dA, A, None, None, what="both None")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(Sd.download(), dA.download()))
    none = np.zeros(0, dtype=np.int32)
    for r, c, shape in ((none, cols, (0, len(cols))), (rows, none, (len(rows), 0)), (none, None, (0, 53)), (None, none, (37, 0)), (none, none, (0, 0))):
        Sd, want = block(ctx, dA, A, r, c, keep_map=True, what=f"empty list {shape}")
        assert Sd.shape == shape and Sd.nnz == 0 and Sd.extract_info()["map_bytes"] == 0


# ------------------------------------------------------------------ 3. the bin boundary
def test_the_bin_boundary(ctx):
    A, rows, cols = ref.fx_boundary()
    Sd, want = block(ctx, up(ctx, A), A, rows, cols, what="source rows of 64 | 65 entries")
    info = Sd.extract_info()
    assert info["lane_rows"] == 1 and info["wave_rows"] == 1, info


# ------------------------------------------------------------------ 4. the wave path
def test_the_wave_path_over_several_chunks_and_determinism(ctx):
    A, rows, cols = ref.fx_wave()
    dA = up(ctx, A)
    Sd, want = block(ctx, dA, A, rows, cols, keep_map=True, what="64*3 + 17 entries")
    rp, ci, v = Sd.download()
    info = Sd.extract_info()
    assert info["wave_rows"] == 3 and info["lane_rows"] == 2 and info["map_bytes"] == 4 * Sd.nnz, info
    first, second = slice(rp[0], rp[1]), slice(rp[2], rp[3])                 # row 0 of A, selected twice
    assert rp[1] - rp[0] >= 64 + 20 + 5
    assert np.array_equal(ci[first], ci[second]) and np.array_equal(bits(v[first]), bits(v[second]))
    assert (bits(v[first]) == ref.NAN_BITS).sum() == 1 and (bits(v[first]) == bits(-0.0)).sum() == 1      # the NaN's payload, the zero's sign
    again = dA.extract(dev(rows), dev(cols), keep_map=True).download()
    assert all(a.tobytes() == b.tobytes() for a, b in zip((rp, ci, v), again))
    block(ctx, dA, A, rows, None, what="the long rows without a column list")


# ------------------------------------------------------------------ 5. index width
def test_index_width(ctx, mg):
    for fx in (ref.fx_wave, ref.fx_rect):
        A, rows, cols = fx()
        dA = up(ctx, A)
        S32, _ = block(ctx, dA, A, rows, cols, np.int32, what="int32")
        S64, _ = block(ctx, dA, A, rows, cols, np.int64, what="int64")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(S32.download(), S64.download()))
    with pytest.raises(TypeError):
        dA.extract(dev(rows, np.int32), dev(cols, np.int64))
    with pytest.raises(TypeError):
        dA.extract(dev(rows, np.int16))
    with pytest.raises(TypeError):
        dA.extract(rows)                                                     # a host array: nothing is converted
    big = np.array([0, 2 ** 32 + 3, 5], dtype=np.int64)                      # would narrow to row 3
    with pytest.raises(mg.MgsError) as e:
        dA.extract(dev(big, np.int64))
    assert e.value.code == INVALID and "position 1 " in str(e.value) and str(2 ** 32 + 3) in str(e.value), str(e.value)
    with pytest.raises(mg.MgsError) as e:
        dA.extract(None, dev(np.array([1, 2 ** 32 + 7], dtype=np.int64), np.int64))
    assert e.value.code == INVALID and "position 1 " in str(e.value) and str(2 ** 32 + 7) in str(e.value), str(e.value)


# ------------------------------------------------------------------ 6. refusals
def test_refusals(ctx, mg):
    L = mg.lib()
    A, rows, cols = ref.fx_rect()
    dA = up(ctx, A)

    def refused(r, c, words, bits=32, dtype=np.int32, a=dA):
        tr, tc = dev(r, dtype), dev(c, dtype)
        out = C.c_void_p(0x1234)
        rc = L.mgs_csr_extract(a.h if a is not None else None, C.c_void_p(tr.data_ptr()) if tr is not None else None, 0 if r is None else len(r),
                               C.c_void_p(tc.data_ptr()) if tc is not None else None, 0 if c is None else len(c), bits, 0, C.byref(out))
        msg = L.mgs_last_error(ctx.h).decode()
        assert rc == INVALID and out.value == 0x1234, (rc, msg)
        for w in words:
            assert w in msg, msg
        want = ref.refusal(A, r, c)
        if want is not None:
            assert f"position {want[1]} " in msg and str(want[2]) in msg, (want, msg)

    refused([0, -1, 5], None, ["row index -1", "position 1 "])
    refused([0, 5, 37, 2, 37], cols, ["row index 37", "position 2 ", "[0, 37)"])      # two offenders: the lower position is named
    refused(None, [0, 5, 53], ["column index 53", "position 2 ", "[0, 53)"])
    refused(rows, [0, 5, 5, 9], ["not strictly ascending", "position 2 "])            # equal adjacent columns
    refused(rows, [0, 9, 5, 3], ["not strictly ascending", "position 2 "])            # descending: positions 2 and 3 offend
    refused(rows, cols, ["index_bits 16"], bits=16)
    out = C.c_void_p(0x1234)
    assert L.mgs_csr_extract(dA.h, C.c_void_p(dev(rows).data_ptr()), -1, None, 0, 32, 0, C.byref(out)) == INVALID and out.value == 0x1234
    assert "negative" in L.mgs_last_error(ctx.h).decode()
    assert L.mgs_csr_extract(dA.h, None, 0, None, 0, 32, 0, None) == INVALID
    shard = ctx.poisson3d(8, 2, 5, local_cols=True)                           # 192 x 320: owned columns, then two halo planes
    assert L.mgs_csr_extract(shard.h, None, 0, None, 0, 32, 0, C.byref(out)) == INVALID and out.value == 0x1234
    assert "row shard" in L.mgs_last_error(ctx.h).decode()
    # the Python face raises the same refusals
    with pytest.raises(mg.MgsError) as e:
        dA.extract(dev([0, 5, 37, 2, 37]), dev(cols))
    assert e.value.code == INVALID and "position 2 " in str(e.value)
    # a valid call afterwards still gives the right bits
    block(ctx, dA, A, rows, cols, what="the context still works")


# ------------------------------------------------------------------ 7. the values again through the kept map
def test_numeric_update_in_place(ctx, mg):
    rng = np.random.default_rng(7)
    cases = [("lane", ) + ref.fx_boundary(), ("wave", ) + ref.fx_wave(), ("no column list", ref.fx_wave()[0], ref.fx_wave()[1], None),
             ("poisson", ref.fx_poisson8_values(0), ref.fx_poisson8()[2], ref.fx_poisson8()[2])]
    for what, A, rows, cols in cases:
        dA = up(ctx, A)
        Sd, want = block(ctx, dA, A, rows, cols, keep_map=True, what=what)
        ptrs = Sd.device_ptrs()
        new = rng.standard_normal(len(A[4]))
        new[::5] = -0.0
        A2 = ref.with_values(A, new)
        dA.update_values(new)
        assert Sd.extract_update(dA) is Sd and Sd.device_ptrs() == ptrs      # enqueued only, nothing moved
        assert_bits(Sd, ref.extract(A2, rows, cols), what + ": new values, in place")
        fresh = up(ctx, A2).extract(dev(rows), dev(cols))
        assert all(p.tobytes() == q.tobytes() for p, q in zip(Sd.download(), fresh.download()))
    # no map kept; a matrix that no extract built; a source of another entry count, of another shape
    A, rows, cols = ref.fx_wave()
    dA = up(ctx, A)
    plain = dA.extract(dev(rows), dev(cols))
    kept = dA.extract(dev(rows), dev(cols), keep_map=True)
    for S in (plain, dA):
        with pytest.raises(mg.MgsError) as e:
            S.extract_update(dA)
        assert e.value.code == STATE and "keeps no source map" in str(e.value)
    R = ref.fx_rect()[0]
    with pytest.raises(mg.MgsError) as e:
        kept.extract_update(up(ctx, R))
    assert e.value.code == INVALID and "37 x 53" in str(e.value)
    fewer = (A[0], A[1], np.minimum(A[2], len(A[3]) - 1).astype(np.int32), A[3][:-1], A[4][:-1])      # the last entry dropped
    with pytest.raises(mg.MgsError) as e:
        kept.extract_update(up(ctx, fewer))
    assert e.value.code == INVALID and f"{len(A[3]) - 1} entries" in str(e.value)
    assert mg.lib().mgs_csr_extract_numeric(None, kept.h) == INVALID and mg.lib().mgs_csr_extract_numeric(dA.h, None) == INVALID
    other = mg.Context(0)
    try:
        oA = up(other, A)
        with pytest.raises(mg.MgsError) as e:
            kept.extract_update(oA)
        assert e.value.code == INVALID and "different context" in str(e.value)
        del oA
    finally:
        other.close()
    assert_bits(kept, ref.extract(A, rows, cols), "after the refused updates")


def agg_P(g, nc):
    ok = g >= 0
    return sps.csr_matrix((np.ones(int(ok.sum())), (np.flatnonzero(ok), g[ok])), shape=(len(g), nc))


def test_extract_update_then_the_hierarchy_refreshes(ctx, mg):
    A1, A2 = ref.fx_poisson8_values(0), ref.fx_poisson8_values(1)
    _, fixed, free = ref.fx_poisson8()
    dA = up(ctx, A1)
    Aff = dA.extract(dev(free), dev(free), keep_map=True)
    ptrs = Aff.device_ptrs()
    h = mg.Hierarchy(Aff, 0.6, 1, 1).coarsen(10.0, 2, 8.0, coarse_rows=40).finalize()
    assert h.nlev >= 2
    b = ctx.vec(448).rand(seed=11); x = ctx.vec(448)
    h.vcycle(b, x); h.vcycle(b, x)
    x1 = x.numpy()
    dA.update_values(A2[4])
    assert Aff.extract_update(dA) is Aff and Aff.device_ptrs() == ptrs
    h.refresh()
    assert h.refresh_info()["kept_graphs"] == 1, h.refresh_info()
    h.vcycle(b, x)
    fresh = up(ctx, A2).extract(dev(free), dev(free))
    assert all(p.tobytes() == q.tobytes() for p, q in zip(Aff.download(), fresh.download()))
    h2 = mg.Hierarchy(fresh, 0.6, 1, 1)
    for l in range(h.nlev - 1):
        P = agg_P(h.level_P(l).agg(), h.level_shape(l + 1)[0])
        h2.push_P(ctx.csr(P.shape[0], P.shape[1], P.indptr, P.indices, P.data))
    h2.finalize()
    x2 = h2.vcycle(b).numpy()
    assert np.isfinite(x2).all() and np.linalg.norm(x2) > 0 and not np.array_equal(x1, x2)
    assert np.array_equal(x.numpy(), x2)


# ------------------------------------------------------------------ 8. gather and scatter
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_gather_and_scatter(ctx, mg, dtype):
    x, idx, y = ref.fx_vectors()
    dx = ctx.vec(x)
    g = dx.gather(dev(idx, dtype))
    assert len(g) == len(idx) and np.array_equal(bits(g.numpy()), bits(ref.gather(x, idx)[0]))
    out = ctx.vec(len(idx) + 3).fill(9.0)
    assert dx.gather(dev(idx, dtype), out=out, check=True) is out
    assert np.array_equal(bits(out.numpy()), bits(np.r_[ref.gather(x, idx)[0], [9.0] * 3]))
    t = ctx.vec(x)
    assert t.scatter(dev(idx[:100], dtype), ctx.vec(y), check=True) is t
    assert np.array_equal(bits(t.numpy()), bits(ref.scatter(x, idx[:100], y)[0]))
    t = ctx.vec(x)
    t.scatter(dev(idx[:100], dtype), ctx.vec(y))
    assert np.array_equal(bits(t.numpy()), bits(ref.scatter(x, idx[:100], y)[0]))
    # one index outside the vector, and only that one: counted, never used
    bad_idx = idx[:100].astype(np.int64); bad_idx[7] = 300 if dtype == np.int32 else 2 ** 32 + 5      # the 64-bit one would narrow to 5
    want_g, nbad = ref.gather(x, bad_idx)
    assert nbad == 1
    out = ctx.vec(100).fill(9.0)
    with pytest.raises(mg.MgsError) as e:
        dx.gather(dev(bad_idx, dtype), out=out, check=True)
    assert e.value.code == INVALID and e.value.bad == 1 and "1 of 100 indices" in str(e.value)
    got = out.numpy()
    assert bits(got[7]) == 0 and np.array_equal(bits(got), bits(want_g))
    out = ctx.vec(100).fill(9.0)
    dx.gather(dev(bad_idx, dtype), out=out)                                   # unchecked: the same result, nothing raised
    ctx.sync()
    assert np.array_equal(bits(out.numpy()), bits(want_g))
    want_s = ref.scatter(x, bad_idx, y)[0]
    t = ctx.vec(x)
    with pytest.raises(mg.MgsError) as e:
        t.scatter(dev(bad_idx, dtype), ctx.vec(y), check=True)
    assert e.value.code == INVALID and e.value.bad == 1
    assert np.array_equal(bits(t.numpy()), bits(want_s))
    t = ctx.vec(x)
    t.scatter(dev(bad_idx, dtype), ctx.vec(y))
    assert np.array_equal(bits(t.numpy()), bits(want_s))
    # refusals that need no index
    L = mg.lib()
    short = ctx.vec(50)
    ti = dev(idx, dtype)
    for rc in (L.mgs_vec_gather(dx.h, C.c_void_p(ti.data_ptr()), len(idx), 64 if dtype == np.int64 else 32, short.h, None),
               L.mgs_vec_scatter(short.h, C.c_void_p(ti.data_ptr()), len(idx), 64 if dtype == np.int64 else 32, dx.h, None)):
        assert rc == INVALID and "y holds 50 entries" in L.mgs_last_error(ctx.h).decode()
    assert L.mgs_vec_gather(dx.h, C.c_void_p(ti.data_ptr()), 10, 16, short.h, None) == INVALID and "index_bits 16" in L.mgs_last_error(ctx.h).decode()
    assert L.mgs_vec_gather(dx.h, C.c_void_p(ti.data_ptr()), -1, 32, short.h, None) == INVALID
    assert L.mgs_vec_gather(dx.h, None, 10, 32, short.h, None) == INVALID and L.mgs_vec_gather(dx.h, C.c_void_p(ti.data_ptr()), 10, 32, None, None) == INVALID
    assert np.array_equal(bits(dx.numpy()), bits(x))


# ------------------------------------------------------------------ 9. Dirichlet conditions end to end
def test_dirichlet_end_to_end(ctx, mg):
    """plane i = 0 of Poisson 8³ fixed to g: A_ff·x_f = b_f − A_fc·g solved with PCG on a hierarchy built on A_ff, the full vector put
    together with two scatters.  1e-8 on x, relative, is the project's bar for a solution."""
    A, fixed, free = ref.fx_poisson8()
    rng = np.random.default_rng(95)
    bh, g = rng.standard_normal(512), rng.standard_normal(64)
    dA = ctx.poisson3d(8)
    dfree, dfixed = dev(free), dev(fixed)
    Aff, Afc = dA.extract(dfree, dfree), dA.extract(dfree, dfixed)
    b, gv = ctx.vec(bh), ctx.vec(g)
    bf = b.gather(dfree).axpby(-1.0, Afc.spmv(gv), 1.0)                       # b_f − A_fc·g
    h = mg.Hierarchy(Aff, 0.6, 1, 1).coarsen(10.0, 2, 8.0, coarse_rows=60).finalize()
    assert h.nlev >= 2
    xf = ctx.vec(448)
    st, it, tol = mg.pcg(Aff, xf, bf, h, 200, 1e-10)
    assert st == 0 and tol <= 1e-10, (st, it, tol)
    x = ctx.vec(512).fill(7.0)
    x.scatter(dfree, xf).scatter(dfixed, gv)
    xh = x.numpy()
    assert np.array_equal(bits(xh[fixed]), bits(g)) and np.array_equal(bits(xh[free]), bits(xf.numpy()))
    Sff, Sfc = ref.to_scipy(ref.matrix(ref.extract(A, free, free))), ref.to_scipy(ref.matrix(ref.extract(A, free, fixed)))
    want = spla.spsolve(sps.csc_matrix(Sff), bh[free] - Sfc @ g)
    assert np.linalg.norm(xh[free] - want) <= 1e-8 * np.linalg.norm(want)


# ------------------------------------------------------------------ 10. a Schur complement composed on the device
def test_schur_complement_composed_on_the_device(ctx):
    """A_cc − A_cf·D_ff⁻¹·A_fc, D_ff the diagonal of A_ff: four blocks, a diagonal, a scaling, a product and a sum, held bit for bit to
    the same chain through the three restatements"""
    A = ref.fx_poisson8_values(0)
    _, c, f = ref.fx_poisson8()
    dA = up(ctx, A)
    dc, df = dev(c), dev(f)
    Acc, Acf, Afc, Aff = dA.extract(dc, dc), dA.extract(dc, df), dA.extract(df, dc), dA.extract(df, df)
    d = Aff.diagonal().numpy()
    hff = ref.matrix(ref.extract(A, f, f))
    assert len(d) == 448 and d.tobytes() == csr_algebra_ref.diag(hff).tobytes()
    dinv = 1.0 / d
    S = Acc.add(Acf.scale(right=ctx.vec(dinv)) @ Afc, 1.0, -1.0)
    hcc, hcf, hfc = (ref.matrix(ref.extract(A, r, q)) for r, q in ((c, c), (c, f), (f, c)))
    want = csr_algebra_ref.add(1.0, hcc, -1.0, spgemm_ref.spgemm(csr_algebra_ref.scale(hcf, None, dinv), hfc))
    assert_bits(S, want, "A_cc - A_cf D_ff^-1 A_fc")
    assert S.shape == (64, 64) and S.nnz >= Acc.nnz
