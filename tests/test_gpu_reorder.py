"""mgs_csr_permute / _numeric / _info and mgs_csr_bmat / _numeric / _info on the device against the host restatement of their contract
(tests/reorder_ref.py): rowptr and col as int32 arrays, val as uint64 arrays, all with np.array_equal.  tests/test_reorder_ref_cpu.py
shows that the restatement is scipy's A[rperm][:, cperm] and scipy.sparse.bmat and that every fixture has the property its test here
relies on (the 64 | 65 boundary, the chunk boundaries, the empty row, −0.0, the NaN's payload, stored zeros).  Index lists are placed
with torch and made visible with torch.cuda.synchronize().

The refusal of a result with 2³¹ − 1 entries or more cannot be reached at test size (it needs gigabytes of blocks): it is left to the
arithmetic of reorder_ref.bmat_refusal, which tests/test_reorder_ref_cpu.py checks at 2³¹ − 2, 2³¹ − 1 and 2³¹."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import extract_ref
import reorder_ref as ref

pytestmark = pytest.mark.gpu

OK, INVALID, STATE = 0, -1, -6
NOT_PERMUTED = {"lane_rows": 0, "wave_rows": 0, "max_row_len": 0, "map_bytes": 0}
NOT_ASSEMBLED = {"blocks": 0, "block_rows": 0, "block_cols": 0, "max_row_len": 0}


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
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def arrays(Cd):
    rp, ci, v = Cd.download()
    return np.asarray(rp, dtype=np.int32), np.asarray(ci, dtype=np.int32), bits(v)


def assert_bits(Cd, want, what=""):
    rp, ci, v = arrays(Cd)
    assert Cd.shape == (want[0], want[1]), what
    assert np.array_equal(rp, want[2]), what
    assert np.array_equal(ci, want[3]), what
    assert np.array_equal(v, bits(want[4])), what


def same_arrays(Xd, Yd):
    return all(np.array_equal(a, b) for a, b in zip(arrays(Xd), arrays(Yd)))


# ------------------------------------------------------------------ 1. permute against the restatement
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("name", sorted(ref.MATRICES))
def test_permute_matches_the_restatement(ctx, name, dtype):
    A = ref.MATRICES[name]()
    dA = up(ctx, A)
    lens = np.diff(A[2])
    for what, (rp, cp) in ref.lists(A[0], A[1]).items():
        Cd = dA.permute(dev(rp, dtype), dev(cp, dtype), keep_map=(what == "random_both"))
        assert_bits(Cd, ref.permute_ref(A, rp, cp), (name, what))
        info = Cd.permute_info()
        assert info == ref.permute_info(A, rp, cp, what == "random_both"), (name, what, info)
        if cp is not None:      # consistent with the row lengths: every row is served by exactly one arm
            assert info["lane_rows"] == int((lens <= 64).sum()) and info["wave_rows"] == int((lens > 64).sum()) and info["lane_rows"] + info["wave_rows"] == A[0]
        else:
            assert info["lane_rows"] == 0 and info["wave_rows"] == 0
        assert Cd.plan_info()["max_row_len"] == info["max_row_len"] == int(lens.max())
        assert Cd.nullspace() is None and Cd.origin() is None
        again = dA.permute(dev(rp, dtype), dev(cp, dtype), keep_map=(what == "random_both"))
        assert same_arrays(Cd, again), (name, what, "two identical calls")
    assert dA.permute_info() == NOT_PERMUTED and dA.bmat_info() == NOT_ASSEMBLED
    copy = dA.permute()
    assert same_arrays(copy, dA) and copy.device_ptrs() != dA.device_ptrs() and copy.permute_info()["max_row_len"] == int(lens.max())


def test_the_crafted_rows_run_on_both_arms(ctx):
    A = ref.fx_crafted()
    rp, cp = ref.lists(40, 330)["random_both"]
    Cd = up(ctx, A).permute(dev(rp), dev(cp))
    assert Cd.permute_info() == {"lane_rows": 36, "wave_rows": 4, "max_row_len": 300, "map_bytes": 0}
    got = arrays(Cd)
    v = got[2]
    assert (v == bits(-0.0)).sum() == 1 and (v == np.uint64(ref.NAN_BITS)).sum() == 1 and (v == 0).sum() == 2      # the zero's sign, the NaN's payload, the stored zeros


def test_index_width_and_list_forms(ctx, mg):
    A = ref.fx_crafted()
    dA = up(ctx, A)
    rp, cp = ref.lists(40, 330)["random_both"]
    assert same_arrays(dA.permute(dev(rp, np.int32), dev(cp, np.int32)), dA.permute(dev(rp, np.int64), dev(cp, np.int64)))
    with pytest.raises(TypeError):
        dA.permute(dev(rp, np.int32), dev(cp, np.int64))
    with pytest.raises(TypeError):
        dA.permute(dev(rp, np.int16))
    with pytest.raises(TypeError):
        dA.permute(rp)                                                       # a host array: nothing is converted
    with pytest.raises(ValueError):
        dA.permute(dev(rp[:-1]))                                             # the C call takes no length: the Python face compares it
    with pytest.raises(ValueError):
        dA.permute(None, dev(rp))


# ------------------------------------------------------------------ 2. round trip
@pytest.mark.parametrize("name", sorted(ref.MATRICES))
def test_round_trip_gives_the_source_bits(ctx, name):
    A = ref.MATRICES[name]()
    dA = up(ctx, A)
    p, q = ref.lists(A[0], A[1])["random_both"]
    back = dA.permute(dev(p), dev(q)).permute(dev(ref.inverse(p)), dev(ref.inverse(q)))
    assert same_arrays(back, dA)
    assert_bits(back, A, name)


# ------------------------------------------------------------------ 3. the vector identity on exact data
@pytest.mark.parametrize("name", sorted(ref.MATRICES))
def test_vector_identity_on_exact_data(ctx, name):
    A = ref.small_ints(ref.MATRICES[name](), 77)
    dA = up(ctx, A)
    p, q = ref.lists(A[0], A[1])["random_both"]
    dp, dq = dev(p), dev(q)
    Cd = dA.permute(dp, dq)
    x = np.random.default_rng(78).integers(-9, 10, A[1]).astype(np.float64)
    dx = ctx.vec(x)
    lhs = Cd.spmv(dx.gather(dq)).numpy()
    rhs = dA.spmv(dx).gather(dp).numpy()
    want = (ref.to_scipy(A) @ x)[p]
    assert np.array_equal(lhs, rhs) and np.array_equal(lhs, want) and np.abs(want).max() > 0


# ------------------------------------------------------------------ 4. refusals
def test_refusals_name_the_lowest_offender(ctx, mg):
    L = mg.lib()
    A = ref.fx_poisson5()
    dA = up(ctx, A)
    n = 125
    good = np.random.default_rng(4).permutation(n).astype(np.int64)

    def changed(at_value):
        out = good.copy()
        for k, v in at_value.items():
            out[k] = v
        return out

    def refused(r, c, dtype=np.int32):
        tr, tc = dev(r, dtype), dev(c, dtype)
        out = C.c_void_p(0x1234)
        rc = L.mgs_csr_permute(dA.h, C.c_void_p(tr.data_ptr()) if tr is not None else None, C.c_void_p(tc.data_ptr()) if tc is not None else None,
                               64 if dtype == np.int64 else 32, 0, C.byref(out))
        msg = L.mgs_last_error(ctx.h).decode()
        name, pos, value, kind = ref.refusal(A, r, c)
        assert rc == INVALID and out.value == 0x1234, (rc, msg)
        assert f"{name} index {value} at position {pos} of the {name} list" in msg, ((name, pos, value, kind), msg)
        assert ("is outside [0, 125)" if kind == "range" else "repeats the entry at position") in msg, (kind, msg)
        return msg

    refused(changed({17: -1}), None)                                         # negative
    refused(None, changed({40: 125}))                                        # ≥ n
    refused(changed({3: 2 ** 32 + 3}), None, np.int64)                       # would narrow to 3: compared as a 64-bit value
    refused(None, changed({3: 2 ** 32 + int(good[9])}), np.int64)            # ... and would then repeat position 9
    msg = refused(changed({60: int(good[20])}), good)                        # a repeat: position 60 holds what position 20 holds
    assert "position 20:" in msg, msg
    refused(changed({90: 500, 60: int(good[20])}), None)                     # a range error above a repeat: the repeat at 60 is named
    refused(changed({30: 500, 60: int(good[20])}), None)                     # a range error below a repeat: the range error at 30
    refused(changed({30: -7, 31: -8, 100: int(good[0])}), changed({2: 125}))   # several at once, both lists: the row list's lowest
    refused(good, changed({2: 125, 1: int(good[0])}))                        # the row list is clean: the column list's lowest
    out = C.c_void_p(0x1234)
    assert L.mgs_csr_permute(dA.h, None, None, 16, 0, C.byref(out)) == INVALID and "index_bits 16" in L.mgs_last_error(ctx.h).decode() and out.value == 0x1234
    assert L.mgs_csr_permute(dA.h, None, None, 32, 0, None) == INVALID
    shard = ctx.poisson3d(8, 2, 5, local_cols=True)                          # 192 x 320: owned columns, then two halo planes
    assert L.mgs_csr_permute(shard.h, None, None, 32, 0, C.byref(out)) == INVALID and out.value == 0x1234
    assert "row shard" in L.mgs_last_error(ctx.h).decode()
    # the Python face raises the same refusals
    with pytest.raises(mg.MgsError) as e:
        dA.permute(dev(changed({60: int(good[20])})), dev(good))
    assert e.value.code == INVALID and "position 60 " in str(e.value)
    # a valid call afterwards on the same context gives the right bits
    assert_bits(dA.permute(dev(good), dev(good)), ref.permute_ref(A, good, good), "the context still works")


# ------------------------------------------------------------------ 5. the values again through the kept map
@pytest.mark.parametrize("name", sorted(ref.MATRICES))
def test_permute_update_in_place(ctx, mg, name):
    A = ref.MATRICES[name]()
    rng = np.random.default_rng(5)
    for what in ("random_both", "random_rows", "reversal_cols"):
        rp, cp = ref.lists(A[0], A[1])[what]
        dA = up(ctx, A)
        Cd = dA.permute(dev(rp), dev(cp), keep_map=True)
        assert Cd.permute_info()["map_bytes"] == 4 * Cd.nnz
        ptrs = Cd.device_ptrs()
        new = rng.standard_normal(len(A[3]))
        new[::5] = -0.0
        A2 = ref.with_values(A, new)
        dA.update_values(new)
        assert Cd.permute_update(dA) is Cd and Cd.device_ptrs() == ptrs      # enqueued only, nothing moved
        assert_bits(Cd, ref.permute_ref(A2, rp, cp), (name, what, "new values, in place"))
        assert same_arrays(Cd, up(ctx, A2).permute(dev(rp), dev(cp)))


def test_permute_update_refusals(ctx, mg):
    A = ref.fx_crafted()
    rp, cp = ref.lists(40, 330)["random_both"]
    dA = up(ctx, A)
    plain, kept = dA.permute(dev(rp), dev(cp)), dA.permute(dev(rp), dev(cp), keep_map=True)
    for Cd in (plain, dA, mg.Csr.hstack(ctx, [dA, dA])):
        with pytest.raises(mg.MgsError) as e:
            Cd.permute_update(dA)
        assert e.value.code == STATE and "keeps no source map" in str(e.value)
    with pytest.raises(mg.MgsError) as e:
        kept.permute_update(up(ctx, ref.fx_poisson5()))
    assert e.value.code == INVALID and "125 x 125" in str(e.value)
    fewer = (A[0], A[1], np.minimum(A[2], len(A[3]) - 1).astype(np.int32), A[3][:-1], A[4][:-1])      # the last entry dropped
    with pytest.raises(mg.MgsError) as e:
        kept.permute_update(up(ctx, fewer))
    assert e.value.code == INVALID and f"{len(A[3]) - 1} entries" in str(e.value)
    L = mg.lib()
    assert L.mgs_csr_permute_numeric(None, kept.h) == INVALID and L.mgs_csr_permute_numeric(dA.h, None) == INVALID
    other = mg.Context(0)
    try:
        oA = up(other, A)
        with pytest.raises(mg.MgsError) as e:
            kept.permute_update(oA)
        assert e.value.code == INVALID and "different context" in str(e.value)
        del oA
    finally:
        other.close()
    assert_bits(kept, ref.permute_ref(A, rp, cp), "after the refused updates")
    # the extract's own update is untouched by the new call: a permuted matrix is no extract, an extracted one no permutation
    with pytest.raises(mg.MgsError) as e:
        kept.extract_update(dA)
    assert e.value.code == STATE
    block = dA.extract(keep_map=True)
    with pytest.raises(mg.MgsError) as e:
        block.permute_update(dA)
    assert e.value.code == STATE
    assert block.extract_update(dA) is block and same_arrays(block, dA)


def agg_P(g, nc):
    ok = g >= 0
    return sps.csr_matrix((np.ones(int(ok.sum())), (np.flatnonzero(ok), g[ok])), shape=(len(g), nc))


def test_permute_update_then_the_hierarchy_refreshes(ctx, mg):
    A1, A2 = extract_ref.fx_poisson8_values(0), extract_ref.fx_poisson8_values(1)
    p = np.random.default_rng(88).permutation(512)
    dA = up(ctx, A1)
    Cd = dA.permute(dev(p), dev(p), keep_map=True)
    ptrs = Cd.device_ptrs()
    h = mg.Hierarchy(Cd, 0.6, 1, 1).coarsen(10.0, 2, 8.0, coarse_rows=40).finalize()
    assert h.nlev >= 2
    b = ctx.vec(512).rand(seed=11); x = ctx.vec(512)
    h.vcycle(b, x); h.vcycle(b, x)
    x1 = x.numpy()
    dA.update_values(A2[4])
    assert Cd.permute_update(dA) is Cd and Cd.device_ptrs() == ptrs
    h.refresh()
    assert h.refresh_info()["kept_graphs"] == 1, h.refresh_info()
    h.vcycle(b, x)
    fresh = up(ctx, A2).permute(dev(p), dev(p))
    assert same_arrays(Cd, fresh)
    assert_bits(Cd, ref.permute_ref(A2, p, p), "the refreshed operator")
    h2 = mg.Hierarchy(fresh, 0.6, 1, 1)
    for l in range(h.nlev - 1):
        P = agg_P(h.level_P(l).agg(), h.level_shape(l + 1)[0])
        h2.push_P(ctx.csr(P.shape[0], P.shape[1], P.indptr, P.indices, P.data))
    h2.finalize()
    x2 = h2.vcycle(b).numpy()
    assert np.isfinite(x2).all() and np.linalg.norm(x2) > 0 and not np.array_equal(x1, x2)
    assert np.array_equal(x.numpy(), x2)


# ------------------------------------------------------------------ 6. bmat against the restatement
def on_device(ctx, mats, grid):
    d = {k: up(ctx, M) for k, M in mats.items() if any(k in row for row in grid)}
    return d, [[d[b] if b is not None else None for b in row] for row in grid]


@pytest.mark.parametrize("name", sorted(ref.bmat_fixtures()))
def test_bmat_matches_the_restatement(ctx, mg, name):
    mats, grid, rs, cs = ref.bmat_fixtures()[name]
    G = ref.resolve(mats, grid)
    d, dgrid = on_device(ctx, mats, grid)
    want = ref.bmat_ref(G, rs, cs)
    Cd = mg.Csr.bmat(ctx, dgrid, rs, cs)
    assert_bits(Cd, want, name)
    assert Cd.bmat_info() == ref.bmat_info(G, rs, cs) and Cd.plan_info()["max_row_len"] == Cd.bmat_info()["max_row_len"]
    assert Cd.permute_info() == NOT_PERMUTED and Cd.nullspace() is None and Cd.origin() is None
    assert same_arrays(Cd, mg.Csr.bmat(ctx, dgrid, rs, cs)), "two identical calls"
    if name == "hstack":
        assert same_arrays(Cd, mg.Csr.hstack(ctx, dgrid[0]))
    if name == "vstack":
        assert same_arrays(Cd, mg.Csr.vstack(ctx, [row[0] for row in dgrid]))
    if name == "block_diag":
        assert same_arrays(Cd, mg.Csr.block_diag(ctx, [dgrid[k][k] for k in range(3)]))
    # an ordinary matrix: pattern code, SpMV (tagged values: the fixture's NaN would spoil the comparison)
    T = ref.with_values(want, np.arange(1, len(want[3]) + 1, dtype=np.float64))
    x = np.random.default_rng(6).integers(-3, 4, want[1]).astype(np.float64)
    Cd.update_values(T[4])
    assert np.array_equal(Cd.optimize().spmv(ctx.vec(x)).numpy(), ref.to_scipy(T) @ x)


def test_bmat_update_in_place(ctx, mg):
    mats, grid, rs, cs = ref.bmat_fixtures()["same_handle_twice"]
    d, dgrid = on_device(ctx, mats, grid)
    Cd = mg.Csr.bmat(ctx, dgrid)
    ptrs = Cd.device_ptrs()
    new = np.random.default_rng(61).standard_normal(len(mats["L"][3]))
    new[::7] = -0.0
    d["L"].update_values(new)                                               # L sits in two places: both change
    mats2 = dict(mats, L=ref.with_values(mats["L"], new))
    assert Cd.bmat_update(dgrid) is Cd and Cd.device_ptrs() == ptrs
    want = ref.bmat_ref(ref.resolve(mats2, grid))
    assert_bits(Cd, want, "new values of one block, in place")
    assert same_arrays(Cd, mg.Csr.bmat(ctx, dgrid))
    # other handles of the same shapes and entry counts: the table is rewritten
    new2 = np.random.default_rng(62).standard_normal(len(mats["D1"][3]))
    mats3 = dict(mats2, D1=ref.with_values(mats["D1"], new2))
    _, dgrid3 = on_device(ctx, mats3, grid)
    assert Cd.bmat_update(dgrid3) is Cd and Cd.device_ptrs() == ptrs
    assert_bits(Cd, ref.bmat_ref(ref.resolve(mats3, grid)), "other handles")
    assert Cd.bmat_update(dgrid) is Cd
    assert_bits(Cd, want, "the first handles again")
    # a matrix with a NULL block and an all-NULL block row
    mats, grid, rs, cs = ref.bmat_fixtures()["null_block_row"]
    d, dgrid = on_device(ctx, mats, grid)
    Cd = mg.Csr.bmat(ctx, dgrid, rs, cs)
    new = np.random.default_rng(63).standard_normal(len(mats["T"][3]))
    d["T"].update_values(new)
    Cd.bmat_update(dgrid)
    assert_bits(Cd, ref.bmat_ref(ref.resolve(dict(mats, T=ref.with_values(mats["T"], new)), grid), rs, cs), "null block row")


def test_bmat_refusals_name_the_block(ctx, mg):
    L = mg.lib()
    mats = ref.bmat_fixtures()["hstack"][0]
    d = {k: up(ctx, mats[k]) for k in ("R", "S", "T", "L")}
    R, S, T = d["R"], d["S"], d["T"]

    def refused(grid, words, rs=None, cs=None):
        assert ref.bmat_refusal([[mats[next(k for k in d if d[k] is b)] if b is not None else None for b in row] for row in grid], rs, cs) is not None
        with pytest.raises(mg.MgsError) as e:
            mg.Csr.bmat(ctx, grid, rs, cs)
        assert e.value.code == INVALID
        for w in words:
            assert w in str(e.value), str(e.value)

    refused([[R, T]], ["block (0, 1)", "10 rows", "block row 0 has 37"])                     # mismatched sizes
    refused([[R], [S]], ["block (1, 0)", "29 columns", "block column 0 has 53"])
    refused([[R, S]], ["block (0, 0)", "37 rows", "has 36"], rs=[36])                         # a given size that disagrees
    refused([[R, S], [None, None]], ["block row 1", "row_sizes"])                             # a missing size
    refused([[R, None], [T, None]], ["block column 1", "col_sizes"])
    refused([[d["L"]] * 257], ["257", "MGS_BMAT_MAX_BLOCKS"])                                # br·bc = 257
    out = C.c_void_p(0x1234)
    one = (C.c_void_p * 1)(R.h)
    assert L.mgs_csr_bmat(ctx.h, 0, 1, one, None, None, C.byref(out)) == INVALID and out.value == 0x1234
    assert L.mgs_csr_bmat(ctx.h, 1, 1, None, None, None, C.byref(out)) == INVALID and L.mgs_csr_bmat(ctx.h, 1, 1, one, None, None, None) == INVALID
    shard = ctx.poisson3d(8, 2, 5, local_cols=True)
    with pytest.raises(mg.MgsError) as e:
        mg.Csr.bmat(ctx, [[R], [shard]])
    assert e.value.code == INVALID and "block (1, 0)" in str(e.value) and "row shard" in str(e.value)
    other = mg.Context(0)
    try:
        oS = up(other, mats["S"])
        with pytest.raises(mg.MgsError) as e:
            mg.Csr.bmat(ctx, [[R, oS]])
        assert e.value.code == INVALID and "block (0, 1)" in str(e.value) and "different context" in str(e.value)
        Cd = mg.Csr.bmat(ctx, [[R, S], [T, None]])
        with pytest.raises(mg.MgsError) as e:
            Cd.bmat_update([[R, oS], [T, None]])
        assert e.value.code == INVALID and "block (0, 1)" in str(e.value) and "different context" in str(e.value)
        del oS
    finally:
        other.close()
    # changed blocks in the values-only pass: NULL-ness, shape, entry count
    want = ref.bmat_ref([[mats["R"], mats["S"]], [mats["T"], None]])
    with pytest.raises(mg.MgsError) as e:
        Cd.bmat_update([[R, S], [None, None]])
    assert e.value.code == INVALID and "block (1, 0)" in str(e.value) and "NULL" in str(e.value)
    with pytest.raises(mg.MgsError) as e:
        Cd.bmat_update([[R, S], [T, T]])
    assert e.value.code == INVALID and "block (1, 1)" in str(e.value)
    with pytest.raises(mg.MgsError) as e:
        Cd.bmat_update([[S, S], [T, None]])
    assert e.value.code == INVALID and "block (0, 0)" in str(e.value) and "37 x 29" in str(e.value) and "37 x 53" in str(e.value)
    M = mats["R"]
    fewer = (M[0], M[1], np.minimum(M[2], len(M[3]) - 1).astype(np.int32), M[3][:-1], M[4][:-1])
    with pytest.raises(mg.MgsError) as e:
        Cd.bmat_update([[up(ctx, fewer), S], [T, None]])
    assert e.value.code == INVALID and "block (0, 0)" in str(e.value) and f"{len(M[3]) - 1} entries" in str(e.value)
    for wrong in ([[R]], [[R, S]], [[R, S], [T, None], [T, None]], [[R, S, S], [T, None, None]]):      # another grid than C's 2 x 2: refused before the C call,
        with pytest.raises(ValueError) as e:                                                          # which takes no dimensions and would read 4 handles
            Cd.bmat_update(wrong)
        assert "2 x 2" in str(e.value), str(e.value)
    with pytest.raises(mg.MgsError) as e:
        R.bmat_update([[R]])                                                # a matrix that mgs_csr_bmat did not build
    assert e.value.code == INVALID and "not built by mgs_csr_bmat" in str(e.value)
    with pytest.raises(mg.MgsError) as e:
        R.permute(keep_map=True).bmat_update([[R]])
    assert e.value.code == INVALID
    assert_bits(Cd, want, "after the refused updates")
    assert_bits(mg.Csr.bmat(ctx, [[R, S], [T, None]]), want, "the context still works")


# ------------------------------------------------------------------ 7. the two-field use, end to end
def test_two_fields_end_to_end(ctx, mg):
    """K = [[L, c·I], [c·I, L]] assembled on the device, renumbered to the interleaved order and back, and solved with PCG whose
    preconditioner is a hierarchy on block_diag(L, L): the unknown-based AMG of a coupled system.  The residual is recomputed on the
    host from the downloaded x: the solver decides on its own true residual at 1e-8, and the host's differs from it by rounding of
    order n·2⁻⁵³·‖K‖‖x‖/‖b‖, six orders below — hence 2e-8."""
    Lh, cIh, Kh, p = ref.fx_two_field()
    n = Lh[0]
    dL = ctx.poisson3d(6)
    assert_bits(dL, Lh, "the fixture is mgs_csr_poisson3d's operator")
    dcI = mg.Csr.from_diag(ctx, ctx.vec(np.full(n, ref.COUPLING)))
    K = mg.Csr.bmat(ctx, [[dL, dcI], [dcI, dL]])
    assert_bits(K, Kh, "K")
    dp, dpinv = dev(p), dev(ref.inverse(p))
    Ki = K.permute(dp, dp)
    assert_bits(Ki, ref.permute_ref(Kh, p, p), "K interleaved")
    back = Ki.permute(dpinv, dpinv)
    assert same_arrays(back, K)
    BD = mg.Csr.block_diag(ctx, [dL, dL])
    h = mg.Hierarchy(BD, 0.6, 1, 1).coarsen(10.0, 2, 8.0, coarse_rows=40).finalize()
    assert h.nlev >= 2
    # no aggregate holds rows of both fields, on any level
    field = (np.arange(2 * n) >= n).astype(np.int64)
    for l in range(h.nlev - 1):
        g = np.asarray(h.level_P(l).agg())
        nc = h.level_shape(l + 1)[0]
        ok = g >= 0
        lo = np.full(nc, 2, dtype=np.int64); hi = np.full(nc, -1, dtype=np.int64)
        np.minimum.at(lo, g[ok], field[ok]); np.maximum.at(hi, g[ok], field[ok])
        assert ok.any() and (lo == hi).all(), f"level {l}: an aggregate holds rows of both fields"
        field = lo
    bh = np.random.default_rng(216).standard_normal(2 * n)
    b, x = ctx.vec(bh), ctx.vec(2 * n)
    st, it, tol = mg.pcg(K, x, b, h, 200, 1e-8)
    assert st == 0, (st, it, tol)
    xh = x.numpy()
    res = np.linalg.norm(bh - ref.to_scipy(Kh) @ xh) / np.linalg.norm(bh)
    print(f"two fields: pcg {it} iterations, reported {tol:.3e}, host residual {res:.3e}")
    assert res < 2e-8, res
