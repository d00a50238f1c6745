"""The C++ face (multigridsolver_amd/cpp/mgs_host.hpp) on the device, every wrapper against the Python face over the same C ABI.

One program per family (tests/cpp_face/*.cpp, compiled once per session) reads the files written here, runs once and writes raw files; the same
operations run in this process through multigridsolver_amd/core.py on the same files, and every output is compared bit for bit
(tests/cpp_face.py: compare).  Both faces call the same kernels with the same launch decisions and the library is deterministic, so equality is
the bar; statuses, iteration counts, written-back tolerances and info vectors are compared with ==.

Where the Python face has no counterpart the expected value is stated here: the error codes of refusals the header raises itself
(bmatUpdate's grid, update_values' pattern), the counts a checked call writes when it succeeds (0), and the sizes of an empty Vector.  The
vector family runs on integer-valued data, so its element-access results are also known exactly without any library and are asserted so.

The generic templates CGiml<...> and MINRESiml<...> run other arithmetic than the fused paths (temporaries, unfused updates): they are held to
status 0, the oracle's true residual <= 1.5·tol (the margin of test_cpp_dropin_driver) and an iteration count <= it_fast + max(4, it_fast // 4)
(the margin of test_device_agmg_hierarchy); both counts are printed."""
import shutil

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import cpp_face as F
from minres_ref import saddle, saddle_rhs

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -6
TOL = 1e-8


@pytest.fixture(autouse=True)
def no_device_work_after_a_dead_child():
    F.fail_if_a_child_died()


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    return F.compile_all(tmp_path_factory.mktemp("cpp_face_gpu"))


def dev(a, dtype):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to("cuda:0")
    torch.cuda.synchronize()
    return t


def write_csr(mg, path, M):
    M = M.tocsr(); M.sort_indices()
    mg.write_mtx(str(path), M.shape[0], M.shape[1], M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64))


def host_csr(mg, path):
    n, m, rp, ci, v = mg.read_mtx(str(path))
    return sps.csr_matrix((v, ci, rp), shape=(n, m))


def random_csr(rng, rows, cols, density, empty=()):
    """values that round in every product, sorted columns, the rows of `empty` without an entry"""
    mask = rng.random((rows, cols)) < density
    mask[list(empty), :] = False
    M = sps.csr_matrix(np.where(mask, rng.standard_normal((rows, cols)), 0.0))
    M.sort_indices()
    return M


def other_values(rng, M):
    M2 = M.copy(); M2.data = rng.standard_normal(M.nnz)
    return M2


def go(exes, family, d):
    out = d / "out"
    print(F.run(exes[family], family, d, out)[-1500:])
    return F.read_outputs(out)


def poisson_files(mg, ctx, d, n2d=32):
    """A2d.mtx: the library's own 2-D Poisson operator at 32², downloaded and written out"""
    A = ctx.poisson2d(n2d)
    rp, ci, v = A.download()
    mg.write_mtx(str(d / "A2d.mtx"), n2d * n2d, n2d * n2d, rp, ci, v)
    return rp, ci, v


def saddle_files(mg, orc, d):
    """the 6³ saddle system of tests/test_gpu_minres.py: K, block_diag(L, S) and the oracle's aggregation of L with empty rows below it for S"""
    sd = saddle(6)
    Bd = sps.block_diag([sd["L"], sd["S"]], format="csr")
    PL = orc.Csr.from_scipy(sd["L"]).agmg(10.0, 2, 8.0, strict=False).to_scipy()
    Pd = sps.vstack([PL, sps.csr_matrix((sd["m"], PL.shape[1]))], format="csr")
    write_csr(mg, d / "K.mtx", sd["K"]); write_csr(mg, d / "Bd.mtx", Bd); write_csr(mg, d / "Pd.mtx", Pd)
    b = saddle_rhs(sd["K"].shape[0])
    F.write_f64(d / "bK.f64", b)
    return b


def saddle_hierarchy(mg, ctx, d, nu1=1):
    B, P = mg.Csr.from_mtx(ctx, str(d / "Bd.mtx")), mg.Csr.from_mtx(ctx, str(d / "Pd.mtx"))
    return mg.Hierarchy(B, 0.6, nu1, 1).push_P(P).coarsen(10.0, 2, 8.0, 2500, 32).finalize()


def hierarchy(mg, A, nu1=1, nu2=1, P=None):
    h = mg.Hierarchy(A, 0.6, nu1, nu2)
    if P is not None:
        h.push_P(P)
    return h.coarsen(10.0, 2, 8.0, 50, 32).finalize()


# ------------------------------------------------------------------------------------------------------ 1. Vector and its host mirror
def test_vector_and_host_mirror(mg, ctx, exes, tmp_path):
    n = 1030                                                   # two workgroups of the 16-byte kernels and a tail
    rng = np.random.default_rng(11)
    a, b = rng.integers(-50, 51, n).astype(np.float64), rng.integers(-50, 51, n).astype(np.float64)
    c, d = rng.standard_normal(n), rng.standard_normal(n)
    for name, arr in (("a", a), ("b", b), ("c", c), ("d", d)):
        F.write_f64(tmp_path / (name + ".f64"), arr)
    cpp = go(exes, "vector", tmp_path)

    V = ctx.vec
    add = lambda x, y: V(len(x)).axpbypcz(1.0, x, 1.0, y, 0.0)          # noqa: E731  operator+
    sub = lambda x, y: V(len(x)).axpbypcz(1.0, x, -1.0, y, 0.0)         # noqa: E731  operator-
    mul = lambda s, x: V(len(x)).axpby(s, x, 0.0)                       # noqa: E731  operator*

    def written(src, **at):
        w = src.copy()
        for i, val in at.items():
            w[int(i[1:])] = val
        return w
    py = F.Record()
    va, vb = V(a), V(b)
    a1 = written(a, _3=7.0); a1[n - 1] = -2.0
    py.vec("write_then_op", add(V(a1), vb))
    v = V(a).axpby(1.0, vb, 1.0)
    py["read_before_op"], py["read_after_op"], py["read_after_op_const"] = float(a[0]), float(v.numpy()[0]), float(v.numpy()[n - 2])
    py.vec("op_then_read", v)
    py.vec("copy_construct", V(n).copy_from(V(written(a, _1=99.0))))
    py.vec("copy_construct_source", written(a, _1=99.0))
    py.vec("copy_construct_written", written(a, _1=99.0, _2=-5.0))
    py["copy_assign_read"] = float(a[2]); py.vec("copy_assign", V(n).copy_from(va))
    py.vec("self_assign", written(b, _4=6.0))
    py.vec("move_construct", written(a, _4=-8.0))
    py["move_assign_read"] = 11.0; py.vec("move_assign", written(b, _0=11.0))
    s = V(written(a, _0=4.0)); s.axpby(1.0, s, 1.0)
    py.vec("self_add", s)
    s.axpby(-1.0, s, 1.0); py.vec("self_sub", s)
    py.vec("set_zero_after_write", V(written(a, _3=5.0)).fill(0.0)); py["set_zero_read"] = 0.0
    u = V(written(np.zeros(n), _2=9.0)).upload(b)
    py.vec("upload_after_write", u)
    py.vec("upload_after_write_then_op", u.axpby(1.0, va, 1.0))
    py["const_read_before"], py["const_read_after_upload"], py["const_read_after_zero"], py["const_read_after_out"] = float(a[2]), float(b[2]), 0.0, float(a[2])
    py.vec("download_pending", V(written(a, _6=42.0)))
    e = V(0)
    py["empty_size"], py["none_size"], py["empty_download"] = len(e), 0, e.numpy().size
    py["empty_copy_size"], py["none_copy_size"] = len(mg.Vec(ctx, 0).copy_from(e)), 0
    e.fill(0.0)
    vc, vd = V(c), V(d)
    py.vec("plus", add(vc, vd)); py.vec("minus", sub(vc, vd))
    py.vec("scaled_left", mul(2.5, vc)); py.vec("scaled_right", mul(-0.3, vd))
    py.vec("plus_assign", V(n).copy_from(vc).axpby(1.0, vd, 1.0)); py.vec("minus_assign", V(n).copy_from(vc).axpby(-1.0, vd, 1.0))
    py.vec("chain", sub(add(vc, mul(0.7, vd)), mul(1.1, sub(vc, vd))))
    py["dot"], py["dot_free"], py["norm"], py["norm_free"], py["dot_int"] = vc.dot(vd), vd.dot(vc), vc.nrm2(), vd.nrm2(), va.dot(vb)
    F.compare(cpp, py)
    # integer data: the same results without any library
    assert np.array_equal(cpp["write_then_op"], a1 + b) and np.array_equal(cpp["op_then_read"], a + b) and cpp["read_after_op"] == a[0] + b[0]
    assert np.array_equal(cpp["copy_assign"], a) and np.array_equal(cpp["self_add"], 2.0 * written(a, _0=4.0)) and not cpp["self_sub"].any()
    assert not cpp["set_zero_after_write"].any() and np.array_equal(cpp["upload_after_write"], b) and np.array_equal(cpp["upload_after_write_then_op"], a + b)
    assert cpp["dot_int"] == float(a @ b) and cpp["empty_size"] == 0 and cpp["empty_download"] == 0


# ------------------------------------------------------------------------------------------------------ 2. matrix algebra
def test_matrix_algebra(mg, ctx, exes, tmp_path):
    rng = np.random.default_rng(23)
    n, k = 300, 170
    Rm = random_csr(rng, n, n, 0.03, empty=(0, 17, 299))
    Bm = random_csr(rng, n, k, 0.04, empty=(3,)).tolil()
    Bm[5, 5] = 1.0; Bm[6, 6] = 0.0
    Bm = Bm.tocsr(); Bm.sort_indices()
    Bm.data[Bm.indptr[5] + int(np.searchsorted(Bm.indices[Bm.indptr[5]:Bm.indptr[6]], 5))] = 0.0      # a stored zero on the diagonal
    assert not Bm[6, :].indices.tolist().count(6)                                                      # and a diagonal entry that is not stored
    R2m, B2m = other_values(rng, Rm), other_values(rng, Bm)
    for name, M in (("R", Rm), ("B", Bm), ("R2", R2m), ("B2", B2m)):
        write_csr(mg, tmp_path / (name + ".mtx"), M)
    back = host_csr(mg, tmp_path / "B.mtx")
    assert back.nnz == Bm.nnz and np.array_equal(back.indices, Bm.indices) and 0.0 in back.data      # the file keeps the stored zero (both faces read the file's values)
    assert np.array_equal(host_csr(mg, tmp_path / "R2.mtx").indices, Rm.indices)
    vecs = {"dl": rng.uniform(0.5, 2.0, n), "dr": rng.uniform(0.5, 2.0, n), "dlB": rng.uniform(0.5, 2.0, n), "drB": rng.uniform(0.5, 2.0, k), "x": rng.standard_normal(n)}
    rows = np.r_[rng.permutation(n)[:90], [17, 17, 4, 0]]                                  # any order, repeats, empty rows
    cols = np.sort(rng.permutation(k)[:60])                                                # strictly ascending, inside both matrices
    rperm, cperm = rng.permutation(n), rng.permutation(n)
    gidx = rng.permutation(n)[:120]                                                        # distinct: scatter is then determined
    lists = {"rows": rows, "cols": cols, "rperm": rperm, "cperm": cperm, "gidx": gidx}
    for name, arr in vecs.items():
        F.write_f64(tmp_path / (name + ".f64"), arr)
    for name, arr in lists.items():
        F.write_i32(tmp_path / (name + ".i32"), arr)
    cpp = go(exes, "algebra", tmp_path)

    Csr = mg.Csr
    R, B = Csr.from_mtx(ctx, str(tmp_path / "R.mtx")), Csr.from_mtx(ctx, str(tmp_path / "B.mtx"))
    t32 = {name: dev(arr, np.int32) for name, arr in lists.items()}
    t64 = {name: dev(arr, np.int64) for name, arr in lists.items()}
    py = F.Record()
    C = R.matmul(B); py.csr("multiply", C)
    Rt, Bt = R.transpose(), B.transpose()
    py.csr("transpose", Bt); py.csr("transpose_square", Rt)
    S = R.add(Rt, 2.5, -0.75); py.csr("add", S)
    py.csr("add_default", R.add(Rt))
    py.vec("diagonal", B.diagonal()); py.vec("diagonal_t", Bt.diagonal())
    py.csr("from_diagonal", Csr.from_diag(ctx, B.diagonal()))
    Eb = R.extract(t64["rows"], t64["cols"], keep_map=True)
    py.csr("extract_rows", R.extract(rows=t32["rows"])); py.csr("extract_cols", B.extract(cols=t32["cols"])); py.csr("extract_both64", Eb)
    py.csr("extract_all", B.extract())
    Pm = R.permute(t32["rperm"], t32["cperm"], keep_map=True)
    py.csr("permute", Pm); py.csr("permute_cols64", R.permute(cols=t64["cperm"])); py.csr("permute_rows", R.permute(rows=t32["rperm"]))
    K1 = Csr.bmat(ctx, [[R, B], [Bt, None]])
    py.csr("bmat", K1); py.csr("bmat_same_block", Csr.bmat(ctx, [[R, R], [None, R]]))
    py.csr("bmat_null_row", Csr.bmat(ctx, [[R, B], [None, None]], row_sizes=[n, 40]))
    X, Y = Csr.from_mtx(ctx, str(tmp_path / "R.mtx")), Csr.from_mtx(ctx, str(tmp_path / "B.mtx"))
    py.csr("scale_left", X.scale(left=ctx.vec(vecs["dl"]))); py.csr("scale_right", X.scale(right=ctx.vec(vecs["dr"])))
    py.csr("scale_both", Y.scale(ctx.vec(vecs["dlB"]), ctx.vec(vecs["drB"])))
    dlB = vecs["dlB"].copy(); dlB[1] = 3.0
    py.csr("scale_after_write", Y.scale(left=ctx.vec(dlB)))
    x = ctx.vec(vecs["x"])
    y = x.gather(t32["gidx"]); py.vec("gather", y)
    y64 = x.gather(t64["gidx"], check=True); py.vec("gather64", y64); py["gather64_bad"] = 0
    py.vec("scatter", ctx.vec(n).scatter(t32["gidx"], y, check=True)); py["scatter_bad"] = 0
    py.vec("scatter64", ctx.vec(n).scatter(t64["gidx"], y64))
    py.vec("spmv", Bt.spmv(x))
    R.update_values(mg.read_mtx(str(tmp_path / "R2.mtx"))[4]); B.update_values(mg.read_mtx(str(tmp_path / "B2.mtx"))[4])
    py.csr("multiply_update", C.matmul_update(R, B))
    py.csr("multiply_update_checked", C.matmul_update(R, B, check=True)); py["multiply_misses"] = 0
    Bt.transpose_update(B); Rt.transpose_update(R, check=True)
    py.csr("transpose_update", Bt); py.csr("transpose_update_checked", Rt); py["transpose_misses"] = 0
    py.csr("add_update", S.add_update(R, Rt, 1.5, -3.25, check=True)); py["add_misses"] = 0
    py.csr("add_update_default", S.add_update(R, Rt))
    py.csr("extract_update", Eb.extract_update(R)); py.csr("permute_update", Pm.permute_update(R))
    py.csr("bmat_update", K1.bmat_update([[R, B], [Bt, None]]))
    F.compare(cpp, py)
    # the cached shapes, stated: a rectangular product, a transpose, blocks by list length and by NULL list, the assembled grid
    shapes = {"multiply": (n, k), "transpose": (k, n), "from_diagonal": (k, k), "extract_rows": (len(rows), n), "extract_cols": (n, len(cols)),
              "extract_both64": (len(rows), len(cols)), "extract_all": (n, k), "bmat": (n + k, n + k), "bmat_null_row": (n + 40, n + k)}
    for name, (r, c) in shapes.items():
        assert (cpp[name + ".rows"], cpp[name + ".cols"]) == (r, c) == (cpp[name + ".lib_rows"], cpp[name + ".lib_cols"]), name
    assert cpp["diagonal"].size == k and cpp["diagonal"][5] == 0.0 and cpp["diagonal"][6] == 0.0 and cpp["from_diagonal.val"].size == k
    assert not np.array_equal(cpp["add_update.val"], cpp["add_update_default.val"]) and not np.array_equal(cpp["multiply.val"], cpp["multiply_update.val"])


# ------------------------------------------------------------------------------------------------------ 3. ingest
def test_ingest_from_device_memory(mg, ctx, exes, tmp_path):
    rng = np.random.default_rng(31)
    rp, ci, v = poisson_files(mg, ctx, tmp_path)
    n = len(rp) - 1
    val = rng.standard_normal(len(ci))
    nt = 3000
    trow, tcol = rng.integers(0, n, nt), rng.integers(0, n + 3, nt)
    trow[nt - 300:], tcol[nt - 300:] = trow[:300], tcol[:300]                               # duplicates, far from their first occurrence
    tval, tval2 = rng.standard_normal(nt), rng.standard_normal(nt)
    d = np.sqrt(rng.uniform(0.5, 2.0, n)); rows_of = np.repeat(np.arange(n), np.diff(rp))
    v2 = v * d[rows_of] * d[ci]
    shutil.copy(str(tmp_path / "A2d.mtx"), str(tmp_path / "A.mtx"))
    mg.write_mtx(str(tmp_path / "A2.mtx"), n, n, rp, ci, v2)
    F.write_i32(tmp_path / "rp.i32", rp); F.write_i32(tmp_path / "ci.i32", ci); F.write_i32(tmp_path / "trow.i32", trow); F.write_i32(tmp_path / "tcol.i32", tcol)
    F.write_f64(tmp_path / "val.f64", val); F.write_f64(tmp_path / "tval.f64", tval); F.write_f64(tmp_path / "tval2.f64", tval2)
    cpp = go(exes, "ingest", tmp_path)

    Csr = mg.Csr
    py = F.Record()
    dval, dtval, dtval2 = ctx.vec(val), ctx.vec(tval), ctx.vec(tval2)
    py.csr("from_device32", Csr.from_device(ctx, n, n, dev(rp, np.int32), dev(ci, np.int32), dval))
    py.csr("from_device64", Csr.from_device(ctx, n, n, dev(rp, np.int64), dev(ci, np.int64), dval))
    py.csr("from_coo32", Csr.from_coo_device(ctx, n, n + 3, dev(trow, np.int32), dev(tcol, np.int32), dtval))
    T = Csr.from_coo_device(ctx, n, n + 3, dev(trow, np.int64), dev(tcol, np.int64), dtval, keep_map=True)
    py.csr("from_coo64_kept", T)
    py.csr("update_values_coo", T.update_values_coo(dtval2))
    py.vec("coo_row_sums", T.spmv(ctx.vec(np.ones(n + 3))))
    A = Csr.from_mtx(ctx, str(tmp_path / "A.mtx"))
    py.csr("update_values", A.update_values(mg.read_mtx(str(tmp_path / "A2.mtx"))[4]))
    py["written.nonzeros"] = len(ci)
    F.compare(cpp, py)
    mg.write_mtx(str(tmp_path / "A2_python.mtx"), n, n, *mg.read_mtx(str(tmp_path / "A2.mtx"))[2:])
    assert open(str(tmp_path / "out" / "A2_written.mtx")).read() == open(str(tmp_path / "A2_python.mtx")).read()      # writeMatrix
    assert np.array_equal(cpp["from_device64.val"], val) and (cpp["from_coo32.rows"], cpp["from_coo32.cols"]) == (n, n + 3)
    assert cpp["from_coo32.val"].size < nt and not np.array_equal(cpp["update_values_coo.val"], cpp["from_coo64_kept.val"])


# ------------------------------------------------------------------------------------------------------ 4. preconditioner
def neumann2d(n):
    """the graph Laplacian of the n × n grid: A·1 = 0"""
    t = sps.diags([-np.ones(n - 1), np.r_[1.0, 2.0 * np.ones(n - 2), 1.0], -np.ones(n - 1)], [-1, 0, 1], format="csr")
    e = sps.eye(n, format="csr")
    return (sps.kron(t, e) + sps.kron(e, t)).tocsr()


def test_preconditioner_options(mg, ctx, exes, inputs, tmp_path):
    rng = np.random.default_rng(41)
    poisson_files(mg, ctx, tmp_path)
    rp, ci, v = ctx.poisson3d(8).download()
    mg.write_mtx(str(tmp_path / "A3d.mtx"), 512, 512, rp, ci, v)
    shutil.copy(inputs["poisson10000"], str(tmp_path / "A10k.mtx")); shutil.copy(inputs["poisson10000promatrix"], str(tmp_path / "P10k.mtx"))
    write_csr(mg, tmp_path / "N.mtx", neumann2d(24))
    v2, v3, v10k = rng.standard_normal(1024), rng.standard_normal(512), rng.standard_normal(10000)
    bN = rng.standard_normal(576); bN -= bN.mean()
    for name, arr in (("v2d", v2), ("v3d", v3), ("v10k", v10k), ("bN", bN)):
        F.write_f64(tmp_path / (name + ".f64"), arr)
    cpp = go(exes, "precond", tmp_path)

    Csr = mg.Csr
    py = F.Record()

    def cycle(name, h, vec, symmetric=True):
        py.vec(name, h.vcycle(vec)); py[name + ".levels"] = h.nlev; py[name + ".precision0"] = h.operand_precision(0); py[name + ".symmetric"] = int(symmetric)
    A2, A3 = Csr.from_mtx(ctx, str(tmp_path / "A2d.mtx")), Csr.from_mtx(ctx, str(tmp_path / "A3d.mtx"))
    d2, d3 = ctx.vec(v2), ctx.vec(v3)
    cycle("v11", hierarchy(mg, A2), d2); cycle("v21", hierarchy(mg, A2, 2, 1), d2, False); cycle("v02", hierarchy(mg, A2, 0, 2), d2, False)
    cycle("v11_3d", hierarchy(mg, A3), d3)
    cycle("sigma", hierarchy(mg, A2).set_correction_scale(1.6), d2)
    cycle("additive", hierarchy(mg, A2).set_additive(True), d2)
    hierarchy(mg, A2)                                                            # use_preconditioner = false still builds it; solve(v) = v
    py.vec("identity", v2); py["identity.use"] = 0
    h = hierarchy(mg, A2).set_operand_precision(32)
    cycle("fp32", h, d2)
    cycle("fp64_again", h.set_operand_precision(64), d2)
    d10 = ctx.vec(v10k)
    A, P = Csr.from_mtx(ctx, str(tmp_path / "A10k.mtx")), Csr.from_mtx(ctx, str(tmp_path / "P10k.mtx"))
    cycle("with_P", hierarchy(mg, A, P=P), d10)
    Ad = Csr.from_mtx(ctx, str(tmp_path / "A10k.mtx"))
    cycle("with_P_device", hierarchy(mg, Ad, P=Csr.from_mtx(ctx, str(tmp_path / "P10k.mtx"))), d10)
    cycle("without_P", hierarchy(mg, Ad), d10)
    N = Csr.from_mtx(ctx, str(tmp_path / "N.mtx"))
    py["nullspace.before"] = int(N.nullspace() == "constant")
    N.set_nullspace("constant")
    py["nullspace.after"] = int(N.nullspace() == "constant")
    hN = hierarchy(mg, N)
    b = ctx.vec(bN)
    cycle("nullspace.cycle", hN, b)
    x = ctx.vec(576)
    py["nullspace.status"], py["nullspace.iterations"], py["nullspace.tol"] = mg.pcg(N, x, b, hN, 200, TOL)
    py.vec("nullspace.x", x)
    py["nullspace.withdrawn"] = int(N.set_nullspace(None).nullspace() == "constant")
    F.compare(cpp, py)
    print({k: cpp[k] for k in sorted(cpp) if k.endswith(".levels") or k.startswith("nullspace.") and not isinstance(cpp[k], np.ndarray)})
    assert cpp["v11.levels"] >= 3 and cpp["v11_3d.levels"] >= 3 and cpp["with_P.levels"] >= 3            # several device-built levels
    assert cpp["fp32.precision0"] == 32 and cpp["fp64_again.precision0"] == 64 and np.array_equal(cpp["fp64_again"], cpp["v11"])
    for other in ("v21", "v02", "sigma", "additive", "fp32", "identity"):
        assert not np.array_equal(cpp[other], cpp["v11"]), other                                         # every option reached the cycle
    assert np.array_equal(cpp["identity"], v2) and not np.array_equal(cpp["with_P"], cpp["without_P"])
    assert cpp["nullspace.status"] == 0 and abs(cpp["nullspace.x"].mean()) < 1e-12 * max(1.0, np.abs(cpp["nullspace.x"]).max())


# ------------------------------------------------------------------------------------------------------ 5. solvers
def test_solvers_fast_paths_and_generic_templates(mg, ctx, orc, exes, tmp_path):
    rng = np.random.default_rng(53)
    poisson_files(mg, ctx, tmp_path)
    b2 = rng.standard_normal(1024)
    F.write_f64(tmp_path / "b2d.f64", b2)
    bK = saddle_files(mg, orc, tmp_path)
    cpp = go(exes, "solvers", tmp_path)

    py = F.Record()

    def solve(name, call, n):
        x = ctx.vec(n)
        py[name + ".status"], py[name + ".iterations"], py[name + ".tol"] = call(x)
        py.vec(name + ".x", x)
    A = mg.Csr.from_mtx(ctx, str(tmp_path / "A2d.mtx"))
    b = ctx.vec(b2)
    h = hierarchy(mg, A)
    solve("cg", lambda x: mg.pcg(A, x, b, h, 300, TOL), 1024)
    solve("cg_host_matrix", lambda x: mg.pcg(A, x, b, h, 300, TOL), 1024)
    solve("bicgstab", lambda x: mg.bicgstab(A, x, b, h, 300, TOL), 1024)
    h21 = hierarchy(mg, A, 2, 1)
    solve("cg_flexible", lambda x: mg.pcg(A, x, b, h21, 300, TOL, flexible=True), 1024)
    K = mg.Csr.from_mtx(ctx, str(tmp_path / "K.mtx"))
    bk = ctx.vec(bK)
    hK = saddle_hierarchy(mg, ctx, tmp_path)
    solve("minres", lambda x: mg.minres(K, x, bk, hK, 300, TOL), len(bK))
    solve("minres_host_matrix", lambda x: mg.minres(hK.A, x, bk, hK, 300, TOL), len(bK))
    generic = [k for k in cpp if k.startswith(("cg_generic.", "minres_generic."))]
    assert len(generic) == 8
    for k in generic:
        py[k] = cpp[k]                                          # held to their own bars below
    F.compare(cpp, py, skip=generic)
    assert cpp["cg.status"] == 0 and cpp["bicgstab.status"] == 0 and cpp["minres.status"] == 0 and cpp["cg_flexible.status"] == 0
    for name, fast, path, rhs in (("cg_generic", "cg", "A2d.mtx", b2), ("minres_generic", "minres", "K.mtx", bK)):
        it, it_fast = cpp[name + ".iterations"], cpp[fast + ".iterations"]
        M = orc.Csr.from_scipy(host_csr(mg, tmp_path / path))
        tr = np.linalg.norm(M.residual(cpp[name + ".x"], rhs)) / np.linalg.norm(rhs)
        tr_fast = np.linalg.norm(M.residual(cpp[fast + ".x"], rhs)) / np.linalg.norm(rhs)
        print(f"{name}: status {cpp[name + '.status']}, {it} iterations (fast path {it_fast}), reported {cpp[name + '.tol']:.4e}, oracle's true residual {tr:.4e} "
              f"(fast path {tr_fast:.4e})")
        assert cpp[name + ".status"] == 0
        assert tr <= 1.5 * TOL and tr_fast <= 1.5 * TOL
        assert it <= it_fast + max(4, it_fast // 4), (it, it_fast)


# ------------------------------------------------------------------------------------------------------ 6. plans and guesses
def test_plans_and_guesses(mg, ctx, orc, exes, tmp_path):
    rng = np.random.default_rng(61)
    rp, ci, v = poisson_files(mg, ctx, tmp_path)
    n = 1024
    d = np.sqrt(rng.uniform(0.5, 2.0, n)); rows_of = np.repeat(np.arange(n), np.diff(rp))
    mg.write_mtx(str(tmp_path / "A2d_new.mtx"), n, n, rp, ci, v * d[rows_of] * d[ci])
    rhs = [rng.standard_normal(n) for _ in range(3)]
    for k in range(3):
        F.write_f64(tmp_path / f"b{k}.f64", rhs[k])
    bK = saddle_files(mg, orc, tmp_path)
    cpp = go(exes, "plans", tmp_path)

    py = F.Record()

    def walk(name, plan, b, enqueued):
        m = len(b)
        for ahead in (0, 1):
            tag = f"{name}.solve{ahead}"
            x = ctx.vec(m)
            py[tag + ".status"], py[tag + ".iterations"], py[tag + ".tol"] = plan.solve(x, b, 300, TOL, ahead)
            py.vec(tag + ".x", x)
            for i, val in enumerate(plan.info()):
                py[f"{tag}.info{i}"] = val
        x = ctx.vec(m)
        plan.enqueue(x, b, enqueued, TOL)
        py[name + ".result.status"], py[name + ".result.iterations"], py[name + ".result.resid"] = plan.result()
        py.vec(name + ".result.x", x)
        for i, val in enumerate(plan.info()):
            py[f"{name}.result.info{i}"] = val
        x = ctx.vec(m)
        py[name + ".default.status"], py[name + ".default.iterations"], py[name + ".default.tol"] = plan.solve(x, b, 300, 1e-6)
        py[name + ".default.info3"] = plan.info()[3]
        py.vec(name + ".default.x", x)

    def recursive(name, plan, b, enqueued):
        plan.enqueue(ctx.vec(len(b)), b, enqueued, TOL)
        for key, val in zip(("status", "iterations", "resid", "recursive_resid"), plan.result(recursive=True)):
            py[f"{name}.recursive.{key}"] = val

    def on_poisson():
        A = mg.Csr.from_mtx(ctx, str(tmp_path / "A2d.mtx"))
        return A, hierarchy(mg, A)
    b0, b1, b2 = (ctx.vec(r) for r in rhs)
    walk("pcg", mg.PcgPlan(*on_poisson()), b0, 6)
    for name, plan, b, enqueued, again, more in (("bicgstab", mg.BicgstabPlan(*on_poisson()), b0, 4, b1, 5), ("fgcr", mg.FgcrPlan(*on_poisson(), restart=4), b0, 6, b1, 7),
                                                  ("minres", mg.MinresPlan(mg.Csr.from_mtx(ctx, str(tmp_path / "K.mtx")), saddle_hierarchy(mg, ctx, tmp_path)), ctx.vec(bK), 10, None, 12)):
        walk(name, plan, b, enqueued)
        recursive(name, plan, again if again is not None else b, more)
    g = mg.Guess(on_poisson()[0], "residual", 3)
    x = ctx.vec(n)
    py["lifetime.apply_empty"] = g.apply(b0, x, rel_resid=True)[1]
    py["lifetime.update"] = int(g.update(b1))
    py["lifetime.apply"] = g.apply(b0, x, rel_resid=True)[1]
    py.vec("lifetime.x0", x)
    py["lifetime.size"], py["lifetime.capacity"] = g.info()["size"], g.info()["capacity"]
    A, h = on_poisson()
    g = mg.Guess(A, "energy", 2)
    x = ctx.vec(n)
    for k, b in enumerate((b0, b1, b2)):
        tag = f"guess.step{k}"
        x.fill(0.0)
        py[tag + ".apply"] = g.apply(b, x, rel_resid=True)[1]
        py.vec(tag + ".x0", x)
        py[tag + ".status"], py[tag + ".iterations"], _ = mg.pcg(A, x, b, h, 300, TOL)
        py[tag + ".added"] = int(g.update(x))
        info = g.info()
        py[tag + ".size"], py[tag + ".restarts"], py[tag + ".refused"] = info["size"], info["restarts"], info["refused"]
    py["guess.refused_again"] = int(g.update(x)); py["guess.refused"] = g.info()["refused"]
    py.vec("guess.apply_async", g.apply(b0, ctx.vec(n)))
    A.update_values(mg.read_mtx(str(tmp_path / "A2d_new.mtx"))[4])
    h.refresh(); g.rebase()
    py["guess.rebased.apply"] = g.apply(b1, x, rel_resid=True)[1]
    py.vec("guess.rebased.x0", x)
    py["guess.rebased.size"], py["guess.capacity"] = g.info()["size"], g.info()["capacity"]
    g.reset()
    py["guess.reset.size"] = g.info()["size"]
    py["guess.reset.apply"] = g.apply(b1, x, rel_resid=True)[1]
    py.vec("guess.reset.x0", x)
    F.compare(cpp, py)
    print({k: cpp[k] for k in sorted(cpp) if not isinstance(cpp[k], np.ndarray) and ".info" not in k})
    for name in ("pcg", "bicgstab", "fgcr", "minres"):
        assert cpp[name + ".solve0.status"] == 0 and np.array_equal(cpp[name + ".solve0.x"], cpp[name + ".solve1.x"]), name      # look-ahead keeps the bits
        assert cpp[name + ".solve0.info3"] == 0, name                                                                          # ahead = 0 runs nothing frozen
    assert cpp["guess.capacity"] == 2 and cpp["lifetime.capacity"] == 3 and cpp["lifetime.size"] == 1 and cpp["lifetime.apply_empty"] == 1.0
    assert [cpp[f"guess.step{k}.added"] for k in range(3)] == [1, 1, 1] and cpp["guess.step2.restarts"] == 1 and cpp["guess.reset.size"] == 0
    assert cpp["guess.step1.apply"] < 1.0 and cpp["guess.reset.apply"] == 1.0 and not cpp["guess.reset.x0"].any()


# ------------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_context_usable(mg, ctx, orc, exes, tmp_path):
    rng = np.random.default_rng(71)
    n, k = 300, 170
    Rm = random_csr(rng, n, n, 0.03, empty=(0, 17))
    Bm = random_csr(rng, n, k, 0.04)
    # Rq: R with one entry of row 9 moved to a column where that row stores nothing and B's row is not empty — the same shape and entry count
    Rq = Rm.copy()
    lo, hi = Rq.indptr[9], Rq.indptr[10]
    assert hi > lo
    free = [j for j in range(n) if j not in set(Rq.indices[lo:hi]) and Bm.indptr[j + 1] > Bm.indptr[j]]
    Rq.indices[lo] = free[-1]
    Rq.sort_indices()
    assert Rq.nnz == Rm.nnz and not np.array_equal(Rq.indices, Rm.indices)
    for name, M in (("R", Rm), ("B", Bm), ("Rq", Rq)):
        write_csr(mg, tmp_path / (name + ".mtx"), M)
    xh = rng.standard_normal(n)
    gbad = np.r_[rng.integers(0, n, 50), [n, -1, 2 ** 31 - 1], rng.integers(0, n, 11)]
    F.write_f64(tmp_path / "x.f64", xh); F.write_i32(tmp_path / "gbad.i32", gbad)
    saddle_files(mg, orc, tmp_path)
    cpp = go(exes, "refusals", tmp_path)

    Csr = mg.Csr
    py = F.Record()

    def code_of(call):
        with pytest.raises(mg.MgsError) as e:
            call()
        return e.value
    R, B, Rqd = (Csr.from_mtx(ctx, str(tmp_path / (name + ".mtx"))) for name in ("R", "B", "Rq"))
    x = ctx.vec(xh)
    K = Csr.bmat(ctx, [[R, B]])
    with pytest.raises(ValueError):
        K.bmat_update([[R, B], [None, R]])
    py["bmat_update_other_grid.code"] = py["bmat_update_other_grid_1x1.code"] = INVALID            # the header's own refusal
    py.csr("after_bmat_update", K.bmat_update([[R, B]]))
    C = R.matmul(B)
    e = code_of(lambda: C.matmul_update(Rqd, B, check=True))
    py["multiply_update_other_pattern.code"], py["multiply_update_other_pattern.misses"] = e.code, e.misses
    py.csr("after_multiply_update", C.matmul_update(R, B, check=True)); py["after_multiply_update.misses"] = 0
    y = ctx.vec(len(gbad))
    e = code_of(lambda: x.gather(dev(gbad, np.int32), out=y, check=True))
    py["gather_out_of_range.code"], py["gather_out_of_range.bad"] = e.code, e.bad
    py.vec("gather_out_of_range.y", y)
    py.vec("after_gather", R.spmv(x))
    py["update_values_other_pattern.code"] = py["update_values_other_shape.code"] = INVALID        # the header's own refusal
    py.csr("after_update_values", R)
    Kd = Csr.from_mtx(ctx, str(tmp_path / "K.mtx"))
    h21 = saddle_hierarchy(mg, ctx, tmp_path, nu1=2)
    py["minres_plan_v21.code"] = code_of(lambda: mg.MinresPlan(Kd, h21)).code
    rows = Kd.shape[0]
    bs = ctx.vec(np.ones(rows))
    py["minres_v21.code"] = code_of(lambda: mg.minres(Kd, ctx.vec(rows), bs, h21, 10, TOL)).code
    py.vec("after_minres", h21.vcycle(bs))
    F.compare(cpp, py)
    print({k: cpp[k] for k in sorted(cpp) if not isinstance(cpp[k], np.ndarray)})
    assert cpp["multiply_update_other_pattern.code"] == STATE and cpp["multiply_update_other_pattern.misses"] > 0
    assert cpp["gather_out_of_range.code"] == INVALID and cpp["gather_out_of_range.bad"] == 3
    assert cpp["minres_plan_v21.code"] == INVALID and cpp["minres_v21.code"] == INVALID
    assert np.array_equal(cpp["after_update_values.val"], host_csr(mg, tmp_path / "R.mtx").data)
