"""The C++ face of the generalised eigensolver (multigridsolver_amd/cpp/mgs_host.hpp: LOBPCGiml with a DeviceMatrix B, eigResidual) on the
device: tests/cpp_eig/eig_gen.cpp, run once as a child process on files written here, against the Python face on the same files.  θ, resid, X
and the residual pass's outputs are equal bit for bit.  The usage path prints `usage:` and exits 1 before it touches a device."""
import os
import subprocess

import numpy as np
import pytest

import cpp_face
import eig_gen_ref as G
from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpp_eig", "eig_gen.cpp")
LIBDIR = cpp_face.LIBDIR
TIME_LIMIT = 120


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    out = str(tmp_path_factory.mktemp("cpp_eig_gen") / "eig_gen")
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O1", "-Wall", "-I", os.path.join(LIBDIR, "cpp"), "-I", cpp_face.SRC, "-o", out, SRC,
                        "-L" + LIBDIR, "-lmgs", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in r.stderr, r.stderr[-4000:]
    return out


def test_usage_path_touches_no_device(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "usage:" in r.stdout


@pytest.mark.gpu
def test_cpp_face_equals_python_face(exe, tmp_path):
    import multigridsolver_amd as mg
    from multigridsolver_amd import synthetic
    cpp_face.fail_if_a_child_died()
    ind, outd = tmp_path / "in", tmp_path / "out"
    os.makedirs(str(ind)); os.makedirs(str(outd))
    rp, ci, v = synthetic._poisson3d_dirichlet(8)
    diag = ci == np.repeat(np.arange(512), np.diff(rp))
    va = v.copy(); va[diag] += np.random.default_rng(5).uniform(0, 1, 512)
    vb = v / 24.0; vb[diag] += G.mass_parts("poisson8d")[0]
    mg.write_mtx(str(ind / "A.mtx"), 512, 512, rp, ci, va)
    mg.write_mtx(str(ind / "B.mtx"), 512, 512, rp, ci, vb)
    X0 = np.random.default_rng(77).standard_normal((512, 4))
    for j in range(4):
        cpp_face.write_f64(ind / f"x{j}.f64", X0[:, j])

    r = subprocess.run(["timeout", "-k", "10", str(TIME_LIMIT), exe, str(ind), str(outd)], capture_output=True, text=True, timeout=TIME_LIMIT + 30)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    cpp = cpp_face.read_outputs(outd)

    ctx = mg.Context(0)
    try:
        A, B = mg.Csr.from_mtx(ctx, str(ind / "A.mtx")), mg.Csr.from_mtx(ctx, str(ind / "B.mtx"))
        py = cpp_face.Record()
        start = lambda: [ctx.vec(np.fromfile(str(ind / f"x{j}.f64"), dtype="<f8")) for j in range(4)]
        X = start()
        rv = ctx.vec(512)
        py["res.nrm2"] = mg.eig_residual(X[0], X[1], 0.625, rv)
        py.vec("res.r", rv)
        py["res.inplace.nrm2"] = mg.eig_residual(X[2], X[3], -1.75, X[2])
        py.vec("res.inplace.r", X[2])
        X = start()
        st, it, th, rs = mg.lobpcg(A, X, None, 200, 1e-6, B=B)
        py["none.status"], py["none.iterations"], py["none.tol"] = st, it, float(rs.max())
        py["none.theta"], py["none.resid"] = th, rs
        for j in range(4):
            py.vec(f"none.x{j}", X[j])
        h = mg.Hierarchy(A, 0.5, 1, 1).coarsen(10.0, 2, 8.0, coarse_rows=30).finalize()
        X = start()
        st, it, th, rs = mg.lobpcg(A, X, h, 200, 1e-6, B=B)
        py["amg.levels"] = h.nlev
        py["amg.status"], py["amg.iterations"], py["amg.tol"], py["amg.theta"], py["amg.resid"] = st, it, float(rs.max()), th, rs
        for j in range(4):
            py.vec(f"amg.x{j}", X[j])
        assert py["none.status"] == 0 and py["amg.status"] == 0 and py["amg.levels"] >= 2
        _, _, brp, bci, bv = mg.read_mtx(str(ind / "B.mtx"))      # B as the file holds it (the writer keeps fewer digits than a double)
        Bh = np.zeros((512, 512)); np.add.at(Bh, (np.repeat(np.arange(512), np.diff(brp)), bci), bv)
        Xh = np.stack([x.numpy() for x in X], axis=1)
        assert np.abs(Xh.T @ Bh @ Xh - np.eye(4)).max() <= 1e-12
        cpp_face.compare(cpp, py)
    finally:
        ctx.close()
