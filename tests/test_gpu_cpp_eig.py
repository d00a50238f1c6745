"""The C++ face of the block passes and the eigensolver (multigridsolver_amd/cpp/mgs_host.hpp: vecsGram, vecsCombine, LOBPCGiml) on the
device: tests/cpp_eig/eig.cpp, run once as a child process on files written here, against the Python face on the same files.  θ, resid, X,
the Gram matrices and the combine outputs are equal bit for bit.  The usage path prints `usage:` and exits 1 before it touches a device."""
import os
import subprocess

import numpy as np
import pytest

import cpp_face
from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpp_eig", "eig.cpp")
LIBDIR = cpp_face.LIBDIR
TIME_LIMIT = 120


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    out = str(tmp_path_factory.mktemp("cpp_eig") / "eig")
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
    v = v.copy(); v[rp[:-1] + np.array([np.flatnonzero(ci[rp[i]:rp[i + 1]] == i)[0] for i in range(512)])] += np.random.default_rng(5).uniform(0, 1, 512)
    mg.write_mtx(str(ind / "A.mtx"), 512, 512, rp, ci, v)
    rng = np.random.default_rng(77)
    X0 = rng.standard_normal((512, 4)); Cm = rng.standard_normal((4, 3))
    for j in range(4):
        cpp_face.write_f64(ind / f"x{j}.f64", X0[:, j])
    cpp_face.write_f64(ind / "c.f64", Cm)

    r = subprocess.run(["timeout", "-k", "10", str(TIME_LIMIT), exe, str(ind), str(outd)], capture_output=True, text=True, timeout=TIME_LIMIT + 30)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    cpp = cpp_face.read_outputs(outd)

    ctx = mg.Context(0)
    try:
        A = mg.Csr.from_mtx(ctx, str(ind / "A.mtx"))
        py = cpp_face.Record()
        start = lambda: [ctx.vec(np.fromfile(str(ind / f"x{j}.f64"), dtype="<f8")) for j in range(4)]
        X = start()
        py["gram_same"] = mg.vecs_gram(X, X).ravel()
        py["gram_4x2"] = mg.vecs_gram(X, X[:2]).ravel()
        Y = [ctx.vec(512) for _ in range(3)]
        mg.vecs_combine(X, np.fromfile(str(ind / "c.f64"), dtype="<f8").reshape(4, 3), Y)
        for j in range(3):
            py.vec(f"combine{j}", Y[j])
        X = start()
        st, it, th, rs = mg.lobpcg(A, X, None, 200, 1e-6)
        py["none.status"], py["none.iterations"], py["none.tol"] = st, it, float(rs.max())
        py["none.theta"], py["none.resid"] = th, rs
        for j in range(4):
            py.vec(f"none.x{j}", X[j])
        h = mg.Hierarchy(A, 0.5, 1, 1).coarsen(10.0, 2, 8.0, coarse_rows=30).finalize()
        X = start()
        st, it, th, rs = mg.lobpcg(A, X, h, 200, 1e-6)
        py["amg.levels"] = h.nlev
        py["amg.status"], py["amg.iterations"], py["amg.tol"], py["amg.theta"] = st, it, float(rs.max()), th
        for j in range(4):
            py.vec(f"amg.x{j}", X[j])
        assert py["none.status"] == 0 and py["amg.status"] == 0 and py["amg.levels"] >= 2
        cpp_face.compare(cpp, py)
    finally:
        ctx.close()
