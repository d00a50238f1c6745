"""The C++ face of the value refresh (mgs_host.hpp): MultiGridPrecond::refresh(A_new) followed by solve(v) gives the bits of the Python
path on the same inputs, and a matrix with another pattern is refused with an exception."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

TU = r"""
#include <fstream>
#include "mgs_host.hpp"
using namespace mgs;
int main(int argc, char **argv) {
  if (argc != 7) { std::cout << "usage: A.mtx P.mtx A_new.mtx A_other.mtx v.bin x.bin" << std::endl; return 1; }
  SMatrix A = readMatrix(argv[1]), P = readMatrix(argv[2]), A_new = readMatrix(argv[3]), A_other = readMatrix(argv[4]);
  std::vector<double> hv((size_t)A.rows());
  { std::ifstream f(argv[5], std::ios::binary); f.read((char *)hv.data(), (std::streamsize)(hv.size() * sizeof(double))); if (!f) return 2; }
  MultiGridPrecond::Options o; o.omega = 0.6; o.coarse_rows = 200;
  MultiGridPrecond precond(A, P, o);
  VectorXd v(A.rows());
  v.upload(hv);
  VectorXd x0 = precond.solve(v);              // operands and graphs exist before the refresh
  precond.refresh(A_new);
  VectorXd x = precond.solve(v);
  std::vector<double> hx = x.download();
  { std::ofstream f(argv[6], std::ios::binary); f.write((const char *)hx.data(), (std::streamsize)(hx.size() * sizeof(double))); }
  try { precond.refresh(A_other); }
  catch (const Error &e) { std::cout << "MISMATCH_THROWN " << e.code << std::endl; return 0; }
  std::cout << "MISMATCH_ACCEPTED" << std::endl;
  return 3;
}
"""


def test_cpp_refresh_matches_python_and_refuses_another_pattern(inputs, tmp_path):
    import multigridsolver_amd as mg
    libdir = os.path.join(REPO, "multigridsolver_amd")
    src = tmp_path / "refresh_gpu_tu.cpp"; src.write_text(TU)
    exe = tmp_path / "refresh_gpu_tu"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O1", "-Wall", "-I", os.path.join(libdir, "cpp"), "-o", str(exe), str(src),
                        "-L" + libdir, "-lmgs", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    # inputs: the 2-D Poisson operator with the reference's P; the same pattern with other values; the same operator less one entry
    n, m, rp, ci, v = mg.read_mtx(inputs["poisson10000"])
    rows = np.repeat(np.arange(n), np.diff(rp))
    d = np.sqrt(np.random.default_rng(3).uniform(0.5, 2.0, n))
    a_new, a_other = str(tmp_path / "A_new.mtx"), str(tmp_path / "A_other.mtx")
    mg.write_mtx(a_new, n, m, rp, ci, v * d[rows] * d[ci])
    drop = rp[7] if ci[rp[7]] != 7 else rp[7] + 1            # an off-diagonal entry of row 7
    keep = np.ones(len(ci), bool); keep[drop] = False
    rp_o = np.r_[0, np.cumsum(np.bincount(rows[keep], minlength=n))].astype(np.int32)
    mg.write_mtx(a_other, n, m, rp_o, ci[keep], v[keep])
    v_np = np.random.default_rng(5).standard_normal(n)
    v_bin, x_bin = str(tmp_path / "v.bin"), str(tmp_path / "x.bin")
    v_np.astype("<f8").tofile(v_bin)
    r = subprocess.run(["timeout", "-k", "10", "240", str(exe), inputs["poisson10000"], inputs["poisson10000promatrix"], a_new, a_other, v_bin, x_bin],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "MISMATCH_THROWN -1" in r.stdout, r.stdout
    x_cpp = np.fromfile(x_bin, dtype="<f8")
    # the Python path on the files the C++ program read
    ctx = mg.Context(0)
    try:
        A = mg.Csr.from_mtx(ctx, inputs["poisson10000"]); P = mg.Csr.from_mtx(ctx, inputs["poisson10000promatrix"])
        h = mg.Hierarchy(A, 0.6, 1, 1).push_P(P).coarsen(10.0, 2, 8.0, 200, 32).finalize()
        b = ctx.vec(v_np)
        h.vcycle(b)
        A.update_values(mg.read_mtx(a_new)[4])
        x_py = h.refresh().vcycle(b).numpy()
    finally:
        ctx.close()
    assert x_cpp.shape == x_py.shape and np.isfinite(x_py).all()
    assert np.array_equal(x_cpp, x_py), float(np.abs(x_cpp - x_py).max())
