"""CPU-only checks that the block-vector passes and the eigensolver are offered on every face of the library: the C header with its two
constants, the built libmgs.so, the ctypes prototypes, the Python package, the solve CLI (--eigs) and the C++ header (LOBPCGiml and the two
block wrappers compile and link; the usage path touches no device)."""
import ctypes as C
import os
import re
import subprocess
import sys

from conftest import REPO

SYMBOLS = {"mgs_vecs_gram": 7, "mgs_vecs_combine": 7, "mgs_vecs_info": 2, "mgs_eig_lobpcg": 9, "mgs_eig_info": 2}


def test_declared_exported_prototyped():
    src = open(os.path.join(REPO, "include", "mgs.h")).read()
    assert re.search(r"#define\s+MGS_VECS_MAX\s+24\b", src) and re.search(r"#define\s+MGS_EIG_MAX_BLOCK\s+8\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    import multigridsolver_amd as mg
    from multigridsolver_amd import _lib, core
    L = C.CDLL(mg.SO_PATH)
    for name, nargs in SYMBOLS.items():
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"include/mgs.h does not declare {name}"
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(L, name), f"libmgs.so does not export {name}"
        res, argtypes = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(argtypes) == nargs, name
    assert _lib.MGS_VECS_MAX == 24 and _lib.MGS_EIG_MAX_BLOCK == 8
    assert _lib.PROTOTYPES["mgs_eig_lobpcg"][1][6:] == _lib.PROTOTYPES["mgs_pcg"][1][5:]      # max_iter, tol, status as in mgs_pcg
    for fn in ("lobpcg", "vecs_gram", "vecs_combine", "vecs_info", "eig_info"):
        assert callable(getattr(mg, fn)) and getattr(mg, fn) is getattr(core, fn), fn


def test_units_in_the_makefile_and_dense_header_is_plain_cxx():
    mk = open(os.path.join(REPO, "multigridsolver_amd", "csrc", "Makefile")).read()
    assert "blockvec.hip" in mk and "eig.hip" in mk and "eig_dense.hpp" in mk
    hdr = open(os.path.join(REPO, "multigridsolver_amd", "csrc", "eig_dense.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", hdr).lower()


def test_solve_cli_offers_eigs():
    r = subprocess.run([sys.executable, "-m", "multigridsolver_amd.solve", "--help"], capture_output=True, text=True, cwd=REPO, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--eigs" in r.stdout


TU = r"""
#include "mgs_host.hpp"
using namespace mgs;
int main(int argc, char **argv) {
  if (argc != 2) { std::cout << "usage: A.mtx" << std::endl; return 1; }
  SMatrix A = readMatrix(argv[1]);
  DeviceMatrix dA(A);
  std::vector<Vector> X;
  for (int j = 0; j < 2; ++j) { Vector v(A.rows()); v.setZero(); v[j] = 1.0; X.push_back(std::move(v)); }
  std::vector<double> theta, resid;
  int max_iter = 10; double tol = 1e-6;
  int st = LOBPCGiml(dA, X, theta, resid, nullptr, max_iter, tol);      // no preconditioner
  MultiGridPrecond precond(dA, nullptr);
  st += LOBPCGiml(dA, X, theta, precond, max_iter, tol);                // CGiml's calling shape
  std::vector<double> G = vecsGram(X, X);
  std::vector<double> Cm = {1.0, 0.0, 0.0, 1.0};
  vecsCombine(X, Cm, X);
  return st + (int)G.size();
}
"""


def test_cpp_face_compiles_and_links(tmp_path):
    hdr = open(os.path.join(REPO, "multigridsolver_amd", "cpp", "mgs_host.hpp")).read()
    assert "mgs_eig_lobpcg(" in hdr and "mgs_vecs_gram(" in hdr and "mgs_vecs_combine(" in hdr
    src = tmp_path / "eig_tu.cpp"
    src.write_text(TU)
    exe = tmp_path / "eig_tu"
    libdir = os.path.join(REPO, "multigridsolver_amd")
    assert os.path.exists(os.path.join(libdir, "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O0", "-Wall", "-I", os.path.join(libdir, "cpp"), "-o", str(exe), str(src),
                        "-L" + libdir, "-lmgs", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in r.stderr, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)      # usage path only: no device is touched
    assert r.returncode == 1 and "usage" in r.stdout
