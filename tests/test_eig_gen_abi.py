"""CPU-only checks that the generalised eigensolver and its residual pass are offered on every face of the library: the C header with the
contract's statements, the built libmgs.so, the ctypes prototypes, the Python package, the solve CLI (--mass) and the C++ header (the
LOBPCGiml overload with a DeviceMatrix B and eigResidual compile and link; the usage path touches no device)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

from conftest import REPO

SYMBOLS = {"mgs_eig_lobpcg_gen": 10, "mgs_eig_residual": 7}


def test_declared_exported_prototyped():
    src = open(os.path.join(REPO, "include", "mgs.h")).read()
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
    gen, std = _lib.PROTOTYPES["mgs_eig_lobpcg_gen"][1], _lib.PROTOTYPES["mgs_eig_lobpcg"][1]
    assert gen[:1] == std[:1] and gen[1] is C.c_void_p and gen[2:] == std[1:]      # mgs_eig_lobpcg's arguments with B behind A
    assert _lib.PROTOTYPES["mgs_eig_residual"][1][1] is C.c_int64 and _lib.PROTOTYPES["mgs_eig_residual"][1][4] is C.c_double
    assert callable(mg.eig_residual) and mg.eig_residual is core.eig_residual
    sig = inspect.signature(mg.lobpcg)
    assert list(sig.parameters) == ["A", "X", "hier", "max_iter", "tol", "B"] and sig.parameters["B"].default is None
    assert sig.parameters["max_iter"].default == 200 and sig.parameters["tol"].default == 1e-6


def test_header_states_the_contract():
    src = open(os.path.join(REPO, "include", "mgs.h")).read()
    block = src[src.index("mgs_eig_lobpcg_gen: the m smallest"):src.index("#define MGS_EIG_MAX_BLOCK")]
    flat = " ".join(block.replace(" * ", " ").split())
    for words in ("B-orthonormal", "‖A‖∞ + |θ_j|·‖B‖∞", "fresh A·X and B·X", "W ← W − X·((BX)ᵀW)", "GB = ½(Sᵀ(BS) + (Sᵀ(BS))ᵀ)", "three mgs_vecs_combine calls",
                  "8m + 2", "out[7] those of B alone", "B == NULL: the call is mgs_eig_lobpcg", "B a row shard", "B-orthogonal", "status 2 also covers",
                  "fl(ax_i − fl(θ·bx_i))", "mgs_dot(r, r)", "r may be ax or bx", "nrm2 == NULL"):
        assert words in flat, words
    i = src.index("Not served:", src.index("the m smallest eigenpairs of a symmetric operator"))
    assert "B·x" not in src[i:src.index(".", i)]      # moved out of the eigensolver's "Not served" sentence


def test_kernel_lives_beside_the_folds_it_uses():
    """one fold: the pass is built from blas1.hpp's macros and k_dot's last stages inside blas1.hip; the solver's file has no kernel of its own for it"""
    b = open(os.path.join(REPO, "multigridsolver_amd", "csrc", "blas1.hip")).read()
    assert "eig_residual_kernel" in b and "eig_residual_vec_kernel" in b and "int k_eig_residual(" in b
    body = b[b.index("void eig_residual_kernel"):b.index("// ------------------------------------------------------------------ constant null space")]
    assert "BLAS1_FOLD1(" in body and "BLAS1_FOLD2(" in body and "__shfl_down" not in body
    e = open(os.path.join(REPO, "multigridsolver_amd", "csrc", "eig.hip")).read()
    gen = e[e.index("int mgs_eig_lobpcg_gen("):e.index("int mgs_eig_info(")]
    assert "k_eig_residual(" in gen and "k_dot(" not in gen
    mk = open(os.path.join(REPO, "multigridsolver_amd", "csrc", "Makefile")).read()
    assert "-ffp-contract=off" in mk and "blas1.hip" in mk and "eig.hip" in mk


def test_solve_cli_offers_mass_and_refuses_it_without_eigs(tmp_path):
    run = lambda *a: subprocess.run([sys.executable, "-m", "multigridsolver_amd.solve", *a], capture_output=True, text=True, cwd=REPO, timeout=120)
    r = run("--help")
    assert r.returncode == 0 and "--mass" in r.stdout, r.stderr
    r = run(str(tmp_path / "absent.mtx"), "--mass", str(tmp_path / "absent_b.mtx"))      # refused before any file is read
    assert r.returncode != 0 and "--mass" in r.stderr and "--eigs" in r.stderr


TU = r"""
#include "mgs_host.hpp"
using namespace mgs;
int main(int argc, char **argv) {
  if (argc != 3) { std::cout << "usage: A.mtx B.mtx" << std::endl; return 1; }
  DeviceMatrix dA(readMatrix(argv[1])), dB(readMatrix(argv[2]));
  std::vector<Vector> X;
  for (int j = 0; j < 2; ++j) { Vector v(dA.rows()); v.setZero(); v[j] = 1.0; X.push_back(std::move(v)); }
  std::vector<double> theta, resid;
  int max_iter = 10; double tol = 1e-6;
  int st = LOBPCGiml(dA, dB, X, theta, resid, nullptr, max_iter, tol);
  MultiGridPrecond precond(dA, nullptr);
  st += LOBPCGiml(dA, dB, X, theta, resid, &precond, max_iter, tol);
  Vector r(dA.rows());
  const double s = eigResidual(X[0], X[1], theta[0], r);
  return st + (s > 0.0);
}
"""


def test_cpp_face_compiles_and_links(tmp_path):
    hdr = open(os.path.join(REPO, "multigridsolver_amd", "cpp", "mgs_host.hpp")).read()
    assert "mgs_eig_lobpcg_gen(" in hdr and "mgs_eig_residual(" in hdr
    src = tmp_path / "eig_gen_tu.cpp"
    src.write_text(TU)
    exe = tmp_path / "eig_gen_tu"
    libdir = os.path.join(REPO, "multigridsolver_amd")
    assert os.path.exists(os.path.join(libdir, "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O0", "-Wall", "-I", os.path.join(libdir, "cpp"), "-o", str(exe), str(src),
                        "-L" + libdir, "-lmgs", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in r.stderr, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)      # usage path only: no device is touched
    assert r.returncode == 1 and "usage" in r.stdout
