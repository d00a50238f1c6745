"""CPU-only checks that preconditioned MINRES is offered on every face of the library: the C header, the built libmgs.so, the ctypes
prototypes, the Python package, the solve CLI (accepted; refused together with --ahead and under a multi-rank launch) and the C++ header
(all three MINRESiml forms compile and link)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from conftest import REPO


def test_mgs_minres_declared_exported_prototyped():
    src = open(os.path.join(REPO, "include", "mgs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+mgs_minres\s*\(([^)]*)\)\s*;", code)
    assert m, "include/mgs.h does not declare mgs_minres"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 7 and args[3] == "mgs_hier *h" and args[4] == "int *max_iter", args
    assert code.index("mgs_pcg(") < code.index("mgs_minres(") < code.index("mgs_pcg_plan_create(")      # beside mgs_pcg
    import multigridsolver_amd as mg
    L = C.CDLL(mg.SO_PATH)
    assert hasattr(L, "mgs_minres"), "libmgs.so does not export mgs_minres"
    from multigridsolver_amd._lib import PROTOTYPES
    res, argtypes = PROTOTYPES["mgs_minres"]
    assert res is C.c_int and len(argtypes) == 7 and argtypes[4:] == PROTOTYPES["mgs_bicgstab"][1][4:]
    assert callable(mg.minres)
    from multigridsolver_amd import core
    assert mg.minres is core.minres


def test_solve_cli_accepts_minres_and_refuses_ahead(monkeypatch):
    r = subprocess.run([sys.executable, "-m", "multigridsolver_amd.solve", "--help"], capture_output=True, text=True, cwd=REPO, timeout=120)
    assert r.returncode == 0, r.stderr
    assert re.search(r"--solver \{[^}]*\bminres\b[^}]*\}", r.stdout), r.stdout
    from multigridsolver_amd import solve
    # the refusals come before any file is read or any device is touched
    with pytest.raises(SystemExit) as e:
        solve.main(["no_such_file.mtx", "--solver", "minres", "--ahead", "1"])
    assert "--ahead" in str(e.value)
    monkeypatch.setenv("WORLD_SIZE", "2"); monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:
        solve.main(["no_such_file.mtx", "--solver", "minres"])
    assert "minres" in str(e.value) and "single GPU" in str(e.value)


TU = r"""
#include "mgs_host.hpp"
using namespace mgs;
// a host-side operator and preconditioner of the caller's own: the generic template must serve them
struct Flip { Vector operator*(const Vector &v) const { return -2.0 * v; } };
struct Half { Vector solve(const Vector &v) const { return 0.5 * v; } };
int main(int argc, char **argv) {
  if (argc != 3) { std::cout << "usage: A.mtx P.mtx" << std::endl; return 1; }
  SMatrix A = readMatrix(argv[1]), P = readMatrix(argv[2]);
  MultiGridPrecond precond(A, P);
  VectorXd x(A.rows()), b(A.rows());
  x.setZero(); b.setZero();
  int max_iter = 10; double tol = 1e-6;
  int s0 = MINRESiml(A, x, b, precond, max_iter, tol);                   // host SMatrix, as the reference's main() calls its solver
  int s1 = MINRESiml(precond.matrix(), x, b, precond, max_iter, tol);    // device fast path (mgs_minres)
  int s2 = MINRESiml(Flip(), x, b, Half(), max_iter, tol);               // generic template
  return s0 + s1 + s2;
}
"""


def test_minresiml_three_forms_compile_and_link(tmp_path):
    hdr = open(os.path.join(REPO, "multigridsolver_amd", "cpp", "mgs_host.hpp")).read()
    assert len(re.findall(r"\bint MINRESiml\(", hdr)) == 3 and "mgs_minres(" in hdr
    src = tmp_path / "minresiml_tu.cpp"
    src.write_text(TU)
    exe = tmp_path / "minresiml_tu"
    libdir = os.path.join(REPO, "multigridsolver_amd")
    assert os.path.exists(os.path.join(libdir, "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O0", "-Wall", "-I", os.path.join(libdir, "cpp"), "-o", str(exe), str(src),
                        "-L" + libdir, "-lmgs", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    # usage path only: no device is touched
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "usage" in r.stdout
