"""CPU-only checks that the null-space declaration is offered on every face of the library: the C header, the built libmgs.so, the
ctypes prototypes, the Python package, the solve CLI, the C++ header — and that what can be decided without a device is."""
import ctypes as C
import os
import re
import subprocess
import sys

from conftest import REPO

INVALID = -1
NEW = {"mgs_csr_set_nullspace": 2, "mgs_csr_nullspace": 2, "mgs_csr_nullspace_defect": 2, "mgs_vec_project_const": 3}


def test_symbols_declared_exported_prototyped():
    src = open(os.path.join(REPO, "include", "mgs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"#define\s+MGS_NULLSPACE_NONE\s+0\b", code) and re.search(r"#define\s+MGS_NULLSPACE_CONSTANT\s+1\b", code)
    import multigridsolver_amd as mg
    from multigridsolver_amd._lib import PROTOTYPES
    L = C.CDLL(mg.SO_PATH)
    for name, nargs in NEW.items():
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"include/mgs.h does not declare {name}"
        assert len(m.group(1).split(",")) == nargs
        assert hasattr(L, name), f"libmgs.so does not export {name}"
        res, argtypes = PROTOTYPES[name]
        assert res is C.c_int and len(argtypes) == nargs
    for meth in ("set_nullspace", "nullspace", "nullspace_defect"):
        assert callable(getattr(mg.Csr, meth))
    assert callable(mg.Vec.project_const)
    from multigridsolver_amd.synthetic import neumann3d
    assert callable(neumann3d)


def test_null_arguments_are_refused_without_a_device():
    import multigridsolver_amd as mg
    L = mg.lib()
    k = C.c_int(7); out = (C.c_double * 2)(5.0, 5.0)
    for kind in (0, 1, 2, -1):
        assert L.mgs_csr_set_nullspace(None, kind) == INVALID
    assert b"NULL" in L.mgs_last_error(None)
    assert L.mgs_csr_nullspace(None, C.byref(k)) == INVALID and k.value == 7
    assert L.mgs_csr_nullspace_defect(None, out) == INVALID and list(out) == [5.0, 5.0]
    assert L.mgs_vec_project_const(None, None, None) == INVALID
    assert b"mgs_vec_project_const" in L.mgs_last_error(None)


def test_python_face_refuses_an_unknown_kind_before_the_library_is_asked():
    import multigridsolver_amd as mg
    import pytest
    A = mg.Csr(None, None, owned=False)
    for bad in ("Constant", "rigid", 1, 0):
        with pytest.raises(ValueError):
            A.set_nullspace(bad)


def test_solve_cli_lists_nullspace():
    r = subprocess.run([sys.executable, "-m", "multigridsolver_amd.solve", "--help"], capture_output=True, text=True, cwd=REPO, timeout=120)
    assert r.returncode == 0, r.stderr
    assert re.search(r"--nullspace \{none,constant\}", r.stdout), r.stdout


TU = r"""
#include "mgs_host.hpp"
using namespace mgs;
int main(int argc, char **argv) {
  if (argc != 2) { std::cout << "usage: A.mtx" << std::endl; return 1; }
  DeviceMatrix A(readMatrix(argv[1]));
  A.setNullspaceConstant(true);
  MultiGridPrecond precond(A, nullptr);
  VectorXd x(A.rows()), b(A.rows());
  x.setZero(); b.setZero();
  int max_iter = 10; double tol = 1e-6;
  int s = CGiml(precond.matrix(), x, b, precond, max_iter, tol);
  A.setNullspaceConstant(false);
  return s + (A.nullspaceConstant() ? 1 : 0);
}
"""


def test_cpp_face_compiles_and_links(tmp_path):
    src = tmp_path / "ns_tu.cpp"
    src.write_text(TU)
    exe = tmp_path / "ns_tu"
    libdir = os.path.join(REPO, "multigridsolver_amd")
    assert os.path.exists(os.path.join(libdir, "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O0", "-Wall", "-I", os.path.join(libdir, "cpp"), "-o", str(exe), str(src),
                        "-L" + libdir, "-lmgs", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)      # usage path only: no device is touched
    assert r.returncode == 1 and "usage" in r.stdout
