"""CPU-only checks that the value refresh (same pattern, new values) is offered on every face of the library: the C header, the built
libmgs.so, the ctypes prototypes, the Python classes and the C++ header; and that the NULL refusals need no device."""
import ctypes as C
import os
import re
import subprocess

from conftest import REPO

SYMBOLS = {"mgs_csr_update_values": 3, "mgs_csr_update_values_dev": 3, "mgs_hier_refresh": 1, "mgs_hier_refresh_info": 2}
MGS_ERR_INVALID = -1


def test_symbols_declared_exported_prototyped():
    src = open(os.path.join(REPO, "include", "mgs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    import multigridsolver_amd as mg
    from multigridsolver_amd._lib import PROTOTYPES
    L = C.CDLL(mg.SO_PATH)
    for name, nargs in SYMBOLS.items():
        m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"include/mgs.h does not declare {name}"
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(L, name), f"libmgs.so does not export {name}"
        res, argtypes = PROTOTYPES[name]
        assert res is C.c_int and len(argtypes) == nargs, (name, argtypes)
    assert callable(mg.Csr.update_values) and callable(mg.Hierarchy.refresh) and callable(mg.Hierarchy.refresh_info)


def test_header_says_what_is_refused_and_the_caveat():
    src = open(os.path.join(REPO, "include", "mgs.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mgs_hier_refresh\(", src, flags=re.S)
    assert m, "mgs_hier_refresh has no header comment"
    text = " ".join(m.group(1).split())
    for word in ("bicg.cpp:19-44", "no reference counterpart", "MGS_ERR_NUMERIC", "MGS_ERR_STATE", "MGS_ERR_INVALID", "row-sharded", "general P",
                 "valcode", "npass", "rounding"):
        assert word in text, word


def test_null_arguments_refused_without_a_device():
    import multigridsolver_amd as mg
    L = mg.lib()
    assert L.mgs_hier_refresh(None) == MGS_ERR_INVALID
    assert b"NULL" in L.mgs_last_error(None)
    v = (C.c_double * 4)()
    assert L.mgs_csr_update_values(None, v, 4) == MGS_ERR_INVALID
    assert L.mgs_csr_update_values_dev(None, None, 4) == MGS_ERR_INVALID
    out = (C.c_int64 * 4)()
    assert L.mgs_hier_refresh_info(None, out) == MGS_ERR_INVALID


TU = r"""
#include "mgs_host.hpp"
using namespace mgs;
int main(int argc, char **argv) {
  if (argc != 4) { std::cout << "usage: A.mtx P.mtx A_new.mtx" << std::endl; return 1; }
  SMatrix A = readMatrix(argv[1]), P = readMatrix(argv[2]), A_new = readMatrix(argv[3]);
  MultiGridPrecond precond(A, P);
  precond.refresh(A_new);                      // the preconditioner's own upload takes A_new's values
  DeviceMatrix Ad(A);
  MultiGridPrecond shared(Ad, &P);
  Ad.update_values(A_new);                     // the caller's matrix, shared with the preconditioner
  shared.refresh();
  return 0;
}
"""


def test_cpp_refresh_forms_compile_and_link(tmp_path):
    src = tmp_path / "refresh_tu.cpp"
    src.write_text(TU)
    exe = tmp_path / "refresh_tu"
    libdir = os.path.join(REPO, "multigridsolver_amd")
    assert os.path.exists(os.path.join(libdir, "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O0", "-Wall", "-I", os.path.join(libdir, "cpp"), "-o", str(exe), str(src),
                        "-L" + libdir, "-lmgs", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)      # usage path only: no device is touched
    assert r.returncode == 1 and "usage" in r.stdout
