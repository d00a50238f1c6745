"""CPU-only checks that the device sparse product is offered on every face of the library — the C header, the built libmgs.so, the
ctypes prototypes, the Python classes — that the header states the contract, and that the refusals need no device."""
import ctypes as C
import os
import re

from conftest import REPO

SYMBOLS = {"mgs_csr_spgemm": 3, "mgs_csr_spgemm_numeric": 4, "mgs_csr_spgemm_info": 2}
MGS_ERR_INVALID = -1


def header():
    return open(os.path.join(REPO, "include", "mgs.h")).read()


def test_names_declared_exported_prototyped():
    src = header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    import multigridsolver_amd as mg
    from multigridsolver_amd import _lib
    L = C.CDLL(mg.SO_PATH)
    for name, nargs in SYMBOLS.items():
        m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"include/mgs.h does not declare {name}"
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(L, name), f"libmgs.so does not export {name}"
        res, argtypes = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(argtypes) == nargs, (name, argtypes)
    # the fourth name is a constant: the header defines it, the loader mirrors it, the library's message quotes it (see below)
    m = re.search(r"#define\s+MGS_SPGEMM_MAX_ROW\s+(\d+)", code)
    assert m and int(m.group(1)) == 8192 == _lib.MGS_SPGEMM_MAX_ROW
    assert b"MGS_SPGEMM_MAX_ROW" in open(mg.SO_PATH, "rb").read()
    for method in ("matmul", "__matmul__", "matmul_update", "spgemm_info"):
        assert callable(getattr(mg.Csr, method)), method
    hpp = open(os.path.join(REPO, "multigridsolver_amd", "cpp", "mgs_host.hpp")).read()
    assert "DeviceMatrix multiply(const DeviceMatrix &B) const" in hpp and "void multiplyUpdate(" in hpp


def test_header_states_the_contract():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define MGS_SPGEMM_MAX_ROW", header(), flags=re.S)
    assert m, "the product's entry points have no header comment"
    text = " ".join(m.group(1).split())
    for word in ("bicg.cpp:32-33", "MGS_SPGEMM_MAX_ROW", "storage order", "MGS_ERR_STATE", "MGS_ERR_INVALID", "rounded once", "-0.0", "ascending",
                 "row shard", "mgs_hier_refresh", "misses == NULL", "2^31"):
        assert word in text, word


def test_refusals_need_no_device():
    import multigridsolver_amd as mg
    L = mg.lib()
    out = C.c_void_p(0x1234)
    fake = C.c_void_p(0)
    assert L.mgs_csr_spgemm(None, None, C.byref(out)) == MGS_ERR_INVALID
    assert b"NULL" in L.mgs_last_error(None) and out.value == 0x1234
    assert L.mgs_csr_spgemm(fake, fake, None) == MGS_ERR_INVALID
    misses = C.c_int64(-7)
    assert L.mgs_csr_spgemm_numeric(None, None, None, C.byref(misses)) == MGS_ERR_INVALID
    assert b"mgs_csr_spgemm_numeric" in L.mgs_last_error(None) and misses.value == -7
    assert L.mgs_csr_spgemm_numeric(None, None, None, None) == MGS_ERR_INVALID
    info = (C.c_int64 * 4)(9, 9, 9, 9)
    assert L.mgs_csr_spgemm_info(None, info) == MGS_ERR_INVALID
    assert list(info) == [9, 9, 9, 9]



TU = r"""
#include "mgs_host.hpp"
using namespace mgs;
int main(int argc, char **argv) {
  if (argc != 3) { std::cout << "usage: A.mtx B.mtx" << std::endl; return 1; }
  SMatrix A = readMatrix(argv[1]), B = readMatrix(argv[2]);
  DeviceMatrix Ad(A), Bd(B);
  DeviceMatrix Cd = Ad.multiply(Bd);
  Cd.multiplyUpdate(Ad, Bd);                   // enqueued only
  int64_t misses = 0;
  Cd.multiplyUpdate(Ad, Bd, &misses);          // synchronises, throws Error(MGS_ERR_STATE) when misses != 0
  return misses == 0 && Cd.rows() == Ad.rows() && Cd.cols() == Bd.cols() ? 0 : 2;
}
"""


def test_cpp_product_forms_compile_and_link(tmp_path):
    import subprocess
    src = tmp_path / "spgemm_tu.cpp"
    src.write_text(TU)
    exe = tmp_path / "spgemm_tu"
    libdir = os.path.join(REPO, "multigridsolver_amd")
    assert os.path.exists(os.path.join(libdir, "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O0", "-Wall", "-I", os.path.join(libdir, "cpp"), "-o", str(exe), str(src),
                        "-L" + libdir, "-lmgs", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)      # usage path only: no device is touched
    assert r.returncode == 1 and "usage" in r.stdout
