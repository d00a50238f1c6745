"""CPU-only checks that the sums and scalings of device matrices are offered on every face of the library — the C header, the built
libmgs.so, the ctypes prototypes, the Python classes, the C++ header — that the header states the contract, and that the refusals need
no device."""
import ctypes as C
import os
import re

from conftest import REPO

D, P, PP, I64P = C.c_double, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)
SYMBOLS = {
    "mgs_csr_add": ("double alpha, const mgs_csr *A, double beta, const mgs_csr *B, mgs_csr **C", [D, P, D, P, PP]),
    "mgs_csr_add_numeric": ("double alpha, const mgs_csr *A, double beta, const mgs_csr *B, mgs_csr *C, int64_t *misses", [D, P, D, P, P, I64P]),
    "mgs_csr_add_info": ("const mgs_csr *C, int64_t out[4]", [P, I64P]),
    "mgs_csr_scale": ("mgs_csr *A, const mgs_vec *dl, const mgs_vec *dr", [P, P, P]),
    "mgs_csr_diag": ("const mgs_csr *A, mgs_vec *d", [P, P]),
    "mgs_csr_from_diag": ("mgs_ctx *ctx, const mgs_vec *d, mgs_csr **out", [P, P, PP]),
}
MGS_ERR_INVALID = -1


def header():
    return open(os.path.join(REPO, "include", "mgs.h")).read()


def test_names_declared_exported_prototyped():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    import multigridsolver_amd as mg
    from multigridsolver_amd import _lib
    L = C.CDLL(mg.SO_PATH)
    for name, (params, argtypes) in SYMBOLS.items():
        m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"include/mgs.h does not declare {name}"
        assert " ".join(m.group(1).split()) == params, (name, m.group(1))
        assert hasattr(L, name), f"libmgs.so does not export {name}"
        res, got = _lib.PROTOTYPES[name]
        assert res is C.c_int and list(got) == argtypes, (name, got)
    for method in ("add", "__add__", "__sub__", "add_update", "add_info", "scale", "diagonal", "from_diag"):
        assert callable(getattr(mg.Csr, method)), method
    hpp = open(os.path.join(REPO, "multigridsolver_amd", "cpp", "mgs_host.hpp")).read()
    for form in ("DeviceMatrix add(const DeviceMatrix &B, double alpha = 1.0, double beta = 1.0) const", "void addUpdate(", "void scale(",
                 "Vector diagonal() const", "static DeviceMatrix fromDiagonal("):
        assert form in hpp, form
    assert "csr_algebra.hip" in open(os.path.join(REPO, "multigridsolver_amd", "csrc", "Makefile")).read()


def test_header_states_the_contract():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mgs_csr_add\(", header(), flags=re.S)
    assert m, "the sum's entry points have no header comment"
    text = " ".join(m.group(1).split())
    for word in ("Nearest reference line", "union", "ascending", "fl(fl(α·a) + fl(β·b))", "fl(α·a)", "fl(β·b)", "-0.0", "No atomics", "row shard", "2^31 - 1",
                 "MGS_ERR_INVALID", "MGS_ERR_STATE", "misses == NULL", "mgs_hier_refresh", "valcode", "fl(fl(dl_i·a_ij)·dr_j)", "min(rows, cols)",
                 "mgs_vec_size(d)", "the same handle", "gives both"):
        assert word in text, word


def test_refusals_need_no_device():
    import multigridsolver_amd as mg
    L = mg.lib()
    out = C.c_void_p(0x1234)
    assert L.mgs_csr_add(1.0, None, 1.0, None, C.byref(out)) == MGS_ERR_INVALID
    assert b"mgs_csr_add: NULL" in L.mgs_last_error(None) and out.value == 0x1234
    misses = C.c_int64(-7)
    assert L.mgs_csr_add_numeric(1.0, None, 1.0, None, None, C.byref(misses)) == MGS_ERR_INVALID
    assert b"mgs_csr_add_numeric: NULL" in L.mgs_last_error(None) and misses.value == -7
    assert L.mgs_csr_add_numeric(1.0, None, 1.0, None, None, None) == MGS_ERR_INVALID
    info = (C.c_int64 * 4)(9, 9, 9, 9)
    assert L.mgs_csr_add_info(None, info) == MGS_ERR_INVALID
    assert b"mgs_csr_add_info: NULL" in L.mgs_last_error(None) and list(info) == [9, 9, 9, 9]
    assert L.mgs_csr_scale(None, None, None) == MGS_ERR_INVALID
    assert b"mgs_csr_scale: NULL" in L.mgs_last_error(None)
    assert L.mgs_csr_diag(None, None) == MGS_ERR_INVALID
    assert b"mgs_csr_diag: NULL" in L.mgs_last_error(None)
    assert L.mgs_csr_from_diag(None, None, C.byref(out)) == MGS_ERR_INVALID
    assert b"mgs_csr_from_diag: NULL" in L.mgs_last_error(None) and out.value == 0x1234


TU = r"""
#include "mgs_host.hpp"
using namespace mgs;
int main(int argc, char **argv) {
  if (argc != 3) { std::cout << "usage: A.mtx B.mtx" << std::endl; return 1; }
  SMatrix A = readMatrix(argv[1]), B = readMatrix(argv[2]);
  DeviceMatrix Ad(A), Bd(B);
  DeviceMatrix Cd = Ad.add(Bd, 0.5, 2.0);
  Cd.addUpdate(Ad, Bd, 0.25, 2.0);             // enqueued only
  int64_t misses = 0;
  Cd.addUpdate(Ad, Bd, 0.25, 2.0, &misses);    // synchronises, throws Error(MGS_ERR_STATE) when misses != 0
  Vector d = Cd.diagonal();
  DeviceMatrix Dd = DeviceMatrix::fromDiagonal(d);
  Cd.scale(&d, nullptr); Cd.scale(nullptr, &d); Cd.scale(&d, &d);
  DeviceMatrix Sd = Cd.add(Dd);
  return misses == 0 && Sd.rows() == Ad.rows() && Sd.cols() == Ad.cols() && Dd.rows() == (int)d.size() ? 0 : 2;
}
"""


def test_cpp_forms_compile_and_link(tmp_path):
    import subprocess
    src = tmp_path / "algebra_tu.cpp"
    src.write_text(TU)
    exe = tmp_path / "algebra_tu"
    libdir = os.path.join(REPO, "multigridsolver_amd")
    assert os.path.exists(os.path.join(libdir, "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O0", "-Wall", "-I", os.path.join(libdir, "cpp"), "-o", str(exe), str(src),
                        "-L" + libdir, "-lmgs", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)      # usage path only: no device is touched
    assert r.returncode == 1 and "usage" in r.stdout
