"""CPU-only checks that blocks of device matrices and the vector gather / scatter are offered on every face of the library — the C header,
the built libmgs.so, the ctypes prototypes, the Python classes, the C++ header — that the header states the contract, and that the
refusals need no device."""
import ctypes as C
import os
import re

from conftest import REPO

P, PP, I, I64, I64P = C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int64, C.POINTER(C.c_int64)
SYMBOLS = {
    "mgs_csr_extract": ("const mgs_csr *A, const void *rows_dev, int64_t nr, const void *cols_dev, int64_t nc, int index_bits, int keep_map, mgs_csr **S",
                        [P, P, I64, P, I64, I, I, PP]),
    "mgs_csr_extract_numeric": ("const mgs_csr *A, mgs_csr *S", [P, P]),
    "mgs_csr_extract_info": ("const mgs_csr *S, int64_t out[4]", [P, I64P]),
    "mgs_vec_gather": ("const mgs_vec *x, const void *idx_dev, int64_t n, int index_bits, mgs_vec *y, int64_t *bad", [P, P, I64, I, P, I64P]),
    "mgs_vec_scatter": ("const mgs_vec *y, const void *idx_dev, int64_t n, int index_bits, mgs_vec *x, int64_t *bad", [P, P, I64, I, P, I64P]),
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
    for method in ("extract", "extract_update", "extract_info"):
        assert callable(getattr(mg.Csr, method)), method
    for method in ("gather", "scatter"):
        assert callable(getattr(mg.Vec, method)), method
    hpp = open(os.path.join(REPO, "multigridsolver_amd", "cpp", "mgs_host.hpp")).read()
    for form in ("DeviceMatrix extract(const void *rows_dev, int64_t nr, const void *cols_dev, int64_t nc, int index_bits = 32, bool keepMap = false) const",
                 "void extractUpdate(const DeviceMatrix &A)", "void gather(const void *idx_dev, int64_t n, int index_bits, Vector &y, int64_t *bad = nullptr) const",
                 "void scatter(const void *idx_dev, int64_t n, int index_bits, Vector &x, int64_t *bad = nullptr) const"):
        assert form in hpp, form
    assert "extract.hip" in open(os.path.join(REPO, "multigridsolver_amd", "csrc", "Makefile")).read()


def test_header_states_the_contract():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mgs_csr_extract\(", header(), flags=re.S)
    assert m, "the block's entry points have no header comment"
    text = " ".join(m.group(1).split())
    assert "Nearest reference line: none" in text
    for word in ("strictly ascending", "lowest", "row shard", "2^31 - 1", "keep_map", "mgs_hier_refresh", "valcode", "-0.0", "MGS_ERR_STATE", "MGS_ERR_INVALID",
                 "bad == NULL", "distinct", "rows_dev == NULL", "cols_dev == NULL", "any order", "repeat", "permutation", "NaN", "structural", "+0.0",
                 "4 B per entry", "mgs_csr_destroy", "null-space", "origin", "identical"):
        assert word in text, word


def test_refusals_need_no_device():
    import multigridsolver_amd as mg
    L = mg.lib()
    out = C.c_void_p(0x1234)
    assert L.mgs_csr_extract(None, None, 0, None, 0, 32, 0, C.byref(out)) == MGS_ERR_INVALID
    assert b"mgs_csr_extract: NULL" in L.mgs_last_error(None) and out.value == 0x1234
    assert L.mgs_csr_extract_numeric(None, None) == MGS_ERR_INVALID
    assert b"mgs_csr_extract_numeric: NULL" in L.mgs_last_error(None)
    info = (C.c_int64 * 4)(9, 9, 9, 9)
    assert L.mgs_csr_extract_info(None, info) == MGS_ERR_INVALID
    assert b"mgs_csr_extract_info: NULL" in L.mgs_last_error(None) and list(info) == [9, 9, 9, 9]
    bad = C.c_int64(-7)
    assert L.mgs_vec_gather(None, None, 0, 32, None, C.byref(bad)) == MGS_ERR_INVALID
    assert b"mgs_vec_gather: NULL" in L.mgs_last_error(None) and bad.value == -7
    assert L.mgs_vec_scatter(None, None, 0, 32, None, C.byref(bad)) == MGS_ERR_INVALID
    assert b"mgs_vec_scatter: NULL" in L.mgs_last_error(None) and bad.value == -7
    assert L.mgs_vec_gather(None, None, 0, 32, None, None) == MGS_ERR_INVALID


TU = r"""
#include "mgs_host.hpp"
using namespace mgs;
int main(int argc, char **argv) {
  if (argc != 2) { std::cout << "usage: A.mtx" << std::endl; return 1; }
  SMatrix A = readMatrix(argv[1]);
  DeviceMatrix Ad(A);
  const void *free_dev = nullptr, *fixed_dev = nullptr;      // index lists in device memory (here: none, every row and every column)
  DeviceMatrix Aff = Ad.extract(free_dev, 0, free_dev, 0, 32, true);
  DeviceMatrix Afc = Ad.extract(free_dev, 0, fixed_dev, 0);
  Aff.extractUpdate(Ad);                                      // enqueued only
  Vector b(Ad.rows()), bf(Aff.rows()), x(Ad.rows());
  int64_t bad = 0;
  b.gather(free_dev, 0, 32, bf);                              // enqueued only
  b.gather(free_dev, 0, 64, bf, &bad);                        // synchronises, throws Error(MGS_ERR_INVALID) when bad != 0
  bf.scatter(free_dev, 0, 32, x);
  bf.scatter(free_dev, 0, 64, x, &bad);
  return bad == 0 && Aff.rows() == Ad.rows() && Afc.cols() == Ad.cols() ? 0 : 2;
}
"""


def test_cpp_forms_compile_and_link(tmp_path):
    import subprocess
    src = tmp_path / "extract_tu.cpp"
    src.write_text(TU)
    exe = tmp_path / "extract_tu"
    libdir = os.path.join(REPO, "multigridsolver_amd")
    assert os.path.exists(os.path.join(libdir, "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O0", "-Wall", "-I", os.path.join(libdir, "cpp"), "-o", str(exe), str(src),
                        "-L" + libdir, "-lmgs", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)      # usage path only: no device is touched
    assert r.returncode == 1 and "usage" in r.stdout
