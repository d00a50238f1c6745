"""CPU-only checks that the reordering and the assembly of device matrices are offered on every face of the library — the C header, the
built libmgs.so, the ctypes prototypes, the Python classes, the C++ header — that the header states the contract, that the constants
agree, and that the refusals which need no device need none."""
import ctypes as C
import os
import re

from conftest import REPO

import reorder_ref as ref

P, PP, I, IP, I64P = C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)
SYMBOLS = {
    "mgs_csr_permute": ("const mgs_csr *A, const void *rperm_dev, const void *cperm_dev, int index_bits, int keep_map, mgs_csr **C", [P, P, P, I, I, PP]),
    "mgs_csr_permute_numeric": ("const mgs_csr *A, mgs_csr *C", [P, P]),
    "mgs_csr_permute_info": ("const mgs_csr *C, int64_t out[4]", [P, I64P]),
    "mgs_csr_bmat": ("mgs_ctx *ctx, int br, int bc, const mgs_csr *const *blocks, const int *row_sizes, const int *col_sizes, mgs_csr **C", [P, I, I, PP, IP, IP, PP]),
    "mgs_csr_bmat_numeric": ("mgs_csr *C, const mgs_csr *const *blocks", [P, PP]),
    "mgs_csr_bmat_info": ("const mgs_csr *C, int64_t out[4]", [P, I64P]),
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
    for method in ("permute", "permute_update", "permute_info", "bmat", "hstack", "vstack", "block_diag", "bmat_update", "bmat_info"):
        assert callable(getattr(mg.Csr, method)), method
    hpp = open(os.path.join(REPO, "multigridsolver_amd", "cpp", "mgs_host.hpp")).read()
    for form in ("DeviceMatrix permute(const void *rperm_dev, const void *cperm_dev, int index_bits = 32, bool keepMap = false) const",
                 "void permuteUpdate(const DeviceMatrix &A)",
                 "static DeviceMatrix bmat(int br, int bc, const DeviceMatrix *const *blocks, const int *row_sizes = nullptr, const int *col_sizes = nullptr)",
                 "void bmatUpdate(int br, int bc, const DeviceMatrix *const *blocks)"):
        assert form in hpp, form
    assert "reorder.hip" in open(os.path.join(REPO, "multigridsolver_amd", "csrc", "Makefile")).read()


def test_constants_agree():
    m = re.search(r"#define\s+MGS_BMAT_MAX_BLOCKS\s+(\d+)", header())
    assert m and int(m.group(1)) == ref.MAX_BLOCKS == 256
    src = open(os.path.join(REPO, "multigridsolver_amd", "csrc", "reorder.hip")).read()
    m = re.search(r"constexpr int PERM_LANE_LEN = (\d+);", src)
    assert m and int(m.group(1)) == ref.LANE_LEN == 64


def test_header_states_the_contract():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define MGS_BMAT_MAX_BLOCKS[^\n]*\n\s*int mgs_csr_permute\(", header(), flags=re.S)
    assert m, "the entry points have no header comment"
    text = " ".join(m.group(1).split())
    assert "Nearest reference line: none" in text
    for word in ("C[i, j] = A[rperm[i], cperm[j]]", "bijection", "lowest", "repeats", "64-bit values", "rperm_dev == NULL", "both NULL give a copy", "same list twice",
                 "mgs_vec_gather", "rank", "atomics", "identical", "64 entries", "chunk", "-0.0", "NaN", "structural", "row shard", "keep_map", "4 B per entry",
                 "mgs_csr_destroy", "mgs_hier_refresh", "valcode", "MGS_ERR_STATE", "MGS_ERR_INVALID", "null-space", "origin", "row-major", "zero block",
                 "several places", "hstack", "vstack", "block-diagonal", "row_sizes", "col_sizes", "bisection", "table in device memory", "64-bit total",
                 "MGS_BMAT_MAX_BLOCKS", "(I, J)", "2^31 - 1", "no map is kept", "cperm_dev == NULL"):
        assert word in text, word


def test_refusals_need_no_device():
    import multigridsolver_amd as mg
    L = mg.lib()
    out = C.c_void_p(0x1234)
    assert L.mgs_csr_permute(None, None, None, 32, 0, C.byref(out)) == MGS_ERR_INVALID
    assert b"mgs_csr_permute: NULL" in L.mgs_last_error(None) and out.value == 0x1234
    assert L.mgs_csr_permute_numeric(None, None) == MGS_ERR_INVALID
    assert b"mgs_csr_permute_numeric: NULL" in L.mgs_last_error(None)
    info = (C.c_int64 * 4)(9, 9, 9, 9)
    assert L.mgs_csr_permute_info(None, info) == MGS_ERR_INVALID
    assert b"mgs_csr_permute_info: NULL" in L.mgs_last_error(None) and list(info) == [9, 9, 9, 9]
    blocks = (C.c_void_p * 1)(None)
    assert L.mgs_csr_bmat(None, 1, 1, blocks, None, None, C.byref(out)) == MGS_ERR_INVALID
    assert b"mgs_csr_bmat: NULL" in L.mgs_last_error(None) and out.value == 0x1234
    assert L.mgs_csr_bmat_numeric(None, blocks) == MGS_ERR_INVALID
    assert b"mgs_csr_bmat_numeric: NULL" in L.mgs_last_error(None)
    assert L.mgs_csr_bmat_info(None, info) == MGS_ERR_INVALID
    assert b"mgs_csr_bmat_info: NULL" in L.mgs_last_error(None) and list(info) == [9, 9, 9, 9]


TU = r"""
#include "mgs_host.hpp"
using namespace mgs;
int main(int argc, char **argv) {
  if (argc != 2) { std::cout << "usage: A.mtx" << std::endl; return 1; }
  SMatrix A = readMatrix(argv[1]);
  DeviceMatrix Ad(A);
  const void *p_dev = nullptr;                                  // a permutation in device memory (here: none, the identity)
  DeviceMatrix C = Ad.permute(p_dev, p_dev, 32, true);
  DeviceMatrix C64 = Ad.permute(p_dev, nullptr, 64);
  C.permuteUpdate(Ad);                                          // enqueued only
  const DeviceMatrix *grid[4] = {&Ad, nullptr, nullptr, &C};    // block_diag(A, C)
  DeviceMatrix K = DeviceMatrix::bmat(2, 2, grid);
  K.bmatUpdate(2, 2, grid);
  const DeviceMatrix *row[2] = {&Ad, &C};
  int sizes[2] = {Ad.cols(), C.cols()};
  DeviceMatrix H = DeviceMatrix::bmat(1, 2, row, nullptr, sizes);
  return K.rows() == 2 * Ad.rows() && H.cols() == 2 * Ad.cols() && C64.rows() == Ad.rows() ? 0 : 2;
}
"""


def test_cpp_forms_compile_and_link(tmp_path):
    import subprocess
    src = tmp_path / "reorder_tu.cpp"
    src.write_text(TU)
    exe = tmp_path / "reorder_tu"
    libdir = os.path.join(REPO, "multigridsolver_amd")
    assert os.path.exists(os.path.join(libdir, "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O0", "-Wall", "-I", os.path.join(libdir, "cpp"), "-o", str(exe), str(src),
                        "-L" + libdir, "-lmgs", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)      # usage path only: no device is touched
    assert r.returncode == 1 and "usage" in r.stdout
