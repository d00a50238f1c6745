"""CPU-only checks that the ingestion from device memory (checked CSR copy, COO assembly, re-assembly through the kept map) is offered on
every face of the library: the C header, the built libmgs.so, the ctypes prototypes, the Python classes and the C++ header; and that the
NULL refusals need no device."""
import ctypes as C
import os
import re
import subprocess

from conftest import REPO

SYMBOLS = {"mgs_csr_from_device": 9, "mgs_csr_from_coo_device": 10, "mgs_csr_update_values_coo_dev": 3, "mgs_csr_coo_info": 2}
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
    assert re.search(r"#define\s+MGS_COO_MAX_ROW\s+8192\b", code)
    for method in ("from_device", "from_coo_device", "from_torch", "update_values_coo", "coo_info"):
        assert callable(getattr(mg.Csr, method)), method


def comment_before(src, name):
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define MGS_COO_MAX_ROW[^\n]*\n)?int %s\(" % name, src, flags=re.S)
    assert m, f"{name} has no header comment"
    return " ".join(m.group(1).split())


def test_header_says_what_a_reader_needs():
    src = open(os.path.join(REPO, "include", "mgs.h")).read()
    common = re.search(r"/\*((?:(?!\*/).)*no host round trip(?:(?!\*/).)*)\*/", src, flags=re.S)
    assert common, "the common rules of the two constructors are not stated"
    common = " ".join(common.group(1).split())
    for word in ("64", "range-checked", "copied", "stream", "synchronises", "caller's job", "MGS_ERR_INVALID", "never faults", "*out"):
        assert word in common, word
    csr = comment_before(src, "mgs_csr_from_device")
    for word in ("MatrixOperations.cu:121-146", "no reference counterpart", "ascending", "monotone", "row boundary", "MGS_ERR_INVALID", "lowest offending row"):
        assert word in csr, word
    coo = comment_before(src, "mgs_csr_from_coo_device")
    for word in ("MatrixIO.cpp:12-37", "no reference counterpart", "ascending", "input order", "-0.0", "MGS_COO_MAX_ROW", "MGS_ERR_INVALID", "keep_map", "64"):
        assert word in coo, word
    upd = comment_before(src, "mgs_csr_update_values_coo_dev")
    for word in ("MatrixIO.cpp:12-37", "no reference counterpart", "MGS_ERR_STATE", "MGS_ERR_INVALID", "keep_map", "bit-identical", "not synchronised", "mgs_hier_refresh", "valcode"):
        assert word in upd, word
    info = comment_before(src, "mgs_csr_coo_info")
    for word in ("no reference counterpart", "out[0]", "out[3]"):
        assert word in info, word


def test_null_arguments_refused_without_a_device():
    import multigridsolver_amd as mg
    L = mg.lib()
    out = C.c_void_p(0x1234)                       # a refusal leaves it as it was
    buf = (C.c_int64 * 4)()
    p = C.cast(buf, C.c_void_p)
    assert L.mgs_csr_from_device(None, 1, 1, 0, p, p, 32, p, C.byref(out)) == MGS_ERR_INVALID
    assert b"NULL" in L.mgs_last_error(None) and out.value == 0x1234
    assert L.mgs_csr_from_coo_device(None, 1, 1, 1, p, p, 32, p, 0, C.byref(out)) == MGS_ERR_INVALID
    assert b"NULL" in L.mgs_last_error(None) and out.value == 0x1234
    fake_ctx = C.c_void_p(0)                       # NULL context with every other argument present, and NULL `out` behind a NULL context
    assert L.mgs_csr_from_device(fake_ctx, 1, 1, 0, p, p, 32, p, None) == MGS_ERR_INVALID
    assert L.mgs_csr_from_coo_device(fake_ctx, 1, 1, 1, p, p, 64, p, 1, None) == MGS_ERR_INVALID
    assert L.mgs_csr_update_values_coo_dev(None, p, 4) == MGS_ERR_INVALID
    assert b"NULL" in L.mgs_last_error(None)
    assert L.mgs_csr_coo_info(None, buf) == MGS_ERR_INVALID
    assert b"NULL" in L.mgs_last_error(None)


def test_python_refuses_host_arrays_and_wrong_dtypes_without_a_device():
    import numpy as np
    import pytest
    import torch
    from multigridsolver_amd import core

    class Ctx:                                     # the type checks run before anything is handed to the library
        h, device = None, 0
    a = np.zeros(3, dtype=np.int32)
    with pytest.raises(TypeError):
        core._dev_array(Ctx, a, "rowptr", True)                     # a host array is not converted or uploaded silently
    with pytest.raises(TypeError):
        core._dev_array(Ctx, torch.zeros(3, dtype=torch.int32), "rowptr", True)      # a CPU tensor

    class Cai:
        def __init__(self, typestr, shape, strides=None):
            self.__cuda_array_interface__ = {"data": (4096, False), "typestr": typestr, "shape": shape, "strides": strides, "version": 3}
    assert core._dev_array(Ctx, Cai("<i8", (5,)), "col", True) == (4096, 5, 64)
    assert core._dev_array(Ctx, Cai("<i4", (5,), (4,)), "col", True) == (4096, 5, 32)
    assert core._dev_array(Ctx, Cai("<f8", (7,)), "val", False) == (4096, 7, 0)
    for bad, index in ((Cai("<i2", (5,)), True), (Cai("<f8", (5,)), True), (Cai("<f4", (5,)), False), (Cai("<i8", (5,)), False), (Cai("<i4", (5,), (8,)), True),
                       (Cai("<i4", (5, 2)), True)):
        with pytest.raises(TypeError):
            core._dev_array(Ctx, bad, "x", index)


TU = r"""
#include "mgs_host.hpp"
using namespace mgs;
int main(int argc, char **argv) {
  if (argc != 2) { std::cout << "usage: ntrip   (assembles an ntrip x ntrip diagonal matrix from device triples)" << std::endl; return 1; }
  const int n = std::atoi(argv[1]);
  Vector val(n);                                  // device memory of the library stands in for the caller's
  const void *idx = nullptr, *rowptr = nullptr;   // a real caller passes its device index arrays here
  DeviceMatrix A = DeviceMatrix::fromDevice(n, n, n, rowptr, idx, 64, mgs_vec_ptr(val.handle()));
  DeviceMatrix B = DeviceMatrix::fromCooDevice(n, n, n, idx, idx, 32, mgs_vec_ptr(val.handle()), true);
  DeviceMatrix B0 = DeviceMatrix::fromCooDevice(n, n, n, idx, idx, 32, mgs_vec_ptr(val.handle()));
  B.update_values_coo(mgs_vec_ptr(val.handle()), n);
  return A.rows() + B.rows() + B0.cols() > 0 ? 0 : 2;
}
"""


def test_cpp_ingest_forms_compile_and_link(tmp_path):
    src = tmp_path / "ingest_tu.cpp"
    src.write_text(TU)
    exe = tmp_path / "ingest_tu"
    libdir = os.path.join(REPO, "multigridsolver_amd")
    assert os.path.exists(os.path.join(libdir, "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O0", "-Wall", "-I", os.path.join(libdir, "cpp"), "-o", str(exe), str(src),
                        "-L" + libdir, "-lmgs", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)      # usage path only: no device is touched
    assert r.returncode == 1 and "usage" in r.stdout
