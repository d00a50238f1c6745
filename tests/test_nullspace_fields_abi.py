"""CPU-only checks that the field-wise null space is offered on every face of the library: the C header with its contract words, the built
libmgs.so, the ctypes prototypes, the Python package, the generator, the C++ header — and that what can be decided without a device is."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO

INVALID = -1
NEW = {"mgs_csr_set_nullspace_fields": 4, "mgs_csr_nullspace_fields": 3, "mgs_vec_project_fields": 4}


def test_symbols_declared_exported_prototyped():
    src = open(os.path.join(REPO, "include", "mgs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"#define\s+MGS_NULLSPACE_FIELDS\s+2\b", code) and re.search(r"#define\s+MGS_NULLSPACE_MAX_FIELDS\s+8\b", code)
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
    for meth in ("set_nullspace_fields", "nullspace_fields", "nullspace"):
        assert callable(getattr(mg.Csr, meth))
    assert callable(mg.Vec.project_fields)


def test_header_documents_the_contract():
    src = " ".join(open(os.path.join(REPO, "include", "mgs.h")).read().split())
    for words in ("MGS_NULLSPACE_FIELDS", "in no field", "NOT verified", "the lowest offending row", "a field without rows", "2³² does not alias 0",
                  "x ← Πx before EVERY true residual", "normb = ‖Πb‖", "z̃ ← Π(M·v)", "the caller's b is only read",
                  "that the two label ARRAYS agree is the caller's responsibility", "naming mgs_minres / mgs_pcg",
                  "an aggregate takes the label of its first member", "A_c + Σ_f (s/n_cf)·z_cf·z_cfᵀ", "mgs_hier_refresh keeps them",
                  "|m_f − mean_f| <= n_f·ε·max|v|", "two identical calls give identical bits", "fl(v_i − m_f)"):
        assert words in src, f"include/mgs.h does not say: {words}"


def test_null_and_bad_arguments_are_refused_without_a_device():
    import multigridsolver_amd as mg
    L = mg.lib()
    nf = C.c_int(7); cnt = (C.c_int64 * 8)(*([5] * 8))
    dummy = C.c_void_p(256)
    for bits, nfields in ((32, 1), (64, 8), (16, 1), (32, 0), (32, 9)):
        assert L.mgs_csr_set_nullspace_fields(None, dummy, bits, nfields) == INVALID
    assert b"mgs_csr_set_nullspace_fields" in L.mgs_last_error(None) and b"NULL" in L.mgs_last_error(None)
    assert L.mgs_csr_nullspace_fields(None, C.byref(nf), cnt) == INVALID and nf.value == 7 and list(cnt) == [5] * 8
    assert L.mgs_vec_project_fields(None, None, None, None) == INVALID
    assert b"mgs_vec_project_fields" in L.mgs_last_error(None)
    assert L.mgs_csr_set_nullspace(None, 2) == INVALID


def test_python_face_checks_before_the_library_is_asked():
    import multigridsolver_amd as mg
    A = mg.Csr(None, None, owned=False)
    with pytest.raises(TypeError):
        A.set_nullspace_fields(np.zeros(4))                    # float labels
    with pytest.raises(TypeError):
        A.set_nullspace_fields([0, 1, -1])                     # neither a device tensor nor a numpy array
    with pytest.raises(ValueError):
        A.set_nullspace("fields")                              # the kind is entered through set_nullspace_fields only


def test_generator_shapes():
    from multigridsolver_amd.synthetic import enclosed_stokes
    g = enclosed_stokes(3)
    m = 27
    assert g["m"] == m and g["n"] == 4 * m and g["labels"].shape == (4 * m,)
    assert (g["labels"][:3 * m] == -1).all() and (g["labels"][3 * m:] == 0).all()
    rp, ci, v = g["D"]
    assert rp[-1] == 6 * m == len(ci) and (np.diff(ci.reshape(m, 6), axis=1) > 0).all()
    assert np.bincount(ci, weights=v, minlength=3 * m).tolist() == [0.0] * (3 * m)      # every column of D sums to 0
    rp, ci, v = g["L"]
    assert len(rp) == 3 * m + 1 and rp[-1] == len(ci) == 3 * len(g["P"][1]) and ci.max() == 3 * m - 1


TU = r"""
#include "mgs_host.hpp"
using namespace mgs;
int main(int argc, char **argv) {
  if (argc != 2) { std::cout << "usage: A.mtx" << std::endl; return 1; }
  DeviceMatrix A(readMatrix(argv[1]));
  const void *labels_dev = nullptr;              // rows() int32 labels in device memory (the caller's)
  A.setNullspaceFields(labels_dev, 32, 2);
  std::vector<int64_t> counts = A.nullspaceFields();
  A.setNullspaceConstant(false);
  return (int)counts.size();
}
"""


def test_cpp_face_compiles_and_links(tmp_path):
    src = tmp_path / "nsf_tu.cpp"
    src.write_text(TU)
    exe = tmp_path / "nsf_tu"
    libdir = os.path.join(REPO, "multigridsolver_amd")
    assert os.path.exists(os.path.join(libdir, "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O0", "-Wall", "-I", os.path.join(libdir, "cpp"), "-o", str(exe), str(src),
                        "-L" + libdir, "-lmgs", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)      # usage path only: no device is touched
    assert r.returncode == 1 and "usage" in r.stdout
