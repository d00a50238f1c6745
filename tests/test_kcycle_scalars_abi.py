"""CPU-only checks that the K step's scalars are offered on every face of the library — the C header, the built libmgs.so, the ctypes
prototypes, the Python class, the documents — that the header says which product each scalar is, and that the refusals need no device."""
import ctypes as C
import os
import re

from conftest import REPO

MGS_ERR_INVALID = -1


def header():
    return open(os.path.join(REPO, "include", "mgs.h")).read()


def test_name_declared_exported_prototyped_documented():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    import multigridsolver_amd as mg
    from multigridsolver_amd import _lib
    m = re.search(r"int\s+mgs_hier_kcycle_scalars\s*\(([^)]*)\)\s*;", code)
    assert m, "include/mgs.h does not declare mgs_hier_kcycle_scalars"
    assert " ".join(m.group(1).split()) == "mgs_hier *h, int level, double out[5]", m.group(1)
    assert hasattr(C.CDLL(mg.SO_PATH), "mgs_hier_kcycle_scalars"), "libmgs.so does not export mgs_hier_kcycle_scalars"
    res, got = _lib.PROTOTYPES["mgs_hier_kcycle_scalars"]
    assert res is C.c_int and list(got) == [C.c_void_p, C.c_int, C.POINTER(C.c_double)], got
    for method in ("kcycle_scalars", "set_kcycle_entry", "set_kcycle"):
        assert callable(getattr(mg.Hierarchy, method)), method
    assert "`mgs_hier_kcycle_scalars`" in open(os.path.join(REPO, "INTEGRATION.md")).read()
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    for path in ("tests/test_gpu_kcycle.py", "tests/kcycle_ref.py"):
        assert path in design and os.path.exists(os.path.join(REPO, path)), path


def test_header_says_which_product_each_scalar_is():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mgs_hier_kcycle_scalars\(", header(), flags=re.S)
    assert m, "mgs_hier_kcycle_scalars has no header comment"
    text = " ".join(m.group(1).split())
    for word in ("ρ1", "α1", "γ", "ρ2", "α2", "GCR form", "energy form", "kcycle_energy", "v1·v1", "c1·v1", "v1·rhs", "c1·rhs", "v2·v1", "c2·v1",
                 "v2'·v2'", "c2'·v2'", "v2'·r'", "c2'·r'", "ρ2 > 0", "ρ1 = 0", "MGS_ERR_INVALID", "MGS_ERR_STATE", "mgs_hier_set_kcycle_entry", "stream"):
        assert word in text, word


def test_refusals_need_no_device():
    import multigridsolver_amd as mg
    L = mg.lib()
    out = (C.c_double * 5)(9, 9, 9, 9, 9)
    assert L.mgs_hier_kcycle_scalars(None, 0, out) == MGS_ERR_INVALID
    assert b"mgs_hier_kcycle_scalars: NULL" in L.mgs_last_error(None) and list(out) == [9.0] * 5
