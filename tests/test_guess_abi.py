"""CPU-only checks that the projected initial guess is offered on every face of the library — the C header, the built libmgs.so, the
ctypes prototypes, the Python package, the C++ header — and that every refusal that can be decided without a device is returned.  The
refusals that need a matrix on a device (not square, halo columns, short vectors) are in tests/test_gpu_guess.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import REPO

INVALID = -1
SYMBOLS = {"mgs_guess_create": 4, "mgs_guess_destroy": 1, "mgs_guess_apply": 4, "mgs_guess_update": 3, "mgs_guess_rebase": 1, "mgs_guess_reset": 1,
           "mgs_guess_info": 2, "mgs_guess_coef": 3, "mgs_guess_gram": 2, "mgs_guess_pair": 4}


def test_symbols_declared_exported_prototyped():
    src = open(os.path.join(REPO, "include", "mgs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"#define\s+MGS_GUESS_ENERGY\s+0\b", code) and re.search(r"#define\s+MGS_GUESS_RESIDUAL\s+1\b", code)
    assert re.search(r"typedef\s+struct\s+mgs_guess\s+mgs_guess\s*;", code)
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
    for meth in ("apply", "update", "rebase", "reset", "info", "coef", "gram", "pair"):
        assert callable(getattr(mg.Guess, meth))


def test_header_comment_in_the_house_style():
    src = open(os.path.join(REPO, "include", "mgs.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*typedef struct mgs_guess", src, flags=re.S)
    assert m, "mgs_guess has no header comment"
    text = " ".join(re.sub(r"\n \*", "\n", m.group(1)).split())          # the comment block's own line starts removed
    for word in ("none: the reference solves one right-hand side, bicg.cpp:159-166", "Fischer", "MGS_ERR_INVALID", "capacity outside 1..16", "row shard",
                 "MGS_NULLSPACE_CONSTANT", "bit for bit", "no atomics", "must outlive"):
        assert word in text, word


def test_refusals_without_a_device():
    import multigridsolver_amd as mg
    L = mg.lib()
    err = lambda: L.mgs_last_error(None).decode()
    out = C.c_void_p(5)
    assert L.mgs_guess_create(None, 0, 8, C.byref(out)) == INVALID and "NULL matrix" in err() and out.value == 5
    assert L.mgs_guess_create(None, 0, 8, None) == INVALID and "NULL" in err()
    for kind in (2, -1, 7):                                # an unknown kind and a capacity outside 1..16 are named before the matrix is looked at
        assert L.mgs_guess_create(None, kind, 8, C.byref(out)) == INVALID and f"unknown kind {kind}" in err()
    for cap in (0, 17, -3):
        for kind in (0, 1):
            assert L.mgs_guess_create(None, kind, cap, C.byref(out)) == INVALID and f"capacity {cap} outside 1..16" in err()
    assert out.value == 5
    r = C.c_double(3.0); a = C.c_int(9)
    assert L.mgs_guess_apply(None, None, None, C.byref(r)) == INVALID and "mgs_guess_apply: NULL" in err() and r.value == 3.0
    assert L.mgs_guess_update(None, None, C.byref(a)) == INVALID and "mgs_guess_update: NULL" in err() and a.value == 9
    assert L.mgs_guess_rebase(None) == INVALID and "mgs_guess_rebase: NULL" in err()
    assert L.mgs_guess_reset(None) == INVALID and "mgs_guess_reset: NULL" in err()
    i6 = (C.c_int64 * 6)()
    assert L.mgs_guess_info(None, i6) == INVALID and "mgs_guess_info: NULL" in err()
    d4 = (C.c_double * 4)()
    assert L.mgs_guess_coef(None, d4, 4) == INVALID and "mgs_guess_coef: NULL" in err()
    assert L.mgs_guess_gram(None, d4) == INVALID and "mgs_guess_gram: NULL" in err()
    assert L.mgs_guess_pair(None, 0, None, None) == INVALID and "mgs_guess_pair: NULL" in err()
    assert L.mgs_guess_destroy(None) == 0                 # as free(NULL)


def test_python_face_refuses_an_unknown_kind_before_the_library_is_asked():
    import multigridsolver_amd as mg
    A = mg.Csr(None, None, owned=False)
    for bad in ("Energy", "l2", 0, None):
        with pytest.raises(ValueError):
            mg.Guess(A, kind=bad)


TU = r"""
#include "mgs_host.hpp"
using namespace mgs;
int main(int argc, char **argv) {
  if (argc != 2) { std::cout << "usage: A.mtx" << std::endl; return 1; }
  DeviceMatrix A(readMatrix(argv[1]));
  SolutionGuess guess(A, MGS_GUESS_RESIDUAL, 8);
  VectorXd x(A.rows()), b(A.rows());
  x.setZero(); b.setZero();
  double rel = guess.apply(b, x);                 // host vectors: x = x0, returns ‖b − A·x0‖/‖b‖
  bool added = guess.update(x);
  guess.rebase();
  guess.reset();
  return (added ? 1 : 0) + guess.size() + guess.capacity() + (int)guess.restarts() + (int)guess.refused() + (rel > 2.0 ? 1 : 0);
}
"""


def test_cpp_face_compiles_and_links(tmp_path):
    src = tmp_path / "guess_tu.cpp"
    src.write_text(TU)
    exe = tmp_path / "guess_tu"
    libdir = os.path.join(REPO, "multigridsolver_amd")
    assert os.path.exists(os.path.join(libdir, "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O0", "-Wall", "-I", os.path.join(libdir, "cpp"), "-o", str(exe), str(src),
                        "-L" + libdir, "-lmgs", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)      # usage path only: no device is touched
    assert r.returncode == 1 and "usage" in r.stdout
