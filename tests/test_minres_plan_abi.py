"""CPU-only checks that the MINRES plan (device-resident scalars, enqueue-only solves) and the values-only transpose are offered on every
face of the library: the C header, the built libmgs.so, the ctypes prototypes, the Python package, the solve CLI and the C++ header."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from conftest import REPO

FUNCS = {"mgs_minres_plan_create": 3, "mgs_minres_plan_destroy": 1, "mgs_minres_plan_solve": 7, "mgs_minres_plan_enqueue": 5,
         "mgs_minres_plan_result": 5, "mgs_minres_plan_info": 2, "mgs_csr_transpose_numeric": 3}
MGS_ERR_INVALID = -1


def test_declared_exported_prototyped():
    src = open(os.path.join(REPO, "include", "mgs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"typedef\s+struct\s+mgs_minres_plan\s+mgs_minres_plan\s*;", code), "include/mgs.h does not declare the handle type"
    assert code.index("mgs_fgcr_plan_info") < code.index("mgs_minres_plan_create"), "the block stands behind the FGCR plan's"
    block = src[src.index("MINRES with device-resident scalars"):src.index("typedef struct mgs_minres_plan")]
    for word in ("src/CPU_Matlab/solve.m:28-33", "LANCZOS", "ROTATE", "apply", "frozen", "why", "deterministic", "create:", "solve:", "enqueue:", "result", "info:",
                 "NO RECALIBRATION ON THE DEVICE", "tol = 0", "nu1 == nu2", "null space", "MGS_ERR_INVALID", "MGS_ERR_STATE"):
        assert word in block, f"the header comment of the plan does not mention {word}"
    m = re.search(r"mgs_csr_transpose_numeric —((?:(?!\*/).)*)\*/", src, flags=re.S)
    assert m, "mgs_csr_transpose_numeric has no header comment"
    text = " ".join(m.group(1).replace(" * ", " ").split())
    for word in ("bisection", "64-bit word", "-0.0", "NaN", "No map is kept", "no atomics", "counted and never written", "mgs_hier_refresh", "mgs_csr_scale works in place",
                 "scaled again", "misses == NULL", "MGS_ERR_STATE", "MGS_ERR_INVALID", "valcode"):
        assert word in text, word
    import multigridsolver_amd as mg
    from multigridsolver_amd._lib import PROTOTYPES
    L = C.CDLL(mg.SO_PATH)
    for name, nargs in FUNCS.items():
        m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"include/mgs.h does not declare {name}"
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(L, name), f"libmgs.so does not export {name}"
        res, argtypes = PROTOTYPES[name]
        assert res is C.c_int and len(argtypes) == nargs, name
    assert list(PROTOTYPES["mgs_minres_plan_solve"][1]) == list(PROTOTYPES["mgs_bicgstab_plan_solve"][1])
    assert list(PROTOTYPES["mgs_minres_plan_enqueue"][1]) == list(PROTOTYPES["mgs_bicgstab_plan_enqueue"][1])
    assert list(PROTOTYPES["mgs_minres_plan_result"][1]) == list(PROTOTYPES["mgs_bicgstab_plan_result"][1])
    assert list(PROTOTYPES["mgs_csr_transpose_numeric"][1]) == [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    assert " ".join(re.search(r"int\s+mgs_csr_transpose_numeric\s*\(([^)]*)\)", code).group(1).split()) == "const mgs_csr *A, mgs_csr *At, int64_t *misses"
    from multigridsolver_amd import core
    assert mg.MinresPlan is core.MinresPlan and issubclass(mg.MinresPlan, core._KrylovPlan)
    for meth in ("solve", "enqueue", "result", "info", "close"):
        assert callable(getattr(mg.MinresPlan, meth))
    assert callable(mg.Csr.transpose_update)
    mk = open(os.path.join(REPO, "multigridsolver_amd", "csrc", "Makefile")).read()
    assert "minres_plan.hip" in mk
    unit = open(os.path.join(REPO, "multigridsolver_amd", "csrc", "minres_plan.hip")).read()
    assert "#pragma clang fp contract(off)" in unit and "krylov::Plan<MinresState>" in unit and "Lookahead" in unit


def test_refusals_need_no_device():
    import multigridsolver_amd as mg
    L = mg.lib()
    out = C.c_void_p(0x1234)
    assert L.mgs_minres_plan_create(None, None, C.byref(out)) == MGS_ERR_INVALID
    assert b"mgs_minres_plan_create: NULL" in L.mgs_last_error(None) and out.value == 0x1234
    mi, t, st = C.c_int(5), C.c_double(1e-6), C.c_int(-1)
    assert L.mgs_minres_plan_solve(None, None, None, 0, C.byref(mi), C.byref(t), C.byref(st)) == MGS_ERR_INVALID
    assert b"mgs_minres_plan_solve: NULL" in L.mgs_last_error(None) and (mi.value, st.value) == (5, -1)
    assert L.mgs_minres_plan_enqueue(None, None, None, 1, 1e-6) == MGS_ERR_INVALID
    assert b"mgs_minres_plan_enqueue: NULL" in L.mgs_last_error(None)
    assert L.mgs_minres_plan_result(None, None, None, None, None) == MGS_ERR_INVALID
    assert b"mgs_minres_plan_result: NULL" in L.mgs_last_error(None)
    info = (C.c_int64 * 6)(*([9] * 6))
    assert L.mgs_minres_plan_info(None, info) == MGS_ERR_INVALID
    assert b"mgs_minres_plan_info: NULL" in L.mgs_last_error(None) and list(info) == [9] * 6
    assert L.mgs_minres_plan_destroy(None) == 0
    miss = C.c_int64(7)
    assert L.mgs_csr_transpose_numeric(None, None, C.byref(miss)) == MGS_ERR_INVALID
    assert b"mgs_csr_transpose_numeric: NULL" in L.mgs_last_error(None) and miss.value == 7


def test_solve_cli_lists_minres_ahead(monkeypatch):
    r = subprocess.run([sys.executable, "-m", "multigridsolver_amd.solve", "--help"], capture_output=True, text=True, cwd=REPO, timeout=120)
    assert r.returncode == 0, r.stderr
    text = " ".join(r.stdout.split())
    opts = text[text.index("options:"):]
    m = re.search(r"--minres-ahead N (.*?) --omega", opts)
    assert m and "--solver minres" in m.group(1) and "MinresPlan" in m.group(1), text
    from multigridsolver_amd import solve
    # accepted with --solver minres: the run gets past the argument checks and fails at the matrix file
    with pytest.raises(Exception) as e:
        solve.main(["no_such_file.mtx", "--solver", "minres", "--minres-ahead", "1"])
    assert not isinstance(e.value, SystemExit) or "goes with --solver" not in str(e.value), str(e.value)
    assert "no_such_file.mtx" in str(e.value)
    # refused with another solver, with none named, and with a negative N; the refusals come before any file is read or any device is touched
    for extra in (["--solver", "bicgstab", "--minres-ahead", "1"], ["--minres-ahead", "1"], ["--solver", "pcg", "--minres-ahead", "0"],
                  ["--solver", "minres", "--minres-ahead", "-1"]):
        with pytest.raises(SystemExit) as e:
            solve.main(["no_such_file.mtx"] + extra)
        assert "--minres-ahead N (N >= 0) goes with --solver minres" in str(e.value), (extra, str(e.value))
    # --solver minres --ahead N stays refused, and the message names both flags
    with pytest.raises(SystemExit) as e:
        solve.main(["no_such_file.mtx", "--solver", "minres", "--ahead", "1"])
    assert "--ahead" in str(e.value)
    monkeypatch.setenv("WORLD_SIZE", "2"); monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:
        solve.main(["no_such_file.mtx", "--solver", "minres", "--minres-ahead", "1"])
    assert "minres" in str(e.value) and "single GPU" in str(e.value)


TU = r"""
#include "mgs_host.hpp"
using namespace mgs;
int main(int argc, char **argv) {
  if (argc != 4) { std::cout << "usage: K.mtx B.mtx P.mtx" << std::endl; return 1; }
  SMatrix K = readMatrix(argv[1]), B = readMatrix(argv[2]), P = readMatrix(argv[3]);
  MultiGridPrecond::Options o; o.omega = 0.6;
  MultiGridPrecond precond(B, P, o);                    // the preconditioner's operator is block_diag(L, S), not K
  DeviceMatrix Kd(K);
  VectorXd x(K.rows()), b(K.rows());
  x.setZero(); b.setZero();
  int max_iter = 10; double tol = 1e-6;
  MinresPlan plan(Kd, precond);
  int s0 = plan.solve(x, b, max_iter, tol);             // mgs_minres's contract, one iteration kept enqueued ahead
  int s1 = plan.solve(x, b, max_iter, tol, 0);
  DeviceMatrix Kt = Kd.transpose();
  Kt.transposeUpdate(Kd);                               // enqueued only
  int64_t misses = -1;
  Kt.transposeUpdate(Kd, &misses);                      // synchronises, throws unless misses == 0
  precond.refresh();
  plan.enqueue(x, b, 5, 1e-6);                          // no host wait
  int it = 0; double resid = 0.0, est = 0.0;
  int s2 = plan.result(it, resid);
  int s3 = plan.result(it, resid, &est);
  try { plan.enqueue(x, x, 5, 1e-6); } catch (const mgs::Error &) { return 9; }
  return s0 + s1 + s2 + s3 + (int)misses + (int)plan.info(5) + (plan.handle() ? 0 : 1);
}
"""


def test_cpp_minres_plan_compiles_and_links(tmp_path):
    src = tmp_path / "minres_plan_tu.cpp"
    src.write_text(TU)
    exe = tmp_path / "minres_plan_tu"
    libdir = os.path.join(REPO, "multigridsolver_amd")
    assert os.path.exists(os.path.join(libdir, "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O0", "-Wall", "-I", os.path.join(libdir, "cpp"), "-o", str(exe), str(src),
                        "-L" + libdir, "-lmgs", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    # usage path only: no device is touched
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "usage" in r.stdout
