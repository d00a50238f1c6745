"""CPU-only checks that the FGCR plan (device-resident coefficients, enqueue-only solves) is offered on every face of the library: the C header,
the built libmgs.so, the ctypes prototypes, the Python package, the solve CLI and the C++ header."""
import ctypes as C
import os
import re
import subprocess
import sys

from conftest import REPO

FUNCS = {"mgs_fgcr_plan_create": 4, "mgs_fgcr_plan_destroy": 1, "mgs_fgcr_plan_solve": 7, "mgs_fgcr_plan_enqueue": 5,
         "mgs_fgcr_plan_result": 5, "mgs_fgcr_plan_info": 2}


def test_declared_exported_prototyped():
    src = open(os.path.join(REPO, "include", "mgs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"typedef\s+struct\s+mgs_fgcr_plan\s+mgs_fgcr_plan\s*;", code), "include/mgs.h does not declare the handle type"
    assert code.index("mgs_bicgstab_plan_info") < code.index("mgs_fgcr_plan_create"), "the block stands behind the BiCGSTAB plan's"
    # the header names the nearest reference line and states the contract
    block = src[src.index("flexible GCR with device-resident coefficients"):src.index("typedef struct mgs_fgcr_plan")]
    for word in ("src/CPU_Matlab/solve.m:28-33", "COEF", "RHOK", "RES", "YSOLVE", "WIN", "m_open", "frozen", "restart in 1..16", "create:", "solve:", "enqueue:",
                 "result", "info:", "MGS_ERR_INVALID", "MGS_ERR_STATE"):
        assert word in block, f"the header comment of the plan does not mention {word}"
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
    assert PROTOTYPES["mgs_fgcr_plan_enqueue"][1][4] is C.c_double and PROTOTYPES["mgs_fgcr_plan_solve"][1][3] is C.c_int
    assert PROTOTYPES["mgs_fgcr_plan_create"][1][2] is C.c_int
    assert callable(mg.FgcrPlan)
    for meth in ("solve", "enqueue", "result", "info", "close"):
        assert callable(getattr(mg.FgcrPlan, meth))


def test_solve_cli_lists_fgcr_ahead():
    r = subprocess.run([sys.executable, "-m", "multigridsolver_amd.solve", "--help"], capture_output=True, text=True, cwd=REPO, timeout=120)
    assert r.returncode == 0, r.stderr
    text = " ".join(r.stdout.split())
    opts = text[text.index("options:"):]
    m = re.search(r"--fgcr-ahead N (.*?) --kcycle-energy", opts)
    assert m and "--solver fgcr" in m.group(1) and "FgcrPlan" in m.group(1), text
    assert opts.index("--kcycle KCYCLE") < opts.index("--fgcr-ahead N")
    # accepted with --solver fgcr: the run gets past the argument check and fails at the matrix file
    r = subprocess.run([sys.executable, "-m", "multigridsolver_amd.solve", "nowhere.mtx", "--solver", "fgcr", "--fgcr-ahead", "1"], capture_output=True, text=True,
                       cwd=REPO, timeout=120)
    assert r.returncode != 0 and "goes with --solver" not in r.stderr and "nowhere.mtx" in r.stderr
    # refused with another solver, with none named, and with a negative N
    for extra in (["--solver", "bicgstab", "--fgcr-ahead", "1"], ["--fgcr-ahead", "1"], ["--solver", "pcg", "--fgcr-ahead", "0"], ["--solver", "fgcr", "--fgcr-ahead", "-1"]):
        r = subprocess.run([sys.executable, "-m", "multigridsolver_amd.solve", "nowhere.mtx"] + extra, capture_output=True, text=True, cwd=REPO, timeout=120)
        assert r.returncode != 0 and "--fgcr-ahead N (N >= 0) goes with --solver fgcr" in r.stderr, (extra, r.stderr)
    # --solver fgcr --ahead N stays refused, with the message that names --solver bicgstab
    r = subprocess.run([sys.executable, "-m", "multigridsolver_amd.solve", "nowhere.mtx", "--solver", "fgcr", "--ahead", "1"], capture_output=True, text=True, cwd=REPO, timeout=120)
    assert r.returncode != 0 and "--solver bicgstab" in r.stderr


TU = r"""
#include "mgs_host.hpp"
using namespace mgs;
int main(int argc, char **argv) {
  if (argc != 3) { std::cout << "usage: A.mtx P.mtx" << std::endl; return 1; }
  SMatrix A = readMatrix(argv[1]), P = readMatrix(argv[2]);
  MultiGridPrecond precond(A, P);
  VectorXd x(A.rows()), b(A.rows());
  x.setZero(); b.setZero();
  int max_iter = 10; double tol = 1e-6;
  FgcrPlan plan(precond.matrix(), precond);             // FGCR(10)
  FgcrPlan plan16(precond.matrix(), precond, 16);
  int s0 = plan.solve(x, b, max_iter, tol);             // mgs_fgcr's contract, nothing speculative
  int s1 = plan16.solve(x, b, max_iter, tol, 4);
  SolutionGuess guess(precond.matrix(), MGS_GUESS_RESIDUAL);
  guess.applyAsync(b, x);
  plan.enqueue(x, b, 5, 1e-6);                          // no host wait
  int it = 0; double resid = 0.0, rec = 0.0;
  int s2 = plan.result(it, resid);
  int s3 = plan.result(it, resid, &rec);
  guess.update(x);
  try { plan.enqueue(x, x, 5, 1e-6); } catch (const mgs::Error &) { return 9; }
  return s0 + s1 + s2 + s3 + (int)plan.info(3) + (plan.handle() ? 0 : 1);
}
"""


def test_cpp_fgcr_plan_compiles_and_links(tmp_path):
    src = tmp_path / "fgcr_plan_tu.cpp"
    src.write_text(TU)
    exe = tmp_path / "fgcr_plan_tu"
    libdir = os.path.join(REPO, "multigridsolver_amd")
    assert os.path.exists(os.path.join(libdir, "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O0", "-Wall", "-I", os.path.join(libdir, "cpp"), "-o", str(exe), str(src),
                        "-L" + libdir, "-lmgs", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    # usage path only: no device is touched
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "usage" in r.stdout
