"""Helper of tests/test_cpp_face_cpu.py and tests/test_gpu_cpp_face.py: compiles the programs of tests/cpp_face (one per family of
multigridsolver_amd/cpp/mgs_host.hpp, each with its own main), runs one as a child process and reads back what it wrote.

A program is called as `program IN_DIR OUT_DIR`.  It reads .mtx files and raw little-endian arrays from IN_DIR and writes to OUT_DIR raw arrays
(NAME.f64, NAME.i32; a device matrix NAME as NAME.rp.i32, NAME.ci.i32, NAME.val.f64) and scalars.txt, one line `NAME i INTEGER` or
`NAME d HEXFLOAT` per scalar.  read_outputs() returns all of it as one dict, and the GPU test builds the same dict through the Python face.

Index lists in device memory (rows_dev, rperm_dev, idx_dev; the arrays of fromDevice / fromCooDevice): mgs_host.hpp offers no raw allocation, so
the programs stage them through an mgs::Vector (tests/cpp_face/face_io.hpp, DevList): the list's bytes are copied into a std::vector<double>,
uploaded, and the address comes from mgs_vec_ptr.  No HIP header and no HIP runtime on the link line.

A child that was killed or died (status 124 or 137 from `timeout`, 134, 139, or a negative status) may have left the device in any state: run()
records it, starts no further child in this session, and fails every later call at once with that record.  Nothing is retried."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpp_face")
LIBDIR = os.path.join(REPO, "multigridsolver_amd")
FAMILIES = ["vector", "algebra", "ingest", "precond", "solvers", "plans", "refusals"]
# seconds a program may take on the device: each one needs a few seconds; the limit only ends a hang
TIME_LIMIT = {"vector": 60, "algebra": 90, "ingest": 60, "precond": 120, "solvers": 120, "plans": 150, "refusals": 90}
DEAD = (124, 137, 134, 139)

_first_death = None


def compile_all(out_dir):
    """→ {family: path of the program}; the command line of the *_abi tests, -Wall with no warning allowed"""
    assert os.path.exists(os.path.join(LIBDIR, "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    exes = {}
    for fam in FAMILIES:
        exe = os.path.join(str(out_dir), "face_" + fam)
        r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-O1", "-Wall", "-I", os.path.join(LIBDIR, "cpp"), "-I", SRC, "-o", exe,
                            os.path.join(SRC, fam + ".cpp"), "-L" + LIBDIR, "-lmgs", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, fam + ":\n" + r.stderr[-4000:]
        assert "warning" not in r.stderr, fam + ":\n" + r.stderr[-4000:]
        exes[fam] = exe
    return exes


def fail_if_a_child_died():
    """called before a test touches the device at all"""
    if _first_death is not None:
        pytest.fail("no further child is started in this session: " + _first_death)


def run(exe, family, in_dir, out_dir):
    """one child under `timeout`; → its stdout.  Fails the test on any status but 0."""
    global _first_death
    fail_if_a_child_died()
    os.makedirs(str(out_dir), exist_ok=True)
    limit = TIME_LIMIT[family]
    r = subprocess.run(["timeout", "-k", "10", str(limit), exe, str(in_dir), str(out_dir)], capture_output=True, text=True, timeout=limit + 30)
    record = f"{family}: status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    if r.returncode in DEAD or r.returncode < 0:
        _first_death = record
    assert r.returncode == 0, record
    return r.stdout


def read_outputs(out_dir):
    out_dir = str(out_dir)
    got = {}
    for fn in sorted(os.listdir(out_dir)):
        p = os.path.join(out_dir, fn)
        if fn.endswith(".f64"):
            got[fn[:-4]] = np.fromfile(p, dtype="<f8")
        elif fn.endswith(".i32"):
            got[fn[:-4]] = np.fromfile(p, dtype="<i4")
    with open(os.path.join(out_dir, "scalars.txt")) as f:
        for line in f:
            name, kind, text = line.split()
            assert name not in got, name
            got[name] = int(text) if kind == "i" else float.fromhex(text)
    return got


class Record(dict):
    """what the Python face computes, under the names the program writes"""

    def vec(self, name, v):
        self[name] = v.numpy() if hasattr(v, "numpy") else np.asarray(v, dtype=np.float64)

    def csr(self, name, M):
        """M: a device Csr; the wrapper's cached shape and the library's are one thing on this face"""
        rp, ci, v = M.download()
        self[name + ".rp"], self[name + ".ci"], self[name + ".val"] = rp, ci, v
        self[name + ".rows"] = self[name + ".lib_rows"] = M.shape[0]
        self[name + ".cols"] = self[name + ".lib_cols"] = M.shape[1]


def bits_equal(a, b):
    """bit equality of two scalars or arrays: −0.0 differs from +0.0, a NaN equals the same NaN"""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape or a.dtype.kind != b.dtype.kind:
            return False
        if a.dtype.kind == "f":
            return np.array_equal(a.astype("<f8").view("<i8"), b.astype("<f8").view("<i8"))
        return np.array_equal(a, b)
    if isinstance(a, float) or isinstance(b, float):
        return isinstance(a, float) and isinstance(b, float) and np.float64(a).view(np.int64) == np.float64(b).view(np.int64)
    return int(a) == int(b)


def compare(cpp, py, skip=()):
    """every name the program wrote against the Python face's, bit for bit; names in `skip` are held to another bar by the caller"""
    assert set(cpp) == set(py), (sorted(set(cpp) - set(py)), sorted(set(py) - set(cpp)))
    wrong = [k for k in sorted(cpp) if k not in skip and not bits_equal(cpp[k], py[k])]
    detail = ""
    if wrong:
        k = wrong[0]
        detail = f"; first: {k}: C++ {cpp[k]!r} Python {py[k]!r}"
        if isinstance(cpp[k], np.ndarray) and cpp[k].shape == np.shape(py[k]) and cpp[k].size:
            d = np.flatnonzero(np.asarray(cpp[k]) != np.asarray(py[k]))
            detail += f"; {d.size} of {cpp[k].size} entries differ, first at {d[:5].tolist()}"
    assert not wrong, f"{len(wrong)} of {len(cpp)} outputs differ: {wrong[:12]}{detail}"


def write_f64(path, a):
    np.ascontiguousarray(a, dtype="<f8").tofile(str(path))


def write_i32(path, a):
    np.ascontiguousarray(a, dtype="<i4").tofile(str(path))
