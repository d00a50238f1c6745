"""bench.py's command line and --dump-outputs writer, on CPU: the checks that run before any device work, and the sample that stands in for
an output larger than the dump's 64 MB budget (fixed rows, float64, the same files in every run)."""
import os
import subprocess
import sys

import numpy as np

from conftest import REPO

sys.path.insert(0, REPO)
import bench  # noqa: E402


def _run(*argv):
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *argv], capture_output=True, text=True, timeout=120, cwd=REPO)


def test_rejects_zero_steps():
    p = _run("--steps", "0")
    assert p.returncode != 0 and "--steps must be at least 1" in p.stderr and p.stdout == ""


def test_dump_outputs_one_gpu_only():
    p = _run("--gpus", "2", "--dump-outputs", "somewhere")
    assert p.returncode != 0 and "--dump-outputs" in p.stderr and p.stdout == ""


def test_dump_small_output_whole(tmp_path):
    x = np.random.default_rng(3).random(1000)
    assert bench.dump_outputs(str(tmp_path), x) == ["x"]
    y = np.load(tmp_path / "x.npy")
    assert y.dtype == np.float64 and np.array_equal(x, y)


def test_dump_large_output_fixed_sample(tmp_path):
    n = bench.DUMP_MAX_BYTES // 8 + 12345                         # one vector over the budget
    x = np.arange(n, dtype=np.float64) * 0.5
    outs = []
    for k in range(2):
        d = tmp_path / str(k)
        assert bench.dump_outputs(str(d), x) == ["x_sample", "x_sample_index"]
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= bench.DUMP_MAX_BYTES
        v, i = np.load(d / "x_sample.npy"), np.load(d / "x_sample_index.npy")
        assert v.dtype == np.float64 and i.dtype == np.float64 and v.shape == i.shape == (bench.DUMP_SAMPLE_ROWS,)
        assert np.all(np.diff(i) > 0) and i[0] >= 0 and i[-1] < n
        assert np.array_equal(v, x[i.astype(np.int64)])
        outs.append((v, i))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
