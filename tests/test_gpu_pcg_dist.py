"""python -m multigridsolver_amd.solve --solver pcg: one process, and 2 ranks (row shards) sharing GPU 0 over gloo, launched as
tests/test_gpu_dist.py::test_solve_cli_single_and_sharded launches them.  The true residual is recomputed by the oracle."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def test_solve_cli_pcg_single_and_sharded(orc, tmp_path):
    import multigridsolver_amd as mg
    Ao = orc.poisson3d(24); n = Ao.shape[0]
    mtx = str(tmp_path / "poisson3d_24.mtx")
    mg.write_mtx(mtx, n, n, Ao.rowptr, Ao.col, Ao.val)
    b = orc.rand_rhs(n)
    counts = {}
    for world in (1, 2):
        dump = str(tmp_path / f"x{world}.bin")
        tail = ["-m", "multigridsolver_amd.solve", mtx, "--solver", "pcg", "--tol", "1e-9", "--dump-x", dump]
        base = [sys.executable] + tail
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MGS_DIST_BACKEND="gloo", MGS_DIST_SHARE_GPU="1")
        if world > 1:
            base = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                    "--master-port", str(28800 + os.getpid() % 1000)] + tail
        r = subprocess.run(base, capture_output=True, text=True, timeout=600, env=env, cwd=REPO)
        assert r.returncode == 0 and "Number of iterations PCG" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
        assert "PCG_SolveTimer" in r.stderr and "BICG" not in r.stdout
        x = np.fromfile(dump, dtype="<f8")
        tr = np.linalg.norm(Ao.residual(x, b)) / np.linalg.norm(b)
        counts[world] = int(re.search(r"Number of iterations PCG\s*: (\d+)", r.stdout).group(1))
        print(f"world {world}: {counts[world]} iterations, true residual {tr:.4e}")
        assert x.size == n and tr < 1.5e-9
    print("iterations by world size (aggregates stop at shard borders):", counts)
