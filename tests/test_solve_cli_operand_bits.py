"""python -m multigridsolver_amd.solve --operand-bits: a single-GPU option.  Under a multi-rank launch it is refused like the CLI's other
single-GPU options, before the library is loaded or a device touched (no GPU needed for this test)."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MTX = os.path.join(REPO, "tests", "golden", "inputs", "CSky3d3.mtx")


def run(args, world):
    env = dict(os.environ, WORLD_SIZE=str(world), RANK="0", LOCAL_RANK="0", PYTHONPATH=REPO)
    # a library path that does not exist: loading libmgs.so (and with it the HIP runtime) would fail loudly instead of the refusal
    env["MGS_LIBMGS"] = os.path.join(REPO, "no_such_dir", "libmgs.so")
    return subprocess.run([sys.executable, "-m", "multigridsolver_amd.solve", MTX] + args, cwd=REPO, env=env, capture_output=True, text=True, timeout=120)


def test_operand_bits_32_refused_on_multi_gpu_launch():
    r = run(["--operand-bits", "32"], world=2)
    assert r.returncode != 0
    assert "multi-GPU" in r.stderr and "operand-bits" in r.stderr, r.stderr
    assert "libmgs" not in r.stderr and "Traceback" not in r.stderr, r.stderr


def test_operand_bits_rejects_other_widths():
    r = run(["--operand-bits", "16"], world=1)
    assert r.returncode == 2 and "invalid choice" in r.stderr, r.stderr
