"""The derived operands of the fused passes (wd → Â → val_nd / FP32 copy / packed copy, A·P → FP32 copy / packed copy) through COMPOUND transitions:
a new ω, new values + refresh, the FP32 switch and the options pack7 / pre_nodiag, each changed while another change is still pending.  The
neighbours (test_gpu_refresh, test_gpu_pre_nodiag, test_gpu_pack7, test_gpu_operand_precision) take one transition at a time.

Poisson 24³, level 0 grouped and packed at this size (the small-level settings of test_gpu_pack7.py::test_whole_cycle_and_rebuilt_operands), one
pairwise pass per level — so a refreshed hierarchy and a twin built on the new values from pushed 0/1 transfers of the same aggregates agree bit
for bit.  After every step one V-cycle of the walked hierarchy has the bits of
  * the twin, freshly built under the same values, ω and operand precision, and
  * the walked hierarchy itself with pack7 and pre_nodiag both off (neither option rounds anything).
No tolerance anywhere.  The kept-graph answers of refresh_info() and the bytes the walk leaves in use beyond a twin's are the figures the library
gave for this walk before its operand code was gathered in hier_operands.hip (KEPT, EXTRA_BYTES below)."""
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_refresh import agg_P

pytestmark = pytest.mark.gpu

N = 24
OPTIONS = (("group_stray_pct", 100, 6), ("group_min_blocks", 16, 1024), ("aggpre_max_rows", 1000, 300000), ("pack7", 1, 1), ("pre_nodiag", 1, 1))
KEPT = {"1": 1, "3": 1, "5a": 1, "5b": 1}      # refresh_info()["kept_graphs"] after the refreshes of steps 1, 3 and 5
EXTRA_BYTES = 110592                             # arena bytes in use after the walk (10399744) minus those of a fresh twin after its first cycle (10289152)


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


def values(v, rp, ci, seed):
    """a symmetric rescaling of v: every value moves, diagonals differ row to row"""
    s = 1.0 + 0.2 * np.random.default_rng(seed).random(len(rp) - 1)
    return v * s[np.repeat(np.arange(len(rp) - 1), np.diff(rp))] * s[ci] * (1.0 + 0.05 * seed)


def twin_of(ctx, mg, h, rp, ci, v, omega, bits):
    """a hierarchy built from scratch on a fresh upload of (rp, ci, v) with h's aggregates, level by level"""
    A2 = ctx.csr(len(rp) - 1, len(rp) - 1, rp, ci, v)
    h2 = mg.Hierarchy(A2, omega, 1, 1)
    for l in range(h.nlev - 1):
        P = agg_P(h.level_P(l).agg(), h.level_shape(l + 1)[0])
        h2.push_P(ctx.csr(P.shape[0], P.shape[1], P.indptr, P.indices, P.data))
    h2.finalize()
    if bits == 32:
        h2.set_operand_precision(32)
    return A2, h2


def walk(ctx, A, h, rp, ci, v, check):
    """the five steps; check(step, values, omega, bits) after each (and inside step 2, on FP32 operands); returns refresh_info()'s kept_graphs"""
    kept = {}
    v1, v2, v3, v5 = (values(v, rp, ci, k) for k in (1, 2, 3, 5))
    # 1. a new ω and new values, no cycle in between
    h.set_smoother(0.8, 1, 1); A.update_values(v1); h.refresh()
    kept["1"] = h.refresh_info()["kept_graphs"]
    check("1", v1, 0.8, 64)
    # 2. new values while the level runs on FP32 copies, then back
    h.set_operand_precision(32); A.update_values(v2); h.refresh()
    check("2 (fp32)", v2, 0.8, 32)
    h.set_operand_precision(64)
    check("2", v2, 0.8, 64)
    # 3. new values while the packed copies are switched off, then back
    ctx.set_option("pack7", 0); A.update_values(v3); h.refresh()
    kept["3"] = h.refresh_info()["kept_graphs"]
    ctx.set_option("pack7", 1)
    check("3", v3, 0.8, 64)
    # 4. a new ω and a cycle while the compact operand is switched off, then back
    ctx.set_option("pre_nodiag", 0); h.set_smoother(0.6, 1, 1); h.vcycle(check.b, check.x); ctx.set_option("pre_nodiag", 1)
    check("4", v3, 0.6, 64)
    # 5. two refreshes in a row
    A.update_values(v5); h.refresh()
    kept["5a"] = h.refresh_info()["kept_graphs"]
    h.refresh()
    kept["5b"] = h.refresh_info()["kept_graphs"]
    check("5", v5, 0.6, 64)
    return kept


def built(ctx, mg):
    """options set, the walked hierarchy with one cycle run; the caller restores the options"""
    for k, on, _ in OPTIONS:
        ctx.set_option(k, on)
    A = ctx.poisson3d(N)
    rp, ci, v = A.download()
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 1, 8.0, 200, 32).finalize()
    return A, h, rp, ci, v


def restore(ctx):
    for k, _, default in OPTIONS:
        ctx.set_option(k, default)


def test_compound_transitions_keep_every_operand_in_step(ctx, mg):
    n = N ** 3
    try:
        A, h, rp, ci, v = built(ctx, mg)
        b, x = ctx.vec(n).rand(seed=7), ctx.vec(n)
        h.vcycle(b, x)
        # the walk is not vacuous: level 0 runs the grouped pre pass on the packed copy of the operand without diagonal entries
        t, r, rc = ctx.vec(n), ctx.vec(n), ctx.vec(h.level_shape(1)[0])
        info = h.pack_info(0)
        assert h.group_info(0)["groups"] > 0 and info["pre_source"] == 2 and info["pre_packed"] >= 1, (h.group_info(0), info)
        assert h.pre_pass(0, b, t, r, rc)
        seen = [x.numpy()]

        def check(step, vals, omega, bits):
            xw = h.vcycle(b).numpy()
            assert np.isfinite(xw).all() and not any(np.array_equal(xw, s) for s in seen), step      # every checkpoint has values, ω or precision of its own
            seen.append(xw)
            assert h.operand_precision(0) == bits, step
            A2, h2 = twin_of(ctx, mg, h, rp, ci, vals, omega, bits)
            x2 = h2.vcycle(b).numpy()
            assert h2.operand_precision(0) == bits and h2.group_info(0)["groups"] > 0, step
            print(f"step {step}: walked vs twin max |dx| {np.abs(xw - x2).max():.3e}")
            assert np.array_equal(xw, x2), (step, "twin", float(np.abs(xw - x2).max()))
            ctx.set_option("pack7", 0); ctx.set_option("pre_nodiag", 0)
            x0 = h.vcycle(b).numpy()
            ctx.set_option("pack7", 1); ctx.set_option("pre_nodiag", 1)
            print(f"step {step}: walked vs itself with pack7 = pre_nodiag = 0 max |dx| {np.abs(xw - x0).max():.3e}")
            assert np.array_equal(xw, x0), (step, "options off", float(np.abs(xw - x0).max()))
        check.b, check.x = b, x

        kept = walk(ctx, A, h, rp, ci, v, check)
        print("kept_graphs", kept)
        assert kept == KEPT, kept
        info = h.pack_info(0)
        assert info["pre_source"] == 2 and info["pre_packed"] >= 1 and h.pre_pass(0, b, t, r, rc), info
    finally:
        restore(ctx)


def test_the_walk_leaves_a_twins_bytes_in_use():
    """in a process of its own (the arena is per process): the walked hierarchy and its matrix hold what a fresh twin and its matrix hold, plus
    EXTRA_BYTES — a figure measured on the library as it was before hier_operands.hip, not derived"""
    from conftest import REPO
    code = r'''
import ctypes as C, os, sys, numpy as np
sys.path[:0] = [%r, os.path.join(%r, "tests")]
import multigridsolver_amd as mg
import test_gpu_operand_chain as T
L = mg.lib()
assert L.mgs_arena_reserve(C.c_size_t(256 << 20)) == 0
def used():
    out = (C.c_size_t * 3)(); assert L.mgs_arena_info(out) == 0; return int(out[1])
ctx = mg.Context(0)
n = T.N ** 3
b, x = ctx.vec(n).rand(seed=7), ctx.vec(n)
ctx.sync(); u0 = used()
A, h, rp, ci, v = T.built(ctx, mg)
h.vcycle(b, x)
state = {}
def check(step, vals, omega, bits):
    h.vcycle(b, x); state.update(vals=vals, omega=omega, bits=bits)
check.b, check.x = b, x
T.walk(ctx, A, h, rp, ci, v, check)
ctx.sync(); u1 = used()
A2, h2 = T.twin_of(ctx, mg, h, rp, ci, state["vals"], state["omega"], state["bits"])
h2.vcycle(b, x)
ctx.sync(); u2 = used()
assert np.array_equal(h.vcycle(b).numpy(), h2.vcycle(b).numpy())
print("WALK_BYTES", u1 - u0, u2 - u1)
ctx.close()
''' % (REPO, REPO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0 and "WALK_BYTES" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    walked, twin = (int(w) for w in r.stdout.split("WALK_BYTES")[1].split()[:2])
    print(f"bytes in use: walked {walked}, twin {twin}, difference {walked - twin}")
    assert walked > 0 and twin > 0 and walked == twin + EXTRA_BYTES, (walked, twin)
