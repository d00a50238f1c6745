"""Pins tests/blas1_ref.py, the host restatement of the BLAS-1 reductions (multigridsolver_amd/csrc/blas1.hip), without a GPU:
its launch arithmetic against figures worked out by hand, its sums against math.fsum within the chain bound that
tests/test_gpu_krylov_scalars.py derives from the kernels, its results at n = 1, 2, 3 against the additions written out, and three
planted wrong orders that must change bits on the fixtures the GPU test uses."""
import math
import struct

import numpy as np
import pytest

import blas1_ref as br

U = 2.0 ** -53
CHAIN_VEC = 37          # test_gpu_krylov_scalars.py: 3 + 6 + 4 + 16 + 8, the longest chain of the 16-byte forms


def chain_scalar(n):
    return math.ceil(n / (4096 * 256)) + 6 + 4 + 16 + 8


def bits(v):
    return struct.pack("<d", float(v))


def make_inputs(n, wide):
    rng = np.random.default_rng(1000 + n + int(wide))
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    if wide:
        x *= 10.0 ** rng.uniform(-4, 4, n); y *= 10.0 ** rng.uniform(-4, 4, n)
    return x, y


def exact_dot(x, y):
    p = x.astype(np.longdouble) * y.astype(np.longdouble)
    hi = p.astype(np.float64)
    lo = (p - hi).astype(np.float64)
    return math.fsum(hi.tolist() + lo.tolist()), float(np.abs(p).sum())


def test_launch_arithmetic():
    # 16-byte grids: one pair per lane; k pairs per lane; the capped grid of 8 workgroups per CU
    assert br.grid_vec(1, 1, 256) == 1 and br.grid_vec(256, 1, 256) == 1 and br.grid_vec(257, 1, 256) == 2
    assert br.grid_vec(1_048_832, 1, 256) == 4097 and br.grid_vec(1_048_832, 2, 256) == 2049
    assert br.grid_vec(1_048_832, 0, 256) == 2048 and br.grid_vec(1_048_832, 0, 304) == 2432 and br.grid_vec(300, 0, 256) == 2
    assert br.grid_vec(0, 1, 256) == 1 and br.grid_vec(0, 0, 256) == 1
    # 8-byte clamp
    assert br.grid_cap(0, 2048) == 1 and br.grid_cap(513, 2048) == 3 and br.grid_cap(1_048_579, 2048) == 2048 and br.grid_cap(1_048_579, 4096) == 4096
    # mgs_dot: n / 2 pairs (the tail rides on lane 0), 16-byte form from two entries on
    assert br.dot_launch(1) == (False, 1) and br.dot_launch(2) == (True, 1) and br.dot_launch(513) == (True, 1) and br.dot_launch(514) == (True, 2)
    assert br.dot_launch(1_048_577) == (True, 2048) and br.dot_launch(1_048_579) == (True, 2049)      # 524 288 pairs, 524 289 pairs
    assert br.dot_launch(2_097_665) == (True, 4097) and br.dot_launch(2_097_665, blas1_pairs=2) == (True, 2049)
    assert br.dot_launch(2_097_665, blas1_vec=0) == (False, 4096) and br.dot_launch(2_097_665, aligned=False) == (False, 4096)
    # the projection: (n + 1) / 2 pairs, 8-byte form clamped to half the slots
    assert br.project_launch(1) == (True, 1) and br.project_launch(513) == (True, 2) and br.project_launch(2_097_665) == (True, 4098)
    assert br.project_launch(2_097_665, aligned=False) == (False, 2048)
    # the middle stage: above 4096 partials, 256 chunks of ceil(nb / 256)
    assert br.mid_chunk(4096) == 0 and br.mid_chunk(4097) == 17 and br.mid_chunk(4098) == 17 and br.mid_chunk(524_288) == 2048


@pytest.mark.parametrize("wide", [False, True], ids=["normal", "range1e8"])
@pytest.mark.parametrize("n", (1, 2, 3, 511, 512, 513, 1_048_579, 2_097_665))
def test_sums_within_the_chain_bound(n, wide):
    x, y = make_inputs(n, wide)
    ref, sabs = exact_dot(x, y)
    for tag, kw, chain in (("16-byte", {}, CHAIN_VEC if n >= 2 else chain_scalar(n)), ("8-byte", {"aligned": False}, chain_scalar(n))):
        err = abs(br.dot(x, y, **kw) - ref)
        print(f"n={n} {tag}: {err / (U * sabs):.2f} u·Σ|xy| (bar {chain + 2})")
        assert err <= (chain + 2) * U * sabs
    ref2, _ = exact_dot(x, x)
    assert abs(br.nrm2(x) - math.sqrt(ref2)) <= ((CHAIN_VEC + 2) / 2 + 2) * U * math.sqrt(ref2)


def test_by_hand_at_1_2_3():
    x, y = np.array([1.1, -2.3, 3.7]), np.array([0.9, 1e-3, -7.1])
    p = [float(np.float64(a) * np.float64(b)) for a, b in zip(x, y)]
    assert bits(br.dot(x[:1], y[:1])) == bits(0.0 + p[0])
    assert bits(br.dot(x[:2], y[:2])) == bits((0.0 + p[0]) + p[1])
    assert bits(br.dot(x, y)) == bits(((0.0 + p[0]) + p[1]) + p[2])                  # lane 0: its pair, then the tail
    assert bits(br.dot(x, y, aligned=False)) == bits(((0.0 + p[0]) + p[2]) + p[1])   # three lanes; shuffle level 2 before level 1
    assert bits(br.dot(x[:2], y[:2], aligned=False)) == bits((0.0 + p[0]) + p[1])
    assert bits(br.nrm2(x[:2])) == bits(math.sqrt(x[0] * x[0] + x[1] * x[1]))
    # the projection at n = 3, 16-byte form: sum on lane 0 (pair, tail); 8-byte form: lanes 0, 1, 2
    v = np.array([0.1, 0.2, 0.4])
    for kw, s in (({}, (0.1 + 0.2) + 0.4), ({"aligned": False}, (0.1 + 0.4) + 0.2)):
        total, m, o, q, nrm = br.project_const(v, **kw)
        assert bits(total) == bits(s) and bits(m) == bits(s / 3.0)
        d = [float(np.float64(e) - np.float64(m)) for e in v]
        assert [bits(e) for e in o] == [bits(e) for e in d]
        sq = [e * e for e in d]
        assert bits(q) == bits((sq[0] + sq[1]) + sq[2] if not kw else (sq[0] + sq[2]) + sq[1])
        assert bits(nrm) == bits(math.sqrt(q))
    # updates: the forms that do not read the output hold even where it is NaN
    nan = np.full(3, np.nan)
    assert [bits(e) for e in br.axpby(2.5, x, 0.0, nan)] == [bits(2.5 * e) for e in x]
    assert [bits(e) for e in br.axpby(2.5, x, -0.5, y)] == [bits(2.5 * a + -0.5 * b) for a, b in zip(x, y)]
    assert [bits(e) for e in br.axpbypcz(2.5, x, -0.5, y, 0.0, nan)] == [bits(2.5 * a + -0.5 * b) for a, b in zip(x, y)]
    assert [bits(e) for e in br.axpbypcz(2.5, x, -0.5, y, 3.0, v)] == [bits((2.5 * a + -0.5 * b) + 3.0 * c) for a, b, c in zip(x, y, v)]


def test_planted_defects_change_bits():
    # 1. the odd tail added first instead of last (lane 0 of workgroup 0).  It reorders three terms of one lane: among a million terms that
    # stays below the result's last bit most of the time, so n = 3 carries this check — x·y on the normal fixture, x·x on both
    x, y = make_inputs(3, False)
    assert bits(br.dot(x, y)) != bits(br.dot(x, y, defect="tail_first"))
    for wide in (False, True):
        x, _ = make_inputs(3, wide)
        assert bits(br.dot(x, x)) != bits(br.dot(x, x, defect="tail_first"))
    x, y = make_inputs(513, True)       # and the lane sums differ wherever there is a tail, seen or not in the result
    assert bits(br.lane_sums(x * y, 1, True)[0, 0]) != bits(br.lane_sums(x * y, 1, True, defect="tail_first")[0, 0])
    # 2. wave sums started from the first wave's sum instead of 0.0: a workgroup whose lanes all hold −0.0 (0.0 + −0.0 = +0.0)
    lanes = np.full((1, br.TB), -0.0)
    assert bits(br.workgroup_fold(lanes)[0]) == bits(0.0)
    assert bits(br.workgroup_fold(lanes, defect="wave_from_first")[0]) == bits(-0.0)
    # 3. the middle stage skipped at 4097 partials: x·y at 2 097 665, both fixtures
    for wide in (False, True):
        x, y = make_inputs(2_097_665, wide)
        assert br.dot_launch(len(x)) == (True, 4097)
        assert bits(br.dot(x, y)) != bits(br.dot(x, y, defect="no_mid"))


def test_all_minus_zero_pair():
    """(−0.0)·(−0.0) = +0.0 and every sum starts from +0.0: the dot is +0.0; the projection's sum is +0.0 too (0.0 + −0.0), so m = +0.0 and
    the shifted entries −0.0 − 0.0 = −0.0 keep their sign"""
    for n in (1, 2, 3, 513):
        z = np.full(n, -0.0)
        assert bits(br.dot(z, z)) == bits(0.0) and bits(br.dot(z, z, aligned=False)) == bits(0.0)
        total, m, o, q, nrm = br.project_const(z)
        assert bits(total) == bits(0.0) and bits(m) == bits(0.0) and all(bits(e) == bits(-0.0) for e in o) and bits(nrm) == bits(0.0)
