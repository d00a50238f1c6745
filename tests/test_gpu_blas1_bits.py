"""The bits of the BLAS-1 reductions and updates (multigridsolver_amd/csrc/blas1.hip: one workgroup fold, one staged fold, one last stage for
all of them) against the exact host restatement tests/blas1_ref.py, which tests/test_blas1_ref_cpu.py pins.  Equal bits, no tolerance.

    n                 why
    1, 2, 3           below one pair, one pair, pair + tail
    511, 512, 513     one workgroup ± tail
    1 048 579         the 8-byte loop runs more than once per lane; the 16-byte form needs the grown scratch (2049 workgroups)
    2 097 665         4097 / 4098 workgroups: the three-stage fold

Inputs: normal and dynamic range 1e8 (make_inputs of test_gpu_krylov_scalars.py), and a pair of all −0.0.  Every length runs with the
operands as allocated (the 16-byte kernels) and 8 bytes into a longer buffer (the 8-byte kernels); 2 097 665 also with blas1_vec = 0,
blas1_pairs = 0 and 2, post_results = 0.  Checked: mgs_dot, mgs_nrm2, mgs_vec_project_const (mean, every shifted entry, the norm),
mgs_axpby and mgs_axpbypcz in both of their forms (the output holds NaN where the form must not read it)."""
import struct

import numpy as np
import pytest

import blas1_ref as br

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 511, 512, 513, 1_048_579, 2_097_665)
DEFAULTS = {"blas1_vec": 1, "blas1_pairs": 1, "post_results": 1}


def bits(v):
    return struct.pack("<d", float(v))


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def n_cu():
    """compute units of the context's device (what mgs_ctx_create reads): the grid of blas1_pairs = 0"""
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


_INPUTS = {}


def inputs(n, kind):
    """(x, y), made once and left unchanged"""
    if (n, kind) not in _INPUTS:
        if kind == "minus0":
            x, y = np.full(n, -0.0), np.full(n, -0.0)
        else:
            rng = np.random.default_rng(1000 + n + int(kind == "range1e8"))
            x, y = rng.standard_normal(n), rng.standard_normal(n)
            if kind == "range1e8":
                x *= 10.0 ** rng.uniform(-4, 4, n); y *= 10.0 ** rng.uniform(-4, 4, n)
        x.setflags(write=False); y.setflags(write=False)
        _INPUTS[(n, kind)] = (x, y)
    return _INPUTS[(n, kind)]


class Placed:
    """device copies of host arrays: as allocated, or 8 bytes into a longer buffer (off 16-byte alignment)"""

    def __init__(self, mg, ctx, aligned):
        self.mg, self.ctx, self.aligned, self.keep = mg, ctx, aligned, []

    def __call__(self, a):
        if self.aligned:
            return self.ctx.vec(a)
        buf = self.ctx.vec(np.concatenate([[7.0], a, [7.0]]))
        self.keep.append(buf)
        return self.mg.Vec.wrap(self.ctx, buf.ptr + 8, len(a))


def check_all(mg, ctx, n, kind, aligned, launch):
    x, y = inputs(n, kind)
    put = Placed(mg, ctx, aligned)
    kw = dict(launch, aligned=aligned)
    tag = f"n={n} {kind} aligned={aligned} {launch}"
    vx, vy = put(x), put(y)
    assert vx.ptr % 16 == (0 if aligned else 8)
    # mgs_dot, mgs_nrm2
    got, want = vx.dot(vy), br.dot(x, y, **kw)
    assert bits(got) == bits(want), (tag, "dot", got, want)
    got, want = vx.nrm2(), br.nrm2(x, **kw)
    assert bits(got) == bits(want), (tag, "nrm2", got, want)
    # mgs_vec_project_const with the norm, on a copy
    total, m, o, q, nrm = br.project_const(x, **kw)
    vp = put(x)
    gm, gn = vp.project_const(nrm2=True)
    assert bits(gm) == bits(m), (tag, "mean", gm, m)
    assert same(vp.numpy(), o), (tag, "shifted entries")
    assert bits(gn) == bits(nrm), (tag, "norm of the projection", gn, nrm)
    # updates: both forms of each; NaN in the output where the form does not read it
    a, b, c = 1.25, -0.3, 3.0
    for bb in (0.0, b):
        out = put(np.full(n, np.nan) if bb == 0.0 else y)
        out.axpby(a, vx, bb)
        assert same(out.numpy(), br.axpby(a, x, bb, y)), (tag, "axpby", bb)
    for cc in (0.0, c):
        z = x[::-1].copy()
        out = put(np.full(n, np.nan) if cc == 0.0 else z)
        out.axpbypcz(a, vx, b, vy, cc)
        assert same(out.numpy(), br.axpbypcz(a, x, b, y, cc, z)), (tag, "axpbypcz", cc)
    del vx, vy, vp, out


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "off8"])
@pytest.mark.parametrize("kind", ["normal", "range1e8"])
@pytest.mark.parametrize("n", LENGTHS)
def test_bits(mg, ctx, n_cu, n, kind, aligned):
    check_all(mg, ctx, n, kind, aligned, {"n_cu": n_cu})


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "off8"])
def test_bits_all_minus_zero(mg, ctx, n_cu, aligned):
    """every sum starts from +0.0, so the sums are +0.0 and the shifted entries keep −0.0; up to one workgroup ± tail (the fold of a
    workgroup is the same code at every length)"""
    for n in LENGTHS[:6]:
        check_all(mg, ctx, n, "minus0", aligned, {"n_cu": n_cu})


@pytest.mark.parametrize("opt,val", [("blas1_vec", 0), ("blas1_pairs", 0), ("blas1_pairs", 2), ("post_results", 0)])
def test_bits_options(mg, ctx, n_cu, opt, val):
    n = 2_097_665
    launch = {"n_cu": n_cu}
    if opt != "post_results":         # posting or copying back the results does not touch their bits
        launch[opt] = val
    try:
        ctx.set_option(opt, val)
        for kind in ("normal", "range1e8"):
            check_all(mg, ctx, n, kind, True, launch)
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)
