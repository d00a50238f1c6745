"""The single-pass entry points ask the cycle's own predicate (csrc/cycle.hip: level_fuses): mgs_hier_pre_pass_info and mgs_hier_post_pass
accept a level exactly when the cycle would run its fused form there — option fuse, V(1,1), multiplicative — and refuse it together
(MGS_ERR_STATE) otherwise; toggling back restores both the acceptance and the cycle's bits.  33³ Poisson, three levels."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = -6


def code_of(mg, fn):
    try:
        fn()
    except mg.MgsError as e:
        return e.code
    return 0


def test_entry_points_follow_the_cycles_fused_predicate():
    import multigridsolver_amd as mg
    ctx = mg.Context(0)
    try:
        N = 33; n = N ** 3
        h = mg.Hierarchy(ctx.poisson3d(N), 0.6, 1, 1).coarsen(10.0, 2, 8.0, 2500, 32).finalize()
        assert h.nlev >= 3
        b = ctx.vec(np.random.default_rng(33).uniform(-1, 1, n))
        x_fused = h.vcycle(b).numpy()

        def both(level):
            rows, nc = h.level_shape(level)[0], h.level_shape(level + 1)[0]
            v = [ctx.vec(rows) for _ in range(4)]
            pre = code_of(mg, lambda: h.pre_pass_info(level, v[0], v[1], v[2], ctx.vec(nc)))
            post = code_of(mg, lambda: h.post_pass(level, v[0], None, ctx.vec(nc), v[3]))
            assert pre == post, (level, pre, post)
            return pre

        for level in range(h.nlev - 1):
            assert both(level) == 0
            ctx.set_option("fuse", 0)
            assert both(level) == STATE
            ctx.set_option("fuse", 1)
            for nu1, nu2 in ((2, 1), (1, 2), (0, 1)):
                h.set_smoother(0.6, nu1, nu2)
                assert both(level) == STATE, (nu1, nu2)
            h.set_smoother(0.7, 1, 1)          # a new ω alone does not refuse: the operands are rescaled by the call itself
            assert both(level) == 0
            h.set_smoother(0.6, 1, 1)
            h.set_additive(True)
            assert both(level) == STATE
            h.set_additive(False)
            assert both(level) == 0
        assert np.array_equal(h.vcycle(b).numpy(), x_fused)
    finally:
        ctx.set_option("fuse", 1)
        ctx.close()
