"""CPU-only: the numpy model of mgs_minres_plan (tests/minres_plan_ref.py) against the restatement of mgs_minres (tests/minres_ref.py):
status, iterations, reported residual and every bit of x, for every `ahead` — including the ones that enqueue iterations past a refused
true-residual check, whose cycles then rewrite the live z̃ from its unchanged v.

Fixtures: saddle(7) (515 rows, odd) and saddle(5) (188 rows) with the explicit two-P hierarchy of tests/test_gpu_minres.py, ω = 0.6,
V(1,1), the oracle's cycle, b = saddle_rhs.  saddle(7) at tol 1e-6 makes true-residual checks at iterations 37 and 39 (refused) and 40
(confirms), at 1e-10 at 60 (refused) and 61; saddle(5) at 1e-10 makes one check, at 51, which confirms."""
import numpy as np
import pytest

from minres_plan_ref import MinresPlanModel
from minres_ref import exact_block_precond, minres_ref, saddle, saddle_rhs
from test_gpu_minres import Saddle

AHEADS = (0, 1, 2, 7, 10000)


@pytest.fixture(scope="module")
def systems(orc):
    made = {}

    def get(N):
        if N not in made:
            made[N] = Saddle(orc, N)
        return made[N]
    return get


def same(got, want, label):
    assert got[:3] == want[:3], (label, got[:3], want[:3])
    assert np.array_equal(got[3], want[3]), (label, "x differs")


@pytest.mark.parametrize("N,tol,want_checks", [(7, 1e-6, [37, 39, 40]), (7, 1e-10, [60, 61]), (5, 1e-10, [51])])
def test_solve_equals_the_restatement_for_every_ahead(systems, N, tol, want_checks):
    s = systems(N)
    if N == 7:
        assert s.rows == 515 and [P.shape for P in s.Ps] == [(515, 71), (71, 9)]
    else:
        assert s.rows == 188
    checks = []
    want = minres_ref(s.Ko, s.b, s.ho.vcycle, tol=tol, max_iter=500, checks=checks)
    print(f"saddle({N}) tol {tol:g}: restatement {want[:3]}, checks {[(j, f'{e:.2e}', f'{r:.2e}') for j, e, r in checks]}")
    assert want[0] == 0 and [c[0] for c in checks] == want_checks and want[1] == want_checks[-1]
    model = MinresPlanModel(s.Ko, s.ho.vcycle)
    for ahead in AHEADS:
        got = model.solve(s.b, 500, tol, ahead)
        info = list(model.info)
        print(f"  ahead {ahead}: {got[:3]}, info {info}")
        same(got, want, f"saddle({N}) tol {tol:g} ahead {ahead}")
        assert model.checks == checks
        assert info[2] - info[3] == want[1] and info[5] == len(want_checks) - 1
        if ahead == 0:
            assert info[3] == 0
        else:
            # what ran frozen: min(ahead, what is left) past every check
            assert info[3] == sum(min(ahead, 1022, 500 - j) for j in want_checks)
    # a second solve on the same model: the plan's vectors hold the last solve's leftovers
    same(model.solve(s.b, 500, tol, 2), want, "again")


def test_max_iter_cuts(systems):
    s = systems(5)
    model = MinresPlanModel(s.Ko, s.ho.vcycle)
    for max_iter in (0, 3, 51, 52, -1):
        want = minres_ref(s.Ko, s.b, s.ho.vcycle, tol=1e-10, max_iter=max_iter)
        for ahead in (0, 1, 7):
            same(model.solve(s.b, max_iter, 1e-10, ahead), want, f"max_iter {max_iter} ahead {ahead}")
    # no preconditioner, cut at 40: status 1 with the true residual
    want = minres_ref(s.Ko, s.b, None, tol=1e-10, max_iter=40)
    assert want[:2] == (1, 40)
    model = MinresPlanModel(s.Ko, None)
    for ahead in AHEADS:
        same(model.solve(s.b, 40, 1e-10, ahead), want, f"h = None ahead {ahead}")


def test_exits():
    """the 2×2 and status cases of tests/test_minres_ref_cpu.py"""
    tol = 1e-12
    sd = saddle(6)
    K, M, b6 = sd["K"], exact_block_precond(sd), saddle_rhs(sd["n"] + sd["m"])
    cases = [
        ("diag(1, -1)", lambda u: np.array([u[0], -u[1]]), np.array([1.0, 1.0]), None, None, 10, (0, 2)),
        ("antidiagonal", lambda u: np.array([u[1], u[0]]), np.array([1.0, 0.0]), None, None, 10, (0, 2)),
        ("singular", lambda u: np.array([u[0], 0.0]), np.array([0.0, 1.0]), None, None, 10, (3, 1)),
        ("singular, x0", lambda u: np.array([u[0], 0.0]), np.array([0.25, 1.0]), None, np.array([0.25, -0.5]), 10, (3, 1)),
        ("b = 0", lambda u: np.array([u[0], -u[1]]), np.zeros(2), None, None, 10, (0, 0)),
        ("negative definite preconditioner", lambda u: K @ u, b6, lambda u: -u, None, 10, (2, 0)),
        ("max_iter 3", lambda u: K @ u, b6, M, None, 3, (1, 3)),
        ("max_iter 0", lambda u: K @ u, b6, M, None, 0, (1, 0)),
    ]
    for name, A, b, pre, x0, max_iter, st_it in cases:
        want = minres_ref(A, b, pre, tol=tol, max_iter=max_iter, x0=x0)
        assert want[:2] == st_it, (name, want[:3])
        model = MinresPlanModel(A, pre)
        for ahead in AHEADS:
            same(model.solve(b, max_iter, tol, ahead, x0=x0), want, f"{name} ahead {ahead}")
        # enqueue + FINAL: the same exit, the same x; the true residual is the restatement's
        st, it, res, x = model.enqueue(b, max_iter, tol, x0=x0)
        assert (st, it) == want[:2] and res == want[2] and np.array_equal(x, want[3]), (name, st, it, res, want[:3])


def test_enqueue_only(systems):
    s = systems(7)
    tol = 1e-6
    model = MinresPlanModel(s.Ko, s.ho.vcycle)
    # past the first check: the estimate freezes the solve at 37, the true residual does not confirm, nothing recalibrates
    st, it, res, x = model.enqueue(s.b, 45, tol)
    cut = minres_ref(s.Ko, s.b, s.ho.vcycle, tol=1e-300, max_iter=37)
    print(f"enqueue(45): {(st, it, res)}; cut at 37: {cut[:3]}; info {model.info}")
    assert (st, it) == (1, 37) and res == cut[2] and np.array_equal(x, cut[3])
    assert model.info[2] == 45 and model.info[3] == 8 and model.info[4] == 0
    # again from that x: κ is measured afresh
    st2, it2, res2, x2 = model.enqueue(s.b, 45, tol, x0=x)
    true = np.linalg.norm(s.Ko.residual(x2, s.b)) / np.linalg.norm(s.b)
    print(f"again from x: {(st2, it2, res2)}, recomputed {true:.4e}")
    assert st2 == 0 and res2 < tol and abs(res2 - true) <= 1e-10 * true
    # tol = 0 runs exactly `iters` iterations
    st, it, res, x = model.enqueue(s.b, 5, 0.0)
    cut = minres_ref(s.Ko, s.b, s.ho.vcycle, tol=0.0, max_iter=5)
    assert (st, it) == (1, 5) and res == cut[2] and np.array_equal(x, cut[3]) and model.info[3] == 0
