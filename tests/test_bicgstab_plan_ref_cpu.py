"""The state machine of mgs_bicgstab_plan (tests/bicgstab_plan_ref.py: scalar steps, frozen / first / half, predicated passes, the host loop
with `ahead`) against the restatement of mgs_bicgstab in the same file: the tuple (status, iterations, resid) and every bit of x
(equal_nan=True), for ahead in {0, 1, 2, 7, 10000}.  The inputs reach every exit; those of the small operators have dyadic
intermediate values (or, for the status-2 operator, a zero that the test first shows the restatement to reach), so no summation order
matters and the same operators serve on the device as block-diagonal copies (tests/test_gpu_bicgstab_plan.py)."""
import numpy as np
import pytest

from bicgstab_plan_ref import BicgstabPlanModel, bicgstab_ref
from krylov_ref import banded

AHEADS = [0, 1, 2, 7, 10000]

I2 = 2.0 * np.eye(2)
A2 = np.array([[-2.0, -2.0], [-2.0, 0.0]])
A3 = np.array([[-2.0, -2.0, -2.0], [-2.0, -2.0, -1.0], [-2.0, -1.0, -2.0]])
A3D = np.array([[-2.0, -2.0, -2.0], [-2.0, -2.0, -2.0], [-2.0, 2.0, 0.0]])


def check(model_run, ref):
    st, it, res, x = model_run
    assert (st, it) == (ref[0], ref[1])
    assert res == ref[2] or (np.isnan(res) and np.isnan(ref[2]))
    assert np.array_equal(x, ref[3], equal_nan=True)


@pytest.fixture(scope="module")
def band():
    B = banded(513)
    b = np.random.default_rng(7).standard_normal(513)
    return B.apply, b


def jacobi(v):
    return 0.6 * v / 5.0


@pytest.mark.parametrize("ahead", AHEADS)
def test_every_exit(ahead):
    # converged at the half step of iteration 1: α = 0.5, s = 0
    b = np.array([3.0, -5.0])
    ref = bicgstab_ref(I2, b, None, 1e-10, 50)
    assert ref[:3] == (0, 1, 0.0) and np.array_equal(ref[3], 0.5 * b)
    m = BicgstabPlanModel(I2)
    check(m.solve(b, 50, 1e-10, ahead), ref)
    assert m.st.alpha == 0.5 and not m.s.any()
    assert m.info[2] == min(50, 1 + min(ahead, 1022)) and m.info[3] == m.info[2] - 1
    # status 3 at iteration 1: α = −0.5, s = (0, −1), t·s = 0; *max_iter untouched
    ref = bicgstab_ref(A2, np.array([1.0, 0.0]), None, 1e-10, 50)
    assert ref[:3] == (3, 50, 1.0) and np.array_equal(ref[3], [-0.5, 0.0])
    m = BicgstabPlanModel(A2)
    check(m.solve(np.array([1.0, 0.0]), 50, 1e-10, ahead), ref)
    assert m.st.alpha == -0.5 and np.array_equal(m.s, [0.0, -1.0]) and m.st.ts == 0.0 and m.st.it == 1
    # r̃·v = 0: α = ∞, every entry NaN from there on, status 1
    ref = bicgstab_ref(A2, np.array([0.0, 1.0]), None, 1e-10, 6)
    assert ref[:2] == (1, 6) and np.isnan(ref[2]) and np.isnan(ref[3]).all()
    m = BicgstabPlanModel(A2)
    check(m.solve(np.array([0.0, 1.0]), 6, 1e-10, ahead), ref)
    assert m.info[2] == 6 and m.info[3] == 0
    m1 = BicgstabPlanModel(A2)
    m1.solve(np.array([0.0, 1.0]), 1, 1e-10, ahead)
    assert m1.st.rtv == 0.0 and np.isinf(m1.st.alpha)
    # status 2 at iteration 2 (the zero ρ depends on rounding: the restatement must reach it first)
    b3 = np.array([2.0, 1.0, 1.0])
    ref = bicgstab_ref(A3, b3, None, 1e-10, 50)
    assert ref[:2] == (2, 50), ref
    assert np.allclose(ref[3], [-0.4, -0.2, -0.2], rtol=1e-15, atol=0) and abs(ref[2] - 0.2 * np.sqrt(2.0)) < 1e-15
    m = BicgstabPlanModel(A3)
    check(m.solve(b3, 50, 1e-10, ahead), ref)
    it2 = m.st.it                      # where the rounded ρ becomes zero: 2 in exact-looking arithmetic, one later with numpy's blocked dot
    assert it2 in (2, 3) and m.st.rho == 0.0
    assert m.info[2] == min(50, it2 + min(ahead, 1022)) and m.info[3] == m.info[2] - it2
    # status 2 at iteration 2 with dyadic values throughout (α = −1/2, ω = 1/2, r = (−1, 0, 0) ⟂ r̃): the zero ρ does not depend on rounding
    bd = np.array([0.0, 1.0, 0.0])
    ref = bicgstab_ref(A3D, bd, None, 1e-10, 50)
    assert ref[:3] == (2, 50, 1.0) and np.array_equal(ref[3], [-0.5, -0.5, 0.5])
    m = BicgstabPlanModel(A3D)
    check(m.solve(bd, 50, 1e-10, ahead), ref)
    assert m.st.it == 2 and m.st.rho == 0.0 and m.st.alpha == -0.5 and m.st.omega == 0.5
    assert m.info[2] == min(50, 2 + min(ahead, 1022)) and m.info[3] == m.info[2] - 2


@pytest.mark.parametrize("ahead", AHEADS)
@pytest.mark.parametrize("pre", [None, jacobi])
def test_contract_cases(band, ahead, pre):
    A, b = band
    n = b.shape[0]
    # full-step convergence
    ref = bicgstab_ref(A, b, pre, 1e-10, 80)
    assert ref[0] == 0 and 5 <= ref[1] <= 60, ref[:3]
    m = BicgstabPlanModel(A, pre)
    check(m.solve(b, 80, 1e-10, ahead), ref)
    assert m.info[2] == min(80, ref[1] + min(ahead, 1022)) and m.info[3] == m.info[2] - ref[1]
    if ahead == 0:
        assert m.info[3] == 0 and m.info[4] == m.info[2] + 1      # nothing speculative: a look per iteration and one at INIT
    if ahead == 10000:
        assert m.info[4] <= 2
    # max_iter in {0, 1, 3}
    for mi in (0, 1, 3):
        ref_m = bicgstab_ref(A, b, pre, 1e-12, mi)
        assert ref_m[:2] == (1, mi)
        m = BicgstabPlanModel(A, pre)
        check(m.solve(b, mi, 1e-12, ahead), ref_m)
        assert m.info[2] == mi and m.info[3] == 0
    # b = 0
    ref0 = bicgstab_ref(A, np.zeros(n), pre, 1e-10, 80)
    assert ref0[:3] == (0, 0, 0.0)
    check(BicgstabPlanModel(A, pre).solve(np.zeros(n), 80, 1e-10, ahead), ref0)
    # an x0 that already solves the system: (0, 0), x untouched
    xs = bicgstab_ref(A, b, pre, 1e-13, 200)[3]
    refs = bicgstab_ref(A, b, pre, 1e-10, 80, x0=xs)
    assert refs[:2] == (0, 0) and np.array_equal(refs[3], xs)
    check(BicgstabPlanModel(A, pre).solve(b, 80, 1e-10, ahead, x0=xs), refs)
    # a random x0; the same model object solves twice (its vectors hold the last solve's values)
    x0 = np.random.default_rng(1).standard_normal(n)
    refx = bicgstab_ref(A, b, pre, 1e-10, 80, x0=x0)
    assert refx[0] == 0
    m = BicgstabPlanModel(A, pre)
    check(m.solve(b, 80, 1e-10, ahead), ref)
    check(m.solve(b, 80, 1e-10, ahead, x0=x0), refx)


@pytest.mark.parametrize("pre", [None, jacobi])
def test_enqueue_model(band, pre):
    A, b = band
    nb = np.sqrt(b @ b)
    ref = bicgstab_ref(A, b, pre, 1e-10, 80)
    count = ref[1]
    m = BicgstabPlanModel(A, pre)
    st, it, tr, rec, x = m.enqueue(b, count + 5, 1e-10)
    t = b - A(x)
    assert tr == np.sqrt(t @ t) / nb                                # the true residual, recomputed
    assert (st, it) == (0 if tr < 1e-10 else 1, count) and rec == ref[2] and np.array_equal(x, ref[3])
    assert m.info[2] == count + 5 and m.info[3] == 5 and m.info[4] == 0
    # fewer iterations than needed: status 1, bicgstab_ref(max_iter)'s x, the true residual
    ref3 = bicgstab_ref(A, b, pre, 1e-10, 3)
    st, it, tr, rec, x = m.enqueue(b, 3, 1e-10)
    assert (st, it) == (1, 3) and rec == ref3[2] and np.array_equal(x, ref3[3]) and m.info[3] == 0
    t = b - A(x)
    assert tr == np.sqrt(t @ t) / nb
    # a second enqueue continues from that x and converges
    st, it2, tr, rec, x = m.enqueue(b, 80, 1e-10, x0=x)
    assert st == 0 and tr < 1e-10 and it2 < 80
    # the exits and the trivial cases
    st, it, tr, rec, x = BicgstabPlanModel(I2).enqueue(np.array([3.0, -5.0]), 4, 1e-10)
    assert (st, it, tr, rec) == (0, 1, 0.0, 0.0) and np.array_equal(x, [1.5, -2.5])
    st, it, tr, rec, x = BicgstabPlanModel(A2).enqueue(np.array([1.0, 0.0]), 4, 1e-10)
    assert (st, it, tr, rec) == (3, 1, 1.0, 1.0) and np.array_equal(x, [-0.5, 0.0])
    st, it, tr, rec, x = BicgstabPlanModel(A2).enqueue(np.array([0.0, 1.0]), 4, 1e-10)
    assert (st, it) == (1, 4) and np.isnan(tr) and np.isnan(x).all()
    st, it, tr, rec, x = BicgstabPlanModel(A3).enqueue(np.array([2.0, 1.0, 1.0]), 6, 1e-10)
    assert st == 2 and it in (2, 3) and abs(tr - 0.2 * np.sqrt(2.0)) < 1e-15
    st, it, tr, rec, x = BicgstabPlanModel(A3D).enqueue(np.array([0.0, 1.0, 0.0]), 6, 1e-10)
    assert (st, it, tr, rec) == (2, 2, 1.0, 1.0) and np.array_equal(x, [-0.5, -0.5, 0.5])
    st, it, tr, rec, x = m.enqueue(b, 7, 1e-10, x0=ref[3])
    assert it == 0 and np.array_equal(x, ref[3]) and m.info[3] == 7
    st, it, tr, rec, x = m.enqueue(np.zeros_like(b), 2, 1e-10)
    assert (st, it, tr) == (0, 0, 0.0)
    # the recursion froze as converged but the true residual is not below tol: status 1 with iters_done < iters
    drift = BicgstabPlanModel(A, pre)
    real_step_final = drift.step_final

    def inflated(iters, tol):                   # FINAL sees a true residual above tol
        drift.red = [(2e-10 * drift.st.normb) ** 2, 0.0]
        real_step_final(iters, tol)
    drift.step_final = inflated
    st, it, tr, rec, x = drift.enqueue(b, 80, 1e-10)
    assert (st, it) == (1, count) and tr >= 1e-10 and rec < 1e-10
