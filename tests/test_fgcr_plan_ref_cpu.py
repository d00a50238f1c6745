"""The state machine of mgs_fgcr_plan (tests/fgcr_plan_ref.py: scalar steps, frozen / why / m_open, predicated passes, the host loop with `ahead`,
the restart from the true residual) against the restatement of mgs_fgcr (tests/fgcr_ref.py): the tuple (status, iterations, resid) and every bit
of x, for ahead in {0, 1, 3, 10000}.  The inputs reach every exit of mgs_fgcr; those of the small operators have dyadic intermediate values, so
no summation order matters and the same operators serve on the device as block-diagonal copies (tests/test_gpu_fgcr_plan.py)."""
import numpy as np
import pytest

from fgcr_plan_ref import FgcrPlanModel, WHY_BREAKDOWN
from fgcr_ref import fgcr_ref
from krylov_ref import banded

AHEADS = [0, 1, 3, 10000]

I2 = 2.0 * np.eye(2)
N2 = np.array([[0.0, 1.0], [0.0, 0.0]])                                   # A·c_0 = 0 for r = (1, 0): breakdown at k = 0
N3 = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]])        # breakdown behind an orthogonalisation


def check(run, ref):
    st, it, res, x = run
    assert (st, it) == (ref[0], ref[1]), (run[:3], ref[:3])
    assert res == ref[2] or (np.isnan(res) and np.isnan(ref[2])), (res, ref[2])
    assert np.array_equal(x, ref[3], equal_nan=True)


def poisson2d(N):
    def apply(v):
        u = v.reshape(N, N)
        out = 4.0 * u
        out[1:, :] -= u[:-1, :]; out[:-1, :] -= u[1:, :]
        out[:, 1:] -= u[:, :-1]; out[:, :-1] -= u[:, 1:]
        return out.reshape(-1)
    return apply


@pytest.fixture(scope="module")
def band():
    B = banded(513)
    b = np.random.default_rng(7).standard_normal(513)
    return B.apply, b


def jacobi(v):
    return 0.6 * v / 5.0


@pytest.mark.parametrize("ahead", AHEADS)
@pytest.mark.parametrize("restart", [2, 3, 10])
def test_every_exit(ahead, restart):
    # converged mid-window at iteration 1: α_0 = t/ρ_0 = 1/2, r = 0; the true residual confirms
    b = np.array([3.0, -5.0])
    ref = fgcr_ref(I2, b, None, restart, 1e-10, 50)
    assert ref[:3] == (0, 1, 0.0) and np.array_equal(ref[3], 0.5 * b)
    m = FgcrPlanModel(I2, None, restart)
    check(m.solve(b, 50, 1e-10, ahead), ref)
    assert m.info[2] == min(50, 1 + min(ahead, 1022)) and m.info[3] == m.info[2] - 1 and m.info[5] == 0
    assert m.x_passes == 1                                                 # the window is applied once, whatever ran on speculation
    # breakdown at k = 0: ρ_0 = 0, status 2 at iteration 1, x = 0, resid 1
    b = np.array([1.0, 0.0])
    ref = fgcr_ref(N2, b, None, restart, 1e-10, 50)
    assert ref[:3] == (2, 1, 1.0) and not ref[3].any()
    m = FgcrPlanModel(N2, None, restart)
    check(m.solve(b, 50, 1e-10, ahead), ref)
    assert m.st.why == WHY_BREAKDOWN and m.st.rho[0] == 0.0 and m.info[3] == m.info[2] - 1
    # breakdown behind an orthogonalisation; with restart = 2 the same answer one iteration later, across one window close
    b = np.array([1.0, 0.0, 1.0])
    ref = fgcr_ref(N3, b, None, restart, 1e-10, 50)
    assert ref[:2] == (2, 3 if restart >= 3 else 4) and ref[2] == 1.0 / np.sqrt(2.0) and np.array_equal(ref[3], [1.0, 1.0, 0.0]), ref
    m = FgcrPlanModel(N3, None, restart)
    check(m.solve(b, 50, 1e-10, ahead), ref)
    assert m.st.why == WHY_BREAKDOWN and m.info[2] == min(50, ref[1] + min(ahead, 1022)) and m.info[3] == m.info[2] - ref[1]


@pytest.mark.parametrize("ahead", AHEADS)
@pytest.mark.parametrize("restart", [1, 3, 10, 16])
@pytest.mark.parametrize("pre", [None, jacobi])
def test_contract_cases(band, ahead, restart, pre):
    A, b = band
    n = b.shape[0]
    ref = fgcr_ref(A, b, pre, restart, 1e-10, 400)
    assert ref[0] == 0 and ref[1] >= 5, ref[:3]
    m = FgcrPlanModel(A, pre, restart)
    check(m.solve(b, 400, 1e-10, ahead), ref)
    if ref[4] == 0:
        assert m.info[2] == min(400, ref[1] + min(ahead, 1022)) and m.info[3] == m.info[2] - ref[1]
    assert m.info[5] == ref[4]
    if ahead == 0:
        assert m.info[3] == 0
    # status 1 mid-window, exactly at a window boundary, just behind one; max_iter = 0
    count12 = fgcr_ref(A, b, pre, restart, 1e-12, 400)[1]
    cases = [mi for mi in sorted({0, 1, 3, restart, restart + 1}) if mi < count12]
    assert {0, 1, 3} <= set(cases) and (restart > 10 or {restart, restart + 1} <= set(cases)), (cases, count12)
    for mi in cases:
        ref_m = fgcr_ref(A, b, pre, restart, 1e-12, mi)
        assert ref_m[:2] == (1, mi)
        m = FgcrPlanModel(A, pre, restart)
        check(m.solve(b, mi, 1e-12, ahead), ref_m)
        assert m.info[2] == mi and m.info[3] == 0
    # b = 0
    ref0 = fgcr_ref(A, np.zeros(n), pre, restart, 1e-10, 80)
    assert ref0[:3] == (0, 0, 0.0)
    check(FgcrPlanModel(A, pre, restart).solve(np.zeros(n), 80, 1e-10, ahead), ref0)
    # an x0 that already solves the system: (0, 0), x untouched
    xs = fgcr_ref(A, b, pre, restart, 1e-13, 2000)[3]
    refs = fgcr_ref(A, b, pre, restart, 1e-10, 80, x0=xs)
    assert refs[:2] == (0, 0) and np.array_equal(refs[3], xs)
    check(FgcrPlanModel(A, pre, restart).solve(b, 80, 1e-10, ahead, x0=xs), refs)
    # a random x0; the same model object solves twice (its vectors and coefficients hold the last solve's values)
    x0 = np.random.default_rng(1).standard_normal(n)
    refx = fgcr_ref(A, b, pre, restart, 1e-10, 400, x0=x0)
    assert refx[0] == 0
    m = FgcrPlanModel(A, pre, restart)
    check(m.solve(b, 400, 1e-10, ahead), ref)
    check(m.solve(b, 400, 1e-10, ahead, x0=x0), refx)


@pytest.mark.parametrize("ahead", [0, 3])
def test_null_space(ahead):
    # a periodic 1-D Laplacian plus a skew part: every row and column sums to zero; declared constant
    n = 16
    def A(v):
        return 2.0 * v - np.roll(v, 1) - np.roll(v, -1) + 0.25 * (np.roll(v, -1) - np.roll(v, 1))
    b = np.random.default_rng(12).standard_normal(n)
    x0 = np.random.default_rng(3).standard_normal(n) + 5.0
    for restart in (3, 10):
        ref = fgcr_ref(A, b, None, restart, 1e-10, 2000, x0=x0, project=True)
        assert ref[0] == 0 and abs(ref[3].mean()) <= 1e-12 * abs(ref[3]).max()
        m = FgcrPlanModel(A, None, restart, project=True)
        check(m.solve(b, 2000, 1e-10, ahead, x0=x0), ref)
        for mi in (0, 2, restart, restart + 1):
            check(FgcrPlanModel(A, None, restart, project=True).solve(b, mi, 1e-12, ahead, x0=x0), fgcr_ref(A, b, None, restart, 1e-12, mi, x0=x0, project=True))


@pytest.mark.parametrize("restart,aheads", [(10, AHEADS), (16, [0, 3]), (3, [0, 3])])
def test_drift_restarts(restart, aheads):
    """2-D Poisson 30², no preconditioner, tol 1e-14: the recursion says converged again and again before the true residual agrees, and the
    method restarts from the true residual each time.  The counts depend on the summation order; what is asserted is that the path runs."""
    A = poisson2d(30)
    b = np.random.default_rng(0).random(900)
    ref = fgcr_ref(A, b, None, restart, 1e-14, 3000)
    print(f"restart {restart}: status {ref[0]}, {ref[1]} iterations, {ref[4]} restarts from the true residual")
    assert ref[0] == 0 and ref[4] >= 1
    for ahead in aheads:
        m = FgcrPlanModel(A, None, restart)
        check(m.solve(b, 3000, 1e-14, ahead), ref)
        assert m.info[5] == ref[4]


@pytest.mark.parametrize("restart", [3, 10])
@pytest.mark.parametrize("pre", [None, jacobi])
def test_enqueue_model(band, restart, pre):
    A, b = band
    nb = np.sqrt(b @ b)
    ref = fgcr_ref(A, b, pre, restart, 1e-10, 400)
    count = ref[1]
    assert ref[4] == 0
    m = FgcrPlanModel(A, pre, restart)
    st, it, tr, rec, x = m.enqueue(b, count + 5, 1e-10)
    t = b - A(x)
    assert tr == np.sqrt(t @ t) / nb                                # the true residual, recomputed
    assert (st, it) == (0, count) and np.array_equal(x, ref[3]) and tr == ref[2]
    assert m.info[2] == count + 5 and m.info[3] == 5 and m.info[4] == 0
    # fewer iterations than needed: status 1, fgcr_ref(max_iter)'s x and residual; mid-window and at a window boundary
    for mi in (3, restart, restart + 1):
        ref3 = fgcr_ref(A, b, pre, restart, 1e-10, mi)
        st, it, tr, rec, x = m.enqueue(b, mi, 1e-10)
        assert (st, it) == (1, mi) and tr == ref3[2] and np.array_equal(x, ref3[3]) and m.info[3] == 0
    # a second enqueue continues from that x and converges
    st, it2, tr, rec, x = m.enqueue(b, 400, 1e-10, x0=x)
    assert st == 0 and tr < 1e-10 and it2 < 400
    # the exits and the trivial cases
    st, it, tr, rec, x = FgcrPlanModel(I2, None, restart).enqueue(np.array([3.0, -5.0]), 4, 1e-10)
    assert (st, it, tr) == (0, 1, 0.0) and np.array_equal(x, [1.5, -2.5])
    st, it, tr, rec, x = FgcrPlanModel(N2, None, restart).enqueue(np.array([1.0, 0.0]), 4, 1e-10)
    assert (st, it, tr) == (2, 1, 1.0) and not x.any()
    st, it, tr, rec, x = FgcrPlanModel(N3, None, restart).enqueue(np.array([1.0, 0.0, 1.0]), 6, 1e-10)
    assert (st, it, tr) == (2, 3, 1.0 / np.sqrt(2.0)) and np.array_equal(x, [1.0, 1.0, 0.0])
    st, it, tr, rec, x = FgcrPlanModel(N3, None, 2).enqueue(np.array([1.0, 0.0, 1.0]), 6, 1e-10)
    assert (st, it, tr) == (2, 4, 1.0 / np.sqrt(2.0)) and np.array_equal(x, [1.0, 1.0, 0.0])
    st, it, tr, rec, x = m.enqueue(b, 7, 1e-10, x0=ref[3])
    assert (st, it) == (0, 0) and np.array_equal(x, ref[3]) and m.info[3] == 7
    st, it, tr, rec, x = m.enqueue(np.zeros_like(b), 2, 1e-10)
    assert (st, it, tr) == (0, 0, 0.0)
    st, it, tr, rec, x = m.enqueue(b, 0, 1e-10)
    assert (st, it) == (1, 0) and not x.any()


def test_enqueue_reports_a_drifted_convergence():
    """no restart from the true residual on the device: a recursion that says converged freezes the solve; the close behind it reports status 1
    with iters_done < iters, and a second enqueue from that x gets there"""
    A = poisson2d(30)
    b = np.random.default_rng(0).random(900)
    ref = fgcr_ref(A, b, None, 10, 1e-14, 3000)
    assert ref[4] >= 1
    m = FgcrPlanModel(A, None, 10)
    st, it, tr, rec, x = m.enqueue(b, 3000, 1e-14)
    assert st == 1 and it < ref[1] and tr >= 1e-14 and m.info[3] == 3000 - it
    assert m.x_passes == 1 + (it - 1) // 10                          # every window once, the frozen one included
    for _ in range(ref[4] + 1):
        if st == 0:
            break
        st, it, tr, rec, x = m.enqueue(b, 3000, 1e-14, x0=x)
    assert st == 0 and tr < 1e-14
