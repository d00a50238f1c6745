"""The state machine of mgs_pcg_plan (tests/pcg_plan_ref.py: scalar steps, frozen / first / pending, predicated passes, the host loop with
`ahead`) against the restatement of mgs_pcg (tests/pcg_ref.py): status, iterations, reported residual and every bit of x, for ahead in
{0, 1, 3, 10⁹}.  The inputs reach every branch: 2-D Poisson 30² at tol 1e-14 converges only after restarts from the true residual, at
1e-15 it runs out of iterations with many of them; the negated operator stops at p·A·p, a negative definite preconditioner at r·z."""
import numpy as np
import pytest

from pcg_plan_ref import PcgPlanModel
from pcg_ref import pcg_ref

AHEADS = [0, 1, 3, 10 ** 9]


@pytest.fixture(scope="module")
def prob(orc):
    A = orc.poisson2d(30)
    return A, orc.rand_rhs(A.shape[0])


def jacobi(v):
    return 0.6 * v / 4.0


PRECONDS = {"none": None, "jacobi": jacobi}


def restarts_of_ref(A, b, precond, tol, max_iter, flexible=False):
    """pcg_ref's restart count, by running it with a counting operator: a true residual is the only SpMV beyond one per iteration and the first"""
    calls = [0]

    def spmv(v):
        calls[0] += 1
        return A.spmv(v)
    st, it, res, x = pcg_ref(spmv, b, precond, tol=tol, max_iter=max_iter, flexible=flexible)
    return (st, it, res, x), calls[0] - 1 - it - (1 if st == 0 and it > 0 else 0)


def check(model_run, ref):
    st, it, res, x = model_run
    assert (st, it) == (ref[0], ref[1])
    assert res == ref[2]
    assert np.array_equal(x, ref[3])


@pytest.mark.parametrize("ahead", AHEADS)
@pytest.mark.parametrize("pname", ["none", "jacobi"])
@pytest.mark.parametrize("flexible", [False, True])
def test_restart_inputs(prob, pname, ahead, flexible):
    A, b = prob
    pre = PRECONDS[pname]
    ref14, nre14 = restarts_of_ref(A, b, pre, 1e-14, 400, flexible)
    ref15, nre15 = restarts_of_ref(A, b, pre, 1e-15, 400, flexible)
    print(f"{pname} flexible {int(flexible)}: tol 1e-14 {ref14[:3]} with {nre14} restarts; tol 1e-15 {ref15[:3]} with {nre15} restarts")
    assert ref14[0] == 0 and nre14 >= 1          # status 0 after restarts
    assert ref15[0] == 1 and nre15 >= 10         # status 1 with many
    for tol, ref, nre in ((1e-14, ref14, nre14), (1e-15, ref15, nre15)):
        m = PcgPlanModel(A, pre, flexible)
        check(m.solve(b, 400, tol, ahead), ref)
        assert m.info[5] == nre
        if ahead == 0:
            assert m.info[3] == 0 and m.info[4] == m.info[2] + 1      # nothing speculative: a look per iteration and one at INIT
        if ahead == 10 ** 9:
            assert m.info[4] <= nre + 2


@pytest.mark.parametrize("ahead", AHEADS)
@pytest.mark.parametrize("flexible", [False, True])
def test_contract_cases(prob, ahead, flexible):
    A, b = prob
    n = b.shape[0]

    def neg(v):
        return -A.spmv(v)
    # the negated operator: (3, 1), x untouched
    ref = pcg_ref(neg, b, None, tol=1e-8, max_iter=50, flexible=flexible)
    assert ref[:2] == (3, 1)
    check(PcgPlanModel(neg, None, flexible).solve(b, 50, 1e-8, ahead), ref)
    assert np.array_equal(ref[3], np.zeros(n))
    # a negative definite preconditioner: (2, 1)
    ref = pcg_ref(A, b, lambda v: -jacobi(v), tol=1e-8, max_iter=50, flexible=flexible)
    assert ref[:2] == (2, 1)
    check(PcgPlanModel(A, lambda v: -jacobi(v), flexible).solve(b, 50, 1e-8, ahead), ref)
    # status 2 in a later iteration, with an update pending: a preconditioner that turns negative at its third application
    calls = [0]

    def turning(v):
        calls[0] += 1
        return jacobi(v) if calls[0] < 3 else -jacobi(v)
    ref = pcg_ref(A, b, turning, tol=1e-8, max_iter=50, flexible=flexible)
    assert ref[:2] == (2, 3)
    calls[0] = 0
    check(PcgPlanModel(A, turning, flexible).solve(b, 50, 1e-8, min(ahead, 0)), ref)      # (a stateful preconditioner: nothing speculative)
    # max_iter = 3
    ref = pcg_ref(A, b, jacobi, tol=1e-12, max_iter=3, flexible=flexible)
    assert ref[:2] == (1, 3)
    m = PcgPlanModel(A, jacobi, flexible)
    check(m.solve(b, 3, 1e-12, ahead), ref)
    assert m.info[2] == 3
    # max_iter = 0
    ref = pcg_ref(A, b, jacobi, tol=1e-12, max_iter=0, flexible=flexible)
    check(PcgPlanModel(A, jacobi, flexible).solve(b, 0, 1e-12, ahead), ref)
    # a converged x0: (0, 0)
    xs = pcg_ref(A, b, jacobi, tol=1e-10, max_iter=400)[3]
    ref = pcg_ref(A, b, jacobi, tol=1e-10, max_iter=400, flexible=flexible, x0=xs)
    assert ref[:2] == (0, 0)
    check(PcgPlanModel(A, jacobi, flexible).solve(b, 400, 1e-10, ahead, x0=xs), ref)
    # b = 0
    ref = pcg_ref(A, np.zeros(n), jacobi, tol=1e-10, max_iter=400, flexible=flexible)
    assert ref[:3] == (0, 0, 0.0)
    check(PcgPlanModel(A, jacobi, flexible).solve(np.zeros(n), 400, 1e-10, ahead), ref)
    # an ordinary solve from a random x0, and how many iterations ran frozen
    x0 = np.random.default_rng(1).standard_normal(n)
    ref = pcg_ref(A, b, jacobi, tol=1e-10, max_iter=400, flexible=flexible, x0=x0)
    assert ref[0] == 0
    m = PcgPlanModel(A, jacobi, flexible)
    check(m.solve(b, 400, 1e-10, ahead, x0=x0), ref)
    assert m.info[2] == min(400, ref[1] + min(ahead, 1022)) and m.info[3] == m.info[2] - ref[1]


@pytest.mark.parametrize("flexible", [False, True])
def test_enqueue_model(prob, flexible):
    A, b = prob
    ref = pcg_ref(A, b, jacobi, tol=1e-10, max_iter=400, flexible=flexible)
    count = ref[1]
    assert ref[0] == 0
    m = PcgPlanModel(A, jacobi, flexible)
    st, it, tr, x = m.enqueue(b, count + 5, 1e-10)
    assert (st, it) == (0, count) and tr == ref[2] and np.array_equal(x, ref[3])
    assert m.info[2] == count + 5 and m.info[3] == 5 and m.info[4] == 0
    # fewer iterations than needed: status 1, pcg_ref(max_iter)'s x, the true residual
    ref3 = pcg_ref(A, b, jacobi, tol=1e-10, max_iter=3, flexible=flexible)
    st, it, tr, x = m.enqueue(b, 3, 1e-10)
    assert (st, it) == (1, 3) and np.array_equal(x, ref3[3]) and m.info[3] == 0
    assert tr == np.linalg.norm(b - A.spmv(x)) / np.linalg.norm(b)
    # the breakdowns and the trivial cases
    st, it, tr, x = PcgPlanModel(lambda v: -A.spmv(v), None, flexible).enqueue(b, 4, 1e-8)
    assert (st, it) == (3, 1) and np.array_equal(x, np.zeros_like(b))
    st, it, tr, x = PcgPlanModel(A, lambda v: -jacobi(v), flexible).enqueue(b, 4, 1e-8)
    assert (st, it) == (2, 1)
    st, it, tr, x = m.enqueue(b, 7, 1e-10, x0=ref[3])
    assert (st, it) == (0, 0) and np.array_equal(x, ref[3]) and m.info[3] == 7
    st, it, tr, x = m.enqueue(np.zeros_like(b), 2, 1e-10)
    assert (st, it, tr) == (0, 0, 0.0)
    # the recursion froze as converged but the true residual is not below tol: status 1 with iters_done < iters; enqueueing again from that x
    # starts from the true residual, which is what mgs_pcg's restart does
    ref14 = pcg_ref(A, b, None, tol=1e-14, max_iter=400, flexible=flexible)
    m = PcgPlanModel(A, None, flexible)
    st, it, tr, x = m.enqueue(b, 400, 1e-14)
    assert st == 1 and it < ref14[1] and tr >= 1e-14
    total = it
    for _ in range(20):
        if st == 0:
            break
        st, it, tr, x = m.enqueue(b, 400, 1e-14, x0=x)
        total += it
    assert st == 0 and tr < 1e-14
    print(f"flexible {int(flexible)}: enqueue rounds reach 1e-14 after {total} iterations, pcg_ref after {ref14[1]}")
