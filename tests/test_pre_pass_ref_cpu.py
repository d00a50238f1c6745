"""The host restatement of the fused pre pass (tests/pre_pass_ref.py) pinned without a GPU, on the operator families of
test_post_pass_ref_cpu.py plus aggregates of 1–9 members:
  (a) its FP64 evaluation stays inside the derived bars of its long-double evaluation, in all three forms (Â in FP64, Â rounded to FP32, the
      gather form on A with wd);
  (b) the bars bite: a dropped smallest term, the neighbouring row's b as the diagonal operand, a member left out of an aggregate and a member
      taken from the neighbouring aggregate are rejected in exactly the rows / aggregates they touch, by a factor > 1e6;
  (c) the order matters: entries visited in reverse change r's bits in at least 10 % of the rows with three or more entries, in every family
      — equal bits with the device is a statement that bites;
  (d) the restatement is Eigen's order: r equals the oracle's Csr.residual(b, b) on the host-built Â, bit for bit;
  (e) it is the cycle's pre pass: chained with the oracle's coarse solve and post_pass_ref.evaluate it reproduces the oracle's V(1,1) cycle."""
import numpy as np
import pytest
import scipy.sparse as sps

import post_pass_ref as R
import pre_pass_ref as Q
from test_post_pass_ref_cpu import families as post_families

OMEGA = 0.6
FORMS = (("hat", False), ("hat", True), ("wd", False))


def families():
    out = list(post_families())
    rng = np.random.default_rng(4048)
    n = 1500
    out.append(("aggregates_1_to_9", R.randomize(R.random_graph(n, 3, rng, True), rng), Q.aggregates_1_to_9(n, rng)))
    out.append(("row_lengths_7_to_64", R.randomize(Q.with_row_lengths(700, (7, 8, 9, 16, 17, 64), rng), rng), Q.aggregates_1_to_9(700, rng)))
    return out


FAMILIES = families()
IDS = [f[0] for f in FAMILIES]


def case(A, agg, seed):
    A = A.tocsr(); A.sort_indices()
    agg = np.asarray(agg, dtype=np.int32)
    return A, agg, int(agg.max()) + 1, R.signed(np.random.default_rng(seed), A.shape[0])


@pytest.mark.parametrize("name,A,agg", FAMILIES, ids=IDS)
def test_fp64_restatement_stays_inside_the_bars(name, A, agg):
    A, agg, nc, b = case(A, agg, 7)
    worst = 0.0
    for form, f32 in FORMS:
        got = Q.evaluate(A, OMEGA, agg, nc, b, np.float64, form, f32)
        ref = Q.evaluate(A, OMEGA, agg, nc, b, np.longdouble, form, f32)
        for what, g, x, br in zip(("t", "r", "rc"), got, ref, Q.bars(A, OMEGA, agg, nc, b, form, f32)):
            q = Q.ratios(g, x, br)
            assert q.max() <= 1.0, (name, form, f32, what, q.max(), int(q.argmax()))
            worst = max(worst, float(q.max()))
    print(f"{name}: largest error/bar {worst:.3f}")


@pytest.mark.parametrize("name,A,agg", FAMILIES, ids=IDS)
def test_the_bars_bite(name, A, agg):
    """one-row and one-aggregate errors: each is rejected wherever it lands and nowhere else"""
    A, agg, nc, b = case(A, agg, 11)
    rng = np.random.default_rng(5)
    ln = np.diff(A.indptr)
    cnt = np.bincount(agg[agg >= 0], minlength=nc)
    for form, f32 in FORMS:
        p, _ = Q._products(A, OMEGA, b, np.float64, form, f32)
        tb, rb, cb = Q.evaluate(A, OMEGA, agg, nc, b, np.longdouble, form, f32)
        bt, br, bc = Q.bars(A, OMEGA, agg, nc, b, form, f32)
        rows = np.sort(rng.choice(np.flatnonzero(ln >= 2), 12, replace=False))
        touched = np.unique(agg[rows][agg[rows] >= 0])

        def held(got, where_rows, where_aggs, what):
            for nm, g, x, bar_, where in (("t", got[0], tb, bt, where_rows), ("r", got[1], rb, br, where_rows), ("rc", got[2], cb, bc, where_aggs)):
                q = Q.ratios(g, x, bar_)
                assert np.array_equal(np.flatnonzero(q > 1.0), where), (name, form, f32, what, nm, np.flatnonzero(q > 1.0), where)
                if len(where):
                    assert q[where].min() > 1e6, (name, form, f32, what, nm, q[where].min())

        # (1) the smallest-magnitude term of a row dropped
        ks = [A.indptr[i] + int(np.argmin(np.abs(p[A.indptr[i]:A.indptr[i + 1]]))) for i in rows]
        held(Q.evaluate(A, OMEGA, agg, nc, b, np.float64, form, f32, skip=ks), rows, touched, "dropped term")
        # (2) the neighbouring row's b as the diagonal operand
        bd = b.copy(); bd[rows] = b[(rows + 1) % len(b)]
        held(Q.evaluate(A, OMEGA, agg, nc, b, np.float64, form, f32, bdiag=bd), rows, touched, "neighbouring b")
        # (3) a member left out of an aggregate, (4) a member taken from the neighbouring aggregate: t and r stay, r_c moves in those aggregates
        t64, r64, _ = Q.evaluate(A, OMEGA, agg, nc, b, np.float64, form, f32)
        big = np.flatnonzero(cnt >= 2)
        aggs = np.sort(rng.choice(big, min(12, len(big)), replace=False))
        none = np.zeros(0, dtype=np.int64)
        g3 = agg.copy()
        for a in aggs:
            g3[np.flatnonzero(agg == a)[-1]] = -1
        held((t64, r64, Q.restrict(r64, g3, nc, np.float64)), none, aggs, "member left out")
        g4 = agg.copy(); moved = []
        for a in aggs:                                                   # the first member of aggregate a + 1 joins a (and leaves a + 1)
            nb = (a + 1) % nc
            g4[np.flatnonzero(agg == nb)[0]] = a
            moved += [a, nb]
        # an aggregate that loses and gains a member still differs; one that only lost its single member reads 0.0
        rc4 = Q.restrict(r64, g4, nc, np.float64)
        changed = np.flatnonzero(rc4 != Q.restrict(r64, agg, nc, np.float64))
        assert set(changed) <= set(moved) and set(aggs) <= set(changed)
        held((t64, r64, rc4), none, changed, "member of the neighbouring aggregate")


@pytest.mark.parametrize("name,A,agg", FAMILIES, ids=IDS)
def test_the_order_matters(name, A, agg):
    A, agg, nc, b = case(A, agg, 13)
    rows3 = np.diff(A.indptr) >= 3
    for form, f32 in FORMS:
        _, r, rc = Q.evaluate(A, OMEGA, agg, nc, b, np.float64, form, f32)
        _, rr, _ = Q.evaluate(A, OMEGA, agg, nc, b, np.float64, form, f32, reverse=True)
        share = float(np.mean(r[rows3] != rr[rows3]))
        rcr = Q.restrict(r, agg, nc, np.float64, reverse=True)
        cnt3 = np.bincount(agg[agg >= 0], minlength=nc) >= 3
        print(f"{name} {form} f32={f32}: reversed entries change r in {100 * share:.0f} % of the rows with >= 3 entries; reversed members change "
              f"r_c in {100 * float(np.mean(rc[cnt3] != rcr[cnt3])) if cnt3.any() else 0:.0f} % of the aggregates with >= 3 members")
        assert share >= 0.10, (name, form, f32, share)
        assert Q.ratios(rr, r.astype(np.longdouble), Q.bars(A, OMEGA, agg, nc, b, form, f32)[1]).max() <= 1.0      # another order, the same bar


@pytest.mark.parametrize("name,A,agg", FAMILIES, ids=IDS)
def test_restatement_is_eigens_order(orc, name, A, agg):
    A, agg, nc, b = case(A, agg, 17)
    _, r, _ = Q.evaluate(A, OMEGA, agg, nc, b, np.float64, "hat")
    assert np.array_equal(r, orc.Csr.from_scipy(Q.hat_matrix(A, OMEGA)).residual(b, b)), name


def test_members_and_numbering_helpers():
    agg = np.array([2, -1, 0, 2, 1, 0, -1, 1, 2], dtype=np.int32)
    cptr, mem = Q.members_of(agg, 3)
    assert cptr.tolist() == [0, 2, 4, 7] and mem.tolist() == [2, 5, 4, 7, 0, 3, 8]
    g = Q.renumber_by_first_member(agg)
    assert g.tolist() == [0, -1, 1, 0, 2, 1, -1, 2, 0]
    first = [int(np.flatnonzero(g == a)[0]) for a in range(3)]
    assert first == sorted(first)
    rng = np.random.default_rng(3)
    big = Q.renumber_by_first_member(Q.aggregates_1_to_9(3000, rng))
    first = np.array([np.flatnonzero(big == a)[0] for a in range(int(big.max()) + 1)])
    assert np.all(np.diff(first) > 0) and set(np.bincount(big[big >= 0]).tolist()) >= set(range(1, 10))


def chain(orc, A, agg, nc, b, omega=OMEGA):
    """exact pre pass → the oracle's coarse solve → host post pass (t-form and (r, b)-form), and the oracle's own cycle"""
    A = A.tocsr(); A.sort_indices()
    ho = orc.Hier(orc.Csr.from_scipy(A), [orc.Csr.from_scipy(R.agg_P(agg, nc))], omega=omega, nu1=1, nu2=1)
    x_ref = ho.vcycle(b)
    d = R.dvec(A, omega)
    out = []
    for form in ("hat", "wd"):
        t, r, rc = Q.evaluate(A, omega, agg, nc, b, np.float64, form)
        ec = orc.Hier(ho.A(1), [], omega=omega, nu1=1, nu2=1).vcycle(rc)          # a one-level hierarchy's cycle is its coarse solve
        for op in (R.operand_mapped(A, agg), R.operand_merged(A, agg)[0]):
            out.append(R.evaluate(op, d, agg, ec, t, None))
            out.append(R.evaluate(op, d, agg, ec, r, b))
    return x_ref, out


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def test_restatement_is_the_cycles_pre_pass(orc, inputs):
    A = orc.Csr.read(inputs["CSky3d10"])
    P = A.agmg(10.0, 2, 8.0).to_scipy().tocsr()
    agg = np.full(P.shape[0], -1, dtype=np.int32)
    rows = np.flatnonzero(np.diff(P.indptr) == 1); agg[rows] = P.indices[P.indptr[rows]]
    b = orc.rand_rhs(A.shape[0])
    x_ref, xs = chain(orc, A.to_scipy(), agg, P.shape[1], b)
    for x in xs:
        print(f"CSky3d10: chain vs oracle cycle {rel(x, x_ref):.3e}")
        assert rel(x, x_ref) <= 1e-13
    rng = np.random.default_rng(9)
    n = 1500
    W = R.random_graph(n, 4, rng, True); W.data = rng.uniform(0.1, 1.1, W.nnz); W = ((W + W.T) * 0.5).tocsr()
    Lp = (sps.diags(np.asarray(W.sum(axis=1)).ravel() + 0.05) - W).tocsr()
    agg = R.random_aggregates(n, rng)
    x_ref, xs = chain(orc, Lp, agg, int(agg.max()) + 1, rng.standard_normal(n))
    for x in xs:
        print(f"graph Laplacian: chain vs oracle cycle {rel(x, x_ref):.3e}")
        assert rel(x, x_ref) <= 1e-13
