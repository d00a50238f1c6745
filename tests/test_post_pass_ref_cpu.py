"""The host restatement of the fused post pass (tests/post_pass_ref.py) pinned without a GPU: its FP64 evaluation stays inside the derived
per-row bar of its long-double evaluation on every operator family the GPU test uses; the bar rejects a dropped term, an e_c of the
neighbouring aggregate and a d of the neighbouring row in every row they touch; and the restatement IS the cycle's post pass — chained with
the host pre pass and the oracle's coarse solve it reproduces the oracle's V(1,1) cycle."""
import numpy as np
import pytest
import scipy.sparse as sps

import post_pass_ref as R


def families():
    """(name, operator, aggregates): the shapes of tests/test_gpu_post_pass.py at sizes a CPU test affords"""
    rng = np.random.default_rng(2024)
    out = []
    for n in (255, 256, 257, 513):
        out.append((f"line_{n}", R.randomize(R.stencil_1d2d(n), rng), R.pairs(n)))
    out.append(("five_point_513", R.randomize(R.stencil_5pt(513), rng), R.pairs(513)))
    out.append(("27_point_513", R.randomize(R.stencil_27pt(513), rng), R.pairs(513)))
    out.append(("unaggregated_rows",) + R.unaggregated_case(1100, rng))     # rows and columns outside every aggregate, a run of 300 among them
    for sym in (True, False):
        n = 2000 + 500 * sym
        out.append((f"graph_sym{int(sym)}", R.randomize(R.random_graph(n, 4, rng, sym), rng), R.random_aggregates(n, rng)))
    n = 1200                                         # long rows: a band plus two dense rows and columns, aggregates of three
    B = R.stencil_5pt(n).tolil()
    for q in (3, 700):
        js = rng.choice(n, 400, replace=False); B[q, js] = 1.0; B[js, q] = 1.0
    out.append(("long_rows", R.randomize(B.tocsr(), rng), (np.arange(n) // 3).astype(np.int32)))
    out.append(("quantized", R.randomize(R.stencil_5pt(600), rng, quantum=2.0 ** -10), R.pairs(600)))
    return out


FAMILIES = families()


@pytest.mark.parametrize("name,A,agg", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_fp64_restatement_stays_inside_the_bar(name, A, agg):
    c = R.Case(A, agg, seed=7)
    S_unmerged = R.abs_sums(c.mapped, c.ec)
    worst = 0.0
    for kind in ("mapped", "merged", "merged32"):
        op = c.operand(kind)
        for form, bvec, xin in c.forms():
            xa = R.evaluate(op, c.d, c.agg, c.ec, bvec, xin, np.float64)
            xb = R.evaluate(op, c.d, c.agg, c.ec, bvec, xin, np.longdouble)
            q = R.ratios(xa, xb, R.bar(op, c.d, c.agg, c.ec, bvec, xin))
            assert q.max() <= 1.0, (name, kind, form, q.max(), int(q.argmax()))
            worst = max(worst, q.max())
            if kind == "merged":       # held to the exact sum over the unmerged operand: the merged values carry their own roundings
                xu = R.evaluate(c.mapped, c.d, c.agg, c.ec, bvec, xin, np.longdouble)
                bu = R.bar(c.mapped, c.d, c.agg, c.ec, bvec, xin, extra=c.longest_run, S=S_unmerged)
                qu = R.ratios(xa, xu, bu)
                assert qu.max() <= 1.0, (name, form, "merged vs unmerged", qu.max())
    print(f"{name}: largest error/bar {worst:.3f}")
    if name == "quantized":            # every A·P sum is exact: the merged operand, rounded to float or not, does not depend on the order
        v = c.merged.val
        assert np.array_equal(v, np.round(v * 1024) / 1024)
        Pm = R.agg_P(c.agg, c.nc)
        AP = (c.A @ Pm).tocsr(); AP.sort_indices()
        assert np.array_equal(AP.indptr, c.merged.rowptr) and np.array_equal(AP.indices, c.merged.col) and np.array_equal(AP.data, v)


def test_merged_operand_is_A_times_P():
    """pattern and (to rounding) values of the merged operand against scipy's product, rows with dropped columns and empty rows included"""
    _, A, agg = FAMILIES[6]
    c = R.Case(A, agg)
    AP = (c.A @ R.agg_P(c.agg, c.nc)).tocsr(); AP.sort_indices()
    assert np.array_equal(AP.indptr, c.merged.rowptr) and np.array_equal(AP.indices, c.merged.col)
    assert np.max(np.abs(AP.data - c.merged.val)) <= 4 * R.U * np.abs(c.A.data).max() * c.longest_run
    assert (c.merged.len == 0).sum() >= 300 and (c.mapped.col < 0).sum() > 300 and c.merged.block_nnz()[3] == 0


@pytest.mark.parametrize("name,A,agg", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_the_bar_bites(name, A, agg):
    """one-row, one-term errors: each is rejected in every row it touches, and no other row moves"""
    c = R.Case(A, agg, seed=11)
    rng = np.random.default_rng(5)
    for kind in ("mapped", "merged"):
        op = c.operand(kind)
        live = np.flatnonzero((np.bincount(np.repeat(np.arange(op.n), op.len), weights=(op.col >= 0), minlength=op.n) >= 2) & (c.agg >= 0))
        rows = rng.choice(live, 12, replace=False)
        for form, bvec, xin in c.forms():
            xb = R.evaluate(op, c.d, c.agg, c.ec, bvec, xin, np.longdouble)
            br = R.bar(op, c.d, c.agg, c.ec, bvec, xin)
            # (1) the smallest-magnitude term of a row dropped
            ks = []
            for i in rows:
                k = np.arange(op.rowptr[i], op.rowptr[i + 1]); k = k[op.col[k] >= 0]
                ks.append(k[np.argmin(np.abs(op.val[k] * c.ec[op.col[k]]))])
            x1 = R.evaluate(op, c.d, c.agg, c.ec, bvec, xin, np.float64, s=R.row_sums(op, c.ec, np.float64, skip=ks))
            # (2) e_c of the neighbouring aggregate as the row's own
            pe = R.pe_of(c.agg, c.ec); pe[rows] = c.ec[(c.agg[rows] + 1) % c.nc]
            x2 = R.evaluate(op, c.d, c.agg, c.ec, bvec, xin, np.float64, pe=pe)
            # (3) d of the neighbouring row
            d3 = c.d.copy(); d3[rows] = c.d[(rows + 1) % c.n]
            x3 = R.evaluate(op, d3, c.agg, c.ec, bvec, xin, np.float64)
            for what, xm in (("dropped term", x1), ("neighbouring e_c", x2), ("neighbouring d", x3)):
                q = R.ratios(xm, xb, br)
                bad = np.flatnonzero(q > 1.0)
                assert np.array_equal(bad, np.sort(rows)), (name, kind, form, what, bad, np.sort(rows))
                assert q[rows].min() > 1e6, (name, kind, form, what, q[rows].min())


def chain(orc, A, agg, nc, b, omega=0.6):
    """host pre pass → the oracle's coarse solve → host post pass (t-form and (r, b)-form), and the oracle's own cycle"""
    A = A.tocsr(); A.sort_indices()
    Ao = orc.Csr.from_scipy(A); Po = orc.Csr.from_scipy(R.agg_P(agg, nc))
    ho = orc.Hier(Ao, [Po], omega=omega, nu1=1, nu2=1)
    x_ref = ho.vcycle(b)
    d = R.dvec(A, omega)
    t, r, rc = R.pre_pass_host(A, d, agg, nc, b)
    ec = orc.Hier(ho.A(1), [], omega=omega, nu1=1, nu2=1).vcycle(rc)          # a one-level hierarchy's cycle is its coarse solve
    out = []
    for op in (R.operand_mapped(A, agg), R.operand_merged(A, agg)[0]):
        out.append(R.evaluate(op, d, agg, ec, t, None))
        out.append(R.evaluate(op, d, agg, ec, r, b))
    return x_ref, out


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def test_restatement_is_the_cycles_post_pass(orc, inputs):
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
    L = (sps.diags(np.asarray(W.sum(axis=1)).ravel() + 0.05) - W).tocsr()
    agg = R.random_aggregates(n, rng)
    x_ref, xs = chain(orc, L, agg, int(agg.max()) + 1, rng.standard_normal(n))
    for x in xs:
        print(f"graph Laplacian: chain vs oracle cycle {rel(x, x_ref):.3e}")
        assert rel(x, x_ref) <= 1e-13
