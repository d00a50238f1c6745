"""tests/nullspace_fields_ref.py held against dense linear algebra on enclosed_stokes(4) and enclosed_stokes(6) (256 and 864 rows).  No GPU.

The restatement's x and x* = pinv(K)·Πb both lie in the range of K (zero pressure mean) and both residuals are at most tol·‖Πb‖ (x*'s is
rounding), so ‖x − x*‖ <= 2·tol·‖Πb‖/σ_min⁺(K) with σ_min⁺ the smallest non-zero singular value from the dense SVD.  The same loop without
the projection and without the regularised coarsest solve does not reach tol in 500 iterations, or its coarsest solve raises."""
import numpy as np
import pytest

import nullspace_fields_ref as nf

EPS = np.finfo(np.float64).eps
TOL = 1e-8


@pytest.fixture(scope="module", params=[4, 6])
def system(request):
    N = request.param
    sd = nf.enclosed_stokes(N)
    As, aggs = nf.build_hierarchy(sd["B"], 50)
    sv = np.linalg.svd(sd["K"].toarray(), compute_uv=False)
    sd["sv"] = sv
    sd["As"], sd["aggs"] = As, aggs
    sd["b"] = np.random.default_rng(N).uniform(0.0, 1.0, sd["n"])      # non-zero pressure mean
    return sd


def test_generator_properties(system):
    sd = system
    m, K, D, S = sd["m"], sd["K"], sd["D"], sd["S"]
    assert abs(K - K.T).max() == 0.0
    assert np.abs(np.asarray(D.sum(axis=0))).max() == 0.0                      # every column of D sums to 0
    z = (sd["labels"] == 0).astype(np.float64)
    assert np.abs(K @ z).max() == 0.0 and np.abs(S @ z[3 * m:]).max() <= 16 * EPS * np.abs(S).sum(axis=1).max()
    sv = sd["sv"]
    assert sv[-1] <= sd["n"] * EPS * sv[0] and sv[-2] > 0.1                    # exactly one null vector
    assert np.allclose(S.diagonal(), 1.0) and (np.diff(S.indptr) == 7).all()   # the 7-point periodic Laplacian / 6


def test_projection_and_coarse_labels():
    lab = np.array([-1, 0, 1, 0, -1, 1, 1])
    v = np.arange(7, dtype=np.float64)
    p = nf.project(v, lab)
    assert p[0] == v[0] and p[4] == v[4]
    assert p[[1, 3]].sum() == 0.0 and abs(p[[2, 5, 6]].sum()) <= 4 * EPS * 6
    assert (nf.coarse_labels(lab, np.array([-1, 0, 1, 0, 2, 1, 1]), 3) == [0, 1, -1]).all()
    with pytest.raises(ValueError, match="row 3"):
        nf.coarse_labels(lab, np.array([-1, 0, 1, 1, 2, 1, 1]), 3)              # row 3 (label 0) joins rows of label 1
    with pytest.raises(ValueError, match="row 1"):
        nf.coarse_labels(lab, np.array([-1, -1, 1, 0, 2, 1, 1]), 3)             # a labelled row outside every aggregate


def test_projected_minres_against_pinv(system):
    sd = system
    K, b, lab = sd["K"], sd["b"], sd["labels"]
    cyc = nf.Cycle(sd["As"], sd["aggs"], 0.6, labels=lab)
    assert len(sd["As"]) >= 2
    status, it, resid, x = nf.minres(K, b, lab, cyc.vcycle, tol=TOL, max_iter=500)
    pb = nf.project(b, lab)
    xs = np.linalg.pinv(K.toarray()) @ pb
    smin = sd["sv"][-2]
    dist, bar = np.linalg.norm(x - xs), 2 * TOL * np.linalg.norm(pb) / smin
    true = np.linalg.norm(nf.project(b - K @ x, lab)) / np.linalg.norm(pb)
    print(f"N³ = {sd['m']}: status {status}, {it} iterations, resid {resid:.3e}, true {true:.3e}, ‖x − x*‖ {dist:.3e} (bar {bar:.3e}), σ_min⁺ {smin:.3f}")
    assert status == 0 and resid < TOL and true <= TOL * (1 + 1e-3)
    assert abs(x[lab == 0].mean()) <= sd["m"] * EPS * np.abs(x).max()
    assert dist <= bar


def test_unprojected_loop_fails(system):
    sd = system
    try:
        cyc = nf.Cycle(sd["As"], sd["aggs"], 0.6, labels=None)
        status, it, resid, _ = nf.minres(sd["K"], sd["b"], sd["labels"], cyc.vcycle, tol=TOL, max_iter=500, projected=False)
    except np.linalg.LinAlgError:
        return
    print(f"unprojected: status {status}, {it} iterations, resid {resid:.3e}")
    assert status != 0 and not resid < TOL


def test_projected_pcg_two_components():
    """two disconnected path-graph Laplacians and a regular block between them: one constant per component"""
    import scipy.sparse as sps

    def path(n):
        return sps.diags([-np.ones(n - 1), np.r_[1.0, 2.0 * np.ones(n - 2), 1.0], -np.ones(n - 1)], [-1, 0, 1], format="csr")
    A = sps.block_diag([path(7), sps.diags([3.0 * np.ones(4)], [0]), path(5)], format="csr")
    lab = np.r_[np.zeros(7), -np.ones(4), np.ones(5)].astype(np.int64)
    b = np.random.default_rng(3).standard_normal(16)
    status, it, resid, x = nf.pcg(A, b, lab, None, tol=1e-12, max_iter=100)
    lam = np.linalg.eigvalsh(A.toarray())
    assert status == 0 and abs(lam[1]) <= 16 * EPS * lam[-1] and lam[2] > 0.1
    xs = np.linalg.pinv(A.toarray()) @ nf.project(b, lab)
    assert np.linalg.norm(x - xs) <= 2 * 1e-12 * np.linalg.norm(nf.project(b, lab)) / lam[2]
    assert abs(x[lab == 0].mean()) <= 7 * EPS * np.abs(x).max() and abs(x[lab == 1].mean()) <= 5 * EPS * np.abs(x).max()
