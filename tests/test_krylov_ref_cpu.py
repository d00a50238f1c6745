"""Pins the yardsticks of tests/test_gpu_krylov_scalars.py (CPU only): the fixed-step restatements of tests/krylov_ref.py agree
across number types, the BiCGSTAB one is the method the oracle runs (oracle_py.bicgstab, itself pinned to the reference's golden
vectors), and the banded operator's slice form and CSR form are the same matrix."""
import numpy as np
import pytest

import krylov_ref as kr

N = 100_003


@pytest.fixture(scope="module")
def ops():
    return {"nonsym": kr.banded(N, seed=11), "spd": kr.banded(N, seed=12, spd=True)}


@pytest.mark.parametrize("solver", ["bicgstab", "pcg", "pcg_flexible", "fgcr"])
def test_float64_run_agrees_with_long_double(ops, solver):
    """the same statements in float64 and in long double: x within 1e-13 relative after 3 steps (one window closure and one open
    window for GCR(2)) — the restatements are well conditioned enough to serve as a 1e-13 yardstick"""
    rng = np.random.default_rng(5)
    b = rng.standard_normal(N); x0 = np.zeros(N)
    A = ops["spd" if solver.startswith("pcg") else "nonsym"]
    run = {"bicgstab": lambda t: kr.bicgstab_fixed(A.apply, b, x0, 3, dtype=t),
           "pcg": lambda t: kr.pcg_fixed(A.apply, b, x0, 3, dtype=t),
           "pcg_flexible": lambda t: kr.pcg_fixed(A.apply, b, x0, 3, flexible=True, dtype=t),
           "fgcr": lambda t: kr.fgcr_fixed(A.apply, b, x0, 3, 2, dtype=t)}[solver]
    x64, r64 = run(np.float64)
    xld, rld = run(np.longdouble)
    assert x64.dtype == np.float64 and xld.dtype == np.longdouble
    d = kr.rel(x64, xld)
    print(f"{solver}: float64 vs long double, n = {N}, 3 steps: x {d:.3e}, resid {float(r64):.6e} vs {float(rld):.6e}")
    assert d <= 1e-13
    assert abs(float(r64) - float(rld)) <= 1e-10 * float(rld)
    assert 0 < float(rld) < 1            # the steps did reduce the residual: not a restatement of nothing


def test_bicgstab_restatement_is_the_oracles_method(orc):
    """oracle_py.bicgstab on poisson10000, stopped after 1..5 iterations, against the float64 restatement: x within 1e-12"""
    A = orc.poisson2d(100)
    n = A.shape[0]
    b = orc.rand_rhs(n)
    for steps in range(1, 6):
        st, it, tol, x = orc.bicgstab(A, b, None, max_iter=steps, tol=1e-300)
        assert st == 1 and it == steps
        xr, resid = kr.bicgstab_fixed(A.spmv, b, np.zeros(n), steps, dtype=np.float64)
        d = kr.rel(xr, x)
        print(f"steps {steps}: restatement vs oracle x {d:.3e}, resid {float(resid):.6e} vs {tol:.6e}")
        assert d <= 1e-12
        assert abs(float(resid) - tol) <= 1e-10 * tol


@pytest.mark.parametrize("n", [1, 2, 3, 299, 300, 301, 513, N])
@pytest.mark.parametrize("spd", [False, True])
def test_csr_form_equals_slice_form(n, spd):
    A = kr.banded(n, seed=3, spd=spd)
    rp, ci, v = A.csr()
    assert rp[0] == 0 and rp[-1] == len(ci) == len(v) and np.all(ci >= 0) and np.all(ci < n)
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert np.all(np.diff(ci)[np.diff(rows) == 0] > 0)             # sorted, no duplicates within a row
    x = np.random.default_rng(n).standard_normal(n)
    for t in (np.float64, np.longdouble):
        a = A.apply(x.astype(t)); c = kr.csr_apply(rp, ci, v, x.astype(t))
        assert a.dtype == t and c.dtype == t
        assert kr.rel(c, a) <= 4 * np.finfo(t).eps                # five terms per row, summed in two orders
    import scipy.sparse as sps
    M = sps.csr_matrix((v, ci, rp), shape=(n, n))
    assert kr.rel(M @ x, A.apply(x)) <= 4 * np.finfo(np.float64).eps
    if spd:
        assert abs(M - M.T).max() == 0.0
    off = abs(M).sum(axis=1).A1 - abs(M.diagonal())
    assert np.all(M.diagonal() > off)                              # strictly row dominant
    if not spd and n > 2 * kr.BAND:
        assert abs(M - M.T).max() > 0.1
