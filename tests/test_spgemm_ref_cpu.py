"""The host restatement of mgs_csr_spgemm's arithmetic (tests/spgemm_ref.py) is itself checked here, without a device: against scipy,
for its sensitivity to the summation order on every fixture the GPU tests compare bit for bit, and against the oracle's Galerkin
product."""
import numpy as np
import pytest
import scipy.sparse as sps

import spgemm_ref as ref

U = 2.0 ** -53


def structural_product(A, B):
    """scipy's A @ B with the explicit zeros kept: the pattern from a product of all-ones matrices (positive terms cannot cancel)"""
    Sa, Sb = ref.to_scipy(A), ref.to_scipy(B)
    Pa, Pb = Sa.copy(), Sb.copy()
    Pa.data = np.ones_like(Pa.data); Pb.data = np.ones_like(Pb.data)
    pat = sps.csr_matrix(Pa @ Pb); pat.sort_indices()
    assert (pat.data > 0).all()
    val = sps.csr_matrix(Sa @ Sb)
    bound = sps.csr_matrix(abs(Sa) @ abs(Sb))
    rows = np.repeat(np.arange(pat.shape[0]), np.diff(pat.indptr))
    dense_v = np.asarray(val[rows, pat.indices]).ravel() if pat.nnz else np.zeros(0)
    dense_b = np.asarray(bound[rows, pat.indices]).ravel() if pat.nnz else np.zeros(0)
    return pat, dense_v, dense_b


FIXTURES = dict(ref.NUMERIC_FIXTURES, zeros=ref.fx_zeros, limit=lambda: ref.fx_limit(ref.MAX_ROW))


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_restatement_agrees_with_scipy(name):
    A, B = FIXTURES[name]()
    m, n, rp, ci, v = ref.spgemm(A, B)
    pat, sv, bound = structural_product(A, B)
    assert (m, n) == pat.shape
    assert np.array_equal(rp, pat.indptr) and np.array_equal(ci, pat.indices)
    err = np.abs(v - sv)
    assert (err <= 4 * U * bound).all(), float((err / np.maximum(bound, 1e-300)).max())


def test_structural_zeros_and_the_lone_negative_zero():
    m, n, rp, ci, v = ref.spgemm(*ref.fx_zeros())
    assert rp.tolist() == [0, 2, 4] and ci.tolist() == [0, 1, 0, 1]
    assert v[0] == 0.0 and not np.signbit(v[0])          # a·b + (−a)·b
    assert v[3] == 0.0 and np.signbit(v[3])              # (−1.0)·0.0 alone


def test_fixture_shapes_hit_the_paths_they_are_meant_for():
    assert ref.row_products(*ref.fx_poisson8()).max() == 49
    A, B = ref.fx_rect()
    ub = ref.row_products(A, B)
    assert len({A[0], A[1], B[1]}) == 3 and ub[3] == 0 and ub[7] == 0 and np.diff(A[2])[7] == 2 and ub.max() <= 64
    ub = ref.row_products(*ref.fx_boundary())
    assert ub.tolist() == [64, 65] and np.diff(ref.spgemm(*ref.fx_boundary())[2])[1] < 64
    A, B = ref.fx_wide()
    rp = ref.spgemm(A, B)[2]
    assert ref.row_products(A, B).tolist() == [4000, 2400, 0] and 2800 <= rp[1] <= 3200
    first = {}                                            # the step in which row 0 first meets each column
    for step in range(5):
        for j in B[3][B[2][step]:B[2][step + 1]]:
            first.setdefault(int(j), step)
    assert set(first.values()) == {0, 1, 2, 3, 4}
    assert np.diff(ref.spgemm(*ref.fx_limit())[2]).tolist() == [ref.MAX_ROW, 0]
    assert np.diff(ref.spgemm(*ref.fx_limit(ref.MAX_ROW + 1))[2])[0] == ref.MAX_ROW + 1
    lens = np.diff(ref.spgemm(*ref.fx_limit_row3())[2])
    assert np.flatnonzero(lens > ref.MAX_ROW).tolist() == [3, 5]


@pytest.mark.parametrize("name", sorted(ref.NUMERIC_FIXTURES))
def test_the_order_of_the_sums_shows_in_the_bits(name):
    """visiting A's entries back to front changes at least one bit — otherwise a bit-for-bit GPU test on this fixture shows nothing"""
    A, B = ref.NUMERIC_FIXTURES[name]()
    fwd, rev = ref.spgemm(A, B), ref.spgemm(A, B, reverse_a=True)
    assert np.array_equal(fwd[2], rev[2]) and np.array_equal(fwd[3], rev[3])
    changed = np.add.reduceat(np.r_[fwd[4].view(np.int64) != rev[4].view(np.int64), False].astype(np.int64), fwd[2][:-1]) * (np.diff(fwd[2]) > 0)
    ub = ref.row_products(A, B)
    assert changed.sum() > 0
    assert (changed[ub > 64] > 0).all(), "every row of the workgroup path shows the order"
    assert not (ub <= 64).any() or ub[ub <= 64].max() < 3 or (changed[ub <= 64] > 0).any(), "the lane path shows the order"


def galerkin_wide():
    """Poisson 2-D n = 20 and the two-entries-per-row P, both with wide random values on their patterns"""
    rng = np.random.default_rng(2020)
    A, P = ref.poisson2d(20), ref.general_P(400, 100)
    return ref.with_values(A, ref.wide(rng, len(A[3]))), ref.with_values(P, ref.wide(rng, len(P[3])))


def test_the_order_shows_in_the_wide_galerkin_fixture():
    A, P = galerkin_wide()
    Pt = ref.csr(ref.to_scipy(P).T)
    T = ref.spgemm(Pt, A)
    assert not np.array_equal(ref.spgemm(T, P)[4].view(np.int64), ref.spgemm(T, P, reverse_a=True)[4].view(np.int64))


def test_general_galerkin_order_equals_the_oracle(orc):
    """(Pᵀ·A)·P restated on the P of test_gpu_parity.py::test_general_P_fallback against the oracle's galerkin"""
    Ao = orc.poisson2d(20)
    n = Ao.shape[0]; nc = n // 4
    P = ref.general_P(n, nc)
    Po = orc.Csr.from_scipy(ref.to_scipy(P))
    A = (n, n, np.asarray(Ao.rowptr, dtype=np.int32), np.asarray(Ao.col, dtype=np.int32), np.asarray(Ao.val, dtype=np.float64))
    m, k, rp, ci, v = ref.galerkin(A, P)
    Aco = Ao.galerkin(Po)
    assert (m, k) == (nc, nc)
    assert np.array_equal(rp, Aco.rowptr) and np.array_equal(ci, Aco.col)
    assert np.linalg.norm(v - Aco.val) <= 1e-14 * np.linalg.norm(Aco.val)
