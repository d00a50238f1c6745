"""The host restatement of mgs_csr_add / mgs_csr_scale / mgs_csr_diag (tests/csr_algebra_ref.py) is itself checked here, without a
device: against scipy, for the shapes its fixtures are meant to have, and for their sensitivity to the roundings include/mgs.h
specifies — equal bits on the device then pin the order of the operations."""
import math
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sps

import csr_algebra_ref as ref

U = 2.0 ** -53
FIXTURES = dict(ref.VALUE_FIXTURES, special=ref.fx_special)


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def union_pattern(A, B):
    """scipy's pattern of A + B with explicit zeros kept: the sum of all-ones matrices (positive terms cannot cancel)"""
    Pa, Pb = ref.to_scipy(A).copy(), ref.to_scipy(B).copy()
    Pa.data = np.ones_like(Pa.data); Pb.data = np.ones_like(Pb.data)
    pat = sps.csr_matrix(Pa + Pb); pat.sort_indices()
    assert (pat.data > 0).all()
    return pat


def at(S, pat):
    rows = np.repeat(np.arange(pat.shape[0]), np.diff(pat.indptr))
    return np.asarray(sps.csr_matrix(S)[rows, pat.indices]).ravel() if pat.nnz else np.zeros(0)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_restatement_agrees_with_scipy_and_its_pattern_is_the_union(name):
    alpha, A, beta, B = FIXTURES[name]()
    m, n, rp, ci, v = ref.add(alpha, A, beta, B)
    pat = union_pattern(A, B)
    assert (m, n) == pat.shape
    assert np.array_equal(rp, pat.indptr) and np.array_equal(ci, pat.indices)
    Sa, Sb = ref.to_scipy(A), ref.to_scipy(B)
    want = at(alpha * Sa + beta * Sb, pat)
    bound = at(abs(alpha) * abs(Sa) + abs(beta) * abs(Sb), pat)
    err = np.abs(v - want)
    assert (err <= 4 * U * bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    # plain loops over the rows, a dict per row: the same bits as the vectorised restatement
    k = 0
    for i in range(m):
        a = {int(A[3][q]): np.float64(alpha) * A[4][q] for q in range(A[2][i], A[2][i + 1])}
        b = {int(B[3][q]): np.float64(beta) * B[4][q] for q in range(B[2][i], B[2][i + 1])}
        for j in sorted(set(a) | set(b)):
            w = a[j] + b[j] if j in a and j in b else (a[j] if j in a else b[j])
            assert ci[k] == j and bits(v[k]) == bits(w), (i, j)
            k += 1
        assert rp[i + 1] == k


def exact_sum(alpha, a, beta, b):
    """α·a + β·b rounded once"""
    return float(Fraction(float(alpha)) * Fraction(float(a)) + Fraction(float(beta)) * Fraction(float(b)))


@pytest.mark.parametrize("name", sorted(ref.VALUE_FIXTURES))
def test_the_specified_roundings_show_in_the_bits(name):
    """for at least one common entry fl(fl(αa) + fl(βb)) differs from the exactly rounded αa + βb — and, where this Python has math.fma, from
    both ways a compiler could contract the sum — otherwise a bit-for-bit GPU test on this fixture shows nothing"""
    alpha, A, beta, B = ref.VALUE_FIXTURES[name]()
    n = A[1]
    ka, kb = ref.rows_of(A) * n + A[3], ref.rows_of(B) * n + B[3]
    _, ia, ib = np.intersect1d(ka, kb, return_indices=True)
    assert len(ia) > 0
    ia, ib = ia[:200], ib[:200]
    spec = np.float64(alpha) * A[4][ia] + np.float64(beta) * B[4][ib]
    exact = np.array([exact_sum(alpha, a, beta, b) for a, b in zip(A[4][ia], B[4][ib])])
    assert (bits(spec) != bits(exact)).any()
    assert np.abs(spec - exact).max() <= 4 * U * np.abs(exact).max() + 1e-300
    if hasattr(math, "fma"):
        fa = np.array([math.fma(alpha, a, float(np.float64(beta) * b)) for a, b in zip(A[4][ia], B[4][ib])])
        fb = np.array([math.fma(beta, b, float(np.float64(alpha) * a)) for a, b in zip(A[4][ia], B[4][ib])])
        assert (bits(spec) != bits(fa)).any() and (bits(spec) != bits(fb)).any()


def test_scale_agrees_with_scipy_and_shows_its_order():
    A, dl, dr = ref.fx_scale()
    S = ref.to_scipy(A)
    for l, r in ((dl, None), (None, dr), (dl, dr)):
        got = ref.scale(A, l, r)
        want = (sps.diags(l) if l is not None else sps.identity(A[0])) @ S @ (sps.diags(r) if r is not None else sps.identity(A[1]))
        want = sps.csr_matrix(want); want.sort_indices()
        assert np.array_equal(got[2], A[2]) and np.array_equal(got[3], A[3])
        assert np.array_equal(want.indptr, A[2]) and np.array_equal(want.indices, A[3])
        assert (np.abs(got[4] - want.data) <= 4 * U * np.abs(want.data)).all()
    assert (bits(ref.scale(A, dl, dr)[4]) != bits(ref.scale(A, dl, dr, right_first=True)[4])).any()
    # one factor: one rounding, the plain product
    rows = ref.rows_of(A)
    assert np.array_equal(bits(ref.scale(A, dl, None)[4]), bits(dl[rows] * A[4]))
    assert np.array_equal(bits(ref.scale(A, None, dr)[4]), bits(A[4] * dr[A[3]]))
    assert np.array_equal(bits(ref.scale(A)[4]), bits(A[4]))


def test_diag_restatement():
    A = ref.fx_missing_diag()
    d = ref.diag(A)
    D = ref.to_scipy(A).toarray()
    assert d.shape == (4,) and np.array_equal(d, np.diag(D)) and d[1] == 0.0 and d[3] == 0.0 and d[0] != 0.0
    assert not np.signbit(d[[1, 2, 3]]).any()


def test_structural_zeros_and_lone_negative_zeros():
    alpha, A, beta, B = ref.fx_special()
    m, n, rp, ci, v = ref.add(alpha, A, beta, B)
    assert rp.tolist() == [0, 2, 4] and ci.tolist() == [0, 1, 0, 2]
    assert v[0] == 0.0 and not np.signbit(v[0])          # x − x stays an entry
    assert v[1] == 0.0 and np.signbit(v[1])              # a lone −0.0 of A
    assert v[2] == 0.0 and np.signbit(v[2])              # −1 · 0.0, alone in B
    assert v[3] == 0.0 and not np.signbit(v[3])


def chunks_with_common(cols, other):
    hit = np.isin(cols, other)
    return [bool(hit[c:c + 64].any()) for c in range(0, len(cols), 64)]


def test_fixture_shapes_hit_the_paths_they_are_meant_for():
    _, A, _, B = ref.fx_lane()
    info = ref.add_info(A, B)
    assert info["lane_rows"] == 512 and info["wave_rows"] == 0 and info["common_entries"] >= 1024 and (np.diff(B[2]) == 5).all()
    _, A, _, B = ref.fx_rect()
    la, lb = np.diff(A[2]), np.diff(B[2])
    assert (A[0], A[1]) == (37, 53) and la[3] == 0 and lb[3] > 0 and lb[11] == 0 and la[11] > 0 and la[20] == 0 and lb[20] == 0 and la[36] == 0
    _, A, _, B = ref.fx_boundary()
    assert (np.diff(A[2]) + np.diff(B[2])).tolist() == [64, 65]
    assert ref.add_info(A, B) == {"lane_rows": 1, "wave_rows": 1, "max_row_len": 55, "common_entries": 20}
    _, A, _, B = ref.fx_wave()
    la, lb = np.diff(A[2]), np.diff(B[2])
    assert list(zip(la.tolist(), lb.tolist())) == [(150, 131), (100, 100), (90, 90), (70, 40), (60, 50), (3, 2), (0, 0)]
    row = lambda M, i: M[3][M[2][i]:M[2][i + 1]]      # noqa: E731
    assert len(np.intersect1d(row(A, 0), row(B, 0))) == 40
    assert chunks_with_common(row(A, 0), row(B, 0)) == [True] * 3 and chunks_with_common(row(B, 0), row(A, 0)) == [True] * 3
    assert np.array_equal(row(A, 1), row(B, 1))
    assert (row(A, 2) % 2 == 0).all() and (row(B, 2) % 2 == 1).all()
    assert np.intersect1d(row(A, 3), row(B, 3)).tolist() == [5, 990] and row(A, 3)[[0, -1]].tolist() == [5, 990] == row(B, 3)[[0, -1]].tolist()
    assert row(B, 4).max() < row(A, 4).min()
    assert ref.add_info(A, B)["wave_rows"] == 5 and ref.add_info(A, B)["lane_rows"] == 2
    _, A, _, B = ref.fx_long()
    assert (A[0], A[1]) == (3, 20000) and np.diff(A[2])[1] == 5000 and np.diff(B[2])[1] == 4000
    assert ref.add_info(A, B)["max_row_len"] == 8000
    Bc, d = ref.fx_compose()
    assert (Bc[0], Bc[1]) == (40, 25) and (d > 0).all()
