"""The coarsest-level dense solve on its own: a hierarchy with ONE level (no coarsen, no push_P) applies exactly inv·b, the explicit inverse
built by Gauss-Jordan elimination with partial pivoting (kernels_aux.hip: gj_*_kernel, dense_gemv_kernel).  Every operator the rest of the
suite feeds it is a diagonally dominant M-matrix, on which the pivot search always picks the diagonal; here the row swaps run, the
singularity rule of mgs_hier_finalize (include/mgs.h: a pivot not greater than 8·n·DBL_EPSILON·max|a_ij|, NaN, Inf) is checked from both
sides, and the same refusals are checked through mgs_hier_refresh.

Reference: numpy.linalg.solve followed by two steps of iterative refinement with long-double residuals.
Bars: rel(x, x_ref) <= n·2^-52·cond_2(A) (cond_2 from numpy.linalg.cond) and ‖A·x − b‖/(‖A‖·‖x‖) <= n·2^-52.
Every test prints the distances it measured."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
NUMERIC, STATE = -5, -6


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


def upload(ctx, A, sparse=False):
    """dense operators as full rows (explicit zeros included); sparse=True: only the non-zero entries"""
    n = A.shape[0]
    if sparse:
        import scipy.sparse as sps
        M = sps.csr_matrix(A); M.sort_indices()
        return ctx.csr(n, n, M.indptr, M.indices, M.data)
    return ctx.csr(n, n, np.arange(0, n * n + 1, n), np.tile(np.arange(n), n), np.ascontiguousarray(A).ravel())


def dense_solve(ctx, mg, A, b, sparse=False):
    Ad = upload(ctx, A, sparse)
    h = mg.Hierarchy(Ad, 0.5, 1, 1).finalize()
    assert h.nlev == 1
    return h.vcycle(ctx.vec(b)).numpy()


def refined_solve(A, b):
    x = np.linalg.solve(A, b).astype(np.longdouble)
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    for _ in range(2):
        r = bl - Al @ x
        x = x + np.linalg.solve(A, r.astype(np.float64))
    return x


def check(tag, A, b, x):
    n = A.shape[0]
    xr = refined_solve(A, b)
    cond = np.linalg.cond(A)
    xl = x.astype(np.longdouble)
    d = float(np.sqrt(((xl - xr) ** 2).sum()) / np.sqrt((xr ** 2).sum()))
    res = float(np.sqrt(((A.astype(np.longdouble) @ xl - b) ** 2).sum())) / (np.linalg.norm(A, 2) * np.linalg.norm(x))
    print(f"{tag}: n = {n}, cond {cond:.3e}: x vs refined reference {d:.3e} (bar {n * EPS * cond:.3e}, {d / (n * EPS * cond):.1e} of it); "
          f"residual {res:.3e} (bar {n * EPS:.3e})")
    assert np.isfinite(x).all()
    assert d <= n * EPS * cond, (tag, d, n * EPS * cond)
    assert res <= n * EPS, (tag, res, n * EPS)


def orth_family(n, lo_exp, seed):
    """Q1·diag(logspace(0, lo_exp, n))·Q2 with Haar-ish orthogonal factors: prescribed singular values, no structure a pivot search could use"""
    rng = np.random.default_rng(seed)
    Q1 = np.linalg.qr(rng.standard_normal((n, n)))[0]
    Q2 = np.linalg.qr(rng.standard_normal((n, n)))[0]
    return (Q1 * np.logspace(0, lo_exp, n)) @ Q2


def laplacian(n, seed, row_scaled):
    """singular weighted graph Laplacian (rows sum to zero, non-integer weights) of a ring plus random chords; row_scaled: D·L, nonsymmetric"""
    rng = np.random.default_rng(seed)
    W = np.zeros((n, n))
    i = np.arange(n)
    W[i, (i + 1) % n] = rng.uniform(0.3, 1.7, n)                       # the ring keeps the graph connected: rank n − 1
    extra = rng.integers(0, n, (3 * n, 2))
    W[extra[:, 0], extra[:, 1]] = rng.uniform(0.3, 1.7, len(extra))
    W = np.triu(W, 1) + np.triu(W.T, 1)                                # every edge once, above the diagonal ...
    W = W + W.T                                                        # ... then mirrored
    L = np.diag(W.sum(axis=1)) - W
    if row_scaled:
        L = rng.uniform(0.2, 5.0, n)[:, None] * L
    return L


# ------------------------------------------------------------------------------------------------------------------- it solves
@pytest.mark.parametrize("n", [2, 63, 64, 65, 255, 256, 257, 1000])
def test_orthogonal_factor_family_cond_1e3(ctx, mg, n):
    """cond 1e3; almost every elimination step swaps rows (61 of 65, 252 of 257, 993 of 1000 on these matrices in a NumPy model of the
    algorithm, which reaches 6e-4 .. 1.3e-2 of the bar on x and 1e-2 .. 2e-2 of the bar on the residual)"""
    A = orth_family(n, 3, seed=n)
    b = np.random.default_rng(n + 1).standard_normal(n)
    check(f"orthogonal factors n={n}", A, b, dense_solve(ctx, mg, A, b))


def test_ill_conditioned_but_regular_is_accepted(ctx, mg):
    """cond 1e10 at n = 64: far from the singularity rule (such matrices keep every pivot above 5.9e5·n·eps·max|a| in the model), must
    finalize and meet the same bars"""
    A = orth_family(64, -10, seed=99)
    b = np.random.default_rng(98).standard_normal(64)
    check("cond 1e10 n=64", A, b, dense_solve(ctx, mg, A, b))


@pytest.mark.parametrize("order", ["K_first", "zero_first"])
def test_saddle_point_zero_diagonal_block(ctx, mg, order):
    """[[K, Bᵀ], [B, 0]], n = 120 + 40, cond about 5; the zero diagonal block is uploaded without entries (40 rows have no diagonal at
    all).  With K first, elimination fills the zero block before it is reached; zero_first is the same system with the two block rows and
    columns exchanged, [[0, B], [Bᵀ, K]], where the first 40 steps find a zero on the diagonal and must swap"""
    rng = np.random.default_rng(21)
    Q = np.linalg.qr(rng.standard_normal((120, 120)))[0]
    K = (Q * rng.uniform(1.0, 2.0, 120)) @ Q.T
    K = 0.5 * (K + K.T)
    B = np.linalg.qr(rng.standard_normal((120, 40)))[0].T
    Z = np.zeros((40, 40))
    A = np.block([[K, B.T], [B, Z]]) if order == "K_first" else np.block([[Z, B], [B.T, K]])
    b = rng.standard_normal(160)
    check(f"saddle point 120+40 {order}", A, b, dense_solve(ctx, mg, A, b, sparse=True))


def cyclic_shift_case(ctx, mg, n, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    b = rng.standard_normal(n)
    i = np.arange(n)
    # row i holds d_i in column i+1 (mod n): A = roll(eye, 1)·d, every diagonal entry is missing, every elimination step swaps
    Ad = ctx.csr(n, n, np.arange(n + 1), (i + 1) % n, d)
    t0 = time.perf_counter()
    h = mg.Hierarchy(Ad, 0.5, 1, 1).finalize()
    x = h.vcycle(ctx.vec(b)).numpy()
    dt = time.perf_counter() - t0
    want = np.empty(n); want[(i + 1) % n] = b / d                      # x_{i+1} = b_i / d_i
    ulps = np.abs(x - want) / np.spacing(np.abs(want))
    print(f"scaled cyclic shift n={n}: finalize + solve {dt:.2f} s, worst entry {ulps.max():.2f} ulp from the closed form")
    assert ulps.max() <= 2.0                                           # inv holds fl(1/d_i), the product with b_i rounds once more
    return dt


def test_scaled_cyclic_shift_closed_form(ctx, mg):
    cyclic_shift_case(ctx, mg, 257, seed=5)


def test_scaled_cyclic_shift_at_the_documented_limit(ctx, mg):
    """n = 8192, the largest coarsest level mgs_hier_finalize solves densely (the work matrix is 8192 x 16384: 1 GiB); inverse and solve
    measured at 1.03 s on one MI355X"""
    cyclic_shift_case(ctx, mg, 8192, seed=6)


def test_column_dominant_m_matrix_needs_no_swaps(ctx, mg):
    """n = 300, nonsymmetric, off-diagonals <= 0, every column strictly dominated by its diagonal — dominance that elimination keeps, so the
    pivot search stays on the diagonal: what the rest of the suite relies on"""
    rng = np.random.default_rng(31)
    A = -rng.uniform(0.0, 1.0, (300, 300)) * (rng.uniform(0, 1, (300, 300)) < 0.2)
    np.fill_diagonal(A, 0.0)
    np.fill_diagonal(A, 1.1 * np.abs(A).sum(axis=0) + 0.1)
    b = rng.standard_normal(300)
    check("column-dominant M-matrix n=300", A, b, dense_solve(ctx, mg, A, b))


def test_pivot_ties(ctx, mg):
    """first column: +2 in row 3, −2 in row 7, smaller entries elsewhere — two candidates of equal size; whichever the search takes (the
    lowest-index rule is not asserted), the solution is the reference's"""
    rng = np.random.default_rng(41)
    A = rng.uniform(-1.0, 1.0, (12, 12))
    A[3, 0], A[7, 0] = 2.0, -2.0
    b = rng.standard_normal(12)
    check("pivot ties n=12", A, b, dense_solve(ctx, mg, A, b))


# ------------------------------------------------------------------------------------------------------------------ it refuses
def refused(ctx, mg, A, sparse=False):
    with pytest.raises(mg.MgsError) as e:
        mg.Hierarchy(upload(ctx, np.asarray(A, dtype=np.float64), sparse), 0.5, 1, 1).finalize()
    return e.value.code


@pytest.mark.parametrize("name,A", [("rank one 2x2", [[1, 2], [2, 4]]),
                                    ("zero row and column", [[1, 0, 2], [0, 0, 0], [3, 0, 4]]),
                                    ("dependent rows", [[2, 4, 6], [1, 2, 3], [0, 1, 1]])])
def test_exactly_singular_is_refused(ctx, mg, name, A):
    """elimination is exact on these: a pivot of exactly zero"""
    assert refused(ctx, mg, A) == NUMERIC, name


@pytest.mark.parametrize("n", [16, 200])
@pytest.mark.parametrize("row_scaled", [False, True], ids=["symmetric", "row_scaled"])
def test_numerically_singular_laplacian_is_refused(ctx, mg, n, row_scaled):
    """rows sum to zero, non-integer weights: elimination leaves a last pivot of rounding size (<= 0.31·n·eps·max|a| in the model for
    n = 4..500), not an exact zero; the inverse it would give has entries of 1e13 and more"""
    L = laplacian(n, seed=n, row_scaled=row_scaled)
    assert np.abs(L.sum(axis=1)).max() <= 1e-13 * np.abs(L).max() and np.linalg.matrix_rank(L) == n - 1
    assert refused(ctx, mg, L) == NUMERIC


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nan_and_inf_are_refused(ctx, mg, bad):
    for where in ((0, 0), (17, 40), (63, 63)):
        A = orth_family(64, 3, seed=64)
        A[where] = bad
        assert refused(ctx, mg, A) == NUMERIC, (bad, where)


def test_refusals_through_refresh(ctx, mg):
    """a regular two-level pair whose fine VALUES are then changed so that the Galerkin coarse operator becomes the singular Laplacian:
    mgs_hier_refresh returns MGS_ERR_NUMERIC and leaves the hierarchy un-finalized (cycles: MGS_ERR_STATE) until a later refresh succeeds"""
    import scipy.sparse as sps
    nc = 16
    L = laplacian(nc, seed=3, row_scaled=False)
    # aggregates of two rows: the coarse entry (I, J) is the sum of the 2x2 fine block.  The second term has zero block sums and keeps the
    # fine diagonal positive; the third makes the coarse operator L + 2·I (regular) resp. L (singular)
    base = np.kron(L, np.full((2, 2), 0.25)) + np.kron(np.eye(nc), np.array([[3.0, -3.0], [-3.0, 3.0]]))
    regular = base + np.eye(2 * nc)
    for name, fine in (("singular", base), ("NaN", np.where(np.arange(4 * nc * nc).reshape(2 * nc, 2 * nc) == 5, np.nan, regular))):
        assert np.all(np.diag(np.nan_to_num(fine, nan=1.0)) > 0)
        A = upload(ctx, regular)
        P = sps.csr_matrix((np.ones(2 * nc), (np.arange(2 * nc), np.arange(2 * nc) // 2)), shape=(2 * nc, nc))
        h = mg.Hierarchy(A, 0.5, 1, 1).push_P(ctx.csr(2 * nc, nc, P.indptr, P.indices, P.data)).finalize()
        b = ctx.vec(np.random.default_rng(1).standard_normal(2 * nc))
        x_before = h.vcycle(b).numpy()
        coarse = h.level_A(1).download()[2].reshape(nc, nc)
        assert np.abs(coarse - (L + 2 * np.eye(nc))).max() <= 8 * EPS * np.abs(L).max()
        A.update_values(fine.ravel())
        with pytest.raises(mg.MgsError) as e:
            h.refresh()
        assert e.value.code == NUMERIC, name
        with pytest.raises(mg.MgsError) as e:
            h.vcycle(b)
        assert e.value.code == STATE, name
        A.update_values(regular.ravel())
        h.refresh()
        x_after = h.vcycle(b).numpy()
        d = np.linalg.norm(x_after - x_before) / np.linalg.norm(x_before)
        print(f"{name}: refused by refresh, restored by the next one; cycle before vs after {d:.2e}")
        assert d <= 1e-13


def test_zero_diagonal_is_refused_once_the_level_is_smoothed(ctx, mg):
    """a one-level hierarchy is the dense solve alone and takes a zero diagonal (the cyclic shift above); as soon as a level is pushed below
    it the fine level is smoothed with D⁻¹, and the same operator is refused"""
    import scipy.sparse as sps
    A = ctx.csr(4, 4, np.arange(5), [1, 2, 3, 0], [1.0, 2.0, 3.0, 4.0])
    h = mg.Hierarchy(A, 0.5, 1, 1)
    P = sps.csr_matrix((np.ones(4), (np.arange(4), np.arange(4) // 2)), shape=(4, 2))
    with pytest.raises(mg.MgsError) as e:
        h.push_P(ctx.csr(4, 2, P.indptr, P.indices, P.data))
    assert e.value.code == NUMERIC
    with pytest.raises(mg.MgsError) as e:
        h.coarsen(10.0, 2, 8.0, 1, 10)
    assert e.value.code == NUMERIC
    assert h.finalize().vcycle(ctx.vec([1.0, 2.0, 3.0, 4.0])).numpy().tolist() == [1.0, 1.0, 1.0, 1.0]
