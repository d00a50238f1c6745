"""mgs_eig_lobpcg_gen and mgs_eig_residual on the device against tests/eig_gen_ref.py.

The residual pass is held bit for bit: r_i = fl(ax_i − fl(θ·bx_i)) and ‖r‖² = blas1_ref.dot(r, r) under k_dot's launch decisions, on both arms.

The solver, on A = poisson6 / poisson8d and B = diag(ρ) + L/24 built on the device (Csr.from_diag, add), with no preconditioner and with a one-level
hierarchy (the dense inverse).  Bars, none of them taken from what the library returns:
  * status 0 at tol 1e-6 within 200 iterations;
  * |θ_j − λ_j| ≤ 1e-8·λ_j, λ from scipy.linalg.eigh(A, B) on the dense matrices;
  * max|XᵀBX − I| ≤ 1e-12 with the downloaded X and NumPy's B;
  * every resid[j] equals ‖A·x_j − θ_j·B·x_j‖₂/(‖A‖∞ + |θ_j|·‖B‖∞) recomputed in NumPy from the downloaded X, to 1e-12 absolute;
  * iterations within ±2 of eig_gen_ref.ITERATIONS (the summation order differs).
With a multilevel V(1,1) hierarchy fewer iterations than without; B = None gives mgs_eig_lobpcg's bits, B = I its θ to 1e-12 and its iteration
count; one capture in a first call, none in a repeated one; 8m + 2 work vectors; two identical calls give identical bits."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg

import eig_gen_ref as G
import eig_ref as E
from test_gpu_blas1_bits import LENGTHS

pytestmark = pytest.mark.gpu

INVALID = -1
TOL = 1e-6
GRID = {"poisson6": 6, "poisson8d": 8}


@pytest.fixture(scope="module")
def mg():
    import multigridsolver_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    c = mg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------- mgs_eig_residual
_RES = {}


def res_inputs(n):
    if n not in _RES:
        ax, bx, th = G.residual_fixture(n)
        ax.setflags(write=False); bx.setflags(write=False)
        _RES[n] = (ax, bx, th)
    return _RES[n]


def place(mg, ctx, a, aligned, keep):
    if aligned:
        return ctx.vec(a)
    buf = ctx.vec(np.concatenate([[7.0], a, [7.0]]))
    keep.append(buf)
    v = mg.Vec.wrap(ctx, buf.ptr + 8, len(a))
    assert v.ptr % 16 == 8
    return v


def check_residual(mg, ctx, n, off, launch, alias=None):
    """off: which of the three vectors sits 8 bytes off 16-byte alignment (None: all aligned); alias: r is "ax" or "bx" """
    ax, bx, th = res_inputs(n)
    keep = []
    vax = place(mg, ctx, ax, off != "ax", keep)
    vbx = place(mg, ctx, bx, off != "bx", keep)
    vr = vax if alias == "ax" else vbx if alias == "bx" else place(mg, ctx, np.full(n, np.nan), off != "r", keep)
    want_r, want_s = G.residual(ax, bx, th, aligned=off is None, **launch)
    got_s = mg.eig_residual(vax, vbx, th, vr)
    tag = (n, off, alias, launch)
    assert np.array_equal(bits(vr.numpy()), bits(want_r)), tag
    assert bits(got_s) == bits(want_s), (tag, got_s, want_s)
    if alias is None:
        again = mg.eig_residual(vax, vbx, th, vr)      # two calls: identical bits
        assert bits(again) == bits(got_s) and np.array_equal(bits(vr.numpy()), bits(want_r)), tag
        assert np.array_equal(bits(vax.numpy()), bits(ax)) and np.array_equal(bits(vbx.numpy()), bits(bx)), tag      # inputs only read
    for buf in keep:      # the guard entries around an offset vector keep their value
        h = buf.numpy()
        assert h[0] == 7.0 and h[-1] == 7.0, tag


@pytest.mark.parametrize("off", [None, "r", "bx"], ids=["aligned", "r_off8", "bx_off8"])
@pytest.mark.parametrize("n", LENGTHS)
def test_residual_bits(mg, ctx, n_cu, n, off):
    check_residual(mg, ctx, n, off, {"n_cu": n_cu})


@pytest.mark.parametrize("alias", ["ax", "bx"])
@pytest.mark.parametrize("n", (1, 2, 513, 1_048_579))
def test_residual_in_place(mg, ctx, n_cu, n, alias):
    check_residual(mg, ctx, n, None, {"n_cu": n_cu}, alias=alias)
    check_residual(mg, ctx, n, alias, {"n_cu": n_cu}, alias=alias)      # in place on the 8-byte arm


def test_residual_without_blas1_vec(mg, ctx, n_cu):
    try:
        ctx.set_option("blas1_vec", 0)
        for n in (513, 2_097_665):
            check_residual(mg, ctx, n, None, {"n_cu": n_cu, "blas1_vec": 0})
    finally:
        ctx.set_option("blas1_vec", 1)


def test_residual_fold_only_and_refusals(mg, ctx, n_cu):
    from multigridsolver_amd._lib import lib
    L = lib()
    n = 513
    ax, bx, th = res_inputs(n)
    vax, vbx, vr = ctx.vec(ax), ctx.vec(bx), ctx.vec(n)
    assert L.mgs_eig_residual(ctx.h, n, vax.h, vbx.h, th, vr.h, None) == 0      # nrm2 NULL: fold only
    ctx.sync()
    assert np.array_equal(bits(vr.numpy()), bits(G.residual(ax, bx, th, n_cu=n_cu)[0]))
    s = C.c_double(-7.0)
    before = vr.numpy()
    call = lambda c, k, a, b, r: L.mgs_eig_residual(c, k, a, b, th, r, C.byref(s))
    assert call(None, n, vax.h, vbx.h, vr.h) == INVALID
    for a, b, r in ((None, vbx.h, vr.h), (vax.h, None, vr.h), (vax.h, vbx.h, None)):
        assert call(ctx.h, n, a, b, r) == INVALID
    assert call(ctx.h, 0, vax.h, vbx.h, vr.h) == INVALID and call(ctx.h, n + 1, vax.h, vbx.h, vr.h) == INVALID
    part = mg.Vec.wrap(ctx, vax.ptr + 16, n - 2)                                      # r inside ax without being ax
    assert call(ctx.h, n - 2, vax.h, vbx.h, part.h) == INVALID and "overlaps ax" in L.mgs_last_error(ctx.h).decode()
    other = mg.Context(0)
    try:
        ov = other.vec(n)
        assert call(ctx.h, n, vax.h, vbx.h, ov.h) == INVALID and "another context" in L.mgs_last_error(ctx.h).decode()
        del ov
    finally:
        other.close()
    assert s.value == -7.0 and np.array_equal(bits(vr.numpy()), bits(before))      # nothing was launched


# ------------------------------------------------------------------------------------------------------------- the solver
_HOST = {}


def host(name):
    """(dense A, dense B, ‖A‖∞, ‖B‖∞, the pencil's eigenvalues, inv(A)), computed once"""
    if name not in _HOST:
        A, _ = E.fixture(name)
        B = G.mass(name)
        _HOST[name] = (A, B, np.abs(A).sum(axis=1).max(), np.abs(B).sum(axis=1).max(), scipy.linalg.eigh(A, B, eigvals_only=True), E.dense_inverse(A, None))
    return _HOST[name]


def device_pair(mg, ctx, name):
    N = GRID[name]
    A = ctx.poisson3d(N)
    if name == "poisson8d":
        A = A + mg.Csr.from_diag(ctx, ctx.vec(np.random.default_rng(5).uniform(0, 1, 512)))
    rho, _ = G.mass_parts(name)
    B = mg.Csr.from_diag(ctx, ctx.vec(rho)).add(ctx.poisson3d(N), 1.0, 1.0 / 24.0)
    return A, B


def hierarchy(mg, A, kind):
    if kind == "none":
        return None
    if kind == "one":
        return mg.Hierarchy(A).finalize()
    h = mg.Hierarchy(A).coarsen(10, 2, 8, coarse_rows=30).finalize()
    assert h.nlev >= 2
    return h


def run(mg, ctx, A, B, h, X0, max_iter=200, tol=TOL):
    X = [ctx.vec(np.ascontiguousarray(X0[:, j])) for j in range(X0.shape[1])]
    st, it, th, rs = mg.lobpcg(A, X, h, max_iter, tol, B=B)
    return dict(status=st, iterations=it, theta=th, resid=rs, X=np.stack([x.numpy() for x in X], axis=1), info=mg.eig_info(ctx))


def solve(mg, ctx, name, m, kind, **kw):
    A, B = device_pair(mg, ctx, name)
    return run(mg, ctx, A, B, hierarchy(mg, A, kind), E.start_block(A.shape[0], m), **kw)


_SOLVED = {}


def solved(mg, ctx, name, m, kind):
    if (name, m, kind) not in _SOLVED:
        _SOLVED[(name, m, kind)] = solve(mg, ctx, name, m, kind)
    return _SOLVED[(name, m, kind)]


def check_result(name, m, r, converged=True):
    A, B, anorm, bnorm, lam, _ = host(name)
    X, th, rs = r["X"], r["theta"], r["resid"]
    assert np.all(np.diff(th) >= 0)
    orth = np.abs(X.T @ B @ X - np.eye(m)).max()
    true = np.linalg.norm(A @ X - (B @ X) * th, axis=0) / (anorm + np.abs(th) * bnorm)
    dth = np.abs(th - lam[:m]) / lam[:m]
    print(f"  max|XtBX-I| {orth:.3e}, max|resid - recomputed| {np.abs(rs - true).max():.3e}, max|dtheta|/theta {dth.max():.3e}")
    assert orth <= 1e-12, orth
    assert np.all(np.abs(rs - true) <= 1e-12), (rs, true)
    if converged:
        assert np.all(dth <= 1e-8), (th, lam[:m])


@pytest.mark.parametrize("kind", ["none", "one"])
@pytest.mark.parametrize("name,m", G.CASES)
def test_converges_to_the_smallest_eigenpairs_of_the_pencil(mg, ctx, name, m, kind):
    r = solved(mg, ctx, name, m, kind)
    it_ref = G.ITERATIONS[(name, m, "none" if kind == "none" else "inverse")]
    print(f"{name} m={m} {kind}: status {r['status']}, iterations {r['iterations']} (eig_gen_ref {it_ref}), info {r['info']}")
    assert r["status"] == 0 and r["iterations"] <= 200 and (r["resid"] < TOL).all(), (r["status"], r["iterations"], r["resid"])
    check_result(name, m, r)
    assert abs(r["iterations"] - it_ref) <= 2, (r["iterations"], it_ref)
    info = r["info"]
    assert info[0] == r["iterations"] and info[5] == 8 * m + 2 and info[4] == m
    assert info[2] == 2 * info[7] and info[7] > 0      # every block goes through A and through B once
    assert (info[1] == 0) == (kind == "none")


def test_multilevel_hierarchy_beats_no_preconditioner(mg, ctx):
    r = solved(mg, ctx, "poisson8d", 4, "multi")
    none = solved(mg, ctx, "poisson8d", 4, "none")
    print(f"poisson8d m=4: V(1,1) {r['iterations']} iterations, none {none['iterations']}; cycles {r['info'][1]}, captures {r['info'][6]}")
    assert r["status"] == 0 and (r["resid"] < TOL).all()
    check_result("poisson8d", 4, r)
    assert r["iterations"] < none["iterations"] and r["info"][1] > 0


def test_without_B_the_call_is_mgs_eig_lobpcg(mg, ctx):
    from multigridsolver_amd._lib import lib
    A, _ = device_pair(mg, ctx, "poisson8d")
    X0 = E.start_block(512, 4)
    a = run(mg, ctx, A, None, None, X0)      # lobpcg(B=None) → mgs_eig_lobpcg_gen(B = NULL)
    X = [ctx.vec(np.ascontiguousarray(X0[:, j])) for j in range(4)]
    th, rs = (C.c_double * 4)(), (C.c_double * 4)()
    mi, tol, st = C.c_int(200), C.c_double(TOL), C.c_int(-1)
    assert lib().mgs_eig_lobpcg(A.h, None, 4, (C.c_void_p * 4)(*[x.h for x in X]), th, rs, C.byref(mi), C.byref(tol), C.byref(st)) == 0
    assert (a["status"], a["iterations"]) == (st.value, mi.value) and a["status"] == 0
    assert np.array_equal(bits(a["theta"]), bits(list(th))) and np.array_equal(bits(a["resid"]), bits(list(rs)))
    assert np.array_equal(bits(a["X"]), bits(np.stack([x.numpy() for x in X], axis=1)))
    assert a["info"][5] == 5 * 4 + 2 and a["info"][7] == 0
    # B = I: the same θ to 1e-12 and the same iteration count, through the generalised loop
    one = run(mg, ctx, A, mg.Csr.from_diag(ctx, ctx.vec(np.ones(512))), None, X0)
    print("B = None / B = I: iterations", a["iterations"], one["iterations"], "max|dtheta|", np.abs(a["theta"] - one["theta"]).max())
    assert one["status"] == 0 and one["iterations"] == a["iterations"] and one["info"][5] == 8 * 4 + 2
    assert np.abs(a["theta"] - one["theta"]).max() <= 1e-12


def test_captures_and_repeats(mg, ctx):
    A, B = device_pair(mg, ctx, "poisson8d")
    h = hierarchy(mg, A, "multi")      # a fresh hierarchy: its graph cache starts empty
    X0 = E.start_block(512, 4)
    a = run(mg, ctx, A, B, h, X0)
    b = run(mg, ctx, A, B, h, X0)
    print("captures:", a["info"][6], b["info"][6])
    assert a["info"][6] == 1 and b["info"][6] == 0      # option "graph" is on by default: one capture, then replays
    assert a["info"][5] == b["info"][5] == 8 * 4 + 2 and a["info"][1] > 0
    for k in ("theta", "resid", "X"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert a["iterations"] == b["iterations"] and a["status"] == b["status"] == 0
    assert a["info"][:6] == b["info"][:6] and a["info"][7] == b["info"][7]


def test_status_paths(mg, ctx):
    A, B = device_pair(mg, ctx, "poisson8d")
    X0 = E.start_block(512, 4)
    r = run(mg, ctx, A, B, None, X0, max_iter=2)
    assert r["status"] == 1 and r["iterations"] == 2
    check_result("poisson8d", 4, r, converged=False)
    X1 = X0.copy(); X1[:, 2] = X1[:, 0]
    r = run(mg, ctx, A, B, None, X1)
    assert r["status"] == 2 and r["iterations"] == 0 and np.array_equal(bits(r["X"]), bits(X1))      # X untouched
    r = run(mg, ctx, A, mg.Csr.from_diag(ctx, ctx.vec(-np.ones(512))), None, X0)
    assert r["status"] == 2 and r["iterations"] == 0 and np.array_equal(bits(r["X"]), bits(X0))      # B = −I is not positive definite


def test_refusals(mg, ctx):
    from multigridsolver_amd import synthetic
    from multigridsolver_amd._lib import lib
    L = lib()
    A, B = device_pair(mg, ctx, "poisson6")
    n = 216
    X = [ctx.vec(np.ascontiguousarray(c)) for c in E.start_block(n, 9).T]
    H = lambda vs: (C.c_void_p * max(len(vs), 1))(*[v.h for v in vs])
    th, rs = (C.c_double * 16)(), (C.c_double * 16)()
    mi, tol, st = C.c_int(10), C.c_double(TOL), C.c_int(-7)
    before = [x.numpy() for x in X]

    def refused(Ah, Bh, hh, m, Xs, word):
        assert L.mgs_eig_lobpcg_gen(Ah, Bh, hh, m, Xs, th, rs, C.byref(mi), C.byref(tol), C.byref(st)) == INVALID, word
        msg = L.mgs_last_error(ctx.h).decode()
        assert "mgs_eig_lobpcg_gen" in msg and word in msg, msg
    small, shard = ctx.poisson3d(5), ctx.poisson3d(6, 0, 3)
    refused(A.h, small.h, None, 2, H(X), "B is 125 x 125")                                              # another size
    refused(A.h, shard.h, None, 2, H(X), "row shard")                                                   # B a row shard
    other = mg.Context(0)
    try:
        oB = other.poisson3d(6)
        refused(A.h, oB.h, None, 2, H(X), "another context")
        del oB
    finally:
        other.close()
    rp, ci, v = synthetic.neumann3d(6)
    N = ctx.csr(216, 216, rp, ci, v).set_nullspace("constant")
    refused(N.h, B.h, None, 2, H(X), "null space is declared on A")
    refused(A.h, N.h, None, 2, H(X), "null space is declared on B")
    assert "B-orthogonal" in L.mgs_last_error(ctx.h).decode()
    refused(A.h, B.h, None, 9, H(X), "block of 9")
    refused(A.h, B.h, None, 0, H(X), "block of 0")
    long = ctx.vec(2 * n)
    short, inside = mg.Vec.wrap(ctx, long.ptr + 8, n - 1), mg.Vec.wrap(ctx, long.ptr + 8 * 100, n)
    refused(A.h, B.h, None, 2, H([X[0], short]), "holds 215")                                           # too short …
    refused(A.h, B.h, None, 2, H([long, inside]), "overlap")                                            # … and overlapping columns
    refused(A.h, B.h, None, 2, H([X[0], X[0]]), "same vector")
    h = mg.Hierarchy(A).coarsen(10, 2, 8, coarse_rows=30).finalize()
    h.set_smoother(0.5, 1, 2)
    refused(A.h, B.h, h.h, 2, H(X), "nu1 == nu2")                                                       # V(1,2)
    h.set_smoother(0.5, 1, 1).set_kcycle(1)
    refused(A.h, B.h, h.h, 2, H(X), "K-cycle")
    h.set_kcycle(0)
    assert st.value == -7 and all(np.array_equal(x.numpy(), b) for x, b in zip(X, before))             # nothing was launched
    assert L.mgs_eig_lobpcg_gen(A.h, B.h, h.h, 2, H(X), th, rs, C.byref(mi), C.byref(tol), C.byref(st)) == 0 and st.value in (0, 1)


def test_solve_cli_eigs_with_mass(mg, tmp_path):
    from multigridsolver_amd import synthetic
    rp, ci, v = synthetic._poisson3d_dirichlet(6)
    a_path, b_path = str(tmp_path / "poisson6.mtx"), str(tmp_path / "mass6.mtx")
    mg.write_mtx(a_path, 216, 216, rp, ci, v)
    rho, _ = G.mass_parts("poisson6")
    vb = v / 24.0
    vb[ci == np.repeat(np.arange(216), np.diff(rp))] += rho
    mg.write_mtx(b_path, 216, 216, rp, ci, vb)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "multigridsolver_amd.solve", a_path, "--eigs", "3", "--mass", b_path], capture_output=True, text=True, timeout=120, cwd=repo)
    assert r.returncode == 0, r.stdout + r.stderr
    vals = [float(m.group(1)) for m in re.finditer(r"Eigenvalue \d+\s+: ([0-9.eE+-]+) \(residual", r.stdout)]
    dense = []
    for path in (a_path, b_path):      # the matrices as the files hold them (the writer keeps fewer digits than a double)
        _, _, frp, fci, fv = mg.read_mtx(path)
        D = np.zeros((216, 216)); np.add.at(D, (np.repeat(np.arange(216), np.diff(frp)), fci), fv)
        dense.append(D)
    anorm, bnorm = (np.abs(D).sum(axis=1).max() for D in dense)
    want = scipy.linalg.eigh(dense[0], dense[1], eigvals_only=True)[:3]
    # the residual theorem for the pencil and a B-normalised x: |θ − λ| ≤ ‖B^(−1/2)·r‖₂ ≤ ‖r‖₂/√λmin(B), with ‖r‖₂ < tol·(‖A‖∞ + θ·‖B‖∞) at status 0 (the
    # CLI's default tol 1e-6) and λmin(B) ≥ 0.75 by Gershgorin; 1e-10 for the twelve printed digits
    bound = 1e-6 * (anorm + want * bnorm) / np.sqrt(0.75) + 1e-10
    assert len(vals) == 3 and np.all(np.abs(np.array(vals) - want) <= bound), (vals, want, bound)
    r = subprocess.run([sys.executable, "-m", "multigridsolver_amd.solve", a_path, "--mass", b_path], capture_output=True, text=True, timeout=120, cwd=repo)
    assert r.returncode != 0 and "--mass" in r.stderr and "--eigs" in r.stderr      # refused before a device is touched
