#!/usr/bin/env python3
"""The m smallest eigenpairs of the 7-point Poisson operator at N³ rows by mgs_eig_lobpcg with PCG's V(1,1) hierarchy (ω = 0.6, device
aggregation), m = 4 and 8, tol 1e-6 on ‖A·x − θ·x‖/‖A‖∞, from Vec.rand start columns.
Every measurement is a FRESH process, the methods alternating round by round; medians of the rounds with min-max.
  lobpcgM   setup, one warm-up solve (captures the cycle's graph, fills the vector pool), one timed solve on the host clock around a
            synchronised call: seconds, iterations, and the counters of mgs_eig_info.
  passes    inside one process, windows alternating: one cycle (mgs_time_vcycle), one SpMV (mgs_time_kernel), the Gram passes and the combines
            one iteration at m = 8 makes (host clock around `reps` synchronised calls), each block pass beside a device-to-device copy of the
            same bytes — Gram (p + q)·8n per tile, combine (k + q)·8n.  The per-iteration split of a solve is these times multiplied by the
            solve's counters; what is left of the measured iteration is host time (dense algebra, launches, the waits for the Gram matrices).
            The split is not taken from device events inside the solve: the library has no such hook.
  scipyM    the detour the call replaces: the matrix downloaded, scipy.sparse.linalg.lobpcg on the host with the device cycle called back per
            column (upload, cycle, download) as preconditioner, the same start block and tolerance; N <= 128 only unless --scipy-max says more.
Nothing here is a pass/fail bar.
usage: ab_eig.py [128 256] [--rounds 3] [--methods lobpcg4,lobpcg8,passes,scipy4] [--timeout 900] [--scipy-max 128]
       ab_eig.py --child METHOD N"""
import argparse, json, os, statistics, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

METHODS = ["lobpcg4", "lobpcg8", "passes", "scipy4"]
TOL = 1e-6


def setup(mg, ctx, N):
    A = ctx.poisson3d(N).optimize()
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 2500, 32).finalize()
    return A, h


def start(ctx, n, m):
    return [ctx.vec(n).rand(1, j * n) for j in range(m)]


def child(method, N):
    import multigridsolver_amd as mg
    ctx = mg.Context(0)
    try:
        if method == "passes":
            return passes(mg, ctx, N)
        m = int(method[-1])
        return scipy_detour(mg, ctx, N, m) if method.startswith("scipy") else solve(mg, ctx, N, m)
    finally:
        ctx.close()


def solve(mg, ctx, N, m):
    A, h = setup(mg, ctx, N)
    n = N ** 3
    mg.lobpcg(A, start(ctx, n, m), h, 500, TOL)          # warm-up
    X = start(ctx, n, m)
    ctx.sync(); t0 = time.perf_counter()
    st, it, th, rs = mg.lobpcg(A, X, h, 500, TOL)
    ctx.sync(); dt = time.perf_counter() - t0
    info = mg.eig_info(ctx)
    print(json.dumps({"method": f"lobpcg{m}", "N": N, "m": m, "levels": h.nlev, "status": st, "it": it, "s": round(dt, 5), "theta": [float(t) for t in th],
                      "resid_max": float(rs.max()), "cycles": info[1], "spmvs": info[2], "restarts": info[3], "work_vectors": info[5], "captures": info[6]}), flush=True)
    return 0


def passes(mg, ctx, N, reps=20, windows=5):
    import numpy as np
    A, h = setup(mg, ctx, N)
    n = N ** 3
    V = [ctx.vec(n).rand(2, j * n) for j in range(24)]
    AV = [ctx.vec(n).rand(3, j * n) for j in range(24)]
    out16 = [ctx.vec(n) for _ in range(16)]
    b, x = ctx.vec(n).rand(4), ctx.vec(n)
    C24 = np.random.default_rng(0).standard_normal((24, 16)) / 24
    C9 = np.random.default_rng(1).standard_normal((9, 1))
    src, dst = ctx.vec(72 * n).rand(5), ctx.vec(72 * n)      # the largest comparator: nine tiles of 16 columns, half read, half written

    def clock(fn):
        fn(); ctx.sync(); t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / reps

    def copy_of(cols):          # a device-to-device copy that moves cols·8n bytes (half read, half written)
        s, d = mg.Vec.wrap(ctx, src.ptr, cols * n // 2), mg.Vec.wrap(ctx, dst.ptr, cols * n // 2)
        return clock(lambda: d.copy_from(s))
    tiles24 = 6 * 16 + 0          # symmetric 24 × 24: six tiles of 8 + 8 columns
    cases = {
        "cycle": lambda: h.time_vcycle(b, x, reps),
        "spmv": lambda: A.time_kernel(mg.OP_SPMV, b, out=x, reps=reps),
        "gram_StS_24": lambda: clock(lambda: mg.vecs_gram(V, V)),                   # six tiles
        "copy_gram_StS_24": lambda: copy_of(tiles24),
        "gram_StAS_24": lambda: clock(lambda: mg.vecs_gram(V, AV)),                 # nine tiles
        "copy_gram_StAS_24": lambda: copy_of(9 * 16),
        "gram_8x8": lambda: clock(lambda: mg.vecs_gram(V[:8], AV[:8])),             # one tile
        "copy_gram_8x8": lambda: copy_of(16),
        "gram_8x1": lambda: clock(lambda: mg.vecs_gram(V[:8], AV[:1])),             # Xᵀw of one column
        "copy_gram_8x1": lambda: copy_of(9),
        "combine_24x16": lambda: clock(lambda: mg.vecs_combine(V, C24, out16)),     # the update of X and P
        "copy_combine_24x16": lambda: copy_of(40),
        "combine_9x1": lambda: clock(lambda: mg.vecs_combine(V[:9], C9, out16[:1])),      # w − X·(Xᵀw)
        "copy_combine_9x1": lambda: copy_of(10),
    }
    res = {k: [] for k in cases}
    for _ in range(windows):
        for k, fn in cases.items():
            res[k].append(fn())
    print(json.dumps({"method": "passes", "N": N, "rows": n, "reps": reps, "ms": {k: [round(v, 5) for v in vs] for k, vs in res.items()}}), flush=True)
    return 0


def scipy_detour(mg, ctx, N, m):
    import numpy as np
    import scipy.sparse as sp
    from scipy.sparse.linalg import LinearOperator, lobpcg
    A, h = setup(mg, ctx, N)
    n = N ** 3
    X0 = np.stack([v.numpy() for v in start(ctx, n, m)], axis=1)
    bv, xv = ctx.vec(n), ctx.vec(n)

    def cycle(R):
        R = R.reshape(n, -1)
        out = np.empty_like(R)
        for j in range(R.shape[1]):
            bv.upload(np.ascontiguousarray(R[:, j])); h.vcycle(bv, xv); out[:, j] = xv.numpy()
        return out
    ctx.sync(); t0 = time.perf_counter()
    rp, ci, v = A.download()
    As = sp.csr_matrix((v, ci, rp), shape=(n, n))
    anorm = abs(As).sum(axis=1).max()
    M = LinearOperator((n, n), matvec=cycle, matmat=cycle, dtype=np.float64)
    th, X, hist = lobpcg(As, X0, M=M, tol=TOL * anorm, maxiter=500, largest=False, retResidualNormsHistory=True)
    dt = time.perf_counter() - t0
    res = np.linalg.norm(As @ X - X * th, axis=0) / anorm
    print(json.dumps({"method": f"scipy{m}", "N": N, "m": m, "it": len(hist) - 1, "s": round(dt, 5), "theta": [float(t) for t in th], "resid_max": float(res.max())}), flush=True)
    return 0


def mmm(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[128, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--methods", default=",".join(METHODS))
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--scipy-max", type=int, default=128)
    ap.add_argument("--child", nargs=2, default=None)
    o = ap.parse_args()
    if o.child:
        return child(o.child[0], int(o.child[1]))
    methods = o.methods.split(",")
    for N in o.sizes:
        runs = {m: [] for m in methods}
        for rnd in range(o.rounds):
            for m in methods:
                if (m == "passes" and rnd > 0) or (m.startswith("scipy") and (N > o.scipy_max or rnd > 0)):      # one process each: windows alternate inside / minutes per run
                    continue
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", m, str(N)], capture_output=True, text=True, timeout=o.timeout)
                if r.returncode != 0:                       # nothing more is started on the device after a failure
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    print(json.dumps({"N": N, "failed": m, "returncode": r.returncode, "partial": runs}), flush=True)
                    return 1
                line = r.stdout.strip().splitlines()[-1]
                sys.stderr.write(line[:300] + "\n"); sys.stderr.flush()
                runs[m].append(json.loads(line))
        out = {"operator": f"poisson:{N}", "rows": N ** 3, "tol": TOL, "omega": 0.6, "rounds": o.rounds, "methods": {}}
        for m in methods:
            if not runs[m]:
                continue
            if m == "passes":
                out["passes_ms"] = {k: mmm(v) for k, v in runs[m][0]["ms"].items()}
                continue
            q0 = runs[m][0]
            out["methods"][m] = {"it": sorted({q["it"] for q in runs[m]}), "s": mmm([q["s"] for q in runs[m]]),
                                 "ms_per_it": mmm([1e3 * q["s"] / max(q["it"], 1) for q in runs[m]]), "resid_max": max(q["resid_max"] for q in runs[m]),
                                 "theta": q0["theta"], **{k: q0[k] for k in ("status", "cycles", "spmvs", "restarts", "work_vectors", "captures", "levels") if k in q0}}
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
