#!/usr/bin/env python3
"""The 4 smallest eigenpairs of A·x = λ·B·x by mgs_eig_lobpcg_gen, A the 7-point Poisson operator at N³ rows, B = diag(ρ) + L/24 (ρ uniform in
[0.75, 1.25], L the same Poisson operator; built on the device with Csr.from_diag and add), with PCG's V(1,1) hierarchy on A (ω = 0.6, device
aggregation), tol 1e-6, from Vec.rand start columns — beside mgs_eig_lobpcg on A alone in the same process.
Every measurement is a FRESH process, the methods alternating round by round; medians of the rounds with min-max.
  pair      setup, one warm-up solve of each kind, then one timed solve of each on the host clock around a synchronised call: seconds, iterations,
            seconds per iteration and the counters of mgs_eig_info for both.  By streams an iteration of the generalised solver moves about 8/5
            of the vector traffic (8 blocks against 5) and twice the SpMVs.
  residual  inside one process, windows alternating, device events on the context's stream around 50 calls on three input columns in turn:
            eig_residual        mgs_eig_residual with nrm2 = NULL (fold only, enqueued);
            eig_residual_fetch  the same with the host look, as mgs_eig_lobpcg_gen calls it;
            combine_dot_fetch   the pair it replaces, a 2 → 1 mgs_vecs_combine followed by mgs_dot with its host look, as mgs_eig_lobpcg calls it;
            copy_32B_per_row    a device-to-device copy of 32 B per row (16 read, 16 written).
Nothing here is a pass/fail bar.
usage: ab_eig_gen.py [128 256] [--rounds 3] [--methods pair,residual] [--timeout 900]
       ab_eig_gen.py --child METHOD N"""
import argparse, json, os, statistics, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

METHODS = ["pair", "residual"]
TOL = 1e-6
M = 4


def setup(mg, ctx, N):
    import numpy as np
    A = ctx.poisson3d(N).optimize()
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 2500, 32).finalize()
    rho = np.random.default_rng(7).uniform(0.75, 1.25, N ** 3)
    B = mg.Csr.from_diag(ctx, ctx.vec(rho)).add(ctx.poisson3d(N), 1.0, 1.0 / 24.0).optimize()
    return A, B, h


def start(ctx, n, m):
    return [ctx.vec(n).rand(1, j * n) for j in range(m)]


def pair(mg, ctx, N):
    A, B, h = setup(mg, ctx, N)
    n = N ** 3
    out = {"method": "pair", "N": N, "m": M, "levels": h.nlev}
    for tag, Bm in (("std", None), ("gen", B)):
        mg.lobpcg(A, start(ctx, n, M), h, 500, TOL, B=Bm)          # warm-up: captures the cycle's graph, fills the vector pool
    for tag, Bm in (("std", None), ("gen", B)):
        X = start(ctx, n, M)
        ctx.sync(); t0 = time.perf_counter()
        st, it, th, rs = mg.lobpcg(A, X, h, 500, TOL, B=Bm)
        ctx.sync(); dt = time.perf_counter() - t0
        info = mg.eig_info(ctx)
        out[tag] = {"status": st, "it": it, "s": round(dt, 5), "theta": [float(t) for t in th], "resid_max": float(rs.max()), "cycles": info[1], "spmvs": info[2],
                    "spmvs_b": info[7], "restarts": info[3], "work_vectors": info[5], "captures": info[6]}
    print(json.dumps(out), flush=True)
    return 0


def residual(mg, ctx, N, calls=50, windows=5):
    import numpy as np
    import torch
    n = N ** 3
    cols = [(ctx.vec(n).rand(2, j * n), ctx.vec(n).rand(3, j * n)) for j in range(3)]
    r = ctx.vec(n)
    src, dst = ctx.vec(2 * n).rand(5), ctx.vec(2 * n)
    stream = torch.cuda.ExternalStream(ctx.stream)
    L = mg.lib()
    c2 = np.array([[0.7], [1.0]])

    def events(fn):
        fn(cols[0]); ctx.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for k in range(calls):
            fn(cols[k % 3])
        e1.record(stream); e1.synchronize()
        return e0.elapsed_time(e1) / calls

    def fused(c):
        assert L.mgs_eig_residual(ctx.h, n, c[0].h, c[1].h, 0.7, r.h, None) == 0

    def fused_fetch(c):
        mg.eig_residual(c[0], c[1], 0.7, r)

    def two_fetch(c):
        mg.vecs_combine([c[1], c[0]], c2, [r]); r.dot(r)
    cases = {"eig_residual": lambda: events(fused), "eig_residual_fetch": lambda: events(fused_fetch), "combine_dot_fetch": lambda: events(two_fetch),
             "copy_32B_per_row": lambda: events(lambda c: dst.copy_from(src))}
    res = {k: [] for k in cases}
    for _ in range(windows):
        for k, fn in cases.items():
            res[k].append(fn())
    print(json.dumps({"method": "residual", "N": N, "rows": n, "calls": calls, "ms": {k: [round(v, 5) for v in vs] for k, vs in res.items()}}), flush=True)
    return 0


def child(method, N):
    if method == "residual":
        import torch  # noqa: F401  — before libmgs.so: both link a HIP runtime, the first one loaded serves the process
    import multigridsolver_amd as mg
    ctx = mg.Context(0)
    try:
        return {"pair": pair, "residual": residual}[method](mg, ctx, N)
    finally:
        ctx.close()


def mmm(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[128, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--methods", default=",".join(METHODS))
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--child", nargs=2, default=None)
    o = ap.parse_args()
    if o.child:
        return child(o.child[0], int(o.child[1]))
    methods = o.methods.split(",")
    for N in o.sizes:
        runs = {m: [] for m in methods}
        for rnd in range(o.rounds):
            for m in methods:
                if m == "residual" and rnd > 0:      # one process: its windows alternate inside
                    continue
                r = subprocess.run(["timeout", "-k", "10", str(o.timeout), sys.executable, os.path.abspath(__file__), "--child", m, str(N)], capture_output=True, text=True)
                if r.returncode != 0:                       # nothing more is started on the device after a failure
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    print(json.dumps({"N": N, "failed": m, "returncode": r.returncode, "partial": runs}), flush=True)
                    return 1
                line = r.stdout.strip().splitlines()[-1]
                sys.stderr.write(line[:300] + "\n"); sys.stderr.flush()
                runs[m].append(json.loads(line))
        out = {"operator": f"poisson:{N}", "rows": N ** 3, "m": M, "tol": TOL, "omega": 0.6, "rounds": o.rounds}
        if runs.get("pair"):
            for tag in ("std", "gen"):
                qs = [q[tag] for q in runs["pair"]]
                out[tag] = {"it": sorted({q["it"] for q in qs}), "s": mmm([q["s"] for q in qs]), "ms_per_it": mmm([1e3 * q["s"] / max(q["it"], 1) for q in qs]),
                            "resid_max": max(q["resid_max"] for q in qs), "theta": qs[0]["theta"],
                            **{k: qs[0][k] for k in ("status", "cycles", "spmvs", "spmvs_b", "restarts", "work_vectors", "captures")}}
            out["levels"] = runs["pair"][0]["levels"]
        if runs.get("residual"):
            out["residual_ms"] = {k: mmm(v) for k, v in runs["residual"][0]["ms"].items()}
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
