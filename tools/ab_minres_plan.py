#!/usr/bin/env python3
"""mgs_minres against the MINRES plan (mgs_minres_plan: scalars on the device) on the saddle-point system of tools/ab_minres.py (L = the
7-point Poisson operator at N³ rows, device-built hierarchy on block_diag(L, S), ω = 0.6, V(1,1)), true residual 1e-8, with the methods
  minres    : mgs_minres — two host looks per iteration; the baseline every other row is held against
  plan_a0   : MinresPlan.solve(ahead = 0) — one host look per iteration, nothing speculative
  plan_a1   : MinresPlan.solve(ahead = 1) — one iteration kept enqueued beyond the last outcome seen
  enqueue   : MinresPlan.enqueue(iters = the count the solve needed, tol = 0) + result() — no host look; also the host time enqueue itself takes
  transpose : Csr.transpose_update(D) for the system's D against a fresh D.transpose() and against a device-to-device copy of D's values
Every solve measurement is a FRESH process (setup, one warm-up solve that captures the graphs, one timed solve: host clock around a
synchronised solve from x = 0), the methods alternating round by round.  Every plan solve must return mgs_minres's tuple: the child
compares with an mgs_minres run of its own.  Prints one JSON line per size: seconds as median with min-max.  Nothing here is a
pass/fail bar.
usage: ab_minres_plan.py [128 256] [--rounds 3] [--methods minres,plan_a0,plan_a1,enqueue,transpose] [--timeout 600]
       ab_minres_plan.py --child METHOD N"""
import argparse, json, os, statistics, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

METHODS = ["minres", "plan_a0", "plan_a1", "enqueue", "transpose"]
TOL, MAXIT = 1e-8, 2000


def solve(mg, ctx, N, method):
    from ab_minres import saddle
    K, h, rows = saddle(mg, ctx, N)
    b = ctx.vec(rows).rand(seed=0)
    x = ctx.vec(rows)
    want = mg.minres(K, x, b, h, MAXIT, TOL)              # the tuple every method is held to; the baseline's warm-up
    extra = {}
    if method == "minres":
        x.fill(0.0); ctx.sync(); t0 = time.perf_counter()
        got = mg.minres(K, x, b, h, MAXIT, TOL)
        ctx.sync(); dt = time.perf_counter() - t0
    else:
        plan = mg.MinresPlan(K, h)
        if method.startswith("plan_a"):
            ahead = int(method[6:])
            x.fill(0.0); plan.solve(x, b, MAXIT, TOL, ahead)                      # warm-up
            x.fill(0.0); ctx.sync(); t0 = time.perf_counter()
            got = plan.solve(x, b, MAXIT, TOL, ahead)
            ctx.sync(); dt = time.perf_counter() - t0
        else:
            x.fill(0.0); plan.enqueue(x, b, want[1], 0.0).result()                # warm-up
            x.fill(0.0); ctx.sync(); t0 = time.perf_counter()
            plan.enqueue(x, b, want[1], 0.0)
            t1 = time.perf_counter()
            st, it, res = plan.result()
            dt = time.perf_counter() - t0
            got = (0 if res < TOL else st, it, res)                               # tol = 0 runs the count and reports status 1: the residual is what counts
            extra["enqueue_host_s"] = round(t1 - t0, 6)
        info = plan.info()
        extra.update({"enqueued": info[2], "frozen": info[3], "waits": info[4], "recalibrations": info[5]})
    true = K.residual(x, b).nrm2() / b.nrm2()
    print(json.dumps({"method": method, "N": N, "rows": rows, "levels": h.nlev, "returned": list(got), "mgs_minres": list(want), "same": tuple(got) == tuple(want),
                      "s": round(dt, 5), "true_res": true, **extra}), flush=True)
    return 0 if tuple(got) == tuple(want) else 3


def transpose(mg, ctx, N, reps=20, windows=7):
    import numpy as np
    n = N ** 3; m = (n + 1) // 2
    r = np.arange(m, dtype=np.int64)
    cols = np.stack([2 * r, 2 * r + 1], axis=1); vals = np.stack([np.ones(m), -np.ones(m)], axis=1)
    keep = cols < n
    rowptr = np.zeros(m + 1, dtype=np.int64); np.cumsum(keep.sum(axis=1), out=rowptr[1:])
    D = ctx.csr(m, n, rowptr.astype(np.int32), cols[keep].astype(np.int32), vals[keep])
    Dt = D.transpose()
    nnz = D.nnz
    src, dst = ctx.vec(nnz).rand(seed=1), ctx.vec(nnz)
    D.update_values(src, nnz)
    Dt.transpose_update(D, check=True)
    fresh = D.transpose()
    same = all(p.tobytes() == q.tobytes() for p, q in zip(Dt.download(), fresh.download()))
    del fresh
    out = {"update": [], "fresh": [], "copy": []}

    def timed(fn, k):
        ctx.sync(); t0 = time.perf_counter()
        for _ in range(k):
            fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / k
    for _ in range(windows):
        out["update"].append(timed(lambda: Dt.transpose_update(D), reps))
        out["fresh"].append(timed(lambda: D.transpose(), 3))
        out["copy"].append(timed(lambda: dst.copy_from(src), reps))
    print(json.dumps({"method": "transpose", "N": N, "shape": [m, n], "nnz": nnz, "same_bits": same, "ms": {k: [round(v, 5) for v in vs] for k, vs in out.items()}}), flush=True)
    return 0 if same else 3


def child(method, N):
    import multigridsolver_amd as mg
    ctx = mg.Context(0)
    try:
        return transpose(mg, ctx, N) if method == "transpose" else solve(mg, ctx, N, method)
    finally:
        ctx.close()


def mmm(v):
    return {"median": round(statistics.median(v), 6), "min": round(min(v), 6), "max": round(max(v), 6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[128, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--methods", default=",".join(METHODS))
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", nargs=2, default=None)
    o = ap.parse_args()
    if o.child:
        return child(o.child[0], int(o.child[1]))
    methods = o.methods.split(",")
    for N in o.sizes:
        runs = {m: [] for m in methods}
        for rnd in range(o.rounds):
            for m in methods:
                if m == "transpose" and rnd > 0:      # its windows alternate inside one process
                    continue
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", m, str(N)], capture_output=True, text=True, timeout=o.timeout)
                if r.returncode != 0:                       # nothing more is started on the device after a failure
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    print(json.dumps({"N": N, "failed": m, "returncode": r.returncode, "partial": runs}), flush=True)
                    return 1
                line = r.stdout.strip().splitlines()[-1]
                sys.stderr.write(line[:400] + "\n"); sys.stderr.flush()        # progress: a size takes minutes
                runs[m].append(json.loads(line))
        out = {"operator": f"saddle on poisson:{N}", "rows": N ** 3 + (N ** 3 + 1) // 2, "tol": TOL, "omega": 0.6, "rounds": o.rounds, "methods": {}}
        for m in methods:
            if m == "transpose":
                q = runs[m][0]
                out["transpose"] = {"shape": q["shape"], "nnz": q["nnz"], "same_bits": q["same_bits"], "ms": {k: mmm(v) for k, v in q["ms"].items()}}
                continue
            e = {"it": sorted({q["returned"][1] for q in runs[m]}), "same_as_mgs_minres": all(q["same"] for q in runs[m]), "s": mmm([q["s"] for q in runs[m]]),
                 "ms_per_it": mmm([1e3 * q["s"] / max(q["returned"][1], 1) for q in runs[m]]), "true_res": max(q["true_res"] for q in runs[m])}
            for k in ("enqueued", "frozen", "waits", "recalibrations"):
                if k in runs[m][0]:
                    e[k] = sorted({q[k] for q in runs[m]})
            if "enqueue_host_s" in runs[m][0]:
                e["enqueue_host_s"] = mmm([q["enqueue_host_s"] for q in runs[m]])
            out["methods"][m] = e
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
