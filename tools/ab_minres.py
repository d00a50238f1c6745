#!/usr/bin/env python3
"""MINRES + V(1,1) (mgs_minres) against BiCGSTAB + V(1,1) on the saddle-point system K = [[L, Dᵀ], [D, −C]] built on the 7-point Poisson
operator L at N³ rows: D every second row of I − shift, C = 1e-2·I, preconditioner the device-built hierarchy (ω = 0.6) on block_diag(L, S),
S = C + D·diag(L)⁻¹·Dᵀ — the recipe of README.md, assembled on the device.  Both methods solve to 1e-8; what counts as reached is the TRUE
residual, recomputed after the solve (BiCGSTAB's status 0 rests on its recursive residual).
Every measurement is a FRESH process (setup, one warm-up solve that captures the graphs and fills the vector pool, one timed solve: host clock
around a synchronised solve), the methods alternating round by round.  Prints one JSON line per size: per method iterations, cycle
applications, seconds and milliseconds per iteration as median with min-max, the true residual, work vectors held.
`update`: k_minres_update alone (mgs_time_kernel op 3, device events, 50 launches per window) with plain stores and with the streaming store on
w_prev (option minres_nt), alternating inside one process, beside a device-to-device copy that moves the same 48 B per row (3 doubles read,
3 written); median with min-max over the windows.  Nothing here is a pass/fail bar.
usage: ab_minres.py [128 256] [--rounds 3] [--methods minres_v,bicgstab_v,update] [--timeout 600]
       ab_minres.py --child METHOD N"""
import argparse, json, os, statistics, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

METHODS = ["minres_v", "bicgstab_v", "update"]
VECTORS = {"minres_v": 7, "bicgstab_v": 8}      # work vectors of the operator's size a solve holds
CYCLES = {"minres_v": 1, "bicgstab_v": 2}       # cycle applications (and SpMVs) per iteration
TOL = 1e-8


def saddle(mg, ctx, N):
    """→ (K, hierarchy on block_diag(L, S), rows of K), everything but D's pattern made on the device"""
    import numpy as np
    n = N ** 3
    m = (n + 1) // 2
    L = ctx.poisson3d(N)
    r = np.arange(m, dtype=np.int64)
    cols = np.stack([2 * r, 2 * r + 1], axis=1)
    vals = np.stack([np.ones(m), -np.ones(m)], axis=1)
    keep = cols < n
    rowptr = np.zeros(m + 1, dtype=np.int64); np.cumsum(keep.sum(axis=1), out=rowptr[1:])
    D = ctx.csr(m, n, rowptr.astype(np.int32), cols[keep].astype(np.int32), vals[keep])
    C = mg.Csr.from_diag(ctx, ctx.vec(np.full(m, 1e-2)))
    Cm = mg.Csr.from_diag(ctx, ctx.vec(np.full(m, -1e-2)))
    K = mg.Csr.bmat(ctx, [[L, D.transpose()], [D, Cm]]).optimize()
    S = C + (D @ D.transpose().scale(left=L.diag_inv()))
    B = mg.Csr.block_diag(ctx, [L, S])
    h = mg.Hierarchy(B, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 2500, 32).finalize()
    return K, h, n + m


def child(method, N):
    import multigridsolver_amd as mg
    ctx = mg.Context(0)
    try:
        return update(mg, ctx, N) if method == "update" else solve(mg, ctx, N, method)
    finally:
        ctx.close()


def solve(mg, ctx, N, method):
    K, h, rows = saddle(mg, ctx, N)
    b = ctx.vec(rows).rand(seed=0)
    run = {"minres_v": lambda x: mg.minres(K, x, b, h, 2000, TOL), "bicgstab_v": lambda x: mg.bicgstab(K, x, b, h, 2000, TOL)}[method]
    x = ctx.vec(rows)
    run(x)                                       # warm-up
    x.fill(0.0); ctx.sync(); t0 = time.perf_counter()
    st, it, res = run(x)
    ctx.sync(); dt = time.perf_counter() - t0
    true = K.residual(x, b).nrm2() / b.nrm2()
    print(json.dumps({"method": method, "N": N, "rows": rows, "levels": h.nlev, "status": st, "it": it, "s": round(dt, 5), "reported": res, "true_res": true}), flush=True)
    return 0                                     # a status other than 0 is a result (it is in the line above), not a failed child


def update(mg, ctx, N, reps=50, windows=7):
    n = N ** 3 + (N ** 3 + 1) // 2               # the rows of the saddle system at this N
    import numpy as np
    A = ctx.csr(n, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))      # an n-row handle: the pass runs over A's rows and does not read the matrix
    z, w, wp, x = (ctx.vec(n).rand(seed=s) for s in (1, 2, 3, 4))
    src, dst = ctx.vec(3 * n).rand(seed=5), ctx.vec(3 * n)
    out = {"upd_plain": [], "upd_nt": [], "copy": []}

    def copy_ms():
        ctx.sync(); t0 = time.perf_counter()
        for _ in range(reps):
            dst.copy_from(src)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / reps
    for nt in (0, 1):                            # warm-up of every variant
        ctx.set_option("minres_nt", nt); A.time_kernel(mg.OP_MINRES_UPDATE, z, w, wp, x, 5)
    copy_ms()
    for _ in range(windows):
        for nt, key in ((0, "upd_plain"), (1, "upd_nt")):
            ctx.set_option("minres_nt", nt)
            out[key].append(A.time_kernel(mg.OP_MINRES_UPDATE, z, w, wp, x, reps))
        out["copy"].append(copy_ms())
    ctx.set_option("minres_nt", 0)
    print(json.dumps({"method": "update", "N": N, "rows": n, "bytes_per_row": 48, "reps": reps,
                      "ms": {k: [round(v, 5) for v in vs] for k, vs in out.items()}}), flush=True)
    return 0


def mmm(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


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
                if m == "update" and rnd > 0:      # its windows alternate inside one process
                    continue
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", m, str(N)], capture_output=True, text=True, timeout=o.timeout)
                if r.returncode != 0:                       # nothing more is started on the device after a failure
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    print(json.dumps({"N": N, "failed": m, "returncode": r.returncode, "partial": runs}), flush=True)
                    return 1
                line = r.stdout.strip().splitlines()[-1]
                sys.stderr.write(line[:300] + "\n"); sys.stderr.flush()        # progress: a size takes minutes
                runs[m].append(json.loads(line))
        out = {"operator": f"saddle on poisson:{N}", "rows": N ** 3 + (N ** 3 + 1) // 2, "tol": TOL, "omega": 0.6, "rounds": o.rounds, "methods": {}}
        for m in methods:
            if m == "update":
                q = runs[m][0]
                out["update_ms"] = {k: mmm(v) for k, v in q["ms"].items()}
                out["update_TBps"] = {k: round(48 * q["rows"] / (statistics.median(v) * 1e-3) / 1e12, 3) for k, v in q["ms"].items()}
                continue
            s = [q["s"] for q in runs[m]]
            out["methods"][m] = {"it": sorted({q["it"] for q in runs[m]}), "cycle_applications": sorted({q["it"] * CYCLES[m] for q in runs[m]}),
                                 "status": sorted({q["status"] for q in runs[m]}),
                                 "s": mmm(s), "ms_per_it": mmm([1e3 * q["s"] / max(q["it"], 1) for q in runs[m]]),
                                 "true_res": max(q["true_res"] for q in runs[m]), "work_vectors": VECTORS[m], "levels": runs[m][0]["levels"]}
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
