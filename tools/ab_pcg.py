#!/usr/bin/env python3
"""PCG against the solvers the library already had, on the 7-point Poisson operator to 1e-10 (ω = 0.6, device-built hierarchy):
  bicgstab_v : BiCGSTAB + V(1,1)                      pcg_v  : PCG + V(1,1)
  fgcr_k4    : FGCR(10) + K-cycle(4 levels, energy)   fpcg_k4: flexible PCG + K-cycle(4 levels, energy)
Every measurement is a FRESH process (setup, one warm-up solve that captures the graphs and fills the vector pool, one timed solve:
host clock around a synchronised solve), the methods alternating round by round so that drift of the machine hits all of them
alike.  Prints one JSON line per size: per method iterations, cycle applications, seconds (every repeat, min, max), true residual,
work vectors held, and the ratio pcg_v / bicgstab_v.  Stops at the first child that fails.
usage: ab_pcg.py [512 256] [--rounds 3] [--methods bicgstab_v,pcg_v,fgcr_k4,fpcg_k4] [--timeout 240]
       ab_pcg.py --child METHOD[+METHOD] N [--eager]     (one measurement per method, in ONE process: `--child pcg_v+bicgstab_v 512 --eager` is the
       run to put under `rocprofv3 --kernel-trace --stats`: the two new kernels and their neighbour update_dot2_partial_vec_kernel in the same
       trace.  --eager: option graph = 0 — rocprofv3 7.2 crashes in its hook for hipGraph capture when torch is not loaded first, see tools/fgcr_trace.py)"""
import argparse, json, os, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

METHODS = ["bicgstab_v", "pcg_v", "fgcr_k4", "fpcg_k4"]
# work vectors of the operator's size a solve holds (krylov.hip): BiCGSTAB p p̂ s ŝ t v r r̃; FGCR(10) r + 10 × (c, v); PCG r z p q
VECTORS = {"bicgstab_v": 8, "pcg_v": 4, "fgcr_k4": 21, "fpcg_k4": 4}
# cycle applications per iteration
CYCLES = {"bicgstab_v": 2, "pcg_v": 1, "fgcr_k4": 1, "fpcg_k4": 1}


def child(methods, N, eager):
    import multigridsolver_amd as mg
    ctx = mg.Context(0)
    if eager:
        ctx.set_option("graph", 0)
    n = N ** 3
    A = ctx.poisson3d(N).optimize()
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 2500, 32).finalize()
    b = ctx.vec(n).rand(seed=0)
    rc = 0
    for method in methods.split("+"):
        k = 4 if method.endswith("_k4") else 0
        h.set_kcycle(k); ctx.set_option("kcycle_energy", int(k > 0))
        rc = max(rc, one(mg, ctx, A, h, b, n, N, method))
    ctx.close()
    return rc


def one(mg, ctx, A, h, b, n, N, method):
    solve = {"bicgstab_v": lambda x: mg.bicgstab(A, x, b, h, 1000, 1e-10),
             "pcg_v": lambda x: mg.pcg(A, x, b, h, 1000, 1e-10, False),
             "fgcr_k4": lambda x: mg.fgcr(A, x, b, h, 10, 1000, 1e-10),
             "fpcg_k4": lambda x: mg.pcg(A, x, b, h, 1000, 1e-10, True)}[method]
    x = ctx.vec(n)
    solve(x)                                     # warm-up
    x.fill(0.0); ctx.sync(); t0 = time.perf_counter()
    st, it, res = solve(x)
    ctx.sync(); dt = time.perf_counter() - t0
    true = A.residual(x, b).nrm2() / b.nrm2()
    print(json.dumps({"method": method, "N": N, "levels": h.nlev, "status": st, "it": it, "s": round(dt, 4), "reported": res, "true_res": true}), flush=True)
    return 0 if st == 0 else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[512, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--methods", default=",".join(METHODS))
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", nargs=2, default=None)
    ap.add_argument("--eager", action="store_true")
    o = ap.parse_args()
    if o.child:
        return child(o.child[0], int(o.child[1]), o.eager)
    methods = o.methods.split(",")
    for N in o.sizes:
        runs = {m: [] for m in methods}
        for _ in range(o.rounds):
            for m in methods:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", m, str(N)], capture_output=True, text=True, timeout=o.timeout)
                if r.returncode != 0:                       # nothing more is started on the device after a failure
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    print(json.dumps({"N": N, "failed": m, "returncode": r.returncode, "partial": runs}), flush=True)
                    return 1
                runs[m].append(json.loads(r.stdout.strip().splitlines()[-1]))
        out = {"operator": f"poisson:{N}", "rows": N ** 3, "tol": 1e-10, "omega": 0.6, "rounds": o.rounds, "methods": {}}
        for m in methods:
            s = [q["s"] for q in runs[m]]
            out["methods"][m] = {"it": sorted({q["it"] for q in runs[m]}), "cycle_applications": sorted({q["it"] * CYCLES[m] for q in runs[m]}),
                                 "s": s, "s_min": min(s), "s_max": max(s), "true_res": max(q["true_res"] for q in runs[m]),
                                 "work_vectors": VECTORS[m], "levels": runs[m][0]["levels"]}
        if "pcg_v" in runs and "bicgstab_v" in runs:
            p, q = out["methods"]["pcg_v"], out["methods"]["bicgstab_v"]
            out["pcg_v_over_bicgstab_v"] = {"min_over_min": round(p["s_min"] / q["s_min"], 4), "lowest": round(p["s_min"] / q["s_max"], 4),
                                            "highest": round(p["s_max"] / q["s_min"], 4)}
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
