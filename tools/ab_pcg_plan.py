#!/usr/bin/env python3
"""mgs_pcg against the PCG plan (mgs_pcg_plan: scalars on the device) on the 7-point Poisson operator at N³ rows and on the reference's
2-D generator poisson2d(1000) (`2d1000`), to 1e-10 (ω = 0.6, V(1,1), device-built hierarchy):
  pcg       : mgs_pcg — three host looks per iteration; the baseline every other row is held against
  plan_aK   : PcgPlan.solve(ahead = K), K in 0 1 2 4 8 — one host look per iteration, K iterations behind the queue
  enqueue   : PcgPlan.enqueue(iters = the count mgs_pcg needed) + result() — no host look; also the host time enqueue itself takes
Every measurement is a FRESH process (setup, one warm-up solve that captures the graph, one timed solve: host clock around a synchronised
solve), the methods alternating round by round so that drift of the machine hits all of them alike.  Prints one JSON line per operator:
per method iterations, seconds (every repeat, min, max), iterations enqueued / run frozen, host waits, and each method's min over the
baseline's min beside the baseline's own spread (max/min).  Stops at the first child that fails.
usage: ab_pcg_plan.py [512 256 128 64 2d1000] [--rounds 3] [--methods pcg,plan_a0,...] [--timeout 240]
       ab_pcg_plan.py --child METHOD SIZE
       ab_pcg_plan.py --report LINES.jsonl     (the JSON lines of earlier runs → the markdown table of profiles/r12_pcg_plan.md on stdout)"""
import argparse, json, os, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

AHEADS = [0, 1, 2, 4, 8]
METHODS = ["pcg"] + [f"plan_a{k}" for k in AHEADS] + ["enqueue"]
TOL, MAXIT = 1e-10, 1000


def child(method, size):
    import multigridsolver_amd as mg
    ctx = mg.Context(0)
    if size.startswith("2d"):
        m = int(size[2:]); n = m * m
        A = ctx.poisson2d(m).optimize()
    else:
        N = int(size); n = N ** 3
        A = ctx.poisson3d(N).optimize()
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 2500, 32).finalize()
    b = ctx.vec(n).rand(seed=0)
    x = ctx.vec(n)
    out = {"method": method, "size": size, "rows": n, "levels": h.nlev}
    plan = None
    if method == "pcg":
        mg.pcg(A, x, b, h, MAXIT, TOL)                                 # warm-up
        x.fill(0.0); ctx.sync(); t0 = time.perf_counter()
        st, it, res = mg.pcg(A, x, b, h, MAXIT, TOL)
        ctx.sync(); dt = time.perf_counter() - t0
        out.update(enqueued=it, frozen=0, waits=3 * it + 2)            # r·z, p·q, ‖r‖ per iteration; ‖b‖ and the first residual
    elif method.startswith("plan_a"):
        ahead = int(method[6:])
        plan = mg.PcgPlan(A, h)
        plan.solve(x, b, MAXIT, TOL, ahead)
        x.fill(0.0); ctx.sync(); t0 = time.perf_counter()
        st, it, res = plan.solve(x, b, MAXIT, TOL, ahead)
        ctx.sync(); dt = time.perf_counter() - t0
        info = plan.info()
        out.update(enqueued=info[2], frozen=info[3], waits=info[4], restarts=info[5])
    else:
        st0, count, _ = mg.pcg(A, x, b, h, MAXIT, TOL)                 # the count, and the warm-up of the operands
        plan = mg.PcgPlan(A, h)
        x.fill(0.0); plan.enqueue(x, b, count, TOL).result()
        x.fill(0.0); ctx.sync(); t0 = time.perf_counter()
        plan.enqueue(x, b, count, TOL)
        t1 = time.perf_counter()
        st, it, res = plan.result()
        dt = time.perf_counter() - t0
        info = plan.info()
        out.update(enqueued=info[2], frozen=info[3], waits=info[4], enqueue_host_s=round(t1 - t0, 5))
    true = A.residual(x, b).nrm2() / b.nrm2()
    out.update(status=st, it=it, s=round(dt, 5), reported=res, true_res=true)
    print(json.dumps(out), flush=True)
    if plan is not None:
        plan.close()
    ctx.close()
    return 0 if st == 0 else 3


def report(path):
    print("| operator | rows | method | iterations | seconds min–max (3 fresh processes) | min / mgs_pcg min | enqueued | ran frozen | host waits |")
    print("|---|---|---|---|---|---|---|---|---|")
    spreads = []
    for line in open(path):
        if not line.strip().startswith("{"):
            continue
        o = json.loads(line)
        if "methods" not in o:
            continue
        base = o["methods"]["pcg"]
        spreads.append((o["operator"], base["s_max"] / base["s_min"]))
        for m, q in o["methods"].items():
            extra = f"; enqueue() itself {min(q['enqueue_host_s']):.4f} s of host time" if "enqueue_host_s" in q else ""
            print(f"| {o['operator']} | {o['rows']} | `{m}` | {'/'.join(map(str, q['it']))} | {q['s_min']:.4f}–{q['s_max']:.4f}{extra} | {q['s_min'] / base['s_min']:.3f} | "
                  f"{'/'.join(map(str, q['enqueued']))} | {'/'.join(map(str, q['frozen']))} | {'/'.join(map(str, q['waits']))} |")
    print()
    for op, s in spreads:
        print(f"* {op}: spread of `pcg` itself (max/min of its three processes) {s:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", default=["512", "256", "128", "64", "2d1000"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--methods", default=",".join(METHODS))
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", nargs=2, default=None)
    ap.add_argument("--report", default=None)
    o = ap.parse_args()
    if o.child:
        return child(o.child[0], o.child[1])
    if o.report:
        return report(o.report)
    methods = o.methods.split(",")
    for size in o.sizes:
        runs = {m: [] for m in methods}
        for _ in range(o.rounds):
            for m in methods:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", m, size], capture_output=True, text=True, timeout=o.timeout)
                if r.returncode != 0:                       # nothing more is started on the device after a failure
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    print(json.dumps({"size": size, "failed": m, "returncode": r.returncode, "partial": runs}), flush=True)
                    return 1
                runs[m].append(json.loads(r.stdout.strip().splitlines()[-1]))
        first = runs[methods[0]][0]
        out = {"operator": f"poisson:{size}", "rows": first["rows"], "levels": first["levels"], "tol": TOL, "omega": 0.6, "rounds": o.rounds, "methods": {}}
        for m in methods:
            s = [q["s"] for q in runs[m]]
            out["methods"][m] = {"it": sorted({q["it"] for q in runs[m]}), "s": s, "s_min": min(s), "s_max": max(s), "true_res": max(q["true_res"] for q in runs[m]),
                                 "enqueued": sorted({q["enqueued"] for q in runs[m]}), "frozen": sorted({q["frozen"] for q in runs[m]}),
                                 "waits": sorted({q["waits"] for q in runs[m]})}
            if "enqueue_host_s" in runs[m][0]:
                out["methods"][m]["enqueue_host_s"] = [q["enqueue_host_s"] for q in runs[m]]
        if "pcg" in runs:
            base = out["methods"]["pcg"]
            out["pcg_spread_max_over_min"] = round(base["s_max"] / base["s_min"], 4)
            out["min_over_pcg_min"] = {m: round(out["methods"][m]["s_min"] / base["s_min"], 4) for m in methods}
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
