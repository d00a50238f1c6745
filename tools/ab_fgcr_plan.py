#!/usr/bin/env python3
"""mgs_fgcr against the FGCR plan (mgs_fgcr_plan: coefficients on the device), FGCR(10) to 1e-8 (ω = 0.6, device-built hierarchy), on
  csky256 : csky3d(256, rowsum_floor = CSKY_ROWSUM_MARGIN), K-cycle on all levels below the finest, GCR form
  256     : the 7-point Poisson operator at 256³, K-cycle on 4 levels, energy form
with the methods
  fgcr      : mgs_fgcr — three host looks per iteration; the baseline every other row is held against
  plan_aK   : FgcrPlan.solve(ahead = K), K in 0 1 4 — one host look per iteration, K iterations behind the queue
  enqueue   : FgcrPlan.enqueue(iters = the count mgs_fgcr needed) + result() — no host look; also the host time enqueue itself takes
One fresh process per operator (csky3d is built on the host, which takes longer than every solve together): setup, one warm-up solve per
method (operands, captured cycles), then `--rounds` rounds in which the methods ALTERNATE, each timed with the host clock around a
synchronised solve from x = 0 — so drift of the machine hits all of them alike, and the baseline's own spread over the rounds stands beside
every ratio.  Every solve must return mgs_fgcr's iteration count and residual (the plan promises its bits).  Prints one JSON line per
operator.  Stops at the first child that fails.
usage: ab_fgcr_plan.py [csky256 256] [--rounds 5] [--methods fgcr,plan_a0,...] [--timeout 900]
       ab_fgcr_plan.py --child OPERATOR
       ab_fgcr_plan.py --report LINES.jsonl     (the JSON lines of earlier runs → the markdown table of profiles/r14_fgcr_plan.md on stdout)"""
import argparse, json, os, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

AHEADS = [0, 1, 4]
METHODS = ["fgcr"] + [f"plan_a{k}" for k in AHEADS] + ["enqueue"]
TOL, MAXIT, RESTART = 1e-8, 1000, 10


def child(op, methods, rounds):
    import multigridsolver_amd as mg
    ctx = mg.Context(0)
    if op.startswith("csky"):
        from multigridsolver_amd.synthetic import csky3d, CSKY_ROWSUM_MARGIN
        N = int(op[4:]); n = N ** 3
        A = ctx.csr(n, n, *csky3d(N, rowsum_floor=CSKY_ROWSUM_MARGIN)).optimize()
    else:
        N = int(op); n = N ** 3
        A = ctx.poisson3d(N).optimize()
        ctx.set_option("kcycle_energy", 1)
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 2500, 32).finalize()
    klev = max(h.nlev - 2, 1) if op.startswith("csky") else min(4, max(h.nlev - 2, 1))
    h.set_kcycle(klev)
    b = ctx.vec(n).rand(seed=0)
    x = ctx.vec(n)
    want = mg.fgcr(A, x, b, h, RESTART, MAXIT, TOL)                       # the count, the residual, and the warm-up of the baseline
    if want[0] != 0:
        print(json.dumps({"operator": op, "failed": "fgcr", "returned": want}), flush=True)
        return 3
    count = want[1]
    plan = mg.FgcrPlan(A, h, RESTART) if any(m != "fgcr" for m in methods) else None

    def run(m):
        """→ (seconds, (status, iterations, residual), extra)"""
        x.fill(0.0); ctx.sync(); t0 = time.perf_counter()
        if m == "fgcr":
            r = mg.fgcr(A, x, b, h, RESTART, MAXIT, TOL)
            ctx.sync(); dt = time.perf_counter() - t0
            # h_j (not at k = 0), (ρ_k, t) and ‖r‖² per iteration, a true residual per window (which makes up for the h_j of its k = 0); ‖b‖ and the first residual
            return dt, r, {"enqueued": r[1], "frozen": 0, "waits": 3 * r[1] + 2}
        if m.startswith("plan_a"):
            r = plan.solve(x, b, MAXIT, TOL, int(m[6:]))
            ctx.sync(); dt = time.perf_counter() - t0
            info = plan.info()
            return dt, r, {"enqueued": info[2], "frozen": info[3], "waits": info[4], "restarts": info[5]}
        plan.enqueue(x, b, count, TOL)
        t1 = time.perf_counter()
        st, it, true_res, rec = plan.result(recursive=True)
        dt = time.perf_counter() - t0
        info = plan.info()
        return dt, (st, it, true_res), {"enqueued": info[2], "frozen": info[3], "waits": info[4], "enqueue_host_s": round(t1 - t0, 5)}

    out = {"operator": op, "rows": n, "levels": h.nlev, "kcycle_levels": klev, "tol": TOL, "omega": 0.6, "restart": RESTART, "rounds": rounds, "it": count,
           "reported": want[2], "methods": {m: {"s": []} for m in methods}}
    for m in methods:                                                       # warm-up
        run(m)
    for _ in range(rounds):
        for m in methods:
            dt, r, extra = run(m)
            if tuple(r) != tuple(want):                                      # status, count and residual: the plan promises mgs_fgcr's bits
                print(json.dumps({"operator": op, "failed": m, "returned": r, "mgs_fgcr": want}), flush=True)
                return 3
            q = out["methods"][m]
            q["s"].append(round(dt, 5))
            for k, v in extra.items():
                q.setdefault(k, []).append(v)
    out["true_res"] = A.residual(x, b).nrm2() / b.nrm2()
    for m in methods:
        q = out["methods"][m]
        q["s_min"], q["s_max"] = min(q["s"]), max(q["s"])
        for k in ("enqueued", "frozen", "waits"):
            q[k] = sorted(set(q[k]))
    if "fgcr" in methods:
        base = out["methods"]["fgcr"]
        out["fgcr_spread_max_over_min"] = round(base["s_max"] / base["s_min"], 4)
        out["min_over_fgcr_min"] = {m: round(out["methods"][m]["s_min"] / base["s_min"], 4) for m in methods}
    print(json.dumps(out), flush=True)
    if plan is not None:
        plan.close()
    ctx.close()
    return 0


def report(path):
    print("| operator | rows | method | iterations | seconds min–max over the rounds | ms per iteration (min) | min / mgs_fgcr min | enqueued | ran frozen | host waits |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    spreads = []
    for line in open(path):
        if not line.strip().startswith("{"):
            continue
        o = json.loads(line)
        if "methods" not in o:
            continue
        base = o["methods"]["fgcr"]
        spreads.append((o["operator"], o["rounds"], base["s_max"] / base["s_min"]))
        for m, q in o["methods"].items():
            extra = f"; enqueue() itself {min(q['enqueue_host_s']):.4f} s of host time" if "enqueue_host_s" in q else ""
            print(f"| {o['operator']} | {o['rows']} | `{m}` | {o['it']} | {q['s_min']:.4f}–{q['s_max']:.4f}{extra} | {1e3 * q['s_min'] / o['it']:.3f} | {q['s_min'] / base['s_min']:.3f} | "
                  f"{'/'.join(map(str, q['enqueued']))} | {'/'.join(map(str, q['frozen']))} | {'/'.join(map(str, q['waits']))} |")
    print()
    for op, rounds, s in spreads:
        print(f"* {op}: spread of `fgcr` itself (max/min of its {rounds} rounds) {s:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("operators", nargs="*", default=["csky256", "256"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--methods", default=",".join(METHODS))
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--child", default=None)
    ap.add_argument("--report", default=None)
    o = ap.parse_args()
    methods = o.methods.split(",")
    if o.child:
        return child(o.child, methods, o.rounds)
    if o.report:
        return report(o.report)
    for op in o.operators:
        sys.stderr.write(f"[ab_fgcr_plan] {op}: {o.rounds} rounds of {o.methods}\n"); sys.stderr.flush()
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", op, "--rounds", str(o.rounds), "--methods", o.methods],
                           capture_output=True, text=True, timeout=o.timeout)
        sys.stdout.write(r.stdout); sys.stdout.flush()
        if r.returncode != 0:                       # nothing more is started on the device after a failure
            sys.stderr.write(r.stderr[-4000:])
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
