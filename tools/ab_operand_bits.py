#!/usr/bin/env python3
"""Operand precision 64 vs 32 bits (Hierarchy.set_operand_precision) on ONE hierarchy in one process, alternating: V-cycle time
(mgs_time_vcycle), a BiCGSTAB + V solve and an FGCR(10) + K(4, energy) solve to 1e-10 — wall time, iterations, true residual — and the
byte ratio from vcycle_bytes.  Prints one JSON line per operator.
usage: ab_operand_bits.py [poisson:512] [csky3d:256] [--rounds 3] [--reps 20] [--cycles-only] [--eager]
(--eager: option graph = 0, every kernel its own dispatch — the form to run under `rocprofv3 --kernel-trace --stats`, whose per-kernel
table then separates the float and the double instantiations of the pre and post kernels by their names)"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import multigridsolver_amd as mg
from multigridsolver_amd import synthetic

import argparse
ap = argparse.ArgumentParser()
ap.add_argument("cases", nargs="*", default=["poisson:512", "csky3d:256"])
ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--cycles-only", action="store_true"); ap.add_argument("--eager", action="store_true")
opts = ap.parse_args()
rounds, reps, cycles_only, cases = opts.rounds, opts.reps, opts.cycles_only, opts.cases
ctx = mg.Context(0)
if opts.eager:
    ctx.set_option("graph", 0)


def true_residual(A, x, b):
    r = A.residual(x, b)
    return r.nrm2() / b.nrm2()


for case in cases:
    kind, N = case.split(":"); N = int(N); n = N ** 3
    if kind == "poisson":
        A = ctx.poisson3d(N)
    else:
        rp, ci, v = synthetic.csky3d(N, rowsum_floor=synthetic.CSKY_ROWSUM_MARGIN)
        A = ctx.csr(n, n, rp, ci, v); del rp, ci, v
    A.optimize()
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 2500, 32).finalize()
    b = ctx.vec(n).rand(seed=0); x = ctx.vec(n)
    res = {"operator": case, "rows": n, "levels": h.nlev, "rounds": rounds, "reps": reps, "bits": {}}
    for bits in (64, 32):          # warm-up of both forms (operand setup, graph capture)
        h.set_operand_precision(bits)
        for _ in range(3): h.vcycle(b, x)
        res["bits"][bits] = {"levels_switched": [l for l in range(h.nlev) if h.operand_precision(l) == 32], "vcycle_bytes": h.vcycle_bytes,
                             "cycle_ms": [], "bicgstab_v": [], "fgcr_k4": []}
    for _ in range(rounds):
        for bits in (64, 32):
            h.set_operand_precision(bits)
            r = res["bits"][bits]
            h.vcycle(b, x)
            r["cycle_ms"].append(round(min(h.time_vcycle(b, x, reps=reps) for _ in range(3)), 4))
            if cycles_only:
                continue
            h.set_kcycle(0); ctx.set_option("kcycle_energy", 0)
            xs = ctx.vec(n); ctx.sync(); t0 = time.perf_counter()
            st, it, _ = mg.bicgstab(A, xs, b, h, 1000, 1e-10)
            ctx.sync(); r["bicgstab_v"].append({"status": st, "it": it, "s": round(time.perf_counter() - t0, 4), "true_res": true_residual(A, xs, b)})
            h.set_kcycle(4); ctx.set_option("kcycle_energy", 1)
            xs = ctx.vec(n); ctx.sync(); t0 = time.perf_counter()
            st, it, _ = mg.fgcr(A, xs, b, h, 10, 1000, 1e-10)
            ctx.sync(); r["fgcr_k4"].append({"status": st, "it": it, "s": round(time.perf_counter() - t0, 4), "true_res": true_residual(A, xs, b)})
            h.set_kcycle(0); ctx.set_option("kcycle_energy", 0)
    c64, c32 = min(res["bits"][64]["cycle_ms"]), min(res["bits"][32]["cycle_ms"])
    res["cycle_time_ratio_32_over_64"] = round(c32 / c64, 4)
    res["byte_ratio_32_over_64"] = round(res["bits"][32]["vcycle_bytes"] / res["bits"][64]["vcycle_bytes"], 4)
    h.set_operand_precision(64)
    print(json.dumps(res), flush=True)
    del h, A, b, x
    ctx.trim() if hasattr(ctx, "trim") else None
