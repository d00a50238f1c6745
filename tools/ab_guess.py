#!/usr/bin/env python3
"""Initial guesses for a sequence of right-hand sides of one operator, three ways in ONE process on the same hierarchy:
  zero      : every solve starts from x = 0
  previous  : every solve starts from the previous solution
  projected : mgs_guess — x0 = the projection onto the span of the last `capacity` solutions (Guess.apply), the solution offered back
              afterwards (Guess.update); ENERGY kind with PCG, RESIDUAL kind with BiCGSTAB
Operator: the 7-point Poisson operator (generated on the device) or the reference's convection-diffusion family csky3d (host-built with
the bundled file's row-sum margin, as bench.py's leg), N³ rows; preconditioner V(1,1), ω = 0.6, device-built hierarchy (--no-hier: none).
Right-hand sides: multigridsolver_amd.synthetic.moving_blob_rhs, steps 0 .. S − 1.
Prints one JSON line: per mode the iterations and seconds of every step (host clock around a synchronised solve; apply and update are
timed apart and NOT included in the solve's seconds), and for the projected mode the cost of apply (with and without the residual
norm) and of update in seconds and in Krylov iterations of the same operator — seconds divided by the seconds per iteration of the
zero-guess solves of this process.  One warm-up solve (graphs, vector pool) precedes everything.
usage: ab_guess.py [--operator poisson|csky3d] [--N 256] [--steps 12] [--solver pcg|bicgstab] [--capacity 8] [--tol 1e-8] [--no-hier]"""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--operator", choices=["poisson", "csky3d"], default="poisson")
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--solver", choices=["pcg", "bicgstab"], default=None)
    ap.add_argument("--capacity", type=int, default=8)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--no-hier", action="store_true")
    o = ap.parse_args()
    solver = o.solver or ("pcg" if o.operator == "poisson" else "bicgstab")
    import multigridsolver_amd as mg
    from multigridsolver_amd.synthetic import csky3d, moving_blob_rhs, CSKY_ROWSUM_MARGIN
    N, n = o.N, o.N ** 3
    ctx = mg.Context(0)
    if o.operator == "poisson":
        A = ctx.poisson3d(N)
    else:
        A = ctx.csr(n, n, *csky3d(N, rowsum_floor=CSKY_ROWSUM_MARGIN))
    A.optimize()
    h = None if o.no_hier else mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 2500, 32).finalize()
    solve = (lambda x, b: mg.pcg(A, x, b, h, 2000, o.tol)) if solver == "pcg" else (lambda x, b: mg.bicgstab(A, x, b, h, 2000, o.tol))
    rhs = [ctx.vec(moving_blob_rhs(N, s)) for s in range(o.steps)]
    x = ctx.vec(n)
    solve(x, rhs[0])                                     # warm-up
    out = {"operator": f"{o.operator}:{N}", "rows": n, "solver": solver + ("" if o.no_hier else "+V(1,1)"), "levels": h.nlev if h else 1, "tol": o.tol,
           "capacity": o.capacity, "steps": o.steps, "modes": {}}
    rc = 0
    for mode in ("zero", "previous", "projected"):
        g = mg.Guess(A, "energy" if solver == "pcg" else "residual", o.capacity) if mode == "projected" else None
        its, secs, t_apply, t_apply_rel, t_update, rels, added = [], [], [], [], [], [], []
        x.fill(0.0)
        for s, b in enumerate(rhs):
            if mode == "zero":
                x.fill(0.0)
            elif mode == "projected":
                ctx.sync(); t0 = time.perf_counter()
                g.apply(b, x)
                ctx.sync(); t_apply.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                _, rel = g.apply(b, x, rel_resid=True)           # the same x0 again, with ‖b − A·x0‖/‖b‖
                t_apply_rel.append(time.perf_counter() - t0); rels.append(rel)
            ctx.sync(); t0 = time.perf_counter()
            st, it, res = solve(x, b)
            ctx.sync(); secs.append(time.perf_counter() - t0)
            its.append(it)
            if st != 0:
                rc = 3
            if g is not None:
                t0 = time.perf_counter()
                added.append(int(g.update(x)))
                t_update.append(time.perf_counter() - t0)
        m = {"iterations": its, "seconds": [round(v, 5) for v in secs], "iterations_total": sum(its), "seconds_total": round(sum(secs), 5),
             "true_residual_last": A.residual(x, rhs[-1]).nrm2() / rhs[-1].nrm2()}
        if g is not None:
            z = out["modes"]["zero"]
            per_it = z["seconds_total"] / max(z["iterations_total"], 1)
            med = lambda v: sorted(v)[len(v) // 2]
            m.update({"rel_resid_of_x0": rels, "added": added, "info": g.info(),
                      "apply_s": [round(v, 6) for v in t_apply], "apply_with_rel_resid_s": [round(v, 6) for v in t_apply_rel], "update_s": [round(v, 6) for v in t_update],
                      "zero_guess_seconds_per_iteration": per_it,
                      "apply_in_iterations_median": med(t_apply) / per_it, "apply_with_rel_resid_in_iterations_median": med(t_apply_rel) / per_it,
                      "update_in_iterations_median": med(t_update) / per_it,
                      "seconds_total_with_apply_and_update": round(sum(secs) + sum(t_apply) + sum(t_update), 5)})
        out["modes"][mode] = m
    print(json.dumps(out), flush=True)
    ctx.close()
    return rc


if __name__ == "__main__":
    sys.exit(main())
