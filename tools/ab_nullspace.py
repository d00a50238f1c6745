#!/usr/bin/env python3
"""What the declared constant null space costs: PCG + V(1,1) to 1e-10 (ω = 0.6, device-built hierarchy) on the N³ 7-point NEUMANN Laplacian
(singular; Csr.set_nullspace("constant"): regularised coarsest solve, projected PCG) against the same solve of the DIRICHLET operator of the
same size, which takes the undeclared path — with --parent-tree <checkout of the parent commit with its libmgs.so built> solved by that
checkout's package and library, so that the comparison is against the code as it stood (the package is imported from there; MGS_LIBMGS
alone does not do: the parent's library lacks the symbols this package resolves at load).
  neumann   : the operator is assembled ON THE DEVICE from COO triples (Csr.from_coo_device): for every grid edge {i, j} the four triples
              (i, j, −1), (j, i, −1), (i, i, 1), (j, j, 1); the duplicates on the diagonal sum to the number of neighbours
  dirichlet : mgs_csr_poisson3d
  project   : the two projection launches alone (sum pass + fold + shift pass; mgs_vec_project_const without a read-back) on a vector of N³
              entries, HIP events on the context's stream around --reps back-to-back calls: the cost one projection adds to an iteration
Every measurement is a FRESH process (setup, one warm-up solve that captures the graphs and fills the vector pool, one timed solve: host clock
around a synchronised solve) with a device-memory arena (MGS_ARENA_GB), the cases alternating round by round so that drift of the machine
hits them alike.  One JSON line per size.  Stops at the first child that fails.
usage: ab_nullspace.py [256] [--rounds 3] [--arena-gb 48] [--parent-tree DIR] [--timeout 600]
       ab_nullspace.py --child neumann|dirichlet|project N [--tree DIR]"""
import argparse, json, os, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

TOL = 1e-10


def neumann_coo(torch, N, dev):
    """→ (row, col, val) device tensors (int32, int32, float64) of the N³ Neumann Laplacian's triples, four per grid edge"""
    idx = torch.arange(N ** 3, dtype=torch.int32, device=dev).reshape(N, N, N)
    rows, cols, vals = [], [], []
    for ax in range(3):
        lo = idx.narrow(ax, 0, N - 1).reshape(-1); hi = idx.narrow(ax, 1, N - 1).reshape(-1)
        rows += [lo, hi, lo, hi]; cols += [hi, lo, lo, hi]
        m = torch.full((lo.numel(),), -1.0, dtype=torch.float64, device=dev)
        vals += [m, m, -m, -m]
    return torch.cat(rows).contiguous(), torch.cat(cols).contiguous(), torch.cat(vals).contiguous()


def child(case, N, reps, tree):
    import torch                                   # before libmgs.so: the first HIP runtime loaded serves the process
    if tree:
        sys.path.insert(0, os.path.abspath(tree))
    import multigridsolver_amd as mg
    ctx = mg.Context(0)
    n = N ** 3
    out = {"case": case, "N": N, "lib": mg.SO_PATH, "arena_gb": os.environ.get("MGS_ARENA_GB")}
    if case == "project":
        v = ctx.vec(n).rand(seed=2)
        stream = torch.cuda.ExternalStream(ctx.stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        from multigridsolver_amd._lib import check
        call = lambda: check(mg.lib().mgs_vec_project_const(v.h, None, None), ctx.h)
        call(); ctx.sync()
        e0.record(stream)
        for _ in range(reps):
            call()
        e1.record(stream); ctx.sync()
        ms = e0.elapsed_time(e1) / reps
        out.update({"reps": reps, "ms_per_projection": round(ms, 5), "bytes_per_row": 24, "TBps": round(24.0 * n / (ms * 1e-3) / 1e12, 3), "mean_after": v.project_const()})
        print(json.dumps(out), flush=True)
        ctx.close()
        return 0
    if case == "neumann":
        dev = torch.device("cuda:0")
        r, c, w = neumann_coo(torch, N, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        A = mg.Csr.from_coo_device(ctx, n, n, r, c, w)
        out["assemble_s"] = round(time.perf_counter() - t0, 4); out["triples"] = int(r.numel())
        del r, c, w
        torch.cuda.empty_cache()
        A.set_nullspace("constant")
        out["defect"] = A.nullspace_defect()
    else:
        A = ctx.poisson3d(N)
    A.optimize()
    out["nnz"] = A.nnz
    ctx.sync(); t0 = time.perf_counter()
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 2500, 32).finalize()
    ctx.sync(); out["setup_s"] = round(time.perf_counter() - t0, 4)
    b = ctx.vec(n).rand(seed=0)
    x = ctx.vec(n)
    mg.pcg(A, x, b, h, 1000, TOL)                  # warm-up
    x.fill(0.0); ctx.sync(); t0 = time.perf_counter()
    st, it, res = mg.pcg(A, x, b, h, 1000, TOL)
    ctx.sync(); dt = time.perf_counter() - t0
    r_ = A.residual(x, b)
    if case == "neumann":
        _, true = r_.project_const(nrm2=True)      # Π(b − A·x) against ‖Πb‖
        _, nb = b.project_const(nrm2=True)
        out["mean_x"] = x.project_const()
    else:
        true, nb = r_.nrm2(), b.nrm2()
    out.update({"levels": h.nlev, "status": st, "it": it, "s": round(dt, 4), "ms_per_it": round(1e3 * dt / max(it, 1), 4), "reported": res, "true_res": true / nb})
    print(json.dumps(out), flush=True)
    ctx.close()
    return 0 if st == 0 else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50, help="projections between the two events of the `project` case")
    ap.add_argument("--arena-gb", type=int, default=48)
    ap.add_argument("--parent-tree", default=None, help="checkout of the parent commit, library built, for the dirichlet case (default: this tree)")
    ap.add_argument("--tree", default=None, help="(child) import the package from this checkout")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", nargs=2, default=None)
    o = ap.parse_args()
    if o.child:
        return child(o.child[0], int(o.child[1]), o.reps, o.tree)
    cases = ["dirichlet", "neumann", "project"]
    for N in o.sizes:
        runs = {c: [] for c in cases}
        for _ in range(o.rounds):
            for c in cases:
                env = dict(os.environ, MGS_ARENA_GB=str(o.arena_gb))
                cmd = [sys.executable, os.path.abspath(__file__), "--child", c, str(N), "--reps", str(o.reps)]
                if c == "dirichlet" and o.parent_tree:
                    cmd += ["--tree", o.parent_tree]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=o.timeout, env=env)
                if r.returncode != 0:                       # nothing more is started on the device after a failure
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    print(json.dumps({"N": N, "failed": c, "returncode": r.returncode, "partial": runs}), flush=True)
                    return 1
                runs[c].append(json.loads(r.stdout.strip().splitlines()[-1]))
        out = {"rows": N ** 3, "tol": TOL, "omega": 0.6, "rounds": o.rounds, "arena_gb": o.arena_gb}
        for c in ("dirichlet", "neumann"):
            q = runs[c]
            out[c] = {"lib": q[0]["lib"], "levels": q[0]["levels"], "it": sorted({k["it"] for k in q}), "s": [k["s"] for k in q], "s_min": min(k["s"] for k in q),
                      "s_max": max(k["s"] for k in q), "ms_per_it": [k["ms_per_it"] for k in q], "setup_s": [k["setup_s"] for k in q],
                      "true_res": max(k["true_res"] for k in q)}
        out["neumann"].update({"assemble_s": [k["assemble_s"] for k in runs["neumann"]], "triples": runs["neumann"][0]["triples"],
                               "defect": runs["neumann"][0]["defect"], "mean_x": [k["mean_x"] for k in runs["neumann"]]})
        out["project"] = {"ms_per_projection": [k["ms_per_projection"] for k in runs["project"]], "TBps": [k["TBps"] for k in runs["project"]],
                          "reps": o.reps}
        # PCG projects z once per iteration: what the two launches add to an iteration, from the events
        pm = min(out["project"]["ms_per_projection"])
        out["projection_share_of_neumann_iteration"] = round(pm / min(out["neumann"]["ms_per_it"]), 4)
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
