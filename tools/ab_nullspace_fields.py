#!/usr/bin/env python3
"""What the field-wise constant null space (Csr.set_nullspace_fields) costs.
  project : the projection launches alone (sum pass + fold + shift pass, no read-back) on a vector of N³ entries, HIP events on the
            context's stream around --reps back-to-back calls, in ONE process per round for the four variants so that they see the same
            machine: project_const (mgs_vec_project_const, the kernel the constant kind has always used), project_fields with 1 field over
            all rows, with 8 fields (label = row mod 8), with the saddle layout (−1 on the first 3/4 of the rows, one field on the rest), and
            a device-to-device copy that moves 24 B per row (12 read, 12 written)
  stokes  : MINRES + V(1,1) to 1e-8 (ω = 0.6, device-built hierarchy of block_diag(L, S)) on enclosed_stokes built from Poisson N³ — L three
            copies of mgs_csr_poisson3d, D from synthetic.stokes_divergence, K and S assembled on the device, labels −1 / 0
  saddle  : the same solver on the README's REGULAR saddle system (tools/ab_minres.py: D every second row of I − shift, C = 1e-2·I) at the
            size whose row count is nearest to 4·N³ — with --parent-tree <checkout of the parent commit with its libmgs.so built> solved by that
            checkout's package and library, so that the comparison is against the code as it stood
Every measurement is a FRESH process (setup, one warm-up solve that captures the graphs and fills the vector pool, one timed solve: host clock
around a synchronised solve), the cases alternating round by round.  One JSON line per size, medians with min-max.  Nothing here is a
pass/fail bar.  Stops at the first child that fails.
usage: ab_nullspace_fields.py [128] [--rounds 3] [--cases project,stokes,saddle] [--parent-tree DIR] [--timeout 600]
       ab_nullspace_fields.py --child project|stokes|saddle N [--tree DIR]"""
import argparse, json, os, statistics, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOL = 1e-8
CASES = ["project", "stokes", "saddle"]


def saddle_size(N):
    """the N' whose regular saddle system (N'³ + N'³/2 rows) has the row count nearest to 4·N³"""
    return round((8.0 / 3.0) ** (1.0 / 3.0) * N)


def project(mg, ctx, N, reps):
    import numpy as np
    import torch
    from multigridsolver_amd._lib import check
    n = N ** 3
    lib = mg.lib()
    ident = lambda: mg.Csr.from_diag(ctx, ctx.vec(np.ones(n)))      # noqa: E731  an n-row handle that carries the labels
    i = np.arange(n)
    A1 = ident().set_nullspace_fields(np.zeros(n, dtype=np.int64))
    A8 = ident().set_nullspace_fields((i % 8).astype(np.int64))
    As = ident().set_nullspace_fields(np.where(i < 3 * (n // 4), -1, 0).astype(np.int64))
    v = ctx.vec(n).rand(seed=2)
    src, dst = ctx.vec(n + n // 2).rand(seed=5), ctx.vec(n + n // 2)
    stream = torch.cuda.ExternalStream(ctx.stream)
    calls = {"project_const": lambda: check(lib.mgs_vec_project_const(v.h, None, None), ctx.h),
             "project_fields_1": lambda: check(lib.mgs_vec_project_fields(v.h, A1.h, None, None), ctx.h),
             "project_fields_8": lambda: check(lib.mgs_vec_project_fields(v.h, A8.h, None, None), ctx.h),
             "project_fields_saddle": lambda: check(lib.mgs_vec_project_fields(v.h, As.h, None, None), ctx.h),
             "copy_24B": lambda: dst.copy_from(src)}
    ms = {k: [] for k in calls}
    for call in calls.values():
        call()
    ctx.sync()
    for _ in range(5):                                                # windows, the variants alternating
        for k, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                call()
            e1.record(stream); ctx.sync()
            ms[k].append(e0.elapsed_time(e1) / reps)
    print(json.dumps({"case": "project", "N": N, "rows": n, "reps": reps, "ms": {k: [round(x, 5) for x in q] for k, q in ms.items()}}), flush=True)
    return 0


def stokes(mg, ctx, N):
    """→ (K, hierarchy, rows): enclosed_stokes from Poisson N³, assembled on the device, both matrices declared"""
    import numpy as np
    from multigridsolver_amd.synthetic import stokes_divergence
    m = N ** 3
    P = ctx.poisson3d(N)
    L = mg.Csr.block_diag(ctx, [P, P, P])
    rp, ci, v = stokes_divergence(N)
    D = ctx.csr(m, 3 * m, rp, ci, v)
    lab = np.r_[np.full(3 * m, -1), np.zeros(m)].astype(np.int64)
    K = mg.Csr.bmat(ctx, [[L, D.transpose()], [D, None]]).optimize().set_nullspace_fields(lab)
    S = D @ D.transpose().scale(left=L.diag_inv())
    B = mg.Csr.block_diag(ctx, [L, S]).set_nullspace_fields(lab)
    h = mg.Hierarchy(B, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 2500, 32).finalize()
    return K, h, 4 * m, lab


def solve(mg, ctx, case, N):
    import numpy as np
    if case == "stokes":
        K, h, rows, lab = stokes(mg, ctx, N)
    else:
        sys.path.insert(0, os.path.join(REPO, "tools"))
        import ab_minres
        Ns = saddle_size(N)
        K, h, rows = ab_minres.saddle(mg, ctx, Ns)
    b = ctx.vec(rows).rand(seed=0)
    x = ctx.vec(rows)
    mg.minres(K, x, b, h, 2000, TOL)              # warm-up
    x.fill(0.0); ctx.sync(); t0 = time.perf_counter()
    st, it, res = mg.minres(K, x, b, h, 2000, TOL)
    ctx.sync(); dt = time.perf_counter() - t0
    r = K.residual(x, b)
    if case == "stokes":
        _, true = r.project_fields(K, nrm2=True)
        bb = ctx.vec(rows).rand(seed=0); _, nb = bb.project_fields(K, nrm2=True)
        xp = x.numpy()[lab == 0]
        extra = {"pressure_mean": float(xp.mean()), "defect": K.nullspace_defect()}
    else:
        true, nb, extra = r.nrm2(), b.nrm2(), {"N_saddle": saddle_size(N)}
    out = {"case": case, "N": N, "rows": rows, "lib": mg.SO_PATH, "levels": h.nlev, "status": st, "it": it, "s": round(dt, 5),
           "ms_per_it": round(1e3 * dt / max(it, 1), 4), "ns_per_row_it": round(1e9 * dt / max(it, 1) / rows, 4), "reported": res, "true_res": true / nb}
    out.update(extra)
    print(json.dumps(out), flush=True)
    return 0


def child(case, N, reps, tree):
    import torch  # noqa: F401                      before libmgs.so: the first HIP runtime loaded serves the process
    sys.path.insert(0, os.path.abspath(tree) if tree else REPO)
    import multigridsolver_amd as mg
    ctx = mg.Context(0)
    try:
        return project(mg, ctx, N, reps) if case == "project" else solve(mg, ctx, case, N)
    finally:
        ctx.close()


def mmm(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[128])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50, help="projections between the two events of the `project` case")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--parent-tree", default=None, help="checkout of the parent commit, library built, for the saddle case (default: this tree)")
    ap.add_argument("--tree", default=None, help="(child) import the package from this checkout")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", nargs=2, default=None)
    o = ap.parse_args()
    if o.child:
        return child(o.child[0], int(o.child[1]), o.reps, o.tree)
    cases = o.cases.split(",")
    for N in o.sizes:
        runs = {c: [] for c in cases}
        for _ in range(o.rounds):
            for c in cases:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", c, str(N), "--reps", str(o.reps)]
                if c == "saddle" and o.parent_tree:
                    cmd += ["--tree", o.parent_tree]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=o.timeout)
                if r.returncode != 0:                       # nothing more is started on the device after a failure
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    print(json.dumps({"N": N, "failed": c, "returncode": r.returncode, "partial": runs}), flush=True)
                    return 1
                runs[c].append(json.loads(r.stdout.strip().splitlines()[-1]))
        out = {"N": N, "tol": TOL, "omega": 0.6, "rounds": o.rounds}
        if "project" in runs:
            keys = runs["project"][0]["ms"].keys()
            out["project"] = {"rows": N ** 3, "ms": {k: mmm([x for q in runs["project"] for x in q["ms"][k]]) for k in keys}}
            pc = out["project"]["ms"]["project_const"]["median"]
            out["project"]["ratio_to_project_const"] = {k: round(out["project"]["ms"][k]["median"] / pc, 4) for k in keys}
        for c in ("stokes", "saddle"):
            if c in runs:
                q = runs[c]
                out[c] = {"lib": q[0]["lib"], "rows": q[0]["rows"], "levels": q[0]["levels"], "status": sorted({k["status"] for k in q}), "it": sorted({k["it"] for k in q}),
                          "s": mmm([k["s"] for k in q]), "ms_per_it": mmm([k["ms_per_it"] for k in q]), "ns_per_row_it": mmm([k["ns_per_row_it"] for k in q]),
                          "true_res": max(k["true_res"] for k in q)}
                for extra in ("pressure_mean", "defect", "N_saddle"):
                    if extra in q[0]:
                        out[c][extra] = q[0][extra]
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
