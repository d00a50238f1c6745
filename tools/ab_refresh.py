#!/usr/bin/env python3
"""What a caller whose matrix VALUES change on a fixed pattern pays per change, two ways, on Poisson 512³ and csky3d 256³ (ω = 0.6, device
aggregation 10 / 2 / 8):
  rebuild : mgs_hier_coarsen + mgs_hier_finalize + the first cycle (operand setup of the fused passes and graph capture included) — what the
            library offered before mgs_hier_refresh.  Meant to run on a build of the PARENT commit, so that the yardstick is not the code
            under test: --rebuild-tree <checkout of the parent with its libmgs.so built> (the package is imported from there; MGS_LIBMGS
            alone does not do, the parent's library lacks the symbols this package resolves at load).
  refresh : mgs_csr_update_values_dev + mgs_hier_refresh + the first cycle, on this build.
Every measurement is a FRESH process, the two alternating round by round (at least 3 rounds), a host clock around synchronised calls.  Both
children first do the work once untimed (build + cycle; the refresh child also one refresh + cycle), so that neither figure contains the
first-use loading of kernels: the timed region is the steady state of a time-stepping caller.  The new values are the old ones × 1.25 on the
device (any values do: no step of either path depends on them).  csky3d is generated once by the parent into a temporary folder the
children load.  Prints one JSON line per operator with every round's figures, the ratio per round and the condition `refresh < rebuild by
more than the ±2.5 % box spread in every round`; stops at the first child that fails.
usage: ab_refresh.py [poisson:512 csky3d:256] [--rounds 3] [--rebuild-tree DIR] [--timeout 300]
       ab_refresh.py --child refresh|rebuild OPERATOR [--eager] [--reps K]    (one process; `--child refresh poisson:512 --eager --reps 3` is the run
       for `rocprofv3 --kernel-trace --stats`: K timed refreshes in one trace.  --eager: option graph = 0, see tools/fgcr_trace.py)"""
import argparse, json, os, shutil, subprocess, sys, tempfile, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BOX_SPREAD = 0.025      # box-to-box / process-to-process spread of whole-process timings


def operator(mg, ctx, spec, cache):
    fam, N = spec.split(":"); N = int(N)
    if fam == "poisson":
        return ctx.poisson3d(N), N ** 3
    import numpy as np
    if cache and os.path.exists(os.path.join(cache, "rp.npy")):
        rp, ci, v = (np.load(os.path.join(cache, f + ".npy")) for f in ("rp", "ci", "v"))
    else:
        from multigridsolver_amd import synthetic
        rp, ci, v = synthetic.csky3d(N, rowsum_floor=synthetic.CSKY_ROWSUM_MARGIN)
    return ctx.csr(N ** 3, N ** 3, rp, ci, v), N ** 3


def child(mode, spec, eager, reps, cache, tree):
    import ctypes as C
    if tree:
        sys.path.insert(0, os.path.abspath(tree))
    import multigridsolver_amd as mg
    ctx = mg.Context(0)
    if eager:
        ctx.set_option("graph", 0)
    A, n = operator(mg, ctx, spec, cache)
    b = ctx.vec(n).rand(seed=0); x = ctx.vec(n)

    def build():
        return mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 2500, 32).finalize()

    h = build(); h.vcycle(b, x); ctx.sync()                   # untimed: kernels loaded, pools filled
    out = {"mode": mode, "operator": spec, "rows": n, "nnz": A.nnz, "levels": h.nlev, "lib": mg.SO_PATH}
    times = []
    if mode == "rebuild":
        for _ in range(reps):
            del h; ctx.sync()
            t0 = time.perf_counter()
            h = build(); t1 = time.perf_counter(); h.vcycle(b, x); ctx.sync()
            t2 = time.perf_counter()
            times.append({"s": round(t2 - t0, 5), "setup_s": round(t1 - t0, 5), "first_cycle_s": round(t2 - t1, 5)})
    else:
        val = C.c_void_p(); mg.lib().mgs_csr_device_ptrs(A.h, None, None, C.byref(val))
        new = ctx.vec(A.nnz).axpby(1.25, mg.Vec.wrap(ctx, val.value, A.nnz), 0.0)
        A.update_values(new); h.refresh(); h.vcycle(b, x); ctx.sync()          # untimed: the numeric kernel loaded, the flags allocated
        for _ in range(reps):
            ctx.sync(); t0 = time.perf_counter()
            A.update_values(new); h.refresh(); ctx.sync(); t1 = time.perf_counter(); h.vcycle(b, x); ctx.sync()
            t2 = time.perf_counter()
            times.append({"s": round(t2 - t0, 5), "refresh_s": round(t1 - t0, 5), "first_cycle_s": round(t2 - t1, 5)})
        out["refresh_info"] = h.refresh_info(); out["graphs"] = h.graph_info()["captured_cycles"]
        out["level_nnz"] = [h.level_shape(l)[1] for l in range(h.nlev)]
    out["times"] = times; out["s"] = min(t["s"] for t in times); out["x_norm"] = x.nrm2()
    print(json.dumps(out), flush=True)
    ctx.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("operators", nargs="*", default=["poisson:512", "csky3d:256"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rebuild-tree", default=None, help="checkout of the parent commit, library built, for the rebuild leg (default: this tree)")
    ap.add_argument("--tree", default=None, help="(child) import the package from this checkout")
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--child", nargs=2, default=None)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--cache", default=None)
    o = ap.parse_args()
    if o.child:
        return child(o.child[0], o.child[1], o.eager, o.reps, o.cache, o.tree)
    rounds = max(o.rounds, 3)
    for spec in o.operators:
        cache = None
        if spec.startswith("csky3d"):
            import numpy as np
            from multigridsolver_amd import synthetic
            cache = tempfile.mkdtemp(prefix="ab_refresh_")
            for f, a in zip(("rp", "ci", "v"), synthetic.csky3d(int(spec.split(":")[1]), rowsum_floor=synthetic.CSKY_ROWSUM_MARGIN)):
                np.save(os.path.join(cache, f + ".npy"), a)
        runs = {"rebuild": [], "refresh": []}
        try:
            for _ in range(rounds):
                for mode in ("rebuild", "refresh"):
                    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, spec] + (["--cache", cache] if cache else [])
                    if mode == "rebuild" and o.rebuild_tree:
                        cmd += ["--tree", o.rebuild_tree]
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=o.timeout)
                    if r.returncode != 0:                       # nothing more is started on the device after a failure
                        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                        print(json.dumps({"operator": spec, "failed": mode, "returncode": r.returncode, "partial": runs}), flush=True)
                        return 1
                    runs[mode].append(json.loads(r.stdout.strip().splitlines()[-1]))
        finally:
            if cache:
                shutil.rmtree(cache, ignore_errors=True)
        a, b = [q["s"] for q in runs["rebuild"]], [q["s"] for q in runs["refresh"]]
        ratios = [round(x / y, 3) for x, y in zip(a, b)]
        print(json.dumps({"operator": spec, "rows": runs["refresh"][0]["rows"], "levels": runs["refresh"][0]["levels"], "rounds": rounds,
                          "rebuild_lib": runs["rebuild"][0]["lib"], "rebuild_s": a, "refresh_s": b,
                          "rebuild_parts": [q["times"][0] for q in runs["rebuild"]], "refresh_parts": [q["times"][0] for q in runs["refresh"]],
                          "rebuild_over_refresh": ratios, "refresh_info": runs["refresh"][0]["refresh_info"], "graphs_kept": runs["refresh"][0]["graphs"],
                          "level_nnz": runs["refresh"][0]["level_nnz"],
                          "refresh_below_rebuild_beyond_spread_every_round": all(y < x * (1.0 - BOX_SPREAD) for x, y in zip(a, b))}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
