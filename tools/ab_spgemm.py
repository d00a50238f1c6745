#!/usr/bin/env python3
"""What the device sparse product (mgs_csr_spgemm, csrc/spgemm.hip) costs, three ways, every measurement a FRESH process, the legs of a
comparison alternating round by round (at least 3 rounds), a host clock around calls that end in a synchronise:
  (a) galerkin N : mgs_csr_galerkin for a P that is NOT an aggregation on Poisson 3-D N³ — P is the composed pairwise aggregation
                   (10 / 2 / 8, two passes) with a second weighted entry per row (0.75 on the row's aggregate, 0.25 on the next one).
                   This build against the PARENT commit's host path: --parent-tree <checkout of the parent with its libmgs.so built> (the
                   package is imported from there, as in tools/ab_refresh.py).  Both legs print a digest of the result's arrays: the
                   bits must agree.
  (b) product N  : mgs_csr_spgemm(A, A) on Poisson 3-D N³, against scipy's A @ A on the CPU (one process per size, no device) and against
                   a device-to-device copy of as many bytes as C's arrays hold (12 B per entry + 4 B per row), the bandwidth floor.
  (c) the same child times mgs_csr_spgemm_numeric alone (the values again, in place) against the full product.
Each child does its work once untimed first (kernels loaded, pools filled).  Prints one JSON line per child and one summary line per
comparison with medians and min–max spreads; stops at the first child that fails.
usage: ab_spgemm.py [--galerkin 128] [--product 128 256] [--rounds 3] [--parent-tree DIR] [--no-scipy] [--timeout 600]
       ab_spgemm.py --child galerkin|product|scipy N [--tree DIR] [--reps K]"""
import argparse, hashlib, json, os, statistics, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def digest(arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()[:16]


def child_galerkin(N, reps, tree):
    import numpy as np
    import torch  # noqa: F401  (before libmgs.so: one HIP runtime per process)
    if tree:
        sys.path.insert(0, os.path.abspath(tree))
    import multigridsolver_amd as mg
    ctx = mg.Context(0)
    A = ctx.poisson3d(N); n = N ** 3
    h = mg.Hierarchy(A, 0.6, 1, 1).coarsen(10.0, 2, 8.0, 2500, 2)      # one coarsening: the composed two-pass aggregation
    g = h.level_P(0).agg().astype(np.int64); nc = h.level_shape(1)[0]
    del h
    ok = g >= 0                                                         # rows outside every aggregate (G0: edges and corners) stay empty rows of P
    ga = g[ok]; c2 = (ga + 1) % nc
    lo, hi = np.minimum(ga, c2), np.maximum(ga, c2)
    col = np.stack([lo, hi], 1).ravel().astype(np.int32)
    val = np.where(np.stack([lo == ga, hi == ga], 1), 0.75, 0.25).ravel()
    P = ctx.csr(n, nc, np.r_[0, np.cumsum(2 * ok)].astype(np.int32), col, val)
    T = mg.Xfer.from_csr(P)
    assert not T.is_aggregation
    Ac = A.galerkin(T); ctx.sync()                                      # untimed
    times = []
    for _ in range(reps):
        del Ac; ctx.sync()
        t0 = time.perf_counter(); Ac = A.galerkin(T); ctx.sync(); times.append(round(time.perf_counter() - t0, 5))
    print(json.dumps({"mode": "galerkin", "N": N, "rows": n, "coarse_rows": nc, "nnz_A": A.nnz, "nnz_Ac": Ac.nnz, "lib": mg.SO_PATH, "times_s": times,
                      "s": min(times), "digest": digest(Ac.download())}), flush=True)
    ctx.close()
    return 0


def child_product(N, reps):
    import torch
    import multigridsolver_amd as mg
    ctx = mg.Context(0)
    A = ctx.poisson3d(N); n = N ** 3
    Cm = A.matmul(A); ctx.sync()                                        # untimed
    info = Cm.spgemm_info(); nnz = Cm.nnz
    full, numeric, copy = [], [], []
    for _ in range(reps):
        del Cm; ctx.sync()
        t0 = time.perf_counter(); Cm = A.matmul(A); ctx.sync(); full.append(round(time.perf_counter() - t0, 5))
    Cm.matmul_update(A, A); ctx.sync()
    for _ in range(max(reps, 5)):
        t0 = time.perf_counter(); Cm.matmul_update(A, A); ctx.sync(); numeric.append(round(time.perf_counter() - t0, 5))
    nbytes = 12 * nnz + 4 * (n + 1)
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0"); dst = torch.empty_like(src)
    dst.copy_(src); torch.cuda.synchronize()
    for _ in range(max(reps, 5)):
        t0 = time.perf_counter(); dst.copy_(src); torch.cuda.synchronize(); copy.append(round(time.perf_counter() - t0, 5))
    print(json.dumps({"mode": "product", "N": N, "rows": n, "nnz_A": A.nnz, "nnz_C": nnz, "info": info, "bytes_C": nbytes, "full_s": full, "numeric_s": numeric,
                      "copy_s": copy, "s": min(full), "numeric_min_s": min(numeric), "copy_min_s": min(copy)}), flush=True)
    ctx.close()
    return 0


def child_scipy(N):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import spgemm_ref as ref
    import scipy.sparse as sps
    m, n, rp, ci, v = ref.poisson3d_pattern(N)
    S = sps.csr_matrix((v, ci, rp), shape=(m, n))
    t0 = time.perf_counter(); Cs = S @ S; t = time.perf_counter() - t0
    print(json.dumps({"mode": "scipy", "N": N, "rows": m, "nnz_A": int(S.nnz), "nnz_C": int(Cs.nnz), "s": round(t, 4)}), flush=True)
    return 0


def run(cmd, timeout):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:                       # nothing more is started on the device after a failure
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(json.dumps({"failed": cmd[2:], "returncode": r.returncode}), flush=True)
        return None
    line = r.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def stats(xs):
    return {"median": round(statistics.median(xs), 5), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--galerkin", type=int, nargs="*", default=[128])
    ap.add_argument("--product", type=int, nargs="*", default=[128, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None, help="checkout of the parent commit, library built, for the host-path leg of (a)")
    ap.add_argument("--tree", default=None, help="(child) import the package from this checkout")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", nargs=2, default=None)
    ap.add_argument("--reps", type=int, default=1)
    o = ap.parse_args()
    if o.child:
        mode, N = o.child[0], int(o.child[1])
        return child_galerkin(N, o.reps, o.tree) if mode == "galerkin" else child_product(N, o.reps) if mode == "product" else child_scipy(N)
    rounds = max(o.rounds, 3)
    me = [sys.executable, os.path.abspath(__file__), "--child"]
    for N in o.galerkin:
        legs = {"device": [], "parent_host": []}
        for _ in range(rounds):
            for leg in (("parent_host", "device") if o.parent_tree else ("device",)):
                q = run(me + ["galerkin", str(N)] + (["--tree", o.parent_tree] if leg == "parent_host" else []), o.timeout)
                if q is None:
                    return 1
                legs[leg].append(q)
        dev = [q["s"] for q in legs["device"]]; par = [q["s"] for q in legs["parent_host"]]
        out = {"compare": "galerkin", "N": N, "rounds": rounds, "device_s": stats(dev), "nnz_Ac": legs["device"][0]["nnz_Ac"]}
        if par:
            out.update({"parent_host_s": stats(par), "parent_lib": legs["parent_host"][0]["lib"], "parent_over_device": [round(p / d, 2) for p, d in zip(par, dev)],
                        "same_bits": len({q["digest"] for q in legs["device"] + legs["parent_host"]}) == 1,
                        "device_not_slower_every_round": all(d <= p for p, d in zip(par, dev))})
        print(json.dumps(out), flush=True)
    for N in o.product:
        runs = []
        for _ in range(rounds):
            q = run(me + ["product", str(N)], o.timeout)
            if q is None:
                return 1
            runs.append(q)
        out = {"compare": "product", "N": N, "rounds": rounds, "nnz_C": runs[0]["nnz_C"], "info": runs[0]["info"], "bytes_C": runs[0]["bytes_C"],
               "full_s": stats([q["s"] for q in runs]), "numeric_s": stats([q["numeric_min_s"] for q in runs]), "copy_s": stats([q["copy_min_s"] for q in runs])}
        if not o.no_scipy:
            q = run(me + ["scipy", str(N)], o.timeout)
            if q is None:
                return 1
            out["scipy_s"] = q["s"]
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
