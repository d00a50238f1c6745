#!/usr/bin/env python3
"""What the device sums and scalings (mgs_csr_add / mgs_csr_add_numeric / mgs_csr_scale, csrc/csr_algebra.hip) cost, every measurement a
FRESH process, the workloads alternating round by round (at least 3 rounds), a host clock around calls that end in a synchronise:
  diag N  : C = α·D + β·K, K = Poisson 3-D N³, D = mgs_csr_from_diag of a random vector (the implicit time step M/Δt + K)
  shift N : C = α·K + β·S, S = K's pattern moved down one row (row i of S holds the columns of row i + 1 of K; the last row is empty): two
            of a row's seven columns are common, the union holds twelve
Each child times, after one untimed pass of everything (kernels loaded, pools filled):
  add       the full mgs_csr_add, C destroyed before every call
  numeric   mgs_csr_add_numeric alone, `--inner` calls per window, per call
  scale     mgs_csr_scale(C, dl, dr) with both vectors, `--inner` calls per window, per call
  copy      a device-to-device copy of as many bytes as C's three arrays hold (12 B per entry + 4 B per row + 4): the bandwidth floor of
            writing C; its rate also prices the least the numeric pass must move — the col, val and rowptr of A, B and C once each
            (floor_numeric_s in the output)
  detour    (once per child, unless --no-detour) what the calls replace: download A and B, scipy's α·A + β·B on the CPU, Csr.upload
and prints a digest of C's arrays: the bits must agree between the rounds.  One JSON line per child, one summary line per workload and
size with medians and min–max spreads; stops at the first child that fails.
usage: ab_add.py [--sizes 128 256] [--rounds 3] [--inner 10] [--no-detour] [--timeout 900]
       ab_add.py --child diag|shift N [--reps K] [--inner K] [--no-detour]"""
import argparse, hashlib, json, os, statistics, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ALPHA, BETA = 1.0 / 3.0, 0.7


def digest(arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()[:16]


def child(mode, N, reps, inner, detour):
    import numpy as np
    import torch
    import multigridsolver_amd as mg
    ctx = mg.Context(0)
    K = ctx.poisson3d(N); n = N ** 3
    if mode == "diag":
        A = mg.Csr.from_diag(ctx, ctx.vec(n).rand(seed=3)); B = K
    else:
        rp, ci, v = K.download()
        A = K; B = ctx.csr(n, n, np.r_[rp[1:] - rp[1], rp[-1] - rp[1]].astype(np.int32), ci[rp[1]:], v[rp[1]:])
        del rp, ci, v
    Cm = A.add(B, ALPHA, BETA); ctx.sync()                              # untimed
    info = Cm.add_info(); nnz = Cm.nnz
    full, numeric, scale, copy = [], [], [], []
    for _ in range(reps):
        del Cm; ctx.sync()
        t0 = time.perf_counter(); Cm = A.add(B, ALPHA, BETA); ctx.sync(); full.append(round(time.perf_counter() - t0, 5))
    dig = digest(Cm.download())
    Cm.add_update(A, B, ALPHA, BETA); ctx.sync()
    for _ in range(max(reps, 3)):
        t0 = time.perf_counter()
        for _ in range(inner):
            Cm.add_update(A, B, ALPHA, BETA)
        ctx.sync(); numeric.append(round((time.perf_counter() - t0) / inner, 6))
    nbytes = 12 * nnz + 4 * (n + 1)
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0"); dst = torch.empty_like(src)
    dst.copy_(src); torch.cuda.synchronize()
    for _ in range(max(reps, 3)):
        t0 = time.perf_counter()
        for _ in range(inner):
            dst.copy_(src)
        torch.cuda.synchronize(); copy.append(round((time.perf_counter() - t0) / inner, 6))
    del src, dst
    rate = 2 * nbytes / min(copy)                                       # bytes read + written per second
    need = 12 * (A.nnz + B.nnz + nnz) + 3 * 4 * (n + 1)
    out = {"mode": mode, "N": N, "rows": n, "nnz_A": A.nnz, "nnz_B": B.nnz, "nnz_C": nnz, "info": info, "bytes_C": nbytes, "digest": dig}
    if detour:
        t0 = time.perf_counter()
        import scipy.sparse as sps
        (rpa, cia, va), (rpb, cib, vb) = A.download(), B.download()
        S = sps.csr_matrix(ALPHA * sps.csr_matrix((va, cia, rpa), shape=(n, n)) + BETA * sps.csr_matrix((vb, cib, rpb), shape=(n, n)))
        S.sort_indices()
        Cd = ctx.csr(n, n, S.indptr, S.indices, S.data); ctx.sync()
        out["detour_s"] = round(time.perf_counter() - t0, 4); out["detour_nnz"] = Cd.nnz
        del Cd, S, rpa, cia, va, rpb, cib, vb
    ones = ctx.vec(n).fill(1.0)                                         # scaling by one leaves the values finite however often it runs
    Cm.scale(ones, ones); ctx.sync()
    for _ in range(max(reps, 3)):
        t0 = time.perf_counter()
        for _ in range(inner):
            Cm.scale(ones, ones)
        ctx.sync(); scale.append(round((time.perf_counter() - t0) / inner, 6))
    out.update({"full_s": full, "numeric_s": numeric, "scale_s": scale, "copy_s": copy, "s": min(full), "numeric_min_s": min(numeric), "scale_min_s": min(scale),
                "copy_min_s": min(copy), "copy_GBps": round(rate / 1e9, 1), "bytes_numeric_min": need, "floor_numeric_s": round(need / rate, 6)})
    print(json.dumps(out), flush=True)
    ctx.close()
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
    return {"median": round(statistics.median(xs), 6), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[128, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--no-detour", action="store_true")
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--child", nargs=2, default=None)
    ap.add_argument("--reps", type=int, default=3)
    o = ap.parse_args()
    if o.child:
        return child(o.child[0], int(o.child[1]), o.reps, max(o.inner, 1), not o.no_detour)
    rounds = max(o.rounds, 3)
    me = [sys.executable, os.path.abspath(__file__), "--child"]
    for N in o.sizes:
        runs = {"diag": [], "shift": []}
        for _ in range(rounds):
            for mode in ("diag", "shift"):                              # alternating
                q = run(me + [mode, str(N), "--reps", str(o.reps), "--inner", str(o.inner)] + (["--no-detour"] if o.no_detour else []), o.timeout)
                if q is None:
                    return 1
                runs[mode].append(q)
        for mode, rs in runs.items():
            out = {"compare": mode, "N": N, "rounds": rounds, "nnz_C": rs[0]["nnz_C"], "info": rs[0]["info"], "bytes_C": rs[0]["bytes_C"],
                   "bytes_numeric_min": rs[0]["bytes_numeric_min"], "same_bits": len({q["digest"] for q in rs}) == 1,
                   "add_s": stats([q["s"] for q in rs]), "numeric_s": stats([q["numeric_min_s"] for q in rs]), "scale_s": stats([q["scale_min_s"] for q in rs]),
                   "copy_s": stats([q["copy_min_s"] for q in rs]), "copy_GBps": stats([q["copy_GBps"] for q in rs]),
                   "floor_numeric_s": stats([q["floor_numeric_s"] for q in rs])}
            if not o.no_detour:
                out["detour_s"] = stats([q["detour_s"] for q in rs])
            print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
