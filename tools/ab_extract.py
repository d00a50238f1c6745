#!/usr/bin/env python3
"""What blocks of a device matrix and the vector gather / scatter (mgs_csr_extract / mgs_csr_extract_numeric / mgs_vec_gather /
mgs_vec_scatter, csrc/extract.hip) cost, every measurement a FRESH process, the workloads alternating round by round (at least 3 rounds), a
host clock around calls that end in a synchronise.  A = Poisson 3-D N³ with the plane i = 0 fixed: `fixed` its N² rows, `free` the others.
  ff N : S = A(free, free), the operator of the reduced system (every row on the lane arm, keep_map on)
  fc N : S = A(free, fixed), its coupling to the boundary values (N² entries in N³ − N² rows: almost all rows come out empty)
Each child times, after one untimed pass of everything (kernels loaded, pools filled):
  extract   the full mgs_csr_extract, S destroyed before every call
  numeric   (ff) mgs_csr_extract_numeric alone, `--inner` calls per window, per call
  gather    (ff) mgs_vec_gather of the free entries of a vector of N³, scatter: mgs_vec_scatter back; per call as above
  copy      a device-to-device copy of as many bytes as S's three arrays hold (12 B per entry + 4 B per row + 4): the floor of writing S;
  copy_val  (ff) ... of S's values alone (8 B per entry), against the numeric pass; copy_vec: of 8 B per free entry, against gather / scatter
  detour    (once per child, unless --no-detour) what the call replaces: download A, scipy's A[rows][:, cols] on the CPU, Csr.upload
and prints a digest of S's arrays: the bits must agree between the rounds.  One JSON line per child, one summary line per workload and
size with medians and min–max spreads; stops at the first child that fails.
usage: ab_extract.py [--sizes 128 256] [--rounds 3] [--inner 10] [--no-detour] [--timeout 900]
       ab_extract.py --child ff|fc N [--reps K] [--inner K] [--no-detour]"""
import argparse, hashlib, json, os, statistics, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def digest(arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()[:16]


def windows(fn, sync, reps, inner):
    """per-call seconds of `inner` enqueued calls between two synchronisations, `reps` windows after one untimed call"""
    fn(); sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        sync(); out.append(round((time.perf_counter() - t0) / inner, 7))
    return out


def child(mode, N, reps, inner, detour):
    import torch
    import multigridsolver_amd as mg
    ctx = mg.Context(0)
    A = ctx.poisson3d(N); n = N ** 3; nfix = N * N
    fixed = torch.arange(0, nfix, dtype=torch.int32, device="cuda:0"); free = torch.arange(nfix, n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rows, cols, keep = (free, free, True) if mode == "ff" else (free, fixed, False)
    S = A.extract(rows, cols, keep_map=keep); ctx.sync()                # untimed
    info = S.extract_info(); nnz = S.nnz; nr = S.shape[0]
    full = []
    for _ in range(reps):
        del S; ctx.sync()
        t0 = time.perf_counter(); S = A.extract(rows, cols, keep_map=keep); ctx.sync(); full.append(round(time.perf_counter() - t0, 5))
    out = {"mode": mode, "N": N, "rows_A": n, "nnz_A": A.nnz, "rows_S": nr, "cols_S": S.shape[1], "nnz_S": nnz, "info": info, "digest": digest(S.download()),
           "full_s": full, "s": min(full)}

    def copy_of(nbytes):
        src = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda:0"); dst = torch.empty_like(src)
        return windows(lambda: dst.copy_(src), torch.cuda.synchronize, max(reps, 3), inner)
    out["bytes_S"] = 12 * nnz + 4 * (nr + 1)
    out["copy_s"] = copy_of(out["bytes_S"]); out["copy_min_s"] = min(out["copy_s"])
    if mode == "ff":
        out["numeric_s"] = windows(lambda: S.extract_update(A), ctx.sync, max(reps, 3), inner); out["numeric_min_s"] = min(out["numeric_s"])
        out["copy_val_s"] = copy_of(8 * nnz); out["copy_val_min_s"] = min(out["copy_val_s"])
        x = ctx.vec(n).rand(seed=3); y = ctx.vec(nr)
        out["gather_s"] = windows(lambda: x.gather(free, out=y), ctx.sync, max(reps, 3), inner); out["gather_min_s"] = min(out["gather_s"])
        out["scatter_s"] = windows(lambda: x.scatter(free, y), ctx.sync, max(reps, 3), inner); out["scatter_min_s"] = min(out["scatter_s"])
        out["copy_vec_s"] = copy_of(8 * nr); out["copy_vec_min_s"] = min(out["copy_vec_s"])
    if detour:
        t0 = time.perf_counter()
        import scipy.sparse as sps
        rp, ci, v = A.download()
        M = sps.csr_matrix((v, ci, rp), shape=(n, n))[rows.cpu().numpy()][:, cols.cpu().numpy()]
        M = sps.csr_matrix(M); M.sort_indices()
        Sd = ctx.csr(M.shape[0], M.shape[1], M.indptr, M.indices, M.data); ctx.sync()
        out["detour_s"] = round(time.perf_counter() - t0, 4); out["detour_nnz"] = Sd.nnz
        del Sd, M, rp, ci, v
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
    return {"median": round(statistics.median(xs), 7), "min": min(xs), "max": max(xs)}


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
        runs = {"ff": [], "fc": []}
        for _ in range(rounds):
            for mode in ("ff", "fc"):                                   # alternating
                q = run(me + [mode, str(N), "--reps", str(o.reps), "--inner", str(o.inner)] + (["--no-detour"] if o.no_detour else []), o.timeout)
                if q is None:
                    return 1
                runs[mode].append(q)
        for mode, rs in runs.items():
            out = {"compare": mode, "N": N, "rounds": rounds, "rows_S": rs[0]["rows_S"], "cols_S": rs[0]["cols_S"], "nnz_S": rs[0]["nnz_S"], "info": rs[0]["info"],
                   "bytes_S": rs[0]["bytes_S"], "same_bits": len({q["digest"] for q in rs}) == 1, "extract_s": stats([q["s"] for q in rs]),
                   "copy_s": stats([q["copy_min_s"] for q in rs])}
            for key in ("numeric", "copy_val", "gather", "scatter", "copy_vec"):
                if key + "_min_s" in rs[0]:
                    out[key + "_s"] = stats([q[key + "_min_s"] for q in rs])
            if not o.no_detour:
                out["detour_s"] = stats([q["detour_s"] for q in rs]); out["detour_same_nnz"] = all(q["detour_nnz"] == q["nnz_S"] for q in rs)
            print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
