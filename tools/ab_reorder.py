#!/usr/bin/env python3
"""What reordering a device matrix and assembling one from blocks (mgs_csr_permute / mgs_csr_permute_numeric / mgs_csr_bmat /
mgs_csr_bmat_numeric, csrc/reorder.hip) cost, every measurement a FRESH process, the workloads alternating round by round (at least 3
rounds), a host clock around calls that end in a synchronise.  L = Poisson 3-D N³, n = N³ rows.
  random N     : C = L(p, p) for a random permutation p (fixed seed): every row on the lane arm, the new columns scattered
  interleave N : C = L(p, p) for p[2k] = k, p[2k+1] = n/2 + k: the two halves of the numbering interleaved, as two fields would be
  bmat N       : K = [[L, c·I], [c·I, L]], the two-field operator of the README's recipe (2n rows)
Each child times, after one untimed pass of everything (kernels loaded, pools filled):
  build     the full mgs_csr_permute (keep_map on) or mgs_csr_bmat, the result destroyed before every call
  numeric   mgs_csr_permute_numeric / mgs_csr_bmat_numeric alone, `--inner` calls per window, per call
  copy      a device-to-device copy of as many bytes as the result's three arrays hold (12 B per entry + 4 B per row + 4): the floor of
            writing it; copy_val: of its values alone (8 B per entry), the floor of the numeric pass
  coo       the device route that existed before: the result's triples built with torch from the operands' arrays (already on the
            device), then Csr.from_coo_device; the triples' construction is inside the window
  detour    (once per child, unless --no-detour or N above --detour-max) download, scipy's A[p][:, p] or scipy.sparse.bmat on the CPU, Csr.upload
and prints a digest of the result's arrays: the bits must agree between the rounds and with the coo route.  One JSON line per child, one
summary line per workload and size with medians and min–max spreads, and the same summaries as a table in --out (default
profiles/r20_reorder.md); stops at the first child that fails.
usage: ab_reorder.py [--sizes 128 256] [--rounds 3] [--inner 10] [--no-detour] [--detour-max 128] [--timeout 900] [--out profiles/r20_reorder.md]
       ab_reorder.py --child random|interleave|bmat N [--reps K] [--inner K] [--no-detour]"""
import argparse, hashlib, json, os, statistics, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
MODES = ("random", "interleave", "bmat")
COUPLING = 0.25


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
    import numpy as np
    import torch
    import multigridsolver_amd as mg
    ctx = mg.Context(0)
    L = ctx.poisson3d(N); n = N ** 3
    rp, ci, v = L.download()
    t_rp = torch.from_numpy(rp.astype(np.int64)).to("cuda:0"); t_ci = torch.from_numpy(ci).to("cuda:0"); t_v = torch.from_numpy(v).to("cuda:0")
    if mode == "bmat":
        D = mg.Csr.from_diag(ctx, ctx.vec(n).fill(COUPLING))
        grid = [[L, D], [D, L]]
        build = lambda: mg.Csr.bmat(ctx, grid)
        numeric = lambda R: R.bmat_update(grid)
    else:
        if mode == "random":
            p = torch.from_numpy(np.random.default_rng(20).permutation(n).astype(np.int32)).to("cuda:0")
        else:
            p = torch.empty(n, dtype=torch.int32, device="cuda:0")
            p[0::2] = torch.arange(0, n // 2, dtype=torch.int32, device="cuda:0"); p[1::2] = torch.arange(n // 2, n, dtype=torch.int32, device="cuda:0")
        build = lambda: L.permute(p, p, keep_map=True)
        numeric = lambda R: R.permute_update(L)
    torch.cuda.synchronize()
    R = build(); ctx.sync()                                              # untimed
    info = R.bmat_info() if mode == "bmat" else R.permute_info()
    nnz, nr = R.nnz, R.shape[0]
    full = []
    for _ in range(reps):
        del R; ctx.sync()
        t0 = time.perf_counter(); R = build(); ctx.sync(); full.append(round(time.perf_counter() - t0, 5))
    out = {"mode": mode, "N": N, "rows": nr, "nnz": nnz, "info": info, "digest": digest(R.download()), "full_s": full, "s": min(full)}

    def copy_of(nbytes):
        src = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda:0"); dst = torch.empty_like(src)
        return windows(lambda: dst.copy_(src), torch.cuda.synchronize, max(reps, 3), inner)
    out["bytes"] = 12 * nnz + 4 * (nr + 1)
    out["numeric_s"] = windows(lambda: numeric(R), ctx.sync, max(reps, 3), inner); out["numeric_min_s"] = min(out["numeric_s"])
    out["copy_s"] = copy_of(out["bytes"]); out["copy_min_s"] = min(out["copy_s"])
    out["copy_val_s"] = copy_of(8 * nnz); out["copy_val_min_s"] = min(out["copy_val_s"])

    def coo():
        rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device="cuda:0"), (t_rp[1:] - t_rp[:-1]))
        if mode == "bmat":
            k = torch.arange(n, dtype=torch.int32, device="cuda:0"); c = torch.full((n,), COUPLING, dtype=torch.float64, device="cuda:0")
            r = torch.cat([rows, k, k + n, rows + n]); q = torch.cat([t_ci, k + n, k, t_ci + n]); w = torch.cat([t_v, c, c, t_v])
            torch.cuda.synchronize()
            return mg.Csr.from_coo_device(ctx, 2 * n, 2 * n, r, q, w)
        pinv = torch.empty(n, dtype=torch.int32, device="cuda:0"); pinv[p.long()] = torch.arange(n, dtype=torch.int32, device="cuda:0")
        r = pinv[rows.long()]; q = pinv[t_ci.long()]
        torch.cuda.synchronize()
        return mg.Csr.from_coo_device(ctx, n, n, r, q, t_v)
    Rc = coo(); ctx.sync()
    out["coo_same_bits"] = digest(Rc.download()) == out["digest"]
    ts = []
    for _ in range(reps):
        del Rc; ctx.sync()
        t0 = time.perf_counter(); Rc = coo(); ctx.sync(); ts.append(round(time.perf_counter() - t0, 5))
    del Rc
    out["coo_s"] = ts; out["coo_min_s"] = min(ts)
    if detour:
        import scipy.sparse as sps
        t0 = time.perf_counter()
        rp, ci, v = L.download()
        M = sps.csr_matrix((v, ci, rp), shape=(n, n))
        if mode == "bmat":
            cI = sps.identity(n, format="csr") * COUPLING
            M = sps.bmat([[M, cI], [cI, M]], format="csr")
        else:
            ph = p.cpu().numpy()
            M = sps.csr_matrix(M[ph][:, ph])
        M.sort_indices()
        Rd = ctx.csr(M.shape[0], M.shape[1], M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data); ctx.sync()
        out["detour_s"] = round(time.perf_counter() - t0, 4); out["detour_same_bits"] = digest(Rd.download()) == out["digest"]
        del Rd, M
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


def ms(s):
    return f"{1e3 * s['median']:.3f} ({1e3 * s['min']:.3f}–{1e3 * s['max']:.3f})"


def write_table(path, summaries, rounds):
    """the whole profile: legend, one row per workload and size in the order they ran, what the numbers do not cover"""
    lines = ["# Reordering and assembling device matrices: mgs_csr_permute, mgs_csr_bmat", "",
             f"`tools/ab_reorder.py`: alternating fresh processes, {rounds} rounds, one GPU, milliseconds, median (min–max) of the rounds' best windows.  L = Poisson N³;",
             "`random`: C = L(p, p), p a random permutation; `interleave`: p[2k] = k, p[2k+1] = n/2 + k; `bmat`: [[L, cI], [cI, L]].  build = the full `mgs_csr_permute`",
             "(map kept) / `mgs_csr_bmat`; numeric = `mgs_csr_permute_numeric` / `mgs_csr_bmat_numeric` alone.  same bits: the digests of the result's arrays agree between",
             "the rounds, with the triple route and, where it ran, with the detour.", "",
             "| case | N | rows | entries | build | numeric | copy of the arrays | copy of the values | torch triples + from_coo_device | download, scipy, upload | same bits |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for s in summaries:
        lines.append(f"| {s['compare']} | {s['N']} | {s['rows']} | {s['nnz']} | {ms(s['build_s'])} | {ms(s['numeric_s'])} | {ms(s['copy_s'])} | {ms(s['copy_val_s'])} | "
                     f"{ms(s['coo_s'])} | {ms(s['detour_s']) if 'detour_s' in s else 'not measured'} | {s['same_bits']} |")
    skipped = sorted({s["N"] for s in summaries if "detour_s" not in s})
    lines += ["", "Not measured: " + (f"the detour at N = {', '.join(map(str, skipped))} (--no-detour or above --detour-max: scipy's indexing of a matrix of that size takes "
                                      "minutes per child on the host); " if skipped else "") +
              "a kernel trace that would split a full call into its allocations, checks, scan, host waits and fill; the wave arm's speed (every Poisson row takes the lane arm)."]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[128, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--no-detour", action="store_true")
    ap.add_argument("--detour-max", type=int, default=128, help="largest N at which the download, scipy, upload detour is run")
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r20_reorder.md"))
    ap.add_argument("--child", nargs=2, default=None)
    ap.add_argument("--reps", type=int, default=3)
    o = ap.parse_args()
    if o.child:
        return child(o.child[0], int(o.child[1]), o.reps, max(o.inner, 1), not o.no_detour)
    rounds = max(o.rounds, 3)
    me = [sys.executable, os.path.abspath(__file__), "--child"]
    summaries = []
    for N in o.sizes:
        no_detour = o.no_detour or N > o.detour_max
        runs = {m: [] for m in MODES}
        for _ in range(rounds):
            for mode in MODES:                                           # alternating
                q = run(me + [mode, str(N), "--reps", str(o.reps), "--inner", str(o.inner)] + (["--no-detour"] if no_detour else []), o.timeout)
                if q is None:
                    return 1
                runs[mode].append(q)
        for mode, rs in runs.items():
            out = {"compare": mode, "N": N, "rounds": rounds, "rows": rs[0]["rows"], "nnz": rs[0]["nnz"], "info": rs[0]["info"], "bytes": rs[0]["bytes"],
                   "same_bits": len({q["digest"] for q in rs}) == 1 and all(q["coo_same_bits"] and q.get("detour_same_bits", True) for q in rs),
                   "build_s": stats([q["s"] for q in rs])}
            for key in ("numeric", "copy", "copy_val", "coo"):
                out[key + "_s"] = stats([q[key + "_min_s"] for q in rs])
            if not no_detour:
                out["detour_s"] = stats([q["detour_s"] for q in rs])
            print(json.dumps(out), flush=True)
            summaries.append(out)
        write_table(o.out, summaries, rounds)
    return 0


if __name__ == "__main__":
    sys.exit(main())
