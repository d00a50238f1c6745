#!/usr/bin/env python3
"""What it costs to bring a matrix that already lives in device memory into the library (mgs_csr_from_device, mgs_csr_from_coo_device,
mgs_csr_update_values_coo_dev), against two yardsticks taken in the same process: a plain device-to-device copy of the same three CSR
arrays (torch Tensor.copy_ of equal dtypes = hipMemcpyAsync device to device) and the host path a caller had before (Csr.upload of host
arrays: mgs_csr_upload's serial host check + three host-to-device copies; this change does not touch that function, so this build's
upload is the parent commit's).
Cases, each a FRESH process (--child), every path timed as the median of --reps calls after one untimed call, a host clock around calls
that end synchronised (the constructors synchronise themselves; update_values_coo is followed by Context.sync):
  poisson512       Poisson 512³: the arrays are those of mgs_csr_poisson3d (mgs_csr_device_ptrs), no host array exists.  from_device with
                   int32 indices, and with int64 index copies made by torch.
  csky256          csky3d 256³ (synthetic.csky3d): from_device int32; Csr.upload of the same host arrays; the triples under a fixed random
                   permutation through from_coo_device (int64 indices, keep_map) and update_values_coo on the kept map; the same triples
                   with every triple split in two (v/2 twice: sums back exactly).
Every assembled matrix is compared with the from_device one through an SpMV of one random vector (same bits expected).  Bytes are the
algorithmic ones: input read once + output written once.  One JSON line per case; the csky3d arrays are generated once by the parent into
a temporary folder the child loads.
usage: ab_ingest.py [poisson:512 csky3d:256] [--reps 3] [--timeout 900]
       ab_ingest.py --child poisson:512 | csky3d:256 [--cache DIR]"""
import argparse, json, os, shutil, statistics, subprocess, sys, tempfile, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


class DevPtr:
    """a raw device pointer as an object with __cuda_array_interface__ (what Csr.from_device and torch.as_tensor accept)"""
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"data": (int(ptr), False), "shape": (int(n),), "typestr": typestr, "strides": None, "version": 3}


def timed(fn, reps, sync):
    fn(); sync()                                              # untimed: kernels loaded, pools filled
    out = []
    for _ in range(reps):
        sync(); t0 = time.perf_counter(); r = fn(); sync(); out.append(time.perf_counter() - t0); del r
    return round(statistics.median(out), 5), [round(t, 5) for t in out]


def child(spec, reps, cache):
    import numpy as np
    import torch
    import multigridsolver_amd as mg
    fam, N = spec.split(":"); N = int(N); n = N ** 3
    ctx = mg.Context(0)
    dev = torch.device("cuda:0")

    def sync():
        ctx.sync(); torch.cuda.synchronize()

    out = {"operator": spec, "rows": n, "device": torch.cuda.get_device_name(0), "reps": reps, "paths": {}}
    host = None
    if fam == "poisson":
        src = ctx.poisson3d(N)
        nnz = src.nnz
        p_rp, p_ci, p_v = src.device_ptrs()
        rp = torch.as_tensor(DevPtr(p_rp, n + 1, "<i4"), device=dev); ci = torch.as_tensor(DevPtr(p_ci, nnz, "<i4"), device=dev)
        v = torch.as_tensor(DevPtr(p_v, nnz, "<f8"), device=dev)
    else:
        if cache and os.path.exists(os.path.join(cache, "rp.npy")):
            host = tuple(np.load(os.path.join(cache, f + ".npy")) for f in ("rp", "ci", "v"))
        else:
            from multigridsolver_amd import synthetic
            host = synthetic.csky3d(N, rowsum_floor=synthetic.CSKY_ROWSUM_MARGIN)
        host = (np.ascontiguousarray(host[0], dtype=np.int32), np.ascontiguousarray(host[1], dtype=np.int32), np.ascontiguousarray(host[2], dtype=np.float64))
        nnz = len(host[1])
        rp, ci, v = (torch.from_numpy(a).to(dev) for a in host)
    out["nnz"] = nnz
    csr_bytes = 4 * (n + 1) + 12 * nnz
    x = ctx.vec(n).rand(seed=1)

    def record(name, fn, nbytes, check=None):
        s, all_s = timed(fn, reps, sync)
        out["paths"][name] = {"s": s, "all_s": all_s, "bytes": nbytes}
        if check is not None:
            out["paths"][name]["same_spmv_bits"] = bool(np.array_equal(check().spmv(x).numpy(), y_ref))
        print(f"# {spec} {name}: {s} s", file=sys.stderr, flush=True)

    # yardstick: device-to-device copy of the three arrays
    d_rp, d_ci, d_v = torch.empty_like(rp), torch.empty_like(ci), torch.empty_like(v)
    record("copy_d2d", lambda: (d_rp.copy_(rp), d_ci.copy_(ci), d_v.copy_(v)) and None, 2 * csr_bytes)
    del d_rp, d_ci, d_v
    A = mg.Csr.from_device(ctx, n, n, rp, ci, v)
    y_ref = A.spmv(x).numpy(); del A
    record("from_device_i32", lambda: mg.Csr.from_device(ctx, n, n, rp, ci, v), 2 * csr_bytes, lambda: mg.Csr.from_device(ctx, n, n, rp, ci, v))
    if fam == "poisson":
        rp64, ci64 = rp.to(torch.int64), ci.to(torch.int64)
        torch.cuda.synchronize()
        record("from_device_i64", lambda: mg.Csr.from_device(ctx, n, n, rp64, ci64, v), 8 * (n + 1) + 16 * nnz + csr_bytes, lambda: mg.Csr.from_device(ctx, n, n, rp64, ci64, v))
        del rp64, ci64
    else:
        record("host_upload", lambda: mg.Csr.upload(ctx, n, n, *host), 2 * csr_bytes)
        rows = torch.repeat_interleave(torch.arange(n, device=dev), (rp[1:] - rp[:-1]).to(torch.int64))
        g = torch.Generator(device=dev); g.manual_seed(7)
        for name, split in (("coo", 1), ("coo_split2", 2)):
            r, c, w = rows, ci.to(torch.int64), v
            if split == 2:
                r, c, w = r.repeat_interleave(2), c.repeat_interleave(2), (w * 0.5).repeat_interleave(2)
            p = torch.randperm(len(r), device=dev, generator=g)
            r, c, w = r[p].contiguous(), c[p].contiguous(), w[p].contiguous()
            del p; torch.cuda.synchronize()
            nt = len(r)
            record("from_" + name + "_i64", lambda: mg.Csr.from_coo_device(ctx, n, n, r, c, w), 24 * nt + csr_bytes, lambda: mg.Csr.from_coo_device(ctx, n, n, r, c, w))
            M = mg.Csr.from_coo_device(ctx, n, n, r, c, w, keep_map=True)
            out["paths"]["from_" + name + "_i64"]["coo_info"] = M.coo_info()
            record("update_values_" + name, lambda: M.update_values_coo(w) and None, 8 * nt + 4 * nt + 4 * nnz + 8 * nnz, lambda: M)
            del M, r, c, w
    copy_s = out["paths"]["copy_d2d"]["s"]
    up = out["paths"].get("host_upload", {}).get("s")
    for q in out["paths"].values():
        q["over_copy"] = round(q["s"] / copy_s, 2)
        if up:
            q["over_host_upload"] = round(q["s"] / up, 4)
    print(json.dumps(out), flush=True)
    ctx.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("operators", nargs="*", default=["poisson:512", "csky3d:256"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--child", default=None)
    ap.add_argument("--cache", default=None)
    o = ap.parse_args()
    if o.child:
        return child(o.child, o.reps, o.cache)
    for spec in o.operators:
        cache = None
        if spec.startswith("csky3d"):
            import numpy as np
            from multigridsolver_amd import synthetic
            cache = tempfile.mkdtemp(prefix="ab_ingest_")
            for f, a in zip(("rp", "ci", "v"), synthetic.csky3d(int(spec.split(":")[1]), rowsum_floor=synthetic.CSKY_ROWSUM_MARGIN)):
                np.save(os.path.join(cache, f + ".npy"), a)
        try:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", spec, "--reps", str(o.reps)] + (["--cache", cache] if cache else [])
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=o.timeout)
            if r.returncode != 0:                               # nothing more is started on the device after a failure
                sys.stderr.write(r.stdout[-2000:])
                print(json.dumps({"operator": spec, "failed": True, "returncode": r.returncode}), flush=True)
                return 1
            print(r.stdout.strip().splitlines()[-1], flush=True)
        finally:
            if cache:
                shutil.rmtree(cache, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
