#!/usr/bin/env python3
"""bench.py — V-cycles/s and fine-level CSR-SpMV HBM GB/s on the synthetic 7-point 3-D Poisson
problem (BASELINE.json configs[4], grid 512^3), one process per GPU.

  python bench.py --gpus N --steps K --warmup W          (N>1: launched by torch.distributed.run)
  python bench.py --gpus 1 --steps K --warmup W --full   (every figure below, not only the headline)
  python bench.py --gpus 1 --steps K --warmup W --dump-outputs bench_outputs

A "step" is one application of the V-cycle preconditioner (MultiGridPrecond::solve, reference
src/common/bicg.cpp:51-61) to a fixed right-hand side that is already resident in HBM.  The
hierarchy is built on the device (mgs_hier_coarsen) before the timed region.  N>1 shards the
fine grid by contiguous plane ranges (strong scaling: the 512^3 problem is fixed) and exchanges
one halo plane per neighbour per SpMV-shaped kernel through torch.distributed (RCCL).

Prints ONE JSON line on rank 0: value = whole-job V-cycles/s over exactly K timed steps,
ms_per_step = milliseconds of one of them.  A plain run does only that: set-up, W warm-up
steps, the K timed steps, the outputs (--dump-outputs) and the line.  --full adds everything
else, as its own untimed legs: "roofline" = achieved HBM GB/s of the fine-level SpMV kernel
measured live with HIP events on the stream the kernel runs on; "solve_check" = solves to
1e-10 (BiCGSTAB and FGCR + K-cycle, the convection-diffusion leg); "bundled_matrices";
"cpu_baseline" = the CPU oracle's V-cycle (port of the same cycle) timed on this host.

--dump-outputs DIR writes what the last timed step computed, x = M^-1 b, as DIR/x.npy (float64)
when it fits in 64 MB, else a fixed sample of it: DIR/x_sample.npy at the row indices in
DIR/x_sample_index.npy (2^20 rows drawn with seed 0).  b is seeded, so the same arguments give
the same inputs in every run.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

HBM_PEAK_GBPS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def log(*a):
    if int(os.environ.get("RANK", "0")) == 0:
        print("[bench]", *a, file=sys.stderr, flush=True)


def spmv_bytes(n, nnz):      # BASELINE.md §2 / SURVEY §8d row d3
    return 12 * nnz + 20 * n + 4


def jacobi_bytes(n, nnz):
    return 12 * nnz + 36 * n + 4


def residual_bytes(n, nnz):
    return 12 * nnz + 28 * n + 4


def pmc_traffic(kernel="spmv", grid=512):
    """HBM/fabric bytes per launch of the dominant kernel from the newest committed rocprofv3 PMC
    summary (profiles/*_summary.json: FETCH_SIZE/WRITE_SIZE in separate passes, corrected as
    MI355X_MICROARCH.md §HBM prescribes).  None if no summary matches this grid."""
    best = pmc_summary(grid)
    if not best:
        return None
    for r in best[0]["fine_level_kernels"]:
        if r["kernel"] == kernel:
            return (r["traffic_bytes"], best[1])
    return None


def kernel_source_sha():
    """identity of the row-block kernels' source (csrc/kernels_spmv.hip): a PMC summary applies to this build only if it was taken on the same text"""
    import hashlib
    try:
        return hashlib.sha256(open(os.path.join(REPO, "multigridsolver_amd", "csrc", "kernels_spmv.hip"), "rb").read()).hexdigest()[:16]
    except OSError:
        return None


def pmc_summary(grid=512):
    """newest committed profile summary for this grid THAT WAS TAKEN ON THIS BUILD'S KERNEL SOURCE (its `kernel_source_sha` equals
    kernel_source_sha(); the GPU box has no git history to ask): (dict, file name) or None — a summary of older kernels never mixes its
    bytes with this run's times (advisor, round 3)"""
    import glob
    best, sha = None, kernel_source_sha()
    for f in sorted(glob.glob(os.path.join(REPO, "profiles", "*_summary.json"))):
        try:
            d = json.load(open(f))
            if d.get("grid") == grid and d.get("fine_level_kernels") and sha and d.get("kernel_source_sha") == sha:
                best = (d, os.path.basename(f))
        except Exception:  # noqa: BLE001
            pass
    return best


def optin_value_patterns(mg, args, N):
    """NOT the headline: the same cycle with the opt-in option valcode = 1 (pattern tuples carry the values, coded row
    blocks stream no matrix entry).  It pays only because this synthetic operator has constant coefficients — a
    variable-coefficient operator falls back to the default path — so it is reported beside `value`, never as it."""
    ctx = mg.Context(0)
    try:
        ctx.set_option("valcode", 1)
        n = N ** 3
        A = ctx.poisson3d(N)
        h = mg.Hierarchy(A, args.omega, args.nu1, args.nu2).coarsen(args.ktg, args.npass, args.tou, args.coarse_rows, 32).finalize()
        b = ctx.vec(n).rand(seed=0); x = ctx.vec(n); xs = ctx.vec(n).rand(seed=1); y = ctx.vec(n)
        for _ in range(3):
            h.vcycle(b, x)
        A.time_kernel(mg.OP_SPMV, xs, out=y, reps=3)
        ms_spmv = A.time_kernel(mg.OP_SPMV, xs, out=y, reps=args.kernel_reps)
        ms_cycle = h.time_vcycle(b, x, reps=args.steps)
        code = A.rowcode_info()
        out = {"option": "valcode=1 (opt-in, off by default)", "vcycles_per_s": 1e3 / ms_cycle, "ms_per_vcycle": ms_cycle, "spmv_ms": ms_spmv,
               "spmv_streamed_bytes": 17 * n + n // 16 + 12 * code["table_ints"] + 8 * (code["blocks"] + 1),
               "coded_row_blocks": code["coded_blocks"], "row_blocks": code["blocks"],
               "note": "same bits as the default path (tests/test_gpu_parity.py::test_value_pattern_coding_bit_identical); benefits only operators "
                       "whose rows repeat index shape AND values (constant / piecewise-constant coefficients)"}
        del h, A, b, x, xs, y
        return out
    finally:
        ctx.close()


def bundled_cases(mg, args):
    """V-cycles/s on the reference's bundled operators (BASELINE.json configs[1..2]; cache-resident,
    launch-latency bound — reported as time, not as an HBM fraction)."""
    import gzip
    import shutil
    import tempfile
    inp = os.path.join(REPO, "tests", "golden", "inputs")
    out = {}
    ctx = mg.Context(0)
    tmp = tempfile.mkdtemp(prefix="mgs_bench_")
    try:
        cases = []
        pP = os.path.join(inp, "poisson10000promatrix.mtx")
        if os.path.exists(pP):
            cases.append(("poisson10000 + bundled promatrix (configs[1])", ctx.poisson2d(100), pP))
        gz = os.path.join(inp, "CSky3d30.mtx.gz")
        if os.path.exists(gz):
            path = os.path.join(tmp, "CSky3d30.mtx")
            with gzip.open(gz, "rb") as f, open(path, "wb") as g:
                shutil.copyfileobj(f, g)
            A3 = mg.Csr.from_mtx(ctx, path)
            cases.append(("CSky3d30 + P from the reference CPU setup", A3, os.path.join(inp, "CSky3d30promatrix_cpu.mtx")))
            cases.append(("CSky3d30, hierarchy aggregated on device (configs[2])", A3, None))
        for name, A, Ppath in cases:
            h = mg.Hierarchy(A, args.omega, args.nu1, args.nu2)
            if Ppath:
                h.push_P(mg.Csr.from_mtx(ctx, Ppath))
            h.coarsen(args.ktg, args.npass, args.tou, args.coarse_rows, 32).finalize()
            n = A.shape[0]
            b = ctx.vec(n).rand(seed=0); x = ctx.vec(n)
            h.time_vcycle(b, x, reps=20)
            ms = min(h.time_vcycle(b, x, reps=200) for _ in range(3))
            xs = ctx.vec(n)
            mg.bicgstab(A, xs, b, h, 2000, 1e-10)          # warm (graph capture)
            xs.fill(0.0); ctx.sync()
            t0 = time.perf_counter()
            st, it, tol = mg.bicgstab(A, xs, b, h, 2000, 1e-10)
            t_solve = time.perf_counter() - t0
            out[name] = {"rows": n, "nnz": A.nnz, "levels": [h.level_shape(l)[0] for l in range(h.nlev)], "ms_per_vcycle": ms,
                         "vcycles_per_s": 1e3 / ms, "bicgstab_iterations_to_1e-10": it, "bicgstab_status": st, "achieved_tol": tol,
                         "bicgstab_solve_ms": t_solve * 1e3}
            del h, b, x, xs
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        ctx.close()
    return out


def convdiff_leg(mg, args, N=256):
    """The reference's own problem class at scale (VERDICT r3 items 4 and Weak #6): the nonsymmetric, variable-coefficient convection-diffusion
    family of its bundled `matrices/CSky3d30.mtx` (multigridsolver_amd/synthetic.py `csky3d`: constant strong upwind convection, periodic cubes
    of 1e3..9e3 times the background diffusion; at N = 30 the generator reproduces the bundled file bit for bit, tests/test_synthetic.py — the 80^3
    member the reference names is absent from its checkout; at N != 30 with the bundled file's row-sum margin, `rowsum_floor`, without which the
    reference's pair rule finds nothing to pair), N^3 rows built on the host and uploaded once.  Untimed region of the bench: kernel and
    cycle time per million rows beside the constant-coefficient Poisson figures, and BiCGSTAB + V-cycle against FGCR(10) + K-cycle in the
    paper's GCR form on every level below the finest (the paper's setting: W-cycle cost while the coarsening ratio stays near 4), three
    right-hand sides, true residuals recomputed."""
    from multigridsolver_amd.synthetic import csky3d, CSKY_ROWSUM_MARGIN
    t0 = time.perf_counter()
    rp, ci, v = csky3d(N, rowsum_floor=CSKY_ROWSUM_MARGIN)
    t_gen = time.perf_counter() - t0
    n = N ** 3
    ctx = mg.Context(0)
    try:
        A = ctx.csr(n, n, rp, ci, v)
        nnz = A.nnz
        del rp, ci, v
        t0 = time.perf_counter()
        h = mg.Hierarchy(A, args.omega, args.nu1, args.nu2).coarsen(args.ktg, args.npass, args.tou, args.coarse_rows, 32).finalize()
        ctx.sync(); t_setup = time.perf_counter() - t0
        levels = [h.level_shape(l) for l in range(h.nlev)]
        b = ctx.vec(n).rand(seed=0); x = ctx.vec(n); xs = ctx.vec(n).rand(seed=1); y = ctx.vec(n)
        A.optimize()
        code = A.rowcode_info()
        A.time_kernel(mg.OP_SPMV, xs, out=y, reps=3)
        ms_spmv = A.time_kernel(mg.OP_SPMV, xs, out=y, reps=20)
        for _ in range(3):
            h.vcycle(b, x)
        ms_cycle = h.time_vcycle(b, x, reps=20)
        runs = []
        # K-cycle levels: every level below the finest while the hierarchy coarsens by >= 3 per level (a K step visits the next level twice: the
        # cost stays that of a W-cycle, sum (2/ratio)^l); a hierarchy that coarsens more slowly keeps K to the levels a sharded run keeps sharded
        ratios = [levels[l - 1][0] / levels[l][0] for l in range(1, h.nlev)]
        klev = h.nlev - 2 if (h.nlev > 2 and min(ratios[:-1]) >= 3.0) else max(1, sum(1 for l in range(1, h.nlev - 1) if levels[l][0] >= 600000))
        for seed in (0, 1, 2):
            bk = b if seed == 0 else ctx.vec(n).rand(seed=100 + seed)
            nb = bk.nrm2()
            xk = ctx.vec(n); ctx.sync(); t0 = time.perf_counter()
            st, it, tol = mg.bicgstab(A, xk, bk, h, 1000, 1e-10)
            t_b = time.perf_counter() - t0
            true_b = A.residual(xk, bk).nrm2() / nb
            run = {"rhs_seed": seed, "bicgstab_vcycle": {"status": st, "iterations": it, "seconds": t_b, "true_residual": true_b}}
            h.set_kcycle(klev)
            for name, fn in (("fgcr10_kcycle_gcr", lambda: mg.fgcr(A, xk, bk, h, 10, 300, 1e-10)),
                             ("bicgstab_kcycle_gcr", lambda: mg.bicgstab(A, xk, bk, h, 300, 1e-10))):
                xk.fill(0.0); ctx.sync(); t0 = time.perf_counter()
                stk, itk, tolk = fn()
                t_k = time.perf_counter() - t0
                run[name] = {"status": stk, "iterations": itk, "max_iterations": 300, "seconds": t_k, "true_residual": A.residual(xk, bk).nrm2() / nb}
            h.set_kcycle(0)
            runs.append(run)
            del xk
        h.set_kcycle(klev)
        ms_kcycle = h.time_vcycle(b, x, reps=5)
        h.set_kcycle(0)
        out = {"operator": f"csky3d_{N}^3 (nonsymmetric upwind convection-diffusion of the reference's CSky3d family: v = (1000,1000,1000), diffusion cubes 1e3..9e3; "
                           "the generator gives the bundled CSky3d30.mtx bit for bit at N = 30; here with that file's row-sum margin 2.86e-6 a_ii on interior rows; host-built, uploaded once)",
               "rows": n, "nnz": nnz, "levels": levels, "host_generation_seconds": t_gen, "setup_seconds": t_setup,
               "coded_row_blocks": code["coded_blocks"], "row_blocks": code["blocks"],
               "spmv_ms": ms_spmv, "spmv_us_per_million_rows": ms_spmv * 1e3 / (n / 1e6), "spmv_effective_csr_gbps": spmv_bytes(n, nnz) / (ms_spmv * 1e-3) / 1e9,
               "vcycle_ms": ms_cycle, "vcycle_us_per_million_rows": ms_cycle * 1e3 / (n / 1e6),
               "kcycle_levels": klev, "kcycle_ms": ms_kcycle, "runs": runs,
               "coarsening_ratios": ratios,
               "note": "K-cycle in the paper's GCR form (nonsymmetric operator: the energy form of the Poisson leg is for SPD operators only) on every level below the "
                       "finest: the hierarchy coarsens 4x per level, so the K-cycle costs about what a W-cycle costs.  Iterations to 1e-10 at 128^3 / 256^3 / 512^3: BiCGSTAB + V "
                       "61 / 107-117 / 208-212; FGCR(10) + K 36 / 43 / no convergence in 300 (restarted GCR stagnates at 0.77); BiCGSTAB + K (a nonlinear preconditioner "
                       "inside BiCGSTAB: outside the theory) 21 / 31-45 / 65-69 with one of three right-hand sides not converging.  In seconds the two are level at 256^3 "
                       "(BiCGSTAB + V 0.29-0.36 s, FGCR(10) + K 0.31 s since the K-cycle's coarse levels replay from one graph) and BiCGSTAB + V wins at 512^3 (3.8 s against 4.4 s): "
                       "with the reference's Jacobi smoother and plain pairwise aggregates the K-cycle lowers the iteration count but is not mesh-independent on this class.  K on the top 1-2 levels only does not converge inside FGCR(10) at 256^3 "
                       "(tools/convdiff_scan.py; profiles/r04_csky_scan.md).  Cycle-vs-oracle parity on nonsymmetric operators: "
                       "tests/test_gpu_parity.py::test_kcycle_vs_oracle_at_128 and ::test_c4_shaped_standin_three_level_vcycle, bundled CSky operators in "
                       "::test_bundled_operators_vs_reference_golden"}
        del h, A, b, x, xs, y
        return out
    finally:
        ctx.close()


def _oracle_sample(mg, orc, args, Ns, min_cycles, min_seconds, keep_fine=False):
    """one CPU sample: the hierarchy the device builds for the Ns^3 grid, downloaded once, the oracle's cycle timed on it
    (1 thread) and compared with the GPU cycle on the same right-hand side"""
    ctx = mg.Context(0)
    try:
        A = ctx.poisson3d(Ns)
        h = mg.Hierarchy(A, args.omega, args.nu1, args.nu2).coarsen(args.ktg, args.npass, args.tou, args.coarse_rows, 32).finalize()
        As, Ps = [], []
        for l in range(h.nlev):
            rp, ci, v = h.level_A(l).download()
            rows = h.level_shape(l)[0]
            As.append(orc.Csr.from_arrays(rows, rows, rp, ci, v))
            del rp, ci, v
            if l < h.nlev - 1:
                T = h.level_P(l); agg = T.agg(); nf, nc = T.shape
                has = agg >= 0                                            # P in CSR straight from the aggregate map: row i holds (agg_i, 1.0)
                prp = np.zeros(nf + 1, dtype=np.int32); np.cumsum(has, out=prp[1:])
                Ps.append(orc.Csr.from_arrays(nf, nc, prp, agg[has], np.ones(int(prp[-1]))))
                del agg, has, prp
        n = Ns ** 3
        b = ctx.vec(n).rand(seed=0).numpy()
        ho = orc.Hier(As[0], Ps, omega=args.omega, nu1=args.nu1, nu2=args.nu2, As=As)
        ho.vcycle(b)  # warm-up (first touch of the work vectors)
        reps, t0 = 0, time.perf_counter()
        while reps < min_cycles or time.perf_counter() - t0 < min_seconds:
            x = ho.vcycle(b); reps += 1
        t_cycle = (time.perf_counter() - t0) / reps
        # the same cycle with the oracle's row loops on the host cores this job may use (rows are independent: same bits, checked below)
        nmax = max(1, min(int(os.environ.get("MGS_CPU_THREADS", "64")), len(os.sched_getaffinity(0))))
        t_all, x_all, nthr, tried = None, None, 1, {}
        try:
            for cand in sorted({min(16, nmax), nmax} - {1}):      # more threads than memory channels can lose: keep the better of 16 and all
                got = orc.set_threads(cand)
                ho.vcycle(b)                    # thread team start-up
                r2, t0 = 0, time.perf_counter()
                while r2 < min_cycles or time.perf_counter() - t0 < min_seconds / 3:
                    xc = ho.vcycle(b); r2 += 1
                tc = (time.perf_counter() - t0) / r2
                tried[got] = tc * 1e3
                if t_all is None or tc < t_all:
                    t_all, x_all, nthr = tc, xc, got
        finally:
            orc.set_threads(1)
        # parity of this very sample against the GPU cycle (cheap, keeps the baseline honest)
        xg = h.vcycle(ctx.vec(b)).numpy()
        err = float(np.linalg.norm(xg - x) / np.linalg.norm(x))
        out = {"grid": Ns, "rows": n, "levels": h.nlev, "cycles": reps, "ms_per_cycle": t_cycle * 1e3, "gpu_vs_oracle_rel_err": err}
        if keep_fine and h.nlev >= 6:
            # the K-cycle the solve leg runs (levels 1-4, energy coefficients) against the oracle's K-cycle AT THIS SIZE, same right-hand side
            # (round-3 review: the benched size had no oracle comparison); the oracle's row loops on the host cores, its inner products sequential
            try:
                ctx.set_option("kcycle_energy", 1); h.set_kcycle(4); ho.set_kcycle_energy(1).set_kcycle(4)
                orc.set_threads(nthr if t_all is not None else 1)
                t0 = time.perf_counter(); xko = ho.vcycle(b); t_ko = time.perf_counter() - t0
                xkg = h.vcycle(ctx.vec(b)).numpy()
                out["kcycle4_energy"] = {"gpu_vs_oracle_rel_err": float(np.linalg.norm(xkg - xko) / np.linalg.norm(xko)), "oracle_seconds": t_ko,
                                         "oracle_threads": nthr if t_all is not None else 1}
            finally:
                orc.set_threads(1); ctx.set_option("kcycle_energy", 0); h.set_kcycle(0); ho.set_kcycle_energy(0).set_kcycle(0)
        if t_all is not None:
            out["all_cores"] = {"threads": nthr, "ms_per_cycle": t_all * 1e3, "same_bits_as_one_thread": bool(np.array_equal(x_all, x)), "ms_per_cycle_by_threads": tried}
        del h, A, ho
        return out, (As[0] if keep_fine else None)
    finally:
        ctx.close()


def cpu_baseline(mg, args):
    """CPU oracle V-cycle (port of the same cycle, 1 thread) AT THE BENCHED SIZE: the hierarchy the device builds for the
    args.grid^3 operator is downloaded once and >= 2 oracle cycles are timed on it — no scale factor.  A 256^3 sample is kept as
    a cross-check of the row scaling.  The reference's own Eigen SpMV kernel (oracle/_ref/libref_eigen*.so) is timed on the
    benched fine operator too, on 1 thread (how the reference ships) and on the host cores of this job."""
    from oracle import oracle_py as orc
    Ns = args.cpu_grid if args.cpu_grid > 0 else args.grid
    full, A0 = _oracle_sample(mg, orc, args, Ns, 2, 6.0 if Ns >= 384 else 12.0, keep_fine=True)
    scale = (args.grid / Ns) ** 3
    n = Ns ** 3
    out = {"value": 1.0 / (full["ms_per_cycle"] * 1e-3 * scale), "unit": "V-cycles/s", "cores": 1, "kind": "port",
           "sample": f"oracle V({args.nu1},{args.nu2}) cycle on the {Ns}^3 grid ({n} rows, {full['levels']} levels built on device, downloaded once), "
                     f"{full['cycles']} cycles of {full['ms_per_cycle']:.1f} ms after one warm-up cycle"
                     + ("" if scale == 1.0 else f", scaled by the row ratio x{scale:.0f} to {args.grid}^3"),
           "sample_ms_per_cycle": full["ms_per_cycle"], "gpu_vs_oracle_rel_err_on_sample": full["gpu_vs_oracle_rel_err"],
           "kcycle4_energy_on_sample": full.get("kcycle4_energy")}
    if full.get("all_cores"):
        # the whole CYCLE (not only its SpMV) on every host core this job may use: the box gives a 1-GPU job 16 of the host's hardware threads
        # (os.sched_getaffinity), which is the cap stated here; value stays the 1-thread figure (how the reference ships: no -fopenmp)
        ac = full["all_cores"]
        out["vcycle_all_cores"] = {"value": 1.0 / (ac["ms_per_cycle"] * 1e-3 * scale), "unit": "V-cycles/s", "cores": ac["threads"], "ms_per_cycle": ac["ms_per_cycle"],
                                   "same_bits_as_one_thread": ac["same_bits_as_one_thread"], "ms_per_cycle_by_threads": ac.get("ms_per_cycle_by_threads"),
                                   "note": "oracle cycle with its row loops (SpMV, residual, Jacobi, prolongation add) on all CPUs of this job's affinity mask"}
    if Ns > 256 and not args.no_cpu_cross:
        try:       # cross-check of the row scaling the earlier rounds reported (256^3 x 8)
            cross, _ = _oracle_sample(mg, orc, args, 256, 3, 3.0)
            cross["scaled_to_benched_grid_vcycles_per_s"] = 1.0 / (cross["ms_per_cycle"] * 1e-3 * (Ns / 256) ** 3)
            out["cross_check_256"] = cross
        except Exception as e:  # noqa: BLE001
            out["cross_check_256"] = {"error": repr(e)}
    # reference's own SpMV kernel (Eigen 3.3.4) on the benched fine operator
    so = os.path.join(REPO, "oracle", "_ref", "libref_eigen.so")
    rp, ci, v = A0.rowptr, A0.col, A0.val
    nnz = len(ci)
    out["spmv_sample"] = f"{Ns}^3 fine operator ({n} rows, {nnz} nnz)"
    xs = np.random.default_rng(0).random(n); y = np.empty(n)
    if os.path.exists(so):
        L = C.CDLL(so)
        L.ref_eigen_spmv.restype = C.c_double
        L.ref_eigen_spmv.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        t = L.ref_eigen_spmv(n, n, nnz, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, xs.ctypes.data, y.ctypes.data, 3)
        out["spmv_eigen_reference_gbps"] = spmv_bytes(n, nnz) / t / 1e9
        out["spmv_eigen_reference_ms"] = t * 1e3
    so_omp = os.path.join(REPO, "oracle", "_ref", "libref_eigen_omp.so")
    if os.path.exists(so_omp):
        try:   # all host cores this job may use (os.sched_getaffinity: 64 of the 256 hardware threads on the boxes seen so far)
            nmax = max(1, min(int(os.environ.get("MGS_CPU_THREADS", "64")), len(os.sched_getaffinity(0))))     # the same cap as the oracle's all-cores cycle
            L2 = C.CDLL(so_omp)
            L2.ref_eigen_spmv.restype = C.c_double
            L2.ref_eigen_spmv.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
            best, by = None, {}
            for cand in sorted({min(16, nmax), nmax}):       # the better of 16 threads and every CPU of the affinity mask
                L2.ref_eigen_set_threads(cand)
                t = L2.ref_eigen_spmv(n, n, nnz, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, xs.ctypes.data, y.ctypes.data, 5)
                by[int(L2.ref_eigen_threads())] = spmv_bytes(n, nnz) / t / 1e9
                if best is None or t < best[0]:
                    best = (t, int(L2.ref_eigen_threads()))
            out["spmv_eigen_reference_all_cores_gbps"] = spmv_bytes(n, nnz) / best[0] / 1e9
            out["spmv_eigen_reference_all_cores_threads"] = best[1]
            out["spmv_eigen_reference_gbps_by_threads"] = by
        except Exception as e:  # noqa: BLE001
            out["spmv_eigen_reference_all_cores_error"] = repr(e)
    t0 = time.perf_counter()
    for _ in range(3):
        A0.spmv(xs)
    t = (time.perf_counter() - t0) / 3
    out["spmv_oracle_port_gbps"] = spmv_bytes(n, nnz) / t / 1e9
    try:
        out["host_cpu"] = [l.split(":")[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
        out["host_nproc"] = os.cpu_count()
    except Exception:  # noqa: BLE001
        pass
    return out


_REAL_STDOUT = None


def emit_json(obj):
    """the ONE JSON line, written to the process's original stdout"""
    line = (json.dumps(obj) + "\n").encode()
    if _REAL_STDOUT is not None:
        os.write(_REAL_STDOUT, line)
    else:
        sys.stdout.write(line.decode()); sys.stdout.flush()


DUMP_MAX_BYTES = 64 << 20
DUMP_SAMPLE_ROWS = 1 << 20


def dump_outputs(d, x):
    """the timed path's result (x = M^-1 b of the last step) as float64 .npy files under d: the whole vector when it fits in
    DUMP_MAX_BYTES, else DUMP_SAMPLE_ROWS rows at indices drawn with a fixed seed (the same rows for the same grid in every run)"""
    os.makedirs(d, exist_ok=True)
    xh = np.ascontiguousarray(x, dtype=np.float64)
    if xh.nbytes <= DUMP_MAX_BYTES:
        np.save(os.path.join(d, "x.npy"), xh)
        return ["x"]
    idx = np.sort(np.random.default_rng(0).choice(xh.size, DUMP_SAMPLE_ROWS, replace=False))
    np.save(os.path.join(d, "x_sample.npy"), xh[idx])
    np.save(os.path.join(d, "x_sample_index.npy"), idx.astype(np.float64))
    return ["x_sample", "x_sample_index"]


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps (V-cycles); >= 1")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true", help="also run every leg beside the headline (roofline kernel timings, unfused A/B, solve checks, "
                                                         "bundled operators, convection-diffusion, CPU baseline); off: headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's result as DIR/<name>.npy (one GPU only)")
    ap.add_argument("--grid", type=int, default=512, help="N of the N^3 7-point Poisson grid (headline: 512)")
    ap.add_argument("--omega", type=float, default=0.6)
    ap.add_argument("--nu1", type=int, default=1)
    ap.add_argument("--nu2", type=int, default=1)
    ap.add_argument("--ktg", type=float, default=10.0)
    ap.add_argument("--npass", type=int, default=2)
    ap.add_argument("--tou", type=float, default=8.0)
    ap.add_argument("--coarse-rows", type=int, default=2500)
    ap.add_argument("--cpu-grid", type=int, default=0, help="grid of the CPU-baseline sample (oracle V-cycle, 1 thread); 0 = the benched grid itself (no scale factor)")
    ap.add_argument("--no-cpu-cross", action="store_true", help="skip the 256^3 cross-check sample of the CPU baseline")
    ap.add_argument("--optin", action="store_true", help="also run the opt-in value-pattern leg (valcode=1; builds a second hierarchy; never the headline)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-convdiff", action="store_true", help="skip the 256^3 convection-diffusion leg (untimed solve comparison)")
    ap.add_argument("--convdiff-grid", type=int, default=256)
    ap.add_argument("--kernel-reps", type=int, default=20)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.gpus != 1:
        ap.error("--dump-outputs is supported with --gpus 1 only")
    return args


def main():
    args = parse_args()
    # ---- launch: N > 1 ranks are CHILD processes of a supervisor that never touches the GPU (multigridsolver_amd/launch.py)
    if os.environ.get("MGS_BENCH_WORKER") != "1":
        from multigridsolver_amd import launch
        world_env = int(os.environ.get("WORLD_SIZE", "1"))
        if world_env > 1:                                   # under torch.distributed.run: one supervisor per rank slot
            if args.gpus != world_env:
                raise SystemExit(f"--gpus {args.gpus} but the launcher started {world_env} ranks")
            sys.exit(launch.supervise_rank(sys.argv, log))
        if args.gpus > 1:                                   # plain `python bench.py --gpus N`: start the ranks ourselves
            sys.exit(launch.spawn_ranks(sys.argv, args.gpus, log))
    # Libraries print banners on fd 1 (RCCL: "RCCL version : ...", Gloo: "[Gloo] Rank ..."); keep stdout
    # clean for the one JSON line by pointing fd 1 at stderr for everything else.
    global _REAL_STDOUT
    sys.stdout.flush()
    _REAL_STDOUT = os.dup(1)
    os.dup2(2, 1)

    # One device-memory arena per process (mgs_arena_reserve / MGS_ARENA_GB): the library places every operator and vector inside one
    # hipMalloc, at the same offsets in every process — the fine-level SpMV then repeats to ±1 % from process to process instead of ±3–4 %
    # (profiles/r03_spread.md).  Sized for the benched grid and this rank's share; MGS_ARENA_GB=0 switches it off.
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    os.environ.setdefault("MGS_ARENA_GB", str(int(min(110.0, 110.0 * (args.grid / 512.0) ** 3 / max(world_env, 1) + 6.0))))

    import torch
    import multigridsolver_amd as mg

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE is {world}")
    if world > 1 or os.environ.get("MGS_FORCE_SHARDED"):   # MGS_FORCE_SHARDED: rehearse the sharded code path on one rank
        if args.dump_outputs:
            raise SystemExit("--dump-outputs is supported on the unsharded one-GPU path only")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29755")
        os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
        from multigridsolver_amd import dist as mgdist
        args.no_cpu_cross = True        # N > 1: the run's time budget (launch.py) goes to transport generations, not to a second oracle sample
        return mgdist.bench_sharded(args, rank, world, local_rank, log, spmv_bytes, emit_json,
                                    cpu_baseline=None if (args.no_cpu or not args.full) else (lambda: cpu_baseline(mg, args)),
                                    pmc_traffic=pmc_traffic)
    torch.cuda.set_device(local_rank)

    ctx = mg.Context(local_rank)
    N = args.grid
    n = N ** 3
    t0 = time.perf_counter()
    A = ctx.poisson3d(N)
    ctx.sync()
    nnz = A.nnz
    log(f"generated {N}^3 operator on device: {n} rows, {nnz} nnz in {time.perf_counter() - t0:.2f}s")
    t0 = time.perf_counter()
    h = mg.Hierarchy(A, args.omega, args.nu1, args.nu2).coarsen(args.ktg, args.npass, args.tou, args.coarse_rows, 32).finalize()
    ctx.sync()
    t_setup = time.perf_counter() - t0
    levels = [h.level_shape(l) for l in range(h.nlev)]
    log(f"hierarchy built on device in {t_setup:.2f}s: " + " > ".join(f"{r}r/{z}nnz" for r, z in levels))
    plans = [h.level_A(l).plan_info() for l in range(h.nlev)]
    log("level plans (max_block_nnz/max_row/far_band/lds): " + " ".join(f"{p['max_block_nnz']}/{p['max_row_len']}/{p['far_band']}/{p['lds_bytes']}" for p in plans[:5]))

    b = ctx.vec(n).rand(seed=0)
    x = ctx.vec(n)
    # ---- roofline of the dominant kernel: fine-level CSR SpMV (HIP events on the kernel's stream), --full only.  A plain run makes the
    # same allocations and the same pattern code in the same order without the timed launches: the arena then places the cycle's operands
    # where a --full run places them, so the headline is the same figure in both (placement moves a kernel by a few %, profiles/r03_spread.md)
    xs = ctx.vec(n).rand(seed=1)
    y = ctx.vec(n)
    dinv = A.diag_inv()
    # plain CSR kernel first (12 B per entry streamed), then the shipped path: pattern-coded column index
    # (mgs_csr_optimize: 8 B per entry + 1 B per row streamed; same products, same bits)
    ctx.set_option("rowcode", 0)
    if args.full:
        A.time_kernel(mg.OP_SPMV, xs, out=y, reps=3)
        ms_spmv_csr = A.time_kernel(mg.OP_SPMV, xs, out=y, reps=args.kernel_reps)
    ctx.set_option("rowcode", 1)
    A.optimize()
    code = A.rowcode_info()
    streamed = (8 * nnz + 17 * n + n // 16 + 4 * code["table_ints"] + 4 * (code["blocks"] + 1) * 2) if code["coded_blocks"] == code["blocks"] else None
    gbps = lambda byts, ms: byts / (ms * 1e-3) / 1e9  # noqa: E731
    if args.full:
        A.time_kernel(mg.OP_SPMV, xs, out=y, reps=3)
        ms_spmv = A.time_kernel(mg.OP_SPMV, xs, out=y, reps=args.kernel_reps)
        ms_res = A.time_kernel(mg.OP_RESIDUAL, xs, b=b, out=y, reps=args.kernel_reps)
        ms_jac = A.time_kernel(mg.OP_JACOBI, xs, b=b, dinv=dinv, out=y, reps=args.kernel_reps)
        spmv_gbps = gbps(spmv_bytes(n, nnz), ms_spmv)
        log(f"fine SpMV, plain CSR kernel {ms_spmv_csr:.3f} ms = {gbps(spmv_bytes(n, nnz), ms_spmv_csr):.0f} GB/s; pattern-coded: streams "
            f"{(streamed or 0) / 1e9:.2f} GB of the {spmv_bytes(n, nnz) / 1e9:.2f} algorithmic GB")
        log(f"fine SpMV {ms_spmv:.3f} ms = {spmv_gbps:.0f} GB/s; residual {ms_res:.3f} ms = {gbps(residual_bytes(n, nnz), ms_res):.0f} GB/s; "
            f"jacobi {ms_jac:.3f} ms = {gbps(jacobi_bytes(n, nnz), ms_jac):.0f} GB/s")
    del xs, y

    # the first cycle builds the setup-time operands of the fused passes (Â = A·diag(ωD⁻¹), A·P, pattern codes, row-block groups):
    # setup work, reported beside setup_seconds, outside the timed region
    t0 = time.perf_counter()
    h.vcycle(b, x)
    ctx.sync()
    t_operands = time.perf_counter() - t0
    log(f"first cycle incl. operand setup: {t_operands:.2f}s")
    # ---- timed region: W warm-up + exactly K V-cycles
    for _ in range(args.warmup):
        h.vcycle(b, x)
    ctx.sync(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        h.vcycle(b, x)
    ctx.sync(); torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    ms_step = elapsed / args.steps * 1e3
    log(f"V-cycle {ms_step:.3f} ms ({args.steps / elapsed:.2f} /s)")
    if args.dump_outputs:          # before any other leg touches x
        names = dump_outputs(args.dump_outputs, x.numpy())
        log(f"outputs of the last timed step written to {args.dump_outputs}: " + ", ".join(names))
    out = {
        "metric": "V-cycles/sec + fine-level SpMV HBM GB/s, 512³ 7-pt Poisson, 1/2/4/8 GPU",
        "value": args.steps / elapsed, "unit": "V-cycles/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms_step, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
        "data": "synthetic", "full": args.full,
        "config": {"workload": f"poisson3d_{N}^3_7pt (BASELINE.json configs[4]); V({args.nu1},{args.nu2}) damped-Jacobi cycle, omega={args.omega}, "
                               f"hierarchy built on device by pairwise aggregation ktg={args.ktg} npass={args.npass} tou={args.tou}",
                   "grid": N, "rows": n, "nnz": nnz, "levels": levels, "parallelism": "1 GPU", "setup_seconds": t_setup,
                   "first_cycle_seconds_incl_operand_setup": t_operands, "device_arena_gb": float(os.environ.get("MGS_ARENA_GB", "0"))},
    }
    if not args.full:
        del h, A, b, x, dinv
        ctx.close()
        emit_json(out)
        return
    vbytes = h.vcycle_bytes

    # A/B inside the same process: the unfused one-kernel-per-step form of the same cycle
    ctx.set_option("fuse", 0)
    for _ in range(2):
        h.vcycle(b, x)
    ms_unfused = h.time_vcycle(b, x, reps=max(3, args.steps // 2))
    ctx.set_option("fuse", 1)
    h.vcycle(b, x)
    log(f"unfused form of the same cycle: {ms_unfused:.3f} ms")

    # quality: residual reduction of one cycle and a preconditioned solve to 1e-10 (untimed)
    r0 = b.nrm2(); r1 = A.residual(x, b).nrm2()
    xsol = ctx.vec(n)
    t0 = time.perf_counter()
    st, it, tol = mg.bicgstab(A, xsol, b, h, 200, 1e-10)
    t_solve = time.perf_counter() - t0
    log(f"one cycle: |r|/|b| = {r1 / r0:.3e}; BiCGSTAB+V-cycle to 1e-10: status {st}, {it} iterations, tol {tol:.2e}, {t_solve:.2f}s")
    # the same solve with the two knobs the reference does not have turned for this operator: ω = 0.8 and over-correction σ = 1.6
    # (x ← x + σ·P e_c, mgs_hier_set_correction_scale); reported beside the default (ω = 0.6, σ = 1 = the reference's form), never instead
    h.set_smoother(0.8, args.nu1, args.nu2).set_correction_scale(1.6)
    xt = ctx.vec(n); h.vcycle(b, xt); xt.fill(0.0); ctx.sync()
    t0 = time.perf_counter()
    stt, itt, tolt = mg.bicgstab(A, xt, b, h, 200, 1e-10)
    t_solve_t = time.perf_counter() - t0
    truet = A.residual(xt, b).nrm2() / r0
    h.set_smoother(args.omega, args.nu1, args.nu2).set_correction_scale(1.0)
    h.vcycle(b, x)                                            # back on the default knobs (operands rescaled, cycle re-captured)
    log(f"tuned knobs (omega 0.8, over-correction 1.6): status {stt}, {itt} iterations, true residual {truet:.2e}, {t_solve_t:.2f}s")
    del xt
    # K-cycle on the first 4 coarse levels (energy / flexible-CG coefficients, option kcycle_energy: this operator is SPD) + flexible
    # GCR(10) (derived from the paper, parity unpinned), three right-hand sides, untimed region as well.  mgs_fgcr reports
    # status 0 only with the TRUE residual below the tolerance; it is recomputed here once more.
    ctx.set_option("kcycle_energy", 1)
    h.set_kcycle(4)
    xk = ctx.vec(n)
    ms_kcycle = h.time_vcycle(b, xk, reps=3)
    kruns = []
    for seed in (0, 1, 2):
        bk = b if seed == 0 else ctx.vec(n).rand(seed=100 + seed)
        xk.fill(0.0); ctx.sync()
        t0 = time.perf_counter()
        stk, itk, tolk = mg.fgcr(A, xk, bk, h, 10, 300, 1e-10)
        t_solve_k = time.perf_counter() - t0
        kruns.append({"rhs_seed": seed, "status": stk, "iterations": itk, "reported_tol": tolk, "true_residual": A.residual(xk, bk).nrm2() / bk.nrm2(),
                      "seconds": t_solve_k})
        del bk
    # the same with the smoother's damping the reference's own two-grid tests also run (omega = 0.8, tests/golden jac2grid_w08): beside the default, never instead
    h.set_smoother(0.8, args.nu1, args.nu2)
    h.vcycle(b, xk)
    kruns08 = []
    for seed in (0, 1, 2):
        bk = b if seed == 0 else ctx.vec(n).rand(seed=100 + seed)
        xk.fill(0.0); ctx.sync()
        t0 = time.perf_counter()
        stk, itk, tolk = mg.fgcr(A, xk, bk, h, 10, 300, 1e-10)
        t_solve_k = time.perf_counter() - t0
        kruns08.append({"rhs_seed": seed, "status": stk, "iterations": itk, "true_residual": A.residual(xk, bk).nrm2() / bk.nrm2(), "seconds": t_solve_k})
        del bk
    h.set_smoother(args.omega, args.nu1, args.nu2)
    h.set_kcycle(0)
    ctx.set_option("kcycle_energy", 0)
    h.vcycle(b, x)
    log("FGCR(10)+K-cycle(4, energy) with omega 0.8: " + "; ".join(f"seed {r['rhs_seed']}: status {r['status']}, {r['iterations']} iterations, {r['seconds']:.2f}s" for r in kruns08))
    log(f"FGCR(10)+K-cycle(4 levels, energy coefficients, {ms_kcycle:.2f} ms per cycle) to 1e-10: " +
        "; ".join(f"seed {r['rhs_seed']}: status {r['status']}, {r['iterations']} iterations, true residual {r['true_residual']:.2e}, {r['seconds']:.2f}s" for r in kruns))
    del xk

    traffic, traffic_src = pmc_traffic("spmv", N) or (None, None)
    # what crosses HBM in one launch of the dominant kernel: the PMC measurement of the committed profile of this build, else the
    # bytes the kernel streams by construction (8 B per entry + 17 B per row: x, y, pattern id; rowptr once per wave; tables), else the CSR byte count (plain CSR kernel)
    phys_bytes = traffic or streamed or spmv_bytes(n, nnz)
    phys_basis = (f"PMC traffic (FETCH_SIZE x2 + WRITE_SIZE, separate passes) of {traffic_src} / this run's ms_per_launch" if traffic else
                  ("bytes the kernel streams by construction / this run's ms_per_launch (no committed PMC summary of THIS kernel source for this grid)" if streamed else
                   "CSR bytes / this run's ms_per_launch (plain CSR kernel)"))
    summ = pmc_summary(N)
    cyc = (summ[0].get("vcycle") if summ else None) or {}
    cyc_bytes = cyc.get("traffic_bytes")
    out.update({
        "spmv_hbm_gbps": gbps(phys_bytes, ms_spmv),
        "spmv_effective_csr_gbps": spmv_gbps,
        # roofline of the dominant kernel = what crosses HBM per second against the 8 TB/s peak.  The SURVEY §8d-d3 figure (CSR bytes /
        # time) is kept under its own name: the pattern-coded kernel never reads the column-index array, so that figure is an
        # effective rate and can exceed the peak.
        "roofline": {"bound": "hbm", "achieved": gbps(phys_bytes, ms_spmv), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": gbps(phys_bytes, ms_spmv) / HBM_PEAK_GBPS, "traffic": traffic, "traffic_source": traffic_src, "basis": phys_basis,
                     "traffic_code_commit": (summ[0].get("code_commit") if summ else None), "kernel_source_sha": kernel_source_sha(),
                     "kernel": "csr_rowblock_coded_kernel<SPMV> (fine level; CSR SpMV with pattern-coded column index)",
                     "ms_per_launch": ms_spmv,
                     "effective_csr_bytes_per_launch": spmv_bytes(n, nnz), "effective_csr_gbps": spmv_gbps, "effective_csr_frac": spmv_gbps / HBM_PEAK_GBPS,
                     "note": "achieved/frac = bytes that cross HBM in one launch / launch time (HIP events on the kernel's stream, this run) / 8 TB/s. "
                             "effective_csr_* = SURVEY §8d-d3 CSR bytes (12·nnz + 20·n + 4) / time: the kernel rebuilds the column index from a per-row-block "
                             "pattern table and streams 8 B per entry + 1 B per row, so fewer bytes cross HBM than that count; csr_kernel = the same "
                             "product with the plain 12 B/entry CSR kernel, which streams all of them",
                     "streamed_bytes_per_launch": streamed, "streamed_gbps": gbps(streamed, ms_spmv) if streamed else None,
                     "csr_kernel": {"ms": ms_spmv_csr, "gbps": gbps(spmv_bytes(n, nnz), ms_spmv_csr), "frac": gbps(spmv_bytes(n, nnz), ms_spmv_csr) / HBM_PEAK_GBPS},
                     "other_kernels": {"residual": {"ms": ms_res, "effective_csr_gbps": gbps(residual_bytes(n, nnz), ms_res)},
                                       "jacobi": {"ms": ms_jac, "effective_csr_gbps": gbps(jacobi_bytes(n, nnz), ms_jac)}},
                     # the cycle: PMC bytes of every dispatch of one cycle in the same profile set (same kernel source, see pmc_summary), over
                     # this run's ms_per_step; the §8d byte count of the cycle's operations beside it as an effective figure
                     "vcycle_hbm_gb": cyc_bytes / 1e9 if cyc_bytes else None,
                     "vcycle_hbm_gbps": cyc_bytes / (ms_step * 1e-3) / 1e9 if cyc_bytes else None,
                     "vcycle_hbm_frac": cyc_bytes / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBPS if cyc_bytes else None,
                     "vcycle_dispatches_in_profile": cyc.get("dispatches"), "vcycle_kernel_ms_in_profile": cyc.get("kernel_ms"),
                     "vcycle_effective_csr_gb": vbytes / 1e9,
                     "vcycle_ms_unfused_form": ms_unfused, "grouped_pre_pass": [h.group_info(l) for l in range(min(h.nlev - 1, 4))]},
        "solve_check": {"one_cycle_residual_reduction": r1 / r0, "bicgstab_status": st, "bicgstab_iterations": it, "bicgstab_tol": tol,
                        "bicgstab_seconds": t_solve,
                        "tuned_omega08_overcorrection16": {"status": stt, "iterations": itt, "true_residual": truet, "seconds": t_solve_t,
                                                            "note": "same V(1,1) cycle with omega = 0.8 and x += 1.6·P e_c (knobs the reference does not have)"},
                        "fgcr10_kcycle4_energy": {"ms_per_kcycle": ms_kcycle, "runs": kruns,
                                                  "spd_only": True,
                                                  "note": "FGCR(10) + K-cycle on levels 1-4 with energy (flexible-CG) coefficients, option kcycle_energy: SYMMETRIC POSITIVE DEFINITE operators only "
                                                          "(the nonsymmetric leg below uses the paper's GCR form); derived from the paper, no reference executable (parity unpinned)"},
                        "fgcr10_kcycle4_energy_omega08": {"runs": kruns08, "spd_only": True,
                                                          "note": "the same solve with the smoother's damping omega = 0.8 (a value the reference's own two-grid tests run; the headline "
                                                                  "cycle and every figure above use the default 0.6); tools/fgcr_knobs.py scans omega x K levels x restart length"}},
    })
    del h, A, b, x, xsol, dinv
    ctx.close()
    if args.optin:       # a second hierarchy for a figure that only constant-coefficient operators see: not part of the default run
        try:
            out["optin_value_patterns"] = optin_value_patterns(mg, args, N)
            log(f"opt-in value patterns (not the headline): {out['optin_value_patterns']['vcycles_per_s']:.1f} V-cycles/s, SpMV {out['optin_value_patterns']['spmv_ms']:.3f} ms")
        except Exception as e:  # noqa: BLE001
            log("opt-in value-pattern leg failed:", repr(e))
    try:
        out["bundled_matrices"] = bundled_cases(mg, args)
    except Exception as e:  # noqa: BLE001
        log("bundled cases failed:", repr(e))
    if not args.no_convdiff:
        try:
            cd = convdiff_leg(mg, args, args.convdiff_grid)
            out["solve_check"][f"convdiff_{args.convdiff_grid}"] = cd
            out["solve_check"][f"convdiff_{args.convdiff_grid}"]["poisson_reference_us_per_million_rows"] = {"spmv": ms_spmv * 1e3 / (n / 1e6), "vcycle": ms_step * 1e3 / (n / 1e6)}
            log(f"convection-diffusion {args.convdiff_grid}^3: SpMV {cd['spmv_us_per_million_rows']:.1f} us/Mrow (Poisson {ms_spmv * 1e3 / (n / 1e6):.1f}), cycle {cd['vcycle_us_per_million_rows']:.1f} "
                f"(Poisson {ms_step * 1e3 / (n / 1e6):.1f}); " + "; ".join(
                    f"seed {r['rhs_seed']}: BiCGSTAB+V {r['bicgstab_vcycle']['iterations']} it / {r['bicgstab_vcycle']['seconds']:.2f}s" +
                    (f", FGCR+K status {r['fgcr10_kcycle_gcr']['status']} after {r['fgcr10_kcycle_gcr']['iterations']} it / {r['fgcr10_kcycle_gcr']['seconds']:.2f}s "
                     f"(residual {r['fgcr10_kcycle_gcr']['true_residual']:.1e})" if "fgcr10_kcycle_gcr" in r else "") for r in cd["runs"]))
        except Exception as e:  # noqa: BLE001
            log("convection-diffusion leg failed:", repr(e))
            out["solve_check"][f"convdiff_{args.convdiff_grid}"] = {"error": repr(e)}
    if not args.no_cpu:
        try:
            out["cpu_baseline"] = cpu_baseline(mg, args)
        except Exception as e:  # noqa: BLE001
            log("cpu_baseline failed:", repr(e))
            out["cpu_baseline"] = None
    emit_json(out)


if __name__ == "__main__":
    main()
