"""python -m multigridsolver_amd.solve <A.mtx> [--P <P.mtx>] [...]   — solve A x = b on one GPU, or on N GPUs when
launched by `python -m torch.distributed.run --nproc-per-node N -m multigridsolver_amd.solve ...` (rows sharded by
contiguous ranges, halo exchange over RCCL).  b is the reference's right-hand side (srand(0); rand()/RAND_MAX,
src/common/bicg.cpp:139,159-162); the two [info] lines of src/common/bicg.cpp:171-176 are printed by rank 0."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np


def ref_rhs(n):
    libc = C.CDLL(None)
    libc.srand(0)
    libc.rand.restype = C.c_int
    return np.array([libc.rand() / 2147483647.0 for _ in range(n)])


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m multigridsolver_amd.solve")
    ap.add_argument("matrix")
    ap.add_argument("--P", default=None, help="prolongation .mtx from the AGMG setup (single GPU only); default: aggregate on device")
    ap.add_argument("--tol", type=float, default=1e-6)           # bicg.cpp:148
    ap.add_argument("--max-iter", type=int, default=10000)       # bicg.cpp:164
    ap.add_argument("--solver", choices=["bicgstab", "fgcr", "pcg", "minres"], default=None,
                    help="default: bicgstab; minres: symmetric indefinite systems with a V(nu, nu) preconditioner, single GPU only (its plan: --minres-ahead)")
    ap.add_argument("--pcg-flexible", action="store_true", help="--solver pcg: flexible β, for a preconditioner that is not a fixed symmetric operator (--nu1 != --nu2, --kcycle)")
    ap.add_argument("--ahead", type=int, default=None, metavar="N",
                    help="--solver pcg or --solver bicgstab, named on the command line: solve through a PcgPlan resp. BicgstabPlan (scalars stay on the "
                         "device, one host look per iteration) that keeps N iterations enqueued beyond the last outcome seen; same result as without "
                         "the flag; single GPU only")
    ap.add_argument("--kcycle", type=int, default=0)
    ap.add_argument("--fgcr-ahead", type=int, default=None, metavar="N",
                    help="--solver fgcr: solve through an FgcrPlan (coefficients stay on the device, one host look per iteration) that keeps N iterations "
                         "enqueued beyond the last outcome seen; same result as without the flag; single GPU only")
    ap.add_argument("--kcycle-energy", action="store_true", help="K-cycle coefficients from energy inner products (flexible-CG form; symmetric positive definite operators only)")
    ap.add_argument("--minres-ahead", type=int, default=None, metavar="N",
                    help="--solver minres: solve through a MinresPlan (scalars stay on the device, one host look per iteration instead of two) that keeps N "
                         "iterations enqueued beyond the last outcome seen; same result as without the flag; single GPU only")
    ap.add_argument("--omega", type=float, default=0.6)
    ap.add_argument("--nu1", type=int, default=1)
    ap.add_argument("--nu2", type=int, default=1)
    ap.add_argument("--ktg", type=float, default=10.0)
    ap.add_argument("--npass", type=int, default=2)
    ap.add_argument("--tou", type=float, default=8.0)
    ap.add_argument("--operand-bits", type=int, choices=[64, 32], default=64,
                    help="stored precision of the cycle's matrix operands Â and A·P (32: values rounded to float, arithmetic stays FP64; single GPU only)")
    ap.add_argument("--nullspace", choices=["none", "constant"], default="none",
                    help="constant: A·1 = 0 and 1ᵀ·A = 0 (pure-Neumann operators, graph Laplacians) — regularised coarsest solve, projected Krylov method, "
                         "zero-mean solution; single GPU only")
    ap.add_argument("--eigs", type=int, default=0, metavar="K",
                    help="instead of a solve: the K smallest eigenpairs of the symmetric A by LOBPCG (K <= 8) with the hierarchy the other options describe "
                         "as preconditioner (V(nu, nu), no K-cycle), from random start vectors; --tol bounds |A x - theta x|/|A|_inf; no right-hand side; "
                         "single GPU only")
    ap.add_argument("--mass", default=None, metavar="FILE.mtx",
                    help="with --eigs: the symmetric positive definite B of the generalised problem A x = theta B x (MatrixMarket, the same reader as the operator); "
                         "the vectors come back B-orthonormal, --tol bounds |A x - theta B x|/(|A|_inf + |theta| |B|_inf); not with --nullspace")
    ap.add_argument("--dump-x", default=None, help="write the solution (rank order, raw little-endian f64)")
    args = ap.parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0"))
    if world > 1 and args.operand_bits != 64:
        raise SystemExit("multi-GPU: FP64 operands only (--operand-bits 32 is a single-GPU option)")
    if world > 1 and args.nullspace != "none":
        raise SystemExit("multi-GPU: --nullspace is a single-GPU option (row shards carry no null-space declaration)")
    if args.ahead is not None and (args.solver not in ("pcg", "bicgstab") or world > 1 or args.ahead < 0):
        raise SystemExit("--ahead N (N >= 0) goes with --solver pcg or --solver bicgstab, named explicitly, on a single GPU")
    if args.solver == "minres" and (args.ahead is not None or world > 1):
        raise SystemExit("--solver minres runs on a single GPU; its plan is chosen with --minres-ahead N (--ahead goes with --solver pcg or --solver bicgstab)")
    if args.fgcr_ahead is not None and (args.solver != "fgcr" or world > 1 or args.fgcr_ahead < 0):
        raise SystemExit("--fgcr-ahead N (N >= 0) goes with --solver fgcr on a single GPU")
    if args.minres_ahead is not None and (args.solver != "minres" or world > 1 or args.minres_ahead < 0):
        raise SystemExit("--minres-ahead N (N >= 0) goes with --solver minres on a single GPU")
    if args.eigs and (world > 1 or args.eigs < 0 or args.solver is not None):
        raise SystemExit("--eigs K (K >= 1) runs on a single GPU and takes no --solver")
    if args.mass is not None and (not args.eigs or args.nullspace != "none"):
        raise SystemExit("--mass FILE.mtx goes with --eigs K and without --nullspace (a null space together with B is not served)")
    if args.solver is None:
        args.solver = "bicgstab"
    if world > 1:
        import torch  # noqa: F401  — before libmgs.so: both link a HIP runtime, the first one loaded serves the process
    import multigridsolver_amd as mg
    rows, cols, rp, ci, v = mg.read_mtx(args.matrix)
    if rows != cols:
        raise SystemExit("square operator required")
    bg = ref_rhs(rows)
    if world == 1:
        ctx = mg.Context(int(os.environ.get("LOCAL_RANK", "0")))
        if args.kcycle_energy:
            ctx.set_option("kcycle_energy", 1)
        A = ctx.csr(rows, cols, rp, ci, v)
        defect = None
        if args.nullspace == "constant":      # before the hierarchy is built: finalize() regularises the coarsest solve
            A.set_nullspace("constant")
            defect = A.nullspace_defect()
        h = mg.Hierarchy(A, args.omega, args.nu1, args.nu2)
        if args.P:
            h.push_P(mg.Csr.from_mtx(ctx, args.P))
        h.coarsen(args.ktg, args.npass, args.tou).finalize().set_kcycle(args.kcycle)
        if args.operand_bits != 64:
            h.set_operand_precision(args.operand_bits)
        if args.eigs:
            X = [ctx.vec(rows).rand(1, j * rows) for j in range(args.eigs)]
            B = None
            if args.mass is not None:
                B = mg.Csr.from_mtx(ctx, args.mass)
                if B.shape != (rows, rows):
                    raise SystemExit("--mass: B is %d x %d, the operator %d x %d" % (B.shape + (rows, rows)))
            ctx.sync(); t0 = time.perf_counter()
            st, it, theta, resid = mg.lobpcg(A, X, h, args.max_iter, args.tol, B)
            ctx.sync(); dt = time.perf_counter() - t0
            sys.stderr.write("    \033[1;34m[time] \033[0m%-42s : %f.\n" % ("LOBPCG_SolveTimer", dt))
            for j in range(args.eigs):
                print("    \033[32m\033[1m[info] \033[00m%-42s : %.12g (residual %.3g)." % ("Eigenvalue %d " % j, theta[j], resid[j]))
            print("    \033[32m\033[1m[info] \033[00m%-42s : %d (status %d)." % ("Number of iterations LOBPCG", it, st))
            if args.dump_x:
                np.concatenate([v.numpy() for v in X]).astype("<f8").tofile(args.dump_x)
            return 0 if st == 0 else 3
        x, b = ctx.vec(rows), ctx.vec(bg)
        plan = None                                                                         # allocations and the cycles' capture: outside the timer
        if args.ahead is not None:
            plan = mg.PcgPlan(A, h, args.pcg_flexible) if args.solver == "pcg" else mg.BicgstabPlan(A, h)
        if args.fgcr_ahead is not None:
            plan = mg.FgcrPlan(A, h, 10)
        if args.minres_ahead is not None:
            plan = mg.MinresPlan(A, h)
        ctx.sync(); t0 = time.perf_counter()
        if plan is not None:
            ahead = next(a for a in (args.ahead, args.fgcr_ahead, args.minres_ahead) if a is not None)
            st, it, tol = plan.solve(x, b, args.max_iter, args.tol, ahead)
        elif args.solver == "pcg":
            st, it, tol = mg.pcg(A, x, b, h, args.max_iter, args.tol, args.pcg_flexible)
        elif args.solver == "minres":
            st, it, tol = mg.minres(A, x, b, h, args.max_iter, args.tol)
        else:
            st, it, tol = (mg.bicgstab if args.solver == "bicgstab" else lambda *a: mg.fgcr(a[0], a[1], a[2], a[3], 10, a[4], a[5]))(A, x, b, h, args.max_iter, args.tol)
        ctx.sync(); dt = time.perf_counter() - t0
        xs = x.numpy()
        if defect is not None:
            print("    \033[32m\033[1m[info] \033[00m%-42s : %g (rows), %g (columns)." % ("Null-space defect |A.1|/||A|.1| ", defect[0], defect[1]))
    else:
        import torch
        import torch.distributed as dist
        from . import dist as mgd
        if args.P or args.solver == "fgcr" or args.kcycle:
            raise SystemExit("multi-GPU: device aggregation + BiCGSTAB or PCG + V-cycle only")
        dist.init_process_group(backend=os.environ.get("MGS_DIST_BACKEND", "nccl"))
        dev = 0 if os.environ.get("MGS_DIST_SHARE_GPU") else int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(dev)
        stream = torch.cuda.Stream(); torch.cuda.set_stream(stream)
        ctx = mg.Context(dev, stream.cuda_stream)
        comm = mgd.Comm()
        lrp, lci, lv, ncols, plan = mgd.shard_from_global(rows, rp, ci, v, world, rank, comm.exchange_lists)
        A = ctx.csr(plan.n_loc, ncols, lrp, lci, lv)
        sh = mgd.ShardedHierarchy(ctx, A, plan, args.omega, args.nu1, args.nu2, comm).build(args.ktg, args.npass, args.tou, tail_rows=max(20000, rows // 50))
        lo, hi = mgd.row_ranges(rows, world)[rank]
        x, b = ctx.vec(ncols), ctx.vec(bg[lo:hi])
        ctx.sync(); comm.barrier(); t0 = time.perf_counter()      # collectives on the side stream (dist.py Comm: the cycle's stream gets captured)
        st, it, tol = sh.pcg(x, b, args.max_iter, args.tol, args.pcg_flexible) if args.solver == "pcg" else sh.bicgstab(x, b, args.max_iter, args.tol)
        ctx.sync(); comm.barrier(); dt = time.perf_counter() - t0
        parts = comm.all_gather_object(x.numpy(plan.n_loc))
        xs = np.concatenate(parts)
    if rank == 0:
        name = {"pcg": "PCG", "minres": "MINRES"}.get(args.solver)
        sys.stderr.write("    \033[1;34m[time] \033[0m%-42s : %f.\n" % (name + "_SolveTimer" if name else "BiCGStab_SolveTimer", dt))
        if st == 0:
            print("    \033[32m\033[1m[info] \033[00m%-42s : %g." % ("Tolerance ", tol))
            print("    \033[32m\033[1m[info] \033[00m%-42s : %d." % ("Number of iterations " + name if name else "Number of iterations BICG", it))
        else:
            print((name + " encountered a problem with status code: %d" if name else "BiCGSTABiml encountered a problem with status code: %d") % st)
        if args.dump_x:
            xs.astype("<f8").tofile(args.dump_x)
    if world > 1:
        import torch.distributed as dist
        dist.barrier(); dist.destroy_process_group()
    return 0 if st == 0 else 3


if __name__ == "__main__":
    sys.exit(main())
