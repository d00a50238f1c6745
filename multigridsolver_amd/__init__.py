"""multigridsolver_amd — MI355X-native aggregation-AMG V-cycle hot path behind the
`solve()` / .mtx surface of mishraiiit/MultiGridSolver.  See DESIGN.md / INTEGRATION.md."""
from ._lib import MgsError, lib, SO_PATH  # noqa: F401
from .core import (BicgstabPlan, Context, Csr, FgcrPlan, Guess, Hierarchy, MinresPlan, PcgPlan, Vec, Xfer, bicgstab, fgcr, minres, pcg, read_mtx, write_mtx, lobpcg, vecs_gram, vecs_combine, vecs_info, eig_info, eig_residual,  # noqa: F401
                   OP_JACOBI, OP_MINRES_UPDATE, OP_RESIDUAL, OP_SPMV)
