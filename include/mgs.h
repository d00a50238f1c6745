/*
 * mgs.h — C ABI of libmgs.so: the MI355X (gfx950) solve-phase hot path of an
 * aggregation-based AMG V-cycle behind the surface of mishraiiit/MultiGridSolver.
 *
 * The reference has no FFI boundary (one translation unit per
 * program); the surface it exposes is source level.  Every entry point below names the
 * reference interface (file:line, relative to the reference checkout) it replaces or
 * serves.  The C++ face that keeps the reference's spelling (readMatrix, SMatrix,
 * MultiGridPrecond(A,P).solve(v), BiCGSTABiml) is multigridsolver_amd/cpp/mgs_host.hpp,
 * written on top of this header only.
 *
 * Conventions
 *   - plain pointers and sizes only; opaque handles; every call returns int
 *     (MGS_OK = 0, negative = error class) and records a message retrievable with
 *     mgs_last_error().
 *   - matrices: CSR, f64 values, int32 indices, columns sorted inside a row — the layout
 *     of `typedef SparseMatrix<double,RowMajor> SMatrix` (src/common/MatrixIO.cpp:10).
 *   - host arrays are caller-owned and copied on upload; device memory is owned by the
 *     library and released by the matching *_destroy.
 *   - one context = one HIP device + one stream; calls are asynchronous on that stream
 *     unless they return a host scalar or copy to host memory.  A context is not
 *     thread-safe.
 *   - there is NO CPU fallback: every compute entry point runs HIP kernels on the
 *     context's device and fails with MGS_ERR_HIP if that is impossible.
 */
#ifndef MGS_H
#define MGS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGS_OK 0
#define MGS_ERR_INVALID (-1) /* bad argument / shape mismatch                        */
#define MGS_ERR_HIP (-2)     /* HIP runtime failure (no device, launch error, ...)   */
#define MGS_ERR_IO (-3)      /* file open / parse failure                            */
#define MGS_ERR_ALLOC (-4)   /* host or device allocation failed                     */
#define MGS_ERR_NUMERIC (-5) /* zero diagonal, singular coarse operator, ...         */
#define MGS_ERR_STATE (-6)   /* call sequence error (e.g. V-cycle before finalize)   */

typedef struct mgs_ctx mgs_ctx;
typedef struct mgs_csr mgs_csr;   /* device CSR matrix                               */
typedef struct mgs_vec mgs_vec;   /* device f64 vector                               */
typedef struct mgs_xfer mgs_xfer; /* prolongation P with its restriction Pᵀ          */
typedef struct mgs_hier mgs_hier; /* multilevel hierarchy = the preconditioner state */

/* ------------------------------------------------------------------ context */
/* Device memory arena (optional; no reference counterpart).  One hipMalloc of `bytes` taken before the library's first device allocation;
 * operators, vectors and setup scratch are then placed inside it (first fit from the low end, 2 MiB alignment for blocks of 1 MiB or more,
 * coalescing on release) and requests that do not fit fall through to hipMalloc.  Same allocation sequence → same addresses in every
 * process: the fine-level SpMV's process-to-process spread shrinks from ±3–4 % to ±1 %.  Environment MGS_ARENA_GB=N does
 * the same at the first allocation; mgs_arena_reserve(0) rules an arena out.  mgs_arena_info: capacity, bytes in use, largest free block. */
int mgs_arena_reserve(size_t bytes);
int mgs_arena_info(size_t out[3]);

/* device: HIP device ordinal.  stream: a hipStream_t to launch on (e.g. the caller's
 * torch stream) or NULL to let the context create its own.                          */
int mgs_ctx_create(int device, void *stream, mgs_ctx **out);
int mgs_ctx_destroy(mgs_ctx *ctx);
const char *mgs_last_error(const mgs_ctx *ctx); /* ctx may be NULL: last global error */
int mgs_sync(mgs_ctx *ctx);                      /* hipStreamSynchronize              */
/* Releases the memory the context keeps between calls (the Krylov solvers' work vectors: eight vectors of the operator's size
 * after a BiCGSTABiml solve, bicg.cpp:75 declares them per call, four after an mgs_pcg solve — five when the caller's x has no
 * halo room on a row shard; the scratch of the fused inner products). */
int mgs_ctx_trim(mgs_ctx *ctx);
void *mgs_ctx_stream(mgs_ctx *ctx);              /* the hipStream_t in use            */
const char *mgs_version(void);

/* ------------------------------------------------ L0 I/O: Matrix-Market loader (host) */
/* readMatrix  — src/common/MatrixIO.cpp:12-37 (twin: src/GPU_CUDAC++/MatrixIO.cu:182-280):
 * leading '%' lines skipped, "M N L", L triples "i j v" 1-based in any order, bucketed by
 * row, each row sorted by column; coordinate real general only.  Output arrays are
 * malloc'ed by the library; release each with mgs_host_free.  Unlike the reference a
 * missing/short file is an error (MGS_ERR_IO) instead of undefined behaviour.          */
int mgs_mtx_read(const char *path, int *rows, int *cols, int *nnz,
                 int **rowptr, int **col, double **val);
/* writeMatrix — src/common/MatrixIO.cpp:39-57: banner "%%MatrixMarket matrix coordinate
 * real general " + "rows cols nnz" + row-major 1-based triples, default ostream precision
 * (6 significant digits).                                                             */
int mgs_mtx_write(const char *path, int rows, int cols, int nnz,
                  const int *rowptr, const int *col, const double *val);
void mgs_host_free(void *p);

/* ------------------------------------------------------------ device CSR (row a1/a10) */
/* Replaces deepCopyMatrixCSRCPUtoGPU / deepCopyMatrixCSRGPUtoCPU
 * (src/GPU_CUDAC++/MatrixOperations.cu:121-146,162-171): sizes stay on the host, raw
 * device arrays inside.  nnz is int64 in the signatures for headroom; indices are int32
 * so nnz must be < 2^31.                                                              */
int mgs_csr_upload(mgs_ctx *ctx, int rows, int cols, int64_t nnz, const int *rowptr,
                   const int *col, const double *val, mgs_csr **out);
int mgs_csr_download(const mgs_csr *A, int *rowptr, int *col, double *val);
int mgs_csr_shape(const mgs_csr *A, int *rows, int *cols, int64_t *nnz);
int mgs_csr_destroy(mgs_csr *A);
/* device pointers (for zero-copy interop, e.g. the Eigen CPU baseline after download) */
int mgs_csr_device_ptrs(const mgs_csr *A, void **rowptr, void **col, void **val);
/* New values for an uploaded matrix, SAME sparsity pattern, in place: the device arrays do not move, so hierarchies built on A
 * and their captured cycles stay valid (follow with mgs_hier_refresh).  No reference counterpart: the reference uploads a new
 * matrix and reruns its constructor per matrix (bicg.cpp:19-44).  host_val / device_val: nnz doubles in A's storage order; the
 * _dev form is a device-to-device copy on the context's stream (not synchronised).  Every other per-matrix cache (row-block
 * bounds, launch plan, index pattern code, origin) depends on the pattern only and is kept.
 * MGS_ERR_INVALID: A or the values NULL; nnz differs from the matrix's; the matrix carries a value-carrying pattern code
 * (option "valcode": its tables hold the old values).                                                                    */
int mgs_csr_update_values(mgs_csr *A, const double *host_val, int64_t nnz);
int mgs_csr_update_values_dev(mgs_csr *A, const void *device_val, int64_t nnz);
/* ---- matrices that already live in device memory: no host round trip of the data ----
 * Common to the two constructors below.  index_bits: 32 or 64, the width of the index arrays given (int32_t / int64_t); 64-bit
 * indices are range-checked as 64-bit values before they are narrowed to the library's int32.  nnz resp. ntrip must be below
 * 2^31.  The inputs are only read and are copied: the caller may release them once the call has returned.  The work is enqueued on
 * the context's stream and the call synchronises before it returns, as mgs_csr_upload does (it needs counts on the host); making
 * the inputs visible to that stream — synchronising the stream that produced them — is the caller's job.  No kernel uses an input
 * index as an address before it has been range-checked: bad input comes back as MGS_ERR_INVALID and never faults; *out is then not
 * written and everything the call allocated is released.  Both end with the launch plan of mgs_csr_upload: the result is
 * indistinguishable from an uploaded matrix (mgs_csr_optimize, hierarchies, Krylov solvers, mgs_csr_update_values*). */
/* CSR arrays in device memory.  Nearest reference line: deepCopyMatrixCSRCPUtoGPU, src/GPU_CUDAC++/MatrixOperations.cu:121-146 (host
 * to device, unchecked); taking device arrays has no reference counterpart.  The acceptance rules are mgs_csr_upload's, checked on
 * the device in the passes that copy and narrow the arrays: rowptr[0] == 0 and rowptr[rows] == nnz, rowptr monotone, every column in
 * [0, cols), columns strictly ascending inside a row (never compared across a row boundary).  MGS_ERR_INVALID: a NULL argument,
 * index_bits neither 32 nor 64, a violated rule — the message names the lowest offending row and the kind of violation in
 * mgs_csr_upload's wording, so it is deterministic. */
int mgs_csr_from_device(mgs_ctx *ctx, int rows, int cols, int64_t nnz, const void *rowptr_dev, const void *col_dev,
                        int index_bits, const void *val_dev, mgs_csr **out);
/* Triples (row[k], col[k], val[k]), 0-based, in any order, in device memory — readMatrix's assembly, src/common/MatrixIO.cpp:12-37
 * (bucket by row, sort each row), on the device; summing duplicates has no reference counterpart (the reference keeps them apart).
 * Entries with equal (row, col) are summed in input order (ascending k), the sum starting from the first value itself: a lone -0.0
 * stays -0.0 and the result is bit-reproducible, whatever the order the device handled the triples in.  Explicit zeros and sums that
 * cancel stay entries (the pattern is what mgs_hier_refresh keys on).  Columns come out ascending inside a row.
 * keep_map != 0: the matrix keeps the sorted source positions (4 B per triple) and the run boundaries (4 B per entry + 4) for
 * mgs_csr_update_values_coo_dev; mgs_csr_destroy frees them.
 * MGS_ERR_INVALID: a NULL argument; index_bits neither 32 nor 64; a row outside [0, rows) or a column outside [0, cols) (the message
 * names the lowest such triple); a row that receives more than MGS_COO_MAX_ROW triples, duplicates included (the message names the
 * lowest such row) — a documented limit: such a row is sorted by one workgroup in 64 KB of LDS. */
#define MGS_COO_MAX_ROW 8192   /* most triples (duplicates included) one row may receive */
int mgs_csr_from_coo_device(mgs_ctx *ctx, int rows, int cols, int64_t ntrip, const void *row_dev, const void *col_dev,
                            int index_bits, const void *val_dev, int keep_map, mgs_csr **out);
/* New triple values for a matrix assembled with keep_map, same triples in the same input order: the gather kernel of the assembly
 * runs again through the kept map into A's existing val array, so the result is bit-identical to assembling from scratch.  Enqueued
 * on the context's stream and not synchronised, like mgs_csr_update_values_dev; the arrays do not move, so hierarchies and cached
 * graphs stay valid (follow with mgs_hier_refresh).  Nearest reference line: MatrixIO.cpp:12-37, which the reference reruns per
 * matrix; re-assembling values only has no reference counterpart.
 * MGS_ERR_STATE: the matrix keeps no map.  MGS_ERR_INVALID: A or the values NULL; ntrip differs from the number of triples the
 * matrix was assembled from; a value-carrying pattern code (option "valcode"). */
int mgs_csr_update_values_coo_dev(mgs_csr *A, const void *val_dev, int64_t ntrip);
/* diagnostics (no reference counterpart): out[0] triples the matrix was assembled from (0: not from COO / no map kept), out[1]
 * entries, out[2] most triples in one row (0: not from COO), out[3] bytes the kept map occupies.  MGS_ERR_INVALID: NULL argument. */
int mgs_csr_coo_info(const mgs_csr *A, int64_t out[4]);
/* ---- declared null space (pure-Neumann Poisson problems, graph Laplacians) ----
 * MGS_NULLSPACE_CONSTANT asserts A·1 = 0 and 1ᵀ·A = 0: a symmetric A with zero row sums, or a nonsymmetric one with zero row and column
 * sums.  Nearest reference line: none — the reference's SparseLU (bicg.cpp:35-36) fails on such a matrix.  Like symmetry in mgs_pcg the
 * assertion is the caller's responsibility and is NOT verified (no threshold for "zero to rounding" can be derived for matrices somebody
 * else assembled); mgs_csr_nullspace_defect is the net.  What acts on the declaration:
 *   - mgs_hier_finalize / mgs_hier_refresh of a hierarchy whose fine operator carries it invert A_c + (s/n_c)·1·1ᵀ, s = max|a_ij| of the
 *     coarsest operator A_c (n_c rows), instead of A_c: for a symmetric semidefinite A_c with null vector 1 that inverse is
 *     A_c⁺ + (1/s)·1·1ᵀ/n_c — exactly A_c⁺·b on a right-hand side orthogonal to 1.  The singularity rule itself is unchanged.
 *   - mgs_pcg, mgs_bicgstab and mgs_fgcr solve A·x = Πb, Π = I − 1·1ᵀ/n, and return the solution of zero mean (see mgs_pcg).
 * Setting the kind on a matrix that a finalized hierarchy already uses takes effect at the next mgs_hier_finalize or mgs_hier_refresh.
 * Without the declaration every call takes exactly the path it took before these entry points existed.
 * mgs_csr_set_nullspace — MGS_ERR_INVALID: A NULL, unknown kind, matrix not square, matrix with halo columns (cols > rows: a row shard).
 * mgs_csr_nullspace_defect: out[0] = ‖A·1‖∞ / ‖|A|·1‖∞, out[1] the same quantity for Aᵀ (0 where the denominator is 0) — mgs_spmv on a ones
 * vector, mgs_csr_transpose and a max-abs reduction; it allocates two private copies of the matrix and synchronises: a diagnostic, never
 * called implicitly. */
#define MGS_NULLSPACE_NONE 0
#define MGS_NULLSPACE_CONSTANT 1
int mgs_csr_set_nullspace(mgs_csr *A, int kind);
int mgs_csr_nullspace(const mgs_csr *A, int *kind);
int mgs_csr_nullspace_defect(const mgs_csr *A, double out[2]);
/* ---- field-wise constant null space (enclosed Stokes / Darcy flow, graph Laplacians with several components) ----
 * MGS_NULLSPACE_FIELDS: the declared null space is the span of up to MGS_NULLSPACE_MAX_FIELDS indicator vectors z_f of disjoint row sets
 * ("fields").  labels_dev: A->rows entries of index_bits (32 or 64) bits in DEVICE memory; a label f in [0, nfields) puts the row in field f,
 * −1 puts it in no field; the numbering may be interleaved.  The declaration asserts A·z_f = 0 and z_fᵀ·A = 0 for every field — the pressure
 * constant of K = [[L, Dᵀ], [D, −C]] with velocity prescribed on the whole boundary, one constant per connected component of a graph
 * Laplacian.  Like the constant kind it is the caller's responsibility and is NOT verified; mgs_csr_nullspace_defect is the net (on a fields
 * matrix: the maximum over the fields of ‖A·z_f‖∞ / ‖|A|·z_f‖∞, and the same for Aᵀ; one SpMV per field and side).  Nearest reference line:
 * none (bicg.cpp:35-36 fails on such a matrix).
 * The labels are range-checked on the device before anything uses them (64-bit entries are compared as 64-bit values: 2³² does not alias 0),
 * narrowed into an int8 array the matrix owns (mgs_csr_destroy frees it, and so does a later mgs_csr_set_nullspace(A, MGS_NULLSPACE_NONE)),
 * and counted per field on the host side.  The call synchronises.  This kind is entered through this call only: mgs_csr_set_nullspace(A, 2)
 * stays MGS_ERR_INVALID.  mgs_csr_nullspace reports MGS_NULLSPACE_FIELDS.
 * MGS_ERR_INVALID, the matrix keeping the declaration it had: a NULL argument; index_bits neither 32 nor 64; nfields outside
 * 1..MGS_NULLSPACE_MAX_FIELDS; a matrix that is not square; a row shard; a label outside [−1, nfields) (the lowest offending row and its
 * value are named); a field without rows (named).
 * What acts on the declaration:
 *   - mgs_hier_finalize / mgs_hier_refresh: see there (coarse labels from the aggregation, A_c + Σ_f (s/n_cf)·z_cf·z_cfᵀ at the coarsest level).
 *   - mgs_minres, mgs_minres_plan_* and mgs_pcg solve A·x = Πb with Π = I − Σ_f z_f·z_fᵀ/n_f and return the x whose fields have zero mean.
 *     When A carries fields, the hierarchy's fine operator must carry MGS_NULLSPACE_FIELDS with the same nfields and the same per-field
 *     counts; that the two label ARRAYS agree is the caller's responsibility (the projections read A's, the coarsest solve follows h's).
 *   - every other solver (mgs_bicgstab, mgs_fgcr, mgs_pcg_plan_*, mgs_bicgstab_plan_*, mgs_fgcr_plan_*, mgs_guess_*) refuses the kind with
 *     MGS_ERR_INVALID and a message naming mgs_minres / mgs_pcg.
 * mgs_csr_nullspace_fields: *nfields (0 when the matrix carries another kind) and the rows of every field (0 beyond nfields).
 * MGS_ERR_INVALID: NULL argument. */
#define MGS_NULLSPACE_FIELDS 2
#define MGS_NULLSPACE_MAX_FIELDS 8
int mgs_csr_set_nullspace_fields(mgs_csr *A, const void *labels_dev, int index_bits, int nfields);
int mgs_csr_nullspace_fields(const mgs_csr *A, int *nfields, int64_t counts[MGS_NULLSPACE_MAX_FIELDS]);
/* Synthetic operator generated on device: 7-point 3-D Poisson on an
 * N^3 grid, 3-D extension of src/common/poisson.cpp:11-33 (diag 6, off-diagonals −1,
 * row e=(i*N+j)*N+k, ascending columns).  Rows of planes [plane_lo, plane_hi) only
 * (row-range shard); columns are global unless local_cols != 0, in which case they are
 * renumbered to [0,n_loc) for owned and n_loc.. for the lower/upper halo planes.       */
int mgs_csr_poisson3d(mgs_ctx *ctx, int N, int plane_lo, int plane_hi, int local_cols,
                      mgs_csr **out);
/* Same stencil family in 2-D exactly as src/common/poisson.cpp:9-37 (n^2 rows, 4/−1).  */
int mgs_csr_poisson2d(mgs_ctx *ctx, int n, mgs_csr **out);
/* Bᵀ materialised row-major (bicg.cpp:32 `Ptrans = P.transpose()`).                    */
int mgs_csr_transpose(const mgs_csr *A, mgs_csr **out);
/* A_c = PᵀAP (bicg.cpp:33).  Runs on device.                                          */
int mgs_csr_galerkin(const mgs_csr *A, const mgs_xfer *P, mgs_csr **out);
/* ---- sparse products on the device ----
 * Nearest reference line: bicg.cpp:32-33, the Eigen products `Ptrans * A * P`; a product of two caller-supplied matrices has no other
 * reference counterpart.  mgs_csr_galerkin with a P that is not a 0/1 aggregation is (Pᵀ·A)·P through these kernels.
 * mgs_csr_spgemm — C = A·B for A (m × k) and B (k × n) of one context.  C is an ordinary matrix, indistinguishable from an uploaded one
 * (launch plan, mgs_csr_optimize, hierarchies, mgs_csr_update_values*).  The pattern is structural: a product that is 0 and sums that
 * cancel stay entries (the pattern is what mgs_hier_refresh keys on); columns come out ascending inside a row; rows without products
 * are empty.  The work is enqueued on the context's stream and the call synchronises before it returns, as mgs_csr_upload does (it
 * needs counts on the host).
 * Arithmetic, which makes the result bit-reproducible and restatable on a host: row i of C visits the entries (i, l) of A in storage
 * order and for each the entries (l, j) of B in storage order; every product a_il·b_lj is rounded once (no fused multiply-add); the first
 * product that reaches column j is stored — a lone -0.0 stays -0.0 — and every later one is added to it, in the order met.  No atomics
 * on values: two identical calls give identical bits.
 * MGS_ERR_INVALID, with a message: a NULL argument; different contexts; A->cols != B->rows; a row shard as either factor (cols > rows on
 * a matrix generated as a plane range by mgs_csr_poisson3d or living in a context that sums over ranks: its halo columns are not a
 * product the library can interpret); more than 2^31 - 1 entries in C; a row of C with more than MGS_SPGEMM_MAX_ROW distinct columns
 * (the message names the lowest such row) — a documented limit like MGS_COO_MAX_ROW: such a row is collected by one workgroup in a
 * 16384-slot hash table in 64 KB of LDS, kept at most half full.  On failure nothing is written to *C and everything the call
 * allocated is released.
 * mgs_csr_spgemm_numeric — the values of C again, in place, from the current values of A and B (mgs_csr_update_values*).  Precondition:
 * A and B have the patterns they had when C was built.  It runs the product's own numeric pass, so the bits are those of a fresh
 * mgs_csr_spgemm; C's arrays do not move, so hierarchies built on C and their cached graphs stay valid (follow with
 * mgs_hier_refresh); no allocation, scan or count pass.  misses == NULL: enqueued on the context's stream with no host wait.
 * misses given: the call synchronises and writes the number of products whose column is not in C's pattern; MGS_ERR_STATE when that
 * number is not 0 (C's values are then unspecified).  MGS_ERR_INVALID: a NULL matrix; different contexts; a row shard; shapes that do
 * not fit C; a C that mgs_csr_spgemm did not build; a value-carrying pattern code on C (option "valcode").
 * mgs_csr_spgemm_info — diagnostics: out[0] rows handled by the lane-per-row kernel (at most 64 products), out[1] rows handled by the
 * workgroup-per-row kernel, out[2] longest row of C, out[3] the largest per-row product count, the sum over the row's entries (i, l)
 * of the length of B's row l.  All four are 0 for a matrix that was not built by a product.  MGS_ERR_INVALID: NULL argument. */
#define MGS_SPGEMM_MAX_ROW 8192   /* most distinct columns one row of C may hold */
int mgs_csr_spgemm(const mgs_csr *A, const mgs_csr *B, mgs_csr **C);
int mgs_csr_spgemm_numeric(const mgs_csr *A, const mgs_csr *B, mgs_csr *C, int64_t *misses);
int mgs_csr_spgemm_info(const mgs_csr *C, int64_t out[4]);
/* ---- sums and scalings of device matrices ----
 * Nearest reference line: none — the reference multiplies matrices (bicg.cpp:32-33) and reads its operators from files
 * (MatrixIO.cpp:12-37); sums such as M/Δt + K, A + σI or AᵀA + λI and the D⁻¹ of B·D⁻¹·Bᵀ are assembled by its callers before that.
 * mgs_csr_add — C = α·A + β·B for A and B of one shape and one context (A == B, the same handle, is allowed).  C is an ordinary matrix,
 * indistinguishable from an uploaded one (launch plan, mgs_csr_optimize, hierarchies, the Krylov solvers, mgs_csr_update_values*, a factor
 * of mgs_csr_spgemm or of another sum); it carries no null-space declaration and no origin.  The pattern is structural: the union of the
 * two stored patterns, columns ascending inside a row; an entry whose sum cancels or whose value is 0 stays an entry (the pattern is what
 * mgs_hier_refresh keys on).  The work is enqueued on the context's stream and the call synchronises before it returns, as
 * mgs_csr_upload and mgs_csr_spgemm do (it needs counts on the host).
 * Arithmetic, which makes the result bit-reproducible and restatable on a host: every product and every sum is rounded separately (no
 * fused multiply-add).  An entry stored only in A is fl(α·a), one stored only in B is fl(β·b), one stored in both is
 * fl(fl(α·a) + fl(β·b)); a lone -0.0 stays -0.0.  No atomics on values: two identical calls give identical bits.
 * Rows are binned by u_i = len_A(i) + len_B(i): u_i <= 64 is merged by one lane, a longer row by one wave in chunks of 64 entries
 * without staging it anywhere, so there is no limit on the length of a row.
 * MGS_ERR_INVALID, with a message: a NULL argument; different contexts; different shapes (the message gives both); a row shard as either
 * operand (see mgs_csr_spgemm); a union of 2^31 - 1 entries or more.  On failure nothing is written to *C and everything the call
 * allocated is released.
 * mgs_csr_add_numeric — the values of C again, in place, from the current values of A and B (mgs_csr_update_values*) and the α, β given
 * here, which may differ from the ones C was built with (a changed Δt).  Precondition: A and B have the patterns they had when C was
 * built.  It runs the fill pass's own merge and writes values only, so the bits are those of a fresh mgs_csr_add; C's arrays do not
 * move, so hierarchies built on C and their cached graphs stay valid (follow with mgs_hier_refresh); no allocation, no scan, at most two
 * launches.  misses == NULL: enqueued on the context's stream with no host wait.  misses given: the call synchronises and writes the
 * number of entries of A or B whose column is not at the computed place in C; MGS_ERR_STATE when that number is not 0 (C's values are
 * then unspecified; nothing is written outside C's rows).  MGS_ERR_INVALID: a NULL matrix; different contexts; shapes that do not fit
 * C; a C that mgs_csr_add did not build; a value-carrying pattern code on C (option "valcode").
 * mgs_csr_add_info — diagnostics: out[0] rows merged by one lane, out[1] rows merged by one wave, out[2] longest row of C, out[3]
 * entries stored in both A and B.  All four are 0 for a matrix that is not a sum.  MGS_ERR_INVALID: NULL argument.
 * mgs_csr_scale — a_ij <- fl(fl(dl_i·a_ij)·dr_j) in place.  Either vector may be NULL: that factor is skipped (one rounding then, none
 * and no launch if both are NULL).  One entry-parallel launch on the context's stream, no host wait.  The pattern, the launch plan and
 * the pattern code stay: follow with mgs_hier_refresh on hierarchies built on A.  MGS_ERR_INVALID: A NULL; a vector of another context;
 * dl shorter than rows or dr shorter than cols; a row shard; a value-carrying pattern code on A (option "valcode").
 * mgs_csr_diag — d_i = a_ii for i < min(rows, cols), +0.0 where row i stores no diagonal entry; any shape; d holds at least
 * min(rows, cols) entries; enqueued, no host wait.  MGS_ERR_INVALID: a NULL argument, another context, a shorter d.
 * mgs_csr_from_diag — the n × n matrix with d_i stored at (i, i) for every i, zeros included, n = mgs_vec_size(d); an ordinary matrix
 * (synchronises like mgs_csr_upload).  A + σI is mgs_csr_add with the diagonal matrix of a filled vector, M/Δt + K with a lumped mass
 * vector likewise.  MGS_ERR_INVALID: a NULL argument, a vector of another context, n >= 2^31 - 1. */
int mgs_csr_add(double alpha, const mgs_csr *A, double beta, const mgs_csr *B, mgs_csr **C);
int mgs_csr_add_numeric(double alpha, const mgs_csr *A, double beta, const mgs_csr *B, mgs_csr *C, int64_t *misses);
int mgs_csr_add_info(const mgs_csr *C, int64_t out[4]);
int mgs_csr_scale(mgs_csr *A, const mgs_vec *dl, const mgs_vec *dr);
int mgs_csr_diag(const mgs_csr *A, mgs_vec *d);
int mgs_csr_from_diag(mgs_ctx *ctx, const mgs_vec *d, mgs_csr **out);
/* ---- blocks of a device matrix, gather and scatter of a vector by an index list ----
 * Nearest reference line: none — the reference reads whole operators from files (MatrixIO.cpp:12-37); the blocks of a reduced system
 * A_ff·x_f = b_f - A_fc·g (essential boundary conditions), of a Schur complement A_cc - A_cf·D_ff⁻¹·A_fc or of a field split are cut out by
 * its callers before that.
 * mgs_csr_extract — S = A(rows, cols): row k of S is row rows[k] of A restricted to the listed columns, column cols[q] renumbered to q;
 * S is nr × nc.  The lists are arrays in device memory (make them visible first) of index_bits = 32 or 64 bits per entry, one width for
 * both, as in mgs_csr_from_device.  rows_dev == NULL: every row in order, nr is ignored and S has A's rows.  A given row list may be
 * in any order and may repeat rows.  cols_dev == NULL: every column, nc is ignored and S has A's columns.  A given column list must be
 * strictly ascending: that keeps every row of S ascending without a sort and makes the list free of duplicates; a general column
 * permutation is mgs_csr_permute.  No kernel uses a list entry as an address before it has compared it with its bounds; 64-bit entries
 * are compared as 64-bit values before they are narrowed.  Value bits are copied unchanged: -0.0 stays -0.0 and a NaN keeps its payload.
 * The pattern is structural: stored zeros stay entries (the pattern is what mgs_hier_refresh keys on).  S is an ordinary matrix,
 * indistinguishable from an uploaded one (launch plan, mgs_csr_optimize, hierarchies, the Krylov solvers, a factor of mgs_csr_spgemm or
 * mgs_csr_add); it carries no null-space declaration and no origin.  The work is enqueued on the context's stream and the call
 * synchronises before it returns, as mgs_csr_add does (it needs counts on the host).  Without a column list an output entry finds
 * its row by bisection and is copied, entry-parallel; with one, an output row whose source row holds at most 64 entries is served by
 * one lane and a longer one by one wave in chunks of 64 entries without staging it anywhere, so there is no limit on the length of a
 * row.  Every place is computed from the row alone, no atomics on values or places: two identical calls give identical arrays.
 * MGS_ERR_INVALID, with a message: a NULL A or S; index_bits neither 32 nor 64; a negative nr or nc; a row index outside [0, A->rows)
 * (the message names the lowest offending position in the list and its value); a column index outside [0, A->cols), named likewise; a
 * column list that is not strictly ascending (the message names the lowest position k with cols[k] <= cols[k-1]; of several column
 * violations the one at the lowest position is reported, a row violation before any of them); a row shard as A (see mgs_csr_spgemm);
 * a result of 2^31 - 1 entries or more (repeated rows can cause it: the total is kept in 64 bits).  On failure nothing is written to
 * *S and everything the call allocated is released.
 * keep_map != 0: S keeps the position in A's arrays of every entry (4 B per entry of S, freed by mgs_csr_destroy) and records A's rows,
 * columns and number of entries.
 * mgs_csr_extract_numeric — S.val[k] = A.val[src[k]] through the kept map, for an A whose values changed and whose pattern did not
 * (mgs_csr_update_values*, *_numeric): one entry-parallel launch on the context's stream, no host wait, no allocation, no scan; the bits
 * are those of a fresh mgs_csr_extract.  S's arrays do not move, so hierarchies built on S and their cached graphs stay valid (follow with
 * mgs_hier_refresh).  MGS_ERR_STATE: S keeps no map.  MGS_ERR_INVALID: a NULL handle; different contexts; an A whose rows, columns or
 * number of entries differ from those recorded; a value-carrying pattern code on S (option "valcode").
 * mgs_csr_extract_info — diagnostics: out[0] rows counted by one lane, out[1] rows counted by one wave, out[2] longest row of S, out[3]
 * bytes of the kept map.  All four are 0 for a matrix that mgs_csr_extract did not build; out[0] and out[1] are 0 for cols_dev == NULL
 * (no pass over columns).  MGS_ERR_INVALID: NULL argument.
 * mgs_vec_gather — y[k] = x[idx[k]] for k < n; indices may repeat.  mgs_vec_scatter — x[idx[k]] = y[k] for k < n; the indices must be
 * distinct: with repeats the entry holds one of the values, unspecified which.  Each is one launch on the context's stream.  Every index
 * is compared with [0, mgs_vec_size(x)) in the kernel, as a 64-bit value, and an index outside is never used: gather stores +0.0 at
 * that place of y, scatter skips it.  bad == NULL: the call is enqueued with no host wait.  bad given: the call synchronises and writes
 * the number of indices outside the range; MGS_ERR_INVALID when that number is not 0.  MGS_ERR_INVALID also: a NULL argument; vectors
 * of different contexts; n < 0 or n above the length of y (the compact side in both calls); index_bits neither 32 nor 64; x and y the
 * same array. */
int mgs_csr_extract(const mgs_csr *A, const void *rows_dev, int64_t nr, const void *cols_dev, int64_t nc,
                    int index_bits, int keep_map, mgs_csr **S);
int mgs_csr_extract_numeric(const mgs_csr *A, mgs_csr *S);
int mgs_csr_extract_info(const mgs_csr *S, int64_t out[4]);
int mgs_vec_gather(const mgs_vec *x, const void *idx_dev, int64_t n, int index_bits, mgs_vec *y, int64_t *bad);
int mgs_vec_scatter(const mgs_vec *y, const void *idx_dev, int64_t n, int index_bits, mgs_vec *x, int64_t *bad);
/* ---- reordering a device matrix, assembling one from a grid of blocks ----
 * Nearest reference line: none — the reference reads whole operators from files (MatrixIO.cpp:12-37); a renumbering of the unknowns
 * (interleaved fields to field-major and back, a bandwidth-reducing or plane-major order) and the assembly of a coupled operator
 * [[A, Bᵀ], [B, -C]] from its fields are done by its callers before that.
 * mgs_csr_permute — C[i, j] = A[rperm[i], cperm[j]]: C has A's shape, row k of C is row rperm[k] of A, column cperm[q] of A is renumbered
 * to q (scipy's A[rperm][:, cperm], the convention of mgs_csr_extract).  rperm_dev holds A->rows entries and cperm_dev A->cols entries,
 * arrays in device memory (make them visible first) of index_bits = 32 or 64 bits per entry, one width for both.  rperm_dev == NULL or
 * cperm_dev == NULL: the identity on that side; both NULL give a copy.  A symmetric reordering P·A·Pᵀ passes the same list twice;
 * rectangular matrices are allowed.  With the vectors moved by mgs_vec_gather: C·gather(x, cperm) = gather(A·x, rperm).
 * Each list must be a bijection, and that is checked on the device before any entry is used as an address: 64-bit entries are compared
 * as 64-bit values before they are narrowed, a value outside [0, n) is refused and so is a value that repeats an earlier entry.  The
 * message names the list, the lowest offending position and its value (a range violation and a repeat are both positions: the lowest
 * one is named, whichever kind it is; a violation of the row list before any of the column list), so it is deterministic.
 * Row i of C holds the entries of A's row rperm[i] in ascending order of their new column.  The new columns of one row are distinct,
 * so an entry's place is its rank, the number of entries of its row with a smaller new column: every place is computed from the row
 * alone, without a sort network, without staging that would limit the length of a row and without atomics on places or values — two
 * identical calls give identical arrays.  Without a column list the rows are copied as they are, entry-parallel (an output entry finds
 * its row by bisection); with one, a source row of at most 64 entries is ranked by one lane and a longer one by one wave that holds 64
 * entries at a time and counts ranks against the row chunk by chunk.  Value bits are copied unchanged: -0.0 stays -0.0 and a NaN keeps
 * its payload.  The pattern is structural: stored zeros stay entries.  C is an ordinary matrix, indistinguishable from an uploaded one
 * (launch plan, mgs_csr_optimize, hierarchies, the Krylov solvers, mgs_csr_update_values*, a factor of mgs_csr_spgemm, mgs_csr_add or
 * mgs_csr_bmat); it carries no null-space declaration and no origin.  The work is enqueued on the context's stream and the call
 * synchronises before it returns, as mgs_csr_extract does.
 * MGS_ERR_INVALID, with a message: a NULL A or C; index_bits neither 32 nor 64; a list that is no bijection (above); a row shard as A
 * (see mgs_csr_spgemm).  On failure nothing is written to *C and everything the call allocated is released.
 * keep_map != 0: C keeps the position in A's arrays of every entry (4 B per entry of C, freed by mgs_csr_destroy) and records A's rows,
 * columns and number of entries.
 * mgs_csr_permute_numeric — C.val[k] = A.val[src[k]] through the kept map, for an A whose values changed and whose pattern did not
 * (mgs_csr_update_values*, *_numeric): one entry-parallel launch on the context's stream, no host wait, no allocation, no scan; the bits
 * are those of a fresh mgs_csr_permute.  C's arrays do not move, so hierarchies built on C and their cached graphs stay valid (follow
 * with mgs_hier_refresh).  MGS_ERR_STATE: C keeps no map.  MGS_ERR_INVALID: a NULL handle; different contexts; an A whose rows, columns
 * or number of entries differ from those recorded; a value-carrying pattern code on C (option "valcode").
 * mgs_csr_permute_info — diagnostics: out[0] rows ranked by one lane, out[1] rows ranked by one wave, out[2] longest row of C, out[3]
 * bytes of the kept map.  All four are 0 for a matrix that mgs_csr_permute did not build; out[0] and out[1] are 0 for cperm_dev == NULL
 * (nothing is ranked).  MGS_ERR_INVALID: NULL argument.
 * mgs_csr_bmat — C assembled from a grid of br × bc blocks (scipy.sparse.bmat): blocks is a host array of br·bc handles, row-major; NULL
 * stands for a zero block and the same handle may appear in several places.  br == 1 is an hstack, bc == 1 a vstack, NULL off the
 * diagonal a block-diagonal matrix.  All blocks of block row I share their row count and all blocks of block column J their column
 * count.  row_sizes (br ints) and col_sizes (bc ints) are host arrays, either may be NULL; a given size must agree with the blocks, and
 * a block row or column made only of NULLs needs its size from the array.  Row roff_I + i of C is the concatenation over J of row i of
 * block (I, J) with coff_J added to the columns, so rows come out ascending without a sort; an all-NULL block row gives empty rows.
 * The block descriptors (rowptr, col, val, column offset) live in a table in device memory that C keeps.  One lane per output row sums
 * at most bc row lengths, a 64-bit total beside them; the library's scan; then an entry-parallel fill with coalesced stores in which
 * an output entry finds its row by bisection in C's rowptr, its block from the row's per-block lengths and its source position from
 * the block's rowptr.  No limit on the length of a row, no atomics on places or values: two identical calls give identical arrays.
 * Value bits are copied unchanged (-0.0, NaN payloads); stored zeros stay entries.  C is an ordinary matrix without null-space
 * declaration or origin; the call synchronises before it returns.
 * MGS_ERR_INVALID, with a message that names the block position (I, J) where there is one: a NULL ctx, blocks or C; br or bc below 1
 * or br·bc above MGS_BMAT_MAX_BLOCKS; a block of another context; sizes that disagree; a block row or column without any size; a row
 * shard as a block; a total of 2^31 - 1 rows, columns or entries or more.  On failure nothing is written to *C and everything the call
 * allocated is released.
 * mgs_csr_bmat_numeric — the values of C again, in place, from the current values of the blocks: the fill pass's own place computation
 * writing values only (no map is kept), so the bits are those of a fresh mgs_csr_bmat; no allocation; C's arrays do not move: follow
 * with mgs_hier_refresh.  blocks holds as many handles as C's grid (out[1]·out[2] of mgs_csr_bmat_info): the call takes no dimensions.
 * ONE LAUNCH WITH NO HOST WAIT ONLY FOR THE RECORDED HANDLES: when blocks are the handles C was assembled from (their arrays do not
 * move under mgs_csr_update_values*), the table in device memory is left alone and the call is enqueued.  Other handles of the same
 * shapes and entry counts are accepted, but the call then waits for the stream, rewrites the table with a blocking copy and
 * records the new handles — it is not enqueue-only in that case.  Precondition: the blocks have the patterns they had.  C records per block position whether it was NULL, its shape
 * and its number of entries; MGS_ERR_INVALID, naming the position: blocks that differ in any of these; also a NULL argument, a C that
 * mgs_csr_bmat did not build, a block of another context, a value-carrying pattern code on C (option "valcode").
 * mgs_csr_bmat_info — diagnostics: out[0] blocks that are not NULL, out[1] br, out[2] bc, out[3] longest row of C.  All four are 0 for
 * a matrix that mgs_csr_bmat did not build.  MGS_ERR_INVALID: NULL argument.
 * mgs_csr_transpose_numeric — the values of At again, in place, from the current values of A, for an At whose pattern is the transpose
 * of A's pattern (what mgs_csr_transpose(A) built) and an A whose values changed and whose pattern did not.  No map is kept and
 * mgs_csr_transpose is unchanged: one entry-parallel launch over A's entries in which entry k finds its row i by bisection in A's
 * rowptr, has column j, and finds its place by bisection of i in At's columns of row j.  The value moves as a 64-bit word (-0.0, NaN
 * payloads); no atomics on values or places, places of distinct entries are distinct; the bits are those of a fresh mgs_csr_transpose.
 * An entry whose place does not exist is counted and never written; nothing is ever written outside At's values.  No allocation; At's
 * arrays do not move: follow with mgs_csr_bmat_numeric, mgs_csr_scale, mgs_csr_spgemm_numeric, ... and mgs_hier_refresh.
 * mgs_csr_scale works in place: a transposed operand that was scaled holds unscaled values after the refill and is scaled again.
 * misses == NULL: enqueued on the context's stream, no host wait.  misses given: the call synchronises and writes the number of entries
 * without a place; MGS_ERR_STATE when it is not 0.  MGS_ERR_INVALID: a NULL handle; different contexts; an At that is not cols × rows
 * of A; different entry counts; a value-carrying pattern code on At (option "valcode"). */
#define MGS_BMAT_MAX_BLOCKS 256   /* most block positions (br·bc) one mgs_csr_bmat call takes */
int mgs_csr_permute(const mgs_csr *A, const void *rperm_dev, const void *cperm_dev,
                    int index_bits, int keep_map, mgs_csr **C);
int mgs_csr_permute_numeric(const mgs_csr *A, mgs_csr *C);
int mgs_csr_permute_info(const mgs_csr *C, int64_t out[4]);
int mgs_csr_bmat(mgs_ctx *ctx, int br, int bc, const mgs_csr *const *blocks,
                 const int *row_sizes, const int *col_sizes, mgs_csr **C);
int mgs_csr_bmat_numeric(mgs_csr *C, const mgs_csr *const *blocks);
int mgs_csr_bmat_info(const mgs_csr *C, int64_t out[4]);
int mgs_csr_transpose_numeric(const mgs_csr *A, mgs_csr *At, int64_t *misses);

/* -------------------------------------------------------------------- device vectors */
/* Eigen::VectorXd on the device (bicg.cpp:153-162).                                    */
int mgs_vec_create(mgs_ctx *ctx, int64_t n, mgs_vec **out);
/* non-owning view of caller device memory (e.g. a torch tensor's data_ptr)            */
int mgs_vec_wrap(mgs_ctx *ctx, void *device_ptr, int64_t n, mgs_vec **out);
int mgs_vec_destroy(mgs_vec *v);
int mgs_vec_upload(mgs_vec *v, const double *host, int64_t n);
int mgs_vec_download(const mgs_vec *v, double *host, int64_t n);
int mgs_vec_fill(mgs_vec *v, double value);
int mgs_vec_copy(const mgs_vec *src, mgs_vec *dst);
int64_t mgs_vec_size(const mgs_vec *v);
void *mgs_vec_ptr(const mgs_vec *v);
/* counter-based uniform [0,1): splitmix64(seed, global_index)      */
int mgs_vec_rand(mgs_vec *v, uint64_t seed, int64_t global_offset);

/* ------------------------------------------------------ L1 hot-path primitives (★)   */
/* y = A x — `A * v`, bicg.cpp:57,82,107,117; Eigen kernel
 * lib/Eigen/src/SparseCore/SparseDenseProduct.h:26-71.                                */
int mgs_spmv(const mgs_csr *A, const mgs_vec *x, mgs_vec *y);
/* r = b − A x — bicg.cpp:82.                                                          */
int mgs_residual(const mgs_csr *A, const mgs_vec *x, const mgs_vec *b, mgs_vec *r);
/* dinv_i = 1/a_ii — M2 = diag(diag(A))\x, src/CPU_Matlab/solve.m:17.  Fails with
 * MGS_ERR_NUMERIC if a diagonal entry is missing or zero.                             */
int mgs_diag_inv(const mgs_csr *A, mgs_vec *dinv);
/* x_out = x_in + ω D⁻¹ (b − A x_in), out of place (x_out must not alias x_in) —
 * SURVEY §8a row a7; spec solve.m:17 + paper eq. (3.5).                               */
int mgs_jacobi(const mgs_csr *A, const mgs_vec *dinv, double omega, const mgs_vec *b,
               const mgs_vec *x_in, mgs_vec *x_out);

/* Prolongation operator.  P is taken as CSR (what readMatrix returns for
 * <name>promatrix_<tag>.mtx, bicg.cpp:151).  If every row holds at most one entry of
 * value exactly 1 (how AGMG builds it: src/CPU_C++/AGMG.cpp:181-186,
 * src/GPU_CUDAC++/Aggregation.cu:252-270) the aggregate-id form is used; any other P
 * runs through the general CSR kernels with Pᵀ materialised (bicg.cpp:32).            */
int mgs_xfer_create(const mgs_csr *P, mgs_xfer **out);
int mgs_xfer_destroy(mgs_xfer *T);
int mgs_xfer_shape(const mgs_xfer *T, int *n_fine, int *n_coarse, int *is_aggregation);
/* r_c = Pᵀ r — `Ptrans * vec`, bicg.cpp:48.                                           */
int mgs_restrict(const mgs_xfer *T, const mgs_vec *r, mgs_vec *rc);
/* e = P e_c — `P * (...)`, bicg.cpp:48.                                               */
int mgs_prolong(const mgs_xfer *T, const mgs_vec *ec, mgs_vec *e);
/* x += P e_c (the coarse-grid correction of the V-cycle).                             */
int mgs_prolong_add(const mgs_xfer *T, const mgs_vec *ec, mgs_vec *x);

/* BLAS-1 used by BiCGSTABiml (bicg.cpp:64-72,95,101-120): free dot()/norm() and the
 * vector updates.  dot/nrm2 synchronise and return a host scalar.                     */
int mgs_dot(const mgs_vec *x, const mgs_vec *y, double *out);
int mgs_nrm2(const mgs_vec *x, double *out);
int mgs_axpby(double a, const mgs_vec *x, double b, mgs_vec *y); /* y = a x + b y      */
int mgs_axpbypcz(double a, const mgs_vec *x, double b, const mgs_vec *y, double c,
                 mgs_vec *z);                                    /* z = a x + b y + c z */

/* v ← v − mean(v): the projection Π = I − 1·1ᵀ/n the Krylov solvers apply for MGS_NULLSPACE_CONSTANT, on a vector of the caller's (tests and
 * diagnostics; no reference counterpart).  Two streaming launches beside the fold — a sum pass with a fixed partial layout; one workgroup
 * (behind a chunk stage above about two million entries) that folds the partials in index order and stores m = sum/n on the device; a
 * shift pass — so the result is bit-reproducible from run to run; 16-byte accesses when v is 16-byte aligned.  mean (may be NULL): the m that was subtracted, read back; nrm2 (may be NULL): ‖v − m‖₂ from the shift pass.  Synchronises when
 * either is asked for.  MGS_ERR_INVALID: v NULL. */
int mgs_vec_project_const(mgs_vec *v, double *mean, double *nrm2);
/* v ← Πv, Π = I − Σ_f z_f·z_fᵀ/n_f with the fields A declared (mgs_csr_set_nullspace_fields): v_i ← v_i − m[label_i] for label_i ≥ 0, rows
 * labelled −1 keep their bits.  Two streaming launches beside the fold: a label-segmented sum pass (one walk over v and the int8 labels, one
 * accumulator per field and lane, an entry added only to its own field's; partials in a fixed [nfields][workgroups] layout, no atomics),
 * a fold per field in index order (behind a chunk stage above about two million entries) that stores m_f = sum_f/n_f in device slots the
 * MATRIX owns (two matrices on one context do not collide), and the shift pass.  16-byte accesses with the labels of a pair loaded together
 * when v is 16-byte aligned; the `nt` store hint under option nt_store.  The contract: every labelled entry comes out as fl(v_i − m_f) for
 * the device's own m_f; |m_f − mean_f| <= n_f·ε·max|v|; two identical calls give identical bits.
 * means (may be NULL): the nfields values m_f that were subtracted, read back; nrm2 (may be NULL): ‖Πv‖₂ over ALL rows, from the shift pass.
 * Synchronises when either is asked for.  MGS_ERR_INVALID: v or A NULL, A without MGS_NULLSPACE_FIELDS, v shorter than A's rows. */
int mgs_vec_project_fields(mgs_vec *v, const mgs_csr *A, double *means /* nfields or NULL */, double *nrm2 /* or NULL */);

/* ------------------------------------------- L3 preconditioner: multilevel V-cycle (★) */
/* MultiGridPrecond(A, P) — bicg.cpp:19-62.  A is borrowed (must outlive the hierarchy).
 * Level l cycle: ν1 damped-Jacobi sweeps, r = b − Ax, r_c = Pᵀr, recurse from 0,
 * x += P e_c, ν2 sweeps; coarsest level solved directly (dense inverse built on device,
 * stands in for SparseLU, bicg.cpp:35-36).  Two-level with ν1=0, ν2=1 is bicg.cpp:46-61
 * with M2 = ωD⁻¹.                                                                     */
int mgs_hier_create(mgs_ctx *ctx, const mgs_csr *A, double omega, int nu1, int nu2,
                    mgs_hier **out);
/* append a level from a given prolongation (P.rows == rows of current coarsest);
 * computes A_c = PᵀAP on device (bicg.cpp:32-33).                                     */
int mgs_hier_push_P(mgs_hier *h, const mgs_csr *P);
/* append levels by on-device pairwise aggregation (Notay AGMG: src/CPU_C++/AGMG.cpp:
 * 299-315, src/GPU_CUDAC++/main.cu:95-277) until the coarsest has <= coarse_rows rows,
 * max_levels is reached or coarsening stalls.  ktg/npass/tou as the reference's argv
 * (src/CPU_C++/main.cpp:155-182; benchmarks use 10 2 8, results.txt:22-24).
 * The matching is deterministic: every undecided row picks its best admissible neighbour and mutual picks pair up.  A row's
 * neighbours are the entries of its row in the stored pattern when that pattern is symmetric, else in the union of the stored
 * patterns of A and Aᵀ; {i,j} is a candidate when a_ij != 0 or a_ji != 0, so a coupling stored (or non-zero) on one side only
 * pairs like any other, as in the reference (AGMG.cpp:151-174 scans row i of A).                                       */
int mgs_hier_coarsen(mgs_hier *h, double ktg, int npass, double tou, int coarse_rows,
                     int max_levels);
/* factor the coarsest operator (dense inverse on device, ≤ 8192 rows: Gauss-Jordan with partial
 * pivoting); must be called once before mgs_vcycle.  If coarsening stalled above that size (e.g.
 * all rows in G0) the coarsest level is smoothed by 8 damped-Jacobi sweeps instead.
 * MGS_ERR_NUMERIC: the coarsest operator is singular to working precision — a pivot is not
 * greater than 8·n·DBL_EPSILON·max|a_ij| (n its rows, a_ij its entries) — or holds a NaN or Inf.
 * A one-level hierarchy (no mgs_hier_push_P / mgs_hier_coarsen) is this dense solve alone and
 * is never smoothed: its operator may have zero or missing diagonal entries.  They are refused
 * with MGS_ERR_NUMERIC as soon as a level is pushed below it or it is smoothed itself.
 * Fine operator declared MGS_NULLSPACE_CONSTANT (mgs_csr_set_nullspace): the dense solve inverts A_c + (s/n_c)·1·1ᵀ, which is valid only
 * if every level inherits the null space (P·1_c = 1).  MGS_ERR_INVALID, with a message naming the level, when some level's transfer is a
 * general P, when a transfer leaves a row outside every aggregate, or when the hierarchy is row-sharded (halo columns, halo callbacks,
 * native plans or tail) — structural checks without a tolerance, made before anything is launched.  A one-level hierarchy is the
 * regularised dense solve alone; the smoothed coarsest form needs no change.  mgs_vcycle itself is not projected: its output on such a
 * hierarchy may carry a constant component, which the Krylov solvers remove.
 * Fine operator declared MGS_NULLSPACE_FIELDS (mgs_csr_set_nullspace_fields): coarse labels are built once per level from the aggregation —
 * an aggregate takes the label of its first member — by a kernel that also checks that all members of an aggregate share one label and
 * that every row with a label >= 0 lies inside an aggregate (rows labelled −1 may stay outside).  MGS_ERR_INVALID names the level and the
 * lowest offending fine row; the structural refusals of the constant kind (a general P, a row shard) apply unchanged.  The dense solve
 * inverts A_c + Σ_f (s/n_cf)·z_cf·z_cfᵀ, s = max|a_ij| of A_c, n_cf the coarsest rows of field f.  Labels depend on the pattern only:
 * mgs_hier_refresh keeps them (and the cached graphs) and only repeats the regularised inverse.  mgs_vcycle stays unprojected.
 * New labels on a matrix that a finalized hierarchy already uses take effect at the next mgs_hier_finalize; mgs_hier_refresh works with the
 * coarse labels it has (MGS_ERR_STATE when the hierarchy was finalized before any fields were declared, or for another number of them). */
int mgs_hier_finalize(mgs_hier *h);
int mgs_hier_set_smoother(mgs_hier *h, double omega, int nu1, int nu2);
/* Values changed, pattern did not (time stepping, Picard / Newton iterations, parameter sweeps): recomputes everything in h
 * that depends on matrix VALUES from the current values of the fine operator — the mgs_csr handle given to mgs_hier_create,
 * after mgs_csr_update_values — and keeps what depends on the pattern only: aggregates, coarse patterns, pattern codes,
 * row-block groups, every buffer.  Nearest reference line: the constructor, bicg.cpp:19-44, which the reference reruns per
 * matrix; reusing the interpolation has no reference counterpart (hypre / PETSc / AmgX offer it as structure reuse).
 * Level by level from the top: D⁻¹ from the new diagonal; the next level's values A_c = PᵀAP with the level's (composed)
 * aggregation, written into that level's existing val array by ONE launch of a numeric Galerkin kernel for the known
 * pattern (no count pass, scan, allocation or host synchronisation; same summation order as mgs_csr_galerkin /
 * mgs_hier_push_P, so bit-identical to them for the same A and P); the operands of the fused passes that a cycle has already
 * built — ωD⁻¹, Â, the values of A·P, their FP32 copies on levels switched to 32 bits — in their existing buffers (operands
 * not built yet are left to the next cycle); at the end the coarsest dense inverse into its existing buffer.  Smoother,
 * K-cycle, additive form, correction scale and operand precision are settings and stay.  No device buffer moves, so the
 * cached cycle graphs (which capture pointers and scalars, not values) are kept and replay with the new values; the host
 * reads one pair of counters per refresh besides what the dense inverse does.  From the second refresh on the bytes in use
 * do not change (the first one keeps 8 bytes of device flags: mgs_hier_refresh_info out[3]).
 * Caveat: mgs_hier_coarsen with npass >= 2 builds A_c as the chained product P2ᵀ(P1ᵀAP1)P2, the refresh forms PᵀAP with the
 * composed P in one pass: the two agree to rounding, not bit for bit, so a refresh with unchanged values may move coarse
 * entries in their last bits.  When the aggregates have aged and a rebuild is due is the caller's decision.
 * MGS_ERR_NUMERIC: a missing or zero diagonal on any level (not counted on a one-level hierarchy, see mgs_hier_finalize), or a
 * coarsest operator that mgs_hier_finalize's singularity rule refuses (pivot not greater than 8·n·DBL_EPSILON·max|a_ij|, NaN,
 * Inf) — the hierarchy is then left
 * un-finalized (cycles return MGS_ERR_STATE, cached graphs are dropped) until a later refresh succeeds.
 * MGS_ERR_STATE: before mgs_hier_finalize; entries of the fine operator fall outside the kept coarse patterns (its pattern is
 * not the one the hierarchy was built for).  MGS_ERR_INVALID: h NULL; a row-sharded hierarchy (halo columns, halo callbacks,
 * native plans or tail); a level whose transfer is a general P, not an aggregation; option "valcode".                    */
int mgs_hier_refresh(mgs_hier *h);
/* diagnostics: out[0] refreshes done, out[1] = 1 if the last one kept the cached graphs, out[2] levels refreshed by the device
 * kernel, out[3] bytes the refresh keeps allocated beyond the hierarchy's own */
int mgs_hier_refresh_info(const mgs_hier *h, int64_t out[4]);
/* Operand precision of the cycle (the reference's GPU path keeps its matrices in float32: SURVEY G3,
 * src/GPU_CUDAC++/MatrixIO.cu:32-36).  Here only the STORED values of the two setup-time operands of the fused zero-guess
 * V(1,1) passes — Â = A·diag(ωD⁻¹) and A·P — are rounded to FP32 (round to nearest, on the device, from the FP64
 * operands); vectors, gathers, products, sums, ωD⁻¹, the coarsest solve and the Krylov methods (which always use the
 * caller's FP64 A) stay FP64.  The cycle is then the FP64 cycle of a slightly different, fixed linear operator.
 *   bits: 64 (default) or 32; levels: how many leading levels to switch (<0: every eligible one).
 *   Applied to the longest eligible prefix not longer than `levels`; every other level runs 64 bits after the call
 *   (bits = 64 switches all levels back: bit-identical to a hierarchy that was never switched).
 * A level is eligible when its fused branch runs on those operands: aggregation P, square operator, options fuse,
 * fuse_operands and merge_ap on, rows of A and A·P no longer than 64.  K-cycle levels use the same passes and follow.
 * Cycles that do not take the fused branch (non-zero guess, ν ≠ 1, additive form, general P) read A itself and stay FP64
 * whatever was set here; mgs_hier_operand_precision reports 64 for them.  Prepares the operands (first-cycle setup) itself
 * and drops the cached graphs.  A new ω (mgs_hier_set_smoother) refreshes the FP32 copies together with Â.  The FP64
 * operands stay allocated beside the copies (+4 B per entry of A and of A·P on a switched level).
 * MGS_ERR_INVALID: bits not 64/32; before mgs_hier_finalize; option valcode on (coded blocks stream no values, nothing to
 * shrink); a row-sharded hierarchy (halo columns, halo callbacks, native transport or tail).                          */
int mgs_hier_set_operand_precision(mgs_hier *h, int bits, int levels);
/* what level `level` runs with right now: *bits = 64 | 32 */
int mgs_hier_operand_precision(const mgs_hier *h, int level, int *bits);
/* K-cycle (docs/AGMG_For_Convection_Diffusion.pdf §3.1, Fortran `nlvcyc`
 * src/CPU_Matlab/dagtwolev_mex.f90:59-61,72): the coarse problems of levels 1..levels are solved
 * by two GCR steps preconditioned by the cycle below instead of one recursive cycle.  0 = V-cycle
 * (default).  Scalars stay on the device; the second direction is orthogonalised explicitly against the first (ρ2 = d2'·v2' on the
 * orthogonalised pair — the paper's β − γ²/ρ1 without the difference of nearly equal numbers).  Option "kcycle_energy" (mgs_ctx_set_option):
 * coefficients from c instead of v = A·c (flexible-CG form) — SYMMETRIC POSITIVE DEFINITE operators only; the default is the paper's GCR form.
 * On a row-sharded hierarchy the inner products are summed over the ranks in three reductions per K step
 * (mgs_ctx_set_native_allreduce, else the mgs_ctx_set_allreduce callback); without either the level runs a V-cycle. */
int mgs_hier_set_kcycle(mgs_hier *h, int levels);
/* K iteration on level 0 itself when the hierarchy is applied from x = 0: for the replicated tail of a row-sharded hierarchy whose
 * K-cycle reaches the last sharded level (that level is the tail's level 0; no rank reduction needed: the tail is replicated). */
int mgs_hier_set_kcycle_entry(mgs_hier *h, int on);
/* diagnostics: the five scalars of the last K step of `level` (levels 1..levels of mgs_hier_set_kcycle; level 0 under
 * mgs_hier_set_kcycle_entry), copied from the device after waiting for the context's stream — read-only, the step is not run.  With
 * c1 = B·rhs, v1 = A·c1, r' = rhs − (α1/ρ1)·v1, c2 = B·r', v2 = A·c2, g = γ/ρ1, c2' = c2 − g·c1, v2' = v2 − g·v1 (B = the cycle below):
 *   out[0] ρ1   GCR form v1·v1     energy form (option kcycle_energy) c1·v1
 *   out[1] α1            v1·rhs                                       c1·rhs
 *   out[2] γ             v2·v1                                        c2·v1
 *   out[3] ρ2            v2'·v2'                                      c2'·v2'
 *   out[4] α2            v2'·r'                                       c2'·r'
 * and the step returns x = k1·c1 + k2·c2 with k2 = α2/ρ2 where ρ2 > 0 (else 0) and k1 = α1/ρ1 − g·k2; ρ1 = 0 gives x = 0.  A quotient by
 * ρ1 = 0 counts as 0 throughout.  All zero between the first cycle that prepared the level and its first K step.
 * MGS_ERR_INVALID: NULL argument, level out of range.  MGS_ERR_STATE: the level holds no K-step state yet (no cycle has run with the
 * K step switched on for it).  Not summed over the ranks of a row-sharded run: every rank already holds the reduced values. */
int mgs_hier_kcycle_scalars(mgs_hier *h, int level, double out[5]);
/* the additive switch of MultiGridPrecond::solve (reference src/common/bicg.cpp:59, `multiplicative_precond = false`; dead in the
 * reference — the constructor fixes it to true, :42): with on != 0 a zero-guess cycle returns, level by level,
 * P·cycle(Pᵀ v) + M2(v) with M2 = ωD⁻¹ instead of the multiplicative form.  The other switch, `use_preconditioner = false`
 * (:53-54, solve(v) = v), is mgs_bicgstab / mgs_fgcr with hier = NULL.  Not offered on row shards. */
int mgs_hier_set_additive(mgs_hier *h, int on);
/* over-correction of unsmoothed aggregation (new knob, default 1 = the reference's form `P * (…)`, bicg.cpp:48): the coarse-grid correction of
 * every level is scaled, x ← x + σ·P e_c.  Piecewise-constant prolongation under-corrects smooth error; σ ≈ 1.5–2 cuts the Krylov iterations of
 * the V-cycle preconditioner on Poisson-like problems at the cost of one axpy on each coarse vector.  Parity fixtures use σ = 1. */
int mgs_hier_set_correction_scale(mgs_hier *h, double sigma);
int mgs_hier_destroy(mgs_hier *h);
int mgs_hier_nlev(const mgs_hier *h);
int mgs_hier_level_shape(const mgs_hier *h, int level, int *rows, int64_t *nnz);
/* borrowed handles of level operators / transfer (valid while h lives)                */
const mgs_csr *mgs_hier_level_A(const mgs_hier *h, int level);
const mgs_xfer *mgs_hier_level_P(const mgs_hier *h, int level);
/* A·P of `level`, the fused post pass's operand under option merge_ap (rows of A, one column per aggregate, built by the first cycle
 * and kept current by mgs_hier_refresh): borrowed and read-only like the two above; NULL while it has not been built (no cycle yet,
 * merge_ap off, a general P, the coarsest level) and on out-of-range levels                                                      */
const mgs_csr *mgs_hier_level_AP(const mgs_hier *h, int level);
/* aggregate id of every fine row of `level` (−1 = not aggregated, G0) to host         */
int mgs_xfer_download_agg(const mgs_xfer *T, int *agg);
/* algorithmic HBM bytes of one V-cycle application (DESIGN.md §5 formula)             */
int64_t mgs_hier_vcycle_bytes(const mgs_hier *h);

/* One V-cycle: x ← cycle(b) from x=0 if zero_guess else improving the x passed in.
 * MultiGridPrecond::solve (bicg.cpp:51-61) == mgs_vcycle(h, v, out, 1).              */
int mgs_vcycle(mgs_hier *h, const mgs_vec *b, mgs_vec *x, int zero_guess);

/* ------------------------------------------------------ L4 Krylov: BiCGSTABiml (f-2) */
/* bicg.cpp:74-136, device resident.  h may be NULL (identity preconditioner).  On
 * return *max_iter = iterations done, *tol = achieved relative residual; the int result
 * of the reference (0 ok / 1 max_iter / 2 rho breakdown / 3 omega breakdown) is written
 * to *status; the function's own return value is the MGS_* error class.               */
int mgs_bicgstab(const mgs_csr *A, mgs_vec *x, const mgs_vec *b, mgs_hier *h,
                 int *max_iter, double *tol, int *status);

/* Flexible GCR(m) — the outer Krylov method AGMG pairs with the K-cycle, whose preconditioner is
 * not a fixed linear operator (BiCGSTAB may break down with it).  Restarted every `restart`
 * directions; same in/out convention as mgs_bicgstab (status 0 converged / 1 max_iter).  Not in the
 * reference's C++ (its Matlab driver calls pcg/bicgstab, src/CPU_Matlab/solve.m:28-33); provided
 * with the K-cycle.  Per iteration beside preconditioner and SpMV: one multi-dot pass (new direction against the
 * window), one fused update pass, one residual pass; x is updated once per window through the triangular coefficient system.  Status 0 is
 * reported only with the TRUE residual b − A·x below *tol (recomputed at every restart and before every return).  restart 1..64. */
int mgs_fgcr(const mgs_csr *A, mgs_vec *x, const mgs_vec *b, mgs_hier *h, int restart,
             int *max_iter, double *tol, int *status);

/* Preconditioned conjugate gradients for symmetric positive definite A — the reference's Matlab driver,
 * src/CPU_Matlab/solve.m:28-31.  Same in/out convention as mgs_bicgstab.  h may be NULL.
 * *status: 0 converged (decided on the TRUE residual b − A·x, as mgs_fgcr does) / 1 max_iter / 2 r·z not positive (the
 * preconditioner is not positive definite) / 3 p·A·p not positive (A is not positive definite along p).  *max_iter returns the
 * iterations done (for status 2 and 3 the iteration that stopped), *tol the last relative residual; whatever the status, x holds
 * every completed update.  Four work vectors (BiCGSTAB: eight), one cycle and one SpMV per iteration (BiCGSTAB: two of each);
 * works on row shards as mgs_bicgstab does.  A's symmetry is the caller's responsibility; statuses 2 and 3 are the net.
 * flexible = 0: classical β = ρ/ρ_prev; requires a fixed symmetric preconditioner — a hierarchy with nu1 != nu2 or with a K-cycle
 * (mgs_hier_set_kcycle, mgs_hier_set_kcycle_entry) is refused with MGS_ERR_INVALID.  The additive form, a correction scale and FP32
 * operand storage are allowed (fixed operators); with 32-bit operands (mgs_hier_set_operand_precision) the cycle is symmetric only
 * to FP32 rounding: flexible = 1 is recommended there.
 * flexible = 1: β = z·(r − r_prev)/ρ_prev, computed as −α·(z·q)/ρ_prev from the vectors already held — accepts a preconditioner
 * that changes from call to call (K-cycle) or is not symmetric (V(2,1)); one more stream in the dots pass (88 instead of 80 B per
 * row beside cycle and SpMV).
 * A declared MGS_NULLSPACE_CONSTANT (all three Krylov solvers): the system solved is A·x = Πb with Π = I − 1·1ᵀ/n, and x comes back with
 * zero mean.  Every true residual is Π(b − A·x); the caller's b is only read.  *tol is then relative to ‖Πb‖ (1 if that is zero).  mgs_pcg
 * projects z after every preconditioner application (h = NULL included), so the preconditioner it sees is ΠMΠ, symmetric when M is;
 * mgs_bicgstab projects both preconditioned vectors of an iteration, mgs_fgcr every direction c_k before v_k = A·c_k; x is projected after
 * its last update, before the true residual that decides the return (mgs_pcg and mgs_fgcr: before every true residual that may decide
 * one — when the recursion says converged or the iterations are used up; an ordinary restart of mgs_fgcr does not project x).  Two
 * streaming launches beside a one-workgroup fold and 24 B per row for every projection.  MGS_ERR_INVALID: A is declared and is a row shard; h is
 * given and its fine operator carries another kind than A (a hierarchy built for a regular twin of A).  Without the declaration no
 * projection is launched. */
int mgs_pcg(const mgs_csr *A, mgs_vec *x, const mgs_vec *b, mgs_hier *h, int flexible,
            int *max_iter, double *tol, int *status);

/* Preconditioned MINRES for symmetric A that may be indefinite (saddle-point systems [[A, Bᵀ], [B, −C]]: Stokes, mixed Darcy, KKT) with a
 * symmetric positive definite preconditioner.  Nearest reference line: src/CPU_Matlab/solve.m:28-33, whose driver chooses between pcg and
 * bicgstab; the reference has no MINRES.  Same in/out convention as mgs_pcg: x is the initial guess, *max_iter returns the iterations done
 * (for status 2 and 3 the iteration that stopped, 0 at the start), *tol the TRUE relative residual ‖b − A·x‖/‖b‖ whatever the status (one
 * more SpMV where none was just made).  h may be NULL (identity preconditioner).
 * The method is the form of Elman, Silvester and Wathen, Alg. 4.1 (Paige-Saunders); v and z̃ = M·v are stored unnormalised:
 *   start:  normb = ‖b‖ (1 if 0); v = b − A·x; resid = ‖v‖/normb, status 0 with 0 iterations if resid <= tol; z̃ = M·v; g2 = z̃·v, status 2
 *           unless g2 > 0; γ = √g2, γ_prev = 1, η = γ, κ = resid·normb/γ, s0 = s1 = 0, c0 = c1 = 1, w_prev = w = v_prev = 0.
 *   step j: q = A·z̃; δ = (q·z̃)/γ²; v_new = (1/γ)·q − (δ/γ)·v − (γ/γ_prev)·v_prev; z̃_new = M·v_new; gn2 = z̃_new·v_new, status 2 unless
 *           gn2 >= 0; γn = √gn2; a0 = c1·δ − c0·s1·γ, a1 = √(a0² + gn2), a2 = s1·δ + c0·c1·γ, a3 = s0·γ; status 3 if a1 == 0 (x not
 *           updated); cn = a0/a1, sn = γn/a1; w_new = ((1/γ)·z̃ − a3·w_prev − a2·w)/a1; x ← x + (cn·η)·w_new; η ← −sn·η; rotate.
 *   stop:   |η| is ‖r‖ in the M⁻¹ norm, not the 2-norm.  est = κ·|η|/normb after every step; when est < tol or γn == 0 the true residual is
 *           formed: below tol → status 0; else γn == 0 → status 3; else κ ← (true·normb)/|η| and the recurrence goes on undisturbed (no
 *           restart, no tuned constant).
 * *status: 0 converged (decided on the true residual only) / 1 max_iter / 2 z̃·v negative or not a number (the preconditioner is not
 * positive definite) / 3 the Krylov space is exhausted above the tolerance (a singular, inconsistent system).
 * Seven work vectors from the context's pool (mgs_bicgstab: eight, mgs_fgcr(10): 21), one cycle and one SpMV per iteration (mgs_bicgstab: two
 * of each), two host looks, 96 B per row of vector passes beside them (mgs_pcg: 80).  The cycle alternates between two (v, z̃) pairs and
 * replays from two cached graphs.  A's symmetry is the caller's responsibility, as in mgs_pcg.
 * MGS_ERR_INVALID, with a message: a NULL out parameter; vectors shorter than A's rows; x aliasing b; a hierarchy that is not a fixed
 * symmetric operator (nu1 != nu2, or a K-cycle set through mgs_hier_set_kcycle / mgs_hier_set_kcycle_entry; the additive form, a correction
 * scale and FP32 operands are allowed, as for mgs_pcg with flexible = 0); a row shard (the criteria of mgs_pcg_plan_create); an A or a
 * hierarchy that declares MGS_NULLSPACE_CONSTANT (the constant vector is not the null space of a saddle system).
 * A declared MGS_NULLSPACE_FIELDS (enclosed flow: the pressure constant) is served: the system solved is A·x = Πb, Π = I − Σ_f z_f·z_fᵀ/n_f.
 *   normb = ‖Πb‖ (1 if that is 0); the caller's b is only read.  x ← Πx before EVERY true residual (at the start, at every check, at the
 *   final one), and every true residual is Π(b − A·x); z̃ ← Π(M·v) after every preconditioner application (h = NULL included), so the
 *   preconditioner seen is ΠMΠ and every Lanczos vector stays in the range.  Status 0 is still decided only on the true residual of the
 *   returned x, whose fields have zero mean.  The hierarchy's fine operator must carry the same nfields and counts (see
 *   mgs_csr_set_nullspace_fields); one more projection per iteration is the only difference in launches.
 * Option "minres_nt" (default 0): the update pass stores its direction vector with the `nt` hint on operators nt_store covers (A/B knob). */
int mgs_minres(const mgs_csr *A, mgs_vec *x, const mgs_vec *b, mgs_hier *h,
               int *max_iter, double *tol, int *status);

/* ------------------------------------- PCG with device-resident scalars: enqueue-only solves, one host look per iteration */
/* Nearest reference line: src/CPU_Matlab/solve.m:28-31 (pcg); the reference has no counterpart for the asynchronous form.  mgs_pcg computes ρ, α, β
 * and the stopping test on the host: three host looks per iteration, each one draining the queue behind it, and the call cannot return before
 * the solve is over.  A plan keeps those scalars in one state block in device memory (normb, rho, rho_prev, alpha, beta, pq, zq, rr, resid,
 * true_resid; flags it, status, frozen, first, pending, wasted).  One-wave scalar-step kernels (INIT, RHO, PQ, RES, FINAL) turn the folded inner
 * products into the next scalars with the operations the host uses in mgs_pcg, the direction, residual and flush passes read α and β from the
 * state block, and everything else is the very launches mgs_pcg makes — so every bit of x agrees with mgs_pcg's.  An iteration is a fixed
 * launch sequence: cycle (or copy), projection (declared null space), dots + fold, RHO, direction, SpMV with p·q + fold, PQ, residual + fold, RES.
 * A solve that converges (by the recursion) or breaks down sets `frozen` on the device: later iterations change no vector the solve depends
 * on (their scalar steps count into `wasted`, their vector passes return at once; cycle, SpMV and reductions still run).
 *   create: borrows A and h (may be NULL); both must outlive the plan.  mgs_pcg's acceptance rules (flexible = 0 refuses nu1 != nu2 and the
 *     K-cycle; the null-space kinds of A and h must agree); runs mgs_csr_optimize(A); allocates r, z, p, q and the state block (inside the arena
 *     when one exists; not from the work-vector pool), a ring of posted results in mapped host memory, the partial-sum buffer, and runs one cycle
 *     on r = 1 so that the hierarchy's operands exist and the cycle is captured: no later call allocates.  r and z never move, so the cycle replays
 *     from one captured graph for the life of the plan.
 *   solve: mgs_pcg's contract — statuses 0/1/2/3, the *max_iter / *tol write-back, x = initial guess, status 0 only on the TRUE residual,
 *     restart from the true residual when the recursion had drifted — and mgs_pcg's bits, for every ahead >= 0.  The host looks once per
 *     iteration (RES posts iteration, status, frozen, resid and a ticket into the ring) and looks BEHIND the queue: iteration k is not enqueued
 *     before the outcome of iteration k − 1 − ahead has been seen, and never beyond *max_iter.  ahead = 0: a look per iteration, nothing
 *     speculative; a large ahead: one look at the end, up to `ahead` wasted iterations (ahead is clamped to 1022, the ring's size).  On a posted
 *     "recursion converged" the host flushes, projects, forms the true residual (a synchronising look) and either returns or clears `frozen`
 *     on the stream and enqueues again from the next iteration.
 *   enqueue: no host wait at all.  INIT, `iters` iterations, then FINAL: the predicated flush of x, the projection (declared null space),
 *     r = b − A·x, its norm, and the status: 0 only if the recursion froze as converged AND the true residual is below tol; 2 or 3 as found;
 *     else 1.  x and b must stay alive and untouched until the result is read or the stream is synchronised.  A second enqueue is ordered
 *     behind the first on the stream.
 *   result (synchronises): of the last enqueue: *iters_done = where the solve froze, or iters; *resid = the true relative residual; *status.
 *     Status 1 with iters_done < iters: the recursion had drifted — enqueue again, which starts from the true residual as mgs_pcg's restart
 *     does.  After a solve: what that solve returned.
 *   info: out = device bytes held, solves + enqueues so far, iterations enqueued by the last call, of those the iterations that ran frozen
 *     (cycle + SpMV wasted; known after solve / result), host waits the last call made, restarts from the true residual in the last call.
 *   A declared MGS_NULLSPACE_CONSTANT is honoured as in mgs_pcg: z is projected after every preconditioner application, ‖Πb‖ is the norm, x is
 *   projected before every true residual that may decide.
 * MGS_ERR_INVALID, with a message: a NULL argument; a matrix without rows; a row shard (A->cols > A->rows, a context that sums over ranks, a hierarchy with halo
 * columns, callbacks, native plans or a tail); h's fine operator carrying another null-space kind than A; vectors shorter than A's rows; x
 * aliasing b; ahead < 0; iters < 0.  MGS_ERR_STATE: the context's stream is being captured (capturing a whole solve is not supported). */
typedef struct mgs_pcg_plan mgs_pcg_plan;
int mgs_pcg_plan_create(const mgs_csr *A, mgs_hier *h, int flexible, mgs_pcg_plan **out);
int mgs_pcg_plan_destroy(mgs_pcg_plan *p);
int mgs_pcg_plan_solve(mgs_pcg_plan *p, mgs_vec *x, const mgs_vec *b, int ahead, int *max_iter, double *tol, int *status);
int mgs_pcg_plan_enqueue(mgs_pcg_plan *p, mgs_vec *x, const mgs_vec *b, int iters, double tol);
int mgs_pcg_plan_result(mgs_pcg_plan *p, int *iters_done, double *resid, int *status);
int mgs_pcg_plan_info(const mgs_pcg_plan *p, int64_t out[6]);

/* ------------------------------------- BiCGSTAB with device-resident scalars: enqueue-only solves, one host look per iteration */
/* Reference: BiCGSTABiml, src/common/bicg.cpp:74-136; the reference has no counterpart for the asynchronous form.  mgs_bicgstab computes ρ, α, ω, β and
 * three stopping tests on the host: four host looks per iteration (r̃·v, ‖s‖, (t·s, t·t), (‖r‖, r̃·r)), each one draining the queue behind it, and
 * the call cannot return before the solve is over.  A plan keeps those scalars in one state block in device memory (normb, rho, rho_next,
 * rho_prev, alpha, omega, beta, nbo = −β·ω, rtv, ts, tt, ss, rr, resid, true_resid; flags it, status (−1 running), frozen, first, half, wasted).
 * One-wave scalar-step kernels turn the folded inner products into the next scalars with the operations, in the order, the host uses in
 * mgs_bicgstab; the vector passes read their coefficients from the state block and evaluate the expressions of the kernels mgs_bicgstab runs
 * (a·x + b·y (+ c·z), unfused; the passes with sums with k_update_dot2's grids, partial layout and fold), and everything else is the very
 * launches mgs_bicgstab makes — so every bit of x agrees with mgs_bicgstab's.  One iteration i is a fixed launch sequence:
 *   RHO     :95     rho = the r̃·r the last residual pass (or INIT) left
 *           :96-99  rho == 0: frozen, status 2; resid keeps √(r·r)/‖b‖
 *           :103    not the first iteration: beta = (rho/rho_prev)·(alpha/omega), nbo = −beta·omega
 *   p-pass  :100-101 first: p ← r;  :104 else p = 1.0·r + nbo·v + beta·p
 *   cycle   :106    p̂ = M·p (a copy when h is NULL), projected when the null space is declared
 *   SpMV    :107    v = A·p̂ with r̃·v from the same pass
 *   ALPHA   :108    alpha = rho/(r̃·v); no test for zero: a non-finite alpha propagates as in mgs_bicgstab
 *   s-pass  :109    s = 1.0·r + (−alpha)·v with ‖s‖²
 *   HALF    :110    resid = ‖s‖/‖b‖; below tol: frozen, status 0, half = 1
 *   cycle   :116    ŝ = M·s, projected likewise
 *   SpMV    :117    t = A·ŝ with (t·s, t·t)
 *   OMEGA   :118    omega = (t·s)/(t·t)
 *   x-pass  :119    x = alpha·p̂ + omega·ŝ + 1.0·x;  :111 frozen with half: x = alpha·p̂ + 1.0·x (p̂ is intact: p did not change)
 *   r-pass  :120    r = 1.0·s + (−omega)·t with (‖r‖², r̃·r)
 *   RES     :122    rho_prev = rho;  :123-127 resid = ‖r‖/‖b‖ below tol: frozen, status 0;  :128-131 else omega == 0: frozen, status 3; the post
 * Nothing on the host depends on a device value.  Once `frozen` is set, later iterations change no vector the solve depends on: their scalar
 * steps do nothing (RHO counts into `wasted`), their vector passes return at once (the half-step x-pass excepted); cycles, SpMVs and folds
 * still run.  INIT (:80-92): ‖b‖ (‖Πb‖ with a declared null space), 0 replaced by 1; r = b − A·x, projected likewise; r̃ ← r; (‖r‖², r̃·r);
 * resid <= tol: frozen, status 0, iteration 0.
 *   create: borrows A and h (may be NULL); both must outlive the plan.  mgs_bicgstab's acceptance rules (the null-space kinds of A and h must
 *     agree); runs mgs_csr_optimize(A); allocates p, p̂, s, ŝ, t, v, r, r̃ and the state block (inside the arena when one exists; not from the
 *     work-vector pool), a ring of 1024 posted results of 64 bytes in mapped host memory, the partial-sum buffer, and runs the cycles p → p̂
 *     and s → ŝ on ones so that the hierarchy's operands exist and both cycles are captured: no later call allocates.  The vectors never move,
 *     so the two cycles replay from two captured graphs for the life of the plan.
 *   solve: mgs_bicgstab's contract and bits for every ahead >= 0 (clamped to 1022).  Write-back as mgs_bicgstab: status 0: *max_iter = the
 *     iteration, *tol = resid; statuses 2 and 3: *tol only, *max_iter untouched; status 1: *tol = resid; *max_iter = 0: status 1 unless INIT
 *     converged.  Status 0 is decided on the recursive residual, as in mgs_bicgstab; there is no restart branch.  The host looks once per
 *     iteration (RES posts ticket, iteration, status, frozen, wasted, resid, ‖b‖ into the ring) and looks BEHIND the queue: iteration k is
 *     not enqueued before the post of iteration k − 1 − ahead has been seen, and never beyond *max_iter; on a frozen post the host stops
 *     enqueuing.  With a declared null space x ← Πx follows the last update, before the call returns.
 *   enqueue: no host wait at all.  INIT, `iters` iterations, then FINAL: x ← Πx (declared null space), the true residual b − A·x into t
 *     (projected likewise), true_resid = ‖t‖/‖b‖, and the status: 0 only if the recursion froze as converged AND true_resid is below tol; 2
 *     or 3 as found; else 1.  x and b must stay alive and untouched until the result is read or the stream is synchronised.
 *   result (synchronises): of the last enqueue: *iters_done = where the solve froze, or iters; *resid = the true relative residual;
 *     *recursive_resid (may be NULL) = the recursion's; *status.  Status 1 with iters_done < iters: the recursion had drifted — enqueue
 *     again; x is then the initial guess.  (mgs_bicgstab itself has no true-residual confirmation and does not change.)  After a solve:
 *     what that solve returned.
 *   info: out = device bytes held, solves + enqueues so far, iterations enqueued by the last call, of those the iterations that ran frozen
 *     (known after solve / result), host waits the last call made, 0 (the PCG plan's restarts; there is no restart here).
 * MGS_ERR_INVALID, with a message: a NULL argument; a matrix without rows; a row shard (A->cols > A->rows, a context that sums over ranks, a
 * hierarchy with halo columns, callbacks, native plans or a tail); h's fine operator carrying another null-space kind than A; vectors shorter
 * than A's rows; x aliasing b; ahead < 0; iters < 0.  MGS_ERR_STATE: the context's stream is being captured. */
typedef struct mgs_bicgstab_plan mgs_bicgstab_plan;
int mgs_bicgstab_plan_create(const mgs_csr *A, mgs_hier *h, mgs_bicgstab_plan **out);
int mgs_bicgstab_plan_destroy(mgs_bicgstab_plan *p);
int mgs_bicgstab_plan_solve(mgs_bicgstab_plan *p, mgs_vec *x, const mgs_vec *b, int ahead, int *max_iter, double *tol, int *status);
int mgs_bicgstab_plan_enqueue(mgs_bicgstab_plan *p, mgs_vec *x, const mgs_vec *b, int iters, double tol);
int mgs_bicgstab_plan_result(mgs_bicgstab_plan *p, int *iters_done, double *resid, double *recursive_resid, int *status);
int mgs_bicgstab_plan_info(const mgs_bicgstab_plan *p, int64_t out[6]);

/* ------------------------------------- flexible GCR with device-resident coefficients: enqueue-only solves, one host look per iteration */
/* Nearest reference line: the Krylov call of src/CPU_Matlab/solve.m:28-33; the reference has no flexible method and no asynchronous form.  mgs_fgcr
 * fetches three results per iteration (the h_j of the multi-dot, (ρ_k, t) of the orthogonalisation pass, ‖r‖² of the residual pass), hands the
 * coefficients U_jk = h_j/ρ_j to the orthogonalisation kernel by value, solves (I + U)·y = α on the host when a window closes and cannot
 * return before the solve is over.  A plan keeps them in one state block in device memory (normb, resid, true_resid, rr; ρ, α, h, y, cf = −y of
 * 16 entries each; U of 16 × 16; flags it, status (−1 running), frozen, why, m_open, wasted).  One-wave scalar-step kernels form every scalar
 * with the operation, in the order, the host code of mgs_fgcr uses; three vector passes read their coefficients from the state block and
 * evaluate the expressions of the kernels mgs_fgcr runs (maxpy_dot2_kernel's z = x − Σ cf_j·w_j with its 16-byte and 8-byte arms, grid, partial
 * layout and fold; k_update_dot2's 1.0·r + (−α_k)·v with its launch decisions and store rule); everything else is the very launches mgs_fgcr
 * makes — so every bit of x agrees with mgs_fgcr's.  One iteration at window slot k (the host always knows k) is a fixed launch sequence:
 *   cycle   C[k] = M·r (a copy when h is NULL), projected when the null space is declared
 *   SpMV    V[k] = A·C[k]
 *   dots    k = 0: (V[0]·V[0], V[0]·r) by k_dot2;  k > 0: h_j = V[j]·V[k], j < k, by k_mdot into the state block
 *   COEF    U_jk = ρ_j != 0 ? h_j/ρ_j : 0
 *   orth    V[k] ← V[k] − Σ_{j<k} U_jk·V[j] with (V[k]·V[k], V[k]·r)                                      (k > 0)
 *   RHOK    ρ_k, t from the fold; m_open = k + 1; ρ_k == 0: α_k = 0, frozen as "breakdown"; else α_k = t/ρ_k
 *   r-pass  r ← 1.0·r + (−α_k)·V[k] with ‖r‖²
 *   RES     resid = √(‖r‖²)/‖b‖; below tol: frozen as "the recursion says converged"; the post, unless the iteration closes its window
 * and a window close is
 *   YSOLVE  (I + U)·y = α over the m_open directions by back substitution, cf_j = −y_j
 *   x-pass  x ← x − Σ_{j<m_open} cf_j·C[j]; guarded by m_open, not by frozen
 *   x ← Πx  where mgs_fgcr projects (a close that may decide a return), declared null space only
 *   r = b − A·x (projected likewise) and its norm
 *   WIN     resid = the true residual; running and below tol: frozen, status 0; frozen as "the recursion says converged": status 0, or "drifted";
 *           frozen as "breakdown": status 0 or 2; m_open = 0; the post
 * Once `frozen` is set, later iterations change no vector the solve depends on: COEF, RHOK and RES do nothing (RHOK counts into `wasted`), the
 * orth and r passes return at once, and cycle and SpMV write C[k], V[k] of slots behind the open ones only.  The first close after a freeze
 * applies the open window once; every later close is a no-op.  INIT: ‖b‖ (‖Πb‖), 0 replaced by 1; x ← Πx; r = b − A·x; resid <= tol: frozen,
 * status 0, iteration 0.
 *   create: borrows A and h (may be NULL); both must outlive the plan.  restart in 1..16 (one multi-vector pass holds 16 vectors, a hierarchy
 *     caches 16 captured cycles; mgs_fgcr itself keeps 1..64).  mgs_fgcr's acceptance rules (the null-space kinds of A and h must agree); runs
 *     mgs_csr_optimize(A); allocates r, C[0..restart), V[0..restart) and the state block (inside the arena when one exists; not from the
 *     work-vector pool), a ring of 1024 posted results of 64 bytes in mapped host memory, the partial-sum buffer, and runs the cycle r → C[k]
 *     once for every k so that the hierarchy's operands exist and the cycles are captured: no later call allocates.
 *   solve: mgs_fgcr's contract and bits for every ahead >= 0 (clamped to 1022): statuses 0/1/2, *max_iter = the iterations run and *tol = the
 *     residual on every path, status 0 only on the true residual, `<=` at iteration 0 and `<` later.  The host looks once per iteration, BEHIND
 *     the queue: iteration k is not enqueued before the post of iteration k − 1 − ahead has been seen, and never beyond *max_iter.  On a posted
 *     "the recursion says converged" or "breakdown" the host stops enqueuing, enqueues close, projection and true residual, and looks: it
 *     returns, or ("drifted") clears `frozen` on the stream and goes on from the next iteration with an empty window — mgs_fgcr's restart from
 *     the true residual.  The close behind the last iteration of all is enqueued behind its look as well.
 *   enqueue: no host wait at all.  INIT, `iters` iterations with a scheduled close every `restart` iterations, then FINAL: the open window is
 *     closed, x ← Πx (declared null space), the true residual b − A·x, and the status: 0 only if the true residual is below tol; 2 for a
 *     breakdown whose true residual is not; else 1.  There is no restart from the true residual on the device.  x and b must stay alive and
 *     untouched until the result is read or the stream is synchronised.
 *   result (synchronises): of the last enqueue: *iters_done = where the solve froze, or iters; *resid = the true relative residual;
 *     *recursive_resid (may be NULL) = the recursion's; *status.  Status 1 with iters_done < iters: the recursion had drifted — enqueue again
 *     from x.  After a solve: what that solve returned.
 *   info: out = device bytes held, solves + enqueues so far, iterations enqueued by the last call, of those the iterations that ran frozen
 *     (known after solve / result), host waits the last call made, restarts from the true residual after a drifted convergence in the last call.
 * MGS_ERR_INVALID, with a message: a NULL argument; a matrix without rows; a row shard (A->cols > A->rows, a context that sums over ranks, a
 * hierarchy with halo columns, callbacks, native plans or a tail); h's fine operator carrying another null-space kind than A; vectors shorter
 * than A's rows; x aliasing b; ahead < 0; iters < 0; restart outside 1..16.  MGS_ERR_STATE: the context's stream is being captured. */
typedef struct mgs_fgcr_plan mgs_fgcr_plan;
int mgs_fgcr_plan_create(const mgs_csr *A, mgs_hier *h, int restart, mgs_fgcr_plan **out);
int mgs_fgcr_plan_destroy(mgs_fgcr_plan *p);
int mgs_fgcr_plan_solve(mgs_fgcr_plan *p, mgs_vec *x, const mgs_vec *b, int ahead, int *max_iter, double *tol, int *status);
int mgs_fgcr_plan_enqueue(mgs_fgcr_plan *p, mgs_vec *x, const mgs_vec *b, int iters, double tol);
int mgs_fgcr_plan_result(mgs_fgcr_plan *p, int *iters_done, double *resid, double *recursive_resid, int *status);
int mgs_fgcr_plan_info(const mgs_fgcr_plan *p, int64_t out[6]);

/* ------------------------------------- MINRES with device-resident scalars: enqueue-only solves, one host look per iteration */
/* Nearest reference line: src/CPU_Matlab/solve.m:28-33; the reference has neither MINRES nor an asynchronous form.  mgs_minres forms δ, the Lanczos
 * coefficients, the Givens rotation and the stopping estimate on the host: two host looks per iteration (q·z̃ and γn² = z̃_new·v_new), each one
 * draining the queue behind it, and the call cannot return before the solve is over.  A plan keeps those scalars in one state block in device
 * memory (normb, γ, γ_prev, η, κ, δ, s0, s1, c0, c1; the coefficients of the two vector passes; resid = the estimate κ·|η|/‖b‖, after INIT the
 * initial true residual; true_resid; flags it, status (−1 running), frozen, why (the estimate fell below tol / γn == 0), wasted, apply).
 * One-wave scalar-step kernels form every scalar with the operations, in the order, of mgs_minres's host code; the Lanczos pass reads
 * (a, b, c) from the state block and evaluates axpbypcz's expression a·q + b·v + c·v_prev with its 16-byte and 8-byte arms, grids and store hint;
 * the update pass reads (1/γ, a3, a2, a1, step) and evaluates the expression of mgs_minres's own pass with its two arms, launch decisions and
 * option "minres_nt"; everything else is the very launches mgs_minres makes — so every bit of x agrees with mgs_minres's.  One iteration j is a
 * fixed launch sequence, (v, z̃) and (w, w_prev) alternating by the parity of j:
 *   SpMV     q = A·z̃ with q·z̃ from the same pass
 *   LANCZOS  δ = (q·z̃)/(γ·γ); a = 1/γ, b = −(δ/γ), c = −(γ/γ_prev)
 *   pass     v_new = a·q + b·v + c·v_prev over v_prev
 *   cycle    z̃_new = M·v_new (a copy when h is NULL)
 *   dot      γn² = z̃_new·v_new
 *   ROTATE   γn² negative or not a number: frozen, status 2; a0 .. a3 as in mgs_minres; a1 == 0: frozen, status 3, x not updated; cn = a0/a1,
 *            sn = γn/a1, step = cn·η, apply = 1; η ← −sn·η; the rotation; est = κ·|η|/‖b‖; est < tol or γn == 0: frozen, status 0, why; the post
 *   pass     apply: w_new = ((1/γ)·z̃ − a3·w_prev − a2·w)/a1 over w_prev, x ← x + step·w_new
 * The iteration that freezes as converged still applies its update, as mgs_minres updates x before it tests: the update pass is predicated on
 * `apply`, which the next LANCZOS step clears, not on `frozen`.  Once `frozen` is set, the scalar steps do nothing (LANCZOS counts into
 * `wasted`) and the two passes return at once; SpMV, cycle and folds still run.  That is not only scratch here: a frozen iteration's cycle
 * rewrites a z̃ from its unchanged v, and every second one rewrites the live z̃ — with the same bits, because the cycle is deterministic.
 * INIT is mgs_minres's start: ‖b‖, 0 replaced by 1; v = b − A·x; resid <= tol: frozen, status 0, iteration 0; z̃ = M·v; g2 = z̃·v, status 2
 * unless g2 > 0; γ = √g2, γ_prev = 1, η = γ, κ = resid·‖b‖/γ; v_prev = w_prev = w = 0.
 *   create: borrows A and h (may be NULL); both must outlive the plan.  mgs_minres's acceptance rules: nu1 == nu2, no K-cycle and no K-cycle
 *     entry, no MGS_NULLSPACE_CONSTANT on A or on h's fine operator (MGS_NULLSPACE_FIELDS is served as in mgs_minres: the same projections at
 *     the same places, as enqueued launches with the means on the device, no host read added); the additive form, a correction scale and FP32 operands are allowed.  Runs
 *     mgs_csr_optimize(A); allocates v ×2, z̃ ×2, q, w ×2 and the state block (inside the arena when one exists; not from the work-vector
 *     pool), a ring of 1024 posted results of 64 bytes in mapped host memory, the partial-sum buffer, and runs one cycle on each (v[k], z̃[k])
 *     pair with ones, so that the hierarchy's operands exist and both cycles are captured: two cached graphs for the life of the plan, and
 *     no later call allocates.
 *   solve: mgs_minres's contract and bits for every ahead >= 0 (clamped to 1022): statuses 0/1/2/3, *max_iter = the iterations done (for
 *     statuses 2 and 3 the iteration that stopped), *tol = the TRUE relative residual on every path.  The host looks once per iteration,
 *     BEHIND the queue: iteration k is not enqueued before the post of iteration k − 1 − ahead has been seen, and never beyond *max_iter.  On
 *     a posted freeze with status 0 the host forms the true residual into q (a synchronising look, as in mgs_minres): below tol → 0; γn == 0
 *     → 3; at *max_iter → 1; otherwise it enqueues the recalibration step (κ = resid·‖b‖/|η| with the true residual passed by value, frozen
 *     cleared) and enqueues again the iterations that ran frozen.  The recurrence is never restarted.  On statuses 2 and 3 and when the
 *     iterations are used up it forms the true residual before it returns.
 *   enqueue: no host wait at all.  INIT, `iters` iterations, then FINAL: the true residual b − A·x into q and the status: 0 only if the solve
 *     froze on its estimate or on γn == 0 AND the true residual is below tol (`<=` at iteration 0); 3 for γn == 0 above tol; 2 or 3 as found;
 *     else 1.  THERE IS NO RECALIBRATION ON THE DEVICE: status 1 with iters_done < iters means the estimate ran ahead of the 2-norm — enqueue
 *     again from x, which measures κ afresh.  tol = 0 runs exactly `iters` iterations.  x and b must stay alive and untouched until the result
 *     is read or the stream is synchronised.
 *   result (synchronises): of the last enqueue: *iters_done = where the solve froze, or iters; *resid = the true relative residual;
 *     *recursive_resid (may be NULL) = the estimate; *status.  After a solve: what that solve returned.
 *   info: out = device bytes held, solves + enqueues so far, iterations enqueued by the last call, of those the iterations that ran frozen
 *     (known after solve / result), host waits the last call made, recalibrations in the last call.
 * MGS_ERR_INVALID, with a message headed mgs_minres_plan_*: a NULL argument; a matrix without rows; a row shard (the criteria of
 * mgs_pcg_plan_create); a hierarchy that is not a fixed symmetric operator; a declared constant null space; vectors shorter than A's rows; x aliasing
 * b; ahead < 0; iters < 0.  MGS_ERR_STATE: the context's stream is being captured. */
typedef struct mgs_minres_plan mgs_minres_plan;
int mgs_minres_plan_create(const mgs_csr *A, mgs_hier *h, mgs_minres_plan **out);
int mgs_minres_plan_destroy(mgs_minres_plan *p);
int mgs_minres_plan_solve(mgs_minres_plan *p, mgs_vec *x, const mgs_vec *b, int ahead, int *max_iter, double *tol, int *status);
int mgs_minres_plan_enqueue(mgs_minres_plan *p, mgs_vec *x, const mgs_vec *b, int iters, double tol);
int mgs_minres_plan_result(mgs_minres_plan *p, int *iters_done, double *resid, double *recursive_resid, int *status);
int mgs_minres_plan_info(const mgs_minres_plan *p, int64_t out[6]);

/* ------------------------------------- projected initial guesses for successive right-hand sides */
/* Nearest reference line: none: the reference solves one right-hand side, bicg.cpp:159-166.  A caller who solves with the same operator again and
 * again (time stepping, Picard / Newton, the pressure Poisson equation) gets a better start than its last solution by projecting the new
 * right-hand side onto the span of the last few solutions (Fischer 1998; PETSc: KSPGuessFischer).  The guess holds size <= capacity pairs
 * (x̃_k, ỹ_k = A·x̃_k), both n doubles, normalised so that <x̃_j, ỹ_k> = δ_jk (MGS_GUESS_ENERGY: A symmetric positive definite, x0 minimises
 * ‖x − x0‖_A over the span) or <ỹ_j, ỹ_k> = δ_jk (MGS_GUESS_RESIDUAL: any nonsingular A, x0 minimises ‖b − A·x0‖₂ over the span); q_k names the
 * vector that is dotted, x̃_k resp. ỹ_k.  Both kinds store pairs: one code path, and no operation but the update's own needs an SpMV.
 * A is borrowed and must outlive the guess.  The 2·capacity vectors, the partial sums and the device scalars are allocated at create (inside
 * the arena when one exists); the update's two scratch vectors come from the context's work-vector pool (mgs_ctx_trim releases them).
 *   apply:  α_k = <q_k, b> in one pass over b and the q_k, then x0 = Σ_k α_k·x̃_k; α stays in device memory between the two launches.  Without
 *     rel_resid the call makes no host round trip and is enqueued on the context's stream.  With rel_resid the second pass also forms
 *     r0 = b − Σ α_k·ỹ_k (not stored), *rel_resid = ‖r0‖/‖b‖ and the call synchronises.  An empty basis gives x0 = 0 and *rel_resid = 1.
 *   update(x): x is a solution the caller just computed (its right-hand side is not needed).  w = A·x (mgs_spmv); c¹_k = <q_k, w> and
 *     ν0² = <x, w> (ENERGY) or <w, w> (RESIDUAL) in one pass; the pair pass x' = x − Σ c¹_k·x̃_k, w' = w − Σ c¹_k·ỹ_k (into the free slot), which also accumulates
 *     c²_k = <q_k, w'> and ν1²; the pair pass again with c², giving x'', w'' and ν2² (classical Gram-Schmidt, twice); one workgroup decides on
 *     the device; a store pass predicated on that decision writes x̃ = s·x'', ỹ = s·w'', s = 1/√ν2², into slot `size` — the only copy out of
 *     scratch.  The host reads one flag at the end.  Accepted (DGKS, η = 1/√2): ν2² finite and positive, ν2² >= ν1²/2, ν0² > 0 and ν2 > 32·2⁻⁵²·ν0 (what the first pass
 *     leaves of a candidate inside the span is rounding noise, which the second pass barely shortens: the floor, PETSc's drop tolerance, refuses it).  A candidate
 *     whose norm falls further in the second pass lies numerically inside the span; an ENERGY candidate with ν0² <= 0 means A is not positive
 *     along x: neither is added, *added = 0 (added may be NULL) and the "refused" counter goes up.  size == capacity: the basis restarts from
 *     the candidate alone (Fischer's restart: nothing is orthogonalised, ν1² = ν2² = ν0², slot 0 takes the normalised (x, w), size = 1, the
 *     restart counter goes up) — measured better than dropping the oldest pair, which carries the bulk of the solution.
 *   rebase: A's values changed (mgs_csr_update_values*): reset followed by update(x̃_k) from the oldest to the newest, in place; every ỹ is
 *     recomputed with the current values.   reset: size = 0; the counters stay.
 *   A declared MGS_NULLSPACE_CONSTANT: update works on a zero-mean copy of x, so every x̃_k and with them x0 have zero mean; a constant
 *     candidate whose mean is exact (e.g. all ones) has ν0² = 0 and is refused.
 *   Arithmetic: every elementwise result is a sum of products in ascending k starting from the first product (x' = x − (c_0·x̃_0 + c_1·x̃_1 + …)),
 *     one rounding per product and per sum, so a host restatement given the coefficient bits reproduces x0, x', w' and the stored pairs bit
 *     for bit; partial sums have a fixed layout and a fixed-order fold, no atomics: two identical calls give identical bits.  16-byte accesses
 *     where the caller's vectors are 16-byte aligned, 8-byte ones otherwise — the same bits.
 *   info: out = size, capacity, kind, restarts, candidates refused, device bytes held.
 *   coef (tests and diagnostics; synchronises): after an apply α_0..α_{K−1}; after an update c¹_0..c¹_{K−1}, c²_0..c²_{K−1}, ν0², ν1², ν2², s,
 *     the accept flag (K = the pairs the call ran against); entries beyond that are 0.
 *   gram (tests and diagnostics; synchronises): host[j·size + k] = <q_j, ỹ_k>.
 *   pair (tests and diagnostics; enqueued): copies of x̃_k and ỹ_k, 0 <= k < size.  k = size < capacity reads the free slot, which the first
 *     Gram-Schmidt pass uses as its output: after a refused update that orthogonalised it holds that candidate's x' and w'.
 * MGS_ERR_INVALID, with a message: a NULL argument (rel_resid, added excepted); an unknown kind; a capacity outside 1..16; A not square or with
 * halo columns (cols > rows: a row shard); vectors shorter than A's rows; x0 aliasing b. */
typedef struct mgs_guess mgs_guess;
#define MGS_GUESS_ENERGY 0
#define MGS_GUESS_RESIDUAL 1
int mgs_guess_create(const mgs_csr *A, int kind, int capacity, mgs_guess **out);
int mgs_guess_destroy(mgs_guess *g);
int mgs_guess_apply(mgs_guess *g, const mgs_vec *b, mgs_vec *x0, double *rel_resid);
int mgs_guess_update(mgs_guess *g, const mgs_vec *x, int *added);
int mgs_guess_rebase(mgs_guess *g);
int mgs_guess_reset(mgs_guess *g);
int mgs_guess_info(const mgs_guess *g, int64_t out[6]);
int mgs_guess_coef(const mgs_guess *g, double *host, int n);
int mgs_guess_gram(mgs_guess *g, double *host);
int mgs_guess_pair(const mgs_guess *g, int k, mgs_vec *x, mgs_vec *y);

/* ------------------------------------------------------------- multi-GPU row shards   */
/* Halo plan of a row-range shard whose CSR uses LOCAL column numbering: columns
 * [0,n_loc) are owned rows, columns n_loc+k are halo slot k.  send_idx lists the owned
 * rows this rank must pack for its peers (concatenated in peer order).  The pack kernel
 * gathers x[send_idx] into send_buf; the exchange itself is done by the caller (RCCL via
 * torch.distributed) between mgs_halo_pack and the next kernel that reads x's halo.   */
int mgs_halo_pack(mgs_ctx *ctx, const mgs_vec *x, const int *send_idx_dev, int64_t n_send,
                  double *send_buf_dev);
/* exchange callback installed on a hierarchy: called with (user, level, x_dev) before
 * every kernel that gathers off-shard entries of x on that level; x_dev has n_loc +
 * n_halo entries and the callee must fill x_dev[n_loc..] on ctx's stream.             */
typedef int (*mgs_halo_fn)(void *user, int level, void *x_dev);
int mgs_hier_set_halo_exchange(mgs_hier *h, mgs_halo_fn fn, void *user);
/* Split-phase form: begin(user, level, x) packs and STARTS the exchange, end(...) waits for it.
 * Between the two the library launches the kernel on the shard's interior row blocks (those that
 * read no halo column), afterwards on the boundary row blocks — the exchange hides behind ~97 %
 * of the rows of a plane-sharded stencil operator.  Falls back to fn for levels whose halo
 * readers are not a prefix + suffix of the row range.                                          */
int mgs_hier_set_halo_exchange_split(mgs_hier *h, mgs_halo_fn begin, mgs_halo_fn end, void *user);
/* Halo exchange of the fused cycle passes on a row shard (kind is always 2: plain values).  The callee delivers, for every halo
 * slot of `level`, the entry of the owner's vector `a` (owned entries of that level on every rank) that the slot stands for, into
 * halo_out — a payload buffer (pre pass: a = the right-hand side; the owners' ωD⁻¹ sits in Â's halo columns since setup) or the halo
 * room of the vector itself (post pass: a = e_c of the coarse level, level = that coarse level).  b is NULL.  phase 0 packs
 * (mgs_halo_pack) and starts the exchange, phase 1 waits for it; the library launches the interior row blocks in between.
 * Without this callback (and without a native plan) a sharded hierarchy runs the one-kernel-per-step form.                */
typedef int (*mgs_halo_fused_fn)(void *user, int level, int kind, const void *a, const void *b, void *halo_out, int phase);
int mgs_hier_set_halo_exchange_fused(mgs_hier *h, mgs_halo_fused_fn fn, void *user);

/* Building blocks of a row-sharded hierarchy (one process per GPU; orchestration in
 * multigridsolver_amd/dist.py).  mgs_aggregate_shard: pairwise aggregation of the OWNED
 * rows only (aggregates never straddle a shard; couplings to halo columns enter s_i and the
 * G0 test as symmetric and never pair; among the owned columns the matching runs on the pattern
 * mgs_hier_coarsen describes: the union of A's and Aᵀ's when A's is not symmetric).  The caller then learns the remote aggregate of every halo slot from
 * its peers and passes the coarse column of each halo slot (host array, n_halo ints, values
 * in [n_coarse, n_coarse+n_halo_coarse) or −1) to mgs_galerkin_shard, which returns the coarse
 * shard (n_coarse rows, n_coarse+n_halo_coarse local columns).  mgs_hier_push_level appends
 * the pair to a hierarchy and takes ownership of both.                                  */
int mgs_aggregate_shard(const mgs_csr *A, double ktg, int npass, double tou, mgs_xfer **T);
/* ... with zones (host array, one int per owned row; NULL = none): rows of different zones never share an aggregate.  Giving the rows each
 * peer sees as halo a zone of their own keeps what that peer asks for at the next level a contiguous id range (plane shards), so every halo
 * exchange of the hierarchy sends ranges straight from the vectors. */
int mgs_aggregate_shard_zoned(const mgs_csr *A, double ktg, int npass, double tou, const int *zone, mgs_xfer **T);
int mgs_galerkin_shard(const mgs_csr *A, const mgs_xfer *T, const int *halo_coarse_col,
                       int n_halo_coarse, mgs_csr **Ac);
int mgs_hier_push_level(mgs_hier *h, mgs_xfer *T, mgs_csr *Ac);
/* aggregation transfer from a host array of aggregate ids (−1 = none)                   */
int mgs_xfer_from_agg(mgs_ctx *ctx, int n_fine, int n_coarse, const int *agg, mgs_xfer **out);
/* coarsest-level solver callback (x_dev = solve(b_dev), both of the coarsest level's owned
 * size) — used for the replicated tail of a sharded hierarchy; replaces the dense inverse. */
typedef int (*mgs_coarse_fn)(void *user, const void *b_dev, void *x_dev);
int mgs_hier_set_coarse_solver(mgs_hier *h, mgs_coarse_fn fn, void *user);
/* reduction callback for dot products of sharded vectors (sum over ranks)             */
typedef int (*mgs_allreduce_fn)(void *user, double *host_scalars, int count);
int mgs_ctx_set_allreduce(mgs_ctx *ctx, mgs_allreduce_fn fn, void *user);

/* ------------------------------------------------------------------ instrumentation  */
/* Time `reps` back-to-back launches of one hot-path kernel with hipEvents on the
 * context's stream (what bench.py's roofline.achieved uses).  op: 0 spmv, 1 residual,
 * 2 jacobi, 3 the update pass of mgs_minres over A's rows (x = z̃, b = w, dinv = w_prev,
 * out = the solution; fixed coefficients; the matrix itself is not read).  Returns mean
 * milliseconds per launch in *ms.                                                      */
int mgs_time_kernel(const mgs_csr *A, int op, const mgs_vec *x, const mgs_vec *b,
                    const mgs_vec *dinv, mgs_vec *out, int reps, double *ms);
/* Time `reps` V-cycles with hipEvents on the context's stream.                        */
int mgs_time_vcycle(mgs_hier *h, const mgs_vec *b, mgs_vec *x, int reps, double *ms);
/* launch plan of a matrix (diagnostics): out[0]=max entries of a 256-row block, [1]=max row
 * length, [2]=far band (max |col−row| over owned columns), [3]=LDS bytes per workgroup of the
 * row-block kernel, [4]=leading and [5]=trailing row blocks that read halo columns, [6]=1 if the
 * interior/boundary split is usable, [7]=1 if some block takes the long-row path.            */
int mgs_csr_plan_info(const mgs_csr *A, int64_t out[8]);
/* "origin" of the rows of a coarse operator built by the device setup: the finest-level row each row descends from (leader of its
 * aggregate, chained through the levels).  The pairwise matching breaks ties between equally strong neighbours in that index space
 * (nearest first, then even multiples of the stride), which keeps aggregates aligned on grid-like problems on every level.  A row-sharded
 * hierarchy hands the origins of its last sharded level (shifted to global finest-level rows) to the replicated tail with these two
 * calls.  get: returns 1 and writes nothing when the operator carries none (= identity).  No reference counterpart (the reference's
 * sequential matching scans neighbours in index order, AGMG.cpp:149-179).
 * set: the origins must be non-negative and distinct (the tie-break key divides by the distance of two origins); they may exceed the
 * row count (the shifted origins of a replicated tail).  Anything else is refused with MGS_ERR_INVALID before the matrix changes.
 * origin_host = NULL removes the origins (= identity). */
int mgs_csr_get_origin(const mgs_csr *A, int *origin_host);
int mgs_csr_set_origin(mgs_csr *A, const int *origin_host);
/* ---- native RCCL transport of a row-sharded hierarchy (no reference counterpart: the reference is single-process) ----
 * One communicator per process/GPU.  librccl is resolved at run time from `librccl_path` — pass the copy the launcher
 * already loaded (for torch.distributed: <torch>/lib/librccl.so) so the process holds a single RCCL instance.  Rank 0
 * calls mgs_comm_unique_id and ships the MGS_COMM_ID_BYTES bytes to the other ranks by any means; every rank then
 * calls mgs_comm_create.  All communication is enqueued on the context's stream.
 *   mgs_hier_set_native_exchange: halo plan of `level` — send_idx (host): owned rows the peers need, peer after peer;
 *     send_counts/recv_counts: per peer; the received values fill the level's halo slots in peer order.  With a plan
 *     installed the cycle packs and exchanges by itself (ncclSend/ncclRecv group) and ignores the exchange callbacks
 *     for that level.  comm = NULL removes the plan.
 *   mgs_hier_set_native_tail: the coarsest sharded level is all-gathered (ncclAllGather) and solved by `tail`, an
 *     unsharded hierarchy on the globally assembled operator replicated on every rank; nlocs = rows per rank.
 *   mgs_hier_native_halo: one plain halo exchange of the level-`level` vector x_dev (owned entries + halo room).
 *   mgs_hier_native_send_segments / mgs_hier_set_native_recv_segments: pack-free exchanges.  Where a peer's rows are a few
 *     contiguous ranges (plane shards: one), they are sent straight from the source vector, one ncclSend per range, and the
 *     peer posts one ncclRecv per range.  Each rank reads what it will send (ranges per peer + their lengths; returns the number
 *     of lengths), the host side ships the lengths to the peers, and every rank installs what it will receive — a COLLECTIVE
 *     step: from that call on the rank itself sends ranges.  Without it every exchange goes through the pack kernel.  */
#define MGS_COMM_ID_BYTES 128
typedef struct mgs_comm mgs_comm;
int mgs_comm_unique_id(mgs_ctx *ctx, const char *librccl_path, void *id_out);
int mgs_comm_create(mgs_ctx *ctx, const char *librccl_path, const void *id, int world, int rank, mgs_comm **out);
int mgs_comm_destroy(mgs_comm *c);
int mgs_comm_size(const mgs_comm *c, int *world, int *rank);
int mgs_hier_set_native_exchange(mgs_hier *h, int level, mgs_comm *c, const int *send_idx, const int *send_counts, const int *recv_counts);
int mgs_hier_set_native_tail(mgs_hier *h, mgs_comm *c, mgs_hier *tail, const int *nlocs);
/* Global tail row of every halo slot of the last sharded level (host array: first tail row of the owner rank + the owner's local
 * row).  The replicated tail's solution holds the neighbours' entries too: the kernel that hands this rank its own slice then fills
 * the level's halo slots from it, and the post pass of the level above needs no halo exchange for e_c.  n = 0 switches it off. */
int mgs_hier_set_native_tail_halo(mgs_hier *h, const int *halo_global, int n);
int mgs_hier_native_halo(mgs_hier *h, int level, void *x_dev);
int mgs_hier_native_send_segments(const mgs_hier *h, int level, int *nseg_per_peer, int *seglens, int cap);
int mgs_hier_set_native_recv_segments(mgs_hier *h, int level, const int *nseg_per_peer, const int *seglens);
/* ---- peer-to-peer transport behind the same mgs_comm handle (no reference counterpart) ----
 * The neighbours store their halo values straight into this rank's memory (IPC-mapped device window, xGMI), one kernel per exchange,
 * sequence-numbered flag words for ordering — no RCCL kernel, no host round trip; captured in the cycle's hipGraph like any kernel.
 * Every rank calls mgs_comm_p2p_create (slot_doubles = the most doubles one peer ever sends it in one exchange, all-gather of the tail
 * included; world <= 8) and gets MGS_P2P_HANDLE_BYTES bytes describing its window; the host side ships those records to all ranks
 * (rank order) and every rank calls mgs_comm_p2p_connect.  From then on the communicator serves mgs_hier_set_native_exchange /
 * _tail / mgs_ctx_set_native_allreduce exactly like an RCCL one.  mgs_comm_p2p_info: out[0] memory kind of the window (1 uncached,
 * 2 fine-grained, 3 coarse-grained), [1] window bytes, [2] slot doubles, [3] exchange kernels launched, [4] error word (0 = none;
 * 1 + k: the wait for the k-th participating peer of some exchange timed out, MGS_P2P_TIMEOUT_S), [5] connected. */
#define MGS_P2P_HANDLE_BYTES 96
int mgs_comm_p2p_create(mgs_ctx *ctx, int world, int rank, size_t slot_doubles, void *handle_out, mgs_comm **out);
int mgs_comm_p2p_connect(mgs_comm *c, const void *handles);
int mgs_comm_p2p_info(const mgs_comm *c, long long out[6]);
/* COLLECTIVE self-test of a connected peer-to-peer communicator: `rounds` exchanges with every peer (sizes from the window slot down to a few
 * doubles, both slots reused many times), every value a function of (round, sender, receiver, position) and verified on the device.
 * *mismatches = wrong values this rank saw (0 = clean).  The launcher runs it before it trusts the transport on hardware it has not seen. */
int mgs_comm_p2p_selftest(mgs_comm *c, int rounds, long long *mismatches);
/* raw operations of a communicator (either transport) on the context's stream — transport tests and microbenchmarks; the cycle uses
 * them internally.  exchange: one group of sends (send_dev[q] != NULL) and receives (recv_dev[q] != NULL) of count[q] doubles with
 * rank peer[q]; the ops addressed to one peer are matched with that peer's ops in posting order.  allgather: count doubles per rank,
 * rank-major into recv_dev.  allreduce: in-place sum of count doubles (p2p: count <= 64, summed in rank order). */
int mgs_comm_exchange_raw(mgs_comm *c, int nops, const int *peer, const size_t *count, const void *const *send_dev, void *const *recv_dev);
int mgs_comm_allgather_raw(mgs_comm *c, const void *send_dev, void *recv_dev, size_t count);
int mgs_comm_allreduce_raw(mgs_comm *c, void *buf_dev, size_t count);
/* inner products of the Krylov solvers summed over the ranks with ncclAllReduce on the context's stream (NULL: off;
 * takes precedence over the mgs_ctx_set_allreduce callback) */
int mgs_ctx_set_native_allreduce(mgs_ctx *ctx, mgs_comm *c);

/* Builds the pattern code of A's column array (one byte per row + a small table per 256-row block) so the
 * SpMV-shaped kernels stream 8 instead of 12 bytes per entry wherever rows repeat their shape (stencil-like
 * operators); results stay bit-identical.  Hierarchies and the Krylov solvers call it for their operators; call
 * it yourself before timing a bare mgs_spmv.  No reference counterpart (device-side layout choice).
 * info: out[0] coded row blocks, out[1] row blocks, out[2] table ints, out[3] LDS table budget (ints). */
int mgs_csr_optimize(mgs_csr *A);
/* which form of the fused passes level `level` runs (filled in by the first cycle): out[0] row blocks, out[1]/out[2]
 * setup-time operands present (scaled values / aggregate-mapped columns), out[3..5] coded row blocks of the column
 * array, of its halo-tagged copy (row shards) and of the aggregate-mapped array. */
int mgs_hier_fused_info(const mgs_hier *h, int level, int64_t out[6]);
int mgs_csr_rowcode_info(const mgs_csr *A, int64_t out[4]);
/* grouped pre pass of level `level` (filled in by the first cycle; option "fuse_restrict", default 1): out[0] row-block groups (0: the
 * level runs the separate pre pass + restriction kernels), out[1] groups made of two row blocks, out[2] stray aggregates (restricted by
 * the trailing kernel), out[3] row blocks. */
int mgs_hier_group_info(const mgs_hier *h, int level, int64_t out[4]);
/* The grouped pre pass of level `level` alone, into the caller's vectors (tests and diagnostics; unsharded levels that mgs_hier_group_info
 * reports as grouped): t = b + r and rc = Pᵀr with r = b − Â·b, Â = A·diag(ωD⁻¹); r receives the residual of the rows whose aggregate
 * leaves its row-block group (other entries are not written).  *nodiag (may be NULL): 1 if the pass ran on the operand without Â's
 * diagonal entries (option "pre_nodiag": coded row blocks stream val_nd and a byte per row; the result has the same bits either way).  Enqueued on the context's stream. */
int mgs_hier_pre_pass(mgs_hier *h, int level, const mgs_vec *b, mgs_vec *t, mgs_vec *r, mgs_vec *rc, int *nodiag);
/* The fused pre pass of level `level` alone, whichever arm the level's own cycle runs under the options as they stand, into the caller's
 * vectors (tests and diagnostics), with a report from the launcher.  With Â_ik = fl(a_ik·fl(ω·fl(1/a_kk))): s_i = Σ_k Â_ik·b_k over row i in
 * stored order (summed from 0, one rounding per product and per sum; an FP32 level reads float(Â_ik), widened before the product; the gather
 * form multiplies a_ik·fl(wd_k·b_k) instead), r_i = fl(b_i − s_i), t_i = fl(b_i + r_i), rc[a] = Σ r over the aggregate's members in ascending
 * row order, summed from 0.  The grouped arm writes t and rc, and r only on the rows of the 64-row waves that hold a member of a stray
 * aggregate; the other three arms write r on every row and rc, and leave t untouched.
 * info: [0] arm (0 gather form on A with wd + restriction kernel, 1 residual kernel on Â + restriction kernel, 2 aggregate-parallel kernel,
 * 3 grouped kernel), [1] kernel (0 gather kernel, 1 pattern-coded kernel FP64, 2 the same on FP32 values, 4 slice kernel, 5 aggregate-parallel
 * kernel, 6 grouped kernel sweeping its row blocks one after the other, 7 the 512-thread pair kernel of option "group_concurrent"), [2] gather
 * width U, [3] the kernel's flags word (coded kernels: bit 0 no row is longer than U; slice and grouped kernel: bit 0 streaming stores; bit 1
 * option "stage_unroll"; bit 2 option "rowptr_scan"; 0 for the gather, the pair and the aggregate-parallel kernel), [4] / [5] LDS budget of a
 * row block in values / ints, [6] what the launched instantiation has: bit 0 FP32 values, bit 1 the operand without diagonal entries (option
 * "pre_nodiag"), bit 2 the packed form (option "pack7"; which row blocks are packed: mgs_hier_pack_info) — the pair kernel has neither of the
 * last two, [7] row blocks that are coded and staged, [8] row blocks staged (coded, or with their index slice), [9] row blocks that walk their
 * rows from global memory ([7..9] from the block bounds, the pattern tables' bounds and [4] / [5], the kernels' own conditions; −1 for the
 * aggregate-parallel kernel), [10] stray aggregates of the level (grouped arm; 0 otherwise), [11] row blocks, [12..15] 0.
 * Served and refused as by mgs_hier_post_pass: unsharded levels with a coarser level and an aggregation transfer that run the fused passes.
 * MGS_ERR_INVALID: NULL argument, level out of range, vectors shorter than the level / its aggregates; MGS_ERR_STATE: before
 * mgs_hier_finalize, a general P, a sharded or value-coded level, a level that does not run the fused passes.
 * Enqueued on the context's stream; the host waits for the block bounds behind the launch, the caller synchronizes before reading. */
int mgs_hier_pre_pass_info(mgs_hier *h, int level, const mgs_vec *b, mgs_vec *t, mgs_vec *r, mgs_vec *rc, int64_t info[16]);
/* Packed operand values of level `level` (option "pack7"; filled in by the first cycle): out[0] row blocks of the pre pass's operand, out[1] those of
 * them whose slice is packed (the others read the FP64 array), out[2] which array that copy is of (0 none, 1 Â's values, 2 Â's values without the
 * diagonal entries), out[3] whether the last launch of the level's pre pass ran the packed form of its kernel (1 / 0; −1: no launch yet),
 * out[4] / out[5] / out[6] the same three of the post pass's operand A·P, out[7] bytes of device memory the copies take.  The host waits for the stream. */
int mgs_hier_pack_info(mgs_hier *h, int level, int64_t out[8]);
/* The fused post pass of level `level` alone, into the caller's vectors (tests and diagnostics): the operand, the kernel and the launch are
 * the ones the level's own cycle uses under the options as they stand — merged A·P, aggregate-mapped A (ω/a_ii from the streamed diagonal
 * with option "diag_from_values") or the gather form on A; FP64 or FP32 operand values; option "group_sweep" (whole-level launches of a grouped level).
 *   xin == NULL, the t-form:   bvec holds t = b + r,           x_i = pe_i + d_i·(t_i − s_i)
 *   xin given, the (r, b)-form: bvec holds r and xin holds b,  x_i = (d_i·b_i + pe_i) + d_i·(r_i − s_i)
 * with s_i = Σ_k v_ik·ec[c_ik] over the row of the operand in stored order (summed from 0, one rounding per product and per sum; an entry
 * whose column lies outside every aggregate adds nothing), pe_i = ec[agg_i] (0 for a row outside every aggregate) and d_i = fl(ω·fl(1/a_ii)).
 * Either form may be asked of any eligible level, whichever its own cycle runs.
 * range (may be NULL: the whole level) = {blk_lo, blk_hi, gap_at, gap_len}: the launch covers blk_hi − blk_lo row blocks of 256 rows starting at
 * blk_lo, and those at or behind gap_at are shifted by gap_len — the interior / boundary split of a row shard; INT_MAX, 0: no gap.  Rows of
 * other row blocks are not written.
 * info: [0] operand (0 A through the column-to-aggregate map, 1 aggregate-mapped A, 2 merged A·P), [1] kernel (0 gather kernel, 1 pattern-coded
 * kernel FP64, 2 the same on FP32 values, 3 FP64 swept group by group), [2] gather width U, [3] the kernel's flags word (bit 0: no row is longer than U, one
 * step without a loop; bit 1 option "stage_unroll"; bit 2 option "rowptr_scan"; 0 for the gather kernel), [4] / [5] LDS budget of a row block in values / ints,
 * [6] row blocks of the operand with more entries than [4] (they walk their rows from global memory), [7] 1 if the level's own cycle runs the t-form
 * (grouped pre pass).  [1..5] are −1 / 0 when the range is empty.
 * Served: unsharded levels with a coarser level and an aggregation transfer that run the fused passes (V(1,1), option "fuse").  MGS_ERR_INVALID: NULL
 * argument (xin and range excepted), level out of range, vectors shorter than the level / its aggregates, a range that leaves the level;
 * MGS_ERR_STATE: before mgs_hier_finalize, a general P, a sharded or value-coded level, a level that does not run the fused passes.
 * Enqueued on the context's stream; the host waits for the block bounds behind the launch ([6]), the caller synchronizes before reading x. */
int mgs_hier_post_pass(mgs_hier *h, int level, const mgs_vec *bvec, const mgs_vec *xin, const mgs_vec *ec, mgs_vec *x, const int range[4], int64_t info[8]);
/* hipGraph state of the cycle (diagnostics): out[0] captured cycles cached, out[1] = 1 on the native RCCL transport, out[2] = 1 if
 * capturing the native cycle failed (eager launches since), out[3] eager native cycles run before the first capture.
 * Option "native_graph" (default 1): capture the row-sharded cycle including its RCCL exchanges (two eager cycles first).
 * Option "native_overlap" (default 0): inside that graph, interior row blocks of the big levels on a second stream beside the exchange.
 * Option "graph_split_rows" (default 1048576; 0 = never): with a K-cycle on an unsharded operator of at least this many rows the fine level's two passes are launched
 * eagerly and the levels below replay from ONE graph that does not depend on (b, x): hipGraphLaunch of a K-cycle's hundreds of nodes takes ≈1.1 ms before its first
 * kernel starts, which then hides behind the fine level's pre pass, and a flexible Krylov method's ten direction vectors no longer overrun the (b, x) cache.  Same kernels, same bits. */
int mgs_hier_graph_info(const mgs_hier *h, int64_t out[4]);

/* ---- block vectors: two tall-skinny passes over lists of columns (blockvec.hip) --------------------------------------------------------
 * Nearest reference line: none — the reference works on one vector at a time (bicg.cpp:64-72).  A block is a list of mgs_vec columns; there
 * is no container type, and mgs_spmv, mgs_vcycle and the projections keep working on each column.  n: the leading entries of every column
 * that take part.
 * mgs_vecs_gram: G[a·q + b] = Σ_{i<n} U_a[i]·V_b[i], G on the host, row-major p × q; synchronises.  One streaming pass per tile of at most
 *   8 × 8 entries reads the tile's at most 16 columns once — 16 bytes per lane and stream where every column of the call starts on 16 bytes
 *   (and option "blas1_vec" is on), 8 bytes otherwise, an odd last element on one lane.  Every product and every sum is rounded on its own;
 *   partials lie in a fixed [tile entries][workgroups] layout, no atomics, folded lanes → wave → workgroup → one workgroup per entry: two
 *   identical calls give identical bits (tests/eig_ref.py restates them).  With the same list on both sides (p == q, the same vectors in the
 *   same order) only the tiles on and above the diagonal are computed and mirrored: G is symmetric bit for bit.
 * mgs_vecs_combine: Y_j[i] = Σ_{a<k} C[a·q + j]·S_a[i] for i < n, C on the host, row-major k × q, copied asynchronously into a slot the
 *   context owns (C itself is read before the call returns: the caller may reuse or free it at once); enqueued, no host wait.  Y_j[i] = fl(…fl(fl(C[0][j]·S_0[i]) + fl(C[1][j]·S_1[i])) + …), a ascending.  One pass reads the k
 *   columns and writes the q.  An output may be the same vector as an input (the same start address): every input element of a row is
 *   loaded before any output of that row is stored.
 * mgs_vecs_info: the launch decisions of the last of the two calls on ctx — out[0] workgroups of a pass, out[1] / out[2] the tile's rows /
 *   columns (combine: k / q), out[3] = 1 for the 16-byte path, out[4] passes launched (Gram: tiles), out[5] = 1 when a Gram call took the
 *   symmetric route, out[6] = 1 after a Gram call and 2 after a combine, out[7] = 0.
 * MGS_ERR_INVALID, with a message, nothing launched: a NULL argument or a NULL column; p or q outside 1..MGS_VECS_MAX (combine: k outside
 *   1..MGS_VECS_MAX, q outside 1..16); a column shorter than n or of another context; n < 1; combine: two outputs that overlap or are the
 *   same vector, an output that overlaps an input without being that vector. */
#define MGS_VECS_MAX 24
int mgs_vecs_gram(mgs_ctx *ctx, int64_t n, int p, const mgs_vec *const *U, int q, const mgs_vec *const *V, double *G);
int mgs_vecs_combine(mgs_ctx *ctx, int64_t n, int k, const mgs_vec *const *S, int q, mgs_vec *const *Y, const double *C);
int mgs_vecs_info(const mgs_ctx *ctx, int64_t out[8]);

/* ---- the m smallest eigenpairs of a symmetric operator: LOBPCG with the cycle as preconditioner (eig.hip) -------------------------------
 * Nearest reference line: none — the reference solves linear systems only.  Method: Knyazev, SISC 23 (2001), with soft locking.
 * A is symmetric (the caller's responsibility, as in mgs_pcg).  X: m start vectors on entry, the Ritz vectors on return — orthonormal,
 * ordered by ascending theta.  resid[j] = ‖A·x_j − θ_j·x_j‖₂ / ‖A‖∞, ‖A‖∞ the largest row sum of |a_ij| (computed once on the device); what
 * is returned is formed from a fresh A·X after the last update, never from the recurrences.  *tol in: the bar every resid[j] must stay
 * below; out: the largest resid[j].  *max_iter in: the cap; out: the iterations done.
 * *status: 0 all m residuals below the bar (decided on the true residuals); 1 max_iter reached; 2 the start block is rank deficient — a
 * Cholesky pivot of XᵀX is not greater than 8·m·DBL_EPSILON·max diag (the dense coarse solve's rule with m for n) — 0 iterations, X untouched
 * (with a declared null space the rule is applied to (ΠX)ᵀ(ΠX), formed on copies); 3 the trial basis was still rank deficient by that rule after P was dropped,
 * or a NaN or Inf appeared.
 * One iteration: R_j = A·x_j − θ_j·x_j; columns below the bar are soft-locked (they stay in X, get no W or P column); W_j = M·R_j for the
 * others, W ← W − X·(XᵀW), Cholesky QR on W, and on P on its own (the pivot rule on the Gram matrix of the
 * normalised columns: residual columns differ in length by orders of magnitude, which is no rank deficiency); A·W by SpMV, A·X and A·P carried by the combine that updates X and P;
 * SᵀAS and SᵀS for S = [X W P] through mgs_vecs_gram; the generalised problem of order at most 24 on the host (Cholesky, cyclic Jacobi; no
 * LAPACK); one coefficient matrix gives the new X, P, A·X and A·P.  When SᵀS fails the pivot rule the iteration is redone on [X W].
 * h: NULL (M = I) or a hierarchy that is a fixed symmetric operator, by mgs_pcg's rule with flexible = 0.  The cycle is applied to every
 * column through one fixed (residual, result) pair of work vectors, so it replays from one cached graph whatever m and the iteration count.
 * Work vectors: 5m + 2 from the context's pool.
 * A declared MGS_NULLSPACE_CONSTANT or MGS_NULLSPACE_FIELDS: X ← ΠX first, W_j ← Π(M·R_j) after every preconditioner application (h = NULL
 * included); the m smallest eigenpairs on the complement come back.  The hierarchy must carry the same kind, by mgs_pcg's rule.
 * mgs_eig_info, of the last call on ctx: out[0] iterations, out[1] cycles applied, out[2] SpMVs, out[3] restarts without P, out[4] columns
 * locked at the end, out[5] work vectors taken, out[6] hipGraph captures made during the call, out[7] = 0.
 * MGS_ERR_INVALID, with a message, nothing launched: a NULL argument; m outside 1..MGS_EIG_MAX_BLOCK; rows < 3m + the declared null
 * vectors; a matrix that is not square; a row shard (the criteria of mgs_pcg_plan_create); columns of X that are the same vector, overlap,
 * or are shorter than A's rows; nu1 != nu2 or a K-cycle; a hierarchy whose null-space kind differs from A's.
 * Not served: the largest eigenvalues, row shards, a device-resident Rayleigh–Ritz, null vectors that are not indicators.
 *
 * mgs_eig_lobpcg_gen: the m smallest eigenpairs of A·x = λ·B·x (vibration modes K·x = λ·M·x, the normalised Laplacian L·x = λ·D·x).  The
 * contract is that of mgs_eig_lobpcg with these differences.
 *   A and B are symmetric (the caller's responsibility) and B is positive definite; the pivot rule on XᵀBX and SᵀBS enforces the latter as
 *   far as it is seen: *status 2 also covers a start block whose XᵀBX fails the rule (an indefinite B, for one); 3 is unchanged.
 *   X returns B-orthonormal (XᵀBX = I), theta ascending.
 *   resid[j] = ‖A·x_j − θ_j·B·x_j‖₂ / (‖A‖∞ + |θ_j|·‖B‖∞), formed from a fresh A·X and B·X; both norms from the same row-sum kernel.
 *   One iteration: R_j = AX_j − θ_j·BX_j (mgs_eig_residual); W_j = M·R_j for the active columns; W ← W − X·((BX)ᵀW); BW = B·W by SpMV;
 *   Cholesky QR of W on ½(WᵀBW + its transpose) — the normalised-column pivot rule, the factor applied to W and BW —; AW = A·W; P is
 *   B-orthonormalised on its own from PᵀBP, the factor applied to P, AP and BP; Rayleigh–Ritz with GA = SᵀAS and GB = ½(Sᵀ(BS) + (Sᵀ(BS))ᵀ)
 *   through mgs_vecs_gram on (S, AS) and (S, BS); one coefficient matrix updates X, P, AX, AP, BX and BP in three mgs_vecs_combine calls.
 *   When the rule refuses GB, P is dropped and the iteration is redone on [X W].
 *   Work vectors: 8m + 2 (the staging pair, then AX, BX, W, AW, BW, P, AP, BP); the staging pair and its one cached cycle graph as above.
 *   mgs_eig_info reports the same counters for this call; out[2] counts the SpMVs of A and B together, out[7] those of B alone.
 *   B == NULL: the call is mgs_eig_lobpcg — the same code path, the same bits.
 *   MGS_ERR_INVALID, with a message, nothing launched: everything mgs_eig_lobpcg refuses (rows < 3m), and: B not square, of another size or
 *   of another context than A; B a row shard; a null space declared on A or on B — the complement would have to be B-orthogonal, which is
 *   not served, and the message says so.
 * mgs_eig_residual: r_i = fl(ax_i − fl(θ·bx_i)) for i < n and *nrm2 = Σ fl(r_i·r_i), one pass (three reads, one write; blas1.hip).  The sum
 *   is taken with mgs_dot's launch decisions and folds — 16-byte lanes when ax, bx and r all start on 16 bytes and option "blas1_vec" is on
 *   (an odd last element on one lane), 8-byte grid-stride lanes otherwise — so *nrm2 carries the bits of mgs_dot(r, r), and two identical
 *   calls give identical bits (tests/eig_gen_ref.py restates them).  r may be ax or bx (the same start address).  nrm2 == NULL: the sum is
 *   folded on the device and not fetched; the call does not wait.  MGS_ERR_INVALID, nothing launched: a NULL context or vector, a vector
 *   of another context or shorter than n, n < 1, r overlapping ax or bx without being that vector. */
#define MGS_EIG_MAX_BLOCK 8
int mgs_eig_lobpcg(const mgs_csr *A, mgs_hier *h, int m, mgs_vec *const *X, double *theta, double *resid, int *max_iter, double *tol, int *status);
int mgs_eig_lobpcg_gen(const mgs_csr *A, const mgs_csr *B, mgs_hier *h, int m, mgs_vec *const *X, double *theta, double *resid, int *max_iter, double *tol, int *status);
int mgs_eig_residual(mgs_ctx *ctx, int64_t n, const mgs_vec *ax, const mgs_vec *bx, double theta, mgs_vec *r, double *nrm2);
int mgs_eig_info(const mgs_ctx *ctx, int64_t out[8]);

/* kernel-variant knobs for A/B measurements (initial values of every context: environment MGS_OPTIONS="key=value,...").  key: "spmv_variant", "xcd_remap", "nontemporal",
 * "graph", "strip", "fuse", "nt_store" (smallest operator, in rows, whose row-block kernels store their outputs with the `nt` hint; default 1000000,
 * 0 = never), "stage_unroll" (row-block kernels stage their value slice without a loop in front of the barrier; default 1), "rowptr_scan" (pattern-coded row blocks take a row's
 * entry range from its pattern's length — one rowptr load per wave + a wave prefix sum — instead of two rowptr loads per row; default 1, same bits), "blas1_vec" / "blas1_pairs" (16-byte update
 * kernels, pairs per lane: 1 = one-shot workgroups; defaults 1 / 1), "post_results" (inner products reach the host through a mapped buffer and a polled ticket; default 1), "valcode" (opt-in: pattern tuples carry the values too, set before
 * mgs_csr_optimize / the hierarchy is built; pays only where coefficients repeat), "rowcode" (pattern-coded index, default 1), "split_min_rows" (row shards: smallest level that
 * overlaps its halo exchange with interior row blocks, default 400000), "fuse_operands" (setup-time operands of the fused cycle passes,
 * +12 B of HBM per matrix entry; default 1), "merge_ap" (fused post pass on A·P with the entries of one aggregate summed at setup instead of A with
 * aggregate-mapped columns; default 1; equal to rounding, not bit for bit), "fuse_restrict" / "group_blocks" / "group_stray_pct" / "group_min_blocks" / "group_strip"
 * (grouped pre pass: restriction inside the pre-smoothing pass, see mgs_hier_group_info), "pre_nodiag" (the grouped pre pass of an unsharded FP64 level whose rows
 * hold exactly one diagonal entry streams Â's diagonal entry — ω up to three roundings for every row — as one byte, its distance from ω in units of the last place: 7 B per row less, +8 B of HBM per
 * off-diagonal entry and 1 B per row; default 1, the same bits as with 0), "pack7" (the fused passes of an unsharded FP64 level stream a packed copy of their operands' values, 7 bytes per
 * entry — sign, three exponent bits against a base exponent per row block, 52 mantissa bits — in the coded row blocks whose values span fewer than 8 binades; +7 B of HBM per entry; the same
 * bits as with 0; see mgs_hier_pack_info), "minres_nt" (see mgs_minres; default 0), "diag_from_values", "fuse_dots", "lds_pad", "blkptr".
 * Unknown key: MGS_ERR_INVALID. */
int mgs_ctx_set_option(mgs_ctx *ctx, const char *key, int value);

#ifdef __cplusplus
}
#endif
#endif /* MGS_H */
