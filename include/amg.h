/*
 * amg.h -- C ABI of the MI355X-native faer-amg V-cycle path (libfaer_amg_amd.so).
 *
 * One handle type, amg_linop, stands for the reference's `Arc<dyn LinOp<f64>>`
 * (faer matrix_free::{LinOp, Precond, BiLinOp, BiPrecond}); every constructor
 * returns one.  Handles are reference counted: amg_linop_destroy drops the
 * caller's reference, and operators that hold other operators (a multigrid
 * holding its A/S/R/P) keep their own.  Each entry point below names the
 * reference interface it replaces (paths relative to the reference root).
 *
 * Errors: every function returns amg_status; AMG_OK is 0.  The message of the
 * last failure on the calling thread is amg_last_error().  The reference
 * panics instead; its binding panics on non-zero status.
 *
 * Memory: vectors are column-major n x k blocks with a leading dimension, as
 * faer MatRef/MatMut.  AMG_MEM_DEVICE pointers are read/written
 * asynchronously on the context's HIP stream (synchronise with
 * amg_ctx_synchronize); AMG_MEM_HOST pointers are staged through the device
 * and the call returns after the result is back on the host.
 *
 * Threading: handles are immutable after construction except through the
 * amg_multigrid_add_level / amg_multigrid_set builders; apply calls on one
 * handle must not run concurrently (workspaces are preallocated).
 */
#ifndef FAER_AMG_AMD_AMG_H
#define FAER_AMG_AMD_AMG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum amg_status {
    AMG_OK = 0,
    AMG_ERR_INVALID = 1,     /* bad argument (null handle, negative size, ...) */
    AMG_ERR_DIM = 2,         /* dimension mismatch (the reference's assert_eq! panics) */
    AMG_ERR_UNSUPPORTED = 3, /* valid input the library does not handle (e.g. nnz >= 2^31) */
    AMG_ERR_NOT_SPD = 4,     /* Cholesky factorization failed */
    AMG_ERR_HIP = 5,         /* HIP runtime error / no device */
    AMG_ERR_RCCL = 6,        /* RCCL error */
    AMG_ERR_OOM = 7          /* device allocation failed */
} amg_status;

typedef enum amg_mem { AMG_MEM_HOST = 0, AMG_MEM_DEVICE = 1 } amg_mem;

typedef enum amg_linop_kind {
    AMG_KIND_CSR = 0,       /* sparse matrix (SparseMatOp / ParSpmmOp / SparseRowMat) */
    AMG_KIND_DIAG = 1,      /* Diag<f64> smoother: Jacobi, L1, L2 */
    AMG_KIND_SGS = 2,       /* multicolor symmetric Gauss-Seidel */
    AMG_KIND_COARSE = 3,    /* coarse Cholesky solve */
    AMG_KIND_MULTIGRID = 4, /* Multigrid */
    AMG_KIND_DIST_CSR = 5,  /* row-block distributed sparse matrix */
    AMG_KIND_DIST_MULTIGRID = 6,
    AMG_KIND_COMPOSITE = 7, /* Composite (preconditioners/composite.rs) */
    AMG_KIND_BLOCK = 8,     /* BlockSmoother (preconditioners/block_smoothers.rs) */
    AMG_KIND_CHEBYSHEV = 9  /* Chebyshev polynomial smoother (no reference counterpart) */
} amg_linop_kind;

typedef struct amg_ctx amg_ctx;
typedef struct amg_linop amg_linop;
typedef struct amg_host_csr amg_host_csr; /* host CSR (loaders, generators, strength graphs) */

/* ---- errors, context ------------------------------------------------------ */

/* Thread-local message of the last non-OK status on this thread ("" if none). */
const char *amg_last_error(void);
/* Library version string. */
const char *amg_version(void);

/* Bind device `device` (one process per GPU).  `hip_stream` may be NULL (the
 * library creates its own non-blocking stream) or an existing hipStream_t to
 * order work with the caller's (e.g. torch.cuda.current_stream()). */
amg_status amg_ctx_create(int device, void *hip_stream, amg_ctx **out);
amg_status amg_ctx_destroy(amg_ctx *ctx);
amg_status amg_ctx_synchronize(amg_ctx *ctx);
amg_status amg_ctx_stream(amg_ctx *ctx, void **hip_stream);
/* Order the context stream against another stream (e.g. the caller's
 * torch.cuda.current_stream()): ctx_waits != 0 makes the context stream wait
 * for the work already queued on `other`; ctx_waits == 0 makes `other` wait for
 * the context stream.  Event-based, no host synchronisation. */
amg_status amg_ctx_join_stream(amg_ctx *ctx, void *other, int32_t ctx_waits);
/* SpMV storage policy for matrices built after the call (process-wide):
 * 0 auto -- per matrix the cheapest of: DIA codes (square, <= 32 diagonals or a
 * known run pattern, >= 80 % filled, <= 256 distinct values), 3x3 block storage
 * (block operators), stencil classes (structured Galerkin operators, >= 64
 * offsets; with a grid hint x-staged per grid tile, also for shorter stencils and
 * instead of a > 27-diagonal DIA pattern when that times faster at setup), pattern
 * SELL (structured operators incl. rectangular R/P; the R/P of amg_sa_build_box
 * get the grid-transfer-class overlay, one 8-bit class per row), x-staged
 * SELL (gather-heavy fp64 SELL whose x footprint per 4096 rows fits LDS),
 * SELL-64 with compressed columns and value codes (short regular rows),
 * wave-per-row (rows averaging >= 256 entries), CSR-stream otherwise
 * (DESIGN.md 2); 1 CSR-stream only, 2 SELL-64 whenever rows are <= 256 long,
 * 3 wave-per-row for every matrix.  Results agree to the summation order of the
 * rows (bitwise for rows summed by one lane, which every storage but the
 * long-row CSR-stream / wave-per-row paths does). */
amg_status amg_set_spmv_format(int32_t policy);
/* Value storage of SELL-64 matrices built after the call (process-wide):
 * 1 (default) stores a 4 / 8 / 16-bit code per entry into a per-matrix table of
 * the distinct fp64 bit patterns when the matrix has at most 16 / 256 / 65536 of
 * them (the padding's 0.0 included); 0 always stores fp64 values.  A decoded
 * value is the stored value bit for bit, so results do not change. */
amg_status amg_set_value_codes(int32_t enable);
/* Device allocation policy for buffers allocated after the call: 0 (default)
 * hipMalloc.  1 (physically contiguous buffers >= 16 MiB) is refused with
 * AMG_ERR_UNSUPPORTED: on gfx950 it let kernels read stale data written by the
 * previous kernel on the same stream. */
amg_status amg_set_alloc_policy(int32_t policy);

/* ---- sparse matrices (replaces SparseMatOp::new core.rs:56-74, ParSpmmOp::new
 *      par_spmm.rs:31-96, and the SparseRowMat<usize,f64> LinOp used at
 *      multigrid.rs:137-158) -------------------------------------------------- */

/* Run-time switches (no reference counterpart; measured A/B paths, every
 * setting bitwise neutral).  Each takes its initial value from the environment
 * variable named.  Setting one makes every multigrid re-capture its hipGraph at
 * its next apply.  amg_get_flag reads the current value.
 *   flag 0  FAMG_FOLD_XSCS    fold the zero-guess step on x-staged class levels
 *                             (default 0)
 *   flag 1  FAMG_DIA_DK       read a constant coded Jacobi diagonal as one scalar
 *                             (default 1)
 *   flag 2  FAMG_VEC_WPR      waves per row of the wave-per-row kernel: 0 auto =
 *                             chosen per matrix at finalize (default), 1/2/4
 *   flag 3  FAMG_GTX_TIME     where the wide grid-transfer classes (gtx.hip) are
 *                             kept: 0 wherever they build, 1 where they beat the
 *                             transfer operator's other storage in a setup-time
 *                             timing, 2 (default) on operators of >= 2^18 rows
 *   flag 4  FAMG_SGS27_MARCH  marching 27-point SGS phases (sgs27.hip): 0 = one
 *                             workgroup per tile and plane, 1 = auto (about one
 *                             workgroup per CU, default), n >= 2 = n planes per
 *                             workgroup
 *   flag 5  FAMG_XS_PIPE      x-staged SELL kernel (xsell.hip): 2 = one burst of
 *                             loads per row group with LDS-DMA staging (default),
 *                             1 = software-pipelined batches, 0 = the round-4 kernel
 *   flag 6  FAMG_BSR_KERNEL   3x3-block SpMV kernel (bsr.hip): 0 = the round-2
 *                             kernel (default), 1 = node columns first, 4-step
 *                             batches, 2 = columns first, 2-step batches pipelined,
 *                             3 = 4-step pipelined
 *   flag 7  FAMG_BSR_LONG     3x3-block matrices whose slices (64 node rows)
 *                             average at least this many block steps take the
 *                             long-row kernel that loads the next 8 steps' node
 *                             columns ahead (default 48; -1 never)
 *   flag 8  FAMG_DIA7_RP      row pairs per lane of the constant 7-point DIA
 *                             kernel: 0 auto (default: 2 for SET, 1 for the cycle's
 *                             epilogues), 1, 2 or 4 adjacent 512-row blocks per
 *                             workgroup
 *   flag 9  FAMG_FINE_FUSE    the fine level of a constant 7-point box hierarchy as
 *                             marching fused kernels (fine.hip): 0 = off, 1 = on
 *                             (default), n >= 2 = n planes per workgroup
 *   flag 10 FAMG_DENSE_TAIL   the dense tail of a mu = 1 cycle: the first level
 *                             1 <= l < L - 1 of at most this many rows and every
 *                             coarser one run as one dense GEMV v = M f, M built
 *                             once from the cycle itself (default 4096; 0 = off)
 *   flag 11 FAMG_BLOCK_CYCLE  k > 1 columns through a multigrid or a Composite:
 *                             1 (default) = one block V-cycle on the n x k block
 *                             (k-wide kernels, the matrices read once per 8
 *                             columns, eager launches), 0 = column by column (k
 *                             graph-replayed cycles); the same bits either way
 *   flag 12 FAMG_BLOCK_SMOOTHER_COLS k > 1 columns through a BlockSmoother: 1
 *                             (default) = the k-wide kernel, every block inverse
 *                             read once per group of up to 8 columns, 0 = one
 *                             launch per column; the same bits either way */
amg_status amg_set_flag(int32_t which, int64_t value);
amg_status amg_get_flag(int32_t which, int64_t *value);
/* Stencil-class storage of a CSR operator (structured Galerkin operators whose
 * rows repeat up to a shift; replaces the value/column streams of
 * interpolation/mod.rs:828's A_c in SpMV): info4 = {classes, offsets K (padded
 * to 8), class-id bits, dictionary bytes}; zeros when the operator uses another
 * storage. */
amg_status amg_csr_class_info(const amg_linop *op, int64_t *info4);
/* Grid hint (no reference counterpart: the reference's SparseMatOp has no
 * geometry): the rows of the square operator are the points of an nx x ny x nz
 * grid, x fastest.  Stencil-class operators whose nonzero offsets are grid steps
 * that stay inside the grid then run x-staged per grid tile (scs.hip,
 * bitwise the same sums).  Re-finalizes the SpMV storage: call before the
 * operator is used (graphs captured earlier would read released storage).  The
 * stencil generators and amg_sa_build_box set it for the levels they make;
 * 0,0,0 clears it (and stops the inference below).  A square operator created
 * without a hint (amg_csr_create: the drop-in path, multigrid.rs:190-239 /
 * core.rs:56-74 callers) gets one inferred at finalize from the stencil of 64
 * sample rows (amg_grid_from_offsets); every consumer of the hint (x-staged
 * classes, grid-transfer classes in amg_multigrid_add_level, fused SGS phases)
 * checks every entry against it.  FAMG_INFER_GRID=0 turns the inference off. */
amg_status amg_csr_set_grid(amg_linop *op, int64_t nx, int64_t ny, int64_t nz);
/* The grid inference on its own (host only, no device): grid3 = (nx, ny, nz) of
 * an n-row square operator whose stencil has the k offsets offs (col - row,
 * any order, repeats allowed); *found = 0 when no grid explains them. */
amg_status amg_grid_from_offsets(const int64_t *offs, int64_t k, int64_t n, int64_t *grid3, int32_t *found);
/* The fused SpMV epilogues the V-cycle runs (multigrid.rs:337-369, 407-424),
 * on device vectors, asynchronous on the context stream: mode 0 y = A x, 1
 * y += A x, 2 y = b - A x, 3 y = x + d (b - A x) (weighted Jacobi step; d the
 * scaled inverse diagonal).  x != y. */
amg_status amg_csr_spmv_epilogue(const amg_linop *op, int32_t mode, const double *x, double *y,
                                 const double *b, const double *d);
/* The k-wide counterpart (the block V-cycle's launches): column-major device
 * blocks X (ldx), Y (ldy), B (ldb) of k columns, d one diagonal shared by all
 * columns; modes as above; asynchronous on the context stream.  Every column is
 * bitwise amg_csr_spmv_epilogue of that column.  Storages with an SpMM kernel
 * (DIA codes, stencil classes, 3x3 blocks, pattern SELL, fp64 SELL-64, x-staged
 * SELL) read the matrix once per 8 columns with the epilogue fused at the
 * store; CSR-stream, value-coded SELL-64 and the 8-bit grid-transfer classes
 * have k-wide launches of their single-vector row sums; wave-per-row, the
 * wide grid-transfer classes and x-staged stencil classes with eight lanes per
 * row (amg_csr_row_lanes) run one SpMV per column.  X != Y; k >= 0; AMG_ERR_INVALID for a leading dimension below the
 * rows it spans. */
amg_status amg_csr_spmm_epilogue(const amg_linop *op, int32_t mode, const double *X, int64_t ldx, double *Y,
                                 int64_t ldy, const double *B, int64_t ldb, const double *d, int64_t k);
/* info12 (13 entries) = {nx, ny, nz (0: no hint), x-staged (0/1), tile tx, ty,
 * tz, halo rx, ry, rz, hint source (0 none, 1 given, 2 inferred), grid-transfer
 * classes (0 none, 1 as P, 2 as R: 8-bit gtc.hip; 3 as P, 4 as R: 16-bit
 * gtx.hip), how the x-staged tile was chosen (1 the frozen per-shape table of
 * tuning.cpp, 2 timed at setup, 3 FAMG_XSCS_TILE)}. */
amg_status amg_csr_grid_info(const amg_linop *op, int64_t *info12);
/* Lanes that share one row sum of the x-staged stencil-class kernel: 8 on few
 * long rows (fewer than 131072 rows, at least 256 padded offsets, 16-bit class
 * ids: eight partial chains and a fixed three-step tree per row), else 1 (one
 * sequential chain per row, the CSR order) -- also for every other storage. */
amg_status amg_csr_row_lanes(const amg_linop *op, int64_t *lanes);

/* Copy a host CSR with usize-compatible (int64) row pointers and column indices
 * and fp64 values to the device.  Columns must be sorted ascending within each
 * row and in [0, ncols).  Stored internally with 32-bit indices: returns
 * AMG_ERR_UNSUPPORTED if nrows, ncols or nnz >= 2^31. */
amg_status amg_csr_create(amg_ctx *ctx, int64_t nrows, int64_t ncols, const int64_t *rowptr,
                          const int64_t *colidx, const double *vals, amg_linop **out);
/* Same from device arrays with 32-bit indices (copied). */
amg_status amg_csr_create_device_i32(amg_ctx *ctx, int64_t nrows, int64_t ncols,
                                     const int32_t *rowptr, const int32_t *colidx,
                                     const double *vals, amg_linop **out);
/* Number of stored entries of a CSR operator. */
amg_status amg_csr_nnz(const amg_linop *op, int64_t *nnz);
/* SpMV storage chosen for a CSR operator: info8 = {kernel (0 CSR-stream,
 * 1 SELL-64, 2 vector, 3 DIA codes, 4 3x3 blocks, 5 pattern SELL with lanes per row, 6 stencil
 * classes, 7 x-staged SELL: slices counted as 16-bit when their x is staged in LDS, 32-bit
 * when they escape to global columns), matrix
 * bytes one SpMV streams, CSR bytes (12 nnz +
 * 4 (n+1)), SELL slices, SELL stored entries incl. padding, SELL slices with
 * implicit / 16-bit delta / 32-bit column indices}. */
amg_status amg_csr_spmv_info(const amg_linop *op, int64_t *info8);
/* Value codes of a CSR operator's SpMV storage: info2 = {code bits (0 = fp64
 * values, 4, 8, 16), table entries}. */
amg_status amg_csr_value_codes(const amg_linop *op, int64_t *info2);
/* DIA-code rows of a CSR operator's SpMV storage: info4 = {first row, end row,
 * diagonals, code bits}; all 0 without DIA storage.  The range is the whole
 * matrix (kernel 3 in amg_csr_spmv_info) or one row segment beside SELL / CSR
 * storage (the halo interior of a distributed level). */
amg_status amg_csr_dia_range(const amg_linop *op, int64_t *info4);
/* Copy a CSR operator back to host arrays (rowptr: nrows+1, colidx/vals: nnz). */
amg_status amg_csr_download(const amg_linop *op, int64_t *rowptr, int64_t *colidx, double *vals);
/* Device-side generators for the benchmark operators:
 * 3-D 7-point Laplacian (6 / -1) and 3-D 27-point anisotropic Q1 diffusion on an
 * nx*ny*nz Dirichlet interior grid; row = x + nx*(y + ny*z). */
amg_status amg_gen_laplace3d_7pt(amg_ctx *ctx, int64_t nx, int64_t ny, int64_t nz,
                                 amg_linop **out);
amg_status amg_gen_aniso27(amg_ctx *ctx, int64_t nx, int64_t ny, int64_t nz, double ex,
                           double ey, double ez, amg_linop **out);
/* General (non-stencil) SPD operator of the same size: the 7-point graph with
 * edge weights 0.5 + U[0,1) (splitmix64 of the edge and seed), a_ij = -w_ij,
 * a_ii = sum of the six incident weights (1.0 for a missing, Dirichlet
 * neighbour), rows and columns permuted symmetrically by a seeded bijection:
 * window < 0 none, 0 over all rows, > 0 within consecutive windows of that many
 * rows (locality of a mesh numbering without stencil structure). */
amg_status amg_gen_random_7pt(amg_ctx *ctx, int64_t nx, int64_t ny, int64_t nz, uint64_t seed, int64_t window,
                              amg_linop **out);

/* In-tree stand-in for config C5 (Flan_1565, which cannot be fetched): Q1
 * hexahedral linear elasticity on an ex x ey x ez element box, per-element
 * Young's modulus 10^(contrast (2u - 1)) (u ~ U[0,1) from splitmix64(seed)),
 * Poisson ratio nu, the x = 0 face clamped, free nodes renumbered by a seeded
 * random permutation (permute 0: none, 1: over all nodes, W >= 2: within
 * consecutive windows of W nodes); 3 dofs per node interleaved
 * (block_size 3).  Host CSR (upload with amg_host_csr_upload). */
amg_status amg_gen_elasticity_q1(int64_t ex, int64_t ey, int64_t ez, double contrast, double nu,
                                 uint64_t seed, int32_t permute, amg_host_csr **out);

/* ---- generic LinOp / Precond / BiPrecond (faer matrix_free traits) -------- */

amg_status amg_linop_kind_of(const amg_linop *op, int32_t *kind);
/* LinOp::nrows / ncols */
amg_status amg_linop_dims(const amg_linop *op, int64_t *nrows, int64_t *ncols);
/* LinOp::apply: out = M * rhs, out overwritten (par_spmm.rs:117,151; multigrid.rs:469).
 * out: nrows x k (ld_out), rhs: ncols x k (ld_rhs).  k > 1: a CSR matrix runs one
 * SpMM; a multigrid or a Composite runs one block cycle (flag 11; chunks of 32
 * columns), a Chebyshev smoother its k-wide vector kernels with A read once per 8
 * columns, a BlockSmoother its k-wide kernel with the block inverses read once
 * per 8 columns (flag 12), each column bitwise the k = 1 result; AMG_MEM_HOST
 * blocks are staged whole.  Other kinds apply column by column. */
amg_status amg_linop_apply(amg_linop *op, double *out, int64_t ld_out, const double *rhs,
                           int64_t ld_rhs, int64_t k, amg_mem mem);
/* BiLinOp::transpose_apply.  Supported for the symmetric operators (smoothers,
 * coarse solve, multigrid -- multigrid.rs:487-502) and for CSR matrices. */
amg_status amg_linop_transpose_apply(amg_linop *op, double *out, int64_t ld_out,
                                     const double *rhs, int64_t ld_rhs, int64_t k, amg_mem mem);
/* Precond::apply_in_place: rhs <- M * rhs (coarse_solvers.rs:254; faer Diag). */
amg_status amg_precond_apply_in_place(amg_linop *op, double *rhs, int64_t ld, int64_t k,
                                      amg_mem mem);
/* BiPrecond::transpose_apply_in_place (coarse_solvers.rs:270). */
amg_status amg_precond_transpose_apply_in_place(amg_linop *op, double *rhs, int64_t ld,
                                                int64_t k, amg_mem mem);
/* Drop the caller's reference. */
amg_status amg_linop_destroy(amg_linop *op);

/* ---- smoothers (smoothers.rs:24-86) and coarse solver (coarse_solvers.rs) -- */

/* new_jacobi: d_i = omega / a_ii (smoothers.rs:78-86). */
amg_status amg_jacobi_create(const amg_linop *A, double omega, amg_linop **out);
/* new_l1: d_i = 1 / sum_j |a_ij| (smoothers.rs:63-76). */
amg_status amg_l1_create(const amg_linop *A, amg_linop **out);
/* new_l2 (smoothers.rs:43-61). */
amg_status amg_l2_create(const amg_linop *A, amg_linop **out);
/* Diag from explicit host values (faer Diag<f64>). */
amg_status amg_diag_create(amg_ctx *ctx, int64_t n, const double *d, amg_linop **out);
/* SmootherKind::SymGaussSeidel (smoothers.rs:20,26 -- unimplemented! in the
 * reference; definition in DESIGN.md): multicolor SGS on A e = r from e = 0.
 * colors: host array of nrows colors in [0, ncolors) or NULL for greedy
 * first-fit coloring in row order. */
amg_status amg_sgs_create(const amg_linop *A, const int32_t *colors, amg_linop **out);
/* SGS smoothers built after the call run their sweeps as fused plane-parity
 * phases (sgs27.hip) where that applies -- a 27-point grid operator stored as
 * DIA codes with the parity colouring -- instead of one launch per colour:
 * enable 1 (default) three phases per SGS step, 2 four phases, 0 colour
 * launches (FAMG_SGS_FUSED=0/2 sets the default).  Bitwise the same results. */
amg_status amg_set_sgs_fused(int32_t enable);
/* *fused = 1 if this SGS smoother runs the fused phases. */
amg_status amg_sgs_fused(const amg_linop *op, int32_t *fused);
/* Number of colors of an SGS smoother. */
amg_status amg_sgs_ncolors(const amg_linop *op, int64_t *ncolors);
/* Storage of the color sweeps: info4 = {colors, kernel (as amg_csr_spmv_info:
 * 1 SELL, 3 DIA codes of the color-permuted copy, ...), diagonals, code bits}. */
amg_status amg_sgs_info(const amg_linop *op, int64_t *info4);
/* Chebyshev polynomial smoother (no reference counterpart -- like SGS a new
 * definition).  With D = diag(A), lambda_max an upper bound on the
 * spectrum of D^-1 A and lambda_min = lambda_max / eig_ratio:
 *   theta = (lambda_max + lambda_min) / 2, delta = (lambda_max - lambda_min) / 2,
 *   sigma = theta / delta, rho_0 = 1 / sigma, c2_0 = 1 / theta,
 *   rho_k = 1 / (2 sigma - rho_{k-1}), c1_k = rho_k rho_{k-1}, c2_k = 2 rho_k / delta
 * (host, fp64, these expressions in this order), and z = S b from z = 0 is
 *   d = c2_0 (dinv b), x = d, r = b;
 *   k = 1 .. steps-1:  r = r - A d;  d = c1_k d + c2_k (dinv r);  x = x + d
 * element-wise without contraction: steps - 1 products with A (the RESID SpMV)
 * and one fused vector pass per term.  S is symmetric (PCG stays valid), needs
 * no colouring, and is k-wide: amg_linop_apply with k > 1 runs the same vector
 * kernels over grid (rows, columns) and reads A once per 8 columns, every column
 * bitwise the k = 1 result; inside a multigrid the block V-cycle (flag 11) has
 * nothing per column left on a Chebyshev level.  Single-GPU: the distributed
 * multigrid takes diagonal and SGS smoothers only and refuses this one
 * (amg_dist_multigrid_create, AMG_ERR_UNSUPPORTED).
 * The bound, at creation, on the device: G = max_i sum_j |a_ij| / a_ii (always
 * >= lambda_max(D^-1 A)) and rho_L, the largest Ritz value of eig_iters Lanczos
 * steps on D^-1 A in the D inner product from the start vector
 * q_i = ((i * 2654435761) mod 2^32) / 2^32 - 0.5 (the ABI carries no RNG; the
 * <= 64 x 64 tridiagonal eigenproblem is solved on the host);
 * lambda_max = min(boost * rho_L, G); eig_iters = 0: G alone; cfg.lambda_max > 0:
 * that value, nothing estimated (info reports rho_L = G = 0).
 * AMG_ERR_INVALID: null handle or out, steps < 1, eig_iters outside 0..64,
 * eig_ratio <= 1, boost < 1, lambda_max < 0 (checked before a device is
 * touched); AMG_ERR_DIM: A not square; AMG_ERR_NOT_SPD: a diagonal entry <= 0
 * or missing. */
typedef struct amg_chebyshev_config {
    int64_t steps;      /* m >= 1 (default 2) */
    int64_t eig_iters;  /* Lanczos steps, 0..64; 0 = the row-sum bound G (default 10) */
    double eig_ratio;   /* > 1 (default 20) */
    double boost;       /* >= 1 (default 1.1) */
    double lambda_max;  /* > 0: use this bound, estimate nothing (default 0) */
} amg_chebyshev_config;
amg_status amg_chebyshev_config_default(amg_chebyshev_config *cfg);
/* cfg NULL = the defaults. */
amg_status amg_chebyshev_create(const amg_linop *A, const amg_chebyshev_config *cfg, amg_linop **out);
/* info6 = {lambda_max, lambda_min, steps, lanczos_ritz (0 if not run), row_sum_bound G
 * (0 if not computed), eig_iters run}; AMG_ERR_INVALID on another kind. */
amg_status amg_chebyshev_info(const amg_linop *op, double *info6);
/* CoarseSolverKind::Cholesky (coarse_solvers.rs:21-33, SparseCholeskySolve
 * :172-181): exact coarse solve.  Returns AMG_ERR_NOT_SPD if A is not SPD and
 * AMG_ERR_UNSUPPORTED above 16384 rows (dense factor). */
amg_status amg_coarse_chol_create(const amg_linop *A, amg_linop **out);

/* ---- multigrid (multigrid.rs:171-424) -------------------------------------- */

/* Multigrid::new(op, smoother) (multigrid.rs:190-199): mu = 1, steps = 1. */
amg_status amg_multigrid_create(amg_linop *op, amg_linop *smoother, amg_linop **out);
/* Multigrid::add_level(op, smoother, r, p) (multigrid.rs:228-239).  r: n_c x n_f,
 * p: n_f x n_c where n_f is the previous level's size and n_c = op's size;
 * AMG_ERR_DIM otherwise (hierarchy.rs:258-264 asserts). */
amg_status amg_multigrid_add_level(amg_linop *mg, amg_linop *op, amg_linop *smoother,
                                   amg_linop *r, amg_linop *p);
/* with_cycle_type(mu) / with_smoothing_steps(steps) (multigrid.rs:204-214); both > 0. */
amg_status amg_multigrid_set(amg_linop *mg, int64_t mu, int64_t steps);
amg_status amg_multigrid_levels(const amg_linop *mg, int64_t *levels);
/* Enable/disable hipGraph capture of whole V-cycles (default on). */
amg_status amg_multigrid_set_graph(amg_linop *mg, int32_t enable);
/* Options: 0 = hipGraph capture (as above); 1 = SGS smoothing in the literal
 * residual form of smooth() (multigrid.rs:418-423: r = f - A x; x += SGS(r))
 * instead of the fused in-place sweep on x (default 0: fused, one SpMV fewer);
 * 2 = fold the first Jacobi step from v = 0 (v = d f, s = 1) into the residual
 * and correction SpMVs instead of storing it (default 1; bitwise identical), on
 * levels whose operator is fp64 SELL with mostly short columns, x-staged SELL,
 * or DIA codes whose P runs the short-slice kernel; amg_multigrid_cycle_plan
 * reports which levels fold (RESID0 / ADD0 launches); 3 = fused grid transfers:
 * removed in round 5 (measured slower twice); only 0 is accepted.  4 = a
 * restriction stored as wide grid-transfer classes (gtx.hip) also writes the
 * next level's first Jacobi step from zero, d_c f_c, beside f_c (SPMV_SETDF)
 * instead of a separate pass (default 1; bitwise identical). */
amg_status amg_multigrid_set_option(amg_linop *mg, int32_t option, int64_t value);
/* Multigrid option 5 -- locality reordering (reorder.hip; no reference
 * counterpart): the cycle runs a level of a general operator (no grid storage,
 * a diagonal smoother, >= 65536 rows) in a locality numbering of its node graph
 * (its nodes grouped by aggregate in the renumbered coarse level's order, or
 * reverse Cuthill-McKee, whichever touches fewer x cache lines) -- renumbered
 * copies of A_l, its diagonal, R_l and P_l whose rows keep their stored entry
 * order and their original's kind of storage -- with one gather of rhs and one
 * scatter of the result per apply when the fine level is renumbered.  0 off,
 * 1 (default) where the result stays bitwise (every operator whose rows move
 * sums a row independently of its neighbours) and it at least halves the x
 * cache lines an SpMV slice of 64 rows touches, 2 every eligible level (equal
 * to rounding).  amg_multigrid_get_level returns the caller's operators,
 * amg_multigrid_get_run_level the ones the cycle runs (the renumbered copies of
 * a renumbered level); *reordered = 1 when level runs renumbered. */
amg_status amg_multigrid_level_reordered(amg_linop *mg, int64_t level, int32_t *reordered);
amg_status amg_multigrid_get_run_level(amg_linop *mg, int64_t level, amg_linop **A, amg_linop **S,
                                       amg_linop **R, amg_linop **P);
/* Multigrid::apply == amg_linop_apply on a multigrid handle (k > 1: the block
 * V-cycle, flag 11). */
amg_status amg_multigrid_apply(amg_linop *mg, double *out, int64_t ld_out, const double *rhs,
                               int64_t ld_rhs, int64_t k, amg_mem mem);

/* Launch plan of one V-cycle: the kernels the library launches for one
 * amg_multigrid_apply, in launch order, each with the algorithmic bytes of
 * that launch (the bytes its storage streams + the vectors it reads and
 * writes) and the same launch priced with 32-bit CSR matrix bytes
 * (SURVEY.md 8(d)).  Recorded by running one eager (non-graph) cycle on
 * scratch vectors with the recorder on, so fold decisions, SGS colour launches
 * and storage choices are the ones the cycle makes.  recs may be NULL (count
 * only); at most cap records are written, *count = records of the cycle. */
typedef enum amg_role {
    AMG_ROLE_SMOOTH = 0,   /* pre/post smoothing (smooth, multigrid.rs:407-424) */
    AMG_ROLE_RESID = 1,    /* r = f - A v (:341-342), incl. a folded zero-guess step */
    AMG_ROLE_RESTRICT = 2, /* f_c = R r (:343) */
    AMG_ROLE_INTERP = 3,   /* v += P v_c (:349-350), incl. a folded d*f */
    AMG_ROLE_COARSE = 4,   /* coarsest solve (:291) */
    AMG_ROLE_OTHER = 5
} amg_role;
typedef struct amg_launch_rec {
    int32_t level, role, kernel, mode; /* kernel as amg_csr_spmv_info (-1: vector op); mode: SET 0,
                                          ADD 1, RESID 2, JACOBI 3, SGS 4, RESID0 5, ADD0 6,
                                          SETDF 7 = SET + d*y (-1) */
    int64_t rows;                      /* rows this launch updates */
    int64_t bytes;                     /* algorithmic bytes */
    int64_t csr_bytes;                 /* with 12 nnz + 4 (m+1) matrix bytes (= bytes for vector ops) */
    char name[32];                     /* storage kernel ("dia", "sell_short", "dia_sgs", "vec_mul" ...) */
} amg_launch_rec;
amg_status amg_multigrid_cycle_plan(amg_linop *mg, amg_launch_rec *recs, int64_t cap, int64_t *count);
/* The launches of one block V-cycle of k >= 1 columns (what amg_multigrid_apply
 * runs for k > 1 with flag 11 on), recorded the same way on scratch blocks.  A
 * k-wide SpMM launch ("spmm_dia", "spmm_scs", "spmm_bsr3", "spmm_sellp",
 * "spmm_sell", "spmm_xsell", "spmm_stream", "spmm_gtc") covers up to 8 columns: bytes = its matrix bytes
 * once + its vector bytes per column; storages without an SpMM kernel show one
 * single-vector record per column.  A BlockSmoother level shows "block_cols"
 * (flag 12): one record per chunk size class and group of up to 8 columns, bytes =
 * the class's inverses and index once + its vector bytes per column. */
amg_status amg_multigrid_block_plan(amg_linop *mg, int64_t k, amg_launch_rec *recs, int64_t cap, int64_t *count);
/* One of the fine level's fused launches (no reference counterpart: the fused
 * forms of multigrid.rs:341-343 and 349-369 on a constant 7-point box
 * hierarchy, fine.hip), exactly as amg_multigrid_apply makes it, on the cycle's
 * own workspace, asynchronous on the context stream: which 0 = the folded
 * residual + restriction (rhs in; level 1's f and first Jacobi step written),
 * 1 = interpolation + post-smoothing (rhs and level 1's v in; out written).
 * Device pointers, n = the fine level's rows.  AMG_ERR_UNSUPPORTED where the
 * cycle does not take that launch.  For timing the cycle's dominant kernels
 * on their own (bench.py roofline). */
amg_status amg_multigrid_fine_launch(amg_linop *mg, int32_t which, double *out, const double *rhs);
/* In-cycle timing of one fused fine-level launch (no reference counterpart:
 * measurement): which 0 / 1 as amg_multigrid_fine_launch, -1 off.  While on,
 * every cycle records a pair of HIP events around that launch on the context
 * stream (the cycle then runs its launches eagerly, not as its hipGraph: HIP
 * cannot time events recorded by graph nodes); *ms = the time between the pair
 * of the last completed cycle.  Setting it drops the captured graphs. */
amg_status amg_multigrid_set_fine_timer(amg_linop *mg, int32_t which);
amg_status amg_multigrid_fine_timer_ms(amg_linop *mg, float *ms);
/* The same for a distributed multigrid: one eager cycle (halo exchanges
 * included: collective, every rank calls it) on this rank's scratch vectors;
 * level = global level index (the redundant tail's levels after the
 * distributed ones), rows = this rank's rows. */
amg_status amg_dist_cycle_plan(amg_linop *dist, amg_launch_rec *recs, int64_t cap, int64_t *count);
/* The first 16 hex digits of sha256 over the library's sources (the .hip,
 * .cpp, .hpp and .inc files of csrc in sorted order, then this header) it was built from: the
 * Python package and __graft_entry__.build() compare it with the tree and
 * refuse / rebuild a stale prebuilt library. */
const char *amg_source_hash(void);
/* Launch the marker kernel k_trace_mark(tag) on the context stream: brackets a
 * region of a rocprofv3 kernel trace (bench.py marks its timed V-cycles, and
 * scripts/prof_summary.py keeps the dispatches between the marks). */
amg_status amg_trace_mark(amg_ctx *ctx, int32_t tag);

/* ---- Galerkin setup kernels (interpolation/mod.rs:716-720, 824-828, 927-946) - */

/* C = A * B (faer sparse x sparse). */
amg_status amg_spgemm(const amg_linop *A, const amg_linop *B, amg_linop **out);
/* R = P^T as a CSR (interpolation/mod.rs:824-827). */
amg_status amg_transpose(const amg_linop *P, amg_linop **out);
/* A_c = R * (A * P) (interpolation/mod.rs:828). */
amg_status amg_galerkin_rap(const amg_linop *R, const amg_linop *A, const amg_linop *P,
                            amg_linop **out);
/* smooth_interpolation: P_s = A P scaled by -(omega/a_ii) per row, plus P
 * (interpolation/mod.rs:927-946). */
amg_status amg_smooth_interpolation(const amg_linop *A, const amg_linop *P, double omega,
                                    amg_linop **out);
/* Tentative SA interpolation for one candidate (interpolation/mod.rs:754-805):
 * agg_of[i] in [0,naggs) (host), near_null (host, n); coarse_nn (host, naggs) out. */
amg_status amg_sa_tentative(amg_ctx *ctx, int64_t n, const int64_t *agg_of, int64_t naggs,
                            const double *near_null, amg_linop **P, double *coarse_nn);
/* Coarse near-null post-processing (hierarchy.rs:219-228): L1 StationaryIteration
 * (`iters` steps, smoothers.rs:146-158) then normalization; x is host, in/out. */
amg_status amg_nn_stationary_l1(const amg_linop *A, int64_t iters, double *x);

/* Smoothed-aggregation hierarchy on a structured nx*ny*nz grid with bx*by*bz box
 * aggregates and one constant candidate (Hierarchy::coarsen, hierarchy.rs:190-248,
 * box aggregates standing in for the modularity partitioner -- DESIGN.md).
 * Coarsens until the coarse size <= coarsest_dim or max_levels (0 = unlimited).
 * smoother: 0 Jacobi(omega), 1 L1, 2 SGS (greedy coloring; L1 on levels needing
 * > 32 colors), 3 BlockSmoother over the level's box aggregates, 4 Chebyshev
 * (amg_chebyshev_create with the default config), on every level but the
 * coarsest, which gets the Cholesky coarse solve.  Returns the multigrid. */
amg_status amg_sa_build_box(amg_linop *A, int64_t nx, int64_t ny, int64_t nz, int64_t bx,
                            int64_t by, int64_t bz, int64_t coarsest_dim, int64_t max_levels,
                            double omega, int32_t smoother, amg_linop **mg_out);
/* ---- smoothed aggregation on general (unstructured, block) matrices -----------
 * Hierarchy::coarsen (hierarchy.rs:190-248) with AggregationConfig /
 * smoothed_aggregation (interpolation/mod.rs:62-156, 730-836): strength graph
 * (partitioners/mod.rs:337-393, block-reduced :294-301), aggregates seeded by
 * maximal_independent_set (:395-423; the default -- amg_set_sa_partitioner(1)
 * runs the reference's modularity partitioner instead), tentative P from a per-aggregate thin SVD of the near-null block,
 * P smoothing by Jacobi (block size 1) or block_jacobi (:963-1028), R = P^T,
 * A_c = R A P, coarse near-null by 3 L1 stationary steps + thin QR; the coarse
 * block size is candidate_dimension. */
typedef struct amg_sa_config {
    int64_t block_size;          /* dofs per node of A (SparseMatOp block_size, core.rs:56) */
    int64_t candidate_dimension; /* candidates kept per aggregate (<= near-null columns) */
    int64_t strength_depth;      /* BFS depth of the strength graph (reference: 3) */
    int64_t smoothing_steps;     /* P smoothing steps (AggregationConfig default 1) */
    int64_t coarsest_dim;        /* stop when the coarse size <= this (default 1000) */
    int64_t max_levels;          /* 0 = unlimited */
    double omega;                /* Jacobi smoother weight (smoother 0) */
    int32_t smoother;            /* 0 Jacobi, 1 L1 (default), 2 SGS, 3 BlockSmoother(aggregates), 4 Chebyshev */
    int32_t chebyshev_steps;     /* smoother 4: steps per application, 0 = the default (2); the former
                                    `reserved` field, same layout */
} amg_sa_config;
amg_status amg_sa_config_default(amg_sa_config *cfg);
/* near_null: n x k column-major (leading dimension ld), host; weights: k host
 * values of the strength inner product or NULL for create_weights
 * (examples/amg/main.rs:571-580: 1 / v^T A v).  Returns the multigrid (smoother
 * per cfg on every level but the coarsest, which gets the Cholesky solve). */
amg_status amg_sa_build(amg_linop *A, const double *near_null, int64_t ld, int64_t k, const double *weights,
                        const amg_sa_config *cfg, amg_linop **mg_out);
/* The pieces (for tests and custom hierarchies): node-level strength graph as a
 * host CSR (values = strengths); MIS-seeded aggregates of such a graph;
 * tentative P for k candidates on nnodes nodes of block_size dofs (coarse_nn:
 * (naggs*cd) x k column-major, leading dimension naggs*cd); block_jacobi P
 * smoothing; coarse near-null post-processing of x (n x k, ld) in place. */
amg_status amg_strength_graph(const amg_linop *A, const double *near_null, int64_t ld, int64_t k,
                              const double *weights, int64_t depth, int64_t block_size, amg_host_csr **out);
amg_status amg_aggregate_mis(const amg_host_csr *graph, int64_t *agg_of, int64_t *naggs);
amg_status amg_sa_tentative_block(amg_ctx *ctx, int64_t nnodes, int64_t block_size, const int64_t *agg_of,
                                  int64_t naggs, const double *near_null, int64_t ld, int64_t k, int64_t cd,
                                  amg_linop **P, double *coarse_nn);
amg_status amg_block_jacobi_smooth(const amg_linop *A, const amg_linop *P, int64_t block_size, double omega,
                                   amg_linop **out);
amg_status amg_nn_postprocess(const amg_linop *A, int64_t iters, double *x, int64_t ld, int64_t k);

/* Where amg_sa_build (on every level) and amg_find_near_null run the strength
 * graph and the aggregation (process-wide, like amg_set_spmv_format): 0 host
 * (default), 1 device (the two functions below; the graph stays on the device
 * between them, only agg_of comes back).  Not one of the numbered flags: those
 * are bitwise neutral and this is not -- the device weighs a kept edge with
 * (t*t)*(t*t) where the host calls pow(t, 4.0) (<= 2 ULP apart; no device code
 * reproduces libm's pow bit for bit), so a device-built hierarchy is an equally
 * valid SA hierarchy but not bit-identical to a host-built one.  The policy holds
 * at every strength_depth >= 1: at depth > 1 the candidates of a dof row are its
 * BFS ball, built on the device (amg_pattern_ball_device).  A level keeps the host
 * path when a candidate list has more than 4096 members (reason 2), when the ball
 * pattern and the dof graph (4 B per ball entry, 8 B per row pointer, 12 B per kept
 * entry) exceed half the free device memory (reason 3), or when the ball or the
 * kept entries reach 2^31 (reason 4); amg_sa_level_info reports which.  With the
 * policy at 0 nothing changes anywhere.  AMG_ERR_INVALID for another value.
 * FAMG_SA_LOG=1 makes amg_sa_build print per-level, per-stage wall times, the
 * longest ball and the reason to stderr under either policy. */
amg_status amg_set_sa_setup(int32_t where);
amg_status amg_get_sa_setup(int32_t *where);
/* amg_strength_graph at depth 1 on the device (new_ls_strength_graph,
 * partitioners/mod.rs:337-393, block-reduced :294-301, :464-497): near_null is
 * n x k column-major (ld), host or device by `mem`; weights: k host values.  The
 * node-level graph comes back as a CSR handle on the device (values =
 * strengths) without SpMV storage: read it with amg_csr_download, pass it to
 * amg_aggregate_mis_device.  Every step gives the host's bits except the weight
 * (t*t)*(t*t) (above).  A wave ranks a dof row of <= 256 off-diagonal entries, a
 * workgroup one of <= 4096; AMG_ERR_UNSUPPORTED beyond. */
amg_status amg_strength_graph_device(const amg_linop *A, const double *near_null, int64_t ld, int64_t k,
                                     const double *weights, int64_t block_size, amg_mem mem,
                                     amg_linop **graph);
/* The BFS ball of every row of the square CSR pattern of A: row i of *ball lists
 * extract_local_subgraph(pattern, i, depth) (partitioners/mod.rs:695-718) without
 * i itself, columns ascending, following stored entries only (an asymmetric
 * pattern, a row without a diagonal; a row storing only its diagonal has an
 * empty ball).  A device CSR handle with unit values and no SpMV storage: read
 * it with amg_csr_download.  A wave builds a ball of <= 256 members (a hash
 * table and the member list in LDS), a workgroup one of <= 4096.
 * AMG_ERR_INVALID: depth < 1 or a null argument (nothing touched);
 * AMG_ERR_DIM: A not square; AMG_ERR_UNSUPPORTED: a ball of more than 4096
 * members (never truncated) or 2^31 or more entries. */
amg_status amg_pattern_ball_device(const amg_linop *A, int64_t depth, amg_linop **ball);
/* amg_strength_graph_device at any depth >= 1 (amg_strength_graph_device is depth
 * 1).  Depth 1: exactly that function.  Depth >= 2: the candidates of a dof row
 * are its ball (above) where depth 1 takes the row's off-diagonal entries; the
 * ranking, merging and scaling are the same kernels, so the result equals the
 * host's amg_strength_graph(depth) as depth 1 does.  The ball is freed before the
 * node-level merge allocates.  max_bytes bounds the ball pattern plus the dof
 * graph (4 B per ball entry, 8 B per row pointer, 12 B per kept entry); 0 = half
 * the free device memory after the ball is counted.  info6 (may be NULL; written
 * whenever the counts were taken) = {longest ball, rows on the wave ball kernel,
 * rows on the workgroup ball kernel, ball entries, kept dof entries, node edges};
 * at depth 1 no ball is built: the first three describe the ranking kernels (the
 * longest row only where it passes 256) and ball entries is 0.
 * AMG_ERR_INVALID: null graph, depth < 1 or max_bytes < 0 (nothing touched), null
 * A / near_null / weights; AMG_ERR_UNSUPPORTED, the message naming the cause: a
 * ball of more than 4096 members, the byte budget, 2^31 or more ball or kept
 * entries. */
amg_status amg_strength_graph_device_depth(const amg_linop *A, const double *near_null, int64_t ld, int64_t k,
                                           const double *weights, int64_t depth, int64_t block_size,
                                           amg_mem mem, int64_t max_bytes, amg_linop **graph, int64_t *info6);
/* The record amg_sa_build kept of coarsening step `level` (0 = from the finest
 * operator) in the multigrid it returned: out8 = {n, block size, nodes,
 * aggregates, strength edges, strength graph and aggregation ran on the device
 * (0/1), why they stayed on the host, longest ball}.  Reasons: 0 none (they ran on
 * the device), 1 the policy (amg_set_sa_setup(0)), 2 a candidate list beyond 4096,
 * 3 the byte budget, 4 the index range.  The longest ball is what the device
 * counted before it decided: 0 under policy 0, a lower bound past the cap, at
 * depth 1 the longest row only where it passes 256.  AMG_ERR_INVALID: null out8,
 * a multigrid without such a record (built another way, or with one level), a
 * level out of range. */
amg_status amg_sa_level_info(const amg_linop *mg, int64_t level, int64_t *out8);
/* The aggregates amg_sa_build recorded for coarsening step `level`: agg_of (host,
 * the step's node count of amg_sa_level_info, may be null) and *naggs (may be null,
 * not both).  AMG_ERR_INVALID as amg_sa_level_info. */
amg_status amg_sa_level_aggregates(const amg_linop *mg, int64_t level, int64_t *agg_of, int64_t *naggs);
/* ---- numeric re-setup: the same sparsity pattern, new values ------------------
 * amg_sa_refresh rebuilds the hierarchy of `mg` -- a multigrid amg_sa_build made;
 * any other one (box, classical, hand-composed, adaptive, distributed):
 * AMG_ERR_UNSUPPORTED -- for A_new, a CSR handle on the same context whose row
 * pointers and column indices equal the build's fine operator (compared on the
 * device; AMG_ERR_INVALID if they differ), and near_null (host, n x k column-major,
 * ld >= n, the build's k: AMG_ERR_INVALID otherwise).  Weights are not taken: they
 * only feed the strength graph.  The result is the hierarchy amg_sa_build would
 * make for A_new had strength and aggregation returned the recorded aggregates:
 * per coarsening step the tentative P of the frozen aggregates and the current
 * near-null space, `smoothing_steps` of P smoothing, R = P^T, A_c = R (A P), the
 * coarse near-null post-processing; then the configured smoothers and the coarsest
 * Cholesky factor.  mu, steps, graph, reorder and every amg_multigrid_set_option
 * value stay as set.
 *   The first refresh of a hierarchy runs the symbolic passes once and records, on
 * the device, the pattern of every A P and D^-1 (A P) intermediate and the
 * transpose permutations (info8[1] bytes, held until the multigrid is destroyed);
 * later refreshes are numeric only.  amg_sa_build itself keeps only its config and
 * the host aggregates.
 *   A refresh that fails at any stage (AMG_ERR_INVALID above, AMG_ERR_NOT_SPD from
 * a diagonal block or the coarsest factor, ...) leaves the multigrid exactly as
 * it was.  On success the next apply rebuilds the renumbered copies, the diagonal
 * codes, the dense tail and every captured graph: no cycle replays a graph
 * captured before the refresh.
 *   Aliasing: the refresh installs new operators.  The multigrid keeps a reference
 * to A_new as its fine operator (destroying the caller's handle is fine; changing
 * its values is not), and handles obtained earlier through amg_multigrid_get_level
 * keep the operators of the hierarchy they were taken from -- they do not see the
 * new values; ask again after the refresh.
 *   info8 (may be null) = {1 if this call recorded the patterns, 0 if it reused
 * them; device bytes of the record; levels; coarsening steps; 0, 0, 0, 0}. */
amg_status amg_sa_refresh(amg_linop *mg, amg_linop *A_new, const double *near_null, int64_t ld, int64_t k,
                          int64_t *info8);
/* The two kernels of a later refresh on their own.
 * amg_spgemm_refill overwrites C's values with A * B on C's given pattern (every
 * row's columns ascending, as amg_spgemm returns them): amg_spgemm's values bit
 * for bit, 0.0 in entries of C outside the product.  AMG_ERR_INVALID if a column of
 * the product is missing from C (reported through a device flag; C's values are
 * then undefined and nothing outside them is written) or C is A or B; AMG_ERR_DIM
 * for mismatched shapes.
 * amg_transpose_perm: perm (host, nnz entries) such that entry q of R = P^T is
 * entry perm[q] of P, for an R with the pattern amg_transpose(P) gives
 * (AMG_ERR_INVALID for another pattern, AMG_ERR_DIM for another shape).
 * amg_transpose_refill: R.val[q] = P.val[perm[q]] (AMG_ERR_INVALID for an entry of
 * perm outside [0, nnz)).  Both refills rebuild the SpMV storage of what they wrote. */
amg_status amg_spgemm_refill(const amg_linop *A, const amg_linop *B, amg_linop *C);
amg_status amg_transpose_perm(const amg_linop *P, const amg_linop *R, int32_t *perm);
amg_status amg_transpose_refill(const amg_linop *P, amg_linop *R, const int32_t *perm);
/* amg_aggregate_mis (maximal_independent_set, partitioners/mod.rs:395-423) of a
 * square CSR handle -- a result of amg_strength_graph_device or a graph uploaded
 * with amg_csr_create: exactly the host's agg_of (host, n entries) and *naggs.
 * With u preceding v when its strength degree is larger (ties: the smaller
 * index) and H(v) the nodes preceding v whose rows list v, v is claimed once some
 * u in H(v) is a root and a root once every u in H(v) is claimed; bounded passes
 * over the undecided nodes decide this in place, the host reading the undecided
 * count every 4 passes (AMG_ERR_INVALID if it stopped falling).  Past max_passes
 * (0: the default budget, 1024) -- a chain-like graph needs n/2 -- the graph is
 * downloaded and the host sweep runs: the same result.  The tail (singleton roots
 * join their strongest neighbour's aggregate, numbering by smallest node) is the
 * host's own, on the singleton roots' rows only.  info4 (may be NULL) = {passes
 * run, roots, singleton roots, fell back to the host (0/1)}. */
amg_status amg_aggregate_mis_device(const amg_linop *graph, int64_t max_passes, int64_t *agg_of,
                                    int64_t *naggs, int64_t *info4);

/* The modularity partitioner (partitioners/modularity.rs; PartitionerConfig,
 * partitioners/mod.rs:249-329): aggregates of about coarsening_factor nodes of a
 * node-level strength graph (square CSR, ascending columns, no self loops, not
 * necessarily symmetric).  Partitioner::new without a starting partition and
 * with unit node weights (:28-134), initialize_partition by pairwise matching
 * rounds (greedy_matching :339-383 on generate_modularity_triplets :305-337,
 * merged by pairwise_merge, mod.rs:109-126, :439-462, :508-578) while
 * nnodes / naggs < coarsening_factor, then improve_partition (:437-510).  The
 * orders the reference leaves to unstable sorts and HashSet iteration are pinned
 * (DESIGN.md 17): candidate edges by weight descending, then by the splitmix64
 * finaliser of (i << 32 | j), i, j; merged vertices numbered by ascending
 * smallest member; equal columns of a merged row summed in member-then-stored
 * order; a swap's destination ties to the smaller aggregate, proposals tie to the
 * smaller node.  powf(2.0) and powf(4.) are products.  Aggregates come back
 * numbered by their smallest node.  AMG_ERR_INVALID for coarsening_factor < 1, a
 * negative penalty or budget, a non-square graph, a non-finite strength or
 * strengths that sum to zero (the reference panics there). */
typedef struct amg_partitioner_config {
    double coarsening_factor;        /* 8.0 */
    double agg_size_penalty;         /* 1.0 */
    int64_t max_improvement_iters;   /* 100 */
    int64_t max_passes;              /* device passes per matching round, 0 = default (256) */
} amg_partitioner_config;
amg_status amg_partitioner_config_default(amg_partitioner_config *cfg);
/* agg_of: n host entries.  info8 (may be NULL) = {matching rounds, device passes
 * summed, most device passes in one round, fell back to the host (0/1),
 * improvement passes that proposed a swap, swaps accepted, smallest aggregate,
 * largest aggregate}. */
amg_status amg_partition_modularity(const amg_host_csr *graph, const amg_partitioner_config *cfg,
                                    int64_t *agg_of, int64_t *naggs, int64_t *info8);
/* The same aggregates, integer for integer, of a square CSR handle (a result of
 * amg_strength_graph_device or a graph uploaded with amg_csr_create).  A
 * matching round runs as locally dominant passes: every live vertex picks its
 * first live incident edge in the pinned order, an edge picked at both ends is
 * matched -- the serial sweep's matching (its stop after T + 1 pairs is a cut at
 * the (T + 1)-th matched key).  Two launches per pass; the host reads the count
 * of vertices that still picked an edge every 4 passes (AMG_ERR_INVALID if it
 * stopped falling).  Past max_passes in one round the current graph is
 * downloaded and the host finishes: the same result.  Contraction (scan of
 * leader flags, merged rows sorted and summed per row) and the swap proposals
 * (a lane per node, a wave per node above 64 entries) run on the device; the
 * serial selection is the host's, on the downloaded proposals.  A graph with a
 * row of more than 4096 entries goes to the host partitioner (fell back = 1). */
amg_status amg_partition_modularity_device(const amg_linop *graph, const amg_partitioner_config *cfg,
                                           int64_t *agg_of, int64_t *naggs, int64_t *info8);
/* Which partitioner amg_sa_build (on every level), amg_find_near_null and through
 * them amg_adaptive_build run on the strength graph (process-wide, like
 * amg_set_sa_setup; amg_sa_config has no slot left): 0 the MIS aggregates
 * (default: nothing changes anywhere), 1 the modularity partitioner with *cfg
 * (NULL: the defaults) -- on the device where amg_set_sa_setup(1) holds and the
 * level runs there, else on the host.  FAMG_SA_LOG lines then carry its rounds
 * and passes.  AMG_ERR_INVALID for another kind or a bad cfg (nothing changes). */
amg_status amg_set_sa_partitioner(int32_t kind, const amg_partitioner_config *cfg);
amg_status amg_get_sa_partitioner(int32_t *kind, amg_partitioner_config *cfg);

/* ---- classical coarsening: the least-squares interpolation search --------------
 * InterpolationConfig::Classical (interpolation/mod.rs:56-60): least_squares
 * (:539-728) picks C-points by compatible relaxation and gives every other row
 * the weights of a small constrained least-squares search over subsets of the
 * C-points near it.  Scalar matrices only (the reference's "TODO: handle
 * fine_mat.block_size?", :553).  The pieces below; DESIGN.md 18 has what is and
 * is not built.  amg_classical_config carries the reference's defaults
 * (LeastSquaresConfig, CompatibleRelaxationConfig) and the hierarchy fields of
 * amg_sa_config. */
typedef struct amg_classical_config {
    int64_t search_depth;       /* strength graph / MIS depth; reference 3, default here 1 (a depth-3 row has ~1000 dofs in 3-D) */
    int64_t depth_ls;           /* 2: candidates come from BFS depth depth_ls + search_depth */
    int64_t max_interp;         /* 3 (<= 4) */
    double tau_threshold;       /* 1.2 */
    double target_convergence;  /* 0.3 */
    int64_t relax_steps;        /* 5 */
    double smoother_coarsening_factor; /* 256: CR's BlockSmoother partition */
    int64_t max_cr_iters;       /* 20: guard, no reference counterpart */
    int64_t coarsest_dim;       /* 1000, as amg_sa_config */
    int64_t max_levels;         /* 0 = unlimited */
    double omega;               /* 0.66 */
    int32_t smoother;           /* 1 (L1), as amg_sa_config */
    int32_t chebyshev_steps;    /* 0 */
    int32_t where;              /* the search: 0 host, 1 device (default) */
    int32_t reserved;
} amg_classical_config;
amg_status amg_classical_config_default(amg_classical_config *cfg);
/* maximal_independent_set with a candidate mask (partitioners/mod.rs:395-423):
 * candidates = n bytes (non-zero: a candidate; the reference's f_points).  The
 * degree of a candidate is the sum, in stored order from 0.0, of its row's
 * weights to neighbours that are candidates; the sweep runs by descending degree,
 * ties to the smaller index (the pin of the reference's unstable sort); a chosen
 * node clears itself and every node its row lists.  c_points: room for n entries,
 * filled with the *n_new chosen nodes in the order chosen.  The mask is not
 * changed.  AMG_ERR_DIM for a non-square graph. */
amg_status amg_cr_mis(const amg_host_csr *graph, const uint8_t *candidates, int64_t *c_points, int64_t *n_new);
/* The compatible-relaxation C/F split (least_squares, interpolation/mod.rs:574-652)
 * of A with the strength graph `graph` (amg_strength_graph at cfg->search_depth;
 * square, ascending columns, no self loops).  Every round: the points labelled F
 * are the candidates of amg_cr_mis and the chosen ones become C; u_0 = the vector
 * of ones (not the near-null) times I_f (1 on F and N points, 0 on C points);
 * A_f = I_f A I_f with the C diagonals set to 1; relax_steps error-propagation
 * steps u <- u - M_f (A_f u) with M_f the BlockSmoother of A_f over the modularity
 * partition of `graph` at smoother_coarsening_factor (rebuilt every round);
 * reduction = (|u_end|_2 / |u_start|_2)^(1 / relax_steps), tol = 1 - reduction;
 * sigma_i = |u_i| / |u|_inf > tol labels i F, otherwise an F point becomes N.  The
 * loop ends when reduction <= target_convergence.  The reference builds a second
 * strength graph at depth 3 for the partition (partitioners/mod.rs:289-292); here
 * `graph` serves both, which is the same at the reference's search_depth = 3.
 * The relaxations run on the device, the relabelling on the host.  Guards the
 * reference lacks: a round whose MIS adds no C-point ends the loop, so does
 * max_cr_iters, a relaxed vector of zeros (or no F point left) counts as
 * reduction 0, and a C-point stays a C-point when the reduction is above 1.
 * point_type: n host entries, 0 F, 1 C, 2 N; c_round (may be NULL): n entries, the
 * round (from 0) that made a node a C-point, else -1; *n_coarse the C count; info
 * (may be NULL): 3 + max_cr_iters doubles = {rounds run, last reduction, stop
 * reason (1 converged, 2 no new C-point, 3 max_cr_iters, 4 zero vector), the C
 * count after each round (0 past the last)}. */
amg_status amg_cr_split(amg_linop *A, const amg_host_csr *graph, const amg_classical_config *cfg, int8_t *point_type,
                        int32_t *c_round, int64_t *n_coarse, double *info);
/* Hierarchy::coarsen (hierarchy.rs:190-248) for InterpolationConfig::Classical:
 * per level the strength graph at search_depth (host), amg_cr_split,
 * amg_ls_interpolation, R = P^T and A_c = R (A P) by the device SpGEMMs, and the
 * coarse near-null through amg_nn_postprocess (3 L1 steps, thin QR); the fine
 * weights (NULL: create_weights, 1 / v^T A v) are used on every level.  Coarsening
 * stops at coarsest_dim or max_levels, or when a level does not shrink.  Returns
 * an ordinary multigrid: cfg->smoother on every level but the coarsest (0 Jacobi,
 * 1 L1, 2 SGS, 4 Chebyshev; 3 has no aggregates here: AMG_ERR_UNSUPPORTED), the
 * Cholesky coarse solve on the last.  FAMG_SA_LOG=1 prints a line per level with
 * the stage times (graph, CR with its rounds, candidate lists, search, RAP).
 * level_info (may be NULL): 1 + 7 * AMG_CLASSICAL_INFO_LEVELS host entries = {the
 * coarsenings run, then per coarsening (the first AMG_CLASSICAL_INFO_LEVELS): rows,
 * coarse rows, CR rounds, the longest candidate list, rows searched on the device,
 * rows searched on the host (with where 1: lists beyond the kernel's cap -- on the
 * levels below the fine one the Galerkin fill-in makes these the rule, DESIGN.md
 * 18), empty rows of P}. */
#define AMG_CLASSICAL_INFO_LEVELS 32
amg_status amg_classical_build(amg_linop *A, const double *near_null, int64_t ld, int64_t k, const double *weights,
                               const amg_classical_config *cfg, amg_linop **mg_out, int64_t *level_info);
/* Candidate lists: for every row i with point_type[i] != 1 the C-points
 * (point_type 1; 0 F, 2 N) of extract_local_subgraph(pattern(A), i, depth)
 * (partitioners/mod.rs:695-718; the centre is in the ball), ascending; the row of
 * a C-point is empty.  A host CSR of n rows with unit values.  The BFS runs on
 * the host over the downloaded pattern. */
amg_status amg_ls_candidates(const amg_linop *A, const int8_t *point_type, int64_t depth, amg_host_csr **lists);
/* ls_interp_weights (interpolation/mod.rs:433-510) without its acceptance rule:
 * for every row i of `lists` (n rows; columns = the candidates, ascending) the
 * best subset of each size r = 1..max_interp -- constrained_subset_qp (:387-431)
 * over combinations(r) in lexicographic order, the first strictly smaller error
 * winning.  near_null: n x k column-major (ld), host; weights: k host values (the
 * diagonal Q).  Slot s = i * max_interp + r - 1: count[s] = r or 0 (no valid
 * subset, or the list is shorter than r), cols[s * max_interp + t] the chosen
 * candidates (matrix columns, ascending; -1 past count), w[...] their weights (0
 * past count), err[s] the weighted squared error (0 where count is 0).
 * where 0: OpenMP on the host (ctx may be NULL).  where 1: the gfx950 kernel, one
 * wave per row, for rows whose list has at most max_list candidates (0: the
 * kernel's cap, 256; values above it are cut to it) -- longer rows run the host
 * function; AMG_ERR_UNSUPPORTED for k > 16.  Host and device share one arithmetic
 * (csrc/ls_pinned.hpp) and return the same bits.  info4 (may be NULL) = {rows
 * searched on the device, rows searched on the host, the longest list, subsets
 * enumerated}.  AMG_ERR_UNSUPPORTED for max_interp > 4, AMG_ERR_INVALID for
 * max_interp < 1, k < 1, ld < n, a list that is not ascending and in range or a
 * non-finite near-null entry or weight. */
amg_status amg_ls_search(amg_ctx *ctx, const amg_host_csr *lists, const double *near_null, int64_t ld, int64_t k,
                         const double *weights, int64_t max_interp, int32_t where, int64_t max_list, int32_t *count,
                         int64_t *cols, double *w, double *err, int64_t *info4);
/* The acceptance rule of ls_interp_weights (:456-509) on amg_ls_search's output,
 * on the host for both search paths (it calls libm pow): accepted starts empty
 * with err = btb = the row's vf Q vf^T; size r replaces it when err_r <
 * pow(accepted err, tau * (r - accepted size)).  A slightly negative accepted
 * error makes pow NaN and nothing larger is accepted, as in the reference.
 * chosen[i] = the accepted size (its slot is chosen[i] - 1) or 0: an empty row. */
amg_status amg_ls_accept(int64_t n, const double *near_null, int64_t ld, int64_t k, const double *weights,
                         int64_t max_interp, double tau, const int32_t *count, const double *err, int32_t *chosen);
/* least_squares' level build after the C/F split (:654-715): P (n x n_coarse) with
 * 1.0 at (c, coarse index of c) for the C-points (coarse indices by ascending
 * fine index) and the accepted weights in the other rows -- a row with no C-point
 * in reach or no valid subset stays empty, as in the reference; coarse_nn
 * (n_coarse x k column-major, ld n_coarse, host) = the near-null rows of the
 * C-points; row_err (n, may be NULL) = the accepted error of each row (btb for an
 * empty row, 0 for a C-point).  Candidates from BFS depth cfg->depth_ls +
 * cfg->search_depth, the search where cfg->where says.  info5 (may be NULL) = {rows
 * searched on the device, rows searched on the host, the longest list, subsets
 * enumerated, empty rows of P}. */
amg_status amg_ls_interpolation(amg_linop *A, const int8_t *point_type, const double *near_null, int64_t ld,
                                int64_t k, const double *weights, const amg_classical_config *cfg, amg_linop **P,
                                double *coarse_nn, double *row_err, int64_t *info5);

/* ---- near-null search (adaptivity.rs:264-390, 434-443) -------------------------
 * From a bare SPD matrix to the candidates amg_sa_build takes, on the device.
 * Blocks are column-major n x k with a leading dimension, 1 <= k <= 64
 * (AMG_ERR_UNSUPPORTED above; AMG_ERR_DIM when n < k; AMG_ERR_INVALID when
 * ld < n).  AMG_MEM_HOST blocks are staged whole through the device.  The C ABI
 * carries no random number generator: the caller supplies the start block (the
 * reference draws it from an unseeded rand::rng()), so results are reproducible,
 * bitwise from call to call. */

/* The thin QR of the search (`x.qr().compute_thin_Q()`, adaptivity.rs:329,349,353):
 * X is overwritten by Q; R (host, k x k column-major, may be NULL) is upper
 * triangular with a strictly positive diagonal.  CholeskyQR2 on the device (Gram
 * matrix on the fp64 matrix cores, k x k Cholesky on the host, X <- X R^-1), with
 * shifted passes when the Cholesky breaks down (kappa(X) beyond ~1e7);
 * AMG_ERR_INVALID when X is rank deficient.  Synchronises the context stream. */
amg_status amg_thin_qr(amg_ctx *ctx, double *X, int64_t ld, int64_t n, int64_t k, double *R, amg_mem mem);
/* smooth_vector (adaptivity.rs:307-390): X <- thinQ(thinQ(X)); `iters` times
 * X <- thinQ(X - pc(A X)) (ErrorPropogator + QR, :351-354); then per column w of X
 * cfs[c] = sqrt(ev^T A ev) / sqrt(w^T A w), ev = w - pc(A w) (:367-382; cfs host,
 * k entries, may be NULL).  A is a CSR operator (A X is one SpMM, the matrix
 * streamed once per 8 columns); pc any preconditioning handle -- a Diag
 * (Jacobi/L1/L2) runs as one fused k-wide update, a multigrid or a Composite as
 * one block cycle (flag 11), a BlockSmoother as its k-wide apply (flag 12),
 * every other kind is applied column by column. */
amg_status amg_smooth_vectors(amg_linop *A, amg_linop *pc, double *X, int64_t ld, int64_t k, int64_t iters,
                              double *cfs, amg_mem mem);
/* create_weights (adaptivity.rs:434-443, examples/amg/main.rs:571-580):
 * w[c] = 1 / (x_c^T A x_c) (w host, k entries); AMG_ERR_NOT_SPD when a quadratic
 * form is <= 0. */
amg_status amg_create_weights(const amg_linop *A, const double *X, int64_t ld, int64_t k, double *w, amg_mem mem);
/* find_near_null (adaptivity.rs:264-305): stage 1 = amg_smooth_vectors with the L1
 * diagonal on a copy of the start block X; weights = amg_create_weights of that
 * basis; a BlockSmoother over amg_aggregate_mis(amg_strength_graph(A, basis,
 * weights, strength_depth, block_size)) (or over the modularity partition under
 * amg_set_sa_partitioner(1), as in amg_sa_build); stage 2 = amg_smooth_vectors with
 * that BlockSmoother from the same start block (the reference draws a fresh random
 * block here).  X returns the stage-2 basis, cfs (host, k, may be NULL) its
 * convergence factors. */
amg_status amg_find_near_null(amg_linop *A, double *X, int64_t ld, int64_t k, int64_t iters, int64_t block_size,
                              int64_t strength_depth, double *cfs, amg_mem mem);

/* AdaptiveConfig::build (adaptivity.rs:55-165): from a bare SPD CSR matrix to the
 * adaptive Composite preconditioner.  dim = coarsening_near_null_dim (32 in the
 * reference; 2 <= dim <= 64 here, AMG_ERR_INVALID below, AMG_ERR_UNSUPPORTED
 * above).  X0: host n x dim column-major start block (ld >= n; the ABI carries
 * no RNG).  Steps:
 *  1. (:56-70) amg_find_near_null on columns 1..dim-1 of a copy of X0 (dim - 1
 *     columns, test_iters, sa.block_size, sa.strength_depth); the constant 1 in
 *     column 0; amg_thin_qr of the n x dim block; amg_create_weights.
 *  2. (:108-115) amg_sa_build -> the first component; Composite(A, first).
 *  3. (:117-162) for m = 1 .. max_components - 1: amg_smooth_vectors(A,
 *     composite, a copy of X0 (all dim columns), test_iters / (2m - 1)) -> a basis
 *     and its convergence factors; amg_sa_build(A, basis, weights = the factors);
 *     push the new component.  The smoothing applies the composite k-wide (the
 *     block cycle, flag 11).
 * cfs_out (host, may be NULL): (max_components - 1) rows of dim factors, row
 * m - 1 from search m.  Deviations from the reference: the same start block for
 * every search (the reference draws a new one each time); MIS aggregates
 * unless amg_set_sa_partitioner(1) selects the modularity partitioner;
 * target_convergence and
 * include_constant_first_near_null have no counterpart (the reference's build
 * reads neither).  sa.candidate_dimension must be <= dim. */
typedef struct amg_adaptive_config {
    amg_sa_config sa;
    int64_t max_components; /* default 5 */
    int64_t test_iters;     /* default 50 */
} amg_adaptive_config;
amg_status amg_adaptive_config_default(amg_adaptive_config *cfg);
amg_status amg_adaptive_build(amg_linop *A, const double *X0, int64_t ld, int64_t dim,
                              const amg_adaptive_config *cfg, double *cfs_out, amg_linop **composite_out);

/* Level accessors of a multigrid: A_l, R_l, P_l (l < levels-1), smoother S_l.
 * Returned handles are new references. */
amg_status amg_multigrid_get_level(const amg_linop *mg, int64_t level, amg_linop **A,
                                   amg_linop **S, amg_linop **R, amg_linop **P);

/* ---- solve drivers (the callers of the hot path) ------- */

/* BlockSmoother (block_smoothers.rs:80-291), BlockSolver(Cholesky) kind:
 * block Jacobi over a partition of the n/block_size nodes (node_partition[i] in
 * 0..naggregates-1); each block is the aggregate's submatrix with the
 * couplings leaving it folded into its diagonal (diagonally_compensate
 * :293-324; block_size > 1: diagonally_compensate_vector :326-400) and is
 * solved exactly (dense LL^T inverse per block, <= 8192 rows per block).
 * AMG_ERR_NOT_SPD if a compensated block is not SPD. */
amg_status amg_block_smoother_create(const amg_linop *A, const int64_t *node_partition,
                                     int64_t naggregates, int64_t block_size, amg_linop **out);
/* BlockSmoother::into_sparse_mat (:122-146): the block-diagonal inverse as CSR. */
amg_status amg_block_smoother_to_csr(const amg_linop *bs, amg_linop **out);
/* Shape of a BlockSmoother's apply (no reference counterpart): out = {blocks,
 * rows of the largest block, chunks (one workgroup each: whole blocks of at most
 * 256 rows together, a larger block alone), bytes of the explicit inverses, and
 * the chunks whose k-wide apply (flag 12) takes 8, 4, 2 and 1 columns per pass
 * over the inverses: 8 up to 1024 rows, then 4 up to 2048, 2 up to 4096, 1}. */
amg_status amg_block_smoother_info(const amg_linop *bs, int64_t out[8]);
/* Composite (preconditioners/composite.rs:11-83) as a LinOp/Precond on A:
 * components c_0..c_{m-1} are applied c_{m-1},...,c_1,c_0,c_1,...,c_{m-1}
 * (2m-1 steps), each step out += c(r); r = rhs - A out, from out = 0 and
 * r = rhs.  Components are any preconditioning handles (apply_in_place). */
amg_status amg_composite_create(const amg_linop *A, amg_linop *const *components,
                                int64_t ncomponents, amg_linop **out);
/* Composite::push */
amg_status amg_composite_push(amg_linop *composite, const amg_linop *component);
amg_status amg_composite_ncomponents(const amg_linop *composite, int64_t *n);
/* Stationary solver of examples/simple_geometric.rs:117-158 on device vectors:
 * loop { r = b - A x; rho = ||r||/||b||; hist[it] = rho; stop if rho < rel_tol or
 * it+1 >= max_iter; x += M r }.  b, x device pointers (n); hist host (max_iter).
 * *iters = number of residual evaluations. */
amg_status amg_stationary_solve(amg_linop *A, amg_linop *M, const double *b, double *x,
                                int64_t max_iter, double rel_tol, double *hist, int64_t *iters);
/* Preconditioned CG (faer conjugate_gradient caller, utils.rs:600): stops when
 * ||r|| <= max(abs_tol, rel_tol ||b||); M may be NULL (identity).
 * *iters = iterations (max_iter+1 if not converged); hist host (max_iter) gets
 * ||r_k||/||b||. */
amg_status amg_pcg_solve(amg_linop *A, amg_linop *M, const double *b, double *x,
                         int64_t max_iter, double rel_tol, double abs_tol, double *hist,
                         int64_t *iters);
/* k right-hand sides through the loop of amg_pcg_solve at once (the n x k
 * `rhs: MatRef` of the reference's solve driver, utils.rs:553-633).  B, X:
 * device, column-major n x k, leading dimensions ldb, ldx >= n; X in/out
 * (initial guess).  Every column runs its own CG recurrence: column c's X,
 * iters[c] and history are bitwise what amg_pcg_solve(A, M, B + c*ldb,
 * X + c*ldx, ...) gives.  This deviates from the reference, whose faer
 * conjugate_gradient couples the columns of an n x k rhs (one k x k system per
 * iteration); independent columns are what keeps each one the single solve, as
 * amg_linop_apply / amg_csr_spmm_epilogue already promise per column
 * (amg_block_cg_solve below is the coupled form).
 * A P and B - A X run as one SpMM per 8 columns when A is a CSR matrix; M
 * through its block apply (a multigrid or a Composite: one block cycle, flag 11;
 * a Diag: one k-wide scale; a BlockSmoother: its k-wide apply, flag 12; other
 * kinds column by column); alpha, beta and r.z
 * stay on the device.  Per iteration the host reads the active columns' r.r in
 * one copy and one stream synchronise (amg_pcg_solve: three per column).  A
 * column that has stopped -- converged, or started at or below its tolerance,
 * which a zero column with a zero guess does -- is frozen: its X is not written
 * again and the SpMM, the preconditioner and the vector kernels run over the
 * remaining columns only.  Chunks of 32 columns, one after another.
 * hist: host, max_iter x k column-major (ld_hist >= max_iter), may be NULL;
 * column c gets min(iters[c], max_iter) entries.  iters: host, k entries, each
 * as amg_pcg_solve's (0: the start residual is within tolerance; max_iter + 1:
 * not converged).  M may be NULL (identity).  k = 0 returns AMG_OK and touches
 * nothing.  AMG_ERR_INVALID: null B, X or iters, k < 0, max_iter < 0, hist with
 * ld_hist < max_iter, B aliasing X (the blocks' extents must not overlap), a
 * null handle, a leading dimension below n; the checks that need no handle come
 * first.  AMG_ERR_DIM as amg_pcg_solve.  AMG_ERR_UNSUPPORTED: a distributed
 * operator or preconditioner -- the distributed multigrid has no block cycle;
 * call amg_dist_pcg_solve per column. */
amg_status amg_pcg_solve_block(amg_linop *A, amg_linop *M, const double *B, int64_t ldb,
                               double *X, int64_t ldx, int64_t k, int64_t max_iter,
                               double rel_tol, double abs_tol, double *hist, int64_t ld_hist,
                               int64_t *iters);
/* The same for amg_stationary_solve (M required, max_iter > 0): per sweep
 * R = B - A X over the active columns, their norms to the host in one copy,
 * Z = M R as a block, X += Z.  Column c's X, iters[c] and history are bitwise
 * amg_stationary_solve's; a column stops below rel_tol or at max_iter. */
amg_status amg_stationary_solve_block(amg_linop *A, amg_linop *M, const double *B, int64_t ldb,
                                      double *X, int64_t ldx, int64_t k, int64_t max_iter,
                                      double rel_tol, double *hist, int64_t ld_hist,
                                      int64_t *iters);

/* ---- coupled block CG (utils.rs:553-633 with an n x k rhs) ----------------------
 * What faer's conjugate_gradient does with an n x k right-hand side, which
 * amg_pcg_solve_block deliberately does not: the columns are coupled, one k x k
 * system for the step and one for the new directions per iteration, and all k
 * solutions are searched in the sum of the k Krylov spaces, so the block needs
 * fewer iterations than its slowest column alone.  faer is not part of the
 * reference tree; the definition is this one.  Blocks are n x k
 * column-major device memory, 1 <= k <= 32; small matrices live on the host in
 * fp64; tol_c = max(abs_tol, rel_tol ||B_c||).
 *
 *   R = B - A X;  if every ||R_c|| <= tol_c: iters = 0, return
 *   Z = M R (M NULL: Z = R);  P = Z
 *   for it = 1 .. max_iter:
 *       Q = A P
 *       G = P^T Q,  S = P^T R                      (k x k each, one pass over P, Q, R)
 *       alpha = G^+ S;  ranks[it-1] = r            (the rank-revealing solve below)
 *       X += P alpha;  R -= Q alpha;  ||R_c|| for every c
 *       hist[it-1, c] = ||R_c|| / ||B_c||          (||B_c|| = 0: ||R_c||)
 *       if every ||R_c|| <= tol_c: iters = it, return
 *       if r = 0: break                            (no direction left: not converged)
 *       Z = M R;  T = Q^T Z;  beta = G^+ T;  P = Z - P beta
 *   iters = max_iter + 1
 *
 * G^+ Y, on the host, the factor of an iteration reused for beta:
 *   1. G <- (G + G^T) / 2;
 *   2. a column j with g_jj <= 0 is dropped (a zero or converged direction, a
 *      non-SPD A or M);
 *   3. the rest is scaled to unit diagonal, C = D^-1/2 G D^-1/2;
 *   4. Cholesky of C with diagonal pivoting -- the largest remaining diagonal
 *      first, ties to the lower index -- stopped at the first pivot <= rank_tol;
 *   5. the r pivoted columns are kept: G^+ Y solves with their factor, the rows
 *      of the dropped columns are zero.
 * rank_tol defaults to 2^-26 = sqrt(eps): a pivot is the squared A-norm distance
 * of a unit direction from the span of those already taken, and kappa(C) <=
 * 1/sqrt(eps) keeps alpha, hence the A-conjugacy of the next block, accurate to
 * about sqrt(eps).  The unit diagonal keeps a right-hand side of norm 1e-9
 * beside one of norm 1 from being taken for a dependent one.  Dropping a
 * direction never makes the answer wrong: X and R move by the same alpha, so
 * R = B - A X holds to rounding whatever r is.
 *
 * Q = A P and B - A X run as one SpMM per 8 columns when A is a CSR matrix; M
 * through its block apply (a multigrid or a Composite: one block cycle; a Diag:
 * one k-wide scale).  At most three host synchronisations per iteration for all
 * columns together: (G, S) down and alpha up, the norms, T down and beta up
 * (amg_pcg_solve: three per column).  Unlike amg_pcg_solve_block, a column is not
 * bitwise its single solve, and no column is frozen: every X_c keeps moving until
 * the whole block is within tolerance.  Two calls give equal bits.
 *
 * rank_tol <= 0: the default 2^-26; >= 1: AMG_ERR_INVALID.
 * hist: host, max_iter x k (ld_hist >= max_iter), may be NULL.
 * ranks: host, max_iter entries, may be NULL.
 * *iters: one count for the block (0: start within tolerance; max_iter + 1: not converged).
 * The checks that need no handle come first and touch no device: null B, X or
 * iters, k < 0, k > 32 (AMG_ERR_UNSUPPORTED), max_iter < 0, hist with ld_hist <
 * max_iter, rank_tol >= 1 or NaN, B aliasing X.  Then the null handle, a
 * distributed A or M (AMG_ERR_UNSUPPORTED), AMG_ERR_DIM, the leading dimensions
 * below n and overlapping extents, as amg_pcg_solve_block.  k = 0 returns AMG_OK
 * and touches nothing. */
amg_status amg_block_cg_solve(amg_linop *A, amg_linop *M, const double *B, int64_t ldb, double *X, int64_t ldx,
                              int64_t k, int64_t max_iter, double rel_tol, double abs_tol, double rank_tol,
                              double *hist, int64_t ld_hist, int64_t *ranks, int64_t *iters);
/* The two tall-skinny kernels of the block CG on their own (device blocks, odd
 * leading dimensions allowed; 1 <= w, m1, m <= 32, 0 <= m2 <= 32, AMG_ERR_UNSUPPORTED
 * above; both synchronise the context stream).
 * C (host, w x (m1 + m2) column-major) = X^T [Y1 | Y2]; device blocks; Y2 may be NULL with m2 = 0.
 * fp64 matrix cores, fixed summation order: two calls give equal bits. */
amg_status amg_block_gram(amg_ctx *ctx, const double *X, int64_t ldx, int64_t w, const double *Y1, int64_t ld1,
                          int64_t m1, const double *Y2, int64_t ld2, int64_t m2, int64_t n, double *C);
/* Y <- Y + sign * X C  (X n x w, C host w x m column-major, Y n x m; sign +1 or -1; X != Y):
 * per entry an fma chain over X's columns from 0, then one addition or subtraction. */
amg_status amg_block_gemm_update(amg_ctx *ctx, double *Y, int64_t ldy, const double *X, int64_t ldx,
                                 const double *C, int64_t w, int64_t m, int64_t n, int32_t sign);

/* ---- multi-GPU (row-block partition + RCCL halo exchange) ------- */

/* The reference has no distributed backend (rayon only).  Here the
 * V-cycle is row-block partitioned: rank p owns a contiguous row range of
 * every level; before each SpMV the ghost entries its rows reference are
 * refreshed by a halo exchange (grouped RCCL send/recv over xGMI); levels with
 * fewer than `agglomerate_rows` rows are gathered (ncclAllGather) and solved
 * redundantly on every rank. */
typedef struct amg_comm amg_comm;
typedef struct amg_loopback_hub amg_loopback_hub;
/* Path of the librccl the library bound to (the one already mapped in the
 * process, e.g. torch's, else $FAMG_RCCL_PATH / librccl.so.1); "" if none loads. */
const char *amg_rccl_library(void);
/* ncclUniqueId size in bytes (128). */
int32_t amg_comm_unique_id_size(void);
/* Fill `id` (amg_comm_unique_id_size() bytes) on rank 0; broadcast it out of band. */
amg_status amg_comm_get_unique_id(void *id);
/* One RCCL communicator per process (one process per GPU). */
amg_status amg_comm_create(amg_ctx *ctx, int32_t nranks, int32_t rank, const void *id,
                           amg_comm **out);
/* In-process transport for validation: `nranks` virtual ranks, each driven by
 * its own host thread with its own context, exchange through device copies. */
amg_status amg_loopback_hub_create(int32_t nranks, amg_loopback_hub **out);
amg_status amg_loopback_hub_destroy(amg_loopback_hub *hub);
amg_status amg_comm_create_loopback(amg_ctx *ctx, amg_loopback_hub *hub, int32_t rank,
                                    amg_comm **out);
amg_status amg_comm_destroy(amg_comm *comm);
amg_status amg_comm_rank(const amg_comm *comm, int32_t *rank, int32_t *nranks);
amg_status amg_comm_barrier(amg_comm *comm);
/* Max / sum over ranks of a host double (reduced on the device). */
amg_status amg_comm_allreduce_max(amg_comm *comm, double *value);
amg_status amg_comm_allreduce_sum(amg_comm *comm, double *value);

/* Distributed multigrid from a global multigrid held by every rank (identical
 * on all ranks, e.g. built redundantly by amg_sa_build_box).  level_splits:
 * nlevels x (nranks+1) row splits (row range of rank p at level l is
 * [s[l*(nranks+1)+p], s[l*(nranks+1)+p+1])).  Levels from the first one with
 * fewer than agglomerate_rows rows down are run redundantly on every rank.
 * Every distributed level must be smoothed by a diagonal (Jacobi/L1/L2) or a
 * multicolor SGS smoother (a Chebyshev level is refused: AMG_ERR_UNSUPPORTED);
 * SGS sweeps the global coloring restricted to the
 * owned rows with one halo exchange before every color (the single-GPU sweep's
 * values on every rank).  apply() maps the rank's owned rows of rhs (n_own) to
 * its owned rows of out.  k > 1 columns run column by column: the distributed
 * multigrid has no block cycle. */
amg_status amg_dist_multigrid_create(amg_comm *comm, const amg_linop *mg_global,
                                     const int64_t *level_splits, int64_t agglomerate_rows,
                                     amg_linop **out);
/* Row range [begin, end) of this rank at the finest level. */
amg_status amg_dist_local_rows(const amg_linop *dist, int64_t *begin, int64_t *end);
/* Per-level plan: info[0..5] = n_owned, n_ghost, n_neighbors, redundant (0/1),
 * halo doubles received per exchange, global rows. */
amg_status amg_dist_level_info(const amg_linop *dist, int64_t level, int64_t *info6);
/* The distributed A_l as a LinOp (owned rows in, owned rows out; halo inside). */
amg_status amg_dist_level_operator(const amg_linop *dist, int64_t level, amg_linop **out);
/* This rank's local CSR of a distributed level (which: 0 A_l, 1 R_l, 2 P_l):
 * owned rows, columns in the level's [owned | ghost] numbering. */
amg_status amg_dist_level_matrix(const amg_linop *dist, int64_t level, int32_t which,
                                 amg_linop **out);
/* Options of a distributed multigrid: 0 = overlap each halo exchange with the
 * interior rows of the SpMV that consumes it (default 1; 0 exchanges first);
 * 1 = replay apply() as a captured hipGraph per (out, rhs) pair (default 0;
 * RCCL communicators only -- the loopback transport always runs eagerly);
 * 2 = multicolor SGS levels exchange, before each colour, only the ghost
 * entries of the colour swept just before it (per-colour halo lists; default
 * 1; 0 refreshes the whole halo before every colour).  The plans of
 * amg_dist_cycle_plan carry the exchanges as records of kernel -2 (bytes this
 * rank sends + receives). */
amg_status amg_dist_set_option(amg_linop *dist, int32_t option, int64_t value);
/* Distributed stationary solve (dots all-reduced over ranks): local vectors. */
amg_status amg_dist_stationary_solve(amg_linop *dist_mg, const double *b, double *x,
                                     int64_t max_iter, double rel_tol, double *hist,
                                     int64_t *iters);
/* Distributed PCG on the finest distributed operator, preconditioned by one
 * distributed V-cycle per iteration (precondition = 0: plain CG): the same loop
 * as amg_pcg_solve with every dot all-reduced over the ranks;
 * b, x local (owned rows). */
amg_status amg_dist_pcg_solve(amg_linop *dist_mg, int32_t precondition, const double *b, double *x,
                              int64_t max_iter, double rel_tol, double abs_tol, double *hist,
                              int64_t *iters);

/* ---- host-side distributed planning (no device; faer-amg_amd/csrc/plan.hpp) --
 * The planner amg_dist_multigrid_create runs per level, exported so it can be
 * driven (and tested) from any process layout: rank p owns rows
 * [splits[p], splits[p+1]); add the global column ids of every local matrix
 * that reads the level's vector (A_l, R_l rows and P_{l-1} rows owned here);
 * amg_halo_plan_requests finalises the ghost set (sorted global ids, grouped by
 * owner) and returns how many ids go to each rank; after the ranks have
 * exchanged their request lists, amg_halo_plan_set_incoming builds the send
 * lists (in_ids: the ids every rank requested from this one, concatenated in
 * rank order) and the neighbour table.  amg_halo_plan_remap renumbers a local
 * matrix's columns into [owned | ghost] and returns the interior row segment
 * [lo, hi) (the longest run of rows reading owned entries only). */
typedef struct amg_halo_plan amg_halo_plan;
amg_status amg_halo_plan_create(int32_t nranks, int32_t rank, const int64_t *splits, amg_halo_plan **out);
amg_status amg_halo_plan_destroy(amg_halo_plan *plan);
amg_status amg_halo_plan_add_columns(amg_halo_plan *plan, int64_t nnz, const int64_t *cols);
/* req_counts: nranks entries (may be NULL); *n_ghost: ghost entries. */
amg_status amg_halo_plan_requests(amg_halo_plan *plan, int64_t *req_counts, int64_t *n_ghost);
amg_status amg_halo_plan_ghost_ids(const amg_halo_plan *plan, int64_t *ids);
amg_status amg_halo_plan_set_incoming(amg_halo_plan *plan, const int64_t *in_counts, const int64_t *in_ids);
/* info6 = {n_own, n_ghost, neighbours, entries sent per refresh, entries received, first owned row} */
amg_status amg_halo_plan_info(const amg_halo_plan *plan, int64_t *info6);
/* Per neighbour (rank order): send offset/count into the send list, receive
 * offset/count into the ghost region.  Arrays of `neighbours` entries (any may be NULL). */
amg_status amg_halo_plan_neighbors(const amg_halo_plan *plan, int32_t *nbr, int64_t *soff, int64_t *scnt,
                                   int64_t *roff, int64_t *rcnt);
/* The owned local indices packed for the neighbours (entries sent per refresh). */
amg_status amg_halo_plan_send_indices(const amg_halo_plan *plan, int32_t *idx);
amg_status amg_halo_plan_remap(const amg_halo_plan *plan, int64_t nrows, const int64_t *rowptr, const int64_t *cols,
                               int32_t *local_cols, int64_t *lo, int64_t *hi);
/* The first level cycled redundantly (agglomerated): the first l < nlevels-1
 * with level_rows[l] < agglomerate_rows, else the coarsest. */
amg_status amg_dist_first_redundant_level(int64_t nlevels, const int64_t *level_rows, int64_t agglomerate_rows,
                                          int64_t *level);

/* ---- Dataset loaders (utils.rs:269-534) -------------------
 * Host-side; no device needed.  Matrix Market: sparse coordinate files
 * (real/integer/pattern, general/symmetric), 1-based indices, explicit 0.0
 * entries dropped, symmetric entries mirrored, duplicates summed, columns
 * sorted (load_matrix_triplets, utils.rs:508-534, + faer try_new_from_triplets). */
amg_status amg_mtx_read(const char *path, amg_host_csr **out);
/* Host CSR from arrays (copied; values kept as given, zeros included). */
amg_status amg_host_csr_create(int64_t nrows, int64_t ncols, const int64_t *rowptr, const int64_t *colidx,
                               const double *vals, amg_host_csr **out);
amg_status amg_host_csr_dims(const amg_host_csr *h, int64_t *nrows, int64_t *ncols, int64_t *nnz);
amg_status amg_host_csr_arrays(const amg_host_csr *h, int64_t *rowptr, int64_t *colidx, double *vals);
/* Upload to the device (amg_csr_create). */
amg_status amg_host_csr_upload(amg_ctx *ctx, const amg_host_csr *h, amg_linop **out);
amg_status amg_host_csr_destroy(amg_host_csr *h);

/* MFEM linear system dir/name.{mtx,bdy,coords,rhs} (load_mfem_linear_system,
 * utils.rs:269-350); delete_boundary removes the .bdy rows/columns and
 * renumbers the rest in order (utils.rs:446-480).  The VTK mesh geometry the
 * reference also attaches (visualisation only) is not loaded. */
typedef struct amg_mfem_system amg_mfem_system;
amg_status amg_mfem_load(const char *dir, const char *name, int32_t delete_boundary,
                         amg_mfem_system **out);
/* info5 = {n (after deletion), rhs columns, coordinate dimension, original n,
 * boundary indices (sorted, unique)} */
amg_status amg_mfem_info(const amg_mfem_system *sys, int64_t *info5);
/* The system matrix (borrowed; valid while sys lives). */
amg_status amg_mfem_matrix(const amg_mfem_system *sys, const amg_host_csr **out);
/* rhs (n x k) and coords (n x d), column-major with leading dimension ld. */
amg_status amg_mfem_rhs(const amg_mfem_system *sys, double *out, int64_t ld);
amg_status amg_mfem_coords(const amg_mfem_system *sys, double *out, int64_t ld);
amg_status amg_mfem_boundary(const amg_mfem_system *sys, int64_t *out);
/* solution_to_mesh (n entries), mesh_to_solution (original n entries, -1 =
 * deleted); either may be NULL. */
amg_status amg_mfem_index_maps(const amg_mfem_system *sys, int64_t *solution_to_mesh,
                               int64_t *mesh_to_solution);
amg_status amg_mfem_destroy(amg_mfem_system *sys);

#ifdef __cplusplus
}
#endif
#endif
