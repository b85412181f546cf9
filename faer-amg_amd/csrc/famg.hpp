// famg.hpp -- host-side object model of the MI355X AMG library.
//
// The classes mirror the reference's operator surface (faer matrix_free
// LinOp / Precond / BiPrecond as used by aujxn/faer-amg):
//   LinOp            <- faer::matrix_free::LinOp<f64>        (trait object)
//   CsrOp            <- SparseMatOp / ParSpmmOp / SparseRowMat (core.rs, par_spmm.rs)
//   DiagOp           <- Diag<f64> from new_jacobi/new_l1/new_l2 (smoothers.rs:43-86)
//   SgsOp            <- SmootherKind::SymGaussSeidel (smoothers.rs:20, unimplemented there)
//   ChebyOp          <- no counterpart: a Chebyshev polynomial smoother
//   CoarseCholOp     <- SparseCholeskySolve (coarse_solvers.rs:164-276)
//   MultigridOp      <- Multigrid (preconditioners/multigrid.rs:171-518)
// All operator data lives in HBM; apply() works on device pointers and is
// asynchronous on the context stream.
#pragma once

#include <memory>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "gpu_csr.hpp"

namespace famg {

// Workgroup b of nb -> the b-th of a contiguous range per XCD (consecutive
// workgroups round-robin over the 8 XCDs, each with its own L2): each XCD then
// walks a contiguous slab of rows and keeps its x window in its L2.
__device__ __forceinline__ int xcd_remap(int b, int nb) {
    const int q = nb >> 3, r = nb & 7;
    const int x = b & 7, idx = b >> 3;
    return x * q + min(x, r) + idx;
}

// q / d for 0 <= q < 2^14 through a float reciprocal r = 1.0f / d: (q + 0.5) / d
// lies at least 0.5 / d from an integer, far beyond the float error, for the
// window and tile extents the staging loops divide by.  fdiv_exact checks every
// q < n on the host before a kernel relies on it (memoised per (n, d) in a
// per-thread table: the eager launch paths of the loopback ranks call it
// without a lock).
__device__ __forceinline__ int fdiv_rcp(int q, float r) { return (int)(((float)q + 0.5f) * r); }
inline bool fdiv_exact(int n, int d, float r) {
    thread_local std::vector<std::pair<int, int>> ok;
    for (const auto &e : ok)
        if (e.first >= n && e.second == d) return true;
    for (int q = 0; q < n; q++)
        if ((int)(((float)q + 0.5f) * r) != q / d) return false;
    ok.push_back({n, d});
    return true;
}

// ------------------------------------------------------------------ CSR data
// (SlabFrame, the storage structs, GpuCsr and SpmvKernel: gpu_csr.hpp)

// Grid dims (nx, ny, nz) of a square operator of n rows whose stencil has the
// offsets offs (col - row over some rows); false if no grid explains them.
bool grid_from_offsets(const std::vector<int64_t> &offs, int64_t n, int64_t *g);
// R and P of a 2x2x2-box level as grid-transfer classes when the fine and coarse
// operators carry grid hints of that relation (Multigrid::add_level)
void attach_box_transfers(const GpuCsr &Af, const GpuCsr &Ac, GpuCsr &R, GpuCsr &P);
// Allocate a CSR with the given shape/nnz (arrays uninitialised).
void csr_alloc(GpuCsr &m, Ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz);
// Device copy of the CSR arrays (rp64/col/val) of src into dst; dst is not
// finalized (call csr_finalize for its SpMV storage).
void csr_clone(const GpuCsr &src, GpuCsr &dst);
// Build rp32 (if nnz < 2^31), the stream schedule, the SELL-64 copy for short
// regular rows, and pick the SpMV kernel; `segments` (row bounds, first 0, last
// nrows) keeps blocks/slices inside segments.  Host pass over the row pointers
// (setup only).  Must be called again after values change in place.
void csr_finalize(GpuCsr &m, const std::vector<int64_t> *segments = nullptr);
// Format policy (process-wide, for matrices finalized afterwards):
// 0 auto, 1 CSR-stream only, 2 SELL whenever rows <= 256, 3 vector (no SELL)
extern int g_spmv_format_policy;
// Value codes for SELL matrices finalized afterwards (1 = when <= 65536
// distinct values, 0 = always fp64 values)
extern int g_value_codes;
// grid-transfer classes (gtc.hip): fg/cg the fine/coarse grids of a 2x2x2-box
// level; the row classes of P (fine rows) or R (coarse rows) as (slot, value)
// lists; gtc_attach builds the overlay storage (true if it applies)
bool gtc_classes(const GpuCsr &M, bool is_r, const int64_t *fg, const int64_t *cg, std::vector<uint8_t> &cls,
                 std::vector<std::vector<std::pair<uint8_t, double>>> &dict);
// which: 1 = R (coarse rows), 0 = P (fine rows), -1 = R if it has fewer rows than columns
bool gtc_attach(GpuCsr &m, const int64_t *fg, const int64_t *cg, int which = -1);
// stencil-class storage for structured operators whose rows repeat up to a
// shift; true if built (scs.hip)
bool build_scs(GpuCsr &m, const std::vector<int64_t> &rp, int64_t other_bytes);
// x-staged SELL for gather-heavy fp64 SELL matrices; true if built (xsell.hip)
bool build_xs(GpuCsr &m, const std::vector<int64_t> &rp);
// pattern SELL (implicit columns from per-slice offset patterns) for structured
// operators; true if built (sellp.hip)
bool build_sellp(GpuCsr &m, const std::vector<int64_t> &rp, int64_t other_bytes);
int csr_value_table(const GpuCsr &m, std::vector<unsigned long long> &tab);
// 3x3 block storage when the matrix is blocked and it streams fewer bytes than
// other_bytes; true if built (bsr.hip)
bool build_bsr(GpuCsr &m, const std::vector<int64_t> &rp, int64_t other_bytes);
void build_sell(GpuCsr &m, const std::vector<int64_t> &rp);
// DIA codes for rows [r0, r1) of m with the vb-bit value table tab; true if built (dia.hip)
bool build_dia(GpuCsr &m, int vb, const std::vector<unsigned long long> &tab, const std::vector<int64_t> &rp,
               int64_t r0, int64_t r1, const int32_t *rowid = nullptr);
// DIA codes of a color-permuted SGS copy (diagonals col - rowid[p]); true if built
bool build_dia_sgs(GpuCsr &m, const int32_t *rowid);
void choose_kernel(GpuCsr &m);
// Host upload from usize-compatible arrays.
void csr_from_host(GpuCsr &m, Ctx *ctx, int64_t nrows, int64_t ncols, const int64_t *rowptr,
                   const int64_t *col, const double *val);
void csr_to_host(const GpuCsr &m, int64_t *rowptr, int64_t *col, double *val);
// Diagonal a_ii per row (device, n); throws if a diagonal entry is missing.
void csr_diagonal(const GpuCsr &m, double *d_out);
void csr_abs_row_sums(const GpuCsr &m, double *d_out);

// ------------------------------------------------------------------ kernels

enum SpmvMode : int {
    SPMV_SET = 0,    // y = A x
    SPMV_ADD = 1,    // y = y + A x
    SPMV_RESID = 2,  // y = b - A x
    SPMV_JACOBI = 3, // y = x + d (b - A x)   (x != y)
    SPMV_SGS = 4,    // e[perm p] = e[perm p] + d_p (b[perm p] - (A e)_p)
    // the zero-guess Jacobi step v = d*b folded into its consumers (never stored):
    SPMV_RESID0 = 5, // y = b - A (d*b)   (x == b; d gathered with x)
    SPMV_ADD0 = 6,   // y = d*b + A x
    // restriction that also takes the next level's first Jacobi step from zero:
    // y = A x, y2 = d*y (wide grid-transfer classes only, gtx.hip)
    SPMV_SETDF = 7
};

struct SpmvEpi {
    const double *b = nullptr;
    const double *d = nullptr;
    const int32_t *perm = nullptr;
    const uint8_t *dc = nullptr;  // JACOBI only: 8-bit codes of d into dt
    const double *dt = nullptr;
    double dk = 0.0;              // d when every entry is this one value (0: not constant)
    double *y2 = nullptr;         // SETDF: the second output d*y
};

// y = epilogue(A x) over all rows (seg < 0) or over row segment `seg`, with the
// kernel chosen for m at finalize (SELL-64 / vector / CSR-stream).
// Y = A X for k columns (column-major, leading dimensions ldx/ldy): SELL
// matrices stream once per 8 columns; bitwise equal to k SpMVs.
void spmm(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k, hipStream_t s);
// the same for DIA-code, stencil-class and 3x3-block storage; false if m has none of them
bool spmm_compressed(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k,
                     hipStream_t s);
void spmv(const GpuCsr &m, const double *x, double *y, SpmvMode mode, const SpmvEpi &epi,
          hipStream_t s, int64_t seg = -1);
// The k-wide SpMV epilogues of the block V-cycle: B column-major with ldb, d one
// diagonal shared by all columns.
struct SpmmEpi {
    const double *b = nullptr;
    int64_t ldb = 0;
    const double *d = nullptr;
};
// Y = A X (SET), Y += A X (ADD), Y = B - A X (RESID), Y = X + d (B - A X) (JACOBI)
// over k columns; every column bitwise spmv(mode) of that column.  Storages with an
// SpMM kernel (DIA codes, stencil classes, 3x3 blocks, pattern SELL, fp64 SELL-64,
// x-staged SELL) read the matrix once per 8 columns with the epilogue fused at the
// store; CSR-stream, value-coded SELL-64 and the 8-bit grid-transfer classes run
// their single-vector row sums over 8 columns per launch; wave-per-row and the
// wide grid-transfer classes run spmv(mode) per column.
void spmm_epi(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k, SpmvMode mode,
              const SpmmEpi &epi, hipStream_t s);
// m's storage has an SpMM kernel (what spmm / spmm_epi launch once per 8 columns)
bool spmm_has_kernel(const GpuCsr &m);
bool spmm_compressed_epi(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k,
                         SpmvMode mode, const SpmmEpi &epi, hipStream_t s);
void spmm_sell_epi(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k, SpmvMode mode,
                   const SpmmEpi &epi, hipStream_t s);
// value-coded SELL-64 (sell.hip) and the 8-bit grid-transfer classes (gtc.hip; SET, and ADD
// for P) over 8 columns per launch: the single-vector kernels' row sums per column
void spmm_sell_coded(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k, SpmvMode mode,
                     const SpmmEpi &epi, hipStream_t s);
void spmm_gtc(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k, SpmvMode mode,
              hipStream_t s);
bool spmm_xs_epi(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k, SpmvMode mode,
                 const SpmmEpi &epi, hipStream_t s);

// What one spmv() call launches, resolved once (spmv_route, spmv.hip): spmv()
// switches on it, the launch plan records it and the format's launcher reads its
// sub-decisions from it -- none of them evaluates a dispatch condition again.
enum SpmvRouteTo : int {
    ROUTE_GTX, ROUTE_GTC, ROUTE_BSR, ROUTE_SCS, ROUTE_XS, ROUTE_SELLP, ROUTE_DIA_SGS, ROUTE_DIA, ROUTE_SELL,
    ROUTE_VECTOR, ROUTE_STREAM
};
struct SpmvRoute {
    SpmvRouteTo to = ROUTE_STREAM;    // the entry point
    int kernel = SPMV_KERNEL_STREAM;  // the SpmvKernel and the name the plan records
    const char *name = "csr-stream";
    int64_t seg = -1, r0 = 0, r1 = 0;  // the segment and its rows [r0, r1)
    int runs = 0;             // DIA: 9 = nine runs of three offsets, -1 = the 7-point pattern, 0 = neither
    int pat = 0;              // DIA: the run-pattern kernel (33, 27), 0 = the generic kernels
    bool cst = false;         // DIA: constant stencil, no codes read
    bool sell_short = false;  // SELL: spmv_sell_short_kernel
    bool dk = false;          // the coded diagonal is one value (epi.dk): d is not read
    bool rc = false;          // RESID0 gathers d as 1-B codes, not 8-B values
};
SpmvRoute spmv_route(const GpuCsr &m, SpmvMode mode, const SpmvEpi &epi, int64_t seg);
// the epilogue takes the one value of a coded diagonal (A/B switch FAMG_DIA_DK=0 /
// amg_set_flag(1, 0): a constant coded diagonal is still read per row)
inline bool epi_dconst(const SpmvEpi &epi) { return epi.dc && epi.dk != 0.0 && flag(FLAG_DIA_DK) != 0; }
// sub-decisions the format files own (dia.hip, sell.hip, scs.hip)
void dia_route(const GpuCsr &m, const SpmvEpi &epi, SpmvRoute &r);
bool sell_takes_short(const GpuCsr &m, SpmvMode mode, int64_t seg);
bool scs_takes_xscs(const GpuCsr &m, int64_t seg);
// lanes that share a row sum of the x-staged class kernel: 8 on few long rows
// (spmv_xscs_split_kernel), else 1 -- also for storages without that kernel
int xscs_row_lanes(const GpuCsr &m);
void spmv_dia(const GpuCsr &m, const double *x, double *y, SpmvMode mode, const SpmvEpi &epi, hipStream_t s,
              const SpmvRoute &r);
void spmv_dia_sgs(const GpuCsr &m, const double *x, double *y, const SpmvEpi &epi, hipStream_t s,
                  const SpmvRoute &r);
void spmv_sell(const GpuCsr &m, const double *x, double *y, SpmvMode mode, const SpmvEpi &epi, hipStream_t s,
               const SpmvRoute &r);
void spmm_sell(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k, hipStream_t s);
void spmv_bsr(const GpuCsr &m, const double *x, double *y, SpmvMode mode, const SpmvEpi &epi, hipStream_t s,
              int64_t seg);
void spmv_scs(const GpuCsr &m, const double *x, double *y, SpmvMode mode, const SpmvEpi &epi, hipStream_t s,
              int64_t seg);
bool xs_supports(SpmvMode mode);
// Y = A X over k columns on x-staged SELL (xsell.hip); false for other storages
bool spmm_xs(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k, hipStream_t s);
// the constant 7-point DIA kernel with a one-value Jacobi diagonal takes m's
// JACOBI / RESID0 launches (dia.hip: no codes read, d = epi.dk)
bool dia7_cst_dk(const GpuCsr &m, const SpmvEpi &epi);
// fine.hip: the folded correction v = d f + P v_c and one Jacobi step on a
// constant 7-point fine level as one marching kernel (out = the Jacobi result)
bool fine_interp_jacobi_ok(const GpuCsr &A, const GpuCsr &P, const SpmvEpi &epi);
void fine_interp_jacobi(const GpuCsr &A, const GpuCsr &P, const double *vc, const double *f, double dk, double *out,
                        hipStream_t s);
// the folded residual r = f - A (d f) and f_c = R r, d_c f_c (SETDF) as one marching kernel
// (epic: the coarse level's d and y2 = d_c f_c, as spmv's SETDF epilogue takes them)
bool fine_resid_restrict_ok(const GpuCsr &A, const GpuCsr &R, const SpmvEpi &epi, const SpmvEpi &epic);
void fine_resid_restrict(const GpuCsr &A, const GpuCsr &R, const double *f, double dk, double *fc,
                         const SpmvEpi &epic, hipStream_t s);
bool gtc_supports(const GpuCsr &m, SpmvMode mode);
// wide grid-transfer classes (gtx.hip); which as gtc_attach
bool gtx_attach(GpuCsr &m, const int64_t *fg, const int64_t *cg, int which = -1);
bool gtx_supports(const GpuCsr &m, SpmvMode mode);
int gtx_mode();
void spmv_gtx(const GpuCsr &m, const double *x, double *y, SpmvMode mode, const SpmvEpi &epi, hipStream_t s,
              int64_t seg = -1);
// seg < 0: every tile; a rank-local matrix (rframe on) also takes segments 1
// (interior z-tiles: no ghost reads) and 0 / 2 (the tiles before / after)
void spmv_gtc(const GpuCsr &m, const double *x, double *y, SpmvMode mode, const SpmvEpi &epi, hipStream_t s,
              int64_t seg = -1);
void spmv_xs(const GpuCsr &m, const double *x, double *y, SpmvMode mode, const SpmvEpi &epi, hipStream_t s);
void spmv_sellp(const GpuCsr &m, const double *x, double *y, SpmvMode mode, const SpmvEpi &epi, hipStream_t s,
                int64_t seg);

// BLAS-1 (n-vectors, device pointers)
void vec_fill(double *x, double v, int64_t n, hipStream_t s);
void vec_copy(double *dst, const double *src, int64_t n, hipStream_t s);
void vec_sub(double *out, const double *a, const double *b, int64_t n, hipStream_t s);  // a-b
void vec_add_inplace(double *x, const double *y, int64_t n, hipStream_t s);           // x+=y
void vec_mul(double *out, const double *d, const double *a, int64_t n, hipStream_t s); // d*a
// out = dt[dc] * a (8-bit codes of the diagonal)
void vec_mul_coded(double *out, const uint8_t *dc, const double *dt, const double *a, int64_t n, hipStream_t s);
// 8-bit codes of v (<= 256 distinct values): returns the table size, 0 if none built
// dconst (optional): set to the value when v holds one distinct nonzero value, else 0
int64_t array_codes_u8(const double *v, int64_t n, Ctx &ctx, DevBuf<uint8_t> &code, DevBuf<double> &table,
                       double *dconst = nullptr);
void vec_axpy(double *y, double alpha, const double *x, int64_t n, hipStream_t s);      // y+=a x
void vec_xpay(double *y, double beta, const double *x, int64_t n, hipStream_t s);       // y=x+b y
void vec_scale(double *x, double alpha, int64_t n, hipStream_t s);                      // x*=a
// x = x + d*(x - r)   (StationaryIteration quirk step, smoothers.rs:153-156)
void vec_nn_step(double *x, const double *d, const double *r, int64_t n, hipStream_t s);
// Deterministic dot product; result left on device in *res (fixed reduction tree).
void vec_dot_dev(const double *x, const double *y, int64_t n, double *res, Ctx &ctx);
// the same with the caller's partial sums (VEC_DOT_PARTIALS doubles): callers that share
// a context across threads (loopback ranks) must not share the context's scratch
constexpr int VEC_DOT_PARTIALS = 1024;
void vec_dot_dev(const double *x, const double *y, int64_t n, double *res, double *partials, hipStream_t s);
double vec_dot(const double *x, const double *y, int64_t n, Ctx &ctx);  // syncs

// k-wide vector kernels of the block solve drivers (pcg.hip): column-major blocks,
// one launch over k columns, every column bitwise the single-vector kernel above.
// partials: k * VEC_DOT_PARTIALS doubles, laid out [column][VEC_DOT_PARTIALS].
// partials[c] = the block sums of x_c . y_c (vec_dot's first launch per column)
void cg_dot_cols(const double *x, int64_t ldx, const double *y, int64_t ldy, int64_t n, int64_t k, double *partials,
                 hipStream_t s);
// t_c = vec_dot's second launch on partials[c], then on the device, per column:
// ALPHA a_c = b_c / t_c;  STORE a_c = t_c (b unused);  BETA a_c = t_c / b_c, b_c = t_c
enum CgFinal : int { CG_FINAL_ALPHA = 0, CG_FINAL_STORE = 1, CG_FINAL_BETA = 2 };
void cg_final_cols(CgFinal op, const double *partials, double *a, double *b, int64_t k, hipStream_t s);
// x_c += alpha_c p_c (vec_axpy) on column map[c] of X; r_c += (-alpha_c) Ap_c (vec_axpy);
// partials[c] = the block sums of the new r_c . r_c -- one pass (P, AP, R: leading dimension ldw)
void cg_update_cols(double *X, int64_t ldx, const int32_t *map, const double *P, const double *AP, double *R,
                    int64_t ldw, const double *alpha, int64_t n, int64_t k, double *partials, hipStream_t s);
// p_c = z_c + beta_c p_c (vec_xpay), beta on the device
void cg_xpay_cols(double *P, int64_t ldp, const double *Z, int64_t ldz, const double *beta, int64_t n, int64_t k,
                  hipStream_t s);
// x_c += z_c (vec_add_inplace) on column map[c] of X
void cg_add_cols(double *X, int64_t ldx, const int32_t *map, const double *Z, int64_t ldz, int64_t n, int64_t k,
                 hipStream_t s);

// G (kp2 entries, a multiple of 256) = nblk partial arrays of kp2 entries summed in a
// fixed order (nearnull.hip k_gram_final: the second launch of a Gram product)
void gram_final(const double *partials, int64_t nblk, int kp2, double *G, hipStream_t s);

// tall-skinny kernels of the coupled block CG (bcg.hip): column-major device blocks
constexpr int64_t BCG_MAX_W = 32;  // widest block: the k x k coupling cannot be chunked
// device scratch of the Gram products of one call
struct BcgWork {
    DevBuf<double> partials, G;
    int64_t gram_blocks = 0, rows_per_block = 0;
    void reserve(const Ctx &ctx, int64_t n);
};
// hC (host; pinned for a copy that overlaps) = X^T [Y1 | Y2], w x (m1 + m2) in a
// row-major array of row stride 16 ceil((m1 + m2) / 16) (returned), 16 ceil(w / 16)
// rows, zero past the operands; 1 <= w, m1 <= 32, 0 <= m2 <= 32 (m2 = 0: Y2 unread).
// Two launches and an asynchronous copy: the caller synchronises before reading hC.
int bcg_gram(const double *X, int64_t ldx, int64_t w, const double *Y1, int64_t ld1, int64_t m1, const double *Y2,
             int64_t ld2, int64_t m2, int64_t n, BcgWork &ws, double *hC, hipStream_t s);
// C (w x m column-major) into bcg_gemm's layout: column stride 8 ceil(w / 8), zero filled
void bcg_pack_coef(const double *C, int64_t w, int64_t m, double *packed);
// OUT = Y + sign * X Cd (X n x w, w <= 32; Cd on the device, packed; sign +1 or -1).
// OUT may be Y or X (every lane reads its row of X before it writes).  name: the
// launch-log entry ("bcg_update", "bcg_dir"); byte model 8 n (2 m + w).
void bcg_gemm(const char *name, double *OUT, int64_t ldo, const double *Y, int64_t ldy, const double *X, int64_t ldx,
              const double *Cd, int64_t w, int64_t m, int64_t n, int sign, hipStream_t s);

// marker kernel for rocprofv3 traces (amg_trace_mark)
void trace_mark(Ctx &ctx, int32_t tag);

// dense row-major GEMV: out = M * x (M n x n)
void dense_gemv(const double *M, const double *x, double *out, int64_t n, hipStream_t s);
// Y = M X over k columns (column-major X, Y): M's rows read once per 8 columns,
// every column bitwise dense_gemv
void dense_gemm_cols(const double *M, const double *X, int64_t ldx, double *Y, int64_t ldy, int64_t n, int64_t k,
                     hipStream_t s);
// k-wide element-wise kernels of the block V-cycle (column-major blocks): out = d * a
// (one diagonal for all columns), out = a - b, x += y, dst = src
void vec_mul_cols(double *out, int64_t ldo, const double *d, const double *a, int64_t lda, int64_t n, int64_t k,
                  hipStream_t s);
void vec_sub_cols(double *out, int64_t ldo, const double *a, int64_t lda, const double *b, int64_t ldb, int64_t n,
                  int64_t k, hipStream_t s);
void vec_add_cols(double *x, int64_t ldx, const double *y, int64_t ldy, int64_t n, int64_t k, hipStream_t s);
void vec_copy_cols(double *dst, int64_t ldd, const double *src, int64_t lds, int64_t n, int64_t k, hipStream_t s);
// RCM node order (new -> old) of the node graph of an n x n CSR, bs dofs per node (reorder.hip)
std::vector<int32_t> rcm_order(const std::vector<int64_t> &rp, const std::vector<int32_t> &col, int64_t n, int bs);

// exclusive scan of int64 counts (n entries) into out (n+1 entries); returns total
int64_t scan_counts(const int64_t *counts, int64_t *out, int64_t n, Ctx &ctx);

// sparse products / setup
// C = A B; finalize = false leaves C without SpMV storage (setup intermediates)
void spgemm(const GpuCsr &A, const GpuCsr &B, GpuCsr &C, bool finalize = true);
// S += P where P's pattern lies within S's (values only; S is not re-finalized)
void csr_add_into(GpuCsr &S, const GpuCsr &P);
void transpose(const GpuCsr &A, GpuCsr &T);
void smooth_interp_fixup(GpuCsr &S, const GpuCsr &P, const double *diag, double omega);
void gen_stencil(GpuCsr &m, Ctx *ctx, int64_t nx, int64_t ny, int64_t nz, const int *offs,
                 const double *coef, int nsten);
// random-coefficient 7-pt operator (edge weights 0.5 + U[0,1), Dirichlet
// diagonal), rows/columns permuted symmetrically (window < 0 none, 0 all rows,
// > 0 within consecutive windows of that many rows)
void gen_random_7pt(GpuCsr &m, Ctx *ctx, int64_t nx, int64_t ny, int64_t nz, uint64_t seed, int64_t window);

// ------------------------------------------------------------------ operators

enum class Kind : int {
    Csr = AMG_KIND_CSR,
    Diag = AMG_KIND_DIAG,
    Sgs = AMG_KIND_SGS,
    Coarse = AMG_KIND_COARSE,
    Multigrid = AMG_KIND_MULTIGRID,
    DistCsr = AMG_KIND_DIST_CSR,
    DistMultigrid = AMG_KIND_DIST_MULTIGRID,
    Composite = AMG_KIND_COMPOSITE,
    Block = AMG_KIND_BLOCK,
    Chebyshev = AMG_KIND_CHEBYSHEV
};

struct LinOp : std::enable_shared_from_this<LinOp> {
    Ctx *ctx = nullptr;
    int64_t nrows = 0, ncols = 0;
    virtual ~LinOp() = default;
    virtual Kind kind() const = 0;
    // LinOp::apply -- out = M rhs (device, one column), out overwritten.
    virtual void apply(double *out, const double *rhs) = 0;
    // out = M rhs over k columns (column-major device blocks, leading dimensions
    // ldo / ldr; out != rhs).  Default: apply() column by column.  Every override
    // computes each column bitwise as apply() does.
    virtual void apply_block(double *out, int64_t ldo, const double *rhs, int64_t ldr, int64_t k);
    // BiLinOp::transpose_apply -- symmetric operators reuse apply.
    virtual void transpose_apply(double *out, const double *rhs) { apply(out, rhs); }
    // Precond::apply_in_place -- default: copy to scratch, then apply.
    virtual void apply_in_place(double *rhs);
    virtual bool is_precond() const { return false; }

  protected:
    DevBuf<double> inplace_scratch_;
};
using LinOpPtr = std::shared_ptr<LinOp>;

struct CsrOp : LinOp {
    GpuCsr m;
    DevBuf<double> diag_;  // cached a_ii (lazy)
    std::shared_ptr<CsrOp> transpose_;  // lazy, for transpose_apply
    Kind kind() const override { return Kind::Csr; }
    void apply(double *out, const double *rhs) override;
    void apply_block(double *out, int64_t ldo, const double *rhs, int64_t ldr, int64_t k) override;  // one SpMM
    void transpose_apply(double *out, const double *rhs) override;
    const double *diagonal();
};
using CsrPtr = std::shared_ptr<CsrOp>;

struct DiagOp : LinOp {
    DevBuf<double> d;
    // 8-bit codes of d (built by the multigrid when d has <= 256 distinct
    // values; the V-cycle's Jacobi steps then read 1 B per row instead of 8)
    DevBuf<uint8_t> dcode;
    DevBuf<double> dtab;
    double dconst = 0.0;  // d when it is one value (set with the codes), else 0
    bool codes_tried = false;
    Kind kind() const override { return Kind::Diag; }
    bool is_precond() const override { return true; }
    void apply(double *out, const double *rhs) override;
    void apply_block(double *out, int64_t ldo, const double *rhs, int64_t ldr, int64_t k) override;  // one k-wide scale
    void apply_in_place(double *rhs) override;
};
// the SpMV epilogue of a Jacobi step with D: d with its 8-bit codes (gathered instead
// of d where the kernel reads them) and its one value; b for JACOBI / RESID0 / ADD0,
// y2 for SETDF
inline SpmvEpi jacobi_epi(const DiagOp &D, const double *b = nullptr, double *y2 = nullptr) {
    SpmvEpi e;
    e.b = b;
    e.d = D.d.get();
    e.dc = D.dcode.get();
    e.dt = D.dtab.get();
    e.dk = D.dconst;
    e.y2 = y2;
    return e;
}

struct SgsOp : LinOp {
    CsrPtr A;              // original operator
    GpuCsr Ap;             // rows grouped by color (columns in original numbering)
    DevBuf<int32_t> perm;  // permuted row p -> original row
    DevBuf<double> dinv;   // 1/a_ii at permuted rows
    std::vector<int64_t> color_ptr;   // rows of color c: [color_ptr[c], color_ptr[c+1]) = Ap segment c
    std::vector<int32_t> host_colors;
    int64_t ncolors = 0;
    DevBuf<double> e_;     // scratch correction
    const double *aii_ = nullptr;  // setup only: a_ii of a rectangular slice's rows
    // fused plane-parity sweeps on a 27-point grid operator (sgs27.hip)
    bool fused27 = false;
    bool const27 = false;  // every row the interior stencil truncated at the faces: no codes loaded
    int nx27 = 0, ny27 = 0, nz27 = 0;
    std::vector<uint32_t> icode27;  // interior row's code group (8 words, unused = ~0)
    std::vector<double> icoef27;    // and its 27 coefficients
    std::vector<uint32_t> fmask27;  // 6 x 8 words: code bits of the entries leaving each grid face
    DevBuf<double> fused_tmp, fused_zero;
    Kind kind() const override { return Kind::Sgs; }
    bool is_precond() const override { return true; }
    // e = SGS(r) from e = 0 (device pointers, e != r)
    void sweep(double *e, const double *r);
    // x <- x + SGS(b - A x), in place on x
    void sweep_x(double *x, const double *b);
    // e_i = dinv_i r_i on the rows of color 0 (the first forward color from e = 0)
    void first_color(double *e, const double *r);
    void apply(double *out, const double *rhs) override;
    void apply_in_place(double *rhs) override;
};

// Chebyshev polynomial smoother (cheby.hip): z = S b is `steps` terms
// of the Chebyshev iteration on D^-1 A over [lambda_max / eig_ratio, lambda_max]
// from z = 0 -- steps - 1 products with A (SPMV_RESID) and one fused vector pass
// per term.  Symmetric; k-wide (apply is k = 1 of apply_block's kernels).
struct ChebyConfig {
    int64_t steps = 2;      // m >= 1
    int64_t eig_iters = 10; // Lanczos steps, 0..64; 0 = the row-sum bound G alone
    double eig_ratio = 20.0, boost = 1.1;
    double lambda_max = 0.0;  // > 0: the caller's bound, nothing estimated
};
struct ChebyOp : LinOp {
    CsrPtr A;
    DevBuf<double> dinv;         // 1 / a_ii
    std::vector<double> c1, c2;  // per term (c1[0] unused), computed once on the host
    int64_t steps = 0, eig_run = 0;
    double lambda_max = 0.0, lambda_min = 0.0;
    double ritz = 0.0, row_bound = 0.0;  // the Lanczos Ritz value / G (0: not computed)
    Kind kind() const override { return Kind::Chebyshev; }
    bool is_precond() const override { return true; }
    // launches on ctx->stream only, never allocates, never synchronises (graph capture)
    void apply(double *out, const double *rhs) override;
    // chunks of MG_BLOCK_COLS columns; A read once per 8 columns (spmm_epi)
    void apply_block(double *out, int64_t ldo, const double *rhs, int64_t ldr, int64_t k) override;

  private:
    friend std::shared_ptr<ChebyOp> make_chebyshev(const CsrPtr &A, const ChebyConfig &cfg);
    DevBuf<double> r0_, r1_, d_;     // single-vector workspace, allocated at creation
    DevBuf<double> br0_, br1_, bd_;  // n x kw block workspace (first block apply, grown on demand)
    void run(double *X, int64_t ldx, const double *B, int64_t ldb, int64_t kw, double *R0, double *R1, double *D,
             int64_t ldw, bool single);
};

struct CoarseCholOp : LinOp {
    DevBuf<double> inv;  // dense A^{-1}, row-major (n <= 8192)
    // above 8192 rows (chol.hip): the envelope Cholesky factor of the RCM-ordered
    // matrix in 64-row blocks -- off-diagonal slabs, inverses of the diagonal blocks
    int64_t nb = 0, env_bytes = 0;
    DevBuf<double> slab, mc, mr;
    DevBuf<int64_t> soff;
    DevBuf<int32_t> cmin, perm;
    mutable DevBuf<double> z;
    Kind kind() const override { return Kind::Coarse; }
    bool is_precond() const override { return true; }
    void apply(double *out, const double *rhs) override;
    // the dense inverse as dense_gemm_cols; the envelope factor column by column
    void apply_block(double *out, int64_t ldo, const double *rhs, int64_t ldr, int64_t k) override;
};

struct MgLevel {
    LinOpPtr A, S, R, P;  // R, P: transfer to the next-coarser level (null on the coarsest)
    // locality reordering (reorder.hip): the operators the caller added when A/S/R/P
    // above are renumbered copies; perm = the level's numbering (new -> original)
    LinOpPtr oA, oS, oR, oP;
    DevBuf<int32_t> perm;
    bool permuted = false;
    const LinOpPtr &origA() const { return oA ? oA : A; }
    const LinOpPtr &origS() const { return oS ? oS : S; }
    const LinOpPtr &origR() const { return oR ? oR : R; }
    const LinOpPtr &origP() const { return oP ? oP : P; }
    // device workspaces (allocated lazily at first apply)
    DevBuf<double> v, f, t, r;
    // the block cycle's n x kw workspaces, kw <= MG_BLOCK_COLS the widest block applied so
    // far (leading dimension n; allocated at the first block apply, grown on demand)
    DevBuf<double> bv, bf, bt, br;
};
constexpr int64_t MG_BLOCK_COLS = 32;  // widest block one block cycle takes; wider blocks run in chunks

// hipGraph replay of one cycle per (out, rhs) pair: the 8 most recently captured pairs.
// Whether to replay at all stays with the owner (MultigridOp / DistMultigridOp::apply).
class GraphCache {
  public:
    GraphCache() = default;
    GraphCache(const GraphCache &) = delete;
    GraphCache &operator=(const GraphCache &) = delete;
    ~GraphCache() { clear(); }
    // drop every graph: what they recorded (operators, options, workspaces) changed
    void clear() {
        for (auto &g : graphs_) (void)hipGraphExecDestroy(g.exec);
        graphs_.clear();
    }
    // a run-time switch changed since the last call (the graphs recorded the old
    // launches, so they are dropped)
    bool flags_moved() {
        if (gen_ == flags_generation()) return false;
        clear();
        gen_ = flags_generation();
        return true;
    }
    // replay the graph of (out, rhs) on s; without one, capture what body() issues on
    // s, keep it in place of the oldest of 8, and launch it
    template <class F> void launch(double *out, const double *rhs, hipStream_t s, F &&body) {
        flags_moved();
        for (auto &g : graphs_)
            if (g.out == out && g.rhs == rhs) {
                FAMG_CHECK_HIP(hipGraphLaunch(g.exec, s));
                return;
            }
        hipGraph_t graph = nullptr;
        FAMG_CHECK_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        try {
            body();
        } catch (...) {
            (void)hipStreamEndCapture(s, &graph);
            if (graph) (void)hipGraphDestroy(graph);
            throw;
        }
        FAMG_CHECK_HIP(hipStreamEndCapture(s, &graph));
        hipGraphExec_t exec = nullptr;
        FAMG_CHECK_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        (void)hipGraphDestroy(graph);
        if (graphs_.size() >= 8) {
            (void)hipGraphExecDestroy(graphs_.front().exec);
            graphs_.erase(graphs_.begin());
        }
        graphs_.push_back({out, rhs, exec});
        FAMG_CHECK_HIP(hipGraphLaunch(exec, s));
    }

  private:
    struct Entry {
        double *out;
        const double *rhs;
        hipGraphExec_t exec;
    };
    std::vector<Entry> graphs_;
    uint64_t gen_ = 0;  // flags_generation() the graphs were captured under
};

// How level l takes its step of the V-cycle (MultigridOp::level_shape): decided in one
// place because producers and consumers of d*f must agree -- smooth() skips that pass
// on its caller's word (pre_df), so a disagreement is a wrong cycle, not an error.
struct LevelShape {
    const CsrOp *A = nullptr, *R = nullptr, *P = nullptr;  // the level's operators where they are CSR
    bool fold = false;     // the zero-guess Jacobi step folded into RESID0 + ADD0 (fold_level)
    bool df = false;       // R also writes level l + 1's first Jacobi step d_c f_c (SPMV_SETDF)
    bool fuse_rr = false;  // folded residual + restriction as one marching launch (fine.hip)
    bool fuse_pj = false;  // interpolation + post-smoothing as one
    SpmvEpi epi0, epic;    // fold: d*f of this level's f / df: d_c and where d_c f_c goes
};

// One coarsening step of sa_build (amg_sa_level_info): on_device = the strength graph
// and the aggregation ran on the device; host_reason = why not (the SG_REASON codes);
// longest_ball = the longest candidate list the device counted (0 when it did not look)
struct SaLevelInfo {
    int64_t n, block_size, nodes, aggregates, strength_edges, on_device = 0, host_reason = 0, longest_ball = 0;
};

struct SaRecord;  // what sa_refresh needs of the build (below, with SaConfig)

struct MultigridOp : LinOp {
    std::vector<MgLevel> levels;
    std::vector<SaLevelInfo> sa_levels;  // sa_build's record, one entry per coarsening step
    std::shared_ptr<SaRecord> sa_rec;    // sa_build only: config and aggregates, later the frozen patterns
    int64_t mu = 1, steps = 1;
    bool use_graph = true;
    bool sgs_residual_form = false;  // true: literal smooth() order (residual SpMV + SGS(r))
    // s = 1 Jacobi levels: fold the first smoothing step from v = 0 (v = d*f)
    // into the residual (RESID0) and the correction (ADD0) instead of storing it
    bool fold_zero_guess = true;
    // R on wide grid-transfer classes writes the next level's first Jacobi step
    // from zero beside f_c (SPMV_SETDF) instead of a separate d*f pass
    bool restrict_df = true;
    // locality renumbering of general levels (reorder.hip): 0 off, 1 where it stays
    // bitwise and at least halves the x lines an SpMV slice touches (default), 2 every
    // eligible level
    int reorder = 1;
    std::mutex mtx;
    Kind kind() const override { return Kind::Multigrid; }
    bool is_precond() const override { return true; }
    void apply(double *out, const double *rhs) override;
    // The V-cycle on n x k blocks (flag FLAG_BLOCK_CYCLE; 0: apply() per column): the
    // literal cycle of multigrid.rs:269-380 per level -- pre-smoothing, R (F - A V),
    // mu visits, V += P V_c, post-smoothing -- through spmm_epi, with none of
    // apply()'s single-vector folds; every column bitwise apply().  Eager launches.
    void apply_block(double *out, int64_t ldo, const double *rhs, int64_t ldr, int64_t k) override;
    // launch records of one block cycle of k columns (eager, recorder on)
    std::vector<LaunchRec> block_plan(int64_t k);
    void add_level(LinOpPtr A, LinOpPtr S, LinOpPtr R, LinOpPtr P);
    // sa_refresh's commit: every level's operators replaced at once (R, P: one per
    // coarsening step), under mtx.  The renumbered copies are dropped, the workspaces'
    // value-derived parts, the graphs and the dense tail are rebuilt at the next apply.
    void install_operators(const std::vector<LinOpPtr> &As, const std::vector<LinOpPtr> &Ss,
                           const std::vector<LinOpPtr> &Rs, const std::vector<LinOpPtr> &Ps);
    void ensure_workspace();
    void invalidate_graphs();
    ~MultigridOp() override;

    // V-cycle building blocks (also used by the distributed multigrid)
    // pre_df: the restriction that produced f already wrote the first Jacobi
    // step from zero (d*f, SPMV_SETDF) into the level's t buffer
    void cycle(int64_t l, double *v, const double *f, bool v_zero, bool pre_df = false);
    // the shape of level l < L - 1 entered with right-hand side f (not kept across
    // calls: operators, options and switches may change in between)
    LevelShape level_shape(int64_t l, const double *f, bool v_zero) const;
    void smooth(int64_t l, double *&v, double *&t, const double *f, bool v_zero, bool pre_df = false);
    // the renumbered fine level's rhs gather, with its first Jacobi step from zero
    // written beside it where the level takes that step unfolded
    void gather_fine(const double *rhs, hipStream_t s);
    // launch records of one V-cycle (eager, recorder on)
    std::vector<LaunchRec> cycle_plan();
    // one of the fine level's fused launches exactly as the cycle makes it, on the
    // cycle's workspace (which 0: folded residual + restriction into level 1's f
    // and t; 1: interpolation + post-smoothing from level 1's v into out); false
    // where the cycle does not take it (amg_multigrid_fine_launch: bench timing)
    bool fine_launch(int which, double *out, const double *rhs);
    // renumber eligible levels (first ensure_workspace) / restore the caller's operators
    void reorder_levels();
    void undo_reorder();
    // the same multigrid over the caller's operators (no renumbering)
    std::shared_ptr<MultigridOp> original_view();
    // the dense tail: with mu = 1 every level l >= tail_level is entered with v = 0,
    // so the part of the cycle from tail_level down (smoothing, residual,
    // restriction, the coarser levels, the coarsest solve, correction, post-
    // smoothing) maps that level's f to its v linearly: v = M f.  M (n x n,
    // row-major) is built once by running that part of the cycle on the n unit
    // vectors; the cycle then takes one GEMV there instead of its launches.
    // The first level 1 <= l < L - 1 with n_l <= flag dense_tail (0: off).
    int64_t tail_level = -1;
    void ensure_tail();
    // in-cycle timing of one fused fine-level launch (amg_multigrid_set_fine_timer)
    int fine_timer = -1;
    hipEvent_t fine_ev[2] = {nullptr, nullptr};

  private:
    GraphCache graphs_;
    bool workspace_ready_ = false;
    bool reorder_done_ = false;
    // before any cycle is issued: the hierarchy's invariants, the workspaces, graphs and
    // dense tail of the current switches
    void prepare();
    void run_cycle(double *out, const double *rhs);  // one cycle on the stream, renumbered fine level or not
    void ensure_block_workspace(int64_t kw);
    void block_check(int64_t kw);  // prepare() and the workspaces for kw columns
    void block_run(double *out, int64_t ldo, const double *rhs, int64_t ldr, int64_t kw);
    void block_cycle(int64_t l, double *V, int64_t ldv, const double *F, int64_t ldf, int64_t kw, bool v_zero);
    void block_smooth(int64_t l, double *&V, int64_t &ldv, double *&T, int64_t &ldt, const double *F, int64_t ldf,
                      int64_t kw, bool v_zero);
    DevBuf<double> perm_bf0_, perm_bv0_;  // the block cycle's perm_f0_ / perm_v0_
    DevBuf<double> perm_f0_, perm_v0_;  // the fine level's rhs / result in its numbering
    DevBuf<double> tail_M_;
    uint64_t tail_key_ = ~uint64_t(0);
};
// out (n x n, row-major) = in^T
void dense_transpose(const double *in, double *out, int64_t n, hipStream_t s);
// v = e_j: zeros with a one at j
void unit_vector(double *v, int64_t n, int64_t j, hipStream_t s);
// y = x[p] / y[p] = x over n entries (reorder.hip; launch-plan records)
void perm_gather(double *out, const double *in, const int32_t *p, int64_t n, hipStream_t s);
void perm_scatter(double *out, const double *in, const int32_t *p, int64_t n, hipStream_t s);
// the same over k columns (column-major blocks)
void perm_gather_cols(double *out, int64_t ldo, const double *in, int64_t ldi, const int32_t *p, int64_t n, int64_t k,
                      hipStream_t s);
void perm_scatter_cols(double *out, int64_t ldo, const double *in, int64_t ldi, const int32_t *p, int64_t n, int64_t k,
                       hipStream_t s);
// the gather and the first Jacobi step from zero in one pass: f0 = in[p], t = d * f0
void perm_gather_df(double *f0, double *t, const double *in, const int32_t *p, const DiagOp &D, int64_t n,
                    hipStream_t s);

// the zero-guess fold decision of one level (RESID0 + ADD0 instead of v = d*f)
// m's DIA codes are a constant 7- or 27-point stencil on an nx x ny x nz grid (nx
// even), truncated at the faces: fills m.dia.cst* (sgs27.hip)
bool dia_constant(GpuCsr &m);
bool fold_level(const CsrOp *A, const DiagOp *D, const CsrOp *P, bool fold_zero_guess, bool v_zero, int64_t steps);
// the level takes its first Jacobi step from zero unfolded (smooth(): t = d*f), so
// whoever produces its f may write that step beside it
inline bool level_wants_df(const CsrOp *A, const DiagOp *D, const CsrOp *P, bool fold_zero_guess, int64_t steps) {
    return A && D && steps >= 1 && !fold_level(A, D, P, fold_zero_guess, true, steps);
}
// the restriction into a level writes that level's first Jacobi step from zero
// (SPMV_SETDF) -- false with FAMG_SETDF=0
bool setdf_enabled();
// R serves SPMV_SETDF (a grid-transfer overlay of either width, pattern SELL or 3x3 blocks)
inline bool r_has_setdf(const CsrOp *R) {
    return R && ((R->m.gtx.built() && R->m.gtx.r) || (R->m.gtc.built() && R->m.gtc.r) || R->m.kernel == SPMV_KERNEL_SELLP ||
                 R->m.kernel == SPMV_KERNEL_BSR);
}

// ---------------------------------------------------------------- factories

// sa_build_box(smoother = SGS): levels whose greedy coloring needs more colors
// than this get the L1 smoother instead (each color is one launch over 1/C of
// the rows: a dense Galerkin level with 20+ colors spent 1.6 ms of the 27-pt
// 256^3 V-cycle in latency-bound color launches, profiles/r02)
constexpr int64_t SGS_MAX_COLORS = 8;

CsrPtr make_csr(Ctx *ctx);
std::shared_ptr<DiagOp> make_jacobi(CsrOp &A, double omega);
std::shared_ptr<DiagOp> make_l1(CsrOp &A);
std::shared_ptr<DiagOp> make_l2(CsrOp &A);
std::shared_ptr<SgsOp> make_sgs(const CsrPtr &A, const int32_t *colors, bool validate = true);
// SGS over the owned rows of a distributed level (A: owned rows x [owned | ghost]
// columns; a row's columns keep the global order, so they need not ascend);
// colors: the global smoother's colors of those rows, ncolors the global count
// (every rank sweeps the same colors); aii: their diagonal (device, owned rows)
std::shared_ptr<SgsOp> make_sgs_slice(const CsrPtr &A, const int32_t *colors, int64_t ncolors, const double *aii);
// fused SGS phases for a 27-point grid operator stored as DIA codes (sgs27.hip)
// SgsOps built afterwards use the fused phases where they apply (default 1,
// FAMG_SGS_FUSED=0 sets 0; amg_set_sgs_fused)
extern int g_sgs_fused;
void sgs27_setup(SgsOp &S);
bool sgs27_applies(const SgsOp &S, const double *x, const double *b);  // fused and 16-B aligned vectors
void sgs27_sweep(SgsOp &S, double *x, const double *b, bool zero);
std::shared_ptr<CoarseCholOp> make_coarse_chol(CsrOp &A);
// AMG_ERR_INVALID for config values out of range (chebyshev_check: host only),
// AMG_ERR_DIM for a non-square A, AMG_ERR_NOT_SPD for a diagonal entry <= 0
void chebyshev_check(const ChebyConfig &cfg);
std::shared_ptr<ChebyOp> make_chebyshev(const CsrPtr &A, const ChebyConfig &cfg);

// SA setup pieces
CsrPtr sa_tentative(Ctx *ctx, int64_t n, const int64_t *agg_of, int64_t naggs,
                    const double *nn, double *coarse_nn);
CsrPtr smooth_interpolation(CsrOp &A, const CsrOp &P, double omega);
// Galerkin A_c = R (A P); grid: the coarse grid dims (hint for the x-staged
// stencil kernels) or null
CsrPtr galerkin_rap(const CsrOp &R, const CsrOp &A, const CsrOp &P, const int64_t *grid = nullptr);
CsrPtr transpose_op(const CsrOp &P);
CsrPtr spgemm_op(const CsrOp &A, const CsrOp &B);
void nn_stationary_l1(CsrOp &A, int64_t iters, double *x_host);
int64_t greedy_coloring(const GpuCsr &A, std::vector<int32_t> &color);
// BlockSmoother apply data: blocks in block-major row order, explicit inverses
// (column-major), chunks of <= 256 rows of whole blocks (block.hip).
struct BlockSmootherOp : LinOp {
    int64_t nblocks = 0, vdim = 1, max_block = 0, nchunks = 0;
    std::vector<int64_t> h_bptr;   // host copies (to_csr)
    std::vector<int32_t> h_rows;
    DevBuf<int32_t> rows;          // block-major original row ids (n)
    DevBuf<int32_t> blk_of;        // block of each block-major position (n)
    DevBuf<int64_t> bptr;          // nblocks+1
    DevBuf<int64_t> ioff;          // nblocks+1 offsets of the inverses
    DevBuf<int32_t> chunk;         // nchunks+1 position bounds (block aligned)
    DevBuf<double> inv;
    // k-wide apply: the chunks by size class, each class with the
    // column width W its LDS tile (8 * rows * W bytes <= 64 KB) admits, decided at setup
    static constexpr int NCLS = 5;
    static constexpr int CLS_ROWS[NCLS] = {256, 1024, 2048, 4096, 8192};  // chunk rows <= this
    static constexpr int CLS_W[NCLS] = {8, 8, 4, 2, 1};
    int64_t inv_elems = 0;             // sum of s_b^2
    int64_t cls_off[NCLS + 1] = {};    // class c owns cls_list[cls_off[c] .. cls_off[c + 1])
    int64_t cls_rows[NCLS] = {}, cls_inv[NCLS] = {}, cls_max_rows[NCLS] = {};
    DevBuf<int32_t> cls_list;          // chunk ids, class by class
    Kind kind() const override { return Kind::Block; }
    bool is_precond() const override { return true; }
    void apply(double *out, const double *rhs) override;
    // each class once per group of up to W columns, the inverses read once per group
    // (FLAG_BLOCK_SMOOTHER_COLS; 0 or k = 1: apply() per column); out == rhs with
    // ldo == ldr is legal
    void apply_block(double *out, int64_t ldo, const double *rhs, int64_t ldr, int64_t k) override;
    void apply_in_place(double *rhs) override { apply(rhs, rhs); }
};
// BlockSmoother (block_smoothers.rs:80-291) over a node partition (ids 0..nagg-1,
// n/vdim nodes); blocks diagonally compensated and inverted exactly (block.hip).
std::shared_ptr<BlockSmootherOp> make_block_smoother(CsrOp &A, const int64_t *part, int64_t nagg, int64_t vdim);
std::shared_ptr<MultigridOp> sa_build_box(const CsrPtr &A, int64_t nx, int64_t ny, int64_t nz,
                                          int64_t bx, int64_t by, int64_t bz,
                                          int64_t coarsest_dim, int64_t max_levels,
                                          double omega, int smoother);

// ------------------------------------------------ general SA setup (sa.hip)

// Node-level strength graph (partitioners/mod.rs:337-393, block-reduced
// :294-301): CSR with strengths in (0, 1].
struct StrengthGraph {
    int64_t n = 0;
    std::vector<int64_t> rp;
    std::vector<int32_t> col;
    std::vector<double> w;
};
StrengthGraph strength_graph(const CsrOp &A, const double *nn, int64_t ld, int64_t k, const double *w,
                             int64_t depth, int64_t bs);
// MIS-seeded aggregates of a strength graph; returns the aggregate count
// (stats2, optional: {roots, singleton roots})
int64_t aggregate_mis(const StrengthGraph &G, std::vector<int64_t> &agg_of, int64_t *stats2 = nullptr);
// The tail of aggregate_mis, shared with the device path: agg = a label per node
// (the root's, indexing size0 = the aggregate sizes before any merge), singles =
// the singleton roots ascending, row q of them = entries [sbeg[q], send[q]) of
// col / w.  Every singleton joins its strongest neighbour's aggregate (size >= 2)
// in that order, then the live aggregates are numbered by their smallest node.
int64_t aggregate_finish(int64_t n, std::vector<int64_t> &agg, const std::vector<int64_t> &size0,
                         const std::vector<int64_t> &singles, const int64_t *sbeg, const int64_t *send,
                         const int32_t *col, const double *w, std::vector<int64_t> &agg_of);
// Where sa_build and find_near_null run the strength graph and the aggregation
// (amg_set_sa_setup): 0 host (default), 1 device (sagraph.hip) at any strength depth
extern int g_sa_setup;
constexpr int64_t SG_MAX_ROW = 4096;  // candidates of a dof row the device strength graph ranks (and the ball cap)
// why a level's strength graph cannot run on the device (SaLevelInfo::host_reason)
enum : int { SG_REASON_NONE = 0, SG_REASON_POLICY = 1, SG_REASON_BALL_CAP = 2, SG_REASON_BYTES = 3, SG_REASON_INDEX = 4 };
// The BFS ball of every row of a square CSR pattern (sagraph.hip): row i lists what
// extract_local_subgraph(pattern, i, depth) reaches over stored entries, without i,
// columns ascending.  kept = sum over rows of the entries the strength graph keeps.
struct BallPattern {
    DevBuf<int64_t> rp;
    DevBuf<int32_t> col;
    int64_t entries = 0, longest = 0, wave_rows = 0, block_rows = 0, kept = 0;
};
// Returns an SG_REASON code: NONE with `out` filled; BALL_CAP for a ball beyond
// SG_MAX_ROW members (out.longest then is a lower bound), INDEX for 2^31 or more ball
// or kept entries, BYTES (only with check_bytes) when 4 B per ball entry + 8 B per row
// pointer + 12 B per kept entry exceed max_bytes (0: half the free device memory).
// Counts are filled in either case; rp / col only with NONE.
int ball_pattern_device(const GpuCsr &m, int64_t depth, bool check_bytes, int64_t max_bytes, BallPattern &out);
struct SgDeviceInfo {
    int64_t longest_ball = 0, wave_rows = 0, block_rows = 0, ball_entries = 0, dof_entries = 0, node_edges = 0;
    int reason = SG_REASON_NONE;
};
// strength_graph at `depth` on the device (nn a device block): the node-level graph
// as a CSR without SpMV storage.  The weight is (t*t)*(t*t) where the host takes
// std::pow(t, 4.0); everything else gives the host's bits.  Depth 1 ranks the
// matrix rows, depth >= 2 the rows of ball_pattern_device (freed before the node
// merge allocates).  A level that cannot run (info->reason: BALL_CAP, BYTES against
// max_bytes, INDEX) gives a null result when `fallback`, else AMG_ERR_UNSUPPORTED.
// At depth 1 longest_ball counts only rows beyond a wave's 256 and ball_entries is 0.
CsrPtr strength_graph_device(const CsrOp &A, const double *nn, int64_t ld, int64_t k, const double *w, int64_t bs,
                             int64_t depth, int64_t max_bytes, SgDeviceInfo *info, bool fallback);
// aggregate_mis of a device graph: the root / claim phase in bounded passes on the
// device, the tail on the host; past max_passes (0: the default budget) the host
// sweep on the downloaded graph.  The same result either way.  info4 (optional) =
// {passes run, roots, singleton roots, fell back (0/1)}
int64_t aggregate_mis_device(const GpuCsr &G, int64_t max_passes, std::vector<int64_t> &agg_of, int64_t *info4);
// ---- the modularity partitioner (partition_host.cpp, partition.hip)
// PartitionerConfig (partitioners/mod.rs:249-329) + the device pass budget per matching round
struct PartitionerConfig {
    double cf = 8.0, pen = 1.0;
    int64_t max_improve = 100, max_passes = 0;
};
// info8: {matching rounds, device passes (sum), most passes in one round, fell back
// to the host (0/1), improvement passes, swaps accepted, smallest, largest aggregate}
// The contracted graph between two matching rounds: vertex v of nv owns row v
// (columns ascending, self loops kept), row sum rs[v], size[v] fine nodes;
// node_to_v maps the n fine nodes.
struct ModState {
    int64_t nv = 0;
    std::vector<int64_t> rp;
    std::vector<int32_t> col;
    std::vector<double> w, rs;
    std::vector<int64_t> size, node_to_v;
};
// splitmix64 finaliser of (i << 32) | j: the tie-break of the edge order
__host__ __device__ inline uint64_t mod_mix(uint64_t i, uint64_t j) {
    uint64_t z = ((i << 32) | j) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// edge (w, i, j) precedes edge (w2, i2, j2): larger w, then smaller mix, i, j
__host__ __device__ inline bool mod_precedes(double w, int64_t i, int64_t j, double w2, int64_t i2, int64_t j2) {
    if (w != w2) return w > w2;
    const uint64_t m = mod_mix((uint64_t)i, (uint64_t)j), m2 = mod_mix((uint64_t)i2, (uint64_t)j2);
    if (m != m2) return m < m2;
    if (i != i2) return i < i2;
    return j < j2;
}
// modularity weight of the candidate edge between vertices of sizes si, sj
__host__ __device__ inline double mod_edge_weight(double s, double inv_total, double rsi, double rsj, int64_t si,
                                                  int64_t sj, double cf, double pen) {
    double w = s - (inv_total * rsi) * rsj;
    const double t = (double)(si + sj) - cf;
    if ((double)(si + sj) > cf) w -= pen * (t * t);
    else w += pen * (t * t);
    return w;
}
// size_cost (modularity.rs:385-389) with products for powf(4.)
__host__ __device__ inline double mod_size_cost(int64_t s, double cf, double pen) {
    const double d = (double)s - cf;
    const double u = 4.0 * ((d < 0.0 ? -d : d) / cf);
    return ((u * u) * (u * u)) * pen;
}
__host__ __device__ inline double mod_delta_q(double in, double out, int64_t dst, int64_t src, double cf, double pen) {
    return (out - in) + pen * ((mod_size_cost(dst, cf, pen) + mod_size_cost(src, cf, pen)) -
                               (mod_size_cost(dst + 1, cf, pen) + mod_size_cost(src - 1, cf, pen)));
}
// base row sums (negative clamped to 0) are the caller's; their total, summed in
// ascending node order, inverted.  AMG_ERR_INVALID for a non-finite or zero total.
double mod_inverse_total(const std::vector<double> &rs);
// matching rounds from state S until nnodes / nv >= cf or a round finds no pair
void mod_rounds_host(ModState &S, const PartitionerConfig &cfg, double inv_total, int64_t *info8);
struct ModProposal {
    int32_t node, agg;
    double dq;
};
// the serial selection of one improvement pass (modularity.rs:477-504) over the
// proposals (any order; sorted here); returns the swaps accepted and lists the
// touched nodes / aggregates (for the device path's uploads)
int64_t mod_select_swaps(std::vector<ModProposal> &props, const int64_t *rp, const int32_t *col,
                         std::vector<int64_t> &agg, std::vector<int64_t> &size, std::vector<int64_t> *moved);
// improvement passes on the host; then aggregates renumbered by smallest node
void mod_improve_host(const StrengthGraph &G, const PartitionerConfig &cfg, std::vector<int64_t> &agg,
                      std::vector<int64_t> &size, int64_t *info8);
int64_t mod_renumber(std::vector<int64_t> &agg, int64_t na, int64_t *info8);
int64_t partition_modularity(const StrengthGraph &G, const PartitionerConfig &cfg, std::vector<int64_t> &agg_of,
                             int64_t *info8);
int64_t partition_modularity_device(const GpuCsr &G, const PartitionerConfig &cfg, std::vector<int64_t> &agg_of,
                                    int64_t *info8);
PartitionerConfig mod_config_from(const amg_partitioner_config *cfg);  // validates: AMG_ERR_INVALID
// amg_set_sa_partitioner: 0 MIS (default), 1 modularity with g_sa_part_cfg
extern int g_sa_partitioner;
extern PartitionerConfig g_sa_part_cfg;
// tentative P for k candidates on nodes of bs dofs (interpolation/mod.rs:754-805)
CsrPtr sa_tentative_block(Ctx *ctx, int64_t nnodes, int64_t bs, const int64_t *agg_of, int64_t naggs,
                          const double *nn, int64_t ld, int64_t k, int64_t cd, double *coarse_nn);
// block_jacobi P smoothing (interpolation/mod.rs:963-1028)
CsrPtr block_jacobi_smooth(CsrOp &A, const CsrOp &P, int64_t bs, double omega);
// its left factor -omega D^-1 (D = A's bs x bs diagonal blocks) as a CSR of full blocks;
// AMG_ERR_NOT_SPD for a block with an eigenvalue <= 1e-6
CsrPtr block_jacobi_dinv(CsrOp &A, int64_t bs, double omega);
// create_weights (examples/amg/main.rs:571-580): w_c = 1 / (v_c^T A v_c), near-null on the host
std::vector<double> default_weights(CsrOp &A, const double *nn, int64_t ld, int64_t k);
// coarse near-null post-processing for k columns (hierarchy.rs:219-228)
void nn_postprocess(CsrOp &A, int64_t iters, double *x, int64_t ld, int64_t k);
struct SaConfig {
    int64_t block_size = 1, candidate_dimension = 1, strength_depth = 1, smoothing_steps = 1;
    int64_t coarsest_dim = 1000, max_levels = 0;
    double omega = 0.66;
    int smoother = 1;
    int chebyshev_steps = 0;  // smoother 4: steps per application (0 = ChebyConfig's default)
};
std::shared_ptr<MultigridOp> sa_build(const CsrPtr &A, const double *nn, int64_t ld, int64_t k,
                                      const double *weights, const SaConfig &cfg, std::vector<SaLevelInfo> *info);
// the smoother cfg names for level operator M (agg / naggs / bs: the level's aggregates, smoother 3)
LinOpPtr sa_make_smoother(const SaConfig &cfg, const CsrPtr &M, const int64_t *agg, int64_t naggs, int64_t bs);

// ------------------------------------------- SA numeric refresh (refresh.hip)

// C's values = A B on C's given pattern (rows' columns ascending): every entry from 0.0,
// fma(a_e, b, acc) in ascending order of the entries e of A's row -- spgemm's values
// bit for bit; entries of C outside the product end 0.0.  AMG_ERR_INVALID (C's values
// then undefined, nothing written outside them) if a product column is missing from C.
// C is not finalized.
void spgemm_refill(const GpuCsr &A, const GpuCsr &B, GpuCsr &C);
// perm (device, P.nnz entries): entry q of R = P^T holds entry perm[q] of P; R's pattern
// must be P's transpose with ascending columns (AMG_ERR_INVALID otherwise)
void transpose_perm(const GpuCsr &P, const GpuCsr &R, int32_t *perm);
// R.val[q] = P.val[perm[q]]; AMG_ERR_INVALID for an entry of perm outside P.  R is not finalized.
void transpose_refill(const GpuCsr &P, GpuCsr &R, const int32_t *perm);
// What a hierarchy of sa_build keeps for sa_refresh: the config, the candidate count
// and every coarsening step's aggregates (host); after the first refresh the patterns
// the symbolic passes produced (device, no values) and the transpose permutations.
struct SaRefreshPatterns {
    struct Step {
        std::vector<GpuCsr> ap, s;  // per smoothing step: A P, and (block size > 1) D^-1 (A P)
        GpuCsr rap_ap;              // A P of the Galerkin product
        DevBuf<int32_t> perm;       // R = P^T as a gather
    };
    std::vector<Step> steps;
    int64_t bytes = 0;
};
struct SaRecord {
    SaConfig cfg;
    int64_t k = 0;
    std::vector<std::vector<int64_t>> aggs;  // per coarsening step: aggregate of every node
    std::vector<int64_t> naggs, bss;         // bss: block size of every level
    std::shared_ptr<SaRefreshPatterns> pat;  // null until the first refresh
};
// The hierarchy sa_build would make for A (the build's pattern, new values) and nn had
// strength and aggregation returned the recorded aggregates; mg changes only if every
// stage succeeds.  info8 = {recorded (1) or reused (0) the patterns, device bytes of the
// record, levels, coarsening steps, 0...}.
void sa_refresh(MultigridOp &mg, const CsrPtr &A, const double *nn, int64_t ld, int64_t k, int64_t *info8);

// ------------------------------------------- near-null search (nearnull.hip)

constexpr int64_t QR_MAX_K = 64;  // widest block of the thin QR
// In-place thin QR of the column-major n x k device block X (CholeskyQR2 with a
// shifted fallback); R (host, k x k column-major, positive diagonal) may be null.
// Synchronises the context stream (the k x k factors are computed on the host).
void thin_qr(Ctx &ctx, double *X, int64_t ld, int64_t n, int64_t k, double *R);
// smooth_vector (adaptivity.rs:307-390) on the device block X (n x k): two QRs,
// `iters` times X <- thinQ(X - pc(A X)); cfs (host, k; may be null) = the A-norm
// convergence factor of every returned column
void smooth_vectors(CsrOp &A, LinOp &pc, double *X, int64_t ld, int64_t k, int64_t iters, double *cfs);
// create_weights (adaptivity.rs:434-443): w_c = 1 / (x_c^T A x_c), X on the device, w on the host
void create_weights(CsrOp &A, const double *X, int64_t ld, int64_t k, double *w);
// find_near_null (adaptivity.rs:264-305): X (device) holds the start block of both
// stages and returns the stage-2 basis
void find_near_null(const CsrPtr &A, double *X, int64_t ld, int64_t k, int64_t iters, int64_t block_size,
                    int64_t strength_depth, double *cfs);

}  // namespace famg
