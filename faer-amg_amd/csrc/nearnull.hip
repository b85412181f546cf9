// nearnull.hip -- the device near-null search (adaptivity.rs:264-390, 434-443):
// a tall-skinny thin QR, the k-wide error-propagation step X <- X - pc(A X), the
// A-norm convergence factors and the A-norm weights of the strength graph.
//
// Thin QR of an n x k block (k <= 64) is CholeskyQR2: G = X^T X on the device,
// the k x k Cholesky factor R and its inverse on the host, X <- X R^-1 on the
// device, twice.  A pass whose Cholesky breaks down (a pivot <= 16 k eps ||G||_F:
// kappa(X) beyond ~1e7) is replaced by a shifted pass, G + s I with
// s = 11 (n k + k (k + 1)) u ||G||_F (shifted CholeskyQR3), after which the two
// ordinary passes start over; a block that still breaks down after two shifted
// passes, or whose R ends with a diagonal entry <= 16 k eps ||X||, is rank
// deficient (DESIGN.md "Near-null search").
//
// The Gram kernel runs on the fp64 matrix cores (v_mfma_f64_16x16x4_f64): a
// workgroup stages 64 rows x k columns through LDS with coalesced loads and each
// wave accumulates the upper 16 x 16 tiles of G over its 16 rows; the waves and
// then the workgroups are summed in a fixed order, no atomics.  The update kernel
// gives every lane one row, held in registers, and reads R^-1 through uniform
// (scalar) loads.  Every reduction here has a fixed shape and order, so repeated
// calls are bitwise equal.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "famg.hpp"

namespace famg {

typedef double dbl4 __attribute__((ext_vector_type(4)));

constexpr int GRAM_ROWS = 64;             // rows a workgroup stages per step (4 waves x 16)
constexpr int GRAM_LDS = GRAM_ROWS + 1;   // LDS column stride (conflict-free operand reads)
constexpr int COLDOT_GRID = 256;          // row blocks of the column-dot reduction

// ------------------------------------------------------------------ Gram

// partials[b] (KP x KP, row-major, KP = 16 NB) = the upper 16 x 16 tiles of X_b^T X_b
// over rows [b * rows_per_block, (b + 1) * rows_per_block) of X; lower tiles 0.
// MFMA operands (one fp64 per lane): A[i = lane & 15][kk = lane >> 4] = x(row kk, column
// 16 I + i), B the same of column block J; D: column lane & 15, row (lane >> 4) + 4 reg.
template <int NB>
__global__ __launch_bounds__(256) void k_gram_partial(const double *__restrict__ X, int64_t ld, int64_t n, int k,
                                                      int64_t rows_per_block, double *__restrict__ partials) {
    constexpr int KP = 16 * NB;
    constexpr int NL = KP / 4;  // staging loads per thread and step: column 4 i + wave, row lane
    constexpr int NT = NB * (NB + 1) / 2;
    __shared__ double sh[KP * GRAM_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r_begin = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r_end = r_begin + rows_per_block < n ? r_begin + rows_per_block : n;
    const int64_t steps = r_end > r_begin ? (r_end - r_begin + GRAM_ROWS - 1) / GRAM_ROWS : 0;
    double reg[NL];
    dbl4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = dbl4{0.0, 0.0, 0.0, 0.0};
    const int c = lane & 15, q = lane >> 4;
    for (int64_t st = 0; st <= steps; st++) {
        if (st > 0) {
            __syncthreads();  // the previous step's operand reads are done
#pragma unroll
            for (int i = 0; i < NL; i++) sh[(4 * i + wave) * GRAM_LDS + lane] = reg[i];
            __syncthreads();
        }
        if (st < steps) {  // the next step's rows, in flight under this step's products
            const int64_t r = r_begin + st * GRAM_ROWS + lane;
#pragma unroll
            for (int i = 0; i < NL; i++) {
                const int col = 4 * i + wave;
                reg[i] = (r < r_end && col < k) ? X[(int64_t)col * ld + r] : 0.0;
            }
        }
        if (st > 0) {
#pragma unroll
            for (int s = 0; s < 4; s++) {
                double a[NB];
#pragma unroll
                for (int b = 0; b < NB; b++) a[b] = sh[(16 * b + c) * GRAM_LDS + 16 * wave + 4 * s + q];
                int t = 0;
#pragma unroll
                for (int I = 0; I < NB; I++)
#pragma unroll
                    for (int J = I; J < NB; J++, t++)
                        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[I], a[J], acc[t], 0, 0, 0);
            }
        }
    }
    // the four waves' tiles summed in wave order (sh reused: KP * KP <= KP * GRAM_LDS)
    for (int w = 0; w < 4; w++) {
        __syncthreads();
        if (wave == w) {
            int t = 0;
#pragma unroll
            for (int I = 0; I < NB; I++)
#pragma unroll
                for (int J = I; J < NB; J++, t++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        double *p = &sh[(16 * I + q + 4 * r) * KP + 16 * J + c];
                        *p = w == 0 ? acc[t][r] : *p + acc[t][r];
                    }
        }
    }
    __syncthreads();
    double *out = partials + (int64_t)blockIdx.x * (KP * KP);
    for (int e = tid; e < KP * KP; e += 256) out[e] = (e / KP) / 16 <= (e % KP) / 16 ? sh[e] : 0.0;
}

// G = the partials summed in a fixed order: 16 entries per workgroup, each by 16
// threads that take every 16th workgroup's partial in ascending order and are then
// summed in thread order (kp2 is a multiple of 256)
__global__ __launch_bounds__(256) void k_gram_final(const double *__restrict__ partials, int64_t nblk, int kp2,
                                                    double *__restrict__ G) {
    __shared__ double sh[16][17];
    const int le = threadIdx.x & 15, j = threadIdx.x >> 4;
    const int e = blockIdx.x * 16 + le;
    double s = 0.0;
    for (int64_t b = j; b < nblk; b += 16) s += partials[b * kp2 + e];
    sh[j][le] = s;
    __syncthreads();
    if (j == 0) {
        double t = 0.0;
        for (int q = 0; q < 16; q++) t += sh[q][le];
        G[e] = t;
    }
}

void gram_final(const double *partials, int64_t nblk, int kp2, double *G, hipStream_t s) {
    k_gram_final<<<dim3((unsigned)(kp2 / 16)), dim3(256), 0, s>>>(partials, nblk, kp2, G);
}

// ------------------------------------------------------------------ update

// X <- X Rinv in place: one row per lane in registers, Rinv (KB x KB column-major, upper
// triangular, zero beyond k) the same address for every lane
template <int KB>
__global__ __launch_bounds__(256) void k_qr_update(double *__restrict__ X, int64_t ld, int64_t n, int k,
                                                   const double *__restrict__ Rinv) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    double x[KB];
#pragma unroll
    for (int i = 0; i < KB; i++) x[i] = i < k ? X[(int64_t)i * ld + r] : 0.0;
#pragma unroll
    for (int j = 0; j < KB; j++) {
        if (j < k) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i <= j; i++) s = fma(x[i], Rinv[j * KB + i], s);
            X[(int64_t)j * ld + r] = s;
        }
    }
}

// ------------------------------------------------ k-wide vector kernels

// X <- X - d o Y over k columns (d == nullptr: X <- X - Y); out != nullptr: written
// there (leading dimension ldo) instead of in place
__global__ __launch_bounds__(256) void k_block_update(double *__restrict__ X, int64_t ldx, const double *__restrict__ Y,
                                                      int64_t ldy, const double *__restrict__ d, int64_t n, int k,
                                                      double *__restrict__ out, int64_t ldo) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double di = d ? d[i] : 1.0;
    for (int c0 = 0; c0 < k; c0 += 8) {
        double x[8], y[8];
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (c0 + u < k) {
                x[u] = X[(int64_t)(c0 + u) * ldx + i];
                y[u] = Y[(int64_t)(c0 + u) * ldy + i];
            }
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (c0 + u < k) {
                const double v = x[u] - di * y[u];
                if (out) out[(int64_t)(c0 + u) * ldo + i] = v;
                else X[(int64_t)(c0 + u) * ldx + i] = v;
            }
    }
}

__device__ __forceinline__ double nn_block_sum(double v, double *sh) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// partials[c * gridDim.x + b] = the part of a_c . b_c over row block b's rows
__global__ __launch_bounds__(256) void k_coldot_partial(const double *__restrict__ A, int64_t lda,
                                                        const double *__restrict__ B, int64_t ldb, int64_t n,
                                                        double *__restrict__ partials) {
    __shared__ double sh[4];
    const double *a = A + (int64_t)blockIdx.y * lda, *b = B + (int64_t)blockIdx.y * ldb;
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) acc = fma(a[i], b[i], acc);
    const double t = nn_block_sum(acc, sh);
    if (threadIdx.x == 0) partials[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void k_coldot_final(const double *__restrict__ partials, int nb,
                                                      double *__restrict__ out) {
    __shared__ double sh[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) acc += partials[(int64_t)blockIdx.x * nb + i];
    const double t = nn_block_sum(acc, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

// ------------------------------------------------------------------ host side

// device and host scratch of the QRs and dots of one call
struct NearNullWork {
    DevBuf<double> partials, G, Rinv, dots, dot_partials;
    std::vector<double> hG, hRinv;
    int64_t gram_blocks = 0, rows_per_block = 0;
    void reserve(const Ctx &ctx, int64_t n, int64_t k) {
        const int64_t kp = 16 * ceil_div(k, 16), chunks = std::max<int64_t>(1, ceil_div(n, GRAM_ROWS));
        const int64_t want = std::min<int64_t>(chunks, 4 * (int64_t)ctx.num_cus);
        rows_per_block = ceil_div(chunks, want) * GRAM_ROWS;
        gram_blocks = std::max<int64_t>(1, ceil_div(n, rows_per_block));
        partials.resize(gram_blocks * kp * kp);
        G.resize(kp * kp);
        Rinv.resize(QR_MAX_K * QR_MAX_K);
        dots.resize(2 * k);
        dot_partials.resize(k * COLDOT_GRID);
        hG.resize(kp * kp);
        hRinv.resize(QR_MAX_K * QR_MAX_K);
    }
};

static void gram(const double *X, int64_t ld, int64_t n, int64_t k, NearNullWork &w, hipStream_t s) {
    const int nb = (int)ceil_div(k, 16), kp = 16 * nb;
    const dim3 grid((unsigned)w.gram_blocks), block(256);
    switch (nb) {
    case 1: k_gram_partial<1><<<grid, block, 0, s>>>(X, ld, n, (int)k, w.rows_per_block, w.partials.get()); break;
    case 2: k_gram_partial<2><<<grid, block, 0, s>>>(X, ld, n, (int)k, w.rows_per_block, w.partials.get()); break;
    case 3: k_gram_partial<3><<<grid, block, 0, s>>>(X, ld, n, (int)k, w.rows_per_block, w.partials.get()); break;
    default: k_gram_partial<4><<<grid, block, 0, s>>>(X, ld, n, (int)k, w.rows_per_block, w.partials.get()); break;
    }
    gram_final(w.partials.get(), w.gram_blocks, kp * kp, w.G.get(), s);
    FAMG_CHECK_HIP(hipGetLastError());
    FAMG_CHECK_HIP(hipMemcpyAsync(w.hG.data(), w.G.get(), (size_t)kp * kp * sizeof(double), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
}

static void qr_update(double *X, int64_t ld, int64_t n, int64_t k, const double *rinv /* k x k column-major */,
                      NearNullWork &w, hipStream_t s) {
    const int kb = 8 * (int)ceil_div(k, 8);
    std::fill(w.hRinv.begin(), w.hRinv.end(), 0.0);
    for (int64_t j = 0; j < k; j++)
        for (int64_t i = 0; i <= j; i++) w.hRinv[j * kb + i] = rinv[j * k + i];
    FAMG_CHECK_HIP(hipMemcpyAsync(w.Rinv.get(), w.hRinv.data(), (size_t)kb * kb * sizeof(double),
                                  hipMemcpyHostToDevice, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));  // hRinv is reused by the next pass
    const dim3 grid((unsigned)ceil_div(n, 256)), block(256);
#define FAMG_QRU(KB) case KB: k_qr_update<KB><<<grid, block, 0, s>>>(X, ld, n, (int)k, w.Rinv.get()); break
    switch (kb) {
        FAMG_QRU(8);
        FAMG_QRU(16);
        FAMG_QRU(24);
        FAMG_QRU(32);
        FAMG_QRU(40);
        FAMG_QRU(48);
        FAMG_QRU(56);
    default: k_qr_update<64><<<grid, block, 0, s>>>(X, ld, n, (int)k, w.Rinv.get()); break;
    }
#undef FAMG_QRU
    FAMG_CHECK_HIP(hipGetLastError());
}

// upper Cholesky factor R (k x k column-major) of the upper triangle of G (row-major,
// row stride kp) + shift I; false when a pivot is <= tol
static bool chol_upper(const double *G, int kp, int64_t k, double shift, double tol, double *R) {
    std::fill(R, R + k * k, 0.0);
    for (int64_t j = 0; j < k; j++) {
        for (int64_t i = 0; i <= j; i++) {
            double s = G[i * kp + j] + (i == j ? shift : 0.0);
            for (int64_t p = 0; p < i; p++) s -= R[i * k + p] * R[j * k + p];
            if (i < j) {
                R[j * k + i] = s / R[i * k + i];
            } else {
                if (!(s > tol)) return false;
                R[j * k + j] = std::sqrt(s);
            }
        }
    }
    return true;
}

// inverse of an upper triangular R (both k x k column-major)
static void tri_inverse(const double *R, int64_t k, double *inv) {
    std::fill(inv, inv + k * k, 0.0);
    for (int64_t j = 0; j < k; j++) {
        inv[j * k + j] = 1.0 / R[j * k + j];
        for (int64_t i = j - 1; i >= 0; i--) {
            double s = 0.0;
            for (int64_t p = i + 1; p <= j; p++) s += R[p * k + i] * inv[j * k + p];
            inv[j * k + i] = -s / R[i * k + i];
        }
    }
}

static void thin_qr_work(Ctx &ctx, double *X, int64_t ld, int64_t n, int64_t k, double *R_out, NearNullWork &w) {
    hipStream_t s = ctx.stream;
    const int kp = 16 * (int)ceil_div(k, 16);
    std::vector<double> R(k * k, 0.0), Rp(k * k), inv(k * k), tmp(k * k);
    for (int64_t j = 0; j < k; j++) R[j * k + j] = 1.0;
    const double eps = 2.220446049250313e-16;
    int clean = 0, shifted = 0;
    double xnorm = 0.0;  // ||G||_F^(1/2) of the block as given: >= ||X||_2
    while (clean < 2) {
        gram(X, ld, n, k, w, s);
        double fro = 0.0;
        for (int64_t i = 0; i < k; i++)
            for (int64_t j = i; j < k; j++) {
                const double g = w.hG[i * kp + j];
                fro += (i == j ? 1.0 : 2.0) * g * g;
            }
        fro = std::sqrt(fro);
        FAMG_REQUIRE(std::isfinite(fro), AMG_ERR_INVALID, "thin_qr: the block has non-finite entries");
        const double tol = 16.0 * (double)k * eps * fro;
        if (clean == 0 && shifted == 0) xnorm = std::sqrt(fro);
        if (chol_upper(w.hG.data(), kp, k, 0.0, tol, Rp.data())) {
            clean++;
        } else {
            // shifted pass (shifted CholeskyQR3): ||X||_2^2 <= ||G||_F
            FAMG_REQUIRE(shifted < 2 && fro > 0.0, AMG_ERR_INVALID,
                         "thin_qr: the block is rank deficient (Cholesky of X^T X broke down after two shifted passes)");
            const double shift = 11.0 * ((double)n * (double)k + (double)k * (double)(k + 1)) * (0.5 * eps) * fro;
            FAMG_REQUIRE(chol_upper(w.hG.data(), kp, k, shift, 0.0, Rp.data()), AMG_ERR_INVALID,
                         "thin_qr: the shifted Cholesky of X^T X broke down");
            shifted++;
            clean = 0;
        }
        tri_inverse(Rp.data(), k, inv.data());
        qr_update(X, ld, n, k, inv.data(), w, s);
        // R <- Rp R
        for (int64_t j = 0; j < k; j++)
            for (int64_t i = 0; i < k; i++) {
                double t = 0.0;
                for (int64_t p = i; p <= j; p++) t += Rp[p * k + i] * R[j * k + p];
                tmp[j * k + i] = i <= j ? t : 0.0;
            }
        R.swap(tmp);
    }
    // a shifted pass turns the rounding noise left of a dependent column into a unit
    // column; R tells: its diagonal entry is that noise, a few eps ||X||
    if (shifted)
        for (int64_t j = 0; j < k; j++)
            FAMG_REQUIRE(R[j * k + j] > 16.0 * (double)k * eps * xnorm, AMG_ERR_INVALID,
                         "thin_qr: the block is rank deficient (a diagonal entry of R <= 16 k eps ||X||)");
    if (R_out) std::memcpy(R_out, R.data(), (size_t)k * k * sizeof(double));
}

void thin_qr(Ctx &ctx, double *X, int64_t ld, int64_t n, int64_t k, double *R) {
    NearNullWork w;
    w.reserve(ctx, n, k);
    thin_qr_work(ctx, X, ld, n, k, R, w);
}

// out[c] (host) = a_c . b_c for k columns
static void coldot(const double *A, int64_t lda, const double *B, int64_t ldb, int64_t n, int64_t k, double *dev_out,
                   NearNullWork &w, hipStream_t s) {
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(COLDOT_GRID, ceil_div(n, 256)));
    k_coldot_partial<<<dim3((unsigned)nb, (unsigned)k), dim3(256), 0, s>>>(A, lda, B, ldb, n, w.dot_partials.get());
    k_coldot_final<<<dim3((unsigned)k), dim3(256), 0, s>>>(w.dot_partials.get(), nb, dev_out);
    FAMG_CHECK_HIP(hipGetLastError());
}

static void block_update(double *X, int64_t ldx, const double *Y, int64_t ldy, const double *d, int64_t n, int64_t k,
                         double *out, int64_t ldo, hipStream_t s) {
    k_block_update<<<dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s>>>(X, ldx, Y, ldy, d, n, (int)k, out, ldo);
    FAMG_CHECK_HIP(hipGetLastError());
}

// out (or X in place) = X - pc(A X); AX and T are n x k workspaces (leading dimension n)
static void error_propagate(CsrOp &A, LinOp &pc, double *X, int64_t ld, int64_t k, double *AX, double *T, double *out,
                            hipStream_t s) {
    const int64_t n = A.nrows;
    spmm(A.m, X, ld, AX, n, k, s);
    if (auto *D = dynamic_cast<DiagOp *>(&pc)) {
        block_update(X, ld, AX, n, D->d.get(), n, k, out, n, s);
        return;
    }
    pc.apply_block(T, n, AX, n, k);  // multigrid / composite: the block cycle; else column by column
    block_update(X, ld, T, n, nullptr, n, k, out, n, s);
}

static void check_block(const CsrOp &A, const double *X, int64_t ld, int64_t k) {
    FAMG_REQUIRE(A.nrows == A.ncols, AMG_ERR_DIM, "near-null search: the matrix must be square");
    FAMG_REQUIRE(X, AMG_ERR_INVALID, "near-null search: null block");
    FAMG_REQUIRE(k >= 1, AMG_ERR_INVALID, "near-null search: need at least one column");
    FAMG_REQUIRE(k <= QR_MAX_K, AMG_ERR_UNSUPPORTED, "near-null search: at most 64 columns");
    FAMG_REQUIRE(A.nrows >= k, AMG_ERR_DIM, "near-null search: more columns than rows");
    FAMG_REQUIRE(ld >= A.nrows, AMG_ERR_INVALID, "near-null search: leading dimension < n");
}

void smooth_vectors(CsrOp &A, LinOp &pc, double *X, int64_t ld, int64_t k, int64_t iters, double *cfs) {
    check_block(A, X, ld, k);
    FAMG_REQUIRE(iters >= 0, AMG_ERR_INVALID, "smooth_vectors: negative iteration count");
    FAMG_REQUIRE(pc.nrows == A.nrows && pc.ncols == A.nrows, AMG_ERR_DIM, "smooth_vectors: preconditioner size");
    FAMG_REQUIRE(pc.ctx == A.ctx, AMG_ERR_INVALID, "smooth_vectors: operands on different contexts");
    Ctx &ctx = *A.ctx;
    hipStream_t s = ctx.stream;
    const int64_t n = A.nrows;
    NearNullWork w;
    w.reserve(ctx, n, k);
    const bool diag = dynamic_cast<DiagOp *>(&pc) != nullptr;
    DevBuf<double> AX(n * k), T(diag && !cfs ? 1 : n * k), EV(cfs ? n * k : 1);
    thin_qr_work(ctx, X, ld, n, k, nullptr, w);  // adaptivity.rs:329
    thin_qr_work(ctx, X, ld, n, k, nullptr, w);  // :349
    for (int64_t it = 0; it < iters; it++) {     // :351-354
        error_propagate(A, pc, X, ld, k, AX.get(), T.get(), nullptr, s);
        thin_qr_work(ctx, X, ld, n, k, nullptr, w);
    }
    if (!cfs) return;
    // :367-382  cf = sqrt(ev^T A ev) / sqrt(w^T A w), ev = w - pc(A w)
    error_propagate(A, pc, X, ld, k, AX.get(), T.get(), EV.get(), s);
    coldot(X, ld, AX.get(), n, n, k, w.dots.get(), w, s);  // w^T A w
    spmm(A.m, EV.get(), n, T.get(), n, k, s);
    coldot(EV.get(), n, T.get(), n, n, k, w.dots.get() + k, w, s);  // ev^T A ev
    std::vector<double> h(2 * k);
    FAMG_CHECK_HIP(hipMemcpyAsync(h.data(), w.dots.get(), 2 * k * sizeof(double), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    for (int64_t c = 0; c < k; c++) cfs[c] = std::sqrt(h[k + c]) / std::sqrt(h[c]);
}

void create_weights(CsrOp &A, const double *X, int64_t ld, int64_t k, double *wout) {
    check_block(A, X, ld, k);
    FAMG_REQUIRE(wout, AMG_ERR_INVALID, "create_weights: null output");
    Ctx &ctx = *A.ctx;
    hipStream_t s = ctx.stream;
    const int64_t n = A.nrows;
    NearNullWork w;
    w.dots.resize(k);
    w.dot_partials.resize(k * COLDOT_GRID);
    DevBuf<double> AX(n * k);
    spmm(A.m, X, ld, AX.get(), n, k, s);
    coldot(X, ld, AX.get(), n, n, k, w.dots.get(), w, s);
    std::vector<double> h(k);
    FAMG_CHECK_HIP(hipMemcpyAsync(h.data(), w.dots.get(), k * sizeof(double), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    for (int64_t c = 0; c < k; c++) {
        FAMG_REQUIRE(h[c] > 0.0, AMG_ERR_NOT_SPD, "create_weights: a column with x^T A x <= 0");
        wout[c] = 1.0 / h[c];
    }
}

void find_near_null(const CsrPtr &A, double *X, int64_t ld, int64_t k, int64_t iters, int64_t block_size,
                    int64_t strength_depth, double *cfs) {
    check_block(*A, X, ld, k);
    FAMG_REQUIRE(block_size >= 1 && A->nrows % block_size == 0, AMG_ERR_DIM,
                 "find_near_null: block size must divide n");
    FAMG_REQUIRE(strength_depth >= 1, AMG_ERR_INVALID, "find_near_null: strength depth must be >= 1");
    Ctx &ctx = *A->ctx;
    hipStream_t s = ctx.stream;
    const int64_t n = A->nrows;
    // stage 1 (adaptivity.rs:270-277): L1 on a copy of the start block
    DevBuf<double> B(n * k);
    FAMG_CHECK_HIP(hipMemcpy2DAsync(B.get(), n * sizeof(double), X, ld * sizeof(double), n * sizeof(double), k,
                                    hipMemcpyDeviceToDevice, s));
    auto l1 = make_l1(*A);
    smooth_vectors(*A, *l1, B.get(), n, k, iters, nullptr);
    // :288-289 weights, strength graph, aggregates (MIS, or the modularity partitioner by policy), BlockSmoother
    std::vector<double> wts(k);
    create_weights(*A, B.get(), n, k, wts.data());
    std::vector<int64_t> agg;
    int64_t na = 0;
    // amg_set_sa_setup(1): the basis stays on the device (sagraph.hip); a null graph
    // (a ball beyond the cap, the byte budget, the index range) takes the host path
    CsrPtr Gd;
    if (g_sa_setup == 1)
        Gd = strength_graph_device(*A, B.get(), n, k, wts.data(), block_size, strength_depth, 0, nullptr, true);
    if (Gd) {
        B.release();
        na = g_sa_partitioner == 1 ? partition_modularity_device(Gd->m, g_sa_part_cfg, agg, nullptr)
                                   : aggregate_mis_device(Gd->m, 0, agg, nullptr);
        Gd.reset();
    } else {
        std::vector<double> basis(n * k);
        FAMG_CHECK_HIP(hipMemcpyAsync(basis.data(), B.get(), n * k * sizeof(double), hipMemcpyDeviceToHost, s));
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
        B.release();
        StrengthGraph G = strength_graph(*A, basis.data(), n, k, wts.data(), strength_depth, block_size);
        na = g_sa_partitioner == 1 ? partition_modularity(G, g_sa_part_cfg, agg, nullptr) : aggregate_mis(G, agg);
    }
    auto blk = make_block_smoother(*A, agg.data(), na, block_size);
    // stage 2 (:290-296) from the caller's start block
    smooth_vectors(*A, *blk, X, ld, k, iters, cfs);
}

}  // namespace famg
