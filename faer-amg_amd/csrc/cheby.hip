// cheby.hip -- Chebyshev polynomial smoother (a new definition,
// like SGS: the reference has no such smoother).
//
// z = S b is `steps` terms of the Chebyshev iteration on D^-1 A over the interval
// [lambda_max / eig_ratio, lambda_max], from z = 0: products with A (the existing
// SPMV_RESID launches) and one fused element-wise pass per term.  The pass is
// k-wide from the start -- the single-vector apply is k = 1 of the same kernel --
// so every column of a block apply is bitwise the single apply of that column.
// Setup estimates lambda_max on the device: the row-sum bound G and the largest
// Ritz value of a few Lanczos steps on D^-1 A in the D inner product.
#include <algorithm>
#include <cmath>

#include "famg.hpp"

namespace famg {

typedef double cheby_dbl2 __attribute__((ext_vector_type(2)));

constexpr int CH_BS = 256;
constexpr int CH_MAX_BLOCKS = 2048;  // 8 workgroups per CU; longer columns grid-stride

// d = c2_0 (dinv b)
template <typename T> __device__ __forceinline__ T cheby_d0(T di, T b, double c2) {
    const T t = di * b;
    return c2 * t;
}
// d = c1 d + c2 (dinv r)
template <typename T> __device__ __forceinline__ T cheby_dk(T di, T r, T d, double c1, double c2) {
    const T t = di * r;
    return (c1 * d) + (c2 * t);
}

// first term over grid (row blocks, columns): d = c2_0 dinv b, x = d.  VEC: 16-B
// accesses (every column base 16-B aligned), the odd last row by one lane.
// M1 (steps == 1): only x is stored.
template <bool VEC, bool M1>
__global__ __launch_bounds__(CH_BS) void k_cheby_first(const double *__restrict__ dinv, const double *__restrict__ B,
                                                       int64_t ldb, double *__restrict__ D, int64_t ldd,
                                                       double *__restrict__ X, int64_t ldx, double c2, int64_t n) {
    const int64_t c = blockIdx.y;
    const double *b = B + c * ldb;
    double *x = X + c * ldx;
    double *d = M1 ? nullptr : D + c * ldd;
    const int64_t stride = (int64_t)gridDim.x * CH_BS;
    const int64_t i0 = (int64_t)blockIdx.x * CH_BS + threadIdx.x;
    if constexpr (VEC) {
        const int64_t n2 = n >> 1;
        for (int64_t i = i0; i < n2; i += stride) {
            const cheby_dbl2 dn = cheby_d0(reinterpret_cast<const cheby_dbl2 *>(dinv)[i],
                                           reinterpret_cast<const cheby_dbl2 *>(b)[i], c2);
            if constexpr (!M1) reinterpret_cast<cheby_dbl2 *>(d)[i] = dn;
            reinterpret_cast<cheby_dbl2 *>(x)[i] = dn;
        }
        if ((n & 1) && i0 == 0) {
            const double dn = cheby_d0(dinv[n - 1], b[n - 1], c2);
            if constexpr (!M1) d[n - 1] = dn;
            x[n - 1] = dn;
        }
    } else {
        for (int64_t i = i0; i < n; i += stride) {
            const double dn = cheby_d0(dinv[i], b[i], c2);
            if constexpr (!M1) d[i] = dn;
            x[i] = dn;
        }
    }
}

// term k >= 1: d = c1 d + c2 dinv r, x += d.  LAST: d is not stored.
template <bool VEC, bool LAST>
__global__ __launch_bounds__(CH_BS) void k_cheby_step(const double *__restrict__ dinv, const double *__restrict__ R,
                                                      int64_t ldr, double *__restrict__ D, int64_t ldd,
                                                      double *__restrict__ X, int64_t ldx, double c1, double c2,
                                                      int64_t n) {
    const int64_t c = blockIdx.y;
    const double *r = R + c * ldr;
    double *d = D + c * ldd;
    double *x = X + c * ldx;
    const int64_t stride = (int64_t)gridDim.x * CH_BS;
    const int64_t i0 = (int64_t)blockIdx.x * CH_BS + threadIdx.x;
    if constexpr (VEC) {
        const int64_t n2 = n >> 1;
        for (int64_t i = i0; i < n2; i += stride) {
            const cheby_dbl2 dn = cheby_dk(reinterpret_cast<const cheby_dbl2 *>(dinv)[i],
                                           reinterpret_cast<const cheby_dbl2 *>(r)[i],
                                           reinterpret_cast<const cheby_dbl2 *>(d)[i], c1, c2);
            if constexpr (!LAST) reinterpret_cast<cheby_dbl2 *>(d)[i] = dn;
            reinterpret_cast<cheby_dbl2 *>(x)[i] = reinterpret_cast<const cheby_dbl2 *>(x)[i] + dn;
        }
        if ((n & 1) && i0 == 0) {
            const double dn = cheby_dk(dinv[n - 1], r[n - 1], d[n - 1], c1, c2);
            if constexpr (!LAST) d[n - 1] = dn;
            x[n - 1] = x[n - 1] + dn;
        }
    } else {
        for (int64_t i = i0; i < n; i += stride) {
            const double dn = cheby_dk(dinv[i], r[i], d[i], c1, c2);
            if constexpr (!LAST) d[i] = dn;
            x[i] = x[i] + dn;
        }
    }
}

// every one of the k column bases p + c * ld is 16-B aligned
static bool cols_aligned16(const void *p, int64_t ld, int64_t k) {
    return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (k == 1 || (ld & 1) == 0);
}
static dim3 cheby_grid(int64_t n, bool vec, int64_t k) {
    const int64_t work = vec ? n / 2 : n;
    return dim3((unsigned)std::min<int64_t>(CH_MAX_BLOCKS, std::max<int64_t>(1, ceil_div(work, CH_BS))), (unsigned)k);
}

static void cheby_first(const double *dinv, const double *B, int64_t ldb, double *D, int64_t ldd, double *X,
                        int64_t ldx, double c2, bool m1, int64_t n, int64_t k, hipStream_t s) {
    log_launch("cheby_first", -1, -1, n, 8 * n + (m1 ? 16 : 24) * n * k);
    const bool vec = n >= 2 && cols_aligned16(B, ldb, k) && cols_aligned16(X, ldx, k) && (m1 || cols_aligned16(D, ldd, k));
    const dim3 grid = cheby_grid(n, vec, k), block(CH_BS);
#define FAMG_CHEBY_FIRST(V, M) \
    hipLaunchKernelGGL((k_cheby_first<V, M>), grid, block, 0, s, dinv, B, ldb, D, ldd, X, ldx, c2, n)
    if (vec && m1) FAMG_CHEBY_FIRST(true, true);
    else if (vec) FAMG_CHEBY_FIRST(true, false);
    else if (m1) FAMG_CHEBY_FIRST(false, true);
    else FAMG_CHEBY_FIRST(false, false);
#undef FAMG_CHEBY_FIRST
    FAMG_CHECK_HIP(hipGetLastError());
}

static void cheby_step(const double *dinv, const double *R, int64_t ldr, double *D, int64_t ldd, double *X,
                       int64_t ldx, double c1, double c2, bool last, int64_t n, int64_t k, hipStream_t s) {
    log_launch("cheby_step", -1, -1, n, 8 * n + (last ? 32 : 40) * n * k);
    const bool vec = n >= 2 && cols_aligned16(R, ldr, k) && cols_aligned16(X, ldx, k) && cols_aligned16(D, ldd, k);
    const dim3 grid = cheby_grid(n, vec, k), block(CH_BS);
#define FAMG_CHEBY_STEP(V, L) \
    hipLaunchKernelGGL((k_cheby_step<V, L>), grid, block, 0, s, dinv, R, ldr, D, ldd, X, ldx, c1, c2, n)
    if (vec && last) FAMG_CHEBY_STEP(true, true);
    else if (vec) FAMG_CHEBY_STEP(true, false);
    else if (last) FAMG_CHEBY_STEP(false, true);
    else FAMG_CHEBY_STEP(false, false);
#undef FAMG_CHEBY_STEP
    FAMG_CHECK_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ apply

// X = S B over kw columns on the workspaces R0 / R1 / D (leading dimension ldw);
// single: the products through spmv (apply), else through spmm_epi (apply_block)
void ChebyOp::run(double *X, int64_t ldx, const double *B, int64_t ldb, int64_t kw, double *R0, double *R1, double *D,
                  int64_t ldw, bool single) {
    hipStream_t s = ctx->stream;
    const int64_t n = nrows;
    if (n <= 0 || kw <= 0) return;
    cheby_first(dinv.get(), B, ldb, D, ldw, X, ldx, c2[0], steps == 1, n, kw, s);
    const double *r = B;  // r = b: never copied
    int64_t ldr = ldb;
    double *nxt = R0;
    for (int64_t k = 1; k < steps; k++) {
        if (single) {
            SpmvEpi epi;
            epi.b = r;
            spmv(A->m, D, nxt, SPMV_RESID, epi, s);  // r' = r - A d
        } else {
            spmm_epi(A->m, D, ldw, nxt, ldw, kw, SPMV_RESID, SpmmEpi{r, ldr, nullptr}, s);
        }
        cheby_step(dinv.get(), nxt, ldw, D, ldw, X, ldx, c1[k], c2[k], k == steps - 1, n, kw, s);
        r = nxt;
        ldr = ldw;
        nxt = nxt == R0 ? R1 : R0;
    }
}

void ChebyOp::apply(double *out, const double *rhs) {
    if (out == rhs) {
        LinOp::apply_in_place(out);
        return;
    }
    run(out, nrows, rhs, nrows, 1, r0_.get(), r1_.get(), d_.get(), nrows, true);
}

void ChebyOp::apply_block(double *out, int64_t ldo, const double *rhs, int64_t ldr, int64_t k) {
    if (out == rhs) {
        LinOp::apply_block(out, ldo, rhs, ldr, k);
        return;
    }
    if (k <= 0 || nrows <= 0) return;
    const int64_t kmax = std::min<int64_t>(k, MG_BLOCK_COLS);
    const int64_t ldw = (nrows + 1) & ~int64_t(1);  // even: every workspace column 16-B aligned
    const size_t sz = (size_t)ldw * kmax;
    if (steps > 1 && bd_.size() < sz) {  // grown on demand, as MgLevel::bv
        bd_.resize(sz);
        br0_.resize(sz);
        if (steps > 2) br1_.resize(sz);
    }
    for (int64_t c0 = 0; c0 < k; c0 += MG_BLOCK_COLS)
        run(out + c0 * ldo, ldo, rhs + c0 * ldr, ldr, std::min<int64_t>(MG_BLOCK_COLS, k - c0), br0_.get(), br1_.get(),
            bd_.get(), ldw, false);
}

// ------------------------------------------------------------------ setup

constexpr int CH_RED = 256;  // workgroups of the setup reduction

// dinv = 1 / a_ii; part[b] = max over block b's rows of rowsum_i / a_ii (rowsum may
// be null: 0), part[CH_RED + b] = their smallest a_ii, 0 once one is not > 0
__global__ __launch_bounds__(256) void k_cheby_diag(const double *aii, const double *rowsum, int64_t n, double *dinv,
                                                    double *part) {
    __shared__ double smax[256], smin[256];
    double gmax = 0.0, amin = INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)CH_RED * 256) {
        const double a = aii[i];
        dinv[i] = 1.0 / a;
        if (!(a > 0.0)) amin = 0.0;
        else amin = fmin(amin, a);
        if (rowsum) gmax = fmax(gmax, rowsum[i] / a);
    }
    smax[threadIdx.x] = gmax;
    smin[threadIdx.x] = amin;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + off]);
            smin[threadIdx.x] = fmin(smin[threadIdx.x], smin[threadIdx.x + off]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[blockIdx.x] = smax[0];
        part[CH_RED + blockIdx.x] = smin[0];
    }
}

// the Lanczos start vector: q_i = ((i * 2654435761) mod 2^32) / 2^32 - 0.5 (exact in fp64)
__global__ void k_cheby_start(double *q, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = (uint32_t)((uint64_t)i * 2654435761ull);
    q[i] = (double)h / 4294967296.0 - 0.5;
}

// largest eigenvalue of the symmetric tridiagonal (a, b: b[j] couples j and j + 1) by
// bisection on the Sturm count
static double tridiag_max_eig(const std::vector<double> &a, const std::vector<double> &b) {
    const int m = (int)a.size();
    double lo = a[0], hi = a[0];
    for (int j = 0; j < m; j++) {
        const double rad = (j > 0 ? std::fabs(b[j - 1]) : 0.0) + (j + 1 < m ? std::fabs(b[j]) : 0.0);
        lo = std::min(lo, a[j] - rad);
        hi = std::max(hi, a[j] + rad);
    }
    auto below = [&](double x) {  // eigenvalues < x
        int cnt = 0;
        double d = 1.0;
        for (int j = 0; j < m; j++) {
            d = (a[j] - x) - (j > 0 ? b[j - 1] * b[j - 1] / d : 0.0);
            if (d == 0.0) d = -1e-300;
            cnt += d < 0.0;
        }
        return cnt;
    };
    hi = hi + 1e-15 * std::fabs(hi) + 1e-300;  // every eigenvalue below hi
    for (int it = 0; it < 200; it++) {
        const double mid = 0.5 * (lo + hi);
        if (!(mid > lo && mid < hi)) break;
        if (below(mid) == m) hi = mid;
        else lo = mid;
    }
    return 0.5 * (lo + hi);
}

// `iters` Lanczos steps on D^-1 A in the D inner product (self-adjoint there), from
// the fixed start vector; returns the largest Ritz value, *run = steps taken
static double cheby_lanczos(CsrOp &A, const double *dinv, int64_t iters, int64_t *run) {
    Ctx &ctx = *A.ctx;
    hipStream_t s = ctx.stream;
    const int64_t n = A.nrows;
    const double *aii = A.diagonal();
    DevBuf<double> bq(n), bp(n), bw(n), bu(n);
    double *q = bq.get(), *qp = bp.get(), *w = bw.get(), *u = bu.get();
    hipLaunchKernelGGL(k_cheby_start, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, q, n);
    FAMG_CHECK_HIP(hipGetLastError());
    vec_mul(u, aii, q, n, s);
    const double nrm0 = std::sqrt(vec_dot(q, u, n, ctx));
    FAMG_REQUIRE(nrm0 > 0.0 && std::isfinite(nrm0), AMG_ERR_NOT_SPD, "chebyshev: the start vector has no D-norm");
    vec_scale(q, 1.0 / nrm0, n, s);
    std::vector<double> al, be;
    double beta = 0.0;
    for (int64_t j = 0; j < iters; j++) {
        spmv(A.m, q, w, SPMV_SET, SpmvEpi{}, s);
        const double alpha = vec_dot(q, w, n, ctx);  // <D^-1 A q, q>_D
        FAMG_REQUIRE(std::isfinite(alpha), AMG_ERR_INVALID, "chebyshev: the eigenvalue estimate is not finite");
        al.push_back(alpha);
        if (j + 1 == iters) break;
        vec_mul(w, dinv, w, n, s);
        vec_axpy(w, -alpha, q, n, s);
        if (j > 0) vec_axpy(w, -beta, qp, n, s);
        vec_mul(u, aii, w, n, s);
        beta = std::sqrt(vec_dot(w, u, n, ctx));
        if (!(beta > 1e-13 * std::fabs(alpha))) break;  // an invariant subspace: the Ritz values are exact
        be.push_back(beta);
        vec_scale(w, 1.0 / beta, n, s);
        std::swap(qp, q);
        std::swap(q, w);
    }
    *run = (int64_t)al.size();
    be.resize(al.size() - 1);
    return tridiag_max_eig(al, be);
}

void chebyshev_check(const ChebyConfig &cfg) {
    FAMG_REQUIRE(cfg.steps >= 1, AMG_ERR_INVALID, "chebyshev: steps must be >= 1");
    FAMG_REQUIRE(cfg.eig_iters >= 0 && cfg.eig_iters <= 64, AMG_ERR_INVALID, "chebyshev: eig_iters must be 0..64");
    FAMG_REQUIRE(cfg.eig_ratio > 1.0 && std::isfinite(cfg.eig_ratio), AMG_ERR_INVALID, "chebyshev: eig_ratio must be > 1");
    FAMG_REQUIRE(cfg.boost >= 1.0 && std::isfinite(cfg.boost), AMG_ERR_INVALID, "chebyshev: boost must be >= 1");
    FAMG_REQUIRE(cfg.lambda_max >= 0.0 && std::isfinite(cfg.lambda_max), AMG_ERR_INVALID,
                 "chebyshev: lambda_max must be >= 0");
}

std::shared_ptr<ChebyOp> make_chebyshev(const CsrPtr &A, const ChebyConfig &cfg) {
    chebyshev_check(cfg);
    FAMG_REQUIRE(A->nrows == A->ncols, AMG_ERR_DIM, "chebyshev: matrix must be square");
    const int64_t n = A->nrows;
    FAMG_REQUIRE(n >= 1, AMG_ERR_INVALID, "chebyshev: empty matrix");
    Ctx *ctx = A->ctx;
    hipStream_t s = ctx->stream;
    auto op = std::make_shared<ChebyOp>();
    op->ctx = ctx;
    op->A = A;
    op->nrows = op->ncols = n;
    op->steps = cfg.steps;
    const double *aii = nullptr;
    try {
        aii = A->diagonal();
    } catch (const AmgError &e) {  // a missing diagonal entry is a zero one
        fail(e.status == AMG_ERR_INVALID ? AMG_ERR_NOT_SPD : e.status, std::string("chebyshev: ") + e.what());
    }
    const bool given = cfg.lambda_max > 0.0;
    DevBuf<double> rowsum, part(2 * CH_RED);
    if (!given) {
        rowsum.resize(n);
        csr_abs_row_sums(A->m, rowsum.get());
    }
    op->dinv.resize(n);
    hipLaunchKernelGGL(k_cheby_diag, dim3(CH_RED), dim3(256), 0, s, aii, given ? nullptr : rowsum.get(), n,
                       op->dinv.get(), part.get());
    FAMG_CHECK_HIP(hipGetLastError());
    std::vector<double> hp(2 * CH_RED);
    FAMG_CHECK_HIP(hipMemcpyAsync(hp.data(), part.get(), hp.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    double G = 0.0, amin = INFINITY;
    for (int b = 0; b < CH_RED; b++) {
        G = std::max(G, hp[b]);
        amin = std::min(amin, hp[CH_RED + b]);
    }
    FAMG_REQUIRE(amin > 0.0, AMG_ERR_NOT_SPD, "chebyshev: a diagonal entry is not positive");
    if (given) {
        op->lambda_max = cfg.lambda_max;
    } else {
        FAMG_REQUIRE(G > 0.0 && std::isfinite(G), AMG_ERR_INVALID, "chebyshev: the row-sum bound is not finite");
        op->row_bound = G;
        op->lambda_max = G;
        if (cfg.eig_iters > 0) {
            op->ritz = cheby_lanczos(*A, op->dinv.get(), cfg.eig_iters, &op->eig_run);
            FAMG_REQUIRE(op->ritz > 0.0, AMG_ERR_NOT_SPD, "chebyshev: the largest Ritz value of D^-1 A is not positive");
            op->lambda_max = std::min(cfg.boost * op->ritz, G);
        }
    }
    op->lambda_min = op->lambda_max / cfg.eig_ratio;
    // the coefficients, once, in double (these expressions in this order)
    const double theta = (op->lambda_max + op->lambda_min) / 2.0;
    const double delta = (op->lambda_max - op->lambda_min) / 2.0;
    const double sigma = theta / delta;
    double rho = 1.0 / sigma;
    op->c1.assign(cfg.steps, 0.0);
    op->c2.assign(cfg.steps, 0.0);
    op->c2[0] = 1.0 / theta;
    for (int64_t k = 1; k < cfg.steps; k++) {
        const double rk = 1.0 / (2.0 * sigma - rho);
        op->c1[k] = rk * rho;
        op->c2[k] = 2.0 * rk / delta;
        rho = rk;
    }
    if (cfg.steps > 1) {  // apply() never allocates: it is captured in the cycle's graph
        op->d_.resize(n);
        op->r0_.resize(n);
        if (cfg.steps > 2) op->r1_.resize(n);
    }
    return op;
}

}  // namespace famg
