// pcg.hip -- the k-wide vector kernels of the block solve drivers
// (pcg_block_impl / stationary_block_impl, solve.cpp).
//
// A workspace block is column-major with one column per active slot; the
// caller's X is reached through a device array mapping slot -> caller column.
// Every kernel computes a column exactly as the single-vector kernel of
// blas1.hip computes that vector: the dots keep k_dot_partial's element-to-thread
// map, fma chain and block_sum, the updates the unfused multiply-then-add that
// k_axpy / k_xpay compile to under -ffp-contract=off.  Columns may be only 8-byte
// aligned (odd leading dimensions), so every access is one double per lane:
// consecutive lanes touch consecutive doubles, 512 B per wave access.
#include <algorithm>

#include "block_sum.hpp"
#include "famg.hpp"

namespace famg {

constexpr int CG_GRID = VEC_DOT_PARTIALS;  // row blocks of a column dot, as vec_dot
constexpr int CG_BS = 256;

// partials[c][b] = block b's share of x_c . y_c: column blockIdx.y, row block
// blockIdx.x; the element map of k_dot_partial (stride CG_GRID * 256)
__global__ __launch_bounds__(CG_BS) void k_cg_dot(const double *x, int64_t ldx, const double *y, int64_t ldy,
                                                  int64_t n, double *partials) {
    __shared__ double sh[4];
    const int64_t c = blockIdx.y;
    const double *xc = x + c * ldx, *yc = y + c * ldy;
    double acc = 0.0;
    const int64_t stride = (int64_t)CG_GRID * CG_BS;
    for (int64_t i = (int64_t)blockIdx.x * CG_BS + threadIdx.x; i < n; i += stride) acc = fma(xc[i], yc[i], acc);
    const double t = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[c * CG_GRID + blockIdx.x] = t;
}

// k_dot_final's sum of column blockIdx.x, then the scalar step of that column in
// IEEE double -- the divisions pcg_impl does on the host
//   OP 0: a[c] = b[c] / t            (alpha = rz / pAp)
//   OP 1: a[c] = t                   (the value itself: r.r, b.b, the first r.z)
//   OP 2: a[c] = t / b[c]; b[c] = t  (beta = rz_new / rz; rz = rz_new)
template <int OP>
__global__ __launch_bounds__(CG_BS) void k_cg_final(const double *partials, double *a, double *b) {
    __shared__ double sh[4];
    const int64_t c = blockIdx.x;
    const double *pc = partials + c * CG_GRID;
    double acc = 0.0;
    for (int i = threadIdx.x; i < CG_GRID; i += CG_BS) acc += pc[i];
    const double t = block_sum(acc, sh);
    if (threadIdx.x == 0) {
        if constexpr (OP == 0) {
            a[c] = b[c] / t;
        } else if constexpr (OP == 1) {
            a[c] = t;
        } else {
            a[c] = t / b[c];
            b[c] = t;
        }
    }
}

// x_c = x_c + alpha_c p_c (the caller's column map[c]); r_c = r_c + (-alpha_c) Ap_c;
// partials of the new r_c . r_c.  A thread owns, in k_cg_dot's order, exactly the
// elements it updated, so the partials are those of the separate dot.
__global__ __launch_bounds__(CG_BS) void k_cg_update(double *X, int64_t ldx, const int32_t *map, const double *P,
                                                     const double *AP, double *R, int64_t ldw, const double *alpha,
                                                     int64_t n, double *partials) {
    __shared__ double sh[4];
    const int64_t c = blockIdx.y;
    const double al = alpha[c], nal = -al;
    double *xc = X + (int64_t)map[c] * ldx, *rc = R + c * ldw;
    const double *pc = P + c * ldw, *apc = AP + c * ldw;
    double acc = 0.0;
    const int64_t stride = (int64_t)CG_GRID * CG_BS;
    for (int64_t i = (int64_t)blockIdx.x * CG_BS + threadIdx.x; i < n; i += stride) {
        xc[i] = xc[i] + al * pc[i];
        const double rn = rc[i] + nal * apc[i];
        rc[i] = rn;
        acc = fma(rn, rn, acc);
    }
    const double t = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[c * CG_GRID + blockIdx.x] = t;
}

// p_c = z_c + beta_c p_c
__global__ __launch_bounds__(CG_BS) void k_cg_xpay(double *P, int64_t ldp, const double *Z, int64_t ldz,
                                                   const double *beta, int64_t n) {
    const int64_t c = blockIdx.y;
    const double be = beta[c];
    double *pc = P + c * ldp;
    const double *zc = Z + c * ldz;
    const int64_t stride = (int64_t)gridDim.x * CG_BS;
    for (int64_t i = (int64_t)blockIdx.x * CG_BS + threadIdx.x; i < n; i += stride) pc[i] = zc[i] + be * pc[i];
}

// x_c = x_c + z_c on the caller's column map[c] (the stationary sweep's update)
__global__ __launch_bounds__(CG_BS) void k_cg_add(double *X, int64_t ldx, const int32_t *map, const double *Z,
                                                  int64_t ldz, int64_t n) {
    const int64_t c = blockIdx.y;
    double *xc = X + (int64_t)map[c] * ldx;
    const double *zc = Z + c * ldz;
    const int64_t stride = (int64_t)gridDim.x * CG_BS;
    for (int64_t i = (int64_t)blockIdx.x * CG_BS + threadIdx.x; i < n; i += stride) xc[i] = xc[i] + zc[i];
}

static inline unsigned cg_ew_grid(int64_t n) {
    return (unsigned)std::min<int64_t>(std::max<int64_t>(1, ceil_div(n, CG_BS)), 65536);
}

void cg_dot_cols(const double *x, int64_t ldx, const double *y, int64_t ldy, int64_t n, int64_t k, double *partials,
                 hipStream_t s) {
    if (k <= 0) return;
    log_launch("cg_dot", -1, -1, n, 16 * n * k);
    hipLaunchKernelGGL(k_cg_dot, dim3(CG_GRID, (unsigned)k), dim3(CG_BS), 0, s, x, ldx, y, ldy, n, partials);
    FAMG_CHECK_HIP(hipGetLastError());
}

void cg_final_cols(CgFinal op, const double *partials, double *a, double *b, int64_t k, hipStream_t s) {
    if (k <= 0) return;
    const dim3 grid((unsigned)k), block(CG_BS);
    switch (op) {
    case CG_FINAL_ALPHA: hipLaunchKernelGGL(k_cg_final<0>, grid, block, 0, s, partials, a, b); break;
    case CG_FINAL_STORE: hipLaunchKernelGGL(k_cg_final<1>, grid, block, 0, s, partials, a, b); break;
    case CG_FINAL_BETA: hipLaunchKernelGGL(k_cg_final<2>, grid, block, 0, s, partials, a, b); break;
    }
    FAMG_CHECK_HIP(hipGetLastError());
}

void cg_update_cols(double *X, int64_t ldx, const int32_t *map, const double *P, const double *AP, double *R,
                    int64_t ldw, const double *alpha, int64_t n, int64_t k, double *partials, hipStream_t s) {
    if (k <= 0) return;
    log_launch("cg_update", -1, -1, n, 48 * n * k);
    hipLaunchKernelGGL(k_cg_update, dim3(CG_GRID, (unsigned)k), dim3(CG_BS), 0, s, X, ldx, map, P, AP, R, ldw, alpha, n,
                       partials);
    FAMG_CHECK_HIP(hipGetLastError());
}

void cg_xpay_cols(double *P, int64_t ldp, const double *Z, int64_t ldz, const double *beta, int64_t n, int64_t k,
                  hipStream_t s) {
    if (k <= 0 || n <= 0) return;
    log_launch("cg_xpay", -1, -1, n, 24 * n * k);
    hipLaunchKernelGGL(k_cg_xpay, dim3(cg_ew_grid(n), (unsigned)k), dim3(CG_BS), 0, s, P, ldp, Z, ldz, beta, n);
    FAMG_CHECK_HIP(hipGetLastError());
}

void cg_add_cols(double *X, int64_t ldx, const int32_t *map, const double *Z, int64_t ldz, int64_t n, int64_t k,
                 hipStream_t s) {
    if (k <= 0 || n <= 0) return;
    log_launch("cg_add", -1, -1, n, 24 * n * k);
    hipLaunchKernelGGL(k_cg_add, dim3(cg_ew_grid(n), (unsigned)k), dim3(CG_BS), 0, s, X, ldx, map, Z, ldz, n);
    FAMG_CHECK_HIP(hipGetLastError());
}

}  // namespace famg
