// bcg.hip -- the tall-skinny kernels of the coupled block CG (block_cg_impl,
// solve.cpp): the rectangular Gram product C = X^T [Y1 | Y2] and the
// row-per-lane update OUT = Y +- X C that serves X += P alpha, R -= Q alpha and
// P <- Z - P beta.
//
// The Gram kernel is nearnull.hip's k_gram_partial recipe on
// v_mfma_f64_16x16x4_f64 -- 64 rows staged through LDS per step with the next
// step's loads in flight, the waves and then the workgroups summed in a fixed
// order by a second launch, no atomics -- with two differences: the operands
// come from different blocks (X on one side, the columns of Y1 then Y2 on the
// other) and every 16 x 16 tile of the rectangular result is computed.  The update
// gives every lane one row of X, held in registers (templated on w rounded up to
// 8, as k_qr_update holds its row), and reads the coefficients at lane-independent
// addresses, i.e. through scalar loads.  Columns may be only 8-byte aligned (odd
// leading dimensions), so every global access is one double per lane.  Every
// reduction has a fixed shape and order: two calls give equal bits.
#include <algorithm>

#include "famg.hpp"

namespace famg {

typedef double bcg_dbl4 __attribute__((ext_vector_type(4)));

constexpr int BCG_ROWS = 64;            // rows a workgroup stages per step (4 waves x 16)
constexpr int BCG_LDS = BCG_ROWS + 1;   // LDS column stride (conflict-free operand reads)

// partials[b] (16 NBX x 16 NBY, row-major) = X_b^T [Y1 | Y2]_b over rows
// [b * rows_per_block, (b + 1) * rows_per_block); rows past w, columns past m1 + m2: 0.
// MFMA operands (one fp64 per lane): A[i = lane & 15][kk = lane >> 4] = x(row kk, column
// 16 I + i), B the same of column block J of [Y1 | Y2]; D: column lane & 15, row
// (lane >> 4) + 4 reg.
template <int NBX, int NBY>
__global__ __launch_bounds__(256) void k_bcg_gram_partial(const double *X, int64_t ldx, int w, const double *Y1,
                                                          int64_t ld1, int m1, const double *Y2, int64_t ld2, int m2,
                                                          int64_t n, int64_t rows_per_block,
                                                          double *__restrict__ partials) {
    constexpr int KPX = 16 * NBX, KPY = 16 * NBY, KP = KPX + KPY;
    constexpr int NL = KP / 4;  // staging loads per thread and step: column 4 i + wave, row lane
    constexpr int NT = NBX * NBY;
    __shared__ double sh[KP * BCG_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r_begin = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r_end = r_begin + rows_per_block < n ? r_begin + rows_per_block : n;
    const int64_t steps = r_end > r_begin ? (r_end - r_begin + BCG_ROWS - 1) / BCG_ROWS : 0;
    double reg[NL];
    bcg_dbl4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = bcg_dbl4{0.0, 0.0, 0.0, 0.0};
    const int c = lane & 15, q = lane >> 4;
    for (int64_t st = 0; st <= steps; st++) {
        if (st > 0) {
            __syncthreads();  // the previous step's operand reads are done
#pragma unroll
            for (int i = 0; i < NL; i++) sh[(4 * i + wave) * BCG_LDS + lane] = reg[i];
            __syncthreads();
        }
        if (st < steps) {  // the next step's rows, in flight under this step's products
            const int64_t r = r_begin + st * BCG_ROWS + lane;
#pragma unroll
            for (int i = 0; i < NL; i++) {
                const int col = 4 * i + wave;  // [0, KPX): X; [KPX, KP): [Y1 | Y2]
                const int j = col - KPX;
                const double *src = col < KPX ? (col < w ? X + (int64_t)col * ldx : nullptr)
                                    : j < m1  ? Y1 + (int64_t)j * ld1
                                    : j < m1 + m2 ? Y2 + (int64_t)(j - m1) * ld2
                                                  : nullptr;
                reg[i] = (src && r < r_end) ? src[r] : 0.0;
            }
        }
        if (st > 0) {
#pragma unroll
            for (int s = 0; s < 4; s++) {
                double a[NBX], b[NBY];
#pragma unroll
                for (int I = 0; I < NBX; I++) a[I] = sh[(16 * I + c) * BCG_LDS + 16 * wave + 4 * s + q];
#pragma unroll
                for (int J = 0; J < NBY; J++) b[J] = sh[(KPX + 16 * J + c) * BCG_LDS + 16 * wave + 4 * s + q];
#pragma unroll
                for (int I = 0; I < NBX; I++)
#pragma unroll
                    for (int J = 0; J < NBY; J++)
                        acc[I * NBY + J] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[I], b[J], acc[I * NBY + J], 0, 0, 0);
            }
        }
    }
    // the four waves' tiles summed in wave order (sh reused: KPX * KPY <= KP * BCG_LDS)
    for (int wv = 0; wv < 4; wv++) {
        __syncthreads();
        if (wave == wv) {
#pragma unroll
            for (int I = 0; I < NBX; I++)
#pragma unroll
                for (int J = 0; J < NBY; J++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        double *p = &sh[(16 * I + q + 4 * r) * KPY + 16 * J + c];
                        *p = wv == 0 ? acc[I * NBY + J][r] : *p + acc[I * NBY + J][r];
                    }
        }
    }
    __syncthreads();
    double *out = partials + (int64_t)blockIdx.x * (KPX * KPY);
    for (int e = tid; e < KPX * KPY; e += 256) out[e] = sh[e];
}

// OUT_j = Y_j + sign * sum_i X_i C_ij for j < m: one row per lane, the row of X in
// registers (KB = w rounded up to 8; entries past w are 0), so OUT may be X itself
// (P <- Z - P beta) or Y (X += P alpha); C (KB x m column-major, rows past w zero)
// at the same address for every lane.  The sum is an fma chain over i = 0 .. KB - 1
// from 0 (explicit fma calls), added to or subtracted from y in one more rounding:
// under -ffp-contract=off that last operation is never fused into the chain.
template <int KB, int SIGN>
__global__ __launch_bounds__(256) void k_bcg_gemm(double *OUT, int64_t ldo, const double *Y, int64_t ldy,
                                                  const double *X, int64_t ldx, const double *__restrict__ C, int w,
                                                  int m, int64_t n) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    double x[KB];
#pragma unroll
    for (int i = 0; i < KB; i++) x[i] = i < w ? X[(int64_t)i * ldx + r] : 0.0;
    for (int j0 = 0; j0 < m; j0 += 4) {
        double y[4], s[4];
#pragma unroll
        for (int u = 0; u < 4; u++) y[u] = j0 + u < m ? Y[(int64_t)(j0 + u) * ldy + r] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            s[u] = 0.0;
            if (j0 + u < m) {
                const double *cj = C + (j0 + u) * KB;
#pragma unroll
                for (int i = 0; i < KB; i++) s[u] = fma(x[i], cj[i], s[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (j0 + u < m) OUT[(int64_t)(j0 + u) * ldo + r] = SIGN > 0 ? y[u] + s[u] : y[u] - s[u];
    }
}

void BcgWork::reserve(const Ctx &ctx, int64_t n) {
    const int64_t chunks = std::max<int64_t>(1, ceil_div(n, BCG_ROWS));
    const int64_t want = std::min<int64_t>(chunks, 4 * (int64_t)ctx.num_cus);
    rows_per_block = ceil_div(chunks, want) * BCG_ROWS;
    gram_blocks = std::max<int64_t>(1, ceil_div(n, rows_per_block));
    partials.resize((size_t)gram_blocks * BCG_MAX_W * 2 * BCG_MAX_W);
    G.resize(BCG_MAX_W * 2 * BCG_MAX_W);
}

int bcg_gram(const double *X, int64_t ldx, int64_t w, const double *Y1, int64_t ld1, int64_t m1, const double *Y2,
             int64_t ld2, int64_t m2, int64_t n, BcgWork &ws, double *hC, hipStream_t s) {
    const int nbx = (int)ceil_div(w, 16), nby = (int)ceil_div(m1 + m2, 16), kp2 = 256 * nbx * nby;
    const dim3 grid((unsigned)ws.gram_blocks), block(256);
    log_launch("bcg_gram", -1, -1, n, 8 * n * (w + m1 + m2));
#define FAMG_BCG_GRAM(NBX, NBY)                                                                                    \
    case 4 * NBX + NBY:                                                                                            \
        k_bcg_gram_partial<NBX, NBY><<<grid, block, 0, s>>>(X, ldx, (int)w, Y1, ld1, (int)m1, Y2, ld2, (int)m2, n, \
                                                            ws.rows_per_block, ws.partials.get());                 \
        break
    switch (4 * nbx + nby) {
        FAMG_BCG_GRAM(1, 1);
        FAMG_BCG_GRAM(1, 2);
        FAMG_BCG_GRAM(1, 3);
        FAMG_BCG_GRAM(1, 4);
        FAMG_BCG_GRAM(2, 1);
        FAMG_BCG_GRAM(2, 2);
        FAMG_BCG_GRAM(2, 3);
        FAMG_BCG_GRAM(2, 4);
    default: fail(AMG_ERR_UNSUPPORTED, "bcg_gram: more than 32 columns on a side");
    }
#undef FAMG_BCG_GRAM
    gram_final(ws.partials.get(), ws.gram_blocks, kp2, ws.G.get(), s);  // the workgroups' partials, in a fixed order
    FAMG_CHECK_HIP(hipGetLastError());
    FAMG_CHECK_HIP(hipMemcpyAsync(hC, ws.G.get(), (size_t)kp2 * sizeof(double), hipMemcpyDeviceToHost, s));
    return 16 * nby;
}

void bcg_pack_coef(const double *C, int64_t w, int64_t m, double *packed) {
    const int64_t kb = 8 * ceil_div(w, 8);
    for (int64_t j = 0; j < m; j++)
        for (int64_t i = 0; i < kb; i++) packed[j * kb + i] = i < w ? C[j * w + i] : 0.0;
}

void bcg_gemm(const char *name, double *OUT, int64_t ldo, const double *Y, int64_t ldy, const double *X, int64_t ldx,
              const double *Cd, int64_t w, int64_t m, int64_t n, int sign, hipStream_t s) {
    if (n <= 0 || m <= 0) return;
    const int kb = 8 * (int)ceil_div(w, 8);
    const dim3 grid((unsigned)ceil_div(n, 256)), block(256);
    log_launch(name, -1, -1, n, 8 * n * (2 * m + w));
#define FAMG_BCG_GEMM(KB)                                                                                           \
    case KB:                                                                                                        \
        if (sign > 0) k_bcg_gemm<KB, 1><<<grid, block, 0, s>>>(OUT, ldo, Y, ldy, X, ldx, Cd, (int)w, (int)m, n);     \
        else k_bcg_gemm<KB, -1><<<grid, block, 0, s>>>(OUT, ldo, Y, ldy, X, ldx, Cd, (int)w, (int)m, n);            \
        break
    switch (kb) {
        FAMG_BCG_GEMM(8);
        FAMG_BCG_GEMM(16);
        FAMG_BCG_GEMM(24);
        FAMG_BCG_GEMM(32);
    default: fail(AMG_ERR_UNSUPPORTED, "bcg_gemm: more than 32 columns of X");
    }
#undef FAMG_BCG_GEMM
    FAMG_CHECK_HIP(hipGetLastError());
}

}  // namespace famg
