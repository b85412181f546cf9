// spmm.hip -- multi-RHS SpMM Y = A X for the compressed storages (SURVEY.md
// 8(f) f2: the k-wide applies of near-null smoothing and the error propagator,
// adaptivity.rs:168-244,307-390, hierarchy.rs:219-226).
//
// The SELL-64 SpMM (sell.hip) covers fp64-valued SELL; here the storages the
// hierarchies actually use: DIA codes (constant-stencil operators, incl. the
// 33- and 27-diagonal run patterns), stencil classes (structured Galerkin
// levels) and 3x3 blocks (elasticity / C5).  Each kernel reads a row's matrix
// data once per group of up to 8 columns and, per column, sums exactly the
// terms the single-vector kernel of that storage sums, in the same order
// (ascending diagonals / offsets / block columns, fma from 0.0; the lanes-per-
// row class kernel with the same lane split and butterfly), so every column is
// bitwise the single-vector SpMV.  Column-major X, Y with leading dimensions.
//
// MODE fuses the V-cycle's epilogue at each kernel's store site (spmm_store,
// spmv_dev.hpp: Y += A X, Y = B - A X, Y = X + d (B - A X)) for the block cycle;
// the SET instantiations are the plain kernels.
#include <algorithm>
#include <type_traits>

#include "spmv_dev.hpp"

namespace famg {

constexpr int SPMM_COLS = 8;  // columns per launch

typedef double spmm_dbl2_t __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------ DIA codes

struct SpmmDiaArgs {
    const uint32_t *codes;
    const double *vtab;
    int32_t ntab, k, nrows, ncols;
    int32_t off[64];
    const double *x;
    int64_t ldx;
    double *y;
    int64_t ldy;
    SpmmEpiDev e;  // B, ldb, d of the fused epilogue (unread by SET)
};

// one row per lane: the row's code words once, then per column the K terms
// fma(value, x[clamp(row + off_k)], acc) (padding terms carry +0.0 codes)
template <int VB, int CW, int KB, int MODE>
__global__ __launch_bounds__(256) void spmm_dia_kernel(SpmmDiaArgs a) {
    __shared__ double stab[VB == 4 ? 16 : 256];
    for (int q = threadIdx.x; q < a.ntab; q += 256) stab[q] = a.vtab[q];
    __syncthreads();
    constexpr uint32_t MASK = (1u << VB) - 1;
    const int row = (int)(xcd_remap(blockIdx.x, gridDim.x) * 256 + threadIdx.x);
    if (row >= a.nrows) return;
    uint32_t w[CW];
#pragma unroll
    for (int q = 0; q < CW; q++) w[q] = __builtin_nontemporal_load(a.codes + (int64_t)row * CW + q);
    double acc[KB];
#pragma unroll
    for (int c = 0; c < KB; c++) acc[c] = 0.0;
    for (int k = 0; k < a.k; k++) {
        const double v = stab[(w[(k * VB) >> 5] >> ((k * VB) & 31)) & MASK];
        const int64_t col = min(max(row + a.off[k], 0), a.ncols - 1);
#pragma unroll
        for (int c = 0; c < KB; c++) acc[c] = fma(v, a.x[col + c * a.ldx], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < KB; c++) spmm_store<MODE>(a.y, a.ldy, a.x, a.ldx, a.e, row, c, acc[c]);
}

// ----------------------------------------------------------- stencil classes

struct SpmmScsArgs {
    const void *cls;
    const double *dict;
    const int32_t *offs;
    int32_t k, nrows, ncols;
    const double *x;
    int64_t ldx;
    double *y;
    int64_t ldy;
    SpmmEpiDev e;  // B, ldb, d of the fused epilogue (unread by SET)
};

template <int IB> __device__ __forceinline__ int spmm_cls(const void *cls, int r) {
    return IB == 1 ? (int)static_cast<const uint8_t *>(cls)[r] : (int)static_cast<const uint16_t *>(cls)[r];
}

// one row per lane (spmv_scs_kernel's order: the K offsets ascending, clamped x)
template <int IB, int KB, int MODE>
__global__ __launch_bounds__(256) void spmm_scs_kernel(SpmmScsArgs a) {
    const int row = (int)(xcd_remap(blockIdx.x, gridDim.x) * 256 + threadIdx.x);
    if (row >= a.nrows) return;
    const double *dct = a.dict + (int64_t)spmm_cls<IB>(a.cls, row) * a.k;
    double acc[KB];
#pragma unroll
    for (int c = 0; c < KB; c++) acc[c] = 0.0;
    for (int k = 0; k < a.k; k++) {
        const double v = dct[k];
        const int64_t col = min(max(row + a.offs[k], 0), a.ncols - 1);
#pragma unroll
        for (int c = 0; c < KB; c++) acc[c] = fma(v, a.x[col + c * a.ldx], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < KB; c++) spmm_store<MODE>(a.y, a.ldy, a.x, a.ldx, a.e, row, c, acc[c]);
}

// one row per wave (spmv_scs_lanes_kernel's order: lane q takes the offset pairs
// 2q, 2q + 1 of every 128-offset block, blocks ascending, the pair's first term
// before its second; past K -- a multiple of 8, so a pair is inside or outside as
// one -- +0.0 at the row itself; then the xor butterfly): every column is bitwise
// the single-vector launch
template <int IB, int KB, int MODE>
__global__ __launch_bounds__(256) void spmm_scs_lanes_kernel(SpmmScsArgs a) {
    const int row = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + (int)(threadIdx.x >> 6));
    if (row >= a.nrows) return;
    const int lane = threadIdx.x & 63;
    const double *dct = a.dict + (int64_t)spmm_cls<IB>(a.cls, row) * a.k;
    double acc[KB];
#pragma unroll
    for (int c = 0; c < KB; c++) acc[c] = 0.0;
    const int nb = (a.k + 127) >> 7;
#pragma unroll 2
    for (int j = 0; j < nb; j++) {
        const int kk = 128 * j + 2 * lane;
        const bool in = kk < a.k;
        const int2 of = in ? *reinterpret_cast<const int2 *>(a.offs + kk) : int2{0, 0};
        const spmm_dbl2_t v = in ? *reinterpret_cast<const spmm_dbl2_t *>(dct + kk) : spmm_dbl2_t{0.0, 0.0};
        const int64_t c0 = min(max(row + of.x, 0), a.ncols - 1);
        const int64_t c1 = min(max(row + of.y, 0), a.ncols - 1);
        double x0[KB], x1[KB];
#pragma unroll
        for (int c = 0; c < KB; c++) {
            x0[c] = a.x[c0 + c * a.ldx];
            x1[c] = a.x[c1 + c * a.ldx];
        }
#pragma unroll
        for (int c = 0; c < KB; c++) {
            acc[c] = fma(v.x, x0[c], acc[c]);
            acc[c] = fma(v.y, x1[c], acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < KB; c++) {
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) acc[c] += __shfl_xor(acc[c], m);
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < KB; c++) spmm_store<MODE>(a.y, a.ldy, a.x, a.ldx, a.e, row, c, acc[c]);
    }
}

// --------------------------------------------------------------- 3x3 blocks

constexpr int64_t SPMM_BSR_STEP = 64 * (9 * 8 + 4);  // bsr.hip's 4864-B block step
constexpr int SPMM_BSR_K8 = 4 * 64 * 16;
constexpr int SPMM_BSR_COL = SPMM_BSR_K8 + 64 * 8;

struct SpmmBsrArgs {
    const char *data;
    const int32_t *row0, *soff;
    int32_t nslices;
    const double *x;
    int64_t ldx;
    double *y;
    int64_t ldy;
    SpmmEpiDev e;  // B, ldb, d of the fused epilogue (unread by SET)
};

// one node row per lane (spmv_bsr3_kernel's order: blocks ascending, dof row
// r of block J sums v(r,0) x(3J), v(r,1) x(3J+1), v(r,2) x(3J+2) with fma)
template <int KB, int MODE>
__global__ __launch_bounds__(256) void spmm_bsr3_kernel(SpmmBsrArgs a) {
    const int sl = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + (int)(threadIdx.x >> 6));
    if (sl >= a.nslices) return;
    const int lane = threadIdx.x & 63;
    const int I = a.row0[sl] + lane;
    const bool live = I < a.row0[sl + 1];
    const int t0 = a.soff[sl], w = a.soff[sl + 1] - t0;
    double acc[KB][3];
#pragma unroll
    for (int c = 0; c < KB; c++) acc[c][0] = acc[c][1] = acc[c][2] = 0.0;
    for (int t = 0; t < w; t++) {
        const char *p = a.data + (int64_t)(t0 + t) * SPMM_BSR_STEP;
        double v[9];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const spmm_dbl2_t u = __builtin_nontemporal_load(reinterpret_cast<const spmm_dbl2_t *>(p + q * 1024) + lane);
            v[2 * q] = u.x;
            v[2 * q + 1] = u.y;
        }
        v[8] = __builtin_nontemporal_load(reinterpret_cast<const double *>(p + SPMM_BSR_K8) + lane);
        const int J = __builtin_nontemporal_load(reinterpret_cast<const int32_t *>(p + SPMM_BSR_COL) + lane);
#pragma unroll
        for (int c = 0; c < KB; c++) {
            const double *xp = a.x + 3 * (int64_t)J + c * a.ldx;
            const double x0 = xp[0], x1 = xp[1], x2 = xp[2];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                acc[c][r] = fma(v[3 * r], x0, acc[c][r]);
                acc[c][r] = fma(v[3 * r + 1], x1, acc[c][r]);
                acc[c][r] = fma(v[3 * r + 2], x2, acc[c][r]);
            }
        }
    }
    if (live) {
#pragma unroll
        for (int c = 0; c < KB; c++)
#pragma unroll
            for (int r = 0; r < 3; r++) spmm_store<MODE>(a.y, a.ldy, a.x, a.ldx, a.e, 3 * (int64_t)I + r, c, acc[c][r]);
    }
}

// ------------------------------------------------------------- pattern SELL

struct SpmmSellpArgs {
    const char *vals;
    const int64_t *eoff;
    const int32_t *row0;
    const int2 *pat;
    const int32_t *offs;
    const int32_t *rbase;
    const double *vtab;
    int32_t ntab, nslices, ncols;
    const double *x;
    int64_t ldx;
    double *y;
    int64_t ldy;
    SpmmEpiDev e;  // B, ldb, d of the fused epilogue (unread by SET)
};

// spmv_sellp_kernel's sums per column: lane q of a row walks its steps t = s L + q
// ascending with fma (fp64 values or 4/8-bit codes from the LDS table), padding
// steps +0.0 at a clamped column, then the same xor butterfly over the L lanes.
// A wave per slice.
template <int L, int VB, int KB, int MODE>
__global__ __launch_bounds__(256) void spmm_sellp_kernel(SpmmSellpArgs a) {
    __shared__ double stab[VB ? 256 : 1];
    if constexpr (VB != 0) {
        for (int i = threadIdx.x; i < a.ntab; i += 256) stab[i] = a.vtab[i];
        __syncthreads();
    }
    const int s = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + (int)(threadIdx.x >> 6));
    if (s >= a.nslices) return;
    const int lane = threadIdx.x & 63, r = lane / L, q = lane % L;
    const int row = a.row0[s] + r;
    const bool live = row < a.row0[s + 1];
    const int rowc = live ? row : a.row0[s];
    const int base = a.rbase ? a.rbase[rowc] : rowc;
    const int2 pw = a.pat[s];
    const int32_t *off = a.offs + pw.x;
    const int w = pw.y, S = (w + L - 1) / L;
    const int64_t e0 = a.eoff[s];
    double acc[KB];
#pragma unroll
    for (int c = 0; c < KB; c++) acc[c] = 0.0;
    // codes: whole words of K lane-steps, as spmv_sellp_kernel walks them
    const int send = VB == 0 ? S : (S + 32 / (VB ? VB : 1) - 1) / (32 / (VB ? VB : 1)) * (32 / (VB ? VB : 1));
    for (int st = 0; st < send; st++) {
        const int t = st * L + q;
        const bool in = t < w;
        const int64_t col = min(max(base + off[in ? t : 0], 0), a.ncols - 1);
        double v;
        if constexpr (VB == 0) {
            v = __builtin_nontemporal_load(reinterpret_cast<const double *>(a.vals) + e0 + (int64_t)st * 64 + lane);
        } else {
            constexpr int K = 32 / VB;
            const uint32_t wd = reinterpret_cast<const uint32_t *>(a.vals)[e0 + (int64_t)(st / K) * 64 + lane];
            v = stab[(wd >> ((st % K) * VB)) & ((1u << VB) - 1)];
        }
        v = in ? v : 0.0;
#pragma unroll
        for (int c = 0; c < KB; c++) acc[c] = fma(v, (L > 1 || VB == 0 || in) ? a.x[col + c * a.ldx] : 0.0, acc[c]);
    }
#pragma unroll
    for (int c = 0; c < KB; c++)
#pragma unroll
        for (int m = L / 2; m > 0; m >>= 1) acc[c] += __shfl_xor(acc[c], m);
    if (live && q == 0) {
#pragma unroll
        for (int c = 0; c < KB; c++) spmm_store<MODE>(a.y, a.ldy, a.x, a.ldx, a.e, row, c, acc[c]);
    }
}

// ------------------------------------------------------------------ dispatch

#define FAMG_SPMM_KB(KB_EXPR, LAUNCH)                                                              \
    switch (KB_EXPR) {                                                                             \
    case 1: LAUNCH(1); break;                                                                      \
    case 2: LAUNCH(2); break;                                                                      \
    case 3: LAUNCH(3); break;                                                                      \
    case 4: LAUNCH(4); break;                                                                      \
    case 5: LAUNCH(5); break;                                                                      \
    case 6: LAUNCH(6); break;                                                                      \
    case 7: LAUNCH(7); break;                                                                      \
    default: LAUNCH(8); break;                                                                     \
    }

// Y = A X over k columns for DIA / stencil-class / 3x3-block storage; false if
// the storage is none of these (the caller applies per column).
// MODE: the epilogue fused at the store sites (SET: none, the plain Y = A X);
// e: its operands B (advanced with the column group here), ldb, d.
enum SpmmKind { SPMM_NONE, SPMM_DIA, SPMM_SCS, SPMM_BSR, SPMM_SELLP, SPMM_XS };
static SpmmKind spmm_kind(const GpuCsr &m) {
    const int sL = m.sellp.L, sV = m.sellp.vbits;
    if (m.kernel == SPMV_KERNEL_XS && m.xs.built()) return SPMM_XS;
    if (m.kernel == SPMV_KERNEL_DIA && m.dia.built() && !m.dia.rowid && m.dia.r0 == 0 && m.dia.r1 == m.nrows &&
        m.dia.k <= 64)
        return SPMM_DIA;
    // (eight lanes per row: no k-wide kernel sums in that order, spmm_epi runs one SpMV per column)
    if (m.kernel == SPMV_KERNEL_SCS && m.scs.built() && m.scs.seg < 0 && xscs_row_lanes(m) == 1) return SPMM_SCS;
    if (m.kernel == SPMV_KERNEL_BSR && m.bsr.built()) return SPMM_BSR;
    if (m.kernel == SPMV_KERNEL_SELLP && m.sellp.built() && m.sellp.seg_slc.size() <= 2 &&
        (sL == 1 || sL == 2 || sL == 4 || sL == 8 || sL == 16 || sL == 32 || sL == 64) &&
        (sV == 0 || sV == 4 || sV == 8))
        return SPMM_SELLP;
    return SPMM_NONE;
}

bool spmm_has_kernel(const GpuCsr &m) {
    return spmm_kind(m) != SPMM_NONE || (m.kernel == SPMV_KERNEL_SELL && !m.sell.vbits);
}

template <int MODE>
static bool spmm_compressed_t(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k,
                              const SpmmEpiDev &e0, hipStream_t s) {
    const SpmmKind kind = spmm_kind(m);
    const bool dia = kind == SPMM_DIA, scs = kind == SPMM_SCS, bsr = kind == SPMM_BSR, xs = kind == SPMM_XS;
    const bool sellp = kind == SPMM_SELLP;
    const int sL = m.sellp.L, sV = m.sellp.vbits;
    if (xs) {  // xsell.hip: per column with its x chunks in LDS
        if constexpr (MODE == SPMV_SET) return spmm_xs(m, x, ldx, y, ldy, k, s);
        else return spmm_xs_epi(m, x, ldx, y, ldy, k, (SpmvMode)MODE, SpmmEpi{e0.b, e0.ldb, e0.d}, s);
    }
    if (!dia && !scs && !bsr && !sellp) return false;
    if (m.nrows == 0 || k == 0) return true;
    for (int64_t c0 = 0; c0 < k; c0 += SPMM_COLS) {
        const int kb = (int)std::min<int64_t>(SPMM_COLS, k - c0);
        const double *xc = x + c0 * ldx;
        double *yc = y + c0 * ldy;
        const SpmmEpiDev e{e0.b ? e0.b + c0 * e0.ldb : nullptr, e0.ldb, e0.d};
        if (dia) {
            SpmmDiaArgs a{};
            a.codes = m.dia.codes.get();
            a.vtab = m.dia.vtab.get();
            a.ntab = (int32_t)m.dia.ntab;
            a.k = m.dia.k;
            a.nrows = (int32_t)m.nrows;
            a.ncols = (int32_t)m.ncols;
            for (int q = 0; q < m.dia.k; q++) a.off[q] = m.dia.off[q];
            a.x = xc;
            a.ldx = ldx;
            a.y = yc;
            a.ldy = ldy;
            a.e = e;
            const dim3 grid((unsigned)ceil_div(m.nrows, 256)), block(256);
            const int key = m.dia.vbits * 16 + m.dia.cw;
#define FAMG_L41(KB) spmm_dia_kernel<4, 1, KB, MODE><<<grid, block, 0, s>>>(a)
#define FAMG_L42(KB) spmm_dia_kernel<4, 2, KB, MODE><<<grid, block, 0, s>>>(a)
#define FAMG_L44(KB) spmm_dia_kernel<4, 4, KB, MODE><<<grid, block, 0, s>>>(a)
#define FAMG_L45(KB) spmm_dia_kernel<4, 5, KB, MODE><<<grid, block, 0, s>>>(a)
#define FAMG_L81(KB) spmm_dia_kernel<8, 1, KB, MODE><<<grid, block, 0, s>>>(a)
#define FAMG_L82(KB) spmm_dia_kernel<8, 2, KB, MODE><<<grid, block, 0, s>>>(a)
#define FAMG_L84(KB) spmm_dia_kernel<8, 4, KB, MODE><<<grid, block, 0, s>>>(a)
#define FAMG_L88(KB) spmm_dia_kernel<8, 8, KB, MODE><<<grid, block, 0, s>>>(a)
#define FAMG_L89(KB) spmm_dia_kernel<8, 9, KB, MODE><<<grid, block, 0, s>>>(a)
            switch (key) {
            case 4 * 16 + 1: FAMG_SPMM_KB(kb, FAMG_L41) break;
            case 4 * 16 + 2: FAMG_SPMM_KB(kb, FAMG_L42) break;
            case 4 * 16 + 4: FAMG_SPMM_KB(kb, FAMG_L44) break;
            case 4 * 16 + 5: FAMG_SPMM_KB(kb, FAMG_L45) break;
            case 8 * 16 + 1: FAMG_SPMM_KB(kb, FAMG_L81) break;
            case 8 * 16 + 2: FAMG_SPMM_KB(kb, FAMG_L82) break;
            case 8 * 16 + 4: FAMG_SPMM_KB(kb, FAMG_L84) break;
            case 8 * 16 + 8: FAMG_SPMM_KB(kb, FAMG_L88) break;
            case 8 * 16 + 9: FAMG_SPMM_KB(kb, FAMG_L89) break;
            default: fail(AMG_ERR_INVALID, "SpMM: unsupported DIA code layout");
            }
        } else if (scs) {
            SpmmScsArgs a{m.scs.cls.get(), m.scs.dict.get(), m.scs.offs.get(), (int32_t)m.scs.k,
                          (int32_t)m.nrows, (int32_t)m.ncols, xc, ldx, yc, ldy, e};
            const dim3 grid((unsigned)ceil_div(m.nrows, m.scs.lanes ? 4 : 256)), block(256);
#define FAMG_S1(KB) spmm_scs_kernel<1, KB, MODE><<<grid, block, 0, s>>>(a)
#define FAMG_S2(KB) spmm_scs_kernel<2, KB, MODE><<<grid, block, 0, s>>>(a)
#define FAMG_SL1(KB) spmm_scs_lanes_kernel<1, KB, MODE><<<grid, block, 0, s>>>(a)
#define FAMG_SL2(KB) spmm_scs_lanes_kernel<2, KB, MODE><<<grid, block, 0, s>>>(a)
            if (m.scs.lanes) {
                if (m.scs.ib == 1) { FAMG_SPMM_KB(kb, FAMG_SL1) }
                else { FAMG_SPMM_KB(kb, FAMG_SL2) }
            } else {
                if (m.scs.ib == 1) { FAMG_SPMM_KB(kb, FAMG_S1) }
                else { FAMG_SPMM_KB(kb, FAMG_S2) }
            }
        } else if (sellp) {
            SpmmSellpArgs a{m.sellp.vals.get(), m.sellp.eoff.get(), m.sellp.row0.get(),
                            reinterpret_cast<const int2 *>(m.sellp.pat.get()), m.sellp.offs.get(), m.sellp.rbase.get(),
                            m.sellp.vtab.get(), (int32_t)m.sellp.ntab, (int32_t)m.sellp.slices, (int32_t)m.ncols,
                            xc, ldx, yc, ldy, e};
            const dim3 grid((unsigned)ceil_div(m.sellp.slices, 4)), block(256);
#define FAMG_P(L, VB, KB) spmm_sellp_kernel<L, VB, KB, MODE><<<grid, block, 0, s>>>(a)
#define FAMG_PL(L, VB)                                                                              \
    {                                                                                               \
        auto go = [&](auto kbc) { FAMG_P(L, VB, decltype(kbc)::value); };                           \
        switch (kb) {                                                                               \
        case 1: go(std::integral_constant<int, 1>{}); break;                                        \
        case 2: go(std::integral_constant<int, 2>{}); break;                                        \
        case 3: go(std::integral_constant<int, 3>{}); break;                                        \
        case 4: go(std::integral_constant<int, 4>{}); break;                                        \
        case 5: go(std::integral_constant<int, 5>{}); break;                                        \
        case 6: go(std::integral_constant<int, 6>{}); break;                                        \
        case 7: go(std::integral_constant<int, 7>{}); break;                                        \
        default: go(std::integral_constant<int, 8>{}); break;                                       \
        }                                                                                           \
    }
#define FAMG_PV(L)                                                                                  \
    if (sV == 0) FAMG_PL(L, 0) else if (sV == 4) FAMG_PL(L, 4) else FAMG_PL(L, 8)
            switch (sL) {
            case 1: FAMG_PV(1) break;
            case 2: FAMG_PV(2) break;
            case 4: FAMG_PV(4) break;
            case 8: FAMG_PV(8) break;
            case 16: FAMG_PV(16) break;
            case 32: FAMG_PV(32) break;
            default: FAMG_PV(64) break;
            }
#undef FAMG_PV
#undef FAMG_PL
#undef FAMG_P
        } else {
            SpmmBsrArgs a{m.bsr.data.get(), m.bsr.row0.get(), m.bsr.soff.get(), (int32_t)m.bsr.slices,
                          xc, ldx, yc, ldy, e};
            const dim3 grid((unsigned)ceil_div(m.bsr.slices, 4)), block(256);
#define FAMG_B(KB) spmm_bsr3_kernel<KB, MODE><<<grid, block, 0, s>>>(a)
            FAMG_SPMM_KB(kb, FAMG_B)
        }
        FAMG_CHECK_HIP(hipGetLastError());
    }
    return true;
}

bool spmm_compressed(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k, hipStream_t s) {
    return spmm_compressed_t<SPMV_SET>(m, x, ldx, y, ldy, k, SpmmEpiDev{nullptr, 0, nullptr}, s);
}

// the same with the cycle's epilogue fused at the store sites (spmm_epi, spmv.hip)
bool spmm_compressed_epi(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k,
                         SpmvMode mode, const SpmmEpi &epi, hipStream_t s) {
    const SpmmEpiDev e{epi.b, epi.ldb, epi.d};
    switch (mode) {
    case SPMV_SET: return spmm_compressed_t<SPMV_SET>(m, x, ldx, y, ldy, k, e, s);
    case SPMV_ADD: return spmm_compressed_t<SPMV_ADD>(m, x, ldx, y, ldy, k, e, s);
    case SPMV_RESID: return spmm_compressed_t<SPMV_RESID>(m, x, ldx, y, ldy, k, e, s);
    case SPMV_JACOBI: return spmm_compressed_t<SPMV_JACOBI>(m, x, ldx, y, ldy, k, e, s);
    default: fail(AMG_ERR_INVALID, "SpMM epilogue: mode must be SET, ADD, RESID or JACOBI");
    }
}

}  // namespace famg
