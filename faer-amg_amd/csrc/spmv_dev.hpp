// spmv_dev.hpp -- what the SpMV kernel files (spmv.hip, sell.hip, dia.hip) share:
// the epilogue operands and their load / store, the vector types, the per-mode
// launch macro and the thresholds both one-lane storages are chosen by.
#pragma once

#include "famg.hpp"

namespace famg {

typedef double dbl2_t __attribute__((ext_vector_type(2)));
typedef double dbl2u_t __attribute__((ext_vector_type(2), aligned(8)));
typedef int32_t i32x2_t __attribute__((ext_vector_type(2)));
typedef int32_t i32x4_t __attribute__((ext_vector_type(4)));

constexpr int SELL_C = 64;
constexpr int64_t SELL_MIN_ROWS = 65536;
constexpr int VECTOR_MIN_AVG = 256;
// rows at least this long on average take the wave-per-row kernel; A/B switch
// FAMG_VECTOR_MIN_AVG (lower values replace SELL on A_2: measured 2.7x slower)
inline int64_t vec_min_avg() {
    static const int64_t x = env_int("FAMG_VECTOR_MIN_AVG", 0);
    return x > 0 ? x : (int64_t)VECTOR_MIN_AVG;
}

struct Epi {
    const double *x;
    double *y;
    const double *b;
    const double *d;
    const int32_t *perm;
    const uint8_t *dc;  // JACOBI: d[i] = dt[dc[i]] when set (8-bit codes of the diagonal)
    const double *dt;
    double dk;          // d when it is one value (the constant-diagonal epilogues)
};

// The epilogue's arithmetic on one row sum -- the one expression every store site
// (the single-vector kernels' EpiOps and the SpMM kernels' spmm_store) goes through.
template <int MODE>
__device__ __forceinline__ double epi_value(double acc, double xr, double br, double dr, double yr) {
    if constexpr (MODE == SPMV_SET) return acc;
    else if constexpr (MODE == SPMV_ADD || MODE == SPMV_ADD0) return yr + acc;
    else if constexpr (MODE == SPMV_RESID || MODE == SPMV_RESID0) return br - acc;
    else return xr + dr * (br - acc);  // JACOBI, SGS
}

// Operands of a k-wide epilogue (spmm_epi): B column-major, d shared by all columns.
struct SpmmEpiDev {
    const double *b;
    int64_t ldb;
    const double *d;
};

// The store site of an SpMM kernel: column c of row `row` (SET / ADD / RESID / JACOBI).
template <int MODE>
__device__ __forceinline__ void spmm_store(double *y, int64_t ldy, const double *x, int64_t ldx, const SpmmEpiDev &e,
                                           int64_t row, int c, double acc) {
    double xr = 0.0, br = 0.0, dr = 0.0, yr = 0.0;
    if constexpr (MODE == SPMV_JACOBI) {
        xr = x[row + c * ldx];
        dr = e.d[row];
    }
    if constexpr (MODE == SPMV_JACOBI || MODE == SPMV_RESID) br = e.b[row + c * e.ldb];
    if constexpr (MODE == SPMV_ADD) yr = y[row + c * ldy];
    y[row + c * ldy] = epi_value<MODE>(acc, xr, br, dr, yr);
}

// Operands of the epilogue that do not depend on the row sum are fetched
// before the row's loads are issued.
template <int MODE> struct EpiOps {
    double xr = 0.0, br = 0.0, dr = 0.0, yr = 0.0;
    int i = 0;
    __device__ __forceinline__ void load(const Epi &a, int row) {
        i = row;
        if constexpr (MODE == SPMV_SGS) i = a.perm[row];
        if constexpr (MODE == SPMV_JACOBI || MODE == SPMV_SGS) {
            xr = a.x[i];
            br = a.b[i];
            dr = (MODE == SPMV_JACOBI && a.dc) ? a.dt[a.dc[row]] : a.d[row];
        }
        if constexpr (MODE == SPMV_RESID || MODE == SPMV_RESID0) br = a.b[row];
        if constexpr (MODE == SPMV_ADD) yr = a.y[row];
        if constexpr (MODE == SPMV_ADD0) yr = (a.dc ? a.dt[a.dc[row]] : a.d[row]) * a.b[row];
    }
    __device__ __forceinline__ void store(const Epi &a, double acc) const {
        a.y[i] = epi_value<MODE>(acc, xr, br, dr, yr);
    }
};

// The x operand of a row sum: x[c], or for RESID0 the zero-guess Jacobi
// iterate d[c]*x[c] -- the same rounded product vec_mul would have stored.
template <int MODE> __device__ __forceinline__ double gx(const Epi &e, int c) {
    if constexpr (MODE == SPMV_RESID0) return e.d[c] * e.x[c];
    else return e.x[c];
}

// Epilogue of two adjacent rows (row, row + 1) with 16-B accesses when both live.
// NT: b, d and y (streamed once, never gathered) bypass the caches.
template <int MODE, bool NT = false> struct EpiOps2 {
    dbl2_t xr = {0.0, 0.0}, br = {0.0, 0.0}, dr = {0.0, 0.0}, yr = {0.0, 0.0};
    int i = 0;
    bool l0 = false, l1 = false;
    __device__ __forceinline__ dbl2_t ld(const double *p) const {
        if (l1) return *reinterpret_cast<const dbl2u_t *>(p + i);
        dbl2_t v = {p[i], 0.0};
        return v;
    }
    __device__ __forceinline__ dbl2_t lds(const double *p) const {  // streamed operand
        if constexpr (NT) {
            if (l1) return __builtin_nontemporal_load(reinterpret_cast<const dbl2u_t *>(p + i));
            dbl2_t v = {__builtin_nontemporal_load(p + i), 0.0};
            return v;
        } else {
            return ld(p);
        }
    }
    __device__ __forceinline__ void load(const Epi &a, int row, bool live0, bool live1) {
        i = row;
        l0 = live0;
        l1 = live1;
        if (!l0) return;
        if constexpr (MODE == SPMV_JACOBI) {
            xr = ld(a.x);
            br = lds(a.b);
            if (a.dc) {
                dr.x = a.dt[a.dc[i]];
                dr.y = l1 ? a.dt[a.dc[i + 1]] : 0.0;
            } else {
                dr = lds(a.d);
            }
        }
        if constexpr (MODE == SPMV_RESID || MODE == SPMV_RESID0) br = lds(a.b);
        if constexpr (MODE == SPMV_ADD) yr = lds(a.y);
        if constexpr (MODE == SPMV_ADD0) {
            if (a.dc) {  // coded diagonal: 1 B per row instead of 8
                dr.x = a.dt[a.dc[i]];
                dr.y = l1 ? a.dt[a.dc[i + 1]] : 0.0;
                yr = dr * lds(a.b);
            } else {
                yr = lds(a.d) * lds(a.b);
            }
        }
    }
    __device__ __forceinline__ void store(const Epi &a, double acc0, double acc1) const {
        if (!l0) return;
        const dbl2_t out = {epi_value<MODE>(acc0, xr.x, br.x, dr.x, yr.x), epi_value<MODE>(acc1, xr.y, br.y, dr.y, yr.y)};
        if constexpr (NT) {
            if (l1) __builtin_nontemporal_store(out, reinterpret_cast<dbl2u_t *>(a.y + i));
            else __builtin_nontemporal_store(out.x, a.y + i);
        } else {
            if (l1) *reinterpret_cast<dbl2u_t *>(a.y + i) = out;
            else a.y[i] = out.x;
        }
    }
};

// KERNEL<MODE [, extra template args]> on (grid, block, stream s); the optional
// trailing argument is pasted after MODE (e.g. FAMG_LAY1).
#define FAMG_LAUNCH_MODES(KERNEL, grid, block, s, args, ...)                             \
    switch (mode) {                                                                     \
    case SPMV_SET: KERNEL<SPMV_SET __VA_ARGS__><<<grid, block, 0, s>>>(args); break;       \
    case SPMV_ADD: KERNEL<SPMV_ADD __VA_ARGS__><<<grid, block, 0, s>>>(args); break;       \
    case SPMV_RESID: KERNEL<SPMV_RESID __VA_ARGS__><<<grid, block, 0, s>>>(args); break;   \
    case SPMV_JACOBI: KERNEL<SPMV_JACOBI __VA_ARGS__><<<grid, block, 0, s>>>(args); break; \
    case SPMV_SGS: KERNEL<SPMV_SGS __VA_ARGS__><<<grid, block, 0, s>>>(args); break;       \
    case SPMV_RESID0: KERNEL<SPMV_RESID0 __VA_ARGS__><<<grid, block, 0, s>>>(args); break; \
    case SPMV_ADD0: KERNEL<SPMV_ADD0 __VA_ARGS__><<<grid, block, 0, s>>>(args); break;     \
    default: break;                                                                     \
    }
#define FAMG_LAY0 , 0
#define FAMG_LAY1 , 1
#define FAMG_LAY4 , 4
#define FAMG_LAY8 , 8
#define FAMG_LAY16 , 16

}  // namespace famg
