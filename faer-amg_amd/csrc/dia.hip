// dia.hip -- DIA-code storage of constant-stencil operators: its kernels (generic,
// run patterns, constant stencils, the SGS colour sweep), its builders and its
// SpMV launches.
#include <algorithm>

#include "spmv_dev.hpp"

namespace famg {

// A/B switches (results are bitwise equal either way).  FAMG_DIA_NT=1 streams the
// epilogue operands (b, d, y) with non-temporal accesses; FAMG_DIA_BANDS=0 turns
// the 2.5-D (plane-band per XCD) block order off; FAMG_DIA_CST=0: a constant
// stencil still reads its rows' codes; FAMG_DIA_PAT=0: no DIA storage for more
// than 32 diagonals; FAMG_DIA_RUNS=0 / FAMG_DIA_RUNS7=0: the 27- / 7-point kernels
// load every diagonal's pair; FAMG_DIA_PAT27=0: the 27-point SpMV takes
// spmv_dia_kernel<NR = 9>; FAMG_DIA_RC=0: the folded residual gathers 8-B values
// of d.
static bool dia_bands() { static const bool on = env_not_zero("FAMG_DIA_BANDS"); return on; }
static bool dia_nt() { static const bool on = env_is_one("FAMG_DIA_NT"); return on; }
static bool dia_cst_enabled() { static const bool on = env_not_zero("FAMG_DIA_CST"); return on; }
static bool dia_pat_enabled() { static const bool on = env_not_zero("FAMG_DIA_PAT"); return on; }
static bool dia_runs() { static const bool on = env_not_zero("FAMG_DIA_RUNS"); return on; }
static bool dia_runs7() { static const bool on = env_not_zero("FAMG_DIA_RUNS7"); return on; }
static bool dia_pat27() { static const bool on = env_not_zero("FAMG_DIA_PAT27"); return on; }
static bool dia_rc_enabled() { static const bool on = env_not_zero("FAMG_DIA_RC"); return on; }

// ---------------------------------------------------------------- DIA codes
//
// A square matrix whose entries lie on at most DIA_MAX diagonals (the union of
// col - row offsets; a constant stencil: 7 for the 7-pt Laplacian, 27 for the
// 27-pt operator), that fills them to >= 80 % and whose values have a 4/8-bit
// value table is stored as one code word group per row: the codes of its K
// diagonals, ascending offset (= ascending column, the stored order), with
// the +0.0 code where a row has no entry.  No per-slice metadata exists, so a
// row's only dependent chain is code + x loads -> fma -> store; each lane takes
// two adjacent rows (16-B accesses throughout).  x indices outside [0, ncols)
// belong to padding entries (value 0.0) and are clamped.
constexpr int DIA_MAX = 40;  // 32 for the generic kernels; longer stencils through a run pattern

struct DiaArgs {
    const uint32_t *codes;  // cw words per row (rows padded by 2)
    const double *vtab;
    int32_t ntab, k, row_begin, row_end, ncols;
    int32_t code_row0;  // first row with codes (the DIA row range may be one segment)
    int32_t band_bp;    // > 0: 512-row blocks per plane; XCD x walks band x of every plane
    int32_t off[DIA_MAX];
    Epi e;
    int32_t gnx, gny, gnz;  // CST: the grid (nx even)
    double cst[27];         // CST: the interior stencil
};

typedef int32_t i32x2u_t __attribute__((ext_vector_type(2), aligned(4)));
typedef int32_t i32x4u_t __attribute__((ext_vector_type(4), aligned(4)));

// x operands of rows (r, r+1) at column c = r + off: x[clamp(c)], x[clamp(c+1)]
// from one 16-B load at clamp(c, 0, ncols-2) and selects -- branch-free, so
// the loads of all diagonals stay in flight together (a divergent edge path
// made the compiler wait for each load at its join).  Needs ncols >= 2.
template <int MODE> __device__ __forceinline__ void dia_gx2(const Epi &e, int c, int ncols, double &x0, double &x1) {
    const int cc = min(max(c, 0), ncols - 2);
    dbl2_t v = *reinterpret_cast<const dbl2u_t *>(e.x + cc);
    if constexpr (MODE == SPMV_RESID0) v = *reinterpret_cast<const dbl2u_t *>(e.d + cc) * v;
    x0 = c > ncols - 2 ? v.y : v.x;
    x1 = c < 0 ? v.x : v.y;
}

template <int CW>
__device__ __forceinline__ void dia_codes2(const uint32_t *cp, uint32_t (&w0)[CW], uint32_t (&w1)[CW]) {
    if constexpr (CW == 1) {
        const i32x2u_t v = __builtin_nontemporal_load(reinterpret_cast<const i32x2u_t *>(cp));
        w0[0] = (uint32_t)v.x;
        w1[0] = (uint32_t)v.y;
    } else if constexpr (CW == 2) {
        const i32x4u_t v = __builtin_nontemporal_load(reinterpret_cast<const i32x4u_t *>(cp));
        w0[0] = (uint32_t)v.x;
        w0[1] = (uint32_t)v.y;
        w1[0] = (uint32_t)v.z;
        w1[1] = (uint32_t)v.w;
    } else {
#pragma unroll
        for (int q = 0; q < CW / 4; q++) {
            const i32x4u_t v0 = __builtin_nontemporal_load(reinterpret_cast<const i32x4u_t *>(cp) + q);
            const i32x4u_t v1 = __builtin_nontemporal_load(reinterpret_cast<const i32x4u_t *>(cp + CW) + q);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                w0[4 * q + j] = (uint32_t)v0[j];
                w1[4 * q + j] = (uint32_t)v1[j];
            }
        }
    }
}

// The weighted-Jacobi epilogue with the 8-bit coded diagonal (d = dt[dc[i]],
// dt padded to 256 entries and staged in LDS with the value table).
constexpr int DIA_JACOBI_DC = 16;
// The folded zero-guess residual y = b - A (d x) with the 8-bit coded diagonal:
// the 7-point kernel gathers the 1-B codes of d beside x (dt staged in LDS)
// instead of 8-B values of d: 17 MB instead of 134 MB more than a residual.
constexpr int DIA_RESID0_DC = 17;
// The same two epilogues when the coded diagonal is one value (Epi::dk: the 7-point
// Laplacian's a_ii = 6 everywhere): d is one scalar load, no per-row or gathered
// codes (the 7-point run kernel only)
constexpr int DIA_JACOBI_DK = 18;
constexpr int DIA_RESID0_DK = 19;

// 8-bit codes at the positions dia_gx2 / dia_gx4 take their x operands from
// (same clamps and selects)
__device__ __forceinline__ void dia_gc2(const uint8_t *dc, int c, int ncols, uint32_t &k0, uint32_t &k1) {
    const int cc = min(max(c, 0), ncols - 2);
    const uint32_t a0 = dc[cc], a1 = dc[cc + 1];
    k0 = c > ncols - 2 ? a1 : a0;
    k1 = c < 0 ? a0 : a1;
}
__device__ __forceinline__ void dia_gc4(const uint8_t *dc, int c, int ncols, uint32_t (&k)[4]) {
    const int p0 = min(max(c, 0), ncols - 2), p1 = min(max(c + 2, 0), ncols - 2);
    const uint32_t a0 = dc[p0], a1 = dc[p0 + 1], b0 = dc[p1], b1 = dc[p1 + 1];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int t = c + j;
        k[j] = t == p0 ? a0 : t == p0 + 1 ? a1 : t == p1 ? b0 : b1;
    }
}

// Epilogue operands of a DIA row pair, loaded without divergence: one 16-B
// load at i2 = min(row, row_end - 2) per vector; a tail row (row_end - 1)
// takes the upper half.  Lanes past row_end load in-range data and store
// nothing.
template <int MODE, bool NT> struct DiaEpi {
    dbl2_t xr = {0.0, 0.0}, br = {0.0, 0.0}, dr = {0.0, 0.0}, yr = {0.0, 0.0};
    int row = 0, i2 = 0;
    uint32_t dc0 = 0, dc1 = 0;
    bool l0 = false, l1 = false;
    __device__ __forceinline__ dbl2_t ldv(const double *p) const {
        const dbl2u_t *q = reinterpret_cast<const dbl2u_t *>(p + i2);
        dbl2_t v = NT ? __builtin_nontemporal_load(q) : *q;
        if (row != i2) v.x = v.y;
        return v;
    }
    // the diagonal codes are loaded first: waiting for them later waits for nothing else
    __device__ __forceinline__ void load_codes(const Epi &a, int r, int row_end) {
        if constexpr (MODE == DIA_JACOBI_DC) {
            dc0 = a.dc[min(r, row_end - 1)];
            dc1 = a.dc[min(r + 1, row_end - 1)];
        }
    }
    __device__ __forceinline__ void load(const Epi &a, int r, int row_end) {
        row = r;
        i2 = min(r, row_end - 2);
        l0 = r < row_end;
        l1 = r + 1 < row_end;
        if constexpr (MODE == SPMV_JACOBI || MODE == DIA_JACOBI_DC || MODE == DIA_JACOBI_DK) {
            const dbl2u_t *q = reinterpret_cast<const dbl2u_t *>(a.x + i2);  // x is gathered: cached
            xr = *q;
            if (row != i2) xr.x = xr.y;
            br = ldv(a.b);
        }
        if constexpr (MODE == SPMV_JACOBI) dr = ldv(a.d);
        if constexpr (MODE == SPMV_RESID || MODE == SPMV_RESID0 || MODE == DIA_RESID0_DC || MODE == DIA_RESID0_DK)
            br = ldv(a.b);
        if constexpr (MODE == SPMV_ADD) yr = ldv(a.y);
        if constexpr (MODE == SPMV_ADD0) yr = ldv(a.d) * ldv(a.b);
    }
    __device__ __forceinline__ void store(const Epi &a, const double *sdt, double acc0, double acc1) {
        const dbl2_t acc = {acc0, acc1};
        dbl2_t out;
        if constexpr (MODE == DIA_JACOBI_DC) dr = dbl2_t{sdt[dc0], sdt[dc1]};
        if constexpr (MODE == SPMV_SET) out = acc;
        else if constexpr (MODE == SPMV_ADD || MODE == SPMV_ADD0) out = yr + acc;
        else if constexpr (MODE == SPMV_RESID || MODE == SPMV_RESID0 || MODE == DIA_RESID0_DC || MODE == DIA_RESID0_DK)
            out = br - acc;
        else out = xr + dr * (br - acc);  // JACOBI
        if (l1) {
            if constexpr (NT) __builtin_nontemporal_store(out, reinterpret_cast<dbl2u_t *>(a.y + row));
            else *reinterpret_cast<dbl2u_t *>(a.y + row) = out;
        } else if (l0) {
            if constexpr (NT) __builtin_nontemporal_store(out.x, a.y + row);
            else a.y[row] = out.x;
        }
    }
};

// Two adjacent rows per lane, 512 rows per workgroup.  Every load is issued
// unconditionally (clamped indices; all KMAX diagonals, off[k] = 0 past K,
// whose terms are not added), so no load waits on another -- a divergent edge
// path or a per-diagonal guard made the compiler wait for each load at the
// join.  The value table (and the coded diagonal's table) is fetched first and
// published to LDS behind an LDS-only barrier after the row loads are issued,
// so they stay in flight across it.
// x[c .. c+3] of rows (r, r+1) for a run of three diagonals (offsets o-1, o, o+1,
// c = r + o - 1) from two 16-B loads at clamp(c) and clamp(c + 2); selects keep
// every in-range position exact at the matrix edges (out-of-range positions
// belong to +0.0 terms).
template <int MODE>
__device__ __forceinline__ void dia_gx4(const Epi &e, int c, int ncols, double (&v)[4]) {
    const int p0 = min(max(c, 0), ncols - 2), p1 = min(max(c + 2, 0), ncols - 2);
    dbl2_t q0 = *reinterpret_cast<const dbl2u_t *>(e.x + p0);
    dbl2_t q1 = *reinterpret_cast<const dbl2u_t *>(e.x + p1);
    if constexpr (MODE == SPMV_RESID0) {
        q0 = *reinterpret_cast<const dbl2u_t *>(e.d + p0) * q0;
        q1 = *reinterpret_cast<const dbl2u_t *>(e.d + p1) * q1;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int t = c + j;
        v[j] = t == p0 ? q0.x : t == p0 + 1 ? q0.y : t == p1 ? q1.x : q1.y;
    }
}

// NR > 0: the K = 3 NR diagonals come in runs of three consecutive offsets (a
// 27-point stencil: NR = 9); a row pair's three x operands per run are four
// consecutive values, two 16-B loads instead of three and 4 NR instead of 2 KMAX
// registers.  NR = -1: the 7-point pattern (single, single, run of three,
// single, single).  The row sums run over the same diagonals in the same order.
// CST (7-point run kernel, dia_constant): no codes, the interior coefficients
// from the arguments, x operands of neighbours outside the grid taken as 0.0
// (bitwise the coded sums, as spmv_dia_pat_kernel CST)
template <int MODE, int VB, int CW, bool NT, int NR = 0, bool CST = false>
__global__ __launch_bounds__(256) void spmv_dia_kernel(DiaArgs a) {
    constexpr bool DC = MODE == DIA_JACOBI_DC;
    constexpr bool RC = MODE == DIA_RESID0_DC && NR == -1;  // coded d gathered beside x
    constexpr bool JK = MODE == DIA_JACOBI_DK, RK = MODE == DIA_RESID0_DK;  // d = dt[0]
    static_assert(!(JK || RK) || NR == -1, "constant-d epilogues: 7-point run kernel only");
    // x operand of the row sums (RC, RK: plain x, multiplied by d after the loads)
    constexpr int GM = DC || JK ? SPMV_JACOBI : RC || RK ? SPMV_SET : MODE == DIA_RESID0_DC ? SPMV_RESID0 : MODE;
    double dk = 0.0;
    if constexpr (JK || RK) dk = a.e.dk;
    __shared__ double stab[VB == 4 ? 16 : 256];
    __shared__ double sdt[DC || RC ? 256 : 1];
    const double tv = (int)threadIdx.x < a.ntab ? a.vtab[threadIdx.x] : 0.0;
    double dv = 0.0;
    if constexpr (DC || RC) dv = a.e.dt[threadIdx.x];
    int blk;
    if (a.band_bp > 0) {
        // 2.5-D order: XCD x takes band x (1/8 of the rows) of every plane in
        // turn, so its x window is three plane bands (768 KB at 512^2 planes),
        // not three whole planes (6 MB > its 4 MB L2)
        const int bb = a.band_bp >> 3, x = blockIdx.x & 7, i = blockIdx.x >> 3;
        blk = (i / bb) * a.band_bp + x * bb + (i % bb);
    } else {
        blk = xcd_remap(blockIdx.x, gridDim.x);
    }
    const int row = a.row_begin + 512 * blk + 2 * (int)threadIdx.x;
    constexpr int KMAX = CW * 32 / VB < DIA_MAX ? CW * 32 / VB : DIA_MAX;
    constexpr uint32_t MASK = (1u << VB) - 1;
    constexpr int KX = NR != 0 ? 1 : KMAX;  // per-diagonal operands (generic path)
    constexpr int NRX = NR > 0 ? NR : 1;    // per-run operands (run path)
    DiaEpi<MODE, NT> ep;
    uint32_t w0[CW], w1[CW];
    double x0[KX], x1[KX], xq[NRX][4];
    ep.load_codes(a.e, row, a.row_end);
    ep.load(a.e, row, a.row_end);
    static_assert(!CST || NR == -1, "constant stencils: the 7-point run kernel");
    if constexpr (!CST) dia_codes2<CW>(a.codes + (int64_t)(min(row, a.row_end - 1) - a.code_row0) * CW, w0, w1);
    double xs7[4][2];  // NR == -1 (7-point): the four single diagonals
    uint32_t ks7[4][2], kq[4];  // RC: their codes of d
    if constexpr (RC) {
        dia_gc2(a.e.dc, row + a.off[0], a.ncols, ks7[0][0], ks7[0][1]);
        dia_gc2(a.e.dc, row + a.off[1], a.ncols, ks7[1][0], ks7[1][1]);
        dia_gc4(a.e.dc, row + a.off[2], a.ncols, kq);
        dia_gc2(a.e.dc, row + a.off[5], a.ncols, ks7[2][0], ks7[2][1]);
        dia_gc2(a.e.dc, row + a.off[6], a.ncols, ks7[3][0], ks7[3][1]);
    }
    if constexpr (NR > 0) {
#pragma unroll
        for (int j = 0; j < NR; j++) dia_gx4<GM>(a.e, row + a.off[3 * j], a.ncols, xq[j]);
    } else if constexpr (NR == -1) {
        dia_gx2<GM>(a.e, row + a.off[0], a.ncols, xs7[0][0], xs7[0][1]);
        dia_gx2<GM>(a.e, row + a.off[1], a.ncols, xs7[1][0], xs7[1][1]);
        dia_gx4<GM>(a.e, row + a.off[2], a.ncols, xq[0]);
        dia_gx2<GM>(a.e, row + a.off[5], a.ncols, xs7[2][0], xs7[2][1]);
        dia_gx2<GM>(a.e, row + a.off[6], a.ncols, xs7[3][0], xs7[3][1]);
    } else {
#pragma unroll
        for (int k = 0; k < KMAX; k++) dia_gx2<GM>(a.e, row + a.off[k], a.ncols, x0[k], x1[k]);
    }
    if ((int)threadIdx.x < a.ntab) stab[threadIdx.x] = tv;
    if constexpr (DC || RC) sdt[threadIdx.x] = dv;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    if (row >= a.row_end) return;
    if constexpr (RC) {  // the zero-guess iterate d*x per column (vec_mul's product)
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 2; j++) xs7[i][j] = sdt[ks7[i][j]] * xs7[i][j];
#pragma unroll
        for (int j = 0; j < 4; j++) xq[0][j] = sdt[kq[j]] * xq[0][j];
    }
    if constexpr (RK) {  // the same product with the one value of d
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 2; j++) xs7[i][j] = dk * xs7[i][j];
#pragma unroll
        for (int j = 0; j < 4; j++) xq[0][j] = dk * xq[0][j];
    }
    if constexpr (JK) ep.dr = dbl2_t{dk, dk};
    double acc0 = 0.0, acc1 = 0.0;
    if constexpr (NR == -1 && CST) {
        // diagonals z-1, y-1, x-1, 0, x+1, y+1, z+1; the row pair shares its grid row
        const int q = row / a.gnx, gx = row - q * a.gnx;
        const int gz = q / a.gny, gy = q - gz * a.gny;
        const bool zlo = gz > 0, ylo = gy > 0, yhi = gy < a.gny - 1, zhi = gz < a.gnz - 1;
        const bool xlo = gx > 0, xhi = gx + 2 < a.gnx;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const double y0 = k < 2 ? xs7[k][0] : k < 5 ? xq[0][k - 2] : xs7[k - 3][0];
            const double y1 = k < 2 ? xs7[k][1] : k < 5 ? xq[0][k - 1] : xs7[k - 3][1];
            const bool in = k == 0 ? zlo : k == 1 ? ylo : k == 5 ? yhi : k == 6 ? zhi : true;
            const bool in0 = in && (k != 2 || xlo), in1 = in && (k != 4 || xhi);
            acc0 = fma(a.cst[k], in0 ? y0 : 0.0, acc0);
            acc1 = fma(a.cst[k], in1 ? y1 : 0.0, acc1);
        }
    } else if constexpr (NR == -1) {
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const double y0 = k < 2 ? xs7[k][0] : k < 5 ? xq[0][k - 2] : xs7[k - 3][0];
            const double y1 = k < 2 ? xs7[k][1] : k < 5 ? xq[0][k - 1] : xs7[k - 3][1];
            acc0 = fma(stab[(w0[(k * VB) >> 5] >> ((k * VB) & 31)) & MASK], y0, acc0);
            acc1 = fma(stab[(w1[(k * VB) >> 5] >> ((k * VB) & 31)) & MASK], y1, acc1);
        }
    } else if constexpr (NR > 0) {
#pragma unroll
        for (int k = 0; k < 3 * NR; k++) {
            acc0 = fma(stab[(w0[(k * VB) >> 5] >> ((k * VB) & 31)) & MASK], xq[k / 3][k % 3], acc0);
            acc1 = fma(stab[(w1[(k * VB) >> 5] >> ((k * VB) & 31)) & MASK], xq[k / 3][k % 3 + 1], acc1);
        }
    } else {
#pragma unroll
        for (int k = 0; k < KMAX; k++) {
            const double f0 = fma(stab[(w0[(k * VB) >> 5] >> ((k * VB) & 31)) & MASK], x0[k], acc0);
            const double f1 = fma(stab[(w1[(k * VB) >> 5] >> ((k * VB) & 31)) & MASK], x1[k], acc1);
            acc0 = k < a.k ? f0 : acc0;
            acc1 = k < a.k ? f1 : acc1;
        }
    }
    ep.store(a.e, sdt, acc0, acc1);
}

// The constant 7-point kernel (CST above) with RP row pairs per lane (FLAG_DIA7_RP:
// 0 auto = 2 for SET, or 2 / 4): a workgroup covers RP adjacent 512-row blocks and issues every load
// of all its row pairs before the first sum -- RP times the bytes in flight per
// wave, fewer and longer-lived workgroups.  Same sums and epilogues, bitwise.
// (Coded-diagonal epilogues, which stage a table in LDS, stay on the kernel above.)
template <int MODE, int RP>
__global__ __launch_bounds__(256) void spmv_dia7c_kernel(DiaArgs a) {
    constexpr bool JK = MODE == DIA_JACOBI_DK, RK = MODE == DIA_RESID0_DK;
    constexpr int GM = JK ? SPMV_JACOBI : RK ? SPMV_SET : MODE;
    int blk;
    if (a.band_bp > 0) {  // the 2.5-D band order in units of RP blocks
        const int bp = a.band_bp / RP, bb = bp >> 3, x = blockIdx.x & 7, i = blockIdx.x >> 3;
        blk = (i / bb) * bp + x * bb + (i % bb);
    } else {
        blk = xcd_remap(blockIdx.x, gridDim.x);
    }
    DiaEpi<MODE, false> ep[RP];
    double xs7[RP][4][2], xq[RP][4];
    int row[RP];
#pragma unroll
    for (int p = 0; p < RP; p++) {
        row[p] = a.row_begin + 512 * (RP * blk + p) + 2 * (int)threadIdx.x;
        ep[p].load(a.e, row[p], a.row_end);
        dia_gx2<GM>(a.e, row[p] + a.off[0], a.ncols, xs7[p][0][0], xs7[p][0][1]);
        dia_gx2<GM>(a.e, row[p] + a.off[1], a.ncols, xs7[p][1][0], xs7[p][1][1]);
        dia_gx4<GM>(a.e, row[p] + a.off[2], a.ncols, xq[p]);
        dia_gx2<GM>(a.e, row[p] + a.off[5], a.ncols, xs7[p][2][0], xs7[p][2][1]);
        dia_gx2<GM>(a.e, row[p] + a.off[6], a.ncols, xs7[p][3][0], xs7[p][3][1]);
    }
#pragma unroll
    for (int p = 0; p < RP; p++) {
        if (row[p] >= a.row_end) break;  // the row pairs ascend
        if constexpr (RK) {
            const double dk = a.e.dk;
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) xs7[p][i][j] = dk * xs7[p][i][j];
#pragma unroll
            for (int j = 0; j < 4; j++) xq[p][j] = dk * xq[p][j];
        }
        if constexpr (JK) ep[p].dr = dbl2_t{a.e.dk, a.e.dk};
        const int q = row[p] / a.gnx, gx = row[p] - q * a.gnx;
        const int gz = q / a.gny, gy = q - gz * a.gny;
        const bool zlo = gz > 0, ylo = gy > 0, yhi = gy < a.gny - 1, zhi = gz < a.gnz - 1;
        const bool xlo = gx > 0, xhi = gx + 2 < a.gnx;
        double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const double y0 = k < 2 ? xs7[p][k][0] : k < 5 ? xq[p][k - 2] : xs7[p][k - 3][0];
            const double y1 = k < 2 ? xs7[p][k][1] : k < 5 ? xq[p][k - 1] : xs7[p][k - 3][1];
            const bool in = k == 0 ? zlo : k == 1 ? ylo : k == 5 ? yhi : k == 6 ? zhi : true;
            const bool in0 = in && (k != 2 || xlo), in1 = in && (k != 4 || xhi);
            acc0 = fma(a.cst[k], in0 ? y0 : 0.0, acc0);
            acc1 = fma(a.cst[k], in1 ? y1 : 0.0, acc1);
        }
        ep[p].store(a.e, nullptr, acc0, acc1);
    }
}

// Run patterns of longer stencils (more than 32 diagonals): the lengths of the
// runs of consecutive offsets, ascending.  PAT 33: the Galerkin operator of
// smoothed aggregation on 2^3 boxes of the 7-point operator (A_1 of the C2
// cycle: the 27 neighbours in {-1,0,1}^3 plus +-2 along each axis) --
// z-2 | three x runs in z-1 | y-2 | x run | x run of five | x run | y+2 |
// three x runs in z+1 | z+2.
// PAT 27: the 27-point stencil, nine x runs of three.
__host__ __device__ constexpr int dia_pat_nrun(int pat) { return pat == 33 ? 13 : pat == 27 ? 9 : 0; }
__host__ __device__ constexpr int dia_pat_len(int pat, int j) {
    return pat == 33 ? (j == 0 || j == 4 || j == 8 || j == 12 ? 1 : j == 6 ? 5 : 3) : pat == 27 ? 3 : 0;
}
__host__ __device__ constexpr int dia_pat_k(int pat) {
    int s = 0;
    for (int j = 0; j < dia_pat_nrun(pat); j++) s += dia_pat_len(pat, j);
    return s;
}
// x registers of run j for a row pair: L + 1 values from (L + 2) / 2 16-B loads
__host__ __device__ constexpr int dia_pat_nq(int pat, int j) { return (dia_pat_len(pat, j) + 2) / 2; }
__host__ __device__ constexpr int dia_pat_nv(int pat) {
    int s = 0;
    for (int j = 0; j < dia_pat_nrun(pat); j++) s += 2 * dia_pat_nq(pat, j);
    return s;
}

// The DIA kernel for a run pattern: two rows per lane as spmv_dia_kernel; run
// j (L diagonals, first offset o) reads x[c .. c+L] of the row pair (c = row +
// o) with (L+2)/2 16-B loads at clamp(c + 2q); value c + i sits in load i/2
// (low half iff it is the load's clamped position), exact for every in-range
// column (out-of-range ones belong to +0.0 terms and read some finite x).
// Codes: cw words per row (not a power of two), the row pair's 2 cw words
// loaded as 16-B + 8-B + 4-B pieces.  Row sums over the K diagonals in
// ascending order, as the other DIA kernels.
template <int GM, int PAT, bool CLAMP>
__device__ __forceinline__ void dia_pat_loads(const DiaArgs &a, int row, double (&xv)[dia_pat_nv(PAT)]) {
    int kd = 0, vo = 0;
#pragma unroll
    for (int j = 0; j < dia_pat_nrun(PAT); j++) {
        const int c = row + a.off[kd];
#pragma unroll
        for (int q = 0; q < dia_pat_nq(PAT, j); q++) {
            const int p = CLAMP ? min(max(c + 2 * q, 0), a.ncols - 2) : c + 2 * q;
            dbl2_t v = *reinterpret_cast<const dbl2u_t *>(a.e.x + p);
            if constexpr (GM == SPMV_RESID0) v = *reinterpret_cast<const dbl2u_t *>(a.e.d + p) * v;
            if constexpr (CLAMP) {
                xv[vo + 2 * q] = c + 2 * q == p ? v.x : v.y;
                xv[vo + 2 * q + 1] = c + 2 * q + 1 == p ? v.x : v.y;
            } else {
                xv[vo + 2 * q] = v.x;
                xv[vo + 2 * q + 1] = v.y;
            }
        }
        kd += dia_pat_len(PAT, j);
        vo += 2 * dia_pat_nq(PAT, j);
    }
}

// CST (PAT 27, dia_constant): no codes; the interior coefficients from the
// arguments and the x operands of neighbours outside the grid taken as 0.0 (the
// coded rows hold the +0.0 code there: the same products up to the sign of a
// zero, added to an accumulator that is never -0.0 -- bitwise equal)
template <int MODE, int VB, int CW, int PAT, bool CST = false>
__global__ __launch_bounds__(256) void spmv_dia_pat_kernel(DiaArgs a) {
    constexpr bool DC = MODE == DIA_JACOBI_DC;
    constexpr int GM = DC ? SPMV_JACOBI : MODE;
    constexpr int NRUN = dia_pat_nrun(PAT), NV = dia_pat_nv(PAT);
    constexpr uint32_t MASK = (1u << VB) - 1;
    static_assert(dia_pat_k(PAT) * VB <= 32 * CW, "code words too short for the pattern");
    __shared__ double stab[VB == 4 ? 16 : 256];
    __shared__ double sdt[DC ? 256 : 1];
    const double tv = (int)threadIdx.x < a.ntab ? a.vtab[threadIdx.x] : 0.0;
    double dv = 0.0;
    if constexpr (DC) dv = a.e.dt[threadIdx.x];
    int blk;
    if (a.band_bp > 0) {
        const int bb = a.band_bp >> 3, x = blockIdx.x & 7, i = blockIdx.x >> 3;
        blk = (i / bb) * a.band_bp + x * bb + (i % bb);
    } else {
        blk = xcd_remap(blockIdx.x, gridDim.x);
    }
    const int row = a.row_begin + 512 * blk + 2 * (int)threadIdx.x;
    DiaEpi<MODE, false> ep;
    ep.load_codes(a.e, row, a.row_end);
    ep.load(a.e, row, a.row_end);
    uint32_t u[2 * CW];
    if constexpr (!CST) {
        const uint32_t *cp = a.codes + (int64_t)(min(row, a.row_end - 1) - a.code_row0) * CW;
#pragma unroll
        for (int q = 0; q < (2 * CW) / 4; q++) {
            const i32x4u_t v = __builtin_nontemporal_load(reinterpret_cast<const i32x4u_t *>(cp) + q);
#pragma unroll
            for (int j = 0; j < 4; j++) u[4 * q + j] = (uint32_t)v[j];
        }
        if constexpr ((2 * CW) % 4 >= 2) {
            const i32x2u_t v = __builtin_nontemporal_load(reinterpret_cast<const i32x2u_t *>(cp + (2 * CW) / 4 * 4));
            u[(2 * CW) / 4 * 4] = (uint32_t)v.x;
            u[(2 * CW) / 4 * 4 + 1] = (uint32_t)v.y;
        }
        if constexpr ((2 * CW) % 2 == 1) u[2 * CW - 1] = __builtin_nontemporal_load(cp + 2 * CW - 1);
    }
    double xv[NV];
    // a block whose x runs all lie inside [0, ncols) (all but the first and last
    // plane or two of blocks) loads them unclamped: no selects, fewer registers
    const int rb = a.row_begin + 512 * blk;
    if (rb + a.off[0] >= 0 && rb + 511 + a.off[dia_pat_k(PAT) - 1] + 1 <= a.ncols - 1)
        dia_pat_loads<GM, PAT, false>(a, row, xv);
    else
        dia_pat_loads<GM, PAT, true>(a, row, xv);
    if ((int)threadIdx.x < a.ntab) stab[threadIdx.x] = tv;
    if constexpr (DC) sdt[threadIdx.x] = dv;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    if (row >= a.row_end) return;
    double acc0 = 0.0, acc1 = 0.0;
    if constexpr (CST) {
        static_assert(PAT == 27, "constant stencils: the 27-point pattern");
        const int q = row / a.gnx, gx = row - q * a.gnx;  // row even, nx even: the pair shares its grid row
        const int gz = q / a.gny, gy = q - gz * a.gny;
        const bool xlo = gx == 0, xhi = gx + 2 == a.gnx;
#pragma unroll
        for (int j = 0; j < 9; j++) {
            const int dz = j / 3 - 1, dy = j % 3 - 1;
            const bool ok = (unsigned)(gy + dy) < (unsigned)a.gny && (unsigned)(gz + dz) < (unsigned)a.gnz;
#pragma unroll
            for (int m = 0; m < 3; m++) {
                const int k = 3 * j + m;
                const double x0 = ok && !(m == 0 && xlo) ? xv[4 * j + m] : 0.0;
                const double x1 = ok && !(m == 2 && xhi) ? xv[4 * j + m + 1] : 0.0;
                acc0 = fma(a.cst[k], x0, acc0);
                acc1 = fma(a.cst[k], x1, acc1);
            }
        }
    } else {
        int kd = 0, vo = 0;
#pragma unroll
        for (int j = 0; j < NRUN; j++) {
#pragma unroll
            for (int m = 0; m < dia_pat_len(PAT, j); m++) {
                const int k = kd + m;
                acc0 = fma(stab[(u[(k * VB) >> 5] >> ((k * VB) & 31)) & MASK], xv[vo + m], acc0);
                acc1 = fma(stab[(u[CW + ((k * VB) >> 5)] >> ((k * VB) & 31)) & MASK], xv[vo + m + 1], acc1);
            }
            kd += dia_pat_len(PAT, j);
            vo += 2 * dia_pat_nq(PAT, j);
        }
    }
    ep.store(a.e, sdt, acc0, acc1);
}

// The run pattern of a sorted offset list (0: none of the patterns above)
static int dia_pattern_of(const std::vector<int> &offs) {
    std::vector<int> len;
    for (size_t k = 0; k < offs.size(); k++) {
        if (k > 0 && offs[k] == offs[k - 1] + 1) len.back()++;
        else len.push_back(1);
    }
    for (int pat : {33, 27}) {
        if ((int)len.size() != dia_pat_nrun(pat)) continue;
        bool ok = true;
        for (int j = 0; ok && j < dia_pat_nrun(pat); j++) ok = len[j] == dia_pat_len(pat, j);
        if (ok) return pat;
    }
    return 0;
}

// One SGS color update with DIA codes of the color-permuted copy: stored row p
// (one per lane, rows of one color contiguous) is original row i = rowid[p];
// x[i] <- x[i] + d[p] (b[i] - sum_k a_k x[i + off_k]) in place (rows of one
// color never couple).  Loads branch-free as in spmv_dia_kernel; padding
// entries (code of +0.0) read a clamped in-range x and add exact zeros.
// NR > 0: nine runs of three consecutive offsets (27-point stencil), each run's
// x[c], x[c+1], x[c+2] from one 16-B and one 8-B load (18 loads instead of 32).
template <int VB, int CW, int NR = 0>
__global__ __launch_bounds__(256) void spmv_dia_sgs_kernel(DiaArgs a, const int32_t *rowid) {
    __shared__ double stab[VB == 4 ? 16 : 256];
    const double tv = (int)threadIdx.x < a.ntab ? a.vtab[threadIdx.x] : 0.0;
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const int p = a.row_begin + 256 * blk + (int)threadIdx.x;
    const int pc = min(p, a.row_end - 1);
    constexpr int KMAX = CW * 32 / VB < DIA_MAX ? CW * 32 / VB : DIA_MAX;
    constexpr uint32_t MASK = (1u << VB) - 1;
    uint32_t w[CW];
    const uint32_t *cp = a.codes + (int64_t)(pc - a.code_row0) * CW;
    if constexpr (CW == 1) {
        w[0] = __builtin_nontemporal_load(cp);
    } else if constexpr (CW == 2) {
        const i32x2_t v = __builtin_nontemporal_load(reinterpret_cast<const i32x2_t *>(cp));
        w[0] = (uint32_t)v.x;
        w[1] = (uint32_t)v.y;
    } else {
#pragma unroll
        for (int q = 0; q < CW / 4; q++) {
            const i32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const i32x4_t *>(cp) + q);
#pragma unroll
            for (int j = 0; j < 4; j++) w[4 * q + j] = (uint32_t)v[j];
        }
    }
    const int i = rowid[pc];
    const double xr = a.e.x[i], br = a.e.b[i], dr = a.e.d[pc];
    constexpr int KX = NR > 0 ? 3 * NR : KMAX;
    double xv[KX];
    if constexpr (NR > 0) {
#pragma unroll
        for (int j = 0; j < NR; j++) {
            const int c = i + a.off[3 * j];
            const int p0 = min(max(c, 0), a.ncols - 2);
            const dbl2_t q = *reinterpret_cast<const dbl2u_t *>(a.e.x + p0);
            const double s2 = a.e.x[min(max(c + 2, 0), a.ncols - 1)];
#pragma unroll
            for (int u = 0; u < 3; u++) {
                const int t = c + u;
                xv[3 * j + u] = t == p0 ? q.x : t == p0 + 1 ? q.y : s2;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < KMAX; k++) xv[k] = a.e.x[min(max(i + a.off[k], 0), a.ncols - 1)];
    }
    if ((int)threadIdx.x < a.ntab) stab[threadIdx.x] = tv;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    if (p >= a.row_end) return;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < KX; k++) {
        const double f = fma(stab[(w[(k * VB) >> 5] >> ((k * VB) & 31)) & MASK], xv[k], acc);
        acc = (NR > 0 || k < a.k) ? f : acc;
    }
    a.e.y[i] = xr + dr * (br - acc);
}

// ---- DIA build
constexpr int DIA_SLOTS = 256;
constexpr int DIA_EMPTY = INT32_MIN;

// rowid (optional): stored row p is the original row rowid[p] (a color-permuted
// SGS copy); offsets are taken against the original row
__global__ __launch_bounds__(256) void k_dia_offsets(const int64_t *rp, const int32_t *col, int64_t r0, int64_t r1,
                                                     const int32_t *rowid, int *slots, unsigned int *cnt) {
    const int64_t i = r0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= r1) return;
    const int64_t ri = rowid ? rowid[i] : i;
    for (int64_t e = rp[i]; e < rp[i + 1]; e++) {
        const int64_t o64 = (int64_t)col[e] - ri;
        if (o64 <= INT32_MIN / 2 || o64 >= INT32_MAX / 2) {
            atomicAdd(cnt, (unsigned)DIA_SLOTS);
            return;
        }
        const int o = (int)o64;
        unsigned h = ((unsigned)o * 2654435761u) >> 24;
        for (int p = 0; p < DIA_SLOTS; p++, h = (h + 1) & (DIA_SLOTS - 1)) {
            int cur = slots[h];
            if (cur == o) break;
            if ((cur == DIA_EMPTY || p >= 8) && *(volatile unsigned *)cnt > (unsigned)DIA_MAX) return;
            if (cur == DIA_EMPTY) {
                cur = atomicCAS(&slots[h], DIA_EMPTY, o);
                if (cur == DIA_EMPTY) {
                    atomicAdd(cnt, 1u);
                    break;
                }
                if (cur == o) break;
            }
        }
    }
}

// codes of row i (rows >= n: padding, all +0.0)
__global__ __launch_bounds__(256) void k_dia_fill(const int64_t *rp, const int32_t *col, const double *val,
                                                  int64_t r0, int64_t r1, int64_t nrows_alloc, const int32_t *rowid,
                                                  DiaArgs off, int vb, int cw, const unsigned long long *tab, int ntab,
                                                  int zero_code, uint32_t *codes) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nrows_alloc) return;
    const int64_t i = r0 + j;
    int c[DIA_MAX];
    for (int k = 0; k < off.k; k++) c[k] = zero_code;
    if (i < r1) {
        const int64_t ri = rowid ? rowid[i] : i;
        for (int64_t e = rp[i]; e < rp[i + 1]; e++) {
            const int o = (int)((int64_t)col[e] - ri);
            int k = 0;
            while (off.off[k] != o) k++;
            const unsigned long long bits = (unsigned long long)__double_as_longlong(val[e]);
            int lo = 0, hi = ntab - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (tab[mid] < bits) lo = mid + 1;
                else hi = mid;
            }
            c[k] = lo;
        }
    }
    for (int q = 0; q < cw; q++) {
        uint32_t wd = 0;
        for (int k = 0; k < off.k; k++)
            if ((k * vb) >> 5 == q) wd |= (uint32_t)c[k] << ((k * vb) & 31);
        codes[j * cw + q] = wd;
    }
}

// DIA codes storage for rows [r0, r1) of m (auto policy, square, >= SELL_MIN_ROWS
// rows, 4/8-bit value table, <= DIA_MAX diagonals filled to >= 80 %).  Returns
// true if built.
bool build_dia(GpuCsr &m, int vb, const std::vector<unsigned long long> &tab, const std::vector<int64_t> &rp,
               int64_t r0, int64_t r1, const int32_t *rowid) {
    const int64_t nr = r1 - r0;
    // a rectangular matrix qualifies only through a row segment (the halo
    // interior of a distributed level: [owned | ghost] columns); every stored
    // entry's column is row + off, so only padding entries are clamped
    const bool square_or_segment = m.nrows == m.ncols || (m.seg_rows.size() > 2 && m.ncols >= m.nrows);
    if (g_spmv_format_policy != 0 || (vb != 4 && vb != 8) || !square_or_segment || nr < SELL_MIN_ROWS ||
        m.ncols >= (int64_t(1) << 30))
        return false;
    hipStream_t s = m.ctx->stream;
    DevBuf<int> slots(DIA_SLOTS);
    DevBuf<unsigned int> cnt(1);
    std::vector<int> hs(DIA_SLOTS, DIA_EMPTY);
    FAMG_CHECK_HIP(hipMemcpyAsync(slots.get(), hs.data(), DIA_SLOTS * sizeof(int), hipMemcpyHostToDevice, s));
    FAMG_CHECK_HIP(hipMemsetAsync(cnt.get(), 0, sizeof(unsigned int), s));
    hipLaunchKernelGGL(k_dia_offsets, dim3((unsigned)ceil_div(nr, 256)), dim3(256), 0, s, m.rp64.get(),
                       m.col.get(), r0, r1, rowid, slots.get(), cnt.get());
    FAMG_CHECK_HIP(hipGetLastError());
    unsigned int c = 0;
    FAMG_CHECK_HIP(hipMemcpyAsync(hs.data(), slots.get(), DIA_SLOTS * sizeof(int), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipMemcpyAsync(&c, cnt.get(), sizeof(c), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    if (c > (unsigned)DIA_MAX) return false;
    std::vector<int> offs;
    for (int o : hs)
        if (o != DIA_EMPTY) offs.push_back(o);
    std::sort(offs.begin(), offs.end());
    const int K = (int)offs.size();
    if (K == 0 || (int64_t)K * nr * 4 > (rp[r1] - rp[r0]) * 5) return false;  // >= 80 % filled
    // more than 32 diagonals: only a run pattern's kernel (no SGS sweep)
    const int pat = K > 32 && dia_pat_enabled() ? dia_pattern_of(offs) : 0;
    if (K > 32 && (rowid || pat == 0)) return false;
    const int bits = K * vb;
    int cw = 1;
    if (pat) cw = (bits + 31) / 32;
    else
        while (cw * 32 < bits) cw *= 2;
    DiaArgs oa{};
    oa.k = K;
    for (int k = 0; k < K; k++) oa.off[k] = offs[k];
    const int zero_code = (int)(std::lower_bound(tab.begin(), tab.end(), 0ull) - tab.begin());
    const int64_t nalloc = nr + 2;
    m.dia.codes.resize(nalloc * cw);
    m.dia.vtab.resize(tab.size());
    FAMG_CHECK_HIP(hipMemcpyAsync(m.dia.vtab.get(), tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_dia_fill, dim3((unsigned)ceil_div(nalloc, 256)), dim3(256), 0, s, m.rp64.get(), m.col.get(),
                       m.val.get(), r0, r1, nalloc, rowid, oa, vb, cw,
                       reinterpret_cast<const unsigned long long *>(m.dia.vtab.get()), (int)tab.size(), zero_code,
                       m.dia.codes.get());
    FAMG_CHECK_HIP(hipGetLastError());
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    m.dia.k = K;
    m.dia.cw = cw;
    m.dia.off = offs;
    m.dia.r0 = r0;
    m.dia.r1 = r1;
    m.dia.vbits = vb;
    m.dia.ntab = (int64_t)tab.size();
    m.dia.rowid = rowid;
    m.dia.pat = pat;
    return true;
}

// DIA codes of a color-permuted SGS copy (rows grouped by color, columns in the
// original numbering): diagonals are col - rowid[p].  Used only by the SGS
// sweep; the copy's other storage stays as chosen.
bool build_dia_sgs(GpuCsr &m, const int32_t *rowid) {
    if (g_spmv_format_policy != 0 || !g_value_codes || m.nrows == 0 || m.nrows != m.ncols) return false;
    std::vector<int64_t> rp(m.nrows + 1);
    FAMG_CHECK_HIP(hipMemcpyAsync(rp.data(), m.rp64.get(), (m.nrows + 1) * sizeof(int64_t), hipMemcpyDeviceToHost,
                                  m.ctx->stream));
    FAMG_CHECK_HIP(hipStreamSynchronize(m.ctx->stream));
    std::vector<unsigned long long> tab;
    const int vb = csr_value_table(m, tab);
    DiaStore keep = std::move(m.dia);  // a segment DIA the finalize may have built
    if (!build_dia(m, vb, tab, rp, 0, m.nrows, rowid)) {
        m.dia = std::move(keep);
        return false;
    }
    m.dia.seg = -2;  // not a row segment of the plain SpMV
    return true;
}

template <int M, int VB, int CW>
static void launch_dia(int runs, bool nt, dim3 grid, dim3 block, hipStream_t s, const DiaArgs &a, bool cst = false) {
    if constexpr (CW * 32 / VB >= 7) {
        if (runs == -1 && cst) {  // constant 7-point stencil: no codes
            if constexpr (M != DIA_JACOBI_DC && M != DIA_RESID0_DC) {
                // auto (0): two pairs for SET (the solve loops' operator apply: 52.3 -> 49.0 us on
                // 256^3), one for the cycle's RESID0 / JACOBI (in-cycle 65.9 -> 74.3 and
                // 84.6 -> 89.4 us with two: profiles/r05/ab_dia7_rp.txt)
                int rp = (int)flag(FLAG_DIA7_RP);
                if (rp == 0) rp = M == SPMV_SET ? 2 : 1;
                if (rp > 1 && (a.band_bp == 0 || a.band_bp % (8 * rp) == 0)) {
                    const dim3 g((unsigned)ceil_div((int64_t)grid.x, rp));
                    if (rp == 2) spmv_dia7c_kernel<M, 2><<<g, block, 0, s>>>(a);
                    else spmv_dia7c_kernel<M, 4><<<g, block, 0, s>>>(a);
                    return;
                }
            }
            spmv_dia_kernel<M, VB, CW, false, -1, true><<<grid, block, 0, s>>>(a);
            return;
        }
    }
    if constexpr (M == DIA_JACOBI_DK || M == DIA_RESID0_DK) {  // chosen only for the 7-point run kernel
        if constexpr (CW * 32 / VB >= 7) {
            if (runs == -1) {
                spmv_dia_kernel<M, VB, CW, false, -1><<<grid, block, 0, s>>>(a);
                return;
            }
        }
        fail(AMG_ERR_INVALID, "DIA: constant-diagonal epilogue outside the 7-point run kernel");
    } else {
    if constexpr (CW * 32 / VB >= 27) {
        if (runs == 9) {
            spmv_dia_kernel<M, VB, CW, false, 9><<<grid, block, 0, s>>>(a);
            return;
        }
    }
    if constexpr (CW * 32 / VB >= 7) {
        if (runs == -1) {
            spmv_dia_kernel<M, VB, CW, false, -1><<<grid, block, 0, s>>>(a);
            return;
        }
    }
    if (nt) spmv_dia_kernel<M, VB, CW, true><<<grid, block, 0, s>>>(a);
    else spmv_dia_kernel<M, VB, CW, false><<<grid, block, 0, s>>>(a);
    }
}

// The 27-point run pattern (nine runs of three consecutive offsets) and the
// 7-point one (single, single, run of three, single, single) of the DIA kernels
static bool dia_run9(const GpuCsr &m) {
    bool runs9 = m.dia.k == 27 && dia_runs();
    for (int j = 0; runs9 && j < 9; j++)
        runs9 = m.dia.off[3 * j + 1] == m.dia.off[3 * j] + 1 && m.dia.off[3 * j + 2] == m.dia.off[3 * j] + 2;
    return runs9;
}
static bool dia_run7(const GpuCsr &m) {
    return m.dia.k == 7 && dia_runs7() && m.dia.off[3] == m.dia.off[2] + 1 && m.dia.off[4] == m.dia.off[2] + 2;
}

// JACOBI / RESID0 with a coded diagonal of one value on the 7-point DIA kernel:
// d is dt[0], no codes are read
static bool dia_dk(const GpuCsr &m, const SpmvEpi &epi) { return epi_dconst(epi) && !m.dia.pat && dia_run7(m); }

bool dia7_cst_dk(const GpuCsr &m, const SpmvEpi &epi) {
    return m.kernel == SPMV_KERNEL_DIA && m.dia.cst && m.dia.k == 7 && dia_cst_enabled() && dia_dk(m, epi) &&
           m.dia.vbits > 0 && m.dia.cw * 32 / m.dia.vbits >= 7 &&
           m.nrows == (int64_t)m.dia.cst_n[0] * m.dia.cst_n[1] * m.dia.cst_n[2];
}

// The DIA part of a route (spmv_route chose ROUTE_DIA or ROUTE_DIA_SGS): which of
// the kernels above the launch takes
void dia_route(const GpuCsr &m, const SpmvEpi &epi, SpmvRoute &r) {
    r.kernel = SPMV_KERNEL_DIA;
    r.runs = dia_run9(m) ? 9 : dia_run7(m) ? -1 : 0;
    if (r.to == ROUTE_DIA_SGS) {
        r.name = "dia_sgs";
        return;
    }
    const int key = m.dia.vbits * 16 + m.dia.cw;
    r.pat = m.dia.pat ? m.dia.pat : r.runs == 9 && dia_pat27() && (key == 4 * 16 + 4 || key == 8 * 16 + 8) ? 27 : 0;
    r.cst = m.dia.cst && r.seg < 0 && dia_cst_enabled() && (r.pat ? r.pat == 27 : r.runs == -1 && m.dia.k == 7);
    r.dk = dia_dk(m, epi);
    r.rc = epi.dc && dia_rc_enabled();
    r.name = r.pat ? "dia_pat" : "dia";
}

// The arguments every DIA launch shares: rows [r.r0, r.r1) of m
static DiaArgs dia_args(const GpuCsr &m, const double *x, double *y, const SpmvEpi &epi, const SpmvRoute &r) {
    DiaArgs a{};
    a.codes = m.dia.codes.get();
    a.ntab = (int32_t)m.dia.ntab;
    a.k = m.dia.k;
    a.row_begin = (int32_t)r.r0;
    a.row_end = (int32_t)r.r1;
    a.ncols = (int32_t)m.ncols;
    a.code_row0 = (int32_t)m.dia.r0;
    a.vtab = m.dia.vtab.get();
    for (int k = 0; k < m.dia.k; k++) a.off[k] = m.dia.off[k];
    a.e = Epi{x, y, epi.b, epi.d, epi.perm, epi.dc, epi.dt, epi.dk};
    if (r.cst) {
        a.gnx = m.dia.cst_n[0];
        a.gny = m.dia.cst_n[1];
        a.gnz = m.dia.cst_n[2];
        for (int k = 0; k < m.dia.k; k++) a.cst[k] = m.dia.cst_v[k];
    }
    return a;
}

// One color sweep of a color-permuted copy
void spmv_dia_sgs(const GpuCsr &m, const double *x, double *y, const SpmvEpi &epi, hipStream_t s,
                  const SpmvRoute &r) {
    FAMG_REQUIRE(epi.perm == m.dia.rowid, AMG_ERR_INVALID, "SGS DIA: permutation mismatch");
    if (r.r1 <= r.r0) return;
    const DiaArgs a = dia_args(m, x, y, epi, r);
    const dim3 grid((unsigned)ceil_div(r.r1 - r.r0, 256)), block(256);
    const int key = m.dia.vbits * 16 + m.dia.cw;
    if (r.runs == 9 && key == 4 * 16 + 4) {
        spmv_dia_sgs_kernel<4, 4, 9><<<grid, block, 0, s>>>(a, m.dia.rowid);
    } else if (r.runs == 9 && key == 8 * 16 + 8) {
        spmv_dia_sgs_kernel<8, 8, 9><<<grid, block, 0, s>>>(a, m.dia.rowid);
    } else {
        switch (key) {
        case 4 * 16 + 1: spmv_dia_sgs_kernel<4, 1><<<grid, block, 0, s>>>(a, m.dia.rowid); break;
        case 4 * 16 + 2: spmv_dia_sgs_kernel<4, 2><<<grid, block, 0, s>>>(a, m.dia.rowid); break;
        case 4 * 16 + 4: spmv_dia_sgs_kernel<4, 4><<<grid, block, 0, s>>>(a, m.dia.rowid); break;
        case 8 * 16 + 1: spmv_dia_sgs_kernel<8, 1><<<grid, block, 0, s>>>(a, m.dia.rowid); break;
        case 8 * 16 + 2: spmv_dia_sgs_kernel<8, 2><<<grid, block, 0, s>>>(a, m.dia.rowid); break;
        case 8 * 16 + 4: spmv_dia_sgs_kernel<8, 4><<<grid, block, 0, s>>>(a, m.dia.rowid); break;
        case 8 * 16 + 8: spmv_dia_sgs_kernel<8, 8><<<grid, block, 0, s>>>(a, m.dia.rowid); break;
        default: fail(AMG_ERR_INVALID, "SGS DIA: unsupported code layout");
        }
    }
    FAMG_CHECK_HIP(hipGetLastError());
}

// The whole matrix, or its DIA row segment (the halo interior of a distributed
// level runs DIA even when the rest of the matrix is SELL storage)
void spmv_dia(const GpuCsr &m, const double *x, double *y, SpmvMode mode, const SpmvEpi &epi, hipStream_t s,
              const SpmvRoute &r) {
    if (r.r1 <= r.r0) return;
    DiaArgs a = dia_args(m, x, y, epi, r);
    {  // plane = the largest diagonal offset (a 3-D stencil's z neighbour)
        const int64_t plane = std::max<int64_t>(std::abs((int64_t)m.dia.off.front()), std::abs((int64_t)m.dia.off.back()));
        if (dia_bands() && plane % 4096 == 0 && plane >= 8 * 4096 && (r.r1 - r.r0) % plane == 0)
            a.band_bp = (int32_t)(plane / 512);
    }
    const dim3 grid((unsigned)ceil_div(r.r1 - r.r0, 512)), block(256);
    const int key = m.dia.vbits * 16 + m.dia.cw;
    if (r.pat) {
#define FAMG_DIAP2(M, VB, CW, P)                                                                  \
    if (r.cst) spmv_dia_pat_kernel<M, VB, CW, P, (P == 27)><<<grid, block, 0, s>>>(a);            \
    else spmv_dia_pat_kernel<M, VB, CW, P><<<grid, block, 0, s>>>(a);
#define FAMG_DIAP(VB, CW, P)                                                                        \
    switch (mode) {                                                                               \
    case SPMV_SET: FAMG_DIAP2(SPMV_SET, VB, CW, P) break;                                            \
    case SPMV_ADD: FAMG_DIAP2(SPMV_ADD, VB, CW, P) break;                                            \
    case SPMV_RESID: FAMG_DIAP2(SPMV_RESID, VB, CW, P) break;                                        \
    case SPMV_JACOBI:                                                                             \
        if (epi.dc) {                                                                             \
            FAMG_DIAP2(DIA_JACOBI_DC, VB, CW, P)                                                     \
        } else {                                                                                  \
            FAMG_DIAP2(SPMV_JACOBI, VB, CW, P)                                                       \
        }                                                                                         \
        break;                                                                                    \
    case SPMV_RESID0: FAMG_DIAP2(SPMV_RESID0, VB, CW, P) break;                                      \
    case SPMV_ADD0: FAMG_DIAP2(SPMV_ADD0, VB, CW, P) break;                                          \
    default: break;                                                                               \
    }
        FAMG_REQUIRE(r.pat == 33 || r.pat == 27, AMG_ERR_INVALID, "DIA: unsupported run pattern");
        if (r.pat == 33 && key == 8 * 16 + 9) {
            FAMG_DIAP(8, 9, 33)
        } else if (r.pat == 33 && key == 4 * 16 + 5) {
            FAMG_DIAP(4, 5, 33)
        } else if (r.pat == 27 && key == 8 * 16 + 8) {
            FAMG_DIAP(8, 8, 27)
        } else if (r.pat == 27 && key == 4 * 16 + 4) {
            FAMG_DIAP(4, 4, 27)
        } else {
            fail(AMG_ERR_INVALID, "DIA: unsupported code layout");
        }
#undef FAMG_DIAP
#undef FAMG_DIAP2
        FAMG_CHECK_HIP(hipGetLastError());
        return;
    }
#define FAMG_DIA2(M, VB, CW) launch_dia<M, VB, CW>(r.runs, dia_nt(), grid, block, s, a, r.cst);
#define FAMG_DIA(VB, CW)                                                                          \
    switch (mode) {                                                                               \
    case SPMV_SET: FAMG_DIA2(SPMV_SET, VB, CW) break;                                             \
    case SPMV_ADD: FAMG_DIA2(SPMV_ADD, VB, CW) break;                                             \
    case SPMV_RESID: FAMG_DIA2(SPMV_RESID, VB, CW) break;                                         \
    case SPMV_JACOBI:                                                                             \
        if (r.dk) {                                                                               \
            FAMG_DIA2(DIA_JACOBI_DK, VB, CW)                                                      \
        } else if (epi.dc) {                                                                      \
            FAMG_DIA2(DIA_JACOBI_DC, VB, CW)                                                      \
        } else {                                                                                  \
            FAMG_DIA2(SPMV_JACOBI, VB, CW)                                                        \
        }                                                                                         \
        break;                                                                                    \
    case SPMV_RESID0:                                                                             \
        if (r.dk) {                                                                               \
            FAMG_DIA2(DIA_RESID0_DK, VB, CW)                                                      \
        } else if (r.rc) {                                                                        \
            FAMG_DIA2(DIA_RESID0_DC, VB, CW)                                                      \
        } else {                                                                                  \
            FAMG_DIA2(SPMV_RESID0, VB, CW)                                                        \
        }                                                                                         \
        break;                                                                                    \
    case SPMV_ADD0: FAMG_DIA2(SPMV_ADD0, VB, CW) break;                                           \
    default: break;                                                                               \
    }
    switch (key) {
    case 4 * 16 + 1: FAMG_DIA(4, 1) break;
    case 4 * 16 + 2: FAMG_DIA(4, 2) break;
    case 4 * 16 + 4: FAMG_DIA(4, 4) break;
    case 8 * 16 + 1: FAMG_DIA(8, 1) break;
    case 8 * 16 + 2: FAMG_DIA(8, 2) break;
    case 8 * 16 + 4: FAMG_DIA(8, 4) break;
    case 8 * 16 + 8: FAMG_DIA(8, 8) break;
    default: fail(AMG_ERR_INVALID, "DIA: unsupported code layout");
    }
#undef FAMG_DIA
#undef FAMG_DIA2
    FAMG_CHECK_HIP(hipGetLastError());
}

}  // namespace famg
