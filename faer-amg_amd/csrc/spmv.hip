// spmv.hip -- fp64 CSR SpMV for gfx950 with fused V-cycle epilogues.
//
// Replaces the reference's CPU SpMV (ParSpmmOp, par_spmm.rs:98-133, and faer's
// SparseRowMat LinOp used at multigrid.rs:137-158) and fuses the vector work of
// Multigrid::cycle / smooth (multigrid.rs:341-350, 407-424) into its epilogue.
//
// This file holds the storages that read the CSR arrays themselves, chosen per
// matrix when it is finalized (csr_finalize), and the dispatch over all storages:
//  * vector (very long rows, >= 256 entries on average: the densest Galerkin
//    operators near the coarsest level): one wavefront per row, lanes stride the
//    row four 64-entry steps at a time, shuffle-tree reduction.
//  * CSR-stream (everything else): blocks of <= 256 rows / <= 2048 entries
//    staged HBM -> LDS with 16-B non-temporal loads, L lanes per row.
//  * the value table (the distinct fp64 bit patterns of a matrix) the coded
//    storages are built from.
//  * spmv_route / spmv(): one route per launch, over these and the storages of
//    sell.hip, dia.hip, scs.hip, sellp.hip, xsell.hip, bsr.hip, gtc.hip, gtx.hip.
// Workgroups are remapped so that each XCD (blocks b and b+8 share one) walks a
// contiguous slab of rows: a slab's x window (3 planes of a 7-pt operator,
// ~1.5 MB at 256^3) then stays in that XCD's 4 MB L2.
// A matrix may be cut into row segments (SGS colors, halo boundary/interior);
// every kernel can run one segment.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "spmv_dev.hpp"

namespace famg {

int g_spmv_format_policy = 0;
int g_value_codes = 1;
int g_alloc_policy = 0;
int g_alloc_experiment = (int)env_int("FAMG_ALLOC_EXPERIMENT", 0);
bool g_alloc_debug = env_is_one("FAMG_ALLOC_DEBUG");

constexpr int SPMV_BS = 256;
constexpr int SPMV_CAP = 2048;

// ---------------------------------------------------------------- CSR-stream

struct StreamArgs {
    const int32_t *rowptr;
    const int32_t *col;
    const double *val;
    const int32_t *sched;
    int32_t nblocks;
    Epi e;
};

template <int MODE>
__global__ __launch_bounds__(SPMV_BS) void spmv_stream_kernel(StreamArgs a) {
    __shared__ __attribute__((aligned(16))) double sval[SPMV_CAP + 2];
    __shared__ __attribute__((aligned(16))) int32_t scol[SPMV_CAP + 4];
    __shared__ double sred[SPMV_BS / 64];

    const int blk = xcd_remap(blockIdx.x, a.nblocks);
    const int r0 = a.sched[blk], r1 = a.sched[blk + 1];
    const int e0 = a.rowptr[r0], e1 = a.rowptr[r1];
    const int tid = threadIdx.x;
    const int nnz = e1 - e0;

    if (nnz > SPMV_CAP) {  // one long row (r1 == r0 + 1): the whole workgroup reduces it
        double acc = 0.0;
        for (int k = e0 + tid; k < e1; k += SPMV_BS) acc = fma(a.val[k], gx<MODE>(a.e, a.col[k]), acc);
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if ((tid & 63) == 0) sred[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) {
            double s = sred[0];
            for (int w = 1; w < SPMV_BS / 64; w++) s += sred[w];
            EpiOps<MODE> ep;
            ep.load(a.e, r0);
            ep.store(a.e, s);
        }
        return;
    }
    const int nrows = r1 - r0;
    int L = 1;
    while (L < 64 && 2 * L * nrows <= SPMV_BS) L <<= 1;
    const int rl = tid / L;
    const int sub = tid & (L - 1);
    EpiOps<MODE> ep;
    if (rl < nrows && sub == 0) ep.load(a.e, r0 + rl);

    const int bv = e0 & ~1;
    const int nv = (e1 - bv + 1) >> 1;
    const dbl2_t *gv = reinterpret_cast<const dbl2_t *>(a.val + bv);
    dbl2_t *sv2 = reinterpret_cast<dbl2_t *>(sval);
    for (int k = tid; k < nv; k += SPMV_BS) sv2[k] = __builtin_nontemporal_load(gv + k);
    const int bc = e0 & ~3;
    const int nc = (e1 - bc + 3) >> 2;
    const i32x4_t *gc = reinterpret_cast<const i32x4_t *>(a.col + bc);
    i32x4_t *sc4 = reinterpret_cast<i32x4_t *>(scol);
    for (int k = tid; k < nc; k += SPMV_BS) sc4[k] = __builtin_nontemporal_load(gc + k);
    __syncthreads();

    const int vo = e0 - bv, co = e0 - bc;
    double acc = 0.0;
    if (rl < nrows) {
        const int rs = a.rowptr[r0 + rl] - e0;
        const int re = a.rowptr[r0 + rl + 1] - e0;
        for (int k = rs + sub; k < re; k += L) acc = fma(sval[vo + k], gx<MODE>(a.e, scol[co + k]), acc);
    }
    for (int off = L >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (rl < nrows && sub == 0) ep.store(a.e, acc);
}

// The same over kb columns (spmm_epi): the block's values and columns are staged
// in LDS once, then every column takes spmv_stream_kernel's row sums -- the same
// lanes per row, the same strided order, the same butterfly -- and its epilogue.
template <int MODE>
__global__ __launch_bounds__(SPMV_BS) void spmm_stream_kernel(StreamArgs a, int kb, int64_t ldx, int64_t ldy,
                                                              int64_t ldb) {
    __shared__ __attribute__((aligned(16))) double sval[SPMV_CAP + 2];
    __shared__ __attribute__((aligned(16))) int32_t scol[SPMV_CAP + 4];
    __shared__ double sred[SPMV_BS / 64];

    const int blk = xcd_remap(blockIdx.x, a.nblocks);
    const int r0 = a.sched[blk], r1 = a.sched[blk + 1];
    const int e0 = a.rowptr[r0], e1 = a.rowptr[r1];
    const int tid = threadIdx.x;
    const int nnz = e1 - e0;
    const Epi e0c = a.e;

    if (nnz > SPMV_CAP) {  // one long row: the whole workgroup reduces it, column after column
        for (int c = 0; c < kb; c++) {
            Epi e = e0c;
            e.x += c * ldx;
            e.y += c * ldy;
            if (e.b) e.b += c * ldb;
            double acc = 0.0;
            for (int k = e0 + tid; k < e1; k += SPMV_BS) acc = fma(a.val[k], gx<MODE>(e, a.col[k]), acc);
            for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
            if (c) __syncthreads();  // the previous column's sum has been read
            if ((tid & 63) == 0) sred[tid >> 6] = acc;
            __syncthreads();
            if (tid == 0) {
                double s = sred[0];
                for (int w = 1; w < SPMV_BS / 64; w++) s += sred[w];
                EpiOps<MODE> ep;
                ep.load(e, r0);
                ep.store(e, s);
            }
        }
        return;
    }
    const int nrows = r1 - r0;
    int L = 1;
    while (L < 64 && 2 * L * nrows <= SPMV_BS) L <<= 1;
    const int rl = tid / L;
    const int sub = tid & (L - 1);

    const int bv = e0 & ~1;
    const int nv = (e1 - bv + 1) >> 1;
    const dbl2_t *gv = reinterpret_cast<const dbl2_t *>(a.val + bv);
    dbl2_t *sv2 = reinterpret_cast<dbl2_t *>(sval);
    for (int k = tid; k < nv; k += SPMV_BS) sv2[k] = __builtin_nontemporal_load(gv + k);
    const int bc = e0 & ~3;
    const int nc = (e1 - bc + 3) >> 2;
    const i32x4_t *gc = reinterpret_cast<const i32x4_t *>(a.col + bc);
    i32x4_t *sc4 = reinterpret_cast<i32x4_t *>(scol);
    for (int k = tid; k < nc; k += SPMV_BS) sc4[k] = __builtin_nontemporal_load(gc + k);
    __syncthreads();

    const int vo = e0 - bv, co = e0 - bc;
    int rs = 0, re = 0;
    if (rl < nrows) {
        rs = a.rowptr[r0 + rl] - e0;
        re = a.rowptr[r0 + rl + 1] - e0;
    }
    for (int c = 0; c < kb; c++) {
        Epi e = e0c;
        e.x += c * ldx;
        e.y += c * ldy;
        if (e.b) e.b += c * ldb;
        EpiOps<MODE> ep;
        if (rl < nrows && sub == 0) ep.load(e, r0 + rl);
        double acc = 0.0;
        for (int k = rs + sub; k < re; k += L) acc = fma(sval[vo + k], gx<MODE>(e, scol[co + k]), acc);
        for (int off = L >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (rl < nrows && sub == 0) ep.store(e, acc);
    }
}

// --------------------------------------------------------------------- vector

struct VecArgs {
    const int32_t *rowptr;
    const int32_t *col;     // int32 columns (O16 == false)
    const int16_t *off;     // col = row + off (O16)
    const double *val;      // fp64 values (VB == 0)
    const void *codes;      // 8 / 16-bit value codes (VB == 8 / 16) into vtab
    const double *vtab;
    int32_t row_begin, nrows;
    Epi e;
};

// Value and column of entry k (CSR order) for the wave-per-row kernel: fp64 or
// a code into the value table; int32 or a 16-bit offset from the row.
template <int VB, bool O16>
__device__ __forceinline__ void vec_entry(const VecArgs &a, int row, int k, double &v, int32_t &c) {
    if constexpr (VB == 0) v = __builtin_nontemporal_load(a.val + k);
    else if constexpr (VB == 8) v = a.vtab[__builtin_nontemporal_load(static_cast<const uint8_t *>(a.codes) + k)];
    else v = a.vtab[__builtin_nontemporal_load(static_cast<const uint16_t *>(a.codes) + k)];
    if constexpr (O16) c = row + (int32_t)__builtin_nontemporal_load(a.off + k);
    else c = __builtin_nontemporal_load(a.col + k);
}

// WPR waves per row (1, 2, 4): a level with few long rows (A_4 of the box
// hierarchies: 4096 rows of ~1400 entries, R_4: 512 rows) has too few waves
// to keep the loads in flight with one wave per row; with WPR > 1 the row's
// 64-entry chunks are dealt round-robin to its waves and the wave sums are
// added in LDS (a different lane split: the sum is bounded, not bitwise).
template <int MODE, int VB, bool O16, int WPR>
__global__ __launch_bounds__(256) void spmv_vector_kernel(VecArgs a) {
    __shared__ double part[4];
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const int wv = threadIdx.x >> 6;
    const int w = blk * (4 / WPR) + wv / WPR;
    const int sub = wv % WPR;
    if constexpr (WPR == 1)
        if (w >= a.nrows) return;
    const bool ok = w < a.nrows;
    const int row = a.row_begin + (ok ? w : 0);
    const int lane = threadIdx.x & 63;
    EpiOps<MODE> ep;
    if (ok && lane == 0 && sub == 0) ep.load(a.e, row);
    const int e0 = ok ? a.rowptr[row] : 0, e1 = ok ? a.rowptr[row + 1] : 0;
    constexpr int S = 64 * WPR;
    double acc = 0.0;
    int k = e0 + sub * 64 + lane;
    for (; k + 3 * S < e1; k += 4 * S) {
        double vv[4];
        int32_t cc[4];
#pragma unroll
        for (int u = 0; u < 4; u++) vec_entry<VB, O16>(a, row, k + S * u, vv[u], cc[u]);
        double xx[4];
#pragma unroll
        for (int u = 0; u < 4; u++) xx[u] = gx<MODE>(a.e, cc[u]);
#pragma unroll
        for (int u = 0; u < 4; u++) acc = fma(vv[u], xx[u], acc);
    }
    for (; k < e1; k += S) {
        double v;
        int32_t c;
        vec_entry<VB, O16>(a, row, k, v, c);
        acc = fma(v, gx<MODE>(a.e, c), acc);
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if constexpr (WPR == 1) {
        if (lane == 0) ep.store(a.e, acc);
    } else {
        if (lane == 0) part[wv] = acc;
        __syncthreads();
        if (ok && lane == 0 && sub == 0) {
            double t = part[wv];
#pragma unroll
            for (int j = 1; j < WPR; j++) t += part[wv + j];
            ep.store(a.e, t);
        }
    }
}

// ------------------------------------------------------------ host: storage

// Greedy blocks of <= SPMV_BS rows and <= SPMV_CAP nonzeros per segment; a row
// longer than SPMV_CAP is a block of its own.
void build_schedule(const std::vector<int64_t> &rp, const std::vector<int64_t> &seg_bounds,
                    std::vector<int32_t> &sched, std::vector<int64_t> &seg_blocks) {
    sched.clear();
    seg_blocks.clear();
    sched.push_back(static_cast<int32_t>(seg_bounds.empty() ? 0 : seg_bounds[0]));
    seg_blocks.push_back(0);
    for (size_t s = 0; s + 1 < seg_bounds.size(); s++) {
        int64_t r0 = seg_bounds[s];
        const int64_t end = seg_bounds[s + 1];
        while (r0 < end) {
            int64_t r1;
            if (rp[r0 + 1] - rp[r0] > SPMV_CAP) {
                r1 = r0 + 1;
            } else {
                r1 = r0;
                while (r1 < end && r1 - r0 < SPMV_BS && rp[r1 + 1] - rp[r0] <= SPMV_CAP) r1++;
            }
            sched.push_back(static_cast<int32_t>(r1));
            r0 = r1;
        }
        seg_blocks.push_back(static_cast<int64_t>(sched.size()) - 1);
    }
}

// ---- value table: the distinct fp64 bit patterns of a matrix (open
// addressing; stops counting past VT_MAX)
constexpr int VT_MAX = 65536;
constexpr int VT_SLOTS = 2 * VT_MAX;
constexpr unsigned long long VT_EMPTY = ~0ull;  // a NaN payload: a matrix holding it keeps fp64 values

__global__ __launch_bounds__(256) void k_value_set(const double *val, int64_t nnz, unsigned long long *slots,
                                                   unsigned int *cnt) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nnz; k += stride) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(val[k]);
        if (b == VT_EMPTY) {
            atomicAdd(cnt, (unsigned)VT_SLOTS);
            return;
        }
        unsigned h = (unsigned)((b * 0x9E3779B97F4A7C15ull) >> 47) & (VT_SLOTS - 1);
        for (int p = 0; p < VT_SLOTS; p++, h = (h + 1) & (VT_SLOTS - 1)) {
            unsigned long long cur = slots[h];
            if (cur == b) break;
            if ((cur == VT_EMPTY || p >= 16) && *(volatile unsigned *)cnt > (unsigned)VT_MAX) return;
            if (cur == VT_EMPTY) {
                cur = atomicCAS(&slots[h], VT_EMPTY, b);
                if (cur == VT_EMPTY) {
                    atomicAdd(cnt, 1u);
                    break;
                }
                if (cur == b) break;
            }
        }
    }
}

// Code width for m's values (0 = keep fp64, 4, 8 or 16) and the table: the
// distinct bit patterns, +0.0 (padding) included, ascending as unsigned.
static int value_table_of(const double *val, int64_t nnz, hipStream_t s, std::vector<unsigned long long> &tab,
                          unsigned *found = nullptr) {
    tab.clear();
    DevBuf<unsigned long long> slots(VT_SLOTS);
    DevBuf<unsigned int> cnt(1);
    FAMG_CHECK_HIP(hipMemsetAsync(slots.get(), 0xff, VT_SLOTS * sizeof(unsigned long long), s));
    FAMG_CHECK_HIP(hipMemsetAsync(cnt.get(), 0, sizeof(unsigned int), s));
    const unsigned grid = (unsigned)std::min<int64_t>(4096, ceil_div(nnz, 256));
    hipLaunchKernelGGL(k_value_set, dim3(grid), dim3(256), 0, s, val, nnz, slots.get(), cnt.get());
    FAMG_CHECK_HIP(hipGetLastError());
    std::vector<unsigned long long> h(VT_SLOTS);
    unsigned int c = 0;
    FAMG_CHECK_HIP(hipMemcpyAsync(h.data(), slots.get(), VT_SLOTS * sizeof(unsigned long long),
                                  hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipMemcpyAsync(&c, cnt.get(), sizeof(c), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    if (found) *found = c;  // distinct values present (the table adds 0.0)
    if (c > (unsigned)VT_MAX) return 0;
    for (unsigned long long b : h)
        if (b != VT_EMPTY) tab.push_back(b);
    if (std::find(tab.begin(), tab.end(), 0ull) == tab.end()) tab.push_back(0ull);
    std::sort(tab.begin(), tab.end());
    if ((int64_t)tab.size() > VT_MAX) {
        tab.clear();
        return 0;
    }
    return tab.size() <= 16 ? 4 : tab.size() <= 256 ? 8 : 16;
}

int csr_value_table(const GpuCsr &m, std::vector<unsigned long long> &tab) {
    tab.clear();
    if (!g_value_codes || m.nnz == 0) return 0;
    return value_table_of(m.val.get(), m.nnz, m.ctx->stream, tab);
}

// ---- 8-bit codes of a vector (the Jacobi diagonal): table + codes, or 0
__global__ __launch_bounds__(256) void k_array_codes(const double *v, int64_t n, const unsigned long long *tab,
                                                     int ntab, uint8_t *code) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v[i]);
    int lo = 0, hi = ntab - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid] < bits) lo = mid + 1;
        else hi = mid;
    }
    code[i] = (uint8_t)lo;
}

int64_t array_codes_u8(const double *v, int64_t n, Ctx &ctx, DevBuf<uint8_t> &code, DevBuf<double> &table,
                       double *dconst) {
    code.release();
    table.release();
    if (dconst) *dconst = 0.0;
    if (!g_value_codes || n == 0) return 0;
    std::vector<unsigned long long> tab;
    unsigned found = 0;
    const int vb = value_table_of(v, n, ctx.stream, tab, &found);
    if (vb != 4 && vb != 8) return 0;
    if (dconst && found == 1)  // one value present (the table's other entry is the added 0.0)
        for (unsigned long long bits : tab)
            if (bits != 0ull) std::memcpy(dconst, &bits, 8);
    table.resize(256);  // padded: kernels stage all 256 entries without a bound
    FAMG_CHECK_HIP(hipMemsetAsync(table.get(), 0, 256 * sizeof(double), ctx.stream));
    code.resize(n + 2);
    FAMG_CHECK_HIP(hipMemcpyAsync(table.get(), tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice,
                                  ctx.stream));
    FAMG_CHECK_HIP(hipMemsetAsync(code.get(), 0, n + 2, ctx.stream));
    hipLaunchKernelGGL(k_array_codes, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx.stream, v, n,
                       reinterpret_cast<const unsigned long long *>(table.get()), (int)tab.size(), code.get());
    FAMG_CHECK_HIP(hipGetLastError());
    FAMG_CHECK_HIP(hipStreamSynchronize(ctx.stream));
    return (int64_t)tab.size();
}

// ---- wave-per-row storage: value codes (8/16-bit) and 16-bit row offsets
__global__ __launch_bounds__(256) void k_vec_maxoff(const int64_t *rp, const int32_t *col, int64_t n,
                                                    unsigned long long *mx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned long long m = 0;
    for (int64_t e = rp[i]; e < rp[i + 1]; e++) {
        const int64_t o = (int64_t)col[e] - i;
        const unsigned long long a = (unsigned long long)(o < 0 ? -o : o);
        m = a > m ? a : m;
    }
    atomicMax(mx, m);
}

__global__ __launch_bounds__(256) void k_vec_fill(const int64_t *rp, const int32_t *col, const double *val, int64_t n,
                                                  int vb, const unsigned long long *tab, int ntab, bool o16,
                                                  void *codes, int16_t *off) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int64_t e = rp[i]; e < rp[i + 1]; e++) {
        if (o16) off[e] = (int16_t)((int64_t)col[e] - i);
        if (vb) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(val[e]);
            int lo = 0, hi = ntab - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (tab[mid] < bits) lo = mid + 1;
                else hi = mid;
            }
            if (vb == 8) static_cast<uint8_t *>(codes)[e] = (uint8_t)lo;
            else static_cast<uint16_t *>(codes)[e] = (uint16_t)lo;
        }
    }
}

static void build_vec_codes(GpuCsr &m) {
    if (m.nnz == 0) return;
    hipStream_t s = m.ctx->stream;
    std::vector<unsigned long long> tab;
    int vb = csr_value_table(m, tab);
    if (vb == 4) vb = 8;
    DevBuf<unsigned long long> mx(1);
    FAMG_CHECK_HIP(hipMemsetAsync(mx.get(), 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_vec_maxoff, dim3((unsigned)ceil_div(m.nrows, 256)), dim3(256), 0, s, m.rp64.get(),
                       m.col.get(), m.nrows, mx.get());
    unsigned long long hmx = 0;
    FAMG_CHECK_HIP(hipMemcpyAsync(&hmx, mx.get(), sizeof(hmx), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    const bool o16 = g_value_codes && hmx <= 32767;
    if (!vb && !o16) return;
    if (vb) {
        m.vec.vtab.resize(tab.size());
        FAMG_CHECK_HIP(hipMemcpyAsync(m.vec.vtab.get(), tab.data(), tab.size() * sizeof(double),
                                      hipMemcpyHostToDevice, s));
        m.vec.codes.resize(m.nnz * (vb / 8));
    }
    if (o16) m.vec.off.resize(m.nnz);
    hipLaunchKernelGGL(k_vec_fill, dim3((unsigned)ceil_div(m.nrows, 256)), dim3(256), 0, s, m.rp64.get(), m.col.get(),
                       m.val.get(), m.nrows, vb, reinterpret_cast<const unsigned long long *>(m.vec.vtab.get()),
                       (int)tab.size(), o16, (void *)m.vec.codes.get(), m.vec.off.get());
    FAMG_CHECK_HIP(hipGetLastError());
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    m.vec.vbits = vb;
    m.vec.o16 = o16;
    m.vec.ntab = vb ? (int64_t)tab.size() : 0;
}

// waves per row of the wave-per-row kernel: few long rows get 2 or 4 waves each.
// Chosen once per matrix at finalize from all of its rows, so every row segment
// (halo interior / boundary launches, rank-local copies) splits its rows the
// same way; flag FLAG_VEC_WPR (FAMG_VEC_WPR, amg_set_flag) forces 1/2/4.
static int vec_waves_per_row(int64_t rows, int64_t nnz) {
    const int64_t avg = nnz / std::max<int64_t>(1, rows);
    if (rows <= 16384 && avg >= 512) return 4;
    if (rows <= 65536 && avg >= 256) return 2;
    return 1;
}

void choose_kernel(GpuCsr &m) {
    if (m.dia.built() && !m.dia.rowid && m.dia.r0 == 0 && m.dia.r1 == m.nrows) m.kernel = SPMV_KERNEL_DIA;
    else if (m.bsr.built()) m.kernel = SPMV_KERNEL_BSR;
    else if (m.kind_pin == 1) {  // a renumbered copy of a wave-per-row matrix (reorder.hip)
        m.kernel = SPMV_KERNEL_VECTOR;
        m.vec.wpr = vec_waves_per_row(m.nrows, m.nnz);
        build_vec_codes(m);
    }
    else if (m.kind_pin == 2) m.kernel = SPMV_KERNEL_STREAM;
    else if (m.scs.built() && m.scs.seg < 0) m.kernel = SPMV_KERNEL_SCS;
    else if (m.sellp.built()) m.kernel = SPMV_KERNEL_SELLP;
    else if (m.xs.built()) m.kernel = SPMV_KERNEL_XS;
    else if (m.sell.built()) m.kernel = SPMV_KERNEL_SELL;
    else if (g_spmv_format_policy == 3 ||
             (g_spmv_format_policy == 0 && m.nrows > 0 && m.nnz >= vec_min_avg() * m.nrows)) {
        m.kernel = SPMV_KERNEL_VECTOR;
        m.vec.wpr = vec_waves_per_row(m.nrows, m.nnz);
        build_vec_codes(m);
    }
    else m.kernel = SPMV_KERNEL_STREAM;
}

// ------------------------------------------------------------------ dispatch

// The launch of one spmv() call.  The storages are tried in this order: the grid-
// transfer overlays, 3x3 blocks, stencil classes, x-staged SELL, pattern SELL, DIA
// codes (a color-permuted copy's sweep, then the matrix or its DIA segment), and
// the storage chosen at finalize (SELL / wave-per-row / CSR-stream).
SpmvRoute spmv_route(const GpuCsr &m, SpmvMode mode, const SpmvEpi &epi, int64_t seg) {
    SpmvRoute r;
    r.seg = seg;
    r.r0 = seg < 0 ? 0 : m.seg_rows[seg];
    r.r1 = seg < 0 ? m.nrows : m.seg_rows[seg + 1];
    auto to = [&](SpmvRouteTo t, int kernel, const char *name) {
        r.to = t;
        r.kernel = kernel;
        r.name = name;
    };
    const bool overlay = seg < 0 || m.rframe.on();
    if (m.gtx.built() && overlay && gtx_supports(m, mode)) {
        to(ROUTE_GTX, SPMV_KERNEL_GTC, "gtx");
        r.dk = (mode == SPMV_ADD0 || mode == SPMV_SETDF) && epi_dconst(epi);
        return r;
    }
    if (m.gtc.built() && overlay && gtc_supports(m, mode)) {
        to(ROUTE_GTC, SPMV_KERNEL_GTC, "gtc");
        r.dk = (mode == SPMV_ADD0 || mode == SPMV_SETDF) && epi_dconst(epi);
        return r;
    }
    FAMG_REQUIRE(mode != SPMV_SETDF || m.kernel == SPMV_KERNEL_SELLP || m.kernel == SPMV_KERNEL_BSR,
                 AMG_ERR_UNSUPPORTED, "SETDF needs a grid-transfer, pattern-SELL or 3x3-block restriction");
    if (m.kernel == SPMV_KERNEL_BSR) {
        FAMG_REQUIRE(mode != SPMV_SGS, AMG_ERR_UNSUPPORTED, "block storage has no SGS sweep");
        to(ROUTE_BSR, SPMV_KERNEL_BSR, "bsr3");
    } else if (m.kernel == SPMV_KERNEL_SCS || (m.scs.built() && seg >= 0 && seg == m.scs.seg && mode != SPMV_SGS)) {
        FAMG_REQUIRE(mode != SPMV_SGS, AMG_ERR_UNSUPPORTED, "stencil-class storage has no SGS sweep");
        const bool xscs = scs_takes_xscs(m, seg);
        to(ROUTE_SCS, SPMV_KERNEL_SCS, xscs ? "xscs" : m.scs.lanes ? "scs_lanes" : "scs");
        r.rc = xscs && epi.dc;
    } else if (m.kernel == SPMV_KERNEL_XS && seg < 0 && xs_supports(mode)) {  // other modes: CSR-stream below
        to(ROUTE_XS, SPMV_KERNEL_XS, "xsell");
    } else if (m.kernel == SPMV_KERNEL_SELLP) {
        FAMG_REQUIRE(mode != SPMV_SGS, AMG_ERR_UNSUPPORTED, "pattern SELL has no SGS sweep");
        to(ROUTE_SELLP, SPMV_KERNEL_SELLP, "sellp");
    } else if (mode == SPMV_SGS && m.dia.built() && m.dia.rowid) {  // color sweep of a color-permuted copy
        r.to = ROUTE_DIA_SGS;
        dia_route(m, epi, r);
    } else if (m.kernel == SPMV_KERNEL_DIA ||
               (m.dia.built() && !m.dia.rowid && seg >= 0 && seg == m.dia.seg && mode != SPMV_SGS)) {
        FAMG_REQUIRE(mode != SPMV_SGS, AMG_ERR_UNSUPPORTED, "DIA storage has no SGS sweep");
        r.to = ROUTE_DIA;
        dia_route(m, epi, r);
    } else if (m.kernel == SPMV_KERNEL_SELL) {
        r.sell_short = sell_takes_short(m, mode, seg);
        to(ROUTE_SELL, SPMV_KERNEL_SELL, r.sell_short ? "sell_short" : "sell");
    } else if (m.kernel == SPMV_KERNEL_VECTOR) {
        to(ROUTE_VECTOR, SPMV_KERNEL_VECTOR, "vector");
    }
    return r;
}

thread_local LaunchLog *g_launch_log = nullptr;

// Launch-plan record of one spmv() call (amg_multigrid_cycle_plan): the route's
// kernel, the bytes its storage streams for the launched rows, x read once, and
// the epilogue's vector traffic per mode.
static void log_spmv(const GpuCsr &m, SpmvMode mode, const SpmvEpi &epi, const SpmvRoute &rt) {
    const int64_t r = rt.r1 - rt.r0;
    if (r <= 0 || m.nrows <= 0) return;
    const double frac = (double)r / (double)m.nrows;
    auto part = [&](int64_t whole) { return rt.seg < 0 ? whole : (int64_t)std::llround((double)whole * frac); };
    const int64_t csr_mat = part(m.index_bytes());
    int64_t mat = 0;
    switch (rt.to) {
    case ROUTE_GTX: mat = m.gtx.stream_bytes(part(m.nrows)); break;
    case ROUTE_GTC: mat = m.gtc.stream_bytes(part(m.nrows)); break;
    case ROUTE_SCS: mat = m.scs.stream_bytes(r); break;
    case ROUTE_XS: mat = m.stream_bytes(); break;
    case ROUTE_DIA_SGS: mat = 4 * (int64_t)m.dia.cw * r + 8 * m.dia.ntab; break;
    case ROUTE_DIA: mat = rt.cst ? (int64_t)m.dia.k * 8 : 4 * (int64_t)m.dia.cw * r + 8 * m.dia.ntab; break;
    case ROUTE_STREAM: mat = csr_mat; break;
    default: mat = part(m.stream_bytes()); break;  // BSR, SELLP, SELL, VECTOR: the finalized storage
    }
    const int64_t xcols = part(m.ncols);
    const int64_t db = rt.dk ? 0 : (epi.dc ? 1 : 8);  // bytes per diagonal entry (8-bit codes or fp64)
    int64_t vec = 8 * xcols;              // x read once
    switch (mode) {
    case SPMV_SET: vec += 8 * r; break;                  // y written
    case SPMV_ADD: vec += 16 * r; break;                 // y read + written
    case SPMV_RESID: vec += 16 * r; break;               // b read, y written
    case SPMV_JACOBI: vec += 16 * r + db * r; break;     // b, d read, y written
    case SPMV_SGS: vec += 28 * r; break;                 // perm, d, b read, x written
    case SPMV_RESID0:  // x = b; d gathered beside x (1-B codes in the DIA and x-staged class kernels); y written
        vec += 8 * r + (rt.dk ? 0 : rt.rc ? 1 : 8) * xcols;
        break;
    case SPMV_ADD0: vec += 16 * r + db * r; break;       // b, d read, y written
    case SPMV_SETDF: vec += 16 * r + db * r; break;      // y and d*y written, d read
    }
    log_launch(rt.name, rt.kernel, mode, r, mat + vec, csr_mat + vec);
}

#define FAMG_VEC(VB, O16, W) , VB, O16, W
static void spmv_vector(const GpuCsr &m, const Epi &e, SpmvMode mode, hipStream_t s, const SpmvRoute &r) {
    if (r.r1 <= r.r0) return;
    VecArgs a{m.rp32.get(), m.col.get(), m.vec.off.get(), m.val.get(), m.vec.codes.get(), m.vec.vtab.get(),
              (int32_t)r.r0, (int32_t)(r.r1 - r.r0), e};
    const int wpr = flag(FLAG_VEC_WPR) ? (int)flag(FLAG_VEC_WPR) : m.vec.wpr;
    const dim3 grid((unsigned)ceil_div(r.r1 - r.r0, 4 / wpr)), block(256);
    const int key = m.vec.vbits * 2 + (m.vec.o16 ? 1 : 0);
#define FAMG_VECW(W)                                                                                   \
    switch (key) {                                                                                 \
    case 0: FAMG_LAUNCH_MODES(spmv_vector_kernel, grid, block, s, a, FAMG_VEC(0, false, W)) break;  \
    case 1: FAMG_LAUNCH_MODES(spmv_vector_kernel, grid, block, s, a, FAMG_VEC(0, true, W)) break;   \
    case 16: FAMG_LAUNCH_MODES(spmv_vector_kernel, grid, block, s, a, FAMG_VEC(8, false, W)) break; \
    case 17: FAMG_LAUNCH_MODES(spmv_vector_kernel, grid, block, s, a, FAMG_VEC(8, true, W)) break;  \
    case 32: FAMG_LAUNCH_MODES(spmv_vector_kernel, grid, block, s, a, FAMG_VEC(16, false, W)) break;\
    default: FAMG_LAUNCH_MODES(spmv_vector_kernel, grid, block, s, a, FAMG_VEC(16, true, W)) break; \
    }
    if (wpr == 4) { FAMG_VECW(4) }
    else if (wpr == 2) { FAMG_VECW(2) }
    else { FAMG_VECW(1) }
#undef FAMG_VECW
    FAMG_CHECK_HIP(hipGetLastError());
}

static void spmv_stream(const GpuCsr &m, const Epi &e, SpmvMode mode, hipStream_t s, const SpmvRoute &r) {
    const int64_t b0 = r.seg < 0 ? 0 : m.seg_blk[r.seg];
    const int64_t b1 = r.seg < 0 ? m.nblocks : m.seg_blk[r.seg + 1];
    if (b1 <= b0) return;
    StreamArgs a{m.rp32.get(), m.col.get(), m.val.get(), m.sched.get() + b0, (int32_t)(b1 - b0), e};
    const dim3 grid((unsigned)(b1 - b0)), block(256);
    FAMG_LAUNCH_MODES(spmv_stream_kernel, grid, block, s, a)
    FAMG_CHECK_HIP(hipGetLastError());
}

void spmv(const GpuCsr &m, const double *x, double *y, SpmvMode mode, const SpmvEpi &epi,
          hipStream_t s, int64_t seg) {
    FAMG_REQUIRE(m.spmv_ready(), AMG_ERR_UNSUPPORTED, "SpMV needs nnz < 2^31 (32-bit row pointers)");
    FAMG_REQUIRE(seg < (int64_t)m.seg_rows.size() - 1, AMG_ERR_INVALID, "SpMV segment out of range");
    FAMG_REQUIRE(mode != SPMV_SGS || epi.perm, AMG_ERR_INVALID, "SGS mode needs a permutation");
    const SpmvRoute r = spmv_route(m, mode, epi, seg);
    if (g_launch_log) log_spmv(m, mode, epi, r);
    const Epi e{x, y, epi.b, epi.d, epi.perm, epi.dc, epi.dt, epi.dk};
    switch (r.to) {
    case ROUTE_GTX: spmv_gtx(m, x, y, mode, epi, s, seg); break;
    case ROUTE_GTC: spmv_gtc(m, x, y, mode, epi, s, seg); break;
    case ROUTE_BSR: spmv_bsr(m, x, y, mode, epi, s, seg); break;
    case ROUTE_SCS: spmv_scs(m, x, y, mode, epi, s, seg); break;
    case ROUTE_XS: spmv_xs(m, x, y, mode, epi, s); break;
    case ROUTE_SELLP: spmv_sellp(m, x, y, mode, epi, s, seg); break;
    case ROUTE_DIA_SGS: spmv_dia_sgs(m, x, y, epi, s, r); break;
    case ROUTE_DIA: spmv_dia(m, x, y, mode, epi, s, r); break;
    case ROUTE_SELL: spmv_sell(m, x, y, mode, epi, s, r); break;
    case ROUTE_VECTOR: spmv_vector(m, e, mode, s, r); break;
    case ROUTE_STREAM: spmv_stream(m, e, mode, s, r); break;
    }
}

void spmm(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k, hipStream_t s) {
    if (spmm_compressed(m, x, ldx, y, ldy, k, s)) return;  // DIA codes, stencil classes, 3x3 blocks (spmm.hip)
    if (m.kernel == SPMV_KERNEL_SELL && !m.sell.vbits) {
        spmm_sell(m, x, ldx, y, ldy, k, s);
        return;
    }
    for (int64_t c = 0; c < k; c++) spmv(m, x + c * ldx, y + c * ldy, SPMV_SET, SpmvEpi{}, s);  // one SpMV per column
}

// Y = epilogue(A X) on CSR-stream storage, 8 columns per launch
static void spmm_stream(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k,
                        SpmvMode mode, const SpmmEpi &epi, hipStream_t s) {
    if (m.nblocks <= 0) return;
    const dim3 grid((unsigned)m.nblocks), block(256);
    for (int64_t c0 = 0; c0 < k; c0 += 8) {
        const int kb = (int)std::min<int64_t>(8, k - c0);
        const Epi e{x + c0 * ldx, y + c0 * ldy, epi.b ? epi.b + c0 * epi.ldb : nullptr, epi.d, nullptr, nullptr, nullptr, 0.0};
        StreamArgs a{m.rp32.get(), m.col.get(), m.val.get(), m.sched.get(), (int32_t)m.nblocks, e};
        switch (mode) {
        case SPMV_SET: spmm_stream_kernel<SPMV_SET><<<grid, block, 0, s>>>(a, kb, ldx, ldy, epi.ldb); break;
        case SPMV_ADD: spmm_stream_kernel<SPMV_ADD><<<grid, block, 0, s>>>(a, kb, ldx, ldy, epi.ldb); break;
        case SPMV_RESID: spmm_stream_kernel<SPMV_RESID><<<grid, block, 0, s>>>(a, kb, ldx, ldy, epi.ldb); break;
        default: spmm_stream_kernel<SPMV_JACOBI><<<grid, block, 0, s>>>(a, kb, ldx, ldy, epi.ldb); break;
        }
        FAMG_CHECK_HIP(hipGetLastError());
    }
}

// Launch-plan records of one spmm_epi() call on a storage with an SpMM kernel: one
// per group of up to 8 columns -- the matrix bytes once, the vector traffic of
// log_spmv per column (x read once per column, fp64 d).  gtc: the grid-transfer
// overlay serves the call (its bytes as log_spmv counts them).
static void log_spmm(const GpuCsr &m, SpmvMode mode, int64_t k, bool gtc = false) {
    static const char *const names[] = {"spmm_stream", "spmm_sell", "spmm_vector", "spmm_dia", "spmm_bsr3",
                                        "spmm_sellp",  "spmm_scs",  "spmm_xsell"};
    const int64_t r = m.nrows;
    const int64_t mat = gtc ? r + 2 * (int64_t)m.gtc.nce + 8 * (int64_t)m.gtc.ntab
                        : m.kernel == SPMV_KERNEL_DIA ? 4 * (int64_t)m.dia.cw * r + 8 * m.dia.ntab : m.stream_bytes();
    int64_t vec = 8 * m.ncols;
    switch (mode) {
    case SPMV_SET: vec += 8 * r; break;
    case SPMV_ADD: vec += 16 * r; break;
    case SPMV_RESID: vec += 16 * r; break;
    default: vec += 24 * r; break;  // JACOBI: b, d read, y written
    }
    for (int64_t c0 = 0; c0 < k; c0 += 8) {
        const int64_t kb = std::min<int64_t>(8, k - c0);
        log_launch(gtc ? "spmm_gtc" : names[m.kernel], gtc ? SPMV_KERNEL_GTC : m.kernel, mode, r, mat + kb * vec,
                   m.index_bytes() + kb * vec);
    }
}

void spmm_epi(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k, SpmvMode mode,
              const SpmmEpi &epi, hipStream_t s) {
    FAMG_REQUIRE(mode >= SPMV_SET && mode <= SPMV_JACOBI, AMG_ERR_INVALID,
                 "SpMM epilogue: mode must be SET, ADD, RESID or JACOBI");
    FAMG_REQUIRE((mode != SPMV_RESID && mode != SPMV_JACOBI) || epi.b, AMG_ERR_INVALID, "SpMM epilogue: B required");
    FAMG_REQUIRE(mode != SPMV_JACOBI || (epi.d && m.nrows == m.ncols), AMG_ERR_INVALID,
                 "SpMM epilogue: JACOBI needs d and a square matrix");
    if (k <= 0 || m.nrows == 0) return;
    FAMG_REQUIRE(m.spmv_ready(), AMG_ERR_UNSUPPORTED, "SpMM needs nnz < 2^31 (32-bit row pointers)");
    // The storages in spmv_route's order, so that every column is the launch the
    // single-vector call makes: the grid-transfer overlays first (gtx per column, gtc
    // k-wide; they sum a row in one lane, the storage below them need not), then the
    // SpMM kernels, then value-coded SELL-64 and CSR-stream.
    const bool gtx_first = m.gtx.built() && gtx_supports(m, mode);
    const bool gtc_first = !gtx_first && m.gtc.built() && gtc_supports(m, mode);
    if (gtc_first && !m.rframe.on()) {
        if (g_launch_log) log_spmm(m, mode, k, true);
        spmm_gtc(m, x, ldx, y, ldy, k, mode, s);
        return;
    }
    const bool overlay = gtx_first || gtc_first;
    if (!overlay && spmm_has_kernel(m)) {
        if (g_launch_log) log_spmm(m, mode, k);
        if (mode == SPMV_SET) spmm(m, x, ldx, y, ldy, k, s);
        else if (!spmm_compressed_epi(m, x, ldx, y, ldy, k, mode, epi, s)) spmm_sell_epi(m, x, ldx, y, ldy, k, mode, epi, s);
        return;
    }
    if (!overlay && m.kernel == SPMV_KERNEL_SELL && m.sell.vbits) {
        if (g_launch_log) log_spmm(m, mode, k);
        spmm_sell_coded(m, x, ldx, y, ldy, k, mode, epi, s);
        return;
    }
    if (!overlay && m.kernel == SPMV_KERNEL_STREAM) {
        if (g_launch_log) log_spmm(m, mode, k);
        spmm_stream(m, x, ldx, y, ldy, k, mode, epi, s);
        return;
    }
    // wave-per-row, the wide grid-transfer classes and x-staged classes with eight
    // lanes per row: no k-wide kernel
    for (int64_t c = 0; c < k; c++) {
        SpmvEpi e;
        e.b = epi.b ? epi.b + c * epi.ldb : nullptr;
        e.d = epi.d;
        spmv(m, x + c * ldx, y + c * ldy, mode, e, s);
    }
}

}  // namespace famg
