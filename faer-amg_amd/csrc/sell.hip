// sell.hip -- SELL-64 storage of short regular rows (the 7-pt fine level, P, R,
// A_1): its kernels, its builder and its SpMV / SpMM launches.
//
// One lane per row, one wavefront per 64-row slice stored column-major -- every
// entry step of a slice is one 512-B value / 256-B index access; no LDS, no
// barrier, no row pointers; all loads of an <= 8-entry chunk are issued before the
// dependent x gathers.  Rows are summed sequentially (bit-identical to the oracle).
#include <algorithm>

#include "spmv_dev.hpp"

namespace famg {

constexpr int SELL_MAX_W = 512;
constexpr int64_t SELL_PAIR_MIN_SLICES = 1;  // pairing paid on every level measured (A_2: 55 vs 60 us)

// ------------------------------------------------------------------- SELL-64
//
// Slice s = up to 64 consecutive rows, one lane per row, w_s entry steps.  The
// slice's block in sell.data is [w_s x 64 fp64 values | column block], the
// column of lane l at step t given by the slice's column mode:
//   0 implicit  col = base[t] + l                    (0 B/entry)
//   1 u16       col = base[t] + d16(t, l)            (2 B/entry)
//   2 i32       col = c32(t, l)                      (4 B/entry)
// Steps are either the k-th stored entry of every row ("plain") or, when it is
// cheaper, the sorted union of the slice's column offsets col - row
// ("aligned"; a stencil row then reads x[row + offset] for offset t: mode 0
// and coalesced x loads).  A row without an entry at a step holds 0.0 at an
// in-range column, so every row is still summed in its stored (ascending
// column) order with fma, interleaved with exact +0 terms: bit-identical to the
// CSR kernels for finite x.
//
// Element order inside a block (values, and the u16/i32 column block alike):
// steps are stored in PAIRS -- step t < 2*floor(w/2) of lane l at element
// (t & ~1)*64 + 2l + (t & 1) -- so one 16-B load per lane brings the values of
// two steps (4 B / 8 B for two compressed columns); an odd last step is stored
// plainly at t*64 + l.  Streamed with 8-B non-temporal loads the values ran at
// roughly 0.54-0.70x the 16-B rate (MI355X_MICROARCH.md, L2-served loads).
// `sell.paired = false` keeps one 512-B row per step (A/B switch,
// FAMG_SELL_LAYOUT=step at build time).
constexpr int SELL_VAL_STEP = SELL_C * 8;  // bytes of values per step

__host__ __device__ __forceinline__ int64_t sell_elem(int t, int w, int lane, bool paired) {
    if (paired && (t | 1) < w) return (int64_t)(t & ~1) * SELL_C + 2 * lane + (t & 1);
    return (int64_t)t * SELL_C + lane;
}

struct SellArgs {
    const int32_t *row0;   // nslices+1 (slices tile the rows)
    const int32_t *soff;   // nslices+1 step offsets
    const uint32_t *desc;  // block offset / 128 | mode << 30
    const int32_t *base;   // one per step
    const char *data;
    int32_t slice0, nslices;
    Epi e;
    const double *vtab;  // value table (code widths 4 / 8 / 16)
    int32_t ntab;
    int32_t spw;  // slices per wave (value codes: 2 on large matrices, else 1)
};

// ---- one step per 512-B row (sell.paired = false)

template <int MODE, int CM, int U>
__device__ __forceinline__ void sell_chunk(const double *__restrict__ v, const void *__restrict__ ix,
                                           const int32_t *__restrict__ bs, int lane, const Epi &e, double &acc) {
    double vv[U];
    int32_t cc[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        vv[u] = __builtin_nontemporal_load(v + u * SELL_C);
        if constexpr (CM == 0) cc[u] = bs[u] + lane;
        else if constexpr (CM == 1)
            cc[u] = bs[u] + (int32_t)__builtin_nontemporal_load(static_cast<const uint16_t *>(ix) + u * SELL_C);
        else cc[u] = __builtin_nontemporal_load(static_cast<const int32_t *>(ix) + u * SELL_C);
    }
    double xx[U];
#pragma unroll
    for (int u = 0; u < U; u++) xx[u] = gx<MODE>(e, cc[u]);
#pragma unroll
    for (int u = 0; u < U; u++) acc = fma(vv[u], xx[u], acc);
}

template <int MODE, int CM>
__device__ __forceinline__ double sell_walk_steps(const char *blkp, const int32_t *bs, int w, int lane,
                                                  const Epi &e) {
    constexpr int IB = CM == 0 ? 0 : CM == 1 ? 2 : 4;  // index bytes per entry
    const double *v = reinterpret_cast<const double *>(blkp) + lane;
    const char *ix = blkp + (int64_t)w * SELL_VAL_STEP + lane * IB;
    double acc = 0.0;
    int k = 0;
    for (; k + 8 <= w; k += 8)
        sell_chunk<MODE, CM, 8>(v + k * SELL_C, ix + (int64_t)k * SELL_C * IB, bs + k, lane, e, acc);
    v += k * SELL_C;
    ix += (int64_t)k * SELL_C * IB;
    bs += k;
    switch (w - k) {
    case 1: sell_chunk<MODE, CM, 1>(v, ix, bs, lane, e, acc); break;
    case 2: sell_chunk<MODE, CM, 2>(v, ix, bs, lane, e, acc); break;
    case 3: sell_chunk<MODE, CM, 3>(v, ix, bs, lane, e, acc); break;
    case 4: sell_chunk<MODE, CM, 4>(v, ix, bs, lane, e, acc); break;
    case 5: sell_chunk<MODE, CM, 5>(v, ix, bs, lane, e, acc); break;
    case 6: sell_chunk<MODE, CM, 6>(v, ix, bs, lane, e, acc); break;
    case 7: sell_chunk<MODE, CM, 7>(v, ix, bs, lane, e, acc); break;
    default: break;
    }
    return acc;
}

// ---- step pairs (sell.paired = true)

// UP step pairs starting at pair p0, plus the odd last step when TAIL; every
// load of the group is issued before the dependent x gathers, and the row sum
// still runs over t ascending.
template <int MODE, int CM, int UP, bool TAIL>
__device__ __forceinline__ void sell_pairs(const char *__restrict__ blkp, int w, int p0,
                                           const int32_t *__restrict__ bs, int lane, const Epi &e, double &acc) {
    constexpr int NS = 2 * UP + (TAIL ? 1 : 0);
    double vv[NS];
    int32_t cc[NS];
    const char *ixb = blkp + (int64_t)w * SELL_VAL_STEP;
#pragma unroll
    for (int u = 0; u < UP; u++) {
        const int64_t q = (int64_t)(p0 + u) * SELL_C + lane;  // 2-element unit of this lane
        const dbl2_t v = __builtin_nontemporal_load(reinterpret_cast<const dbl2_t *>(blkp) + q);
        vv[2 * u] = v.x;
        vv[2 * u + 1] = v.y;
        const int t = 2 * (p0 + u);
        if constexpr (CM == 0) {
            cc[2 * u] = bs[t] + lane;
            cc[2 * u + 1] = bs[t + 1] + lane;
        } else if constexpr (CM == 1) {
            const uint32_t d = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(ixb) + q);
            cc[2 * u] = bs[t] + (int32_t)(d & 0xffffu);
            cc[2 * u + 1] = bs[t + 1] + (int32_t)(d >> 16);
        } else {
            const i32x2_t d = __builtin_nontemporal_load(reinterpret_cast<const i32x2_t *>(ixb) + q);
            cc[2 * u] = d.x;
            cc[2 * u + 1] = d.y;
        }
    }
    if constexpr (TAIL) {
        const int t = w - 1;
        const int64_t el = (int64_t)t * SELL_C + lane;
        vv[NS - 1] = __builtin_nontemporal_load(reinterpret_cast<const double *>(blkp) + el);
        if constexpr (CM == 0) cc[NS - 1] = bs[t] + lane;
        else if constexpr (CM == 1)
            cc[NS - 1] = bs[t] + (int32_t)__builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(ixb) + el);
        else cc[NS - 1] = __builtin_nontemporal_load(reinterpret_cast<const int32_t *>(ixb) + el);
    }
    double xx[NS];
#pragma unroll
    for (int u = 0; u < NS; u++) xx[u] = gx<MODE>(e, cc[u]);
#pragma unroll
    for (int u = 0; u < NS; u++) acc = fma(vv[u], xx[u], acc);
}

template <int MODE, int CM>
__device__ __forceinline__ double sell_walk_pairs(const char *blkp, const int32_t *bs, int w, int lane,
                                                  const Epi &e) {
    double acc = 0.0;
    const int np = w >> 1;
    int p = 0;
    for (; p + 4 <= np; p += 4) sell_pairs<MODE, CM, 4, false>(blkp, w, p, bs, lane, e, acc);
    switch (2 * (np - p) + (w & 1)) {
    case 1: sell_pairs<MODE, CM, 0, true>(blkp, w, p, bs, lane, e, acc); break;
    case 2: sell_pairs<MODE, CM, 1, false>(blkp, w, p, bs, lane, e, acc); break;
    case 3: sell_pairs<MODE, CM, 1, true>(blkp, w, p, bs, lane, e, acc); break;
    case 4: sell_pairs<MODE, CM, 2, false>(blkp, w, p, bs, lane, e, acc); break;
    case 5: sell_pairs<MODE, CM, 2, true>(blkp, w, p, bs, lane, e, acc); break;
    case 6: sell_pairs<MODE, CM, 3, false>(blkp, w, p, bs, lane, e, acc); break;
    case 7: sell_pairs<MODE, CM, 3, true>(blkp, w, p, bs, lane, e, acc); break;
    default: break;
    }
    return acc;
}

// ---- value codes (sell.vbits = 4, 8 or 16)
//
// A matrix whose stored values take at most 16 / 256 / 65536 distinct fp64 bit
// patterns (the padding's +0.0 included) stores a 4 / 8 / 16-bit code per
// entry into a per-matrix table sorted by bit pattern instead of the value
// (index/value compression in the manner of CSR-VI).  The 8 codes of steps
// 8g..8g+7 of one lane form one 4 / 8 / 16-B unit at g*64 + lane.  Column
// blocks (u16 / i32) use the same grouping: step t of lane l at element
// 8g*64 + r_g*l + (t - 8g), r_g = min(8, w - 8g), so a full group is one (u16)
// or two (i32) 16-B loads per lane.  Tables of <= 256 entries are staged in
// LDS per workgroup, 16-bit tables are read through the caches.  A decoded
// value is the stored value bit for bit, so every row sum is unchanged.
__host__ __device__ __forceinline__ int sell_code_bytes(int vb) { return vb == 4 ? 4 : vb == 8 ? 8 : 16; }

__host__ __device__ __forceinline__ int64_t sell_value_bytes(int64_t w, int vb) {
    return vb ? ((w + 7) >> 3) * SELL_C * sell_code_bytes(vb) : w * SELL_VAL_STEP;
}

__host__ __device__ __forceinline__ int64_t sell_group_elem(int t, int w, int lane) {
    const int g0 = t & ~7;
    const int r = w - g0 < 8 ? w - g0 : 8;
    return (int64_t)g0 * SELL_C + r * lane + (t & 7);
}

template <int VB>
__device__ __forceinline__ void sell_load_codes(const char *__restrict__ blkp, int g, int lane, uint32_t (&q)[4]) {
    const int64_t unit = (int64_t)g * SELL_C + lane;
    if constexpr (VB == 4) {
        q[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(blkp) + unit);
    } else if constexpr (VB == 8) {
        const i32x2_t v = __builtin_nontemporal_load(reinterpret_cast<const i32x2_t *>(blkp) + unit);
        q[0] = (uint32_t)v.x;
        q[1] = (uint32_t)v.y;
    } else {
        const i32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const i32x4_t *>(blkp) + unit);
        q[0] = (uint32_t)v.x;
        q[1] = (uint32_t)v.y;
        q[2] = (uint32_t)v.z;
        q[3] = (uint32_t)v.w;
    }
}

template <int VB> __device__ __forceinline__ int sell_code(const uint32_t (&q)[4], int u) {
    if constexpr (VB == 4) return (int)((q[0] >> (4 * u)) & 15u);
    else if constexpr (VB == 8) return (int)((q[u >> 2] >> (8 * (u & 3))) & 255u);
    else return (int)((q[u >> 1] >> (16 * (u & 1))) & 0xffffu);
}

// Columns of the R (<= 8) steps of group g (first step t0 = 8g).
template <int CM, int R>
__device__ __forceinline__ void sell_group_cols(const char *__restrict__ ixb, const int32_t *__restrict__ bs, int t0,
                                                int lane, int32_t (&cc)[R]) {
    if constexpr (CM == 0) {
#pragma unroll
        for (int u = 0; u < R; u++) cc[u] = bs[t0 + u] + lane;
    } else if constexpr (R == 8) {
        const int64_t el = (int64_t)t0 * SELL_C + 8 * lane;
        if constexpr (CM == 1) {
            const i32x4_t d = __builtin_nontemporal_load(reinterpret_cast<const i32x4_t *>(ixb + 2 * el));
#pragma unroll
            for (int u = 0; u < 4; u++) {
                cc[2 * u] = bs[t0 + 2 * u] + (int32_t)((uint32_t)d[u] & 0xffffu);
                cc[2 * u + 1] = bs[t0 + 2 * u + 1] + (int32_t)((uint32_t)d[u] >> 16);
            }
        } else {
            const i32x4_t *p = reinterpret_cast<const i32x4_t *>(ixb + 4 * el);
            const i32x4_t d0 = __builtin_nontemporal_load(p);
            const i32x4_t d1 = __builtin_nontemporal_load(p + 1);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                cc[u] = d0[u];
                cc[4 + u] = d1[u];
            }
        }
    } else {
        const int64_t el = (int64_t)t0 * SELL_C + R * lane;
#pragma unroll
        for (int u = 0; u < R; u++) {
            if constexpr (CM == 1)
                cc[u] = bs[t0 + u] +
                        (int32_t)__builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(ixb) + el + u);
            else cc[u] = __builtin_nontemporal_load(reinterpret_cast<const int32_t *>(ixb) + el + u);
        }
    }
}

// R (<= 8) steps of group g: every load of the group is issued before the
// dependent x gathers; the row sum runs over t ascending.
template <int MODE, int CM, int VB, int R>
__device__ __forceinline__ void sellc_group(const char *__restrict__ blkp, const char *__restrict__ ixb, int g,
                                            const int32_t *__restrict__ bs, int lane, const double *tab,
                                            const Epi &e, double &acc) {
    uint32_t q[4];
    sell_load_codes<VB>(blkp, g, lane, q);
    int32_t cc[R];
    sell_group_cols<CM, R>(ixb, bs, 8 * g, lane, cc);
    double xx[R];
#pragma unroll
    for (int u = 0; u < R; u++) xx[u] = gx<MODE>(e, cc[u]);
#pragma unroll
    for (int u = 0; u < R; u++) acc = fma(tab[sell_code<VB>(q, u)], xx[u], acc);
}

// The same for two slices of equal width and column mode in lockstep: the
// loads of both slices are in flight together (a codes slice streams few
// bytes, so one slice per wave leaves the memory system latency-bound).
template <int MODE, int CM, int VB, int R>
__device__ __forceinline__ void sellc_group2(const char *__restrict__ ba, const char *__restrict__ bb,
                                             const char *__restrict__ ia, const char *__restrict__ ib, int g,
                                             const int32_t *__restrict__ sa, const int32_t *__restrict__ sb,
                                             int lane, const double *tab, const Epi &e, double &acca,
                                             double &accb) {
    uint32_t qa[4], qb[4];
    sell_load_codes<VB>(ba, g, lane, qa);
    sell_load_codes<VB>(bb, g, lane, qb);
    int32_t ca[R], cb[R];
    sell_group_cols<CM, R>(ia, sa, 8 * g, lane, ca);
    sell_group_cols<CM, R>(ib, sb, 8 * g, lane, cb);
    double xa[R], xb[R];
#pragma unroll
    for (int u = 0; u < R; u++) {
        xa[u] = gx<MODE>(e, ca[u]);
        xb[u] = gx<MODE>(e, cb[u]);
    }
#pragma unroll
    for (int u = 0; u < R; u++) acca = fma(tab[sell_code<VB>(qa, u)], xa[u], acca);
#pragma unroll
    for (int u = 0; u < R; u++) accb = fma(tab[sell_code<VB>(qb, u)], xb[u], accb);
}

template <int MODE, int CM, int VB>
__device__ __forceinline__ void sellc_walk2(const char *ba, const char *bb, const int32_t *sa, const int32_t *sb,
                                            int w, int lane, const double *tab, const Epi &e, double &acca,
                                            double &accb) {
    const int ng = (w + 7) >> 3;
    const char *ia = ba + (int64_t)ng * SELL_C * sell_code_bytes(VB);
    const char *ib = bb + (int64_t)ng * SELL_C * sell_code_bytes(VB);
    acca = 0.0;
    accb = 0.0;
    const int full = w >> 3;
    for (int g = 0; g < full; g++) sellc_group2<MODE, CM, VB, 8>(ba, bb, ia, ib, g, sa, sb, lane, tab, e, acca, accb);
    switch (w & 7) {
    case 1: sellc_group2<MODE, CM, VB, 1>(ba, bb, ia, ib, full, sa, sb, lane, tab, e, acca, accb); break;
    case 2: sellc_group2<MODE, CM, VB, 2>(ba, bb, ia, ib, full, sa, sb, lane, tab, e, acca, accb); break;
    case 3: sellc_group2<MODE, CM, VB, 3>(ba, bb, ia, ib, full, sa, sb, lane, tab, e, acca, accb); break;
    case 4: sellc_group2<MODE, CM, VB, 4>(ba, bb, ia, ib, full, sa, sb, lane, tab, e, acca, accb); break;
    case 5: sellc_group2<MODE, CM, VB, 5>(ba, bb, ia, ib, full, sa, sb, lane, tab, e, acca, accb); break;
    case 6: sellc_group2<MODE, CM, VB, 6>(ba, bb, ia, ib, full, sa, sb, lane, tab, e, acca, accb); break;
    case 7: sellc_group2<MODE, CM, VB, 7>(ba, bb, ia, ib, full, sa, sb, lane, tab, e, acca, accb); break;
    default: break;
    }
}

template <int MODE, int CM, int VB>
__device__ __forceinline__ double sellc_walk(const char *blkp, const int32_t *bs, int w, int lane, const double *tab,
                                             const Epi &e) {
    const int ng = (w + 7) >> 3;
    const char *ixb = blkp + (int64_t)ng * SELL_C * sell_code_bytes(VB);
    double acc = 0.0;
    const int full = w >> 3;
    // two groups' loads in one block, except RESID0 (two gathers per entry
    // already; the doubled footprint cost occupancy)
    constexpr int UNR = MODE == SPMV_RESID0 ? 1 : 2;
#pragma unroll UNR
    for (int g = 0; g < full; g++) sellc_group<MODE, CM, VB, 8>(blkp, ixb, g, bs, lane, tab, e, acc);
    switch (w & 7) {
    case 1: sellc_group<MODE, CM, VB, 1>(blkp, ixb, full, bs, lane, tab, e, acc); break;
    case 2: sellc_group<MODE, CM, VB, 2>(blkp, ixb, full, bs, lane, tab, e, acc); break;
    case 3: sellc_group<MODE, CM, VB, 3>(blkp, ixb, full, bs, lane, tab, e, acc); break;
    case 4: sellc_group<MODE, CM, VB, 4>(blkp, ixb, full, bs, lane, tab, e, acc); break;
    case 5: sellc_group<MODE, CM, VB, 5>(blkp, ixb, full, bs, lane, tab, e, acc); break;
    case 6: sellc_group<MODE, CM, VB, 6>(blkp, ixb, full, bs, lane, tab, e, acc); break;
    case 7: sellc_group<MODE, CM, VB, 7>(blkp, ixb, full, bs, lane, tab, e, acc); break;
    default: break;
    }
    return acc;
}

// ---- lockstep pair, two adjacent rows per lane
//
// Lanes 0-31 take rows 2h, 2h+1 (h = lane & 31) of slice A, lanes 32-63 the
// same rows of slice B.  A value-code slice streams few matrix bytes, so its
// time goes to the vector accesses; with two rows per lane the codes, the
// column blocks, x (implicit columns), b, d and y all move in 16-B accesses
// (8-B-per-lane accesses run at ~0.5-0.7x the 16-B rate on MI355X).  Each row
// is still summed by one lane in ascending steps: bitwise unchanged.

template <int MODE, int CM, int VB, int R>
__device__ __forceinline__ void sellc_group_rp(const char *__restrict__ blk, const char *__restrict__ ixb, int g,
                                               const int32_t *__restrict__ sa, const int32_t *__restrict__ sb,
                                               bool hb, int r0, const double *tab, const Epi &e, double &acc0,
                                               double &acc1) {
    const int t0 = 8 * g;
    uint32_t q0[4], q1[4];
    if constexpr (VB == 4) {
        const i32x2_t v = __builtin_nontemporal_load(reinterpret_cast<const i32x2_t *>(blk) + ((int64_t)g * SELL_C + r0) / 2);
        q0[0] = (uint32_t)v.x;
        q1[0] = (uint32_t)v.y;
    } else if constexpr (VB == 8) {
        const i32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const i32x4_t *>(blk) + ((int64_t)g * SELL_C + r0) / 2);
        q0[0] = (uint32_t)v.x;
        q0[1] = (uint32_t)v.y;
        q1[0] = (uint32_t)v.z;
        q1[1] = (uint32_t)v.w;
    } else {
        const i32x4_t *p = reinterpret_cast<const i32x4_t *>(blk) + (int64_t)g * SELL_C + r0;
        const i32x4_t v0 = __builtin_nontemporal_load(p);
        const i32x4_t v1 = __builtin_nontemporal_load(p + 1);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            q0[k] = (uint32_t)v0[k];
            q1[k] = (uint32_t)v1[k];
        }
    }
    int32_t bse[R];
#pragma unroll
    for (int u = 0; u < R; u++) bse[u] = hb ? sb[t0 + u] : sa[t0 + u];
    int32_t c0[R], c1[R];
    if constexpr (CM == 0) {
#pragma unroll
        for (int u = 0; u < R; u++) {
            c0[u] = bse[u] + r0;
            c1[u] = c0[u] + 1;
        }
    } else if constexpr (R == 8) {
        const int64_t el = (int64_t)t0 * SELL_C + 8 * r0;  // row r0: 8 elements, then row r0 + 1
        if constexpr (CM == 1) {
            const i32x4_t *p = reinterpret_cast<const i32x4_t *>(ixb + 2 * el);
            const i32x4_t d0 = __builtin_nontemporal_load(p);
            const i32x4_t d1 = __builtin_nontemporal_load(p + 1);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                c0[2 * u] = bse[2 * u] + (int32_t)((uint32_t)d0[u] & 0xffffu);
                c0[2 * u + 1] = bse[2 * u + 1] + (int32_t)((uint32_t)d0[u] >> 16);
                c1[2 * u] = bse[2 * u] + (int32_t)((uint32_t)d1[u] & 0xffffu);
                c1[2 * u + 1] = bse[2 * u + 1] + (int32_t)((uint32_t)d1[u] >> 16);
            }
        } else {
            const i32x4_t *p = reinterpret_cast<const i32x4_t *>(ixb + 4 * el);
            const i32x4_t d0 = __builtin_nontemporal_load(p), d1 = __builtin_nontemporal_load(p + 1);
            const i32x4_t d2 = __builtin_nontemporal_load(p + 2), d3 = __builtin_nontemporal_load(p + 3);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                c0[u] = d0[u];
                c0[4 + u] = d1[u];
                c1[u] = d2[u];
                c1[4 + u] = d3[u];
            }
        }
    } else if constexpr (CM == 1) {
        // the 2R u16 of rows r0, r0 + 1 as R dwords (4-B aligned: r0 is even)
        // instead of 2R 2-B loads (P_0: 4-5 steps per row)
        const int64_t el = (int64_t)t0 * SELL_C + R * r0;
        const uint32_t *p = reinterpret_cast<const uint32_t *>(ixb + 2 * el);
        uint32_t dw[R];
#pragma unroll
        for (int k = 0; k < R; k++) dw[k] = __builtin_nontemporal_load(p + k);
#pragma unroll
        for (int u = 0; u < R; u++) {
            const int j0 = u, j1 = R + u;  // element indices of the two rows
            c0[u] = bse[u] + (int32_t)((dw[j0 >> 1] >> (16 * (j0 & 1))) & 0xffffu);
            c1[u] = bse[u] + (int32_t)((dw[j1 >> 1] >> (16 * (j1 & 1))) & 0xffffu);
        }
    } else {
        const int64_t el = (int64_t)t0 * SELL_C + R * r0;  // row r0: R elements, then row r0 + 1
#pragma unroll
        for (int u = 0; u < R; u++) {
            const int32_t *p = reinterpret_cast<const int32_t *>(ixb) + el;
            c0[u] = __builtin_nontemporal_load(p + u);
            c1[u] = __builtin_nontemporal_load(p + R + u);
        }
    }
    double x0[R], x1[R];
#pragma unroll
    for (int u = 0; u < R; u++) {
        if constexpr (CM == 0) {
            const dbl2_t v = *reinterpret_cast<const dbl2u_t *>(e.x + c0[u]);
            x0[u] = v.x;
            x1[u] = v.y;
        } else {
            x0[u] = e.x[c0[u]];
            x1[u] = e.x[c1[u]];
        }
    }
#pragma unroll
    for (int u = 0; u < R; u++) acc0 = fma(tab[sell_code<VB>(q0, u)], x0[u], acc0);
#pragma unroll
    for (int u = 0; u < R; u++) acc1 = fma(tab[sell_code<VB>(q1, u)], x1[u], acc1);
}

template <int MODE, int CM, int VB>
__device__ __forceinline__ void sellc_walk_rp(const char *ba, const char *bb, const int32_t *sa, const int32_t *sb,
                                              int w, int lane, const double *tab, const Epi &e, double &acc0,
                                              double &acc1) {
    const bool hb = lane >= 32;
    const int r0 = 2 * (lane & 31);
    const char *blk = hb ? bb : ba;
    const int ng = (w + 7) >> 3;
    const char *ixb = blk + (int64_t)ng * SELL_C * sell_code_bytes(VB);
    acc0 = 0.0;
    acc1 = 0.0;
    const int full = w >> 3;
    for (int g = 0; g < full; g++) sellc_group_rp<MODE, CM, VB, 8>(blk, ixb, g, sa, sb, hb, r0, tab, e, acc0, acc1);
    switch (w & 7) {
    case 1: sellc_group_rp<MODE, CM, VB, 1>(blk, ixb, full, sa, sb, hb, r0, tab, e, acc0, acc1); break;
    case 2: sellc_group_rp<MODE, CM, VB, 2>(blk, ixb, full, sa, sb, hb, r0, tab, e, acc0, acc1); break;
    case 3: sellc_group_rp<MODE, CM, VB, 3>(blk, ixb, full, sa, sb, hb, r0, tab, e, acc0, acc1); break;
    case 4: sellc_group_rp<MODE, CM, VB, 4>(blk, ixb, full, sa, sb, hb, r0, tab, e, acc0, acc1); break;
    case 5: sellc_group_rp<MODE, CM, VB, 5>(blk, ixb, full, sa, sb, hb, r0, tab, e, acc0, acc1); break;
    case 6: sellc_group_rp<MODE, CM, VB, 6>(blk, ixb, full, sa, sb, hb, r0, tab, e, acc0, acc1); break;
    case 7: sellc_group_rp<MODE, CM, VB, 7>(blk, ixb, full, sa, sb, hb, r0, tab, e, acc0, acc1); break;
    default: break;
    }
}

template <int MODE>
__host__ __device__ constexpr bool sell_row_pairs(int lay) {
    return lay >= 4 && (MODE == SPMV_SET || MODE == SPMV_ADD || MODE == SPMV_RESID || MODE == SPMV_JACOBI ||
                        MODE == SPMV_ADD0);
}

template <int MODE, int CM, int LAY>
__device__ __forceinline__ double sellc_walk_any(const char *blkp, const int32_t *bs, int w, int lane,
                                                 const double *stab, const SellArgs &a) {
    if constexpr (LAY == 16) return sellc_walk<MODE, CM, 16>(blkp, bs, w, lane, a.vtab, a.e);
    else return sellc_walk<MODE, CM, LAY>(blkp, bs, w, lane, stab, a.e);
}

// Slices per wave: one for fp64 values, two (in lockstep when their width and
// column mode agree) for value codes -- except RESID0, whose rows gather two
// vectors (d and x) and which ran slower with the doubled register footprint.
__host__ __device__ constexpr int sell_slices_per_wave(int lay, int mode) {
    return lay >= 4 && mode != SPMV_RESID0 ? 2 : 1;
}

// LAY: 0 one step per 512-B row, 1 step pairs (fp64 values); 4 / 8 / 16 value codes
template <int MODE, int LAY>
__device__ __forceinline__ void sell_wave(const SellArgs &a, const double *stab, int sl) {
    const int slice = a.slice0 + sl;
    const int lane = threadIdx.x & 63;
    if constexpr (sell_row_pairs<MODE>(LAY) && sell_slices_per_wave(LAY, MODE) == 2) {
        // two slices of equal width and column mode: two adjacent rows per lane
        if (a.spw == 2 && sl + 1 < a.nslices) {
            const int ta = a.soff[slice], tb = a.soff[slice + 1], te = a.soff[slice + 2];
            const uint32_t da = a.desc[slice], db = a.desc[slice + 1];
            if (tb - ta == te - tb && (da >> 30) == (db >> 30)) {
                const bool hb = lane >= 32;
                const int rs = hb ? a.row0[slice + 1] : a.row0[slice];
                const int re = hb ? a.row0[slice + 2] : a.row0[slice + 1];
                const int row = rs + 2 * (lane & 31);
                EpiOps2<MODE> ep2;
                ep2.load(a.e, row, row < re, row + 1 < re);
                const char *ba = a.data + (int64_t)(da & 0x3fffffffu) * 128;
                const char *bb = a.data + (int64_t)(db & 0x3fffffffu) * 128;
                const int32_t *sa = a.base + ta, *sbp = a.base + tb;
                const double *tab = LAY == 16 ? a.vtab : stab;
                double acc0, acc1;
                switch (da >> 30) {
                case 0: sellc_walk_rp<MODE, 0, LAY>(ba, bb, sa, sbp, tb - ta, lane, tab, a.e, acc0, acc1); break;
                case 1: sellc_walk_rp<MODE, 1, LAY>(ba, bb, sa, sbp, tb - ta, lane, tab, a.e, acc0, acc1); break;
                default: sellc_walk_rp<MODE, 2, LAY>(ba, bb, sa, sbp, tb - ta, lane, tab, a.e, acc0, acc1); break;
                }
                ep2.store(a.e, acc0, acc1);
                return;
            }
        }
    }
    const int row = a.row0[slice] + lane;
    const bool live = row < a.row0[slice + 1];
    EpiOps<MODE> ep;
    if (live) ep.load(a.e, row);
    const int t0 = a.soff[slice];
    const int w = a.soff[slice + 1] - t0;
    const uint32_t d = a.desc[slice];
    const char *blkp = a.data + (int64_t)(d & 0x3fffffffu) * 128;
    const int32_t *bs = a.base + t0;
    double acc;
    if (LAY >= 4 && (sell_slices_per_wave(LAY, MODE) == 1 || a.spw == 1)) {
        switch (d >> 30) {
        case 0: acc = sellc_walk_any<MODE, 0, LAY>(blkp, bs, w, lane, stab, a); break;
        case 1: acc = sellc_walk_any<MODE, 1, LAY>(blkp, bs, w, lane, stab, a); break;
        default: acc = sellc_walk_any<MODE, 2, LAY>(blkp, bs, w, lane, stab, a); break;
        }
    } else if constexpr (LAY >= 4) {
        // second slice of the wave
        const bool two = sl + 1 < a.nslices;
        int rowb = 0, wb = 0;
        bool liveb = false;
        uint32_t db = 0;
        EpiOps<MODE> epb;
        if (two) {
            rowb = a.row0[slice + 1] + lane;
            liveb = rowb < a.row0[slice + 2];
            if (liveb) epb.load(a.e, rowb);
            wb = a.soff[slice + 2] - a.soff[slice + 1];
            db = a.desc[slice + 1];
        }
        const char *blkb = a.data + (int64_t)(db & 0x3fffffffu) * 128;
        const int32_t *bsb = a.base + t0 + w;
        double accb = 0.0;
        if (two && wb == w && (db >> 30) == (d >> 30)) {
            switch (d >> 30) {
            case 0: sellc_walk2<MODE, 0, LAY>(blkp, blkb, bs, bsb, w, lane, LAY == 16 ? a.vtab : stab, a.e, acc, accb); break;
            case 1: sellc_walk2<MODE, 1, LAY>(blkp, blkb, bs, bsb, w, lane, LAY == 16 ? a.vtab : stab, a.e, acc, accb); break;
            default: sellc_walk2<MODE, 2, LAY>(blkp, blkb, bs, bsb, w, lane, LAY == 16 ? a.vtab : stab, a.e, acc, accb); break;
            }
        } else {
            switch (d >> 30) {
            case 0: acc = sellc_walk_any<MODE, 0, LAY>(blkp, bs, w, lane, stab, a); break;
            case 1: acc = sellc_walk_any<MODE, 1, LAY>(blkp, bs, w, lane, stab, a); break;
            default: acc = sellc_walk_any<MODE, 2, LAY>(blkp, bs, w, lane, stab, a); break;
            }
            if (two) {
                switch (db >> 30) {
                case 0: accb = sellc_walk_any<MODE, 0, LAY>(blkb, bsb, wb, lane, stab, a); break;
                case 1: accb = sellc_walk_any<MODE, 1, LAY>(blkb, bsb, wb, lane, stab, a); break;
                default: accb = sellc_walk_any<MODE, 2, LAY>(blkb, bsb, wb, lane, stab, a); break;
                }
            }
        }
        if (live) ep.store(a.e, acc);
        if (liveb) epb.store(a.e, accb);
        return;
    } else if constexpr (LAY == 1) {
        switch (d >> 30) {
        case 0: acc = sell_walk_pairs<MODE, 0>(blkp, bs, w, lane, a.e); break;
        case 1: acc = sell_walk_pairs<MODE, 1>(blkp, bs, w, lane, a.e); break;
        default: acc = sell_walk_pairs<MODE, 2>(blkp, bs, w, lane, a.e); break;
        }
    } else {
        switch (d >> 30) {
        case 0: acc = sell_walk_steps<MODE, 0>(blkp, bs, w, lane, a.e); break;
        case 1: acc = sell_walk_steps<MODE, 1>(blkp, bs, w, lane, a.e); break;
        default: acc = sell_walk_steps<MODE, 2>(blkp, bs, w, lane, a.e); break;
        }
    }
    if (live) ep.store(a.e, acc);
}

// Consecutive slice groups per wave (1: four per wave made the small coarse
// levels launch too few waves and did not speed up the fine level).
__host__ __device__ constexpr int sell_groups_per_wave(int) { return 1; }

template <int MODE, int LAY>
__global__ __launch_bounds__(256) void spmv_sell_kernel(SellArgs a) {
    constexpr int TABN = LAY == 4 ? 16 : LAY == 8 ? 256 : 1;
    __shared__ double stab[TABN];
    if constexpr (LAY == 4 || LAY == 8) {
        for (int i = threadIdx.x; i < a.ntab; i += 256) stab[i] = a.vtab[i];
        __syncthreads();
    }
    constexpr int SPW = sell_slices_per_wave(LAY, MODE);
    constexpr int NSEQ = sell_groups_per_wave(LAY);
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const int wv = __builtin_amdgcn_readfirstlane(blk * 4 + (int)(threadIdx.x >> 6));
    for (int k = 0; k < NSEQ; k++) {
        const int sl = (wv * NSEQ + k) * (SPW == 2 ? a.spw : 1);
        if (sl >= a.nslices) return;
        sell_wave<MODE, LAY>(a, stab, sl);
    }
}

// 16-bit codes with the table staged in LDS (dynamic, ntab doubles) by a
// persistent grid: each workgroup stages once and walks virtual blocks v, v + G,
// ... of the spmv_sell_kernel decomposition (the table reads become LDS reads
// instead of dependent L2 gathers; per-block staging alone measured slower).
template <int MODE>
__global__ __launch_bounds__(256) void spmv_sell_t16_kernel(SellArgs a, int nvb) {
    extern __shared__ double dtab[];
    for (int i = threadIdx.x; i < a.ntab; i += 256) dtab[i] = a.vtab[i];
    __syncthreads();
    SellArgs b = a;
    b.vtab = dtab;
    constexpr int SPW = sell_slices_per_wave(16, MODE);
    for (int v = blockIdx.x; v < nvb; v += gridDim.x) {
        const int blk = xcd_remap(v, nvb);
        const int wv = __builtin_amdgcn_readfirstlane(blk * 4 + (int)(threadIdx.x >> 6));
        const int sl = wv * (SPW == 2 ? b.spw : 1);
        if (sl < b.nslices) sell_wave<MODE, 16>(b, nullptr, sl);
    }
}

// 16-bit-code SELL with its table in LDS for long rows (>= 32 entries on average:
// R_1 of the 256^3 cycle, 87 entries per row, 40 -> 35 us; short rows such as P_1's
// 11 pay more for the staging than they save: 47 -> 48 us with a persistent grid
// of 2 workgroups per CU, 56 us with 4).  A/B switch FAMG_SELL_T16=0: off; N > 0:
// also for short rows, at most N workgroups per CU.
static int sell_t16_mode() { static const int v = (int)env_int("FAMG_SELL_T16", -1); return v; }

// Value-code SELL whose slices are all at most 4 steps wide with implicit or
// u16 columns and pair up (equal width and column mode): P_0 of a box
// hierarchy (4 entries per row).  Only the lockstep row-pair path of
// spmv_sell_kernel, with R = w known per case: a fraction of the generic
// kernel's registers (which it sizes for 8-step groups of every layout), so
// more waves keep their loads in flight.  Same row sums in the same order.
template <int MODE, int LAY>
__global__ __launch_bounds__(256) void spmv_sell_short_kernel(SellArgs a) {
    constexpr int TABN = LAY == 4 ? 16 : LAY == 8 ? 256 : 1;
    __shared__ double stab[TABN];
    if constexpr (LAY == 4 || LAY == 8) {
        for (int i = threadIdx.x; i < a.ntab; i += 256) stab[i] = a.vtab[i];
        __syncthreads();
    }
    const double *tab = LAY == 16 ? a.vtab : stab;
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const int sl = 2 * __builtin_amdgcn_readfirstlane(blk * 4 + (int)(threadIdx.x >> 6));
    if (sl >= a.nslices) return;
    const int slice = a.slice0 + sl;
    const int lane = threadIdx.x & 63;
    const int ta = a.soff[slice], tb = a.soff[slice + 1];
    const uint32_t da = a.desc[slice], db = a.desc[slice + 1];
    const bool hb = lane >= 32;
    const int rs = hb ? a.row0[slice + 1] : a.row0[slice];
    const int re = hb ? a.row0[slice + 2] : a.row0[slice + 1];
    const int row = rs + 2 * (lane & 31);
    // ADD0 (the folded correction d*b + P x): its operands are loaded here and the
    // coded diagonal decoded after the row's loads are issued (EpiOps2 decodes it
    // first, and the dependent table read held up the row: 119 vs 99 us for ADD)
    constexpr bool A0 = MODE == SPMV_ADD0;
    EpiOps2<A0 ? SPMV_SET : MODE> ep2;
    const bool l0 = row < re, l1 = row + 1 < re;
    ep2.load(a.e, row, l0, l1);
    dbl2_t b0 = {0.0, 0.0}, d0 = {0.0, 0.0};
    uint32_t k0 = 0, k1 = 0;
    if constexpr (A0) {
        if (l0) {
            if (l1) b0 = *reinterpret_cast<const dbl2u_t *>(a.e.b + row);
            else b0.x = a.e.b[row];
            if (a.e.dc) {
                k0 = a.e.dc[row];
                k1 = a.e.dc[l1 ? row + 1 : row];
            } else if (l1) {
                d0 = *reinterpret_cast<const dbl2u_t *>(a.e.d + row);
            } else {
                d0.x = a.e.d[row];
            }
        }
    }
    const char *blk2 = a.data + (int64_t)((hb ? db : da) & 0x3fffffffu) * 128;
    const char *ixb = blk2 + (int64_t)SELL_C * sell_code_bytes(LAY);
    const int32_t *sa = a.base + ta, *sbp = a.base + tb;
    const int r0 = 2 * (lane & 31);
    double acc0 = 0.0, acc1 = 0.0;
    switch ((int)(da >> 30) * 8 + (tb - ta)) {
    case 1: sellc_group_rp<MODE, 0, LAY, 1>(blk2, ixb, 0, sa, sbp, hb, r0, tab, a.e, acc0, acc1); break;
    case 2: sellc_group_rp<MODE, 0, LAY, 2>(blk2, ixb, 0, sa, sbp, hb, r0, tab, a.e, acc0, acc1); break;
    case 3: sellc_group_rp<MODE, 0, LAY, 3>(blk2, ixb, 0, sa, sbp, hb, r0, tab, a.e, acc0, acc1); break;
    case 4: sellc_group_rp<MODE, 0, LAY, 4>(blk2, ixb, 0, sa, sbp, hb, r0, tab, a.e, acc0, acc1); break;
    case 9: sellc_group_rp<MODE, 1, LAY, 1>(blk2, ixb, 0, sa, sbp, hb, r0, tab, a.e, acc0, acc1); break;
    case 10: sellc_group_rp<MODE, 1, LAY, 2>(blk2, ixb, 0, sa, sbp, hb, r0, tab, a.e, acc0, acc1); break;
    case 11: sellc_group_rp<MODE, 1, LAY, 3>(blk2, ixb, 0, sa, sbp, hb, r0, tab, a.e, acc0, acc1); break;
    case 12: sellc_group_rp<MODE, 1, LAY, 4>(blk2, ixb, 0, sa, sbp, hb, r0, tab, a.e, acc0, acc1); break;
    default: break;  // width 0
    }
    if constexpr (A0) {
        if (!l0) return;
        if (a.e.dc) {
            d0.x = a.e.dt[k0];
            d0.y = l1 ? a.e.dt[k1] : 0.0;
        }
        const dbl2_t out = d0 * b0 + dbl2_t{acc0, acc1};
        if (l1) *reinterpret_cast<dbl2u_t *>(a.e.y + row) = out;
        else a.e.y[row] = out.x;
    } else {
        ep2.store(a.e, acc0, acc1);
    }
}

// SpMM: Y = A X for up to SPMM_KB columns per launch (column-major X, Y with
// leading dimensions).  The slice is streamed once per column group; each
// (row, column) sum keeps the SpMV's order (ascending steps, fma), so every
// column is bitwise equal to a single-column SpMV.
constexpr int SPMM_KB = 8;

template <int CM, int KB>
__device__ __forceinline__ void spmm_step4(const char *__restrict__ blkp, int w, int k, bool paired,
                                           const int32_t *__restrict__ bs, int lane, int nu,
                                           const double *__restrict__ x, int64_t ldx, double (&acc)[KB]) {
    const char *ixb = blkp + (int64_t)w * SELL_VAL_STEP;
    double vv[4];
    int32_t cc[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        if (u < nu) {
            const int t = k + u;
            const int64_t el = sell_elem(t, w, lane, paired);
            vv[u] = __builtin_nontemporal_load(reinterpret_cast<const double *>(blkp) + el);
            if constexpr (CM == 0) cc[u] = bs[t] + lane;
            else if constexpr (CM == 1)
                cc[u] = bs[t] + (int32_t)__builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(ixb) + el);
            else cc[u] = __builtin_nontemporal_load(reinterpret_cast<const int32_t *>(ixb) + el);
        }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
        if (u < nu) {
#pragma unroll
            for (int c = 0; c < KB; c++) acc[c] = fma(vv[u], x[cc[u] + c * ldx], acc[c]);
        }
    }
}

template <int CM, int KB>
__device__ __forceinline__ void spmm_walk(const char *blkp, bool paired, const int32_t *bs, int w, int lane,
                                          const double *x, int64_t ldx, double (&acc)[KB]) {
    for (int k = 0; k < w; k += 4) spmm_step4<CM, KB>(blkp, w, k, paired, bs, lane, min(4, w - k), x, ldx, acc);
}

// MODE: the cycle's epilogue fused at the store (spmm_store; SET: the plain Y = A X)
template <int KB, int MODE>
__global__ __launch_bounds__(256) void spmm_sell_kernel(SellArgs a, bool paired, int64_t ldx, double *y,
                                                        int64_t ldy, SpmmEpiDev e) {
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const int sl = __builtin_amdgcn_readfirstlane(blk * 4 + (int)(threadIdx.x >> 6));
    if (sl >= a.nslices) return;
    const int slice = a.slice0 + sl;
    const int lane = threadIdx.x & 63;
    const int row = a.row0[slice] + lane;
    const bool live = row < a.row0[slice + 1];
    const int t0 = a.soff[slice];
    const int w = a.soff[slice + 1] - t0;
    const uint32_t d = a.desc[slice];
    const char *blkp = a.data + (int64_t)(d & 0x3fffffffu) * 128;
    const int32_t *bs = a.base + t0;
    double acc[KB];
#pragma unroll
    for (int c = 0; c < KB; c++) acc[c] = 0.0;
    switch (d >> 30) {
    case 0: spmm_walk<0, KB>(blkp, paired, bs, w, lane, a.e.x, ldx, acc); break;
    case 1: spmm_walk<1, KB>(blkp, paired, bs, w, lane, a.e.x, ldx, acc); break;
    default: spmm_walk<2, KB>(blkp, paired, bs, w, lane, a.e.x, ldx, acc); break;
    }
    if (live) {
#pragma unroll
        for (int c = 0; c < KB; c++) spmm_store<MODE>(y, ldy, a.e.x, ldx, e, row, c, acc[c]);
    }
}

// ---- SELL build: one wavefront per slice walks its rows in step order.

__device__ __forceinline__ int64_t wave_min64(int64_t v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, (int64_t)__shfl_xor((long long)v, o));
    return v;
}
__device__ __forceinline__ int64_t wave_max64(int64_t v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, (int64_t)__shfl_xor((long long)v, o));
    return v;
}

constexpr int64_t SELL_NONE = INT64_MAX;

// Walk the steps of one slice (all 64 lanes of the wave, uniform control flow).
// f(t, col, val, step_mode, step_base) per step; returns the step count, or -1
// if it would exceed max_steps.
template <bool ALIGNED, class F>
__device__ int sell_walk_build(const int64_t *rp, const int32_t *col, const double *val, int64_t row, bool live,
                               int64_t ncols, int max_steps, F &&f) {
    const int lane = threadIdx.x & 63;
    int64_t p = live ? rp[row] : 0;
    const int64_t e = live ? rp[row + 1] : 0;
    for (int t = 0;; t++) {
        bool real;
        if constexpr (ALIGNED) {
            const int64_t my = p < e ? (int64_t)col[p] - row : SELL_NONE;
            const int64_t m = wave_min64(my);
            if (m == SELL_NONE) return t;
            real = my == m;
        } else {
            real = p < e;
            if (!__any(real)) return t;
        }
        if (t >= max_steps) return -1;
        int64_t c = 0;
        double v = 0.0;
        if (real) { c = col[p]; v = val[p]; p++; }
        const int64_t b = wave_min64(real ? c - lane : SELL_NONE);
        if (!real) c = std::min<int64_t>(std::max<int64_t>(b + lane, 0), ncols - 1);
        const bool impl = __all(c == b + lane);
        const int64_t mn = wave_min64(c), mx = wave_max64(c);
        const int mode = impl ? 0 : (mx - mn < 65536 ? 1 : 2);
        f(t, c, v, mode, mode == 0 ? b : mn);
    }
}

__host__ __device__ inline int64_t sell_slice_bytes(int64_t w, int mode, int vb) {
    return sell_value_bytes(w, vb) + w * (mode == 0 ? 0 : mode == 1 ? 2 * SELL_C : 4 * SELL_C);
}

// plan[4 s ..] = {w_aligned (-1 = too wide), mode_aligned, w_plain, mode_plain}
__global__ __launch_bounds__(256) void k_sell_plan(const int64_t *rp, const int32_t *col, const double *val,
                                                   const int32_t *row0, int64_t nslices, int64_t ncols,
                                                   int max_steps, int32_t *plan) {
    const int64_t sl = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (sl >= nslices) return;
    const int64_t row = row0[sl] + (threadIdx.x & 63);
    const bool live = row < row0[sl + 1];
    int ma = 0, mp = 0;
    const int wa = sell_walk_build<true>(rp, col, val, row, live, ncols, max_steps,
                                         [&](int, int64_t, double, int m, int64_t) { ma = max(ma, m); });
    const int wp = sell_walk_build<false>(rp, col, val, row, live, ncols, max_steps,
                                          [&](int, int64_t, double, int m, int64_t) { mp = max(mp, m); });
    if ((threadIdx.x & 63) == 0) {
        plan[4 * sl + 0] = wa;
        plan[4 * sl + 1] = ma;
        plan[4 * sl + 2] = wp;
        plan[4 * sl + 3] = mp;
    }
}

// aligned[s] chooses the layout; desc/soff as uploaded; vb != 0: values as
// vb-bit codes into tab (ntab entries, ascending bit patterns)
__global__ __launch_bounds__(256) void k_sell_fill(const int64_t *rp, const int32_t *col, const double *val,
                                                   const int32_t *row0, const int32_t *soff, const uint32_t *desc,
                                                   const uint8_t *aligned, int64_t nslices, int64_t ncols,
                                                   bool paired, int vb, const unsigned long long *tab, int ntab,
                                                   int32_t *base, char *data) {
    const int64_t sl = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (sl >= nslices) return;
    const int lane = threadIdx.x & 63;
    const int64_t row = row0[sl] + lane;
    const bool live = row < row0[sl + 1];
    const int w = soff[sl + 1] - soff[sl];
    const uint32_t d = desc[sl];
    const int smode = (int)(d >> 30);
    char *blkp = data + (int64_t)(d & 0x3fffffffu) * 128;
    char *ixb = blkp + sell_value_bytes(w, vb);
    double *vals = reinterpret_cast<double *>(blkp);
    int32_t *bs = base + soff[sl];
    unsigned long long cacc = 0;
    auto put = [&](int t, int64_t c, double v, int, int64_t b) {
        // the slice mode can exceed the step's: u16 steps use base = min column
        const int64_t sb = smode == 1 ? wave_min64(c) : b;
        const int64_t el = vb ? sell_group_elem(t, w, lane) : sell_elem(t, w, lane, paired);
        if (vb == 0) {
            vals[el] = v;
        } else {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
            int lo = 0, hi = ntab - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (tab[mid] < bits) lo = mid + 1;
                else hi = mid;
            }
            const int64_t unit = (int64_t)(t >> 3) * SELL_C + lane;
            if (vb == 16) {
                reinterpret_cast<uint16_t *>(blkp)[unit * 8 + (t & 7)] = (uint16_t)lo;
            } else {
                cacc |= (unsigned long long)lo << (vb * (t & 7));
                if ((t & 7) == 7 || t == w - 1) {
                    if (vb == 4) reinterpret_cast<uint32_t *>(blkp)[unit] = (uint32_t)cacc;
                    else reinterpret_cast<unsigned long long *>(blkp)[unit] = cacc;
                    cacc = 0;
                }
            }
        }
        if (lane == 0) bs[t] = smode == 2 ? 0 : (int32_t)sb;
        if (smode == 1) reinterpret_cast<uint16_t *>(ixb)[el] = (uint16_t)(c - sb);
        else if (smode == 2) reinterpret_cast<int32_t *>(ixb)[el] = (int32_t)c;
    };
    if (aligned[sl]) sell_walk_build<true>(rp, col, val, row, live, ncols, w, put);
    else sell_walk_build<false>(rp, col, val, row, live, ncols, w, put);
}

void build_sell(GpuCsr &m, const std::vector<int64_t> &rp) {
    const int pol = g_spmv_format_policy;
    if (pol == 1 || pol == 3 || m.kind_pin >= 1 || m.nrows == 0 || m.nnz == 0) return;
    // slices never straddle a segment
    std::vector<int32_t> row0;
    std::vector<int64_t> seg_slc{0};
    int64_t maxlen = 0;
    for (size_t g = 0; g + 1 < m.seg_rows.size(); g++) {
        for (int64_t r0 = m.seg_rows[g]; r0 < m.seg_rows[g + 1]; r0 += SELL_C) row0.push_back((int32_t)r0);
        seg_slc.push_back((int64_t)row0.size());
    }
    for (int64_t r = 0; r < m.nrows; r++) maxlen = std::max<int64_t>(maxlen, rp[r + 1] - rp[r]);
    const int max_w = pol == 2 ? 256 : SELL_MAX_W;
    if (maxlen > max_w) return;
    row0.push_back((int32_t)m.nrows);
    const int64_t ns = (int64_t)row0.size() - 1;
    std::vector<unsigned long long> tab;
    const int vb = csr_value_table(m, tab);
    // DIA codes on the whole matrix, or (several row segments: the halo
    // interior of a distributed level) on its longest segment beside SELL
    int64_t dseg = 0;
    for (size_t g = 1; g + 1 < m.seg_rows.size(); g++)
        if (m.seg_rows[g + 1] - m.seg_rows[g] > m.seg_rows[dseg + 1] - m.seg_rows[dseg]) dseg = (int64_t)g;
    // (a renumbered copy, reorder.hip, keeps its rows' stored order: no DIA, no aligned slices)
    if (!m.order_fixed && build_dia(m, vb, tab, rp, m.seg_rows[dseg], m.seg_rows[dseg + 1])) {
        m.dia.seg = dseg;
        if (m.dia.r0 == 0 && m.dia.r1 == m.nrows) return;
    }
    hipStream_t s = m.ctx->stream;
    DevBuf<int32_t> drow0(ns + 1), dplan(4 * ns);
    FAMG_CHECK_HIP(hipMemcpyAsync(drow0.get(), row0.data(), (ns + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const dim3 grid((unsigned)ceil_div(ns, 4));
    hipLaunchKernelGGL(k_sell_plan, grid, dim3(256), 0, s, m.rp64.get(), m.col.get(), m.val.get(), drow0.get(), ns,
                       m.ncols, max_w, dplan.get());
    FAMG_CHECK_HIP(hipGetLastError());
    std::vector<int32_t> plan(4 * ns);
    FAMG_CHECK_HIP(hipMemcpyAsync(plan.data(), dplan.get(), plan.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    // per slice: the cheaper layout; then offsets
    std::vector<int32_t> soff(ns + 1, 0);
    std::vector<uint32_t> desc(ns);
    std::vector<uint8_t> aligned(ns);
    int64_t bytes = 0, steps = 0, cnt[3] = {0, 0, 0};
    for (int64_t k = 0; k < ns; k++) {
        const int wa = plan[4 * k], ma = plan[4 * k + 1], wp = plan[4 * k + 2], mp = plan[4 * k + 3];
        const bool al = !m.order_fixed && wa >= 0 && sell_slice_bytes(wa, ma, vb) <= sell_slice_bytes(wp, mp, vb);
        const int w = al ? wa : wp, md = al ? ma : mp;
        aligned[k] = al;
        if (bytes / 128 >= (int64_t(1) << 30) || steps + w >= (int64_t(1) << 31)) return;
        desc[k] = (uint32_t)(bytes / 128) | ((uint32_t)md << 30);
        bytes += sell_slice_bytes(w, md, vb);
        steps += w;
        soff[k + 1] = (int32_t)steps;
        cnt[md]++;
    }
    // auto: SELL pays when there are enough slices to fill the chip (>= 1024
    // slices = 64K rows) and it streams no more than 1.25x the CSR bytes;
    // measured on the 256^3 hierarchy (scripts/ab_levels.py).
    const bool ok = pol == 2 || m.kind_pin == 0 || (bytes * 100 <= 12 * m.nnz * 125 && (m.nrows >= SELL_MIN_ROWS || maxlen <= 16) &&
                                 (vec_min_avg() >= VECTOR_MIN_AVG || m.nnz < vec_min_avg() * m.nrows));
    if (!ok) return;
    m.sell.row0 = std::move(drow0);
    m.sell.soff.resize(ns + 1);
    m.sell.desc.resize(ns);
    m.sell.base.resize(std::max<int64_t>(1, steps));
    m.sell.data.resize(std::max<int64_t>(128, bytes));
    DevBuf<uint8_t> dal(ns);
    const char *lay = getenv("FAMG_SELL_LAYOUT");
    m.sell.paired = !(lay && std::string(lay) == "step");
    FAMG_CHECK_HIP(hipMemcpyAsync(m.sell.soff.get(), soff.data(), (ns + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    FAMG_CHECK_HIP(hipMemcpyAsync(m.sell.desc.get(), desc.data(), ns * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    FAMG_CHECK_HIP(hipMemcpyAsync(dal.get(), aligned.data(), ns, hipMemcpyHostToDevice, s));
    if (vb) {
        m.sell.vtab.resize(tab.size());
        FAMG_CHECK_HIP(hipMemcpyAsync(m.sell.vtab.get(), tab.data(), tab.size() * sizeof(double),
                                      hipMemcpyHostToDevice, s));
    }
    hipLaunchKernelGGL(k_sell_fill, grid, dim3(256), 0, s, m.rp64.get(), m.col.get(), m.val.get(),
                       m.sell.row0.get(), m.sell.soff.get(), m.sell.desc.get(), dal.get(), ns, m.ncols,
                       m.sell.paired, vb, reinterpret_cast<const unsigned long long *>(m.sell.vtab.get()),
                       (int)tab.size(), m.sell.base.get(), m.sell.data.get());
    FAMG_CHECK_HIP(hipGetLastError());
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    m.sell.nslices = ns;
    m.sell.steps = steps;
    m.sell.bytes = bytes;
    m.sell.vbits = vb;
    m.sell.ntab = vb ? (int64_t)tab.size() : 0;
    for (int k = 0; k < 3; k++) m.sell.mode_slices[k] = cnt[k];
    m.sell.seg_slc = seg_slc;
    // short slices (coded, <= 4 steps, implicit / u16 columns, pairs of equal
    // width and column mode, one row segment): spmv_sell_short_kernel
    bool sh = vb != 0 && ns % 2 == 0 && cnt[2] == 0 && m.seg_rows.size() == 2;
    for (int64_t k = 0; sh && k < ns; k += 2) {
        const int32_t wa = soff[k + 1] - soff[k], wb = soff[k + 2] - soff[k + 1];
        sh = wa <= 4 && wa == wb && (desc[k] >> 30) == (desc[k + 1] >> 30) && row0[k + 1] - row0[k] == 64;
    }
    m.sell.is_short = sh;
}

// A/B switch FAMG_SELL_SHORT=0: short-slice operators take the generic SELL kernel
bool sell_takes_short(const GpuCsr &m, SpmvMode mode, int64_t seg) {
    static const bool enabled = env_not_zero("FAMG_SELL_SHORT");
    return m.sell.is_short && seg < 0 && mode != SPMV_SGS && mode != SPMV_RESID0 && enabled;
}

void spmv_sell(const GpuCsr &m, const double *x, double *y, SpmvMode mode, const SpmvEpi &epi, hipStream_t s,
               const SpmvRoute &r) {
    const int64_t s0 = r.seg < 0 ? 0 : m.sell.seg_slc[r.seg];
    const int64_t s1 = r.seg < 0 ? m.sell.nslices : m.sell.seg_slc[r.seg + 1];
    if (s1 <= s0) return;
    SellArgs a{m.sell.row0.get(), m.sell.soff.get(), m.sell.desc.get(), m.sell.base.get(),
               m.sell.data.get(), (int32_t)s0, (int32_t)(s1 - s0), Epi{x, y, epi.b, epi.d, epi.perm, epi.dc, epi.dt, epi.dk},
               m.sell.vtab.get(), (int32_t)m.sell.ntab, 1};
    // value codes: two slices per wave when there are enough waves to fill the chip twice over
    const int lay = m.sell.vbits ? 4 : 0;
    if (sell_slices_per_wave(lay, mode) == 2 && s1 - s0 >= SELL_PAIR_MIN_SLICES) a.spw = 2;
    const dim3 grid((unsigned)ceil_div(s1 - s0, 4 * a.spw * sell_groups_per_wave(lay))), block(256);
    if (r.sell_short) {
        const dim3 g2((unsigned)ceil_div(s1 - s0, 8));
        if (m.sell.vbits == 4) {
            FAMG_LAUNCH_MODES(spmv_sell_short_kernel, g2, block, s, a, FAMG_LAY4)
        } else if (m.sell.vbits == 8) {
            FAMG_LAUNCH_MODES(spmv_sell_short_kernel, g2, block, s, a, FAMG_LAY8)
        } else {
            FAMG_LAUNCH_MODES(spmv_sell_short_kernel, g2, block, s, a, FAMG_LAY16)
        }
    } else if (m.sell.vbits == 4) {
        FAMG_LAUNCH_MODES(spmv_sell_kernel, grid, block, s, a, FAMG_LAY4)
    } else if (m.sell.vbits == 8) {
        FAMG_LAUNCH_MODES(spmv_sell_kernel, grid, block, s, a, FAMG_LAY8)
    } else if (m.sell.vbits == 16 && m.sell.ntab <= 8192 && mode != SPMV_SGS &&
               ((sell_t16_mode() < 0 && m.nnz >= 32 * m.nrows) || sell_t16_mode() > 0)) {
        const int nvb = (int)grid.x;
        const dim3 g2((unsigned)(sell_t16_mode() > 0 ? std::min(nvb, 256 * sell_t16_mode()) : nvb));
        const size_t lds = (size_t)m.sell.ntab * sizeof(double);
        switch (mode) {
        case SPMV_SET: spmv_sell_t16_kernel<SPMV_SET><<<g2, block, lds, s>>>(a, nvb); break;
        case SPMV_ADD: spmv_sell_t16_kernel<SPMV_ADD><<<g2, block, lds, s>>>(a, nvb); break;
        case SPMV_RESID: spmv_sell_t16_kernel<SPMV_RESID><<<g2, block, lds, s>>>(a, nvb); break;
        case SPMV_JACOBI: spmv_sell_t16_kernel<SPMV_JACOBI><<<g2, block, lds, s>>>(a, nvb); break;
        case SPMV_RESID0: spmv_sell_t16_kernel<SPMV_RESID0><<<g2, block, lds, s>>>(a, nvb); break;
        case SPMV_ADD0: spmv_sell_t16_kernel<SPMV_ADD0><<<g2, block, lds, s>>>(a, nvb); break;
        default: break;
        }
    } else if (m.sell.vbits == 16) {
        FAMG_LAUNCH_MODES(spmv_sell_kernel, grid, block, s, a, FAMG_LAY16)
    } else if (m.sell.paired) {
        FAMG_LAUNCH_MODES(spmv_sell_kernel, grid, block, s, a, FAMG_LAY1)
    } else {
        FAMG_LAUNCH_MODES(spmv_sell_kernel, grid, block, s, a, FAMG_LAY0)
    }
    FAMG_CHECK_HIP(hipGetLastError());
}

// Value-coded SELL over kb columns (spmm_epi): spmv_sell_kernel's decomposition --
// the value table staged once, then each wave walks its slices once per column
// with sell_wave, the single-vector walk (the slices come from HBM for the first
// column and from L2 for the others, as in spmm_xs_group_kernel).  Bitwise per
// column every single-vector kernel of the storage (generic, short, t16: the same
// row sums in the same order).
template <int MODE, int LAY>
__global__ __launch_bounds__(256) void spmm_sell_coded_kernel(SellArgs a, int kb, int64_t ldx, int64_t ldy,
                                                              int64_t ldb) {
    constexpr int TABN = LAY == 4 ? 16 : LAY == 8 ? 256 : 1;
    __shared__ double stab[TABN];
    if constexpr (LAY == 4 || LAY == 8) {
        for (int i = threadIdx.x; i < a.ntab; i += 256) stab[i] = a.vtab[i];
        __syncthreads();
    }
    constexpr int SPW = sell_slices_per_wave(LAY, MODE);
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const int wv = __builtin_amdgcn_readfirstlane(blk * 4 + (int)(threadIdx.x >> 6));
    const int sl = wv * (SPW == 2 ? a.spw : 1);
    if (sl >= a.nslices) return;
    for (int c = 0; c < kb; c++) {
        SellArgs b = a;
        b.e.x += c * ldx;
        b.e.y += c * ldy;
        if (b.e.b) b.e.b += c * ldb;
        sell_wave<MODE, LAY>(b, stab, sl);
    }
}

void spmm_sell_coded(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k, SpmvMode mode,
                     const SpmmEpi &epi, hipStream_t s) {
    if (m.sell.nslices == 0) return;
    const int lay = 4;  // (what spmv_sell passes for every coded layout)
    const dim3 block(256);
    for (int64_t c0 = 0; c0 < k; c0 += SPMM_KB) {
        const int kb = (int)std::min<int64_t>(SPMM_KB, k - c0);
        SellArgs a{m.sell.row0.get(), m.sell.soff.get(), m.sell.desc.get(), m.sell.base.get(), m.sell.data.get(), 0,
                   (int32_t)m.sell.nslices,
                   Epi{x + c0 * ldx, y + c0 * ldy, epi.b ? epi.b + c0 * epi.ldb : nullptr, epi.d, nullptr, nullptr, nullptr, 0.0},
                   m.sell.vtab.get(), (int32_t)m.sell.ntab, 1};
        if (sell_slices_per_wave(lay, mode) == 2 && m.sell.nslices >= SELL_PAIR_MIN_SLICES) a.spw = 2;
        const dim3 grid((unsigned)ceil_div(m.sell.nslices, 4 * a.spw * sell_groups_per_wave(lay)));
#define FAMG_SELLC(LAY)                                                                                      \
    switch (mode) {                                                                                        \
    case SPMV_SET: spmm_sell_coded_kernel<SPMV_SET, LAY><<<grid, block, 0, s>>>(a, kb, ldx, ldy, epi.ldb); break;     \
    case SPMV_ADD: spmm_sell_coded_kernel<SPMV_ADD, LAY><<<grid, block, 0, s>>>(a, kb, ldx, ldy, epi.ldb); break;     \
    case SPMV_RESID: spmm_sell_coded_kernel<SPMV_RESID, LAY><<<grid, block, 0, s>>>(a, kb, ldx, ldy, epi.ldb); break; \
    default: spmm_sell_coded_kernel<SPMV_JACOBI, LAY><<<grid, block, 0, s>>>(a, kb, ldx, ldy, epi.ldb); break;        \
    }
        if (m.sell.vbits == 4) { FAMG_SELLC(4) }
        else if (m.sell.vbits == 8) { FAMG_SELLC(8) }
        else { FAMG_SELLC(16) }
#undef FAMG_SELLC
        FAMG_CHECK_HIP(hipGetLastError());
    }
}

// Y = epilogue(A X) on fp64-valued SELL storage, SPMM_KB columns per launch
template <int MODE>
static void spmm_sell_t(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k,
                        const SpmmEpi &epi, hipStream_t s) {
    if (m.sell.nslices == 0) return;
    const dim3 grid((unsigned)ceil_div(m.sell.nslices, 4)), block(256);
    for (int64_t c0 = 0; c0 < k; c0 += SPMM_KB) {
        const int kb = (int)std::min<int64_t>(SPMM_KB, k - c0);
        Epi e{x + c0 * ldx, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        SellArgs a{m.sell.row0.get(), m.sell.soff.get(), m.sell.desc.get(), m.sell.base.get(),
                   m.sell.data.get(), 0, (int32_t)m.sell.nslices, e, nullptr, 0, 1};
        double *yc = y + c0 * ldy;
        const SpmmEpiDev se{epi.b ? epi.b + c0 * epi.ldb : nullptr, epi.ldb, epi.d};
#define FAMG_SELLMM(KB) \
    hipLaunchKernelGGL((spmm_sell_kernel<KB, MODE>), grid, block, 0, s, a, m.sell.paired, ldx, yc, ldy, se)
        switch (kb) {
        case 1: FAMG_SELLMM(1); break;
        case 2: FAMG_SELLMM(2); break;
        case 3: FAMG_SELLMM(3); break;
        case 4: FAMG_SELLMM(4); break;
        case 5: FAMG_SELLMM(5); break;
        case 6: FAMG_SELLMM(6); break;
        case 7: FAMG_SELLMM(7); break;
        default: FAMG_SELLMM(8); break;
        }
#undef FAMG_SELLMM
        FAMG_CHECK_HIP(hipGetLastError());
    }
}

void spmm_sell(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k, hipStream_t s) {
    spmm_sell_t<SPMV_SET>(m, x, ldx, y, ldy, k, SpmmEpi{}, s);
}

void spmm_sell_epi(const GpuCsr &m, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t k, SpmvMode mode,
                   const SpmmEpi &epi, hipStream_t s) {
    switch (mode) {
    case SPMV_SET: spmm_sell_t<SPMV_SET>(m, x, ldx, y, ldy, k, epi, s); break;
    case SPMV_ADD: spmm_sell_t<SPMV_ADD>(m, x, ldx, y, ldy, k, epi, s); break;
    case SPMV_RESID: spmm_sell_t<SPMV_RESID>(m, x, ldx, y, ldy, k, epi, s); break;
    case SPMV_JACOBI: spmm_sell_t<SPMV_JACOBI>(m, x, ldx, y, ldy, k, epi, s); break;
    default: fail(AMG_ERR_INVALID, "SpMM epilogue: mode must be SET, ADD, RESID or JACOBI");
    }
}

}  // namespace famg
