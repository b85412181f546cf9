// partition.hip -- the modularity partitioner (partition_host.cpp) on the
// device: the O(edges) parts of every matching round (candidate edges, the
// matching itself, the contraction) and the swap proposals of every improvement
// pass.  The serial parts -- the total of the row sums, the cut of an over-full
// round, the swap selection -- are the host's own functions, so the two paths
// give the same integers.
//
// A matching round in parallel form (the reference's note at modularity.rs:357,
// "could be par with change of algorithm to Luby's style local max"): every live
// vertex picks the first live edge at it in the pinned order; an edge picked at
// both ends is what the serial sweep would take next there, so it is matched and
// its ends die.  k_mod_choose reads `mate` and writes `choose`; k_mod_match reads
// `choose` and writes only the lane's own `mate` entry: neither launch reads what
// it writes, and no workgroup waits for another.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "handles.hpp"

namespace famg {

namespace {

constexpr int64_t MOD_DEFAULT_PASSES = 256;
constexpr int MOD_CHECK_EVERY = 4;    // passes between two looks at the live count
constexpr int MOD_LANE_ROW = 64;      // longest fine row one lane proposes for; a wave above
constexpr int32_t MOD_LIVE = -1, MOD_ALONE = -2;  // mate[]: still matching / unmatched for good

unsigned grid256(int64_t n) { return (unsigned)std::max<int64_t>(1, ceil_div(n, 256)); }

__global__ void k_mod_init(int64_t n, int32_t *size, int32_t *node_to_v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    size[i] = 1;
    node_to_v[i] = (int32_t)i;
}

// base row sums in stored order, negative sums clamped to 0
__global__ void k_mod_rowsum(const int64_t *rp, const double *val, int64_t n, double *rs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int64_t e = rp[i]; e < rp[i + 1]; e++) s += val[e];
    rs[i] = s < 0.0 ? 0.0 : s;
}

// candidate edges of a round: the entries (i, j) with j < i
__global__ void k_mod_ecount(const int64_t *rp, const int32_t *col, int64_t nv, int64_t *cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    int64_t c = 0;
    for (int64_t e = rp[i]; e < rp[i + 1]; e++) c += col[e] < i;
    cnt[i] = c;
}
__global__ void k_mod_efill(const int64_t *rp, const int32_t *col, const double *val, const double *rs,
                            const int32_t *size, int64_t nv, const int64_t *erp, double inv_total, double cf,
                            double pen, int32_t *ei, int32_t *ej, double *ew, unsigned long long *tcnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    int64_t o = erp[i];
    const int64_t oend = erp[i + 1];
    const double rsi = rs[i];
    const int64_t si = size[i];
    for (int64_t e = rp[i]; e < rp[i + 1] && o < oend; e++) {
        const int64_t j = col[e];
        if (j >= i || j < 0) continue;
        ei[o] = (int32_t)i;
        ej[o] = (int32_t)j;
        ew[o] = mod_edge_weight(val[e], inv_total, rsi, rs[j], si, size[j], cf, pen);
        atomicAdd(&tcnt[j], 1ull);
        o++;
    }
}
// the edges at their smaller end j (any order: a pass takes the first by key)
__global__ void k_mod_tfill(const int32_t *ej, int64_t ne, unsigned long long *cursor, int32_t *tinc) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < ne) tinc[atomicAdd(&cursor[ej[e]], 1ull)] = (int32_t)e;
}

__global__ void k_mod_choose(int64_t nv, const int64_t *erp, const int32_t *ei, const int32_t *ej, const double *ew,
                             const int64_t *trp, const int32_t *tinc, const int32_t *mate, int32_t *choose,
                             unsigned int *live) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool found = false;
    if (v < nv && mate[v] == MOD_LIVE) {
        int64_t best = -1, bi = 0, bj = 0;
        double bw = 0.0;
        for (int64_t e = erp[v]; e < erp[v + 1]; e++) {  // v is the larger end
            const int64_t j = ej[e];
            if (mate[j] != MOD_LIVE) continue;
            if (best < 0 || mod_precedes(ew[e], v, j, bw, bi, bj)) {
                best = e; bw = ew[e]; bi = v; bj = j;
            }
        }
        for (int64_t t = trp[v]; t < trp[v + 1]; t++) {  // v is the smaller end
            const int64_t e = tinc[t], i = ei[e];
            if (mate[i] != MOD_LIVE) continue;
            if (best < 0 || mod_precedes(ew[e], i, v, bw, bi, bj)) {
                best = e; bw = ew[e]; bi = i; bj = v;
            }
        }
        choose[v] = (int32_t)best;
        found = best >= 0;
    }
    const unsigned long long mask = __ballot(found);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(live, (unsigned int)__popcll(mask));
}

// mw[i] = the matched edge's weight at its larger end; *pairs += the pairs made
__global__ void k_mod_match(int64_t nv, const int32_t *ei, const int32_t *ej, const double *ew, const int32_t *choose,
                            int32_t *mate, double *mw, unsigned int *pairs) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool made = false;
    if (v < nv && mate[v] == MOD_LIVE) {
        const int64_t e = choose[v];
        if (e < 0) {
            mate[v] = MOD_ALONE;  // no live edge is left at v, and none comes back
        } else {
            const int64_t i = ei[e], j = ej[e], u = i == v ? j : i;
            if (choose[u] == e) {
                mate[v] = (int32_t)u;
                if (v == i) {
                    mw[v] = ew[e];
                    made = true;
                }
            }
        }
    }
    const unsigned long long mask = __ballot(made);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(pairs, (unsigned int)__popcll(mask));
}

// the serial sweep stops after T + 1 pairs: pairs after the cut key are undone
__global__ void k_mod_cut(int64_t nv, int32_t *mate, const double *mw, double cw, int64_t ci, int64_t cj) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const int64_t m = mate[v];
    if (m < 0) return;
    const int64_t i = v > m ? v : m, j = v > m ? m : v;
    if (mod_precedes(cw, ci, cj, mw[i], i, j)) mate[v] = MOD_ALONE;
}

__device__ __forceinline__ int64_t mod_leader(const int32_t *mate, int64_t v) {
    const int64_t m = mate[v];
    return (m >= 0 && m < v) ? m : v;
}
__global__ void k_mod_leader(int64_t nv, const int32_t *mate, int64_t *flag) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < nv) flag[v] = mod_leader(mate, v) == v;
}
__global__ void k_mod_newlen(int64_t nv, const int32_t *mate, const int64_t *lid, const int64_t *rp, int32_t *lead_of,
                             int64_t *len) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv || mod_leader(mate, v) != v) return;
    const int64_t id = lid[v], m = mate[v];
    lead_of[id] = (int32_t)v;
    len[id] = (rp[v + 1] - rp[v]) + (m >= 0 ? rp[m + 1] - rp[m] : 0);
}
// One lane per merged row: members in ascending old id, their entries in stored
// order under the new ids, sorted stably by id (insertion: rows are short and
// nearly sorted); cnt = the distinct ids.  Row sums and sizes add.
__global__ void k_mod_merge(int64_t q, const int32_t *lead_of, const int32_t *mate, const int64_t *lid,
                            const int64_t *rp, const int32_t *col, const double *val, const double *rs,
                            const int32_t *size, const int64_t *trp, int32_t *tcol, double *tval, int64_t *cnt,
                            double *nrs, int32_t *nsize) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= q) return;
    const int64_t a = lead_of[id], b = mate[a];
    const int64_t o0 = trp[id], o1 = trp[id + 1];
    int64_t o = o0;
    for (int which = 0; which < 2; which++) {
        const int64_t m = which ? b : a;
        if (m < 0) continue;
        for (int64_t e = rp[m]; e < rp[m + 1] && o < o1; e++) {
            const int32_t c = (int32_t)lid[mod_leader(mate, col[e])];
            const double w = val[e];
            int64_t p = o;
            while (p > o0 && tcol[p - 1] > c) {
                tcol[p] = tcol[p - 1];
                tval[p] = tval[p - 1];
                p--;
            }
            tcol[p] = c;
            tval[p] = w;
            o++;
        }
    }
    int64_t u = 0;
    for (int64_t p = o0; p < o; p++) u += p == o0 || tcol[p] != tcol[p - 1];
    cnt[id] = u;
    nrs[id] = b < 0 ? rs[a] : rs[a] + rs[b];
    nsize[id] = b < 0 ? size[a] : size[a] + size[b];
}
__global__ void k_mod_sum(int64_t q, const int64_t *trp, const int32_t *tcol, const double *tval, const int64_t *nrp,
                          int32_t *ncol, double *nval) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= q) return;
    int64_t o = nrp[id];
    const int64_t oend = nrp[id + 1];
    for (int64_t p = trp[id]; p < trp[id + 1] && o < oend;) {
        double sum = tval[p];
        int64_t r = p + 1;
        for (; r < trp[id + 1] && tcol[r] == tcol[p]; r++) sum += tval[r];
        ncol[o] = tcol[p];
        nval[o] = sum;
        o++;
        p = r;
    }
}
__global__ void k_mod_relabel(int64_t n, int32_t *node_to_v, const int32_t *mate, const int64_t *lid) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f < n) node_to_v[f] = (int32_t)lid[mod_leader(mate, node_to_v[f])];
}

// ---- swap proposals (modularity.rs:437-469): the best destination of node i

// in = the strength to i's own aggregate, stored order
__device__ __forceinline__ double mod_in_sum(const int32_t *col, const double *val, const int32_t *agg, int64_t s0,
                                             int64_t s1, int32_t src) {
    double in = 0.0;
    for (int64_t e = s0; e < s1; e++)
        if (agg[col[e]] == src) in += val[e];
    return in;
}
// entry e's aggregate as a destination: false unless e is its first entry in the
// row; out summed in stored order
__device__ __forceinline__ bool mod_dest(const int32_t *col, const double *val, const int32_t *agg, int64_t s0,
                                         int64_t s1, int64_t e, int32_t src, int32_t *dst, double *out) {
    const int32_t a = agg[col[e]];
    if (a == src) return false;
    for (int64_t p = s0; p < e; p++)
        if (agg[col[p]] == a) return false;
    double s = 0.0;
    for (int64_t p = e; p < s1; p++)
        if (agg[col[p]] == a) s += val[p];
    *dst = a;
    *out = s;
    return true;
}
__device__ __forceinline__ void mod_emit(int64_t i, int32_t best, double bdq, int64_t cap, unsigned int *count,
                                         int32_t *pn, int32_t *pa, double *pd) {
    const unsigned int slot = atomicAdd(count, 1u);
    if ((int64_t)slot < cap) {
        pn[slot] = (int32_t)i;
        pa[slot] = best;
        pd[slot] = bdq;
    }
}
__global__ void k_mod_propose_lane(const int64_t *rp, const int32_t *col, const double *val, int64_t n,
                                   const int32_t *agg, const int32_t *size, double cf, double pen, int64_t cap,
                                   unsigned int *count, int32_t *pn, int32_t *pa, double *pd) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t s0 = rp[i], s1 = rp[i + 1];
    const int32_t src = agg[i];
    if (s1 - s0 > MOD_LANE_ROW || size[src] <= 1) return;
    const double in = mod_in_sum(col, val, agg, s0, s1, src);
    int32_t best = -1;
    double bdq = 0.0;
    for (int64_t e = s0; e < s1; e++) {
        int32_t a;
        double out;
        if (!mod_dest(col, val, agg, s0, s1, e, src, &a, &out)) continue;
        const double dq = mod_delta_q(in, out, size[a], size[src], cf, pen);
        if (dq > 0.0 && (best < 0 || dq > bdq || (dq == bdq && a < best))) {
            best = a;
            bdq = dq;
        }
    }
    if (best >= 0) mod_emit(i, best, bdq, cap, count, pn, pa, pd);
}
// rows of more than MOD_LANE_ROW entries, from `rows`: a wave per node, the
// entries dealt over its lanes, the best of the lanes' bests by the same rule
__global__ __launch_bounds__(256) void k_mod_propose_wave(const int64_t *rp, const int32_t *col, const double *val,
                                                          const int32_t *rows, int64_t nrows, const int32_t *agg,
                                                          const int32_t *size, double cf, double pen, int64_t cap,
                                                          unsigned int *count, int32_t *pn, int32_t *pa, double *pd) {
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (q >= nrows) return;  // whole waves leave together
    const int64_t i = rows[q], s0 = rp[i], s1 = rp[i + 1];
    const int32_t src = agg[i];
    if (size[src] <= 1) return;
    const double in = mod_in_sum(col, val, agg, s0, s1, src);
    int32_t best = -1;
    double bdq = 0.0;
    for (int64_t e = s0 + lane; e < s1; e += 64) {
        int32_t a;
        double out;
        if (!mod_dest(col, val, agg, s0, s1, e, src, &a, &out)) continue;
        const double dq = mod_delta_q(in, out, size[a], size[src], cf, pen);
        if (dq > 0.0 && (best < 0 || dq > bdq || (dq == bdq && a < best))) {
            best = a;
            bdq = dq;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t ob = __shfl_xor(best, off);
        const double od = __shfl_xor(bdq, off);
        if (ob >= 0 && (best < 0 || od > bdq || (od == bdq && ob < best))) {
            best = ob;
            bdq = od;
        }
    }
    if (lane == 0 && best >= 0) mod_emit(i, best, bdq, cap, count, pn, pa, pd);
}

__global__ void k_mod_scatter(const int32_t *idx, const int32_t *v, int64_t m, int32_t *dst, int64_t bound) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < m && idx[t] >= 0 && idx[t] < bound) dst[idx[t]] = v[t];
}

template <typename T> void download(std::vector<T> &h, const T *d, int64_t count, hipStream_t s) {
    h.resize(count);
    if (count) FAMG_CHECK_HIP(hipMemcpyAsync(h.data(), d, count * sizeof(T), hipMemcpyDeviceToHost, s));
}

struct MatchedKey {
    double w;
    int32_t i, j;
};

}  // namespace

int64_t partition_modularity_device(const GpuCsr &G, const PartitionerConfig &cfg, std::vector<int64_t> &agg_of,
                                    int64_t *info8) {
    FAMG_REQUIRE(G.nrows == G.ncols, AMG_ERR_INVALID, "graph must be square");
    FAMG_REQUIRE(G.nnz < (int64_t(1) << 31) && G.nrows < (int64_t(1) << 31), AMG_ERR_UNSUPPORTED,
                 "device partitioner: 2^31 or more nodes or edges");
    Ctx &ctx = *G.ctx;
    hipStream_t s = ctx.stream;
    const int64_t n = G.nrows, budget = cfg.max_passes ? cfg.max_passes : MOD_DEFAULT_PASSES;
    int64_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // the fine pattern on the host, once: the row-length test now, the swap selection later
    StrengthGraph H;
    H.n = n;
    download(H.rp, G.rp64.get(), n + 1, s);
    download(H.col, G.col.get(), G.nnz, s);
    if (n == 0) H.rp.assign(1, 0);
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    int64_t longest = 0;
    std::vector<int32_t> longrows;
    for (int64_t i = 0; i < n; i++) {
        const int64_t L = H.rp[i + 1] - H.rp[i];
        longest = std::max(longest, L);
        if (L > MOD_LANE_ROW) longrows.push_back((int32_t)i);
        for (int64_t e = H.rp[i]; e < H.rp[i + 1]; e++)  // the kernels index by these columns
            FAMG_REQUIRE(H.col[e] >= 0 && H.col[e] < n && H.col[e] != i, AMG_ERR_INVALID,
                         "graph rows need columns in range and no self loops");
    }
    auto host_values = [&] {
        download(H.w, G.val.get(), G.nnz, s);
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
    };
    if (longest > SG_MAX_ROW || n == 0) {  // the whole graph on the host partitioner
        host_values();
        const int64_t na = partition_modularity(H, cfg, agg_of, info);
        info[3] = 1;
        if (info8) std::copy(info, info + 8, info8);
        return na;
    }
    // base row sums on the device; their total in ascending order on the host
    DevBuf<double> rs(n), rs2;
    DevBuf<int32_t> size(n), size2, node_to_v(n);
    hipLaunchKernelGGL(k_mod_rowsum, dim3(grid256(n)), dim3(256), 0, s, G.rp64.get(), G.val.get(), n, rs.get());
    hipLaunchKernelGGL(k_mod_init, dim3(grid256(n)), dim3(256), 0, s, n, size.get(), node_to_v.get());
    FAMG_CHECK_HIP(hipGetLastError());
    std::vector<double> hrs;
    download(hrs, rs.get(), n, s);
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    for (double r : hrs)
        FAMG_REQUIRE(std::isfinite(r), AMG_ERR_INVALID, "modularity partitioner: a strength is not finite");
    const double inv_total = mod_inverse_total(hrs);

    // the current graph: G's own arrays in the first round, then the contracted ones
    DevBuf<int64_t> crp;
    DevBuf<int32_t> ccol;
    DevBuf<double> cval;
    const int64_t *rp = G.rp64.get();
    const int32_t *col = G.col.get();
    const double *val = G.val.get();
    int64_t nv = n, nnz = G.nnz;
    bool fell_back = false;
    while ((double)n / (double)nv < cfg.cf) {
        DevBuf<int64_t> ecnt(nv), erp(nv + 1);
        hipLaunchKernelGGL(k_mod_ecount, dim3(grid256(nv)), dim3(256), 0, s, rp, col, nv, ecnt.get());
        FAMG_CHECK_HIP(hipGetLastError());
        const int64_t ne = scan_counts(ecnt.get(), erp.get(), nv, ctx);
        if (ne == 0) break;  // "no more matches are possible"
        DevBuf<int32_t> ei(ne), ej(ne), tinc(ne), mate(nv), choose(nv);
        DevBuf<double> ew(ne), mw(nv);
        DevBuf<unsigned long long> tcnt(nv + 1);
        DevBuf<int64_t> trp(nv + 1);
        DevBuf<unsigned int> ctr(MOD_CHECK_EVERY + 1);  // live counts of a group of passes, then the pairs
        FAMG_CHECK_HIP(hipMemsetAsync(tcnt.get(), 0, (nv + 1) * sizeof(unsigned long long), s));
        hipLaunchKernelGGL(k_mod_efill, dim3(grid256(nv)), dim3(256), 0, s, rp, col, val, rs.get(), size.get(), nv,
                           erp.get(), inv_total, cfg.cf, cfg.pen, ei.get(), ej.get(), ew.get(), tcnt.get());
        FAMG_CHECK_HIP(hipGetLastError());
        const int64_t tne = scan_counts(reinterpret_cast<const int64_t *>(tcnt.get()), trp.get(), nv, ctx);
        FAMG_REQUIRE(tne == ne, AMG_ERR_INVALID, "device partitioner: incidence count mismatch");
        FAMG_CHECK_HIP(hipMemcpyAsync(tcnt.get(), trp.get(), nv * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(k_mod_tfill, dim3(grid256(ne)), dim3(256), 0, s, ej.get(), ne, tcnt.get(), tinc.get());
        FAMG_CHECK_HIP(hipMemsetAsync(mate.get(), 0xff, nv * sizeof(int32_t), s));  // MOD_LIVE
        FAMG_CHECK_HIP(hipMemsetAsync(ctr.get() + MOD_CHECK_EVERY, 0, sizeof(unsigned int), s));
        FAMG_CHECK_HIP(hipGetLastError());
        int64_t passes = 0, prev = nv + 1;
        bool decided = false;
        while (!decided && passes < budget) {
            const int group = (int)std::min<int64_t>(MOD_CHECK_EVERY, budget - passes);
            unsigned int h[MOD_CHECK_EVERY] = {0, 0, 0, 0};
            FAMG_CHECK_HIP(hipMemsetAsync(ctr.get(), 0, MOD_CHECK_EVERY * sizeof(unsigned int), s));
            for (int p = 0; p < group; p++) {
                hipLaunchKernelGGL(k_mod_choose, dim3(grid256(nv)), dim3(256), 0, s, nv, erp.get(), ei.get(), ej.get(),
                                   ew.get(), trp.get(), tinc.get(), mate.get(), choose.get(), ctr.get() + p);
                hipLaunchKernelGGL(k_mod_match, dim3(grid256(nv)), dim3(256), 0, s, nv, ei.get(), ej.get(), ew.get(),
                                   choose.get(), mate.get(), mw.get(), ctr.get() + MOD_CHECK_EVERY);
            }
            FAMG_CHECK_HIP(hipGetLastError());
            FAMG_CHECK_HIP(hipMemcpyAsync(h, ctr.get(), sizeof(h), hipMemcpyDeviceToHost, s));
            FAMG_CHECK_HIP(hipStreamSynchronize(s));
            for (int p = 0; p < group && !decided; p++) {
                decided = h[p] == 0;
                if (!decided) passes++;  // a pass that found live edges matched at least the first of them
            }
            if (!decided) {
                FAMG_REQUIRE((int64_t)h[group - 1] < prev, AMG_ERR_INVALID,
                             "device partitioner: the live vertex count stopped falling");
                prev = h[group - 1];
            }
        }
        info[1] += passes;
        info[2] = std::max(info[2], passes);
        if (!decided) {
            fell_back = true;
            break;
        }
        unsigned int pairs = 0;
        FAMG_CHECK_HIP(hipMemcpyAsync(&pairs, ctr.get() + MOD_CHECK_EVERY, sizeof(pairs), hipMemcpyDeviceToHost, s));
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
        FAMG_REQUIRE(pairs > 0, AMG_ERR_INVALID, "device partitioner: a round with edges matched nothing");
        const int64_t target = (int64_t)std::ceil((double)nv - (double)n / cfg.cf) + 1;
        if ((int64_t)pairs > target + 1) {  // keep the first target + 1 pairs of the order
            std::vector<int32_t> hm;
            std::vector<double> hw;
            download(hm, mate.get(), nv, s);
            download(hw, mw.get(), nv, s);
            FAMG_CHECK_HIP(hipStreamSynchronize(s));
            std::vector<MatchedKey> keys;
            keys.reserve(pairs);
            for (int64_t v = 0; v < nv; v++)
                if (hm[v] >= 0 && hm[v] < v) keys.push_back({hw[v], (int32_t)v, hm[v]});
            FAMG_REQUIRE((int64_t)keys.size() == (int64_t)pairs, AMG_ERR_INVALID, "device partitioner: pair count mismatch");
            std::nth_element(keys.begin(), keys.begin() + target, keys.end(), [](const MatchedKey &a, const MatchedKey &b) {
                return mod_precedes(a.w, a.i, a.j, b.w, b.i, b.j);
            });
            const MatchedKey c = keys[target];
            hipLaunchKernelGGL(k_mod_cut, dim3(grid256(nv)), dim3(256), 0, s, nv, mate.get(), mw.get(), c.w,
                               (int64_t)c.i, (int64_t)c.j);
            FAMG_CHECK_HIP(hipGetLastError());
        }
        info[0]++;
        // contraction
        DevBuf<int64_t> flag(nv), lid(nv + 1);
        hipLaunchKernelGGL(k_mod_leader, dim3(grid256(nv)), dim3(256), 0, s, nv, mate.get(), flag.get());
        FAMG_CHECK_HIP(hipGetLastError());
        const int64_t q = scan_counts(flag.get(), lid.get(), nv, ctx);
        FAMG_REQUIRE(q > 0 && q < nv, AMG_ERR_INVALID, "device partitioner: contraction made no progress");
        DevBuf<int32_t> lead_of(q), tcol(std::max<int64_t>(1, nnz));
        DevBuf<int64_t> len(q), mrp(q + 1), ucnt(q), nrp(q + 1);
        DevBuf<double> tval(std::max<int64_t>(1, nnz));
        hipLaunchKernelGGL(k_mod_newlen, dim3(grid256(nv)), dim3(256), 0, s, nv, mate.get(), lid.get(), rp,
                           lead_of.get(), len.get());
        FAMG_CHECK_HIP(hipGetLastError());
        const int64_t tot = scan_counts(len.get(), mrp.get(), q, ctx);
        FAMG_REQUIRE(tot == nnz, AMG_ERR_INVALID, "device partitioner: merged row lengths do not add up");
        rs2.resize(q);
        size2.resize(q);
        hipLaunchKernelGGL(k_mod_merge, dim3(grid256(q)), dim3(256), 0, s, q, lead_of.get(), mate.get(), lid.get(), rp,
                           col, val, rs.get(), size.get(), mrp.get(), tcol.get(), tval.get(), ucnt.get(), rs2.get(),
                           size2.get());
        FAMG_CHECK_HIP(hipGetLastError());
        const int64_t nnz2 = scan_counts(ucnt.get(), nrp.get(), q, ctx);
        DevBuf<int32_t> ncol(std::max<int64_t>(1, nnz2));
        DevBuf<double> nval(std::max<int64_t>(1, nnz2));
        hipLaunchKernelGGL(k_mod_sum, dim3(grid256(q)), dim3(256), 0, s, q, mrp.get(), tcol.get(), tval.get(), nrp.get(),
                           ncol.get(), nval.get());
        hipLaunchKernelGGL(k_mod_relabel, dim3(grid256(n)), dim3(256), 0, s, n, node_to_v.get(), mate.get(), lid.get());
        FAMG_CHECK_HIP(hipGetLastError());
        FAMG_CHECK_HIP(hipStreamSynchronize(s));  // the round's buffers are released below
        crp = std::move(nrp);
        ccol = std::move(ncol);
        cval = std::move(nval);
        std::swap(rs, rs2);
        std::swap(size, size2);
        rp = crp.get();
        col = ccol.get();
        val = cval.get();
        nv = q;
        nnz = nnz2;
    }
    std::vector<int32_t> h32;
    std::vector<int64_t> hsize;
    if (fell_back) {  // past the pass budget: the host finishes from the current graph
        ModState S;
        S.nv = nv;
        download(S.rp, rp, nv + 1, s);
        download(S.col, col, nnz, s);
        download(S.w, val, nnz, s);
        download(S.rs, rs.get(), nv, s);
        std::vector<int32_t> hs32;
        download(hs32, size.get(), nv, s);
        download(h32, node_to_v.get(), n, s);
        host_values();
        S.size.assign(hs32.begin(), hs32.end());
        S.node_to_v.assign(h32.begin(), h32.end());
        info[3] = 1;
        mod_rounds_host(S, cfg, inv_total, info);
        agg_of = std::move(S.node_to_v);
        mod_improve_host(H, cfg, agg_of, S.size, info);
        const int64_t na = mod_renumber(agg_of, S.nv, info);
        if (info8) std::copy(info, info + 8, info8);
        return na;
    }
    // improvement: proposals on the device, the serial selection on the host
    const int64_t na0 = nv;
    download(h32, node_to_v.get(), n, s);
    std::vector<int32_t> hs32;
    download(hs32, size.get(), na0, s);
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    agg_of.assign(h32.begin(), h32.end());
    hsize.assign(hs32.begin(), hs32.end());
    if (cfg.max_improve > 0) {
        const int64_t nlong = (int64_t)longrows.size();
        DevBuf<int32_t> drows(std::max<int64_t>(1, nlong)), pn(n), pa(n), upi(3 * n), upv(3 * n);
        DevBuf<double> pd(n);
        DevBuf<unsigned int> cnt(1);
        if (nlong)
            FAMG_CHECK_HIP(hipMemcpyAsync(drows.get(), longrows.data(), nlong * sizeof(int32_t), hipMemcpyHostToDevice, s));
        std::vector<ModProposal> props;
        std::vector<int32_t> hn, ha, ui, uv;
        std::vector<double> hd;
        std::vector<int64_t> moved;
        for (int64_t pass = 0; pass < cfg.max_improve; pass++) {
            FAMG_CHECK_HIP(hipMemsetAsync(cnt.get(), 0, sizeof(unsigned int), s));
            hipLaunchKernelGGL(k_mod_propose_lane, dim3(grid256(n)), dim3(256), 0, s, G.rp64.get(), G.col.get(),
                               G.val.get(), n, node_to_v.get(), size.get(), cfg.cf, cfg.pen, n, cnt.get(), pn.get(),
                               pa.get(), pd.get());
            if (nlong)
                hipLaunchKernelGGL(k_mod_propose_wave, dim3((unsigned)ceil_div(nlong, 4)), dim3(256), 0, s,
                                   G.rp64.get(), G.col.get(), G.val.get(), drows.get(), nlong, node_to_v.get(),
                                   size.get(), cfg.cf, cfg.pen, n, cnt.get(), pn.get(), pa.get(), pd.get());
            FAMG_CHECK_HIP(hipGetLastError());
            unsigned int m = 0;
            FAMG_CHECK_HIP(hipMemcpyAsync(&m, cnt.get(), sizeof(m), hipMemcpyDeviceToHost, s));
            FAMG_CHECK_HIP(hipStreamSynchronize(s));
            FAMG_REQUIRE((int64_t)m <= n, AMG_ERR_INVALID, "device partitioner: more proposals than nodes");
            if (m == 0) break;
            download(hn, pn.get(), m, s);
            download(ha, pa.get(), m, s);
            download(hd, pd.get(), m, s);
            FAMG_CHECK_HIP(hipStreamSynchronize(s));
            props.resize(m);
            for (unsigned int t = 0; t < m; t++) props[t] = {hn[t], ha[t], hd[t]};
            moved.clear();
            info[4]++;
            info[5] += mod_select_swaps(props, H.rp.data(), H.col.data(), agg_of, hsize, &moved);
            // only what changed goes back: the moved nodes' aggregates, their aggregates' sizes
            ui.clear();
            uv.clear();
            for (int64_t v : moved) {
                ui.push_back((int32_t)v);
                uv.push_back((int32_t)agg_of[v]);
            }
            const int64_t mn = (int64_t)moved.size();
            // every swap touched two aggregates that no other swap of this pass touched
            std::vector<int32_t> touched;
            for (int64_t v : moved) {
                touched.push_back((int32_t)agg_of[v]);
                touched.push_back(h32[v]);  // where it came from
                h32[v] = (int32_t)agg_of[v];
            }
            for (int32_t a : touched) {
                ui.push_back(a);
                uv.push_back((int32_t)hsize[a]);
            }
            const int64_t mt = (int64_t)touched.size();
            FAMG_CHECK_HIP(hipMemcpyAsync(upi.get(), ui.data(), (mn + mt) * sizeof(int32_t), hipMemcpyHostToDevice, s));
            FAMG_CHECK_HIP(hipMemcpyAsync(upv.get(), uv.data(), (mn + mt) * sizeof(int32_t), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_mod_scatter, dim3(grid256(mn)), dim3(256), 0, s, upi.get(), upv.get(), mn,
                               node_to_v.get(), n);
            hipLaunchKernelGGL(k_mod_scatter, dim3(grid256(mt)), dim3(256), 0, s, upi.get() + mn, upv.get() + mn, mt,
                               size.get(), na0);
            FAMG_CHECK_HIP(hipGetLastError());
            FAMG_CHECK_HIP(hipStreamSynchronize(s));  // ui / uv are reused by the next pass
        }
    }
    const int64_t na = mod_renumber(agg_of, na0, info);
    if (info8) std::copy(info, info + 8, info8);
    return na;
}

}  // namespace famg

// ------------------------------------------------------------------ C ABI

using namespace famg;

extern "C" {

amg_status amg_partition_modularity_device(const amg_linop *graph, const amg_partitioner_config *cfg, int64_t *agg_of,
                                           int64_t *naggs, int64_t *info8) {
    return guard([&] {
        FAMG_REQUIRE(agg_of && naggs, AMG_ERR_INVALID, "null output");
        const PartitionerConfig c = mod_config_from(cfg);
        FAMG_REQUIRE(graph && graph->op, AMG_ERR_INVALID, "null amg_linop handle");
        auto g = std::dynamic_pointer_cast<CsrOp>(graph->op);
        FAMG_REQUIRE(g, AMG_ERR_INVALID, "operator is not a CSR matrix");
        FAMG_REQUIRE(g->nrows == g->ncols, AMG_ERR_INVALID, "graph must be square");
        g->ctx->set_device();
        std::vector<int64_t> agg;
        *naggs = partition_modularity_device(g->m, c, agg, info8);
        std::copy(agg.begin(), agg.end(), agg_of);
    });
}

}  // extern "C"
