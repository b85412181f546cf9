// sagraph.hip -- the two O(nnz) / serial stages of the general SA setup on the
// device (policy amg_set_sa_setup(1), any strength depth): the strength graph and
// the root / claim phase of the MIS aggregation.  DESIGN.md 10.
//
// Restated from the reference (paths relative to its root):
//  * BFS balls        extract_local_subgraph (partitioners/mod.rs:695-718) minus
//                     the centre, the candidates of a dof row at depth >= 2, as a
//                     CSR with ascending columns (k_ball): the host sorts its
//                     candidates by (d, j), so discovery order never shows
//  * strength graph   AdjacencyList::new_ls_strength_graph
//                     (partitioners/mod.rs:337-393), block reduction aggregate +
//                     filter_diag (:294-301, :464-497) -- the arithmetic of
//                     strength_graph (sa.hip), expression for expression, with
//                     one deliberate difference: the weight t^4 is (t*t)*(t*t)
//                     where the host calls std::pow(t, 4.0) (<= 2 ULP apart)
//  * aggregation      maximal_independent_set (:395-423) as sa.hip's
//                     aggregate_mis runs it, in its parallel form: with u
//                     preceding v when deg[u] > deg[v] or (equal and u < v), and
//                     H(v) the in-neighbours of v that precede it, v is claimed
//                     once some u in H(v) is a root and a root once every u in
//                     H(v) is claimed.  Decisions are final, so bounded passes
//                     update in place; the host watches the undecided count.
//                     The singleton / renumbering tail stays on the host
//                     (aggregate_finish, sa.hip): it is order dependent.
#include <algorithm>
#include <cstring>

#include "handles.hpp"

namespace famg {

int g_sa_setup = 0;  // amg_set_sa_setup: 0 host (default), 1 device

constexpr int SG_WAVE_CAP = 256;    // candidates a wave ranks in LDS
constexpr int SG_BLOCK_CAP = 4096;  // candidates a workgroup ranks in LDS (SG_MAX_ROW)
static_assert(SG_BLOCK_CAP == SG_MAX_ROW, "famg.hpp's bound is the workgroup kernel's");

// ------------------------------------------------------------ strength graph

// v_i W v_i^T floored at 1e-30, one lane per dof, ascending c
__global__ void k_sg_vn(const double *nn, int64_t ld, int64_t k, const double *w, int64_t n, double *vn) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int64_t c = 0; c < k; c++) s += (nn[i + c * ld] * w[c]) * nn[i + c * ld];
    vn[i] = s < 1e-30 ? 1e-30 : s;
}

// position of the diagonal entry among the row's entries [s0, s1) (columns
// ascending), s1 when the row stores none
__device__ __forceinline__ int64_t sg_diag_pos(const int32_t *col, int64_t s0, int64_t s1, int64_t i) {
    int64_t lo = s0, hi = s1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (col[mid] < i) lo = mid + 1;
        else hi = mid;
    }
    return (lo < s1 && col[lo] == i) ? lo : s1;
}

// kept entries per dof row: max(L / 2, 1) of its L off-diagonal entries, 0 for
// L = 0.  Rows of more than SG_WAVE_CAP candidates go on the workgroup kernel's
// list; maxlen = the longest of them.
__global__ void k_sg_count(const int64_t *rp, const int32_t *col, int64_t n, int64_t *cnt, int32_t *longrows,
                           unsigned int *nlong, unsigned long long *maxlen) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t s0 = rp[i], s1 = rp[i + 1];
    const int64_t L = (s1 - s0) - (sg_diag_pos(col, s0, s1, i) < s1 ? 1 : 0);
    cnt[i] = L == 0 ? 0 : (L / 2 > 1 ? L / 2 : 1);
    if (L > SG_WAVE_CAP) {
        longrows[atomicAdd(nlong, 1u)] = (int32_t)i;
        atomicMax(maxlen, (unsigned long long)L);
    }
}

// One dof row per GROUP lanes (64: a wave, rows of <= CAP = 256 candidates; 256:
// the workgroup, rows from `rowlist`).  Each candidate's distance by one lane,
// its rank among the keys (d, j) by counting smaller keys in LDS, the kept ones
// (rank < keep) written in ascending column order: the position is the number
// of kept candidates stored before it (ballots per 64 candidates).
template <int GROUP, int CAP>
__global__ __launch_bounds__(256) void k_sg_fill(const int64_t *rp, const int32_t *col, const double *nn, int64_t ld,
                                                 int64_t k, const double *w, const double *vn, int64_t nrows,
                                                 const int32_t *rowlist, const int64_t *drp, int32_t *dcol,
                                                 double *dw) {
    constexpr int RPB = 256 / GROUP, IT = CAP / GROUP, CH = CAP / 64;
    __shared__ double sd[RPB][CAP];
    __shared__ int32_t sj[RPB][CAP];
    __shared__ double sdm[RPB][2];
    __shared__ int32_t scnt[RPB][CH];
    const int g = threadIdx.x / GROUP, t = threadIdx.x % GROUP, lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * RPB; base < nrows; base += (int64_t)gridDim.x * RPB) {
        const int64_t q = base + g;
        int64_t i = -1, s0 = 0, p = 0;
        int L = 0;
        if (q < nrows) {
            i = rowlist ? (int64_t)rowlist[q] : q;
            s0 = rp[i];
            const int64_t s1 = rp[i + 1];
            p = sg_diag_pos(col, s0, s1, i);
            const int64_t Lr = (s1 - s0) - (p < s1 ? 1 : 0);
            L = Lr > CAP ? 0 : (int)Lr;  // longer rows belong to the workgroup kernel
            p -= s0;
        }
        for (int u = t; u < L; u += GROUP) {
            const int64_t j = col[s0 + (u < p ? u : u + 1)];
            // the pair is always evaluated as (min, max): one value per edge
            const int64_t a = i < j ? i : j, b = i < j ? j : i;
            double x = 0.0;
            for (int64_t c = 0; c < k; c++) x += (nn[a + c * ld] * w[c]) * nn[b + c * ld];
            const double rho2 = (x * x) / (vn[a] * vn[b]);
            double om = 1.0 - rho2;
            om = om < 0.0 ? 0.0 : om;
            sd[g][u] = 2.0 * sqrt(om);
            sj[g][u] = (int32_t)j;
        }
        if (t < 2) sdm[g][t] = 0.0;
        __syncthreads();
        const int keep = L / 2 > 1 ? L / 2 : 1;
        int rk[IT];
        unsigned long long km[IT];
#pragma unroll
        for (int it = 0; it < IT; it++) {
            const int u = t + it * GROUP;
            int r = CAP;
            if (u < L) {
                const double du = sd[g][u];
                const int32_t ju = sj[g][u];
                r = 0;
                for (int v = 0; v < L; v++) {
                    const double dv = sd[g][v];
                    r += (dv < du || (!(du < dv) && sj[g][v] < ju)) ? 1 : 0;
                }
                if (r == 0) sdm[g][0] = du;
                if (r == keep - 1) sdm[g][1] = du;
            }
            rk[it] = r;
            km[it] = __ballot(r < keep);
            if (lane == 0) scnt[g][(t >> 6) + it * (GROUP >> 6)] = (int32_t)__popcll(km[it]);
        }
        __syncthreads();
        const double dmin = sdm[g][0], dmax = sdm[g][1];
#pragma unroll
        for (int it = 0; it < IT; it++) {
            const int u = t + it * GROUP;
            if (u < L && rk[it] < keep) {
                const int ch = (t >> 6) + it * (GROUP >> 6);
                int pos = __popcll(km[it] & ((1ull << lane) - 1ull));
                for (int c = 0; c < ch; c++) pos += scnt[g][c];
                double wt;
                if (fabs(dmax - dmin) < 1e-12) wt = 1.0;
                else {
                    const double tt = (dmax - sd[g][u]) / (dmax - dmin + 1e-12);
                    wt = (tt * tt) * (tt * tt);  // alpha = 4; the host's std::pow(t, 4.0)
                }
                if (pos < keep) {  // always, for distinct columns
                    dcol[drp[i] + pos] = sj[g][u];
                    dw[drp[i] + pos] = wt;
                }
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int64_t sg_lower_bound(const int32_t *col, int64_t lo, int64_t hi, int64_t key) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (col[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Block reduction, one lane per node: the bs kept lists of the node's dofs
// (columns ascending) merged by neighbour id j / bs in ascending id; equal ids
// summed left to right in (dof ascending, column ascending) order.  FILL =
// false counts the ids other than the node itself; FILL = true stores them with
// their sums and folds every sum, self loops included, into the global maximum
// (sums are >= 0: their bit patterns order as the values do).
template <bool FILL>
__global__ void k_sg_node(const int64_t *drp, const int32_t *dcol, const double *dw, int64_t nnodes, int64_t bs,
                          int64_t *cnt, const int64_t *grp, int32_t *gcol, double *gval, unsigned long long *gmax) {
    const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double lm = 0.0;
    if (I < nnodes) {
        int64_t J = -1, c = 0, o = FILL ? grp[I] : 0;
        for (;;) {
            int64_t next = INT64_MAX;
            for (int64_t r = 0; r < bs; r++) {
                const int64_t e1 = drp[I * bs + r + 1];
                const int64_t lb = sg_lower_bound(dcol, drp[I * bs + r], e1, (J + 1) * bs);
                if (lb < e1) {
                    const int64_t id = dcol[lb] / bs;
                    next = id < next ? id : next;
                }
            }
            if (next == INT64_MAX) break;
            J = next;
            if (FILL) {
                double sum = 0.0;
                bool first = true;
                for (int64_t r = 0; r < bs; r++) {
                    const int64_t e1 = drp[I * bs + r + 1];
                    for (int64_t e = sg_lower_bound(dcol, drp[I * bs + r], e1, J * bs); e < e1 && dcol[e] < (J + 1) * bs;
                         e++) {
                        sum = first ? dw[e] : sum + dw[e];
                        first = false;
                    }
                }
                lm = lm < sum ? sum : lm;
                if (J != I) {
                    gcol[o] = (int32_t)J;
                    gval[o] = sum;
                    o++;
                }
            } else {
                c += J != I;
            }
        }
        if (!FILL) cnt[I] = c;
    }
    if (FILL) {
        unsigned long long v = (unsigned long long)__double_as_longlong(lm);
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o2 = __shfl_xor(v, off);
            v = v > o2 ? v : o2;
        }
        if ((threadIdx.x & 63) == 0 && v) atomicMax(gmax, v);
    }
}

__global__ void k_sg_scale(double *val, int64_t nnz, double gmax) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < nnz) val[e] = val[e] / gmax;
}

static unsigned grid256(int64_t n) { return (unsigned)std::max<int64_t>(1, ceil_div(n, 256)); }

// ------------------------------------------------------------ BFS balls

constexpr int BALL_SUB = 16;  // lanes that walk one frontier member's row together

// v joins the visited set `tab` (SLOTS words, -1 = free): true for the lane that
// put it there.  Multiplicative hash (ids that differ by multiples of a power of two
// spread), linear probing; the callers keep free slots in the table.
template <int SLOTS>
__device__ __forceinline__ bool ball_insert(int32_t *tab, int32_t v) {
    static_assert((SLOTS & (SLOTS - 1)) == 0, "a power of two");
    unsigned h = ((unsigned)v * 2654435761u) >> (32 - __builtin_ctz(SLOTS));
    for (int p = 0; p < SLOTS; p++) {
        const int32_t old = atomicCAS(&tab[h], -1, v);
        if (old == -1) return true;
        if (old == v) return false;
        h = (h + 1) & (SLOTS - 1);
    }
    return false;
}

// The ball of one row per GROUP lanes (64: a wave, balls of <= CAP = 256 members,
// four rows per workgroup; 256: the workgroup, rows from `rowlist`, CAP = 4096).
// The visited set is a hash table in LDS; the member list (without the centre) is
// appended through an LDS counter and is the BFS queue as well: level d is the
// slice of it that level d - 1 appended.  A lane stops inserting once the counter
// has passed CAP, so at most CAP + GROUP members and the centre are ever in the
// table, which therefore never fills.
// FILL = false: cnt[i] = the ball's size, *kept += what the strength graph keeps of
// it, *maxlen = the longest; a ball beyond CAP goes on `longrows` (GROUP 64) or is
// reported through *maxlen alone with cnt[i] = 0 (GROUP 256).
// FILL = true: the members sorted ascending (rank by counting in a wave, a bitonic
// network in the workgroup) into bcol[brp[i] ...); rows whose size is not in
// (0, CAP] are another launch's.
template <int GROUP, int CAP, int SLOTS, bool FILL>
__global__ __launch_bounds__(256) void k_ball(const int64_t *rp, const int32_t *col, int depth, int64_t nrows,
                                              const int32_t *rowlist, int64_t *cnt, int32_t *longrows,
                                              unsigned int *nlong, unsigned long long *maxlen,
                                              unsigned long long *kept, const int64_t *brp, int32_t *bcol) {
    constexpr int RPB = 256 / GROUP;
    static_assert(2 * SLOTS >= 3 * (CAP + GROUP + 1), "the table stays under two thirds full");
    __shared__ int32_t tab[RPB][SLOTS];
    __shared__ int32_t list[RPB][CAP];
    __shared__ int scnt[RPB];
    const int g = threadIdx.x / GROUP, t = threadIdx.x % GROUP;
    for (int64_t base = (int64_t)blockIdx.x * RPB; base < nrows; base += (int64_t)gridDim.x * RPB) {
        const int64_t q = base + g;
        const int64_t i = q < nrows ? (rowlist ? (int64_t)rowlist[q] : q) : -1;
        bool live = i >= 0;
        int64_t len = 0;
        if (FILL && live) {
            len = brp[i + 1] - brp[i];
            live = len > 0 && len <= CAP;
        }
        for (int s = t; s < SLOTS; s += GROUP) tab[g][s] = -1;
        if (t == 0) scnt[g] = 0;
        __syncthreads();
        if (live && t == 0) ball_insert<SLOTS>(tab[g], (int32_t)i);
        __syncthreads();
        int lo = 0, hi = 0, c = 0;
        bool more = live;  // this row's BFS still has a frontier and room
        for (int d = 0; d < depth; d++) {
            const int nf = d == 0 ? 1 : hi - lo;
            if (more)
                for (int f = t / BALL_SUB; f < nf; f += GROUP / BALL_SUB) {
                    const int64_t u = d == 0 ? i : (int64_t)list[g][lo + f];
                    const int64_t e1 = rp[u + 1];
                    for (int64_t e = rp[u] + t % BALL_SUB; e < e1; e += BALL_SUB) {
                        if (__hip_atomic_load(&scnt[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) > CAP) break;
                        const int32_t v = col[e];
                        if (ball_insert<SLOTS>(tab[g], v)) {
                            const int pos = atomicAdd(&scnt[g], 1);
                            if (pos < CAP) list[g][pos] = v;
                        }
                    }
                }
            __syncthreads();
            c = scnt[g];
            lo = hi;
            hi = c < CAP ? c : CAP;
            more = more && c <= CAP && hi > lo;
            if (!__syncthreads_or(more)) break;
        }
        // the loop left through a barrier: c and the list are final for every lane
        if constexpr (!FILL) {
            if (live && t == 0) {
                if (c <= CAP) {
                    cnt[i] = c;
                    if (c) atomicAdd(kept, (unsigned long long)(c / 2 > 1 ? c / 2 : 1));
                    atomicMax(maxlen, (unsigned long long)c);
                } else if (GROUP == 64) {
                    cnt[i] = 0;
                    longrows[atomicAdd(nlong, 1u)] = (int32_t)i;
                } else {
                    cnt[i] = 0;
                    atomicMax(maxlen, (unsigned long long)c);
                }
            }
        } else if constexpr (GROUP == 64) {
            if (live && c == (int)len)
                for (int u = t; u < c; u += GROUP) {
                    const int32_t ju = list[g][u];
                    int r = 0;
                    for (int v = 0; v < c; v++) r += list[g][v] < ju ? 1 : 0;
                    bcol[brp[i] + r] = ju;
                }
        } else {
            // RPB == 1: live, c and len are the workgroup's
            const bool ok = live && c == (int)len;
            int m = 1;
            while (m < c) m <<= 1;
            if (ok) {
                for (int u = c + t; u < m; u += GROUP) list[g][u] = INT32_MAX;
                __syncthreads();
                for (int kk = 2; kk <= m; kk <<= 1)
                    for (int j = kk >> 1; j > 0; j >>= 1) {
                        for (int u = t; u < m; u += GROUP) {
                            const int x = u ^ j;
                            if (x > u) {
                                const int32_t a = list[g][u], b = list[g][x];
                                if ((a > b) == ((u & kk) == 0)) {
                                    list[g][u] = b;
                                    list[g][x] = a;
                                }
                            }
                        }
                        __syncthreads();
                    }
                for (int u = t; u < c; u += GROUP) bcol[brp[i] + u] = list[g][u];
            }
        }
        __syncthreads();
    }
}

__global__ void k_ball_ones(double *val, int64_t nnz) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < nnz) val[e] = 1.0;
}

constexpr int BALL_WAVE_SLOTS = 1024, BALL_BLOCK_SLOTS = 8192;

int ball_pattern_device(const GpuCsr &m, int64_t depth, bool check_bytes, int64_t max_bytes, BallPattern &out) {
    FAMG_REQUIRE(m.nrows == m.ncols, AMG_ERR_DIM, "pattern ball: matrix must be square");
    FAMG_REQUIRE(depth >= 1, AMG_ERR_INVALID, "pattern ball: depth must be >= 1");
    FAMG_REQUIRE(max_bytes >= 0, AMG_ERR_INVALID, "pattern ball: negative byte budget");
    Ctx &ctx = *m.ctx;
    hipStream_t s = ctx.stream;
    const int64_t n = m.nrows;
    const int d = (int)std::min<int64_t>(depth, std::max<int64_t>(1, n));  // a BFS settles within n levels
    out = BallPattern{};
    DevBuf<int64_t> cnt(std::max<int64_t>(1, n));
    DevBuf<int32_t> longrows(std::max<int64_t>(1, n));
    DevBuf<unsigned long long> meta(3);  // {long rows (low 32 bits), longest ball, kept entries}
    FAMG_CHECK_HIP(hipMemsetAsync(meta.get(), 0, 3 * sizeof(unsigned long long), s));
    unsigned long long hmeta[3] = {0, 0, 0};
    const unsigned gw = (unsigned)std::min<int64_t>(std::max<int64_t>(1, ceil_div(n, 4)), int64_t(1) << 20);
    if (n) {
        hipLaunchKernelGGL((k_ball<64, SG_WAVE_CAP, BALL_WAVE_SLOTS, false>), dim3(gw), dim3(256), 0, s, m.rp64.get(),
                           m.col.get(), d, n, (const int32_t *)nullptr, cnt.get(), longrows.get(),
                           reinterpret_cast<unsigned int *>(meta.get()), meta.get() + 1, meta.get() + 2,
                           (const int64_t *)nullptr, (int32_t *)nullptr);
        FAMG_CHECK_HIP(hipGetLastError());
        FAMG_CHECK_HIP(hipMemcpyAsync(hmeta, meta.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
    }
    const int64_t nlong = (int64_t)(hmeta[0] & 0xffffffffull);
    if (nlong) {
        hipLaunchKernelGGL((k_ball<256, SG_BLOCK_CAP, BALL_BLOCK_SLOTS, false>),
                           dim3((unsigned)std::min<int64_t>(nlong, 65536)), dim3(256), 0, s, m.rp64.get(), m.col.get(),
                           d, nlong, longrows.get(), cnt.get(), (int32_t *)nullptr, (unsigned int *)nullptr,
                           meta.get() + 1, meta.get() + 2, (const int64_t *)nullptr, (int32_t *)nullptr);
        FAMG_CHECK_HIP(hipGetLastError());
    }
    DevBuf<int64_t> brp(n + 1);
    const int64_t entries = scan_counts(cnt.get(), brp.get(), n, ctx);  // synchronises
    FAMG_CHECK_HIP(hipMemcpyAsync(hmeta, meta.get(), sizeof(hmeta), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    out.entries = entries;
    out.longest = (int64_t)hmeta[1];
    out.block_rows = nlong;
    out.wave_rows = n - nlong;
    out.kept = (int64_t)hmeta[2];
    if (out.longest > SG_BLOCK_CAP) return SG_REASON_BALL_CAP;
    if (entries >= (int64_t(1) << 31) || out.kept >= (int64_t(1) << 31)) return SG_REASON_INDEX;
    if (check_bytes) {
        int64_t budget = max_bytes;
        if (budget == 0) {
            size_t fr = 0, tot = 0;
            FAMG_CHECK_HIP(hipMemGetInfo(&fr, &tot));
            budget = (int64_t)(fr / 2);
        }
        if (4 * entries + 8 * (n + 1) + 12 * out.kept > budget) return SG_REASON_BYTES;
    }
    DevBuf<int32_t> bcol(std::max<int64_t>(1, entries));
    if (n && entries) {
        hipLaunchKernelGGL((k_ball<64, SG_WAVE_CAP, BALL_WAVE_SLOTS, true>), dim3(gw), dim3(256), 0, s, m.rp64.get(),
                           m.col.get(), d, n, (const int32_t *)nullptr, (int64_t *)nullptr, (int32_t *)nullptr,
                           (unsigned int *)nullptr, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                           brp.get(), bcol.get());
        if (nlong)
            hipLaunchKernelGGL((k_ball<256, SG_BLOCK_CAP, BALL_BLOCK_SLOTS, true>),
                               dim3((unsigned)std::min<int64_t>(nlong, 65536)), dim3(256), 0, s, m.rp64.get(),
                               m.col.get(), d, nlong, longrows.get(), (int64_t *)nullptr, (int32_t *)nullptr,
                               (unsigned int *)nullptr, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                               brp.get(), bcol.get());
        FAMG_CHECK_HIP(hipGetLastError());
    }
    FAMG_CHECK_HIP(hipStreamSynchronize(s));  // the counts and the row list are released here
    out.rp = std::move(brp);
    out.col = std::move(bcol);
    return SG_REASON_NONE;
}

static const char *sg_reason_text(int reason) {
    switch (reason) {
    case SG_REASON_BALL_CAP: return "device strength graph: a row has more than 4096 candidates";
    case SG_REASON_BYTES: return "device strength graph: the ball pattern and the dof graph exceed the byte budget";
    case SG_REASON_INDEX: return "device strength graph: 2^31 or more ball or kept entries";
    default: return "device strength graph: unsupported";
    }
}

CsrPtr strength_graph_device(const CsrOp &A, const double *nn, int64_t ld, int64_t k, const double *w, int64_t bs,
                             int64_t depth, int64_t max_bytes, SgDeviceInfo *info, bool fallback) {
    FAMG_REQUIRE(A.nrows == A.ncols, AMG_ERR_DIM, "strength graph: matrix must be square");
    FAMG_REQUIRE(bs >= 1 && A.nrows % bs == 0, AMG_ERR_DIM, "strength graph: block size must divide n");
    FAMG_REQUIRE(k >= 1 && ld >= A.nrows && depth >= 1 && max_bytes >= 0, AMG_ERR_INVALID,
                 "strength graph: bad near-null block, depth or byte budget");
    SgDeviceInfo local;
    SgDeviceInfo &inf = info ? *info : local;
    inf = SgDeviceInfo{};
    auto cannot = [&](int reason) -> CsrPtr {
        inf.reason = reason;
        if (!fallback) fail(AMG_ERR_UNSUPPORTED, sg_reason_text(reason));
        return nullptr;
    };
    Ctx *ctx = A.ctx;
    hipStream_t s = ctx->stream;
    const GpuCsr &m = A.m;
    const int64_t n = A.nrows;
    // depth >= 2: the candidates of a row are its BFS ball; the kernels below take
    // them from the ball's rp / col exactly as depth 1 takes them from the matrix's
    BallPattern ball;
    if (depth > 1) {
        const int reason = ball_pattern_device(m, depth, true, max_bytes, ball);
        inf.longest_ball = ball.longest;
        inf.wave_rows = ball.wave_rows;
        inf.block_rows = ball.block_rows;
        inf.ball_entries = ball.entries;
        if (reason != SG_REASON_NONE) return cannot(reason);
    }
    const int64_t *crp = depth > 1 ? ball.rp.get() : m.rp64.get();
    const int32_t *ccol = depth > 1 ? ball.col.get() : m.col.get();
    DevBuf<double> wd(k), vn(std::max<int64_t>(1, n));
    FAMG_CHECK_HIP(hipMemcpyAsync(wd.get(), w, k * sizeof(double), hipMemcpyHostToDevice, s));
    DevBuf<int64_t> cnt(std::max<int64_t>(1, n));
    DevBuf<int32_t> longrows(std::max<int64_t>(1, n));
    DevBuf<unsigned long long> meta(3);  // {long rows (low 32 bits), longest row, gmax bits}
    FAMG_CHECK_HIP(hipMemsetAsync(meta.get(), 0, 3 * sizeof(unsigned long long), s));
    auto D = make_csr(ctx);  // the dof-level graph (the result when bs == 1)
    if (n) {
        hipLaunchKernelGGL(k_sg_vn, dim3(grid256(n)), dim3(256), 0, s, nn, ld, k, wd.get(), n, vn.get());
        hipLaunchKernelGGL(k_sg_count, dim3(grid256(n)), dim3(256), 0, s, crp, ccol, n, cnt.get(), longrows.get(),
                           reinterpret_cast<unsigned int *>(meta.get()), meta.get() + 1);
        FAMG_CHECK_HIP(hipGetLastError());
    }
    DevBuf<int64_t> drp(n + 1);
    const int64_t dnnz = scan_counts(cnt.get(), drp.get(), n, *ctx);  // synchronises
    unsigned long long hmeta[2] = {0, 0};
    FAMG_CHECK_HIP(hipMemcpyAsync(hmeta, meta.get(), sizeof(hmeta), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    const int64_t nlong = (int64_t)(hmeta[0] & 0xffffffffull);
    if (depth == 1) {
        inf.longest_ball = (int64_t)hmeta[1];
        inf.wave_rows = n - nlong;
        inf.block_rows = nlong;
    }
    inf.dof_entries = dnnz;
    if ((int64_t)hmeta[1] > SG_BLOCK_CAP) return cannot(SG_REASON_BALL_CAP);
    if (dnnz >= (int64_t(1) << 31)) return cannot(SG_REASON_INDEX);
    csr_alloc(D->m, ctx, n, n, dnnz);
    D->m.rp64 = std::move(drp);
    D->nrows = D->ncols = n;
    if (n) {
        const unsigned gw = (unsigned)std::min<int64_t>(ceil_div(n, 4), int64_t(1) << 20);
        hipLaunchKernelGGL((k_sg_fill<64, SG_WAVE_CAP>), dim3(gw), dim3(256), 0, s, crp, ccol, nn, ld, k, wd.get(),
                           vn.get(), n, (const int32_t *)nullptr, D->m.rp64.get(), D->m.col.get(), D->m.val.get());
        if (nlong)
            hipLaunchKernelGGL((k_sg_fill<256, SG_BLOCK_CAP>), dim3((unsigned)std::min<int64_t>(nlong, 65536)),
                               dim3(256), 0, s, crp, ccol, nn, ld, k, wd.get(), vn.get(), nlong, longrows.get(),
                               D->m.rp64.get(), D->m.col.get(), D->m.val.get());
        FAMG_CHECK_HIP(hipGetLastError());
    }
    if (depth > 1) {  // the ball goes before the node-level merge allocates
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
        ball.col.release();
        ball.rp.release();
    }
    if (bs == 1) {
        FAMG_CHECK_HIP(hipStreamSynchronize(s));  // wd, vn and the row list are released here
        inf.node_edges = dnnz;
        return D;
    }
    const int64_t nnodes = n / bs;
    DevBuf<int64_t> ncnt(std::max<int64_t>(1, nnodes)), grp(nnodes + 1);
    if (nnodes)
        hipLaunchKernelGGL((k_sg_node<false>), dim3(grid256(nnodes)), dim3(256), 0, s, D->m.rp64.get(), D->m.col.get(),
                           D->m.val.get(), nnodes, bs, ncnt.get(), (const int64_t *)nullptr, (int32_t *)nullptr,
                           (double *)nullptr, (unsigned long long *)nullptr);
    FAMG_CHECK_HIP(hipGetLastError());
    const int64_t gnnz = scan_counts(ncnt.get(), grp.get(), nnodes, *ctx);
    auto G = make_csr(ctx);
    csr_alloc(G->m, ctx, nnodes, nnodes, gnnz);
    G->m.rp64 = std::move(grp);
    G->nrows = G->ncols = nnodes;
    if (nnodes)
        hipLaunchKernelGGL((k_sg_node<true>), dim3(grid256(nnodes)), dim3(256), 0, s, D->m.rp64.get(), D->m.col.get(),
                           D->m.val.get(), nnodes, bs, (int64_t *)nullptr, G->m.rp64.get(), G->m.col.get(),
                           G->m.val.get(), meta.get() + 2);
    FAMG_CHECK_HIP(hipGetLastError());
    unsigned long long gbits = 0;
    FAMG_CHECK_HIP(hipMemcpyAsync(&gbits, meta.get() + 2, sizeof(gbits), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    double gmax;
    std::memcpy(&gmax, &gbits, sizeof(gmax));
    FAMG_REQUIRE(gmax > 0.0, AMG_ERR_INVALID, "strength graph has no edges");
    if (gnnz) hipLaunchKernelGGL(k_sg_scale, dim3(grid256(gnnz)), dim3(256), 0, s, G->m.val.get(), gnnz, gmax);
    FAMG_CHECK_HIP(hipGetLastError());
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    inf.node_edges = gnnz;
    return G;
}

// ------------------------------------------------------------ aggregation

// strength degree: the row's weights summed in stored order by one lane
__global__ void k_mis_deg(const int64_t *rp, const double *val, int64_t n, double *deg) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int64_t e = rp[i]; e < rp[i + 1]; e++) s += val[e];
    deg[i] = s;
}

// the transposed pattern (rows = in-neighbours; their order within a row is
// free: the passes take "any" and "the first by precedence" over them)
__global__ void k_mis_tcount(const int32_t *col, int64_t nnz, unsigned long long *cnt) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < nnz) atomicAdd(&cnt[col[e]], 1ull);
}
__global__ void k_mis_tfill(const int64_t *rp, const int32_t *col, int64_t n, unsigned long long *cursor,
                            int32_t *tcol) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int64_t e = rp[i]; e < rp[i + 1]; e++) tcol[atomicAdd(&cursor[col[e]], 1ull)] = (int32_t)i;
}

__device__ __forceinline__ bool mis_precedes(double du, int64_t u, double dv, int64_t v) {
    return du > dv || (du == dv && u < v);
}

enum : int { MIS_UNDECIDED = 0, MIS_ROOT = 1, MIS_CLAIMED = 2 };

// One pass over the nodes still undecided.  A decision reads only final states
// (an undecided in-neighbour read late is read as undecided: the node waits a
// pass longer), so the passes update in place.  *undecided += the nodes this
// pass left waiting.
__global__ void k_mis_pass(const int64_t *trp, const int32_t *tcol, const double *deg, int64_t n, int32_t *state,
                           unsigned int *undecided) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool waits = false;
    if (v < n && state[v] == MIS_UNDECIDED) {
        const double dv = deg[v];
        bool claimed = false;
        for (int64_t e = trp[v]; e < trp[v + 1] && !claimed; e++) {
            const int64_t u = tcol[e];
            if (u == v || !mis_precedes(deg[u], u, dv, v)) continue;
            const int32_t su = __hip_atomic_load(&state[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (su == MIS_ROOT) claimed = true;
            else if (su == MIS_UNDECIDED) waits = true;
        }
        if (claimed) waits = false;
        if (claimed || !waits)
            __hip_atomic_store(&state[v], claimed ? MIS_CLAIMED : MIS_ROOT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned long long mask = __ballot(waits);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(undecided, (unsigned int)__popcll(mask));
}

// owner(v): v itself for a root, else the root in H(v) that precedes all others
__global__ void k_mis_owner(const int64_t *trp, const int32_t *tcol, const double *deg, int64_t n,
                            const int32_t *state, int32_t *owner) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    if (state[v] == MIS_ROOT) {
        owner[v] = (int32_t)v;
        return;
    }
    const double dv = deg[v];
    int64_t best = -1;
    double db = 0.0;
    for (int64_t e = trp[v]; e < trp[v + 1]; e++) {
        const int64_t u = tcol[e];
        if (u == v || state[u] != MIS_ROOT) continue;
        const double du = deg[u];
        if (!mis_precedes(du, u, dv, v)) continue;
        if (best < 0 || mis_precedes(du, u, db, best)) {
            best = u;
            db = du;
        }
    }
    owner[v] = (int32_t)best;
}

__global__ void k_mis_rowlen(const int64_t *rp, const int32_t *rows, int64_t m, int64_t *len) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q < m) len[q] = rp[rows[q] + 1] - rp[rows[q]];
}
__global__ void k_mis_rowcopy(const int64_t *rp, const int32_t *col, const double *val, const int32_t *rows, int64_t m,
                              const int64_t *off, int32_t *ocol, double *oval) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= m) return;
    const int64_t s0 = rp[rows[q]], len = rp[rows[q] + 1] - s0, o = off[q];
    for (int64_t e = 0; e < len; e++) {
        ocol[o + e] = col[s0 + e];
        oval[o + e] = val[s0 + e];
    }
}

constexpr int64_t MIS_DEFAULT_PASSES = 1024;
constexpr int MIS_CHECK_EVERY = 4;  // passes between two looks at the undecided count

int64_t aggregate_mis_device(const GpuCsr &G, int64_t max_passes, std::vector<int64_t> &agg_of, int64_t *info4) {
    FAMG_REQUIRE(G.nrows == G.ncols, AMG_ERR_DIM, "graph must be square");
    FAMG_REQUIRE(max_passes >= 0, AMG_ERR_INVALID, "aggregation: negative pass budget");
    Ctx &ctx = *G.ctx;
    hipStream_t s = ctx.stream;
    const int64_t n = G.nrows, budget = max_passes ? max_passes : MIS_DEFAULT_PASSES;
    int64_t info[4] = {0, 0, 0, 0};
    auto done = [&](int64_t na) {
        if (info4) std::copy(info, info + 4, info4);
        return na;
    };
    if (n == 0) {
        agg_of.clear();
        return done(0);
    }
    DevBuf<double> deg(n);
    DevBuf<unsigned long long> tcnt(n + 1);
    DevBuf<int64_t> trp(n + 1);
    DevBuf<int32_t> tcol(std::max<int64_t>(1, G.nnz)), state(n), owner(n);
    DevBuf<unsigned int> und(MIS_CHECK_EVERY);
    hipLaunchKernelGGL(k_mis_deg, dim3(grid256(n)), dim3(256), 0, s, G.rp64.get(), G.val.get(), n, deg.get());
    FAMG_CHECK_HIP(hipMemsetAsync(tcnt.get(), 0, (n + 1) * sizeof(unsigned long long), s));
    if (G.nnz) hipLaunchKernelGGL(k_mis_tcount, dim3(grid256(G.nnz)), dim3(256), 0, s, G.col.get(), G.nnz, tcnt.get());
    FAMG_CHECK_HIP(hipGetLastError());
    const int64_t tnnz = scan_counts(reinterpret_cast<const int64_t *>(tcnt.get()), trp.get(), n, ctx);
    FAMG_REQUIRE(tnnz == G.nnz, AMG_ERR_INVALID, "aggregation: transposed pattern count mismatch");
    FAMG_CHECK_HIP(hipMemcpyAsync(tcnt.get(), trp.get(), n * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_mis_tfill, dim3(grid256(n)), dim3(256), 0, s, G.rp64.get(), G.col.get(), n, tcnt.get(),
                       tcol.get());
    FAMG_CHECK_HIP(hipMemsetAsync(state.get(), 0, n * sizeof(int32_t), s));
    FAMG_CHECK_HIP(hipGetLastError());
    // phase 1: bounded passes; the host looks at the undecided count every MIS_CHECK_EVERY
    int64_t passes = 0, prev = n;
    bool decided = false;
    while (!decided && passes < budget) {
        const int group = (int)std::min<int64_t>(MIS_CHECK_EVERY, budget - passes);
        unsigned int h[MIS_CHECK_EVERY] = {0, 0, 0, 0};
        FAMG_CHECK_HIP(hipMemsetAsync(und.get(), 0, MIS_CHECK_EVERY * sizeof(unsigned int), s));
        for (int p = 0; p < group; p++)
            hipLaunchKernelGGL(k_mis_pass, dim3(grid256(n)), dim3(256), 0, s, trp.get(), tcol.get(), deg.get(), n,
                               state.get(), und.get() + p);
        FAMG_CHECK_HIP(hipGetLastError());
        FAMG_CHECK_HIP(hipMemcpyAsync(h, und.get(), sizeof(h), hipMemcpyDeviceToHost, s));
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
        for (int p = 0; p < group && !decided; p++) {
            passes++;
            decided = h[p] == 0;
        }
        if (!decided) {
            // the undecided node that precedes all others decides in every pass
            FAMG_REQUIRE((int64_t)h[group - 1] < prev, AMG_ERR_INVALID, "aggregation: the undecided count stopped falling");
            prev = h[group - 1];
        }
    }
    info[0] = passes;
    if (!decided) {  // past the budget (a chain-like graph): the host sweep on the downloaded graph
        StrengthGraph H;
        H.n = n;
        H.rp.resize(n + 1);
        H.col.resize(G.nnz);
        H.w.resize(G.nnz);
        FAMG_CHECK_HIP(hipMemcpyAsync(H.rp.data(), G.rp64.get(), (n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        if (G.nnz) {
            FAMG_CHECK_HIP(hipMemcpyAsync(H.col.data(), G.col.get(), G.nnz * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            FAMG_CHECK_HIP(hipMemcpyAsync(H.w.data(), G.val.get(), G.nnz * sizeof(double), hipMemcpyDeviceToHost, s));
        }
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
        info[3] = 1;
        const int64_t na = aggregate_mis(H, agg_of, info + 1);
        return done(na);
    }
    hipLaunchKernelGGL(k_mis_owner, dim3(grid256(n)), dim3(256), 0, s, trp.get(), tcol.get(), deg.get(), n, state.get(),
                       owner.get());
    FAMG_CHECK_HIP(hipGetLastError());
    std::vector<int32_t> ho(n);
    FAMG_CHECK_HIP(hipMemcpyAsync(ho.data(), owner.get(), n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    // phase 2 on the host: labels are the root nodes; only the singleton roots' rows come over
    std::vector<int64_t> agg(n), size0(n, 0), singles;
    for (int64_t v = 0; v < n; v++) {
        FAMG_REQUIRE(ho[v] >= 0 && ho[v] < n, AMG_ERR_INVALID, "aggregation: a node without an owner");
        agg[v] = ho[v];
        size0[ho[v]]++;
    }
    for (int64_t v = 0; v < n; v++) {
        if (ho[v] != v) continue;
        info[1]++;
        if (size0[v] == 1) singles.push_back(v);
    }
    info[2] = (int64_t)singles.size();
    const int64_t ms = (int64_t)singles.size();
    std::vector<int64_t> off(ms + 1, 0);
    std::vector<int32_t> scol;
    std::vector<double> sw;
    if (ms) {
        std::vector<int32_t> rows(singles.begin(), singles.end());
        DevBuf<int32_t> drows(ms);
        DevBuf<int64_t> dlen(ms), doff(ms + 1);
        FAMG_CHECK_HIP(hipMemcpyAsync(drows.get(), rows.data(), ms * sizeof(int32_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_mis_rowlen, dim3(grid256(ms)), dim3(256), 0, s, G.rp64.get(), drows.get(), ms, dlen.get());
        FAMG_CHECK_HIP(hipGetLastError());
        const int64_t tot = scan_counts(dlen.get(), doff.get(), ms, ctx);
        DevBuf<int32_t> dcol(std::max<int64_t>(1, tot));
        DevBuf<double> dval(std::max<int64_t>(1, tot));
        hipLaunchKernelGGL(k_mis_rowcopy, dim3(grid256(ms)), dim3(256), 0, s, G.rp64.get(), G.col.get(), G.val.get(),
                           drows.get(), ms, doff.get(), dcol.get(), dval.get());
        FAMG_CHECK_HIP(hipGetLastError());
        scol.resize(tot);
        sw.resize(tot);
        FAMG_CHECK_HIP(hipMemcpyAsync(off.data(), doff.get(), (ms + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        if (tot) {
            FAMG_CHECK_HIP(hipMemcpyAsync(scol.data(), dcol.get(), tot * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            FAMG_CHECK_HIP(hipMemcpyAsync(sw.data(), dval.get(), tot * sizeof(double), hipMemcpyDeviceToHost, s));
        }
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
    }
    return done(aggregate_finish(n, agg, size0, singles, off.data(), off.data() + 1, scol.data(), sw.data(), agg_of));
}

}  // namespace famg

// ------------------------------------------------------------------ C ABI

using namespace famg;

namespace {
CsrPtr need_csr_sg(const amg_linop *h) {
    FAMG_REQUIRE(h && h->op, AMG_ERR_INVALID, "null amg_linop handle");
    auto p = std::dynamic_pointer_cast<CsrOp>(h->op);
    FAMG_REQUIRE(p, AMG_ERR_INVALID, "operator is not a CSR matrix");
    return p;
}
}  // namespace

extern "C" {

amg_status amg_set_sa_setup(int32_t where) {
    return guard([&] {
        FAMG_REQUIRE(where == 0 || where == 1, AMG_ERR_INVALID, "sa setup policy must be 0 (host) or 1 (device)");
        g_sa_setup = where;
    });
}

amg_status amg_get_sa_setup(int32_t *where) {
    return guard([&] {
        FAMG_REQUIRE(where, AMG_ERR_INVALID, "null output");
        *where = g_sa_setup;
    });
}

amg_status amg_strength_graph_device(const amg_linop *A, const double *near_null, int64_t ld, int64_t k,
                                     const double *weights, int64_t block_size, amg_mem mem, amg_linop **graph) {
    return amg_strength_graph_device_depth(A, near_null, ld, k, weights, 1, block_size, mem, 0, graph, nullptr);
}

amg_status amg_strength_graph_device_depth(const amg_linop *A, const double *near_null, int64_t ld, int64_t k,
                                           const double *weights, int64_t depth, int64_t block_size, amg_mem mem,
                                           int64_t max_bytes, amg_linop **graph, int64_t *info6) {
    return guard([&] {
        FAMG_REQUIRE(graph, AMG_ERR_INVALID, "null output");
        FAMG_REQUIRE(depth >= 1, AMG_ERR_INVALID, "strength graph: depth must be >= 1");
        FAMG_REQUIRE(max_bytes >= 0, AMG_ERR_INVALID, "strength graph: negative byte budget");
        auto a = need_csr_sg(A);
        FAMG_REQUIRE(near_null && weights, AMG_ERR_INVALID, "null argument");
        FAMG_REQUIRE(mem == AMG_MEM_DEVICE || mem == AMG_MEM_HOST, AMG_ERR_INVALID, "bad amg_mem");
        FAMG_REQUIRE(k >= 1 && ld >= a->nrows, AMG_ERR_INVALID, "strength graph: bad near-null block");
        a->ctx->set_device();
        hipStream_t s = a->ctx->stream;
        const int64_t n = a->nrows;
        DevBuf<double> stage;
        const double *nn = near_null;
        int64_t ldd = ld;
        if (mem == AMG_MEM_HOST) {
            stage.resize(std::max<int64_t>(1, n * k));
            if (n)
                FAMG_CHECK_HIP(hipMemcpy2DAsync(stage.get(), n * sizeof(double), near_null, ld * sizeof(double),
                                                n * sizeof(double), k, hipMemcpyHostToDevice, s));
            nn = stage.get();
            ldd = n;
        }
        SgDeviceInfo inf;
        CsrPtr G = strength_graph_device(*a, nn, ldd, k, weights, block_size, depth, max_bytes, &inf, true);
        if (info6) {
            const int64_t v[6] = {inf.longest_ball, inf.wave_rows, inf.block_rows,
                                  inf.ball_entries, inf.dof_entries, inf.node_edges};
            std::copy(v, v + 6, info6);
        }
        if (!G) fail(AMG_ERR_UNSUPPORTED, sg_reason_text(inf.reason));
        *graph = new amg_linop{G};
    });
}

amg_status amg_pattern_ball_device(const amg_linop *A, int64_t depth, amg_linop **ball) {
    return guard([&] {
        FAMG_REQUIRE(ball, AMG_ERR_INVALID, "null output");
        FAMG_REQUIRE(depth >= 1, AMG_ERR_INVALID, "pattern ball: depth must be >= 1");
        auto a = need_csr_sg(A);
        FAMG_REQUIRE(a->nrows == a->ncols, AMG_ERR_DIM, "pattern ball: matrix must be square");
        a->ctx->set_device();
        hipStream_t s = a->ctx->stream;
        BallPattern b;
        const int reason = ball_pattern_device(a->m, depth, false, 0, b);
        FAMG_REQUIRE(reason != SG_REASON_BALL_CAP, AMG_ERR_UNSUPPORTED,
                     "pattern ball: a ball has more than 4096 members");
        FAMG_REQUIRE(reason == SG_REASON_NONE, AMG_ERR_UNSUPPORTED, "pattern ball: 2^31 or more entries");
        const int64_t n = a->nrows;
        auto B = make_csr(a->ctx);
        csr_alloc(B->m, a->ctx, n, n, b.entries);
        B->m.rp64 = std::move(b.rp);
        B->nrows = B->ncols = n;
        if (b.entries) {
            FAMG_CHECK_HIP(hipMemcpyAsync(B->m.col.get(), b.col.get(), b.entries * sizeof(int32_t),
                                          hipMemcpyDeviceToDevice, s));
            hipLaunchKernelGGL(k_ball_ones, dim3(grid256(b.entries)), dim3(256), 0, s, B->m.val.get(), b.entries);
            FAMG_CHECK_HIP(hipGetLastError());
        }
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
        *ball = new amg_linop{B};
    });
}

amg_status amg_aggregate_mis_device(const amg_linop *graph, int64_t max_passes, int64_t *agg_of, int64_t *naggs,
                                    int64_t *info4) {
    return guard([&] {
        FAMG_REQUIRE(agg_of && naggs, AMG_ERR_INVALID, "null output");
        auto g = need_csr_sg(graph);
        g->ctx->set_device();
        std::vector<int64_t> agg;
        *naggs = aggregate_mis_device(g->m, max_passes, agg, info4);
        std::copy(agg.begin(), agg.end(), agg_of);
    });
}

}  // extern "C"
