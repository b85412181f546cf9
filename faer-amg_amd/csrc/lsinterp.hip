// lsinterp.hip -- the least-squares interpolation search of classical coarsening
// on gfx950, and the level build around it.
//
// ls_interp_weights (interpolation/mod.rs:433-510) enumerates, for one fine row,
// every subset of up to max_interp of its L candidate C-points and solves a
// constrained r x r least-squares problem for each: C(L, r) dense tiny solves,
// independent over rows and subsets.  One wave takes one row:
//  * the candidates' near-null rows, the row's own and the weights are staged
//    in LDS; g = V Q vf^T is computed once; lists of at most LS_DEV_GRAM_LIST
//    candidates also keep the upper triangle of the Gram matrix V Q V^T there,
//    longer ones recompute an entry from the staged rows -- the same ascending
//    sum, so the same bits;
//  * the C(L, r) subsets in lexicographic order are cut into 64 contiguous rank
//    ranges, one per lane; a lane unranks its first subset, then advances;
//  * every lane runs ls_pinned.hpp's solver (the host's) and keeps its first
//    strict minimum; a butterfly over (err, rank) gives the serial loop's first
//    strict minimum, and the lane that owns it stores the row's result with plain
//    vector stores.  No atomics, no floating-point reduction.
// Rows are sorted by list length and launched in bins, so the waves of a launch
// do alike work and its LDS is sized by the bin's longest list.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <numeric>

#include "classical.hpp"
#include "handles.hpp"
#include "ls_pinned.hpp"

namespace famg {

namespace {

struct LsDev {
    const int32_t *rows;  // the launch's rows
    int64_t nrows;
    const int64_t *lrp;
    const int32_t *lci;
    const double *nn;  // n x k column-major, ld n
    const double *d;
    int64_t n;
    int k, mi, lmax, gram;  // lmax: the longest list of the launch; gram: the Gram matrix is kept in LDS
    int per_wave;           // doubles of LDS per wave
    int32_t *count;
    int64_t *cols;
    double *w, *err;
};

template <int R>
__device__ __forceinline__ void ls_wave_size(const LsDev &p, int64_t row, int L, const int32_t *cand, const double *vc,
                                             const double *g, const double *gram, const double *dl, double btb,
                                             int lane) {
    if (L < R) return;
    const int64_t total = ls_choose(L, R);
    const int64_t chunk = (total + 63) / 64;
    const int64_t r0 = (int64_t)lane * chunk, r1 = r0 + chunk < total ? r0 + chunk : total;
    int idx[R], bidx[R];
    double bp[R], berr = 0.0;
    int64_t brank = INT64_MAX;
#pragma unroll
    for (int t = 0; t < R; t++) {
        idx[t] = t;
        bidx[t] = 0;
        bp[t] = 0.0;
    }
    if (r0 < r1) ls_unrank<R>(r0, L, idx);
    for (int64_t rank = r0; rank < r1; rank++) {
        double G[R][R], gs[R], q[R], err;
#pragma unroll
        for (int a = 0; a < R; a++) {
            gs[a] = g[idx[a]];
#pragma unroll
            for (int b = a; b < R; b++) {
                G[a][b] = p.gram ? gram[idx[a] * L + idx[b]]
                                 : ls_gram_entry(vc + idx[a] * p.k, 1, vc + idx[b] * p.k, 1, dl, p.k);
                G[b][a] = G[a][b];
            }
        }
        if (ls_subset_qp<R>(G, gs, btb, q, err) && (brank == INT64_MAX || err < berr)) {
            brank = rank;
            berr = err;
#pragma unroll
            for (int t = 0; t < R; t++) {
                bidx[t] = idx[t];
                bp[t] = q[t];
            }
        }
        if (rank + 1 < r1) ls_next<R>(L, idx);
    }
    // the first strict minimum of the serial loop: the smallest (err, rank)
    double werr = berr;
    int64_t wrank = brank;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double oe = __shfl_xor(werr, off);
        const int64_t orank = __shfl_xor(wrank, off);
        const bool take = orank != INT64_MAX && (wrank == INT64_MAX || oe < werr || (oe == werr && orank < wrank));
        if (take) {
            werr = oe;
            wrank = orank;
        }
    }
    if (brank != INT64_MAX && brank == wrank) {
        const int64_t slot = row * p.mi + (R - 1);
        p.count[slot] = R;
        p.err[slot] = berr;
#pragma unroll
        for (int t = 0; t < R; t++) {
            p.cols[slot * p.mi + t] = cand[bidx[t]];
            p.w[slot * p.mi + t] = bp[t];
        }
    }
}

// blockDim.x = 64 * waves; wave v of block b takes rows[b * waves + v]
__global__ __launch_bounds__(256) void k_ls_search(const LsDev p) {
    extern __shared__ double ls_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * waves + wave;
    const bool active = q < p.nrows;
    const int64_t row = active ? p.rows[q] : 0;
    const int64_t l0 = active ? p.lrp[row] : 0;
    int L = active ? (int)(p.lrp[row + 1] - l0) : 0;
    if (L > p.lmax) L = 0;  // never: the host bins rows by length
    const int32_t *cand = p.lci + l0;
    // LDS of this wave: dl[k], vf[k], g[lmax], then the Gram matrix or the staged rows
    double *dl = ls_smem + (size_t)wave * p.per_wave;
    double *vf = dl + p.k, *g = vf + p.k, *big = g + p.lmax;
    for (int c = lane; c < p.k; c += 64) {
        dl[c] = p.d[c];
        vf[c] = active ? p.nn[row + (int64_t)c * p.n] : 0.0;
    }
    if (!p.gram)
        for (int e = lane; e < L * p.k; e += 64) {
            const int l = e / p.k, c = e - l * p.k;
            big[e] = p.nn[cand[l] + (int64_t)c * p.n];
        }
    // the LDS written above and below belongs to this wave alone: a wave-level barrier would
    // do; __syncthreads is used because every wave of the block reaches both of them
    __syncthreads();
    for (int l = lane; l < L; l += 64) {
        g[l] = p.gram ? ls_gram_entry(p.nn + cand[l], p.n, vf, 1, dl, p.k) : ls_gram_entry(big + l * p.k, 1, vf, 1, dl, p.k);
    }
    if (p.gram)
        for (int e = lane; e < L * L; e += 64) {
            const int a = e / L, b = e - a * L;
            if (a <= b) big[e] = ls_gram_entry(p.nn + cand[a], p.n, p.nn + cand[b], p.n, dl, p.k);
        }
    __syncthreads();
    if (L == 0) return;
    const double btb = ls_gram_entry(vf, 1, vf, 1, dl, p.k);
    ls_wave_size<1>(p, row, L, cand, big, g, big, dl, btb, lane);
    if (p.mi >= 2) ls_wave_size<2>(p, row, L, cand, big, g, big, dl, btb, lane);
    if (p.mi >= 3) ls_wave_size<3>(p, row, L, cand, big, g, big, dl, btb, lane);
    if (p.mi >= 4) ls_wave_size<4>(p, row, L, cand, big, g, big, dl, btb, lane);
}

template <typename T> void upload(DevBuf<T> &buf, const T *src, size_t count, hipStream_t s) {
    buf.resize(std::max<size_t>(1, count));
    if (count) FAMG_CHECK_HIP(hipMemcpyAsync(buf.get(), src, count * sizeof(T), hipMemcpyHostToDevice, s));
}

}  // namespace

void ls_search_device(Ctx *ctx, int64_t n, const int64_t *lrp, const int64_t *lci, const double *nn, int64_t ld,
                      int64_t k, const double *d, int64_t max_list, const LsOut &out, int64_t *info4) {
    hipStream_t s = ctx->stream;
    const int64_t mi = out.mi, nl = lrp[n];
    FAMG_REQUIRE(max_list >= 1 && max_list <= LS_DEV_MAX_LIST && k <= LS_DEV_MAX_K, AMG_ERR_INVALID,
                 "ls_search_device: list cap or k out of range");
    // rows by list length (ties: by index); empty rows keep the initial "none"
    std::vector<int32_t> dev_rows;
    std::vector<int64_t> host_rows;
    int64_t subsets = 0;
    for (int64_t i = 0; i < n; i++) {
        const int64_t L = lrp[i + 1] - lrp[i];
        if (L == 0) continue;
        if (L <= max_list) {
            dev_rows.push_back((int32_t)i);
            for (int r = 1; r <= mi; r++) subsets += ls_choose(L, r);
        } else {
            host_rows.push_back(i);
        }
    }
    std::stable_sort(dev_rows.begin(), dev_rows.end(),
                     [&](int32_t a, int32_t b) { return lrp[a + 1] - lrp[a] < lrp[b + 1] - lrp[b]; });
    std::vector<int32_t> lci32(nl);
    for (int64_t e = 0; e < nl; e++) lci32[e] = (int32_t)lci[e];
    std::vector<double> nnp((size_t)n * k);
    for (int64_t c = 0; c < k; c++) std::copy(nn + c * ld, nn + c * ld + n, nnp.begin() + c * n);
    DevBuf<int32_t> d_rows, d_lci, d_count;
    DevBuf<int64_t> d_lrp, d_cols;
    DevBuf<double> d_nn, d_d, d_w, d_err;
    upload(d_rows, dev_rows.data(), dev_rows.size(), s);
    upload(d_lci, lci32.data(), lci32.size(), s);
    upload(d_lrp, lrp, (size_t)n + 1, s);
    upload(d_nn, nnp.data(), nnp.size(), s);
    upload(d_d, d, (size_t)k, s);
    const size_t slots = std::max<size_t>(1, (size_t)n * mi);
    d_count.resize(slots);
    d_err.resize(slots);
    d_cols.resize(slots * mi);
    d_w.resize(slots * mi);
    FAMG_CHECK_HIP(hipMemsetAsync(d_count.get(), 0, d_count.bytes(), s));
    FAMG_CHECK_HIP(hipMemsetAsync(d_err.get(), 0, d_err.bytes(), s));
    FAMG_CHECK_HIP(hipMemsetAsync(d_w.get(), 0, d_w.bytes(), s));
    FAMG_CHECK_HIP(hipMemsetAsync(d_cols.get(), 0xFF, d_cols.bytes(), s));  // -1
    // one launch per bin of list lengths: its LDS and its waves' work are sized by the bin
    const int64_t bins[] = {4, 8, 16, 32, LS_DEV_GRAM_LIST, 128, LS_DEV_MAX_LIST};
    size_t begin = 0;
    for (int64_t top : bins) {
        size_t end = begin;
        while (end < dev_rows.size() && lrp[dev_rows[end] + 1] - lrp[dev_rows[end]] <= top) end++;
        if (end == begin) continue;
        LsDev p;
        p.rows = d_rows.get() + begin;
        p.nrows = (int64_t)(end - begin);
        p.lrp = d_lrp.get();
        p.lci = d_lci.get();
        p.nn = d_nn.get();
        p.d = d_d.get();
        p.n = n;
        p.k = (int)k;
        p.mi = (int)mi;
        p.lmax = (int)(lrp[dev_rows[end - 1] + 1] - lrp[dev_rows[end - 1]]);
        p.gram = top <= LS_DEV_GRAM_LIST ? 1 : 0;
        p.per_wave = 2 * p.k + p.lmax + (p.gram ? p.lmax * p.lmax : p.lmax * p.k);
        p.count = d_count.get();
        p.cols = d_cols.get();
        p.w = d_w.get();
        p.err = d_err.get();
        const size_t wave_bytes = (size_t)p.per_wave * sizeof(double);  // <= 35 KiB
        const int waves = (int)std::max<size_t>(1, std::min<size_t>(4, 65536 / wave_bytes));
        hipLaunchKernelGGL(k_ls_search, dim3((unsigned)ceil_div(p.nrows, waves)), dim3(64 * waves),
                           wave_bytes * waves, s, p);
        FAMG_CHECK_HIP(hipGetLastError());
        begin = end;
    }
    FAMG_CHECK_HIP(hipMemcpyAsync(out.count, d_count.get(), (size_t)n * mi * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipMemcpyAsync(out.err, d_err.get(), (size_t)n * mi * sizeof(double), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipMemcpyAsync(out.cols, d_cols.get(), (size_t)n * mi * mi * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipMemcpyAsync(out.w, d_w.get(), (size_t)n * mi * mi * sizeof(double), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    // lists beyond the cap: the host function, the same result
    if (!host_rows.empty())
        subsets += ls_search_host(host_rows.data(), (int64_t)host_rows.size(), lrp, lci, nn, ld, k, d, out);
    if (info4) {
        info4[0] = (int64_t)dev_rows.size();
        info4[1] = (int64_t)host_rows.size();
        info4[3] = subsets;
    }
}

static void candidates_of(const CsrOp &A, const int8_t *point_type, int64_t depth, std::vector<int64_t> &lrp,
                          std::vector<int64_t> &lci) {
    const GpuCsr &m = A.m;
    std::vector<int64_t> rp(m.nrows + 1);
    std::vector<int32_t> col(std::max<int64_t>(1, m.nnz));
    hipStream_t s = m.ctx->stream;
    FAMG_CHECK_HIP(hipMemcpyAsync(rp.data(), m.rp64.get(), (m.nrows + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (m.nnz)
        FAMG_CHECK_HIP(hipMemcpyAsync(col.data(), m.col.get(), m.nnz * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    ls_candidates_host(m.nrows, rp.data(), col.data(), point_type, depth, lrp, lci);
}

CsrPtr ls_interpolation(CsrOp &A, const int8_t *point_type, const double *near_null, int64_t ld, int64_t k,
                        const double *weights, int64_t depth, int64_t mi, double tau, int where, double *coarse_nn,
                        double *row_err, LsStageInfo *stage) {
    const int64_t n = A.nrows;
    FAMG_REQUIRE(A.nrows == A.ncols, AMG_ERR_DIM, "ls_interpolation: matrix must be square");
    FAMG_REQUIRE(mi >= 1 && k >= 1 && ld >= n && depth >= 0, AMG_ERR_INVALID,
                 "ls_interpolation: need max_interp >= 1, k >= 1, a leading dimension >= n, depths >= 0");
    FAMG_REQUIRE(mi <= LS_MAX_INTERP, AMG_ERR_UNSUPPORTED, "ls_interpolation: max_interp above 4");
    FAMG_REQUIRE(where == 0 || (where == 1 && k <= LS_DEV_MAX_K), AMG_ERR_UNSUPPORTED,
                 "ls_interpolation: where must be 0, or 1 with k <= 16");
    for (int64_t c = 0; c < k; c++) {
        FAMG_REQUIRE(std::isfinite(weights[c]), AMG_ERR_INVALID, "ls_interpolation: a weight is not finite");
        for (int64_t i = 0; i < n; i++)
            FAMG_REQUIRE(std::isfinite(near_null[i + c * ld]), AMG_ERR_INVALID,
                         "ls_interpolation: a near-null entry is not finite");
    }
    Ctx *ctx = A.ctx;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int64_t> cidx(n, -1);
    int64_t nc = 0;
    for (int64_t i = 0; i < n; i++)
        if (point_type[i] == 1) cidx[i] = nc++;
    std::vector<int64_t> lrp, lci;
    candidates_of(A, point_type, depth, lrp, lci);
    for (int64_t i = 0; i < n; i++)
        FAMG_REQUIRE(lrp[i + 1] - lrp[i] < 32768, AMG_ERR_UNSUPPORTED,
                     "ls_interpolation: a list of 32768 candidates or more");
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<int32_t> count(n * mi), chosen(n);
    std::vector<int64_t> cols(n * mi * mi);
    std::vector<double> w(n * mi * mi), err(n * mi), rerr(n);
    const LsOut out{mi, count.data(), cols.data(), w.data(), err.data()};
    int64_t info[4] = {0, 0, 0, 0};
    for (int64_t i = 0; i < n; i++) info[1] += lrp[i + 1] > lrp[i];  // the host search: every row with a candidate
    if (where == 1)
        ls_search_device(ctx, n, lrp.data(), lci.data(), near_null, ld, k, weights, LS_DEV_MAX_LIST, out, info);
    else
        info[3] = ls_search_host(nullptr, n, lrp.data(), lci.data(), near_null, ld, k, weights, out);
    const auto t2 = std::chrono::steady_clock::now();
    ls_accept(n, near_null, ld, k, weights, mi, tau, count.data(), err.data(), chosen.data(), rerr.data());
    std::vector<int64_t> prp(n + 1, 0), pci;
    std::vector<double> pva;
    int64_t empty_rows = 0;
    for (int64_t i = 0; i < n; i++) {
        if (point_type[i] == 1) {
            pci.push_back(cidx[i]);
            pva.push_back(1.0);
            rerr[i] = 0.0;
            for (int64_t c = 0; c < k; c++) coarse_nn[cidx[i] + c * nc] = near_null[i + c * ld];
        } else if (chosen[i] > 0) {
            const int64_t slot = i * mi + chosen[i] - 1;
            for (int64_t t = 0; t < chosen[i]; t++) {
                pci.push_back(cidx[cols[slot * mi + t]]);
                pva.push_back(w[slot * mi + t]);
            }
        } else {
            empty_rows++;
        }
        prp[i + 1] = (int64_t)pci.size();
    }
    if (row_err) std::copy(rerr.begin(), rerr.end(), row_err);
    pci.push_back(0);  // never empty arrays
    pva.push_back(0.0);
    auto Pm = make_csr(ctx);
    csr_from_host(Pm->m, ctx, n, nc, prp.data(), pci.data(), pva.data());
    Pm->nrows = n;
    Pm->ncols = nc;
    if (stage) {
        const auto t3 = std::chrono::steady_clock::now();
        stage->ms_candidates = std::chrono::duration<double, std::milli>(t1 - t0).count();
        stage->ms_search = std::chrono::duration<double, std::milli>(t2 - t1).count();
        stage->ms_build = std::chrono::duration<double, std::milli>(t3 - t2).count();
        stage->device_rows = info[0];
        stage->host_rows = info[1];
        stage->subsets = info[3];
        stage->empty_rows = empty_rows;
        int64_t longest = 0;
        for (int64_t i = 0; i < n; i++) longest = std::max(longest, lrp[i + 1] - lrp[i]);
        stage->longest = longest;
    }
    return Pm;
}

}  // namespace famg

// ------------------------------------------------------------------ C ABI

using namespace famg;

extern "C" {

amg_status amg_ls_candidates(const amg_linop *A, const int8_t *point_type, int64_t depth, amg_host_csr **lists) {
    return guard([&] {
        auto a = need_csr_handle(A);
        FAMG_REQUIRE(point_type && lists, AMG_ERR_INVALID, "null argument");
        FAMG_REQUIRE(depth >= 0, AMG_ERR_INVALID, "ls_candidates: negative depth");
        FAMG_REQUIRE(a->nrows == a->ncols, AMG_ERR_DIM, "ls_candidates: matrix must be square");
        a->ctx->set_device();
        auto h = std::make_unique<amg_host_csr>();
        h->nrows = h->ncols = a->nrows;
        candidates_of(*a, point_type, depth, h->rp, h->ci);
        h->va.assign(h->ci.size(), 1.0);
        *lists = h.release();
    });
}

amg_status amg_ls_interpolation(amg_linop *A, const int8_t *point_type, const double *near_null, int64_t ld,
                                int64_t k, const double *weights, const amg_classical_config *cfg, amg_linop **P,
                                double *coarse_nn, double *row_err, int64_t *info5) {
    return guard([&] {
        auto a = need_csr_handle(A);
        FAMG_REQUIRE(point_type && near_null && weights && cfg && P && coarse_nn, AMG_ERR_INVALID, "null argument");
        FAMG_REQUIRE(cfg->depth_ls >= 0 && cfg->search_depth >= 0, AMG_ERR_INVALID, "ls_interpolation: negative depth");
        a->ctx->set_device();
        LsStageInfo st;
        *P = new amg_linop{ls_interpolation(*a, point_type, near_null, ld, k, weights, cfg->depth_ls + cfg->search_depth,
                                            cfg->max_interp, cfg->tau_threshold, cfg->where, coarse_nn, row_err, &st)};
        if (info5) {
            info5[0] = st.device_rows;
            info5[1] = st.host_rows;
            info5[2] = st.longest;
            info5[3] = st.subsets;
            info5[4] = st.empty_rows;
        }
    });
}

}  // extern "C"
