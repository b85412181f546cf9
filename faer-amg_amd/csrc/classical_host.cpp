// classical_host.cpp -- classical coarsening on the host: the C-point MIS with a
// candidate mask, the candidate lists, the least-squares search and its
// acceptance rule.  DESIGN.md 18.  The search's arithmetic is ls_pinned.hpp's,
// shared with the kernel (lsinterp.hip), which falls back to the function here
// for long lists.
//
// Restated from the reference (paths relative to its root):
//  * AdjacencyList::maximal_independent_set  (partitioners/mod.rs:395-423)
//  * extract_local_subgraph                  (partitioners/mod.rs:695-718)
//  * ls_interp_weights                       (interpolation/mod.rs:433-510)
//  * constrained_subset_qp and its helpers   (:312-356, :387-431; ls_pinned.hpp)
// The unstable sort of the MIS is pinned: descending degree, ties to the smaller
// index.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

#include "classical.hpp"
#include "handles.hpp"
#include "ls_pinned.hpp"

namespace famg {

std::vector<int64_t> cr_mis(int64_t n, const int64_t *rp, const int64_t *ci, const double *va,
                            const uint8_t *candidates) {
    std::vector<uint8_t> f(candidates, candidates + n);
    std::vector<std::pair<double, int64_t>> deg;
    for (int64_t i = 0; i < n; i++) {
        if (!f[i]) continue;
        double s = 0.0;
        for (int64_t e = rp[i]; e < rp[i + 1]; e++)
            if (f[ci[e]]) s += va[e];
        FAMG_REQUIRE(!std::isnan(s), AMG_ERR_INVALID, "cr_mis: a strength degree is NaN");  // "bad float" (:411)
        deg.emplace_back(s, i);
    }
    std::sort(deg.begin(), deg.end(), [](const std::pair<double, int64_t> &a, const std::pair<double, int64_t> &b) {
        return a.first > b.first || (a.first == b.first && a.second < b.second);
    });
    std::vector<int64_t> chosen;
    for (const auto &d : deg) {
        const int64_t i = d.second;
        if (!f[i]) continue;
        f[i] = 0;
        chosen.push_back(i);
        for (int64_t e = rp[i]; e < rp[i + 1]; e++) f[ci[e]] = 0;
    }
    return chosen;
}

void ls_candidates_host(int64_t n, const int64_t *rp, const int32_t *col, const int8_t *point_type, int64_t depth,
                        std::vector<int64_t> &lrp, std::vector<int64_t> &lci) {
    std::vector<std::vector<int64_t>> rows(n);
#pragma omp parallel
    {
        std::vector<int64_t> stamp(n, -1), queue;
#pragma omp for schedule(dynamic, 64)
        for (int64_t i = 0; i < n; i++) {
            if (point_type[i] == 1) continue;
            queue.clear();
            queue.push_back(i);
            stamp[i] = i;
            size_t head = 0, level_end = 1;
            for (int64_t dep = 0; dep < depth && head < queue.size(); dep++) {
                for (; head < level_end; head++) {
                    const int64_t j = queue[head];
                    for (int64_t e = rp[j]; e < rp[j + 1]; e++) {
                        const int64_t c = col[e];
                        if (stamp[c] != i) {
                            stamp[c] = i;
                            queue.push_back(c);
                        }
                    }
                }
                level_end = queue.size();
            }
            std::vector<int64_t> &r = rows[i];
            for (int64_t j : queue)
                if (point_type[j] == 1) r.push_back(j);
            std::sort(r.begin(), r.end());
        }
    }
    lrp.assign(n + 1, 0);
    for (int64_t i = 0; i < n; i++) lrp[i + 1] = lrp[i] + (int64_t)rows[i].size();
    lci.resize(lrp[n]);
    for (int64_t i = 0; i < n; i++) std::copy(rows[i].begin(), rows[i].end(), lci.begin() + lrp[i]);
}

namespace {

// the best subset of size R of one row: combinations(R) in lexicographic order,
// the first strictly smaller error wins (interpolation/mod.rs:463-490)
template <int R>
int64_t search_size(int64_t L, const double *vc, const double *g, double btb, const double *d, int k, int64_t row,
                    const int64_t *cand, const LsOut &out) {
    const int64_t slot = row * out.mi + (R - 1);
    out.count[slot] = 0;
    out.err[slot] = 0.0;
    for (int64_t t = 0; t < out.mi; t++) {
        out.cols[slot * out.mi + t] = -1;
        out.w[slot * out.mi + t] = 0.0;
    }
    if (L < R || out.mi < R) return 0;
    const int64_t total = ls_choose(L, R);
    int idx[R], bidx[R];
    for (int t = 0; t < R; t++) idx[t] = t;
    double berr = 0.0, bp[R];
    bool have = false;
    for (int64_t rank = 0; rank < total; rank++) {
        double G[R][R], gs[R], p[R], err;
        for (int a = 0; a < R; a++) {
            gs[a] = g[idx[a]];
            for (int b = a; b < R; b++) {
                G[a][b] = ls_gram_entry(vc + (int64_t)idx[a] * k, 1, vc + (int64_t)idx[b] * k, 1, d, k);
                G[b][a] = G[a][b];
            }
        }
        if (ls_subset_qp<R>(G, gs, btb, p, err) && (!have || err < berr)) {
            have = true;
            berr = err;
            for (int t = 0; t < R; t++) {
                bidx[t] = idx[t];
                bp[t] = p[t];
            }
        }
        if (rank + 1 < total) ls_next<R>((int)L, idx);
    }
    if (have) {
        out.count[slot] = R;
        out.err[slot] = berr;
        for (int t = 0; t < R; t++) {
            out.cols[slot * out.mi + t] = cand[bidx[t]];
            out.w[slot * out.mi + t] = bp[t];
        }
    }
    return total;
}

}  // namespace

int64_t ls_search_row_host(int64_t row, int64_t L, const int64_t *cand, const double *nn, int64_t ld, int64_t k,
                           const double *d, const LsOut &out) {
    std::vector<double> vc(std::max<int64_t>(1, L * k)), g(std::max<int64_t>(1, L));
    for (int64_t l = 0; l < L; l++)
        for (int64_t c = 0; c < k; c++) vc[l * k + c] = nn[cand[l] + c * ld];
    const double *vf = nn + row;
    for (int64_t l = 0; l < L; l++) g[l] = ls_gram_entry(vc.data() + l * k, 1, vf, ld, d, (int)k);
    const double btb = ls_gram_entry(vf, ld, vf, ld, d, (int)k);
    int64_t subsets = 0;
    subsets += search_size<1>(L, vc.data(), g.data(), btb, d, (int)k, row, cand, out);
    if (out.mi >= 2) subsets += search_size<2>(L, vc.data(), g.data(), btb, d, (int)k, row, cand, out);
    if (out.mi >= 3) subsets += search_size<3>(L, vc.data(), g.data(), btb, d, (int)k, row, cand, out);
    if (out.mi >= 4) subsets += search_size<4>(L, vc.data(), g.data(), btb, d, (int)k, row, cand, out);
    return subsets;
}

int64_t ls_search_host(const int64_t *rows, int64_t nrows, const int64_t *lrp, const int64_t *lci, const double *nn,
                       int64_t ld, int64_t k, const double *d, const LsOut &out) {
    int64_t subsets = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : subsets)
    for (int64_t q = 0; q < nrows; q++) {
        const int64_t i = rows ? rows[q] : q;
        subsets += ls_search_row_host(i, lrp[i + 1] - lrp[i], lci + lrp[i], nn, ld, k, d, out);
    }
    return subsets;
}

void ls_accept(int64_t n, const double *nn, int64_t ld, int64_t k, const double *d, int64_t mi, double tau,
               const int32_t *count, const double *err, int32_t *chosen, double *row_err) {
    for (int64_t i = 0; i < n; i++) {
        double acc_err = ls_gram_entry(nn + i, ld, nn + i, ld, d, (int)k);  // LsInterpResult::empty(btb)
        int64_t acc_size = 0;
        for (int64_t r = 1; r <= mi; r++) {
            if (count[i * mi + r - 1] == 0) continue;  // "continue to next size" (:493)
            const double e = err[i * mi + r - 1];
            const double dr = (double)(r - acc_size);
            if (e < std::pow(acc_err, tau * dr)) {  // :496-506; NaN for a negative accepted error: false
                acc_err = e;
                acc_size = r;
            }
        }
        chosen[i] = (int32_t)acc_size;
        if (row_err) row_err[i] = acc_err;
    }
}

}  // namespace famg

// ------------------------------------------------------------------ C ABI

using namespace famg;

extern "C" {

amg_status amg_classical_config_default(amg_classical_config *cfg) {
    return guard([&] {
        FAMG_REQUIRE(cfg, AMG_ERR_INVALID, "null config");
        std::memset(cfg, 0, sizeof(*cfg));
        cfg->search_depth = 1;   // LeastSquaresConfig::default has 3 (interpolation/mod.rs); DESIGN.md 18
        cfg->depth_ls = 2;
        cfg->max_interp = 3;
        cfg->tau_threshold = 1.2;
        cfg->target_convergence = 0.3;  // CompatibleRelaxationConfig::default
        cfg->relax_steps = 5;
        cfg->smoother_coarsening_factor = 256.0;
        cfg->max_cr_iters = 20;
        cfg->coarsest_dim = 1000;  // HierarchyConfig::default (hierarchy.rs:28-35)
        cfg->max_levels = 0;
        cfg->omega = 0.66;
        cfg->smoother = 1;
        cfg->chebyshev_steps = 0;
        cfg->where = 1;  // the device search: 104x the 16-thread host search at depth 3
    });
}

amg_status amg_cr_mis(const amg_host_csr *graph, const uint8_t *candidates, int64_t *c_points, int64_t *n_new) {
    return guard([&] {
        FAMG_REQUIRE(graph && candidates && c_points && n_new, AMG_ERR_INVALID, "null argument");
        FAMG_REQUIRE(graph->nrows == graph->ncols, AMG_ERR_DIM, "graph must be square");
        const int64_t n = graph->nrows;
        for (int64_t c : graph->ci) FAMG_REQUIRE(c >= 0 && c < n, AMG_ERR_INVALID, "graph column out of range");
        const std::vector<int64_t> c = cr_mis(n, graph->rp.data(), graph->ci.data(), graph->va.data(), candidates);
        std::copy(c.begin(), c.end(), c_points);
        *n_new = (int64_t)c.size();
    });
}

amg_status amg_ls_search(amg_ctx *ctx, const amg_host_csr *lists, const double *near_null, int64_t ld, int64_t k,
                         const double *weights, int64_t max_interp, int32_t where, int64_t max_list, int32_t *count,
                         int64_t *cols, double *w, double *err, int64_t *info4) {
    return guard([&] {
        FAMG_REQUIRE(lists && near_null && weights && count && cols && w && err, AMG_ERR_INVALID, "null argument");
        FAMG_REQUIRE(max_interp >= 1, AMG_ERR_INVALID, "ls_search: max_interp must be >= 1");
        FAMG_REQUIRE(max_interp <= LS_MAX_INTERP, AMG_ERR_UNSUPPORTED, "ls_search: max_interp above 4");
        FAMG_REQUIRE(where == 0 || where == 1, AMG_ERR_INVALID, "ls_search: where must be 0 (host) or 1 (device)");
        const int64_t n = lists->nrows;
        FAMG_REQUIRE(k >= 1 && ld >= n && max_list >= 0, AMG_ERR_INVALID,
                     "ls_search: need k >= 1, a leading dimension >= n and max_list >= 0");
        FAMG_REQUIRE(lists->ncols == n, AMG_ERR_DIM, "ls_search: the lists must have n rows and n columns");
        FAMG_REQUIRE(n < (int64_t(1) << 31), AMG_ERR_UNSUPPORTED, "ls_search: n >= 2^31");
        int64_t longest = 0;
        for (int64_t i = 0; i < n; i++) {
            for (int64_t e = lists->rp[i]; e < lists->rp[i + 1]; e++)
                FAMG_REQUIRE(lists->ci[e] >= 0 && lists->ci[e] < n && (e == lists->rp[i] || lists->ci[e - 1] < lists->ci[e]),
                             AMG_ERR_INVALID, "ls_search: a list is not ascending and in range");
            longest = std::max(longest, lists->rp[i + 1] - lists->rp[i]);
        }
        FAMG_REQUIRE(longest < 32768, AMG_ERR_UNSUPPORTED, "ls_search: a list of 32768 candidates or more");
        for (int64_t c = 0; c < k; c++) {
            FAMG_REQUIRE(std::isfinite(weights[c]), AMG_ERR_INVALID, "ls_search: a weight is not finite");
            for (int64_t i = 0; i < n; i++)
                FAMG_REQUIRE(std::isfinite(near_null[i + c * ld]), AMG_ERR_INVALID,
                             "ls_search: a near-null entry is not finite");
        }
        const LsOut out{max_interp, count, cols, w, err};
        int64_t info[4] = {0, n, longest, 0};
        if (where == 0) {
            info[3] = ls_search_host(nullptr, n, lists->rp.data(), lists->ci.data(), near_null, ld, k, weights, out);
        } else {
            FAMG_REQUIRE(ctx, AMG_ERR_INVALID, "ls_search: the device search needs a context");
            FAMG_REQUIRE(k <= LS_DEV_MAX_K, AMG_ERR_UNSUPPORTED, "ls_search: the device search takes k <= 16");
            Ctx *c = reinterpret_cast<Ctx *>(ctx);
            c->set_device();
            ls_search_device(c, n, lists->rp.data(), lists->ci.data(), near_null, ld, k, weights,
                             max_list == 0 ? LS_DEV_MAX_LIST : std::min(max_list, LS_DEV_MAX_LIST), out, info);
            info[2] = longest;
        }
        if (info4) std::copy(info, info + 4, info4);
    });
}

amg_status amg_ls_accept(int64_t n, const double *near_null, int64_t ld, int64_t k, const double *weights,
                         int64_t max_interp, double tau, const int32_t *count, const double *err, int32_t *chosen) {
    return guard([&] {
        FAMG_REQUIRE(near_null && weights && count && err && chosen, AMG_ERR_INVALID, "null argument");
        FAMG_REQUIRE(n >= 0 && k >= 1 && ld >= n && max_interp >= 1, AMG_ERR_INVALID,
                     "ls_accept: need n >= 0, k >= 1, a leading dimension >= n and max_interp >= 1");
        ls_accept(n, near_null, ld, k, weights, max_interp, tau, count, err, chosen, nullptr);
    });
}

}  // extern "C"
