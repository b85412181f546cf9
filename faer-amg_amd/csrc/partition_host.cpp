// partition_host.cpp -- the modularity partitioner on the host: target-size aggregates
// of a node-level strength graph by pairwise matching rounds and swap
// improvement.  DESIGN.md 17.  The device path (partition.hip) shares the edge
// order, the weights and the serial swap selection declared in famg.hpp, and
// falls back to the functions here.
//
// Restated from the reference (paths relative to its root):
//  * Partitioner::new without a starting partition, unit node weights
//                         (partitioners/modularity.rs:28-134)
//  * initialize_partition, greedy_matching, generate_modularity_triplets,
//    pairwise_merge_rowsums (:179-206, :293-383)
//  * AdjacencyList::pairwise_merge / merge_pair, Partition::pairwise_merge
//                         (partitioners/mod.rs:109-126, :439-462, :508-578)
//  * size_cost, delta_q, improve_partition (modularity.rs:385-510)
// The orders the reference leaves to unstable sorts and HashSet iteration are
// pinned: edges by (weight descending, splitmix64 of the pair, i, j); merged
// vertices numbered by ascending smallest member; a merged row sums equal new
// ids in member-then-stored order; the best destination of a swap ties to the
// smaller aggregate id, proposals tie to the smaller node.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "handles.hpp"

namespace famg {

int g_sa_partitioner = 0;
PartitionerConfig g_sa_part_cfg;

double mod_inverse_total(const std::vector<double> &rs) {
    double total = 0.0;
    for (double r : rs) total += r;
    FAMG_REQUIRE(std::isfinite(total) && total > 0.0, AMG_ERR_INVALID,
                 "modularity partitioner: the strengths sum to zero or are not finite");
    return 1.0 / total;
}

namespace {

struct ModEdge {
    double w;
    int32_t i, j;
};

// Merge the matched pairs of S (mate[v] = the partner or -1): new ids by
// ascending smallest member, rows summed in the pinned order.
void mod_contract(ModState &S, const std::vector<int64_t> &mate) {
    const int64_t nv = S.nv;
    std::vector<int32_t> newid(nv);
    int64_t q = 0;
    for (int64_t v = 0; v < nv; v++) newid[v] = (mate[v] < 0 || v < mate[v]) ? (int32_t)q++ : newid[mate[v]];
    ModState N;
    N.nv = q;
    N.rp.assign(q + 1, 0);
    N.rs.resize(q);
    N.size.resize(q);
    N.col.reserve(S.col.size());
    N.w.reserve(S.w.size());
    std::vector<std::pair<int32_t, double>> tmp;
    for (int64_t v = 0; v < nv; v++) {
        if (!(mate[v] < 0 || v < mate[v])) continue;
        const int64_t a = v, b = mate[v], id = newid[v];
        tmp.clear();
        for (int64_t m : {a, b}) {
            if (m < 0) continue;
            for (int64_t e = S.rp[m]; e < S.rp[m + 1]; e++) tmp.emplace_back(newid[S.col[e]], S.w[e]);
        }
        std::stable_sort(tmp.begin(), tmp.end(),
                         [](const std::pair<int32_t, double> &x, const std::pair<int32_t, double> &y) {
                             return x.first < y.first;
                         });
        for (size_t t = 0; t < tmp.size();) {
            double sum = tmp[t].second;
            size_t u = t + 1;
            for (; u < tmp.size() && tmp[u].first == tmp[t].first; u++) sum += tmp[u].second;
            N.col.push_back(tmp[t].first);
            N.w.push_back(sum);
            t = u;
        }
        N.rp[id + 1] = (int64_t)N.col.size();
        N.rs[id] = b < 0 ? S.rs[a] : S.rs[a] + S.rs[b];
        N.size[id] = b < 0 ? S.size[a] : S.size[a] + S.size[b];
    }
    N.node_to_v.resize(S.node_to_v.size());
    for (size_t f = 0; f < S.node_to_v.size(); f++) N.node_to_v[f] = newid[S.node_to_v[f]];
    S = std::move(N);
}

}  // namespace

void mod_rounds_host(ModState &S, const PartitionerConfig &cfg, double inv_total, int64_t *info8) {
    const int64_t n = (int64_t)S.node_to_v.size();
    std::vector<ModEdge> ed;
    while (S.nv > 0 && (double)n / (double)S.nv < cfg.cf) {
        ed.clear();
        for (int64_t i = 0; i < S.nv; i++)
            for (int64_t e = S.rp[i]; e < S.rp[i + 1]; e++) {
                const int64_t j = S.col[e];
                if (j >= i) continue;
                ed.push_back({mod_edge_weight(S.w[e], inv_total, S.rs[i], S.rs[j], S.size[i], S.size[j], cfg.cf, cfg.pen),
                              (int32_t)i, (int32_t)j});
            }
        if (ed.empty()) break;  // "no more matches are possible"
        std::sort(ed.begin(), ed.end(),
                  [](const ModEdge &a, const ModEdge &b) { return mod_precedes(a.w, a.i, a.j, b.w, b.i, b.j); });
        const int64_t target = (int64_t)std::ceil((double)S.nv - (double)n / cfg.cf) + 1;
        std::vector<int64_t> mate(S.nv, -1);
        int64_t pairs = 0;
        for (const ModEdge &e : ed) {
            if (mate[e.i] >= 0 || mate[e.j] >= 0) continue;
            mate[e.i] = e.j;
            mate[e.j] = e.i;
            if (++pairs > target) break;
        }
        info8[0]++;
        mod_contract(S, mate);
    }
}

int64_t mod_select_swaps(std::vector<ModProposal> &props, const int64_t *rp, const int32_t *col,
                         std::vector<int64_t> &agg, std::vector<int64_t> &size, std::vector<int64_t> *moved) {
    std::sort(props.begin(), props.end(), [](const ModProposal &a, const ModProposal &b) {
        return a.dq > b.dq || (a.dq == b.dq && a.node < b.node);
    });
    std::vector<char> alive_nodes(agg.size(), 1), alive_aggs(size.size(), 1);
    int64_t swaps = 0;
    for (const ModProposal &p : props) {
        const int64_t v = p.node, to = p.agg, from = agg[v];
        if (!(alive_nodes[v] && alive_aggs[to] && alive_aggs[from])) continue;
        agg[v] = to;
        size[from]--;
        size[to]++;
        swaps++;
        if (moved) moved->push_back(v);
        alive_aggs[to] = alive_aggs[from] = 0;
        alive_nodes[v] = 0;
        for (int64_t e = rp[v]; e < rp[v + 1]; e++) {
            alive_nodes[col[e]] = 0;
            alive_aggs[agg[col[e]]] = 0;
        }
    }
    return swaps;
}

void mod_improve_host(const StrengthGraph &G, const PartitionerConfig &cfg, std::vector<int64_t> &agg,
                      std::vector<int64_t> &size, int64_t *info8) {
    std::vector<ModProposal> props;
    std::vector<std::pair<int64_t, double>> outs;
    for (int64_t pass = 0; pass < cfg.max_improve; pass++) {
        props.clear();
        for (int64_t i = 0; i < G.n; i++) {
            const int64_t src = agg[i];
            if (size[src] <= 1) continue;  // the only member stays: the aggregate count is kept
            double in = 0.0;
            outs.clear();
            for (int64_t e = G.rp[i]; e < G.rp[i + 1]; e++) {
                const int64_t a = agg[G.col[e]];
                if (a == src) {
                    in += G.w[e];
                    continue;
                }
                size_t t = 0;
                while (t < outs.size() && outs[t].first != a) t++;
                if (t == outs.size()) outs.emplace_back(a, 0.0);
                outs[t].second += G.w[e];
            }
            int64_t best = -1;
            double bdq = 0.0;
            for (const auto &o : outs) {
                const double dq = mod_delta_q(in, o.second, size[o.first], size[src], cfg.cf, cfg.pen);
                if (!(dq > 0.0)) continue;
                if (best < 0 || dq > bdq || (dq == bdq && o.first < best)) {
                    best = o.first;
                    bdq = dq;
                }
            }
            if (best >= 0) props.push_back({(int32_t)i, (int32_t)best, bdq});
        }
        if (props.empty()) break;
        info8[4]++;
        info8[5] += mod_select_swaps(props, G.rp.data(), G.col.data(), agg, size, nullptr);
    }
}

int64_t mod_renumber(std::vector<int64_t> &agg, int64_t na, int64_t *info8) {
    std::vector<int64_t> ren(na, -1), cnt;
    int64_t q = 0;
    for (int64_t &a : agg) {
        if (ren[a] < 0) {
            ren[a] = q++;
            cnt.push_back(0);
        }
        a = ren[a];
        cnt[a]++;
    }
    info8[6] = cnt.empty() ? 0 : *std::min_element(cnt.begin(), cnt.end());
    info8[7] = cnt.empty() ? 0 : *std::max_element(cnt.begin(), cnt.end());
    return q;
}

int64_t partition_modularity(const StrengthGraph &G, const PartitionerConfig &cfg, std::vector<int64_t> &agg_of,
                             int64_t *info8) {
    int64_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t n = G.n;
    ModState S;
    S.nv = n;
    S.rp = G.rp;
    S.col = G.col;
    S.w = G.w;
    S.rs.assign(n, 0.0);
    for (int64_t i = 0; i < n; i++) {
        double s = 0.0;
        for (int64_t e = G.rp[i]; e < G.rp[i + 1]; e++) s += G.w[e];
        FAMG_REQUIRE(std::isfinite(s), AMG_ERR_INVALID, "modularity partitioner: a strength is not finite");
        S.rs[i] = s < 0.0 ? 0.0 : s;
    }
    const double inv_total = mod_inverse_total(S.rs);
    S.size.assign(n, 1);
    S.node_to_v.resize(n);
    for (int64_t i = 0; i < n; i++) S.node_to_v[i] = i;
    mod_rounds_host(S, cfg, inv_total, info);
    agg_of = std::move(S.node_to_v);
    mod_improve_host(G, cfg, agg_of, S.size, info);
    const int64_t na = mod_renumber(agg_of, S.nv, info);
    if (info8) std::copy(info, info + 8, info8);
    return na;
}

PartitionerConfig mod_config_from(const amg_partitioner_config *cfg) {
    FAMG_REQUIRE(cfg, AMG_ERR_INVALID, "null partitioner config");
    FAMG_REQUIRE(cfg->coarsening_factor >= 1.0 && std::isfinite(cfg->coarsening_factor), AMG_ERR_INVALID,
                 "partitioner config: coarsening_factor must be >= 1");
    FAMG_REQUIRE(cfg->agg_size_penalty >= 0.0 && std::isfinite(cfg->agg_size_penalty), AMG_ERR_INVALID,
                 "partitioner config: agg_size_penalty must be >= 0");
    FAMG_REQUIRE(cfg->max_improvement_iters >= 0 && cfg->max_passes >= 0, AMG_ERR_INVALID,
                 "partitioner config: negative iteration or pass budget");
    PartitionerConfig c;
    c.cf = cfg->coarsening_factor;
    c.pen = cfg->agg_size_penalty;
    c.max_improve = cfg->max_improvement_iters;
    c.max_passes = cfg->max_passes;
    return c;
}

}  // namespace famg

// ------------------------------------------------------------------ C ABI

using namespace famg;

extern "C" {

amg_status amg_partitioner_config_default(amg_partitioner_config *cfg) {
    return guard([&] {
        FAMG_REQUIRE(cfg, AMG_ERR_INVALID, "null config");
        cfg->coarsening_factor = 8.0;  // PartitionerConfig::default (partitioners/mod.rs:249-329)
        cfg->agg_size_penalty = 1.0;
        cfg->max_improvement_iters = 100;
        cfg->max_passes = 0;
    });
}

amg_status amg_partition_modularity(const amg_host_csr *graph, const amg_partitioner_config *cfg, int64_t *agg_of,
                                    int64_t *naggs, int64_t *info8) {
    return guard([&] {
        FAMG_REQUIRE(agg_of && naggs, AMG_ERR_INVALID, "null output");
        FAMG_REQUIRE(graph, AMG_ERR_INVALID, "null graph");
        const PartitionerConfig c = mod_config_from(cfg);
        FAMG_REQUIRE(graph->nrows == graph->ncols, AMG_ERR_INVALID, "graph must be square");
        StrengthGraph G;
        G.n = graph->nrows;
        G.rp = graph->rp;
        G.col.resize(graph->ci.size());
        for (int64_t i = 0; i < G.n; i++)
            for (int64_t e = G.rp[i]; e < G.rp[i + 1]; e++) {
                const int64_t j = graph->ci[e];
                FAMG_REQUIRE(j >= 0 && j < G.n && j != i && (e == G.rp[i] || graph->ci[e - 1] < j), AMG_ERR_INVALID,
                             "graph rows need ascending columns in range and no self loops");
                G.col[e] = (int32_t)j;
            }
        G.w = graph->va;
        std::vector<int64_t> agg;
        *naggs = partition_modularity(G, c, agg, info8);
        std::copy(agg.begin(), agg.end(), agg_of);
    });
}

amg_status amg_set_sa_partitioner(int32_t kind, const amg_partitioner_config *cfg) {
    return guard([&] {
        FAMG_REQUIRE(kind == 0 || kind == 1, AMG_ERR_INVALID, "sa partitioner must be 0 (MIS) or 1 (modularity)");
        const PartitionerConfig c = cfg ? mod_config_from(cfg) : PartitionerConfig{};
        g_sa_partitioner = kind;
        g_sa_part_cfg = c;
    });
}

amg_status amg_get_sa_partitioner(int32_t *kind, amg_partitioner_config *cfg) {
    return guard([&] {
        FAMG_REQUIRE(kind, AMG_ERR_INVALID, "null output");
        *kind = g_sa_partitioner;
        if (cfg) {
            cfg->coarsening_factor = g_sa_part_cfg.cf;
            cfg->agg_size_penalty = g_sa_part_cfg.pen;
            cfg->max_improvement_iters = g_sa_part_cfg.max_improve;
            cfg->max_passes = g_sa_part_cfg.max_passes;
        }
    });
}

}  // extern "C"
