// classical.hip -- classical coarsening: the compatible-relaxation C/F split and
// the hierarchy build.  DESIGN.md 18.
//
// Restated from the reference (paths relative to its root):
//  * least_squares, the CR loop        (interpolation/mod.rs:574-652)
//  * Hierarchy::coarsen                (hierarchy.rs:190-248) for
//    InterpolationConfig::Classical    (interpolation/mod.rs:56-60, :158-214)
// The relaxations run on the device with what the library has (the SpMV of A_f,
// the BlockSmoother apply, the dot product); the relabelling runs on the host on
// the downloaded vector.  One strength graph at search_depth serves the MIS and
// the CR smoother's modularity partition (the reference builds a second one at
// depth 3 inside PartitionerConfig::build, partitioners/mod.rs:289-292: the same
// graph at its default search_depth = 3).  Guards the reference does not have
// (it loops forever or divides by zero): a round whose MIS adds no C-point
// stops the loop, so does max_iters, and a relaxed vector of zeros counts as
// reduction 0.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "classical.hpp"
#include "handles.hpp"

namespace famg {

int64_t cr_split(const CsrPtr &A, const StrengthGraph &G, const CrConfig &cfg, int8_t *point_type, int32_t *c_round,
                 CrInfo &info) {
    const int64_t n = A->nrows;
    FAMG_REQUIRE(A->nrows == A->ncols, AMG_ERR_DIM, "cr_split: matrix must be square");
    FAMG_REQUIRE(G.n == n, AMG_ERR_DIM, "cr_split: the graph must have one node per row");
    FAMG_REQUIRE(cfg.relax_steps >= 1 && cfg.max_iters >= 1 && cfg.smoother_cf >= 1.0, AMG_ERR_INVALID,
                 "cr_split: need relax_steps >= 1, max_cr_iters >= 1, smoother_coarsening_factor >= 1");
    Ctx *ctx = A->ctx;
    hipStream_t s = ctx->stream;
    info = CrInfo{};
    std::fill(point_type, point_type + n, (int8_t)0);
    std::vector<int32_t> made(n, -1);  // the round that made a node a C-point
    if (c_round) std::fill(c_round, c_round + n, -1);
    if (n == 0) {
        info.stop = CR_NO_NEW_C;
        return 0;
    }
    // the CR smoother's partition: modularity at smoother_coarsening_factor (:158-214)
    PartitionerConfig pc;
    pc.cf = cfg.smoother_cf;
    std::vector<int64_t> part;
    const int64_t nparts = partition_modularity(G, pc, part, nullptr);
    // A on the host: A_f keeps its pattern, the values change per round
    std::vector<int64_t> rp(n + 1), col(std::max<int64_t>(1, A->m.nnz)), grp(G.rp), gci(G.col.begin(), G.col.end());
    std::vector<double> val(std::max<int64_t>(1, A->m.nnz)), vf(val.size());
    csr_to_host(A->m, rp.data(), col.data(), val.data());
    std::vector<uint8_t> cand(n);
    std::vector<double> u(n);
    DevBuf<double> du(n), dt(n), dz(n);
    int64_t nc = 0;
    info.stop = CR_MAX_ITERS;
    for (int64_t round = 0; round < cfg.max_iters; round++) {
        for (int64_t i = 0; i < n; i++) cand[i] = point_type[i] == 0;
        const std::vector<int64_t> fresh = cr_mis(n, grp.data(), gci.data(), G.w.data(), cand.data());
        if (fresh.empty()) {  // guard: the reference would relax the same A_f for ever
            info.stop = CR_NO_NEW_C;
            break;
        }
        for (int64_t c : fresh) {
            point_type[c] = 1;
            made[c] = (int32_t)round;
        }
        nc += (int64_t)fresh.size();
        info.rounds = round + 1;
        info.c_per_round.push_back(nc);
        if (nc == n) {  // nothing left to relax: u_0f = 0
            info.reduction = 0.0;
            info.stop = CR_ZERO_VECTOR;
            break;
        }
        // A_f = I_f A I_f with the C diagonals at 1 (:595-608); u_0f = I_f 1
        for (int64_t i = 0; i < n; i++) {
            const bool ci = point_type[i] == 1;
            u[i] = ci ? 0.0 : 1.0;
            for (int64_t e = rp[i]; e < rp[i + 1]; e++) {
                const bool cj = point_type[col[e]] == 1;
                vf[e] = (ci || cj) ? (col[e] == i ? 1.0 : 0.0) : val[e];
            }
        }
        auto Af = make_csr(ctx);
        csr_from_host(Af->m, ctx, n, n, rp.data(), col.data(), vf.data());
        Af->nrows = Af->ncols = n;
        auto Mf = make_block_smoother(*Af, part.data(), nparts, 1);
        FAMG_CHECK_HIP(hipMemcpyAsync(du.get(), u.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
        const double start = std::sqrt(vec_dot(du.get(), du.get(), n, *ctx));
        for (int64_t st = 0; st < cfg.relax_steps; st++) {  // ErrorPropogator: u <- u - M (A_f u)
            Af->apply(dt.get(), du.get());
            Mf->apply(dz.get(), dt.get());
            vec_axpy(du.get(), -1.0, dz.get(), n, s);
        }
        const double end = std::sqrt(vec_dot(du.get(), du.get(), n, *ctx));
        FAMG_CHECK_HIP(hipMemcpyAsync(u.data(), du.get(), n * sizeof(double), hipMemcpyDeviceToHost, s));
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
        double inf_norm = 0.0;
        for (int64_t i = 0; i < n; i++) inf_norm = std::max(inf_norm, std::fabs(u[i]));
        FAMG_REQUIRE(std::isfinite(end) && std::isfinite(inf_norm), AMG_ERR_INVALID,
                     "cr_split: the relaxed vector is not finite");
        if (inf_norm == 0.0) {  // guard: sigma_i would be 0 / 0
            info.reduction = 0.0;
            info.stop = CR_ZERO_VECTOR;
            break;
        }
        info.reduction = std::pow(end / start, 1.0 / (double)cfg.relax_steps);  // :627
        const double tol = 1.0 - info.reduction;
        for (int64_t i = 0; i < n; i++) {  // :636-645
            const double sigma = std::fabs(u[i]) / inf_norm;
            if (sigma > tol) point_type[i] = 0;
            else if (point_type[i] == 0) point_type[i] = 2;
        }
        // guard: a C-point relaxes to exactly 0 (its row of A_f is the unit row), so
        // sigma = 0 <= tol unless the reduction is above 1, where the reference would
        // relabel it F and pick it again: a C-point stays a C-point
        for (int64_t i = 0; i < n; i++)
            if (made[i] >= 0) point_type[i] = 1;
        if (!(info.reduction > cfg.target)) {
            info.stop = CR_CONVERGED;
            break;
        }
    }
    if (c_round) std::copy(made.begin(), made.end(), c_round);
    return nc;
}

namespace {
struct StageClock {
    bool on;
    hipStream_t s;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double lap() {
        if (on) FAMG_CHECK_HIP(hipStreamSynchronize(s));
        const auto t1 = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return ms;
    }
};
}  // namespace

std::shared_ptr<MultigridOp> classical_build(const CsrPtr &A, const double *nn_in, int64_t ld, int64_t k,
                                             const double *weights_in, const ClassicalConfig &cfg,
                                             std::vector<ClassicalLevelInfo> *info) {
    FAMG_REQUIRE(A->nrows == A->ncols, AMG_ERR_DIM, "classical_build: matrix must be square");
    FAMG_REQUIRE(k >= 1 && ld >= A->nrows, AMG_ERR_INVALID,
                 "classical_build: need k >= 1 and a near-null leading dimension >= n");
    FAMG_REQUIRE(cfg.max_interp >= 1 && cfg.search_depth >= 1 && cfg.depth_ls >= 0, AMG_ERR_INVALID,
                 "classical_build: need max_interp >= 1, search_depth >= 1, depth_ls >= 0");
    FAMG_REQUIRE(cfg.max_interp <= 4, AMG_ERR_UNSUPPORTED, "classical_build: max_interp above 4");
    FAMG_REQUIRE(cfg.smoother == 0 || cfg.smoother == 1 || cfg.smoother == 2 || cfg.smoother == 4, AMG_ERR_UNSUPPORTED,
                 "classical_build: smoother must be 0 Jacobi, 1 L1, 2 SGS or 4 Chebyshev (no aggregates for 3)");
    FAMG_REQUIRE(cfg.where == 0 || cfg.where == 1, AMG_ERR_INVALID, "classical_build: where must be 0 or 1");
    Ctx *ctx = A->ctx;
    const int64_t max_levels = cfg.max_levels <= 0 ? INT64_MAX : cfg.max_levels;
    const std::vector<double> w =
        weights_in ? std::vector<double>(weights_in, weights_in + k) : default_weights(*A, nn_in, ld, k);
    std::vector<CsrPtr> As{A}, Rs, Ps;
    int64_t cur_ld = A->nrows;
    std::vector<double> nn(A->nrows * k);
    for (int64_t c = 0; c < k; c++) std::memcpy(nn.data() + c * cur_ld, nn_in + c * ld, A->nrows * sizeof(double));
    int64_t level = 1, coarse_dim = -1;
    static const bool log_on = env_is_one("FAMG_SA_LOG");
    StageClock clk{log_on, ctx->stream};
    while ((coarse_dim < 0 || coarse_dim > cfg.coarsest_dim) && level < max_levels) {
        CsrPtr cur = As.back();
        const int64_t n = cur->nrows;
        clk.lap();
        StrengthGraph G = strength_graph(*cur, nn.data(), cur_ld, k, w.data(), cfg.search_depth, 1);
        const double ms_graph = clk.lap();
        std::vector<int8_t> pt(n);
        std::vector<int32_t> cround(n);
        CrInfo cr;
        const int64_t nc = cr_split(cur, G, cfg.cr, pt.data(), cround.data(), cr);
        const double ms_cr = clk.lap();
        if (nc >= n || nc == 0) break;  // the level does not shrink: stop here
        std::vector<double> cnn(nc * k);
        LsStageInfo st;
        CsrPtr P = ls_interpolation(*cur, pt.data(), nn.data(), cur_ld, k, w.data(), cfg.depth_ls + cfg.search_depth,
                                    cfg.max_interp, cfg.tau, cfg.where, cnn.data(), nullptr, &st);
        clk.lap();
        CsrPtr R = transpose_op(*P);
        CsrPtr Ac = galerkin_rap(*R, *cur, *P);
        const double ms_rap = clk.lap();
        nn_postprocess(*Ac, 3, cnn.data(), nc, k);  // hierarchy.rs:219-228
        const double ms_nn = clk.lap();
        if (log_on)
            fprintf(stderr,
                    "famg classical level %lld: n %lld coarse %lld edges %lld cr rounds %lld reduction %.4f stop %d "
                    "longest list %lld subsets %lld device rows %lld host rows %lld empty rows %lld "
                    "ms: graph %.3f cr %.3f candidates %.3f search %.3f assemble %.3f rap %.3f nearnull %.3f\n",
                    (long long)(level - 1), (long long)n, (long long)nc, (long long)G.rp.back(), (long long)cr.rounds,
                    cr.reduction, cr.stop, (long long)st.longest, (long long)st.subsets, (long long)st.device_rows,
                    (long long)st.host_rows, (long long)st.empty_rows, ms_graph, ms_cr, st.ms_candidates, st.ms_search,
                    st.ms_build, ms_rap, ms_nn);
        if (info) info->push_back({n, nc, cr.rounds, st.longest, st.device_rows, st.host_rows, st.empty_rows});
        Rs.push_back(R);
        Ps.push_back(P);
        As.push_back(Ac);
        nn.swap(cnn);
        cur_ld = nc;
        coarse_dim = Ac->nrows;
        level++;
    }
    auto make_smoother = [&](const CsrPtr &M) -> LinOpPtr {
        switch (cfg.smoother) {
        case 0: return make_jacobi(*M, cfg.omega);
        case 1: return make_l1(*M);
        case 2: {
            std::vector<int32_t> colors;
            const int64_t ncol = greedy_coloring(M->m, colors);
            if (ncol <= SGS_MAX_COLORS) return make_sgs(M, colors.data(), false);
            return make_l1(*M);
        }
        default: {
            ChebyConfig cc;
            if (cfg.chebyshev_steps > 0) cc.steps = cfg.chebyshev_steps;
            return make_chebyshev(M, cc);
        }
        }
    };
    auto mg = std::make_shared<MultigridOp>();
    mg->ctx = ctx;
    mg->nrows = mg->ncols = A->nrows;
    MgLevel L0;
    L0.A = A;
    L0.S = As.size() == 1 ? LinOpPtr(make_coarse_chol(*A)) : make_smoother(A);
    mg->levels.push_back(std::move(L0));
    for (size_t l = 1; l < As.size(); l++) {
        LinOpPtr S = (l + 1 == As.size()) ? LinOpPtr(make_coarse_chol(*As[l])) : make_smoother(As[l]);
        mg->add_level(As[l], S, Rs[l - 1], Ps[l - 1]);
    }
    return mg;
}

}  // namespace famg

// ------------------------------------------------------------------ C ABI

using namespace famg;

namespace {
CrConfig cr_config_from(const amg_classical_config *cfg) {
    CrConfig c;
    c.target = cfg->target_convergence;
    c.smoother_cf = cfg->smoother_coarsening_factor;
    c.relax_steps = cfg->relax_steps;
    c.max_iters = cfg->max_cr_iters;
    FAMG_REQUIRE(std::isfinite(c.target) && std::isfinite(c.smoother_cf), AMG_ERR_INVALID,
                 "classical config: target_convergence and smoother_coarsening_factor must be finite");
    return c;
}
}  // namespace

extern "C" {

amg_status amg_cr_split(amg_linop *A, const amg_host_csr *graph, const amg_classical_config *cfg, int8_t *point_type,
                        int32_t *c_round, int64_t *n_coarse, double *info) {
    return guard([&] {
        auto a = need_csr_handle(A);
        FAMG_REQUIRE(graph && cfg && point_type && n_coarse, AMG_ERR_INVALID, "null argument");
        FAMG_REQUIRE(graph->nrows == graph->ncols && graph->nrows == a->nrows, AMG_ERR_DIM,
                     "cr_split: the graph must be square with one node per row");
        const CrConfig c = cr_config_from(cfg);
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
        a->ctx->set_device();
        CrInfo ci;
        std::vector<int32_t> cround(G.n);
        *n_coarse = cr_split(a, G, c, point_type, cround.data(), ci);
        if (c_round) std::copy(cround.begin(), cround.end(), c_round);
        if (info) {
            info[0] = (double)ci.rounds;
            info[1] = ci.reduction;
            info[2] = (double)ci.stop;
            for (int64_t r = 0; r < cfg->max_cr_iters; r++)
                info[3 + r] = r < (int64_t)ci.c_per_round.size() ? (double)ci.c_per_round[r] : 0.0;
        }
    });
}

amg_status amg_classical_build(amg_linop *A, const double *near_null, int64_t ld, int64_t k, const double *weights,
                               const amg_classical_config *cfg, amg_linop **mg_out, int64_t *level_info) {
    return guard([&] {
        auto a = need_csr_handle(A);
        FAMG_REQUIRE(near_null && cfg && mg_out, AMG_ERR_INVALID, "null argument");
        ClassicalConfig c;
        c.search_depth = cfg->search_depth;
        c.depth_ls = cfg->depth_ls;
        c.max_interp = cfg->max_interp;
        c.tau = cfg->tau_threshold;
        c.cr = cr_config_from(cfg);
        c.coarsest_dim = cfg->coarsest_dim;
        c.max_levels = cfg->max_levels;
        c.omega = cfg->omega;
        c.smoother = cfg->smoother;
        FAMG_REQUIRE(cfg->chebyshev_steps >= 0, AMG_ERR_INVALID, "classical config: negative chebyshev_steps");
        c.chebyshev_steps = cfg->chebyshev_steps;
        c.where = cfg->where;
        a->ctx->set_device();
        std::vector<ClassicalLevelInfo> li;
        *mg_out = new amg_linop{classical_build(a, near_null, ld, k, weights, c, &li)};
        if (level_info) {
            const int64_t shown = std::min<int64_t>((int64_t)li.size(), AMG_CLASSICAL_INFO_LEVELS);
            level_info[0] = (int64_t)li.size();
            for (int64_t l = 0; l < shown; l++) {
                const int64_t v[7] = {li[l].n, li[l].coarse, li[l].cr_rounds, li[l].longest, li[l].device_rows,
                                      li[l].host_rows, li[l].empty_rows};
                std::copy(v, v + 7, level_info + 1 + 7 * l);
            }
        }
    });
}

}  // extern "C"
