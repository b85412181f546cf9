// classical.hpp -- classical coarsening: what the host pieces
// (classical_host.cpp) and the device search (lsinterp.hip) share.
#pragma once

#include "famg.hpp"

namespace famg {

constexpr int64_t LS_DEV_MAX_LIST = 256;  // the longest candidate list the kernel takes
constexpr int64_t LS_DEV_MAX_K = 16;      // near-null columns the kernel stages
constexpr int64_t LS_DEV_GRAM_LIST = 64;  // lists up to here keep their Gram matrix in LDS (32 KiB)

// amg_ls_search's output arrays (slot s = row * mi + r - 1)
struct LsOut {
    int64_t mi;
    int32_t *count;
    int64_t *cols;
    double *w, *err;
};

// maximal_independent_set with a mask (partitioners/mod.rs:395-423); the chosen nodes in order
std::vector<int64_t> cr_mis(int64_t n, const int64_t *rp, const int64_t *ci, const double *va,
                            const uint8_t *candidates);
// the C-points of the BFS ball of every non-C row, ascending (:695-718)
void ls_candidates_host(int64_t n, const int64_t *rp, const int32_t *col, const int8_t *point_type, int64_t depth,
                        std::vector<int64_t> &lrp, std::vector<int64_t> &lci);
// one row of the search on the host; returns the subsets enumerated
int64_t ls_search_row_host(int64_t row, int64_t L, const int64_t *cand, const double *nn, int64_t ld, int64_t k,
                           const double *d, const LsOut &out);
// rows[0..nrows) of the search on the host (OpenMP); returns the subsets enumerated
int64_t ls_search_host(const int64_t *rows, int64_t nrows, const int64_t *lrp, const int64_t *lci, const double *nn,
                       int64_t ld, int64_t k, const double *d, const LsOut &out);
// the rows with lists of at most max_list on the device, the others through ls_search_host
void ls_search_device(Ctx *ctx, int64_t n, const int64_t *lrp, const int64_t *lci, const double *nn, int64_t ld,
                      int64_t k, const double *d, int64_t max_list, const LsOut &out, int64_t *info4);
void ls_accept(int64_t n, const double *nn, int64_t ld, int64_t k, const double *d, int64_t mi, double tau,
               const int32_t *count, const double *err, int32_t *chosen, double *row_err);
// stage times and counts of one ls_interpolation call (the FAMG_SA_LOG line of classical_build)
struct LsStageInfo {
    double ms_candidates = 0, ms_search = 0, ms_build = 0;
    int64_t device_rows = 0, host_rows = 0, subsets = 0, longest = 0, empty_rows = 0;
};
// least_squares' level build after the split (interpolation/mod.rs:654-715): P, the
// coarse near-null (n_coarse x k, ld n_coarse), the accepted error per row (optional)
CsrPtr ls_interpolation(CsrOp &A, const int8_t *point_type, const double *near_null, int64_t ld, int64_t k,
                        const double *weights, int64_t depth, int64_t mi, double tau, int where, double *coarse_nn,
                        double *row_err, LsStageInfo *stage);

// the compatible-relaxation loop (interpolation/mod.rs:574-652) and its guards
enum CrStop : int { CR_CONVERGED = 1, CR_NO_NEW_C = 2, CR_MAX_ITERS = 3, CR_ZERO_VECTOR = 4 };
struct CrConfig {
    double target = 0.3, smoother_cf = 256.0;
    int64_t relax_steps = 5, max_iters = 20;
};
struct CrInfo {
    int64_t rounds = 0;
    double reduction = 1.0;
    int stop = 0;
    std::vector<int64_t> c_per_round;  // the C count after each round
};
// point_type: n entries, 0 F, 1 C, 2 N; c_round (optional, n): the round that made a node a C-point, else -1
int64_t cr_split(const CsrPtr &A, const StrengthGraph &G, const CrConfig &cfg, int8_t *point_type, int32_t *c_round,
                 CrInfo &info);

struct ClassicalConfig {
    int64_t search_depth = 1, depth_ls = 2, max_interp = 3;
    double tau = 1.2;
    CrConfig cr;
    int64_t coarsest_dim = 1000, max_levels = 0;
    double omega = 0.66;
    int smoother = 1, chebyshev_steps = 0, where = 0;
};
// Hierarchy::coarsen (hierarchy.rs:190-248) for InterpolationConfig::Classical
// one coarsening of classical_build: what amg_classical_build's level_info carries
struct ClassicalLevelInfo {
    int64_t n, coarse, cr_rounds, longest, device_rows, host_rows, empty_rows;
};
std::shared_ptr<MultigridOp> classical_build(const CsrPtr &A, const double *nn, int64_t ld, int64_t k,
                                             const double *weights, const ClassicalConfig &cfg,
                                             std::vector<ClassicalLevelInfo> *info);

}  // namespace famg
