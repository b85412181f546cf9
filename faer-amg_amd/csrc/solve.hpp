// solve.hpp -- device-resident solve loops and the Composite preconditioner.
//
// The loops keep every vector in HBM; only the scalars of each iteration (dots)
// come back to the host.  They are written once over a small set of callbacks so
// the single-GPU and distributed (dots all-reduced over ranks) drivers share the
// arithmetic exactly.
#pragma once

#include <functional>
#include <mutex>

#include "famg.hpp"

namespace famg {

struct SolveOps {
    Ctx *ctx = nullptr;
    int64_t n = 0;                                                          // local rows
    // allocation length of the vectors A and resid read (>= n): a distributed
    // operator keeps its halo entries behind the owned rows, so the loops keep
    // x and p in buffers of this length and A reads them in place
    int64_t n_alloc = 0;
    std::function<void(double *out, double *x)> A;                          // out = A x (x: n_alloc, halo written)
    std::function<void(double *r, const double *b, double *x)> resid;        // r = b - A x (x: n_alloc)
    std::function<void(double *out, const double *r)> M;                    // out = M r (empty: identity)
    std::function<double(const double *, const double *)> dot;              // global dot
};

// Stationary iteration (examples/simple_geometric.rs:117-158): rho_k =
// ||b - A x_k|| / ||b||, stop below rel_tol or at max_iter, else x += M r.
int64_t stationary_impl(const SolveOps &o, const double *b, double *x, int64_t max_iter, double rel_tol,
                        double *hist);

// Preconditioned CG (the counterpart of faer conjugate_gradient as called by
// utils.rs:600-609): stop when ||r|| <= max(rel_tol ||b||, abs_tol).
int64_t pcg_impl(const SolveOps &o, const double *b, double *x, int64_t max_iter, double rel_tol, double abs_tol,
                 double *hist);

// The two loops over k right-hand sides at once (single GPU; B, X column-major
// device blocks).  Every column runs its own recurrence -- unlike faer's
// conjugate_gradient on an n x k rhs, which couples the columns -- and is bitwise
// the single-vector loop above: A P / B - A X as one SpMM when A is a CSR matrix,
// M through apply_block, the vector work in pcg.hip's k-wide kernels, alpha, beta
// and r.z on the device.  Per iteration the host reads the active columns' r.r in
// one copy and one stream synchronise, and does sqrt, history and the stopping
// test as the single-vector loop does.  A column that stops is frozen (its X never
// written again) and leaves the workspace, which stays compact: the SpMM, the
// preconditioner and the vector kernels run over the active columns only.
// Chunks of MG_BLOCK_COLS columns, one after another.  M null: identity (PCG only).
// hist: max_iter x k column-major (ld_hist) or null; iters: k entries.
void pcg_block_impl(LinOp &A, LinOp *M, const double *B, int64_t ldb, double *X, int64_t ldx, int64_t k,
                    int64_t max_iter, double rel_tol, double abs_tol, double *hist, int64_t ld_hist, int64_t *iters);
void stationary_block_impl(LinOp &A, LinOp &M, const double *B, int64_t ldb, double *X, int64_t ldx, int64_t k,
                           int64_t max_iter, double rel_tol, double *hist, int64_t ld_hist, int64_t *iters);

// The rank-revealing solve G^+ Y of the coupled block CG (host, fp64; amg.h and
// DESIGN.md 15): G symmetrised, columns with g_jj <= 0 dropped, the rest scaled
// to unit diagonal, Cholesky with diagonal pivoting (largest remaining diagonal
// first, ties to the lower index) stopped at the first pivot <= rank_tol.
// G and Y are read as element (i, j) at [i * ld + j]; solve() writes a k x m
// column-major result whose rows of dropped columns are zero.
struct RankChol {
    int64_t nc = 0;                   // columns with a positive diagonal
    std::vector<int64_t> cand, order; // their indices; the pivots taken, as positions in cand
    std::vector<double> sc, C, L;     // D^-1/2; the scaled matrix and its factor (nc x nc, row a = candidate a)
    int64_t rank() const { return (int64_t)order.size(); }
    void factor(const double *G, int64_t ldg, int64_t k, double rank_tol);
    void solve(const double *Y, int64_t ldy, int64_t k, int64_t m, double *out) const;
};

// Coupled block CG over k <= 32 right-hand sides (single GPU; the counterpart of
// faer's conjugate_gradient on an n x k rhs, defined in amg.h / DESIGN.md 15): one
// k x k system for the step and one for the new directions per iteration, all
// columns searched in the sum of their Krylov spaces.  The workspace R, Z, P, Q
// is n x k (leading dimension n), allocated once per call.  Q = A P and B - A X
// run as one SpMM when A is a CSR matrix, M through apply_block; the Gram products
// and the updates are bcg.hip's kernels, the norms cg_dot_cols after the update.
// At most three host synchronisations per iteration for all columns together --
// (G, S) down and alpha up, the norms, T down and beta up (amg_pcg_solve: three
// per column).  hist: max_iter x k column-major or null; ranks: max_iter entries
// or null; *iters: one count for the block.
void block_cg_impl(LinOp &A, LinOp *M, const double *B, int64_t ldb, double *X, int64_t ldx, int64_t k,
                   int64_t max_iter, double rel_tol, double abs_tol, double rank_tol, double *hist, int64_t ld_hist,
                   int64_t *ranks, int64_t *iters);

// Composite (preconditioners/composite.rs:11-83): components c_0..c_{m-1}
// applied c_{m-1}, ..., c_1, c_0, c_1, ..., c_{m-1}; each step
// out += c(r); r = rhs - A out, starting from out = 0, r = rhs.
struct CompositeOp : LinOp {
    LinOpPtr A;
    std::vector<LinOpPtr> comps;
    DevBuf<double> ws, bws;  // bws: the n x k workspace of apply_block
    std::mutex mtx;
    Kind kind() const override { return Kind::Composite; }
    bool is_precond() const override { return true; }
    void apply(double *out, const double *rhs) override;
    // the same 2m - 1 steps on n x k blocks: each component through its apply_block,
    // R = RHS - A OUT as one SpMM with the residual epilogue when A is a CSR matrix
    // (flag FLAG_BLOCK_CYCLE; 0: apply() per column)
    void apply_block(double *out, int64_t ldo, const double *rhs, int64_t ldr, int64_t k) override;
};

// r = b - A x using the fused residual SpMV when A is a CSR matrix.
void residual(LinOp &A, double *r, const double *b, const double *x);

}  // namespace famg
