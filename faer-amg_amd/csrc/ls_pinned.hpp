// ls_pinned.hpp -- the arithmetic of the classical least-squares interpolation
// search, stated once for the host search (classical_host.cpp) and the device
// kernel (lsinterp.hip).  DESIGN.md 18.
//
// Restated from the reference (paths relative to its root):
//  * constrained_subset_qp          (interpolation/mod.rs:387-431)
//  * validate_weights_constrained   (:312-336)
//  * eval_err                       (:351-356)
//  * the Gram sums of ls_interp_weights (:450-454)
// InterpMode::Constrained only: least_squares hard-codes it (:690) and
// LeastSquaresConfig::solver is never read; weighted_least_squares
// (Regularized, :358-385) is not restated.
//
// faer is not part of the reference tree, so what it computes inside
// self_adjoint_eigen, pseudoinverse() and Lblt is pinned here instead:
//  * sums run in ascending index from 0.0, one product per term;
//  * only the upper triangle of the Gram matrix is formed, and mirrored;
//  * the eigen-decomposition is cyclic Jacobi: sweeps over (0,1), (0,2), ...,
//    (r-2,r-1) in that order, a rotation skipped where the entry is exactly 0,
//    stopping before a sweep once off2 <= 1e-32 * (2 off2 + diag2) (off2, diag2:
//    the squares of the upper off-diagonal and of the diagonal entries) or after
//    LS_JACOBI_SWEEPS sweeps;
//  * the pseudo-inverse drops eigenvalues with |l| <= r * 2^-52 * max|l|;
//  * the KKT system [[G, 1], [1^T, 0]] is solved by Gaussian elimination with
//    partial pivoting, the first row winning ties; a zero pivot divides by zero
//    and the non-finite weights fail validation.
// Only + - * / sqrt appear, each correctly rounded in fp64 on the host and on
// gfx950, and the library is built with -ffp-contract=off: both sides give the
// same bits.  Every loop has compile-time bounds so the kernel keeps the
// matrices in registers.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LS_HD __host__ __device__ __forceinline__
#else
#define LS_HD inline
#endif

namespace famg {

constexpr int LS_MAX_INTERP = 4;      // r <= 4 (amg_classical_config::max_interp)
constexpr int LS_JACOBI_SWEEPS = 16;
constexpr double LS_EPS = 2.220446049250313e-16;  // 2^-52
constexpr double LS_FEAS_TOL = 1e-12, LS_MIN_ABS = 1e-10, LS_MIN_REL = 1e-2;  // :394-396

LS_HD bool ls_finite(double x) { return (x - x) == 0.0; }
LS_HD double ls_abs(double x) { return x < 0.0 ? -x : x; }

// one Gram entry: sum over c of (a[c * lda] * d[c]) * b[c * ldb]
LS_HD double ls_gram_entry(const double *a, int64_t lda, const double *b, int64_t ldb, const double *d, int k) {
    double s = 0.0;
    for (int c = 0; c < k; c++) s += (a[c * lda] * d[c]) * b[c * ldb];
    return s;
}

// validate_weights_constrained (:312-336)
template <int R> LS_HD bool ls_validate(const double (&p)[R]) {
    double max_w = 0.0, sum = 0.0;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < R; i++) {
        if (!ls_finite(p[i]) || p[i] < LS_MIN_ABS) ok = false;
        max_w = max_w > p[i] ? max_w : p[i];
        sum += p[i];
    }
    if (!ok) return false;
    if (sum > 1.0 + LS_FEAS_TOL) return false;
    const double thr = LS_MIN_REL * max_w;
#pragma unroll
    for (int i = 0; i < R; i++)
        if (p[i] < thr) ok = false;
    return ok;
}

// eval_err (:351-356): btb + p G p^T - 2 g.p
template <int R> LS_HD double ls_eval_err(const double (&G)[R][R], const double (&p)[R], const double (&g)[R], double btb) {
    double quad = 0.0, lin = 0.0;
#pragma unroll
    for (int i = 0; i < R; i++) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < R; j++) t += G[i][j] * p[j];
        quad += p[i] * t;
    }
#pragma unroll
    for (int i = 0; i < R; i++) lin += g[i] * p[i];
    return (btb + quad) - 2.0 * lin;
}

// candidate A: p = pinv(G) g by cyclic Jacobi
template <int R> LS_HD void ls_pinv_solve(const double (&G)[R][R], const double (&g)[R], double (&p)[R]) {
    double A[R][R], V[R][R];
#pragma unroll
    for (int i = 0; i < R; i++)
#pragma unroll
        for (int j = 0; j < R; j++) {
            A[i][j] = G[i][j];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < LS_JACOBI_SWEEPS; sweep++) {
        double off2 = 0.0, diag2 = 0.0;
#pragma unroll
        for (int i = 0; i < R; i++) {
            diag2 += A[i][i] * A[i][i];
#pragma unroll
            for (int j = i + 1; j < R; j++) off2 += A[i][j] * A[i][j];
        }
        if (off2 <= 1e-32 * (2.0 * off2 + diag2)) break;
        if (!ls_finite(off2)) break;  // non-finite input: the weights come out non-finite too
#pragma unroll
        for (int pp = 0; pp < R - 1; pp++)
#pragma unroll
            for (int q = pp + 1; q < R; q++) {
                const double apq = A[pp][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[pp][pp]) / (2.0 * apq);
                const double at = ls_abs(theta) + sqrt(theta * theta + 1.0);
                const double t = theta < 0.0 ? -1.0 / at : 1.0 / at;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                A[pp][pp] = A[pp][pp] - t * apq;
                A[q][q] = A[q][q] + t * apq;
                A[pp][q] = 0.0;
                A[q][pp] = 0.0;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    if (r != pp && r != q) {
                        const double arp = A[r][pp], arq = A[r][q];
                        A[r][pp] = c * arp - s * arq;
                        A[pp][r] = A[r][pp];
                        A[r][q] = s * arp + c * arq;
                        A[q][r] = A[r][q];
                    }
                    const double vrp = V[r][pp], vrq = V[r][q];
                    V[r][pp] = c * vrp - s * vrq;
                    V[r][q] = s * vrp + c * vrq;
                }
            }
    }
    double lmax = 0.0;
#pragma unroll
    for (int i = 0; i < R; i++) {
        const double a = ls_abs(A[i][i]);
        lmax = lmax > a ? lmax : a;
    }
    const double thr = (double)R * LS_EPS * lmax;
    double z[R];
#pragma unroll
    for (int i = 0; i < R; i++) {
        double y = 0.0;
#pragma unroll
        for (int j = 0; j < R; j++) y += V[j][i] * g[j];
        z[i] = ls_abs(A[i][i]) <= thr ? 0.0 : y / A[i][i];
        if (!ls_finite(A[i][i])) z[i] = A[i][i] - A[i][i];  // NaN
    }
#pragma unroll
    for (int j = 0; j < R; j++) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < R; i++) s += V[j][i] * z[i];
        p[j] = s;
    }
}

// candidate B: the KKT system with sum(p) = 1 active
template <int R> LS_HD void ls_kkt_solve(const double (&G)[R][R], const double (&g)[R], double (&p)[R]) {
    constexpr int N = R + 1;
    double M[N][N + 1];
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j <= N; j++) {
            if (j == N) M[i][j] = i < R ? g[i < R ? i : 0] : 1.0;
            else if (i < R && j < R) M[i][j] = G[i][j];
            else M[i][j] = (i == R && j == R) ? 0.0 : 1.0;
        }
#pragma unroll
    for (int c = 0; c < N; c++) {
        int piv = c;
        double best = ls_abs(M[c][c]);
#pragma unroll
        for (int i = c + 1; i < N; i++) {
            const double a = ls_abs(M[i][c]);
            if (a > best) {
                best = a;
                piv = i;
            }
        }
#pragma unroll
        for (int i = c + 1; i < N; i++)
            if (i == piv) {
#pragma unroll
                for (int j = 0; j <= N; j++) {
                    const double t = M[c][j];
                    M[c][j] = M[i][j];
                    M[i][j] = t;
                }
            }
#pragma unroll
        for (int i = c + 1; i < N; i++) {
            const double f = M[i][c] / M[c][c];
#pragma unroll
            for (int j = c + 1; j <= N; j++) M[i][j] = M[i][j] - f * M[c][j];
        }
    }
    double x[N];
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double s = M[i][N];
#pragma unroll
        for (int j = i + 1; j < N; j++) s = s - M[i][j] * x[j];
        x[i] = s / M[i][i];
    }
#pragma unroll
    for (int i = 0; i < R; i++) p[i] = x[i];
}

// constrained_subset_qp (:387-431): weights and error of one subset, or false
template <int R> LS_HD bool ls_subset_qp(const double (&G)[R][R], const double (&g)[R], double btb, double (&p)[R],
                                         double &err) {
    ls_pinv_solve<R>(G, g, p);
    if (!ls_validate<R>(p)) {
        ls_kkt_solve<R>(G, g, p);
        if (!ls_validate<R>(p)) return false;
    }
    err = ls_eval_err<R>(G, p, g, btb);
    return true;
}

// C(n, r) for r <= 4; n <= 2^15 keeps it inside int64
LS_HD int64_t ls_choose(int64_t n, int r) {
    if (n < r) return 0;
    switch (r) {
    case 0: return 1;
    case 1: return n;
    case 2: return n * (n - 1) / 2;
    case 3: return n * (n - 1) / 2 * (n - 2) / 3;
    default: return n * (n - 1) / 2 * (n - 2) / 3 * (n - 3) / 4;
    }
}

// the rank-th r-subset of 0..L-1 in lexicographic order (combinations(r), :463)
template <int R> LS_HD void ls_unrank(int64_t rank, int L, int (&idx)[R]) {
    int a = 0;
#pragma unroll
    for (int t = 0; t < R; t++) {
        for (;; a++) {
            const int64_t below = ls_choose(L - a - 1, R - 1 - t);
            if (rank < below) break;
            rank -= below;
        }
        idx[t] = a++;
    }
}

// the next subset in lexicographic order (the caller stops at the last one)
template <int R> LS_HD void ls_next(int L, int (&idx)[R]) {
    bool done = false;
#pragma unroll
    for (int t = R - 1; t >= 0; t--) {
        if (!done && idx[t] < L - R + t) {
            idx[t]++;
#pragma unroll
            for (int u = t + 1; u < R; u++) idx[u] = idx[u - 1] + 1;
            done = true;
        }
    }
}

}  // namespace famg
