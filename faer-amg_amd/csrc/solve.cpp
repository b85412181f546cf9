// solve.cpp -- solve loops, Composite, and their C ABI (include/amg.h).
#include "solve.hpp"

#include <algorithm>
#include <cmath>

#include "handles.hpp"

using namespace famg;

namespace famg {

void residual(LinOp &A, double *r, const double *b, const double *x) {
    hipStream_t s = A.ctx->stream;
    if (auto *c = dynamic_cast<CsrOp *>(&A)) {
        SpmvEpi epi;
        epi.b = b;
        spmv(c->m, x, r, SPMV_RESID, epi, s);
        return;
    }
    A.apply(r, x);
    vec_sub(r, b, r, A.nrows, s);
}

// x in a buffer of the operator's allocation length (the caller's when that is n)
static double *padded_x(const SolveOps &o, double *x, DevBuf<double> &xp) {
    if (o.n_alloc <= o.n) return x;
    xp.resize(o.n_alloc);
    vec_copy(xp.get(), x, o.n, o.ctx->stream);
    return xp.get();
}

int64_t stationary_impl(const SolveOps &o, const double *b, double *x_user, int64_t max_iter, double rel_tol,
                        double *hist) {
    hipStream_t s = o.ctx->stream;
    const int64_t n = o.n;
    DevBuf<double> r(std::max<int64_t>(1, n)), z(std::max<int64_t>(1, n)), xp;
    double *x = padded_x(o, x_user, xp);
    const double bn = std::sqrt(o.dot(b, b));
    int64_t it = 0;
    for (;;) {
        o.resid(r.get(), b, x);
        const double rel = std::sqrt(o.dot(r.get(), r.get())) / bn;
        it++;
        if (hist) hist[it - 1] = rel;
        if (rel < rel_tol || it >= max_iter) break;
        o.M(z.get(), r.get());
        vec_add_inplace(x, z.get(), n, s);
    }
    if (x != x_user) vec_copy(x_user, x, n, s);
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    return it;
}

int64_t pcg_impl(const SolveOps &o, const double *b, double *x, int64_t max_iter, double rel_tol, double abs_tol,
                 double *hist) {
    hipStream_t s = o.ctx->stream;
    const int64_t n = o.n;
    const int64_t nb = std::max<int64_t>(1, n);
    DevBuf<double> r(nb), z(nb), p(std::max(nb, o.n_alloc)), Ap(nb), xp;
    o.resid(r.get(), b, padded_x(o, x, xp));  // x itself only moves by axpys below
    const double bn = std::sqrt(o.dot(b, b));
    const double tol = std::max(rel_tol * bn, abs_tol);
    int64_t it = 0;
    if (std::sqrt(o.dot(r.get(), r.get())) > tol) {
        auto pc = [&](double *dst, const double *src) {
            if (o.M) o.M(dst, src);
            else vec_copy(dst, src, n, s);
        };
        pc(z.get(), r.get());
        vec_copy(p.get(), z.get(), n, s);
        double rz = o.dot(r.get(), z.get());
        for (it = 1; it <= max_iter; it++) {
            o.A(Ap.get(), p.get());
            const double alpha = rz / o.dot(p.get(), Ap.get());
            vec_axpy(x, alpha, p.get(), n, s);
            vec_axpy(r.get(), -alpha, Ap.get(), n, s);
            const double rn = std::sqrt(o.dot(r.get(), r.get()));
            if (hist) hist[it - 1] = rn / bn;
            if (rn <= tol) break;
            pc(z.get(), r.get());
            const double rzn = o.dot(r.get(), z.get());
            const double beta = rzn / rz;
            rz = rzn;
            vec_xpay(p.get(), beta, z.get(), n, s);
        }
    }
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    return it;
}

// ------------------------------------------------------- block solve drivers

namespace {

// pinned host memory for the per-iteration copies (freed when the call ends)
template <typename T> struct PinnedBuf {
    T *p = nullptr;
    explicit PinnedBuf(size_t n) { FAMG_CHECK_HIP(hipHostMalloc((void **)&p, std::max<size_t>(1, n) * sizeof(T))); }
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
};

// the workspace of one block solve, allocated once per call: nblk blocks of
// n x kmax (leading dimension n), the dots' partials, the per-slot scalars
// (alpha, beta, rz, and two rows of results the host copies) and the slot map
struct BlockWs {
    int64_t kmax, ld;
    DevBuf<double> blocks, scal;
    DevBuf<int32_t> map;
    PinnedBuf<double> h_res;
    PinnedBuf<int32_t> h_map;
    BlockWs(int64_t n, int64_t k, int nblk)
        : kmax(std::min<int64_t>(k, MG_BLOCK_COLS)), ld(std::max<int64_t>(1, n)),
          blocks((size_t)nblk * ld * kmax), scal((size_t)kmax * (VEC_DOT_PARTIALS + 5)), map((size_t)kmax),
          h_res(2 * (size_t)kmax), h_map((size_t)kmax) {}
    double *block(int b) const { return blocks.get() + (size_t)b * ld * kmax; }
    double *partials() const { return scal.get(); }
    double *alpha() const { return scal.get() + kmax * VEC_DOT_PARTIALS; }
    double *beta() const { return alpha() + kmax; }
    double *rz() const { return beta() + kmax; }
    double *res() const { return rz() + kmax; }  // 2 * kmax
    // the first na entries of the host map to the device (the host copy is only
    // rewritten after a stream synchronise, so the copy has left it by then)
    void upload_map(int64_t na, hipStream_t s) const {
        if (na > 0)
            FAMG_CHECK_HIP(hipMemcpyAsync(map.get(), h_map.p, na * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    // cnt results to the host, then wait: the one host round trip of an iteration
    void fetch(int64_t cnt, hipStream_t s) const {
        FAMG_CHECK_HIP(hipMemcpyAsync(h_res.p, res(), cnt * sizeof(double), hipMemcpyDeviceToHost, s));
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
    }
};

// OUT (ld n) = B - A X over kw columns, as residual() does per column
void residual_block(LinOp &A, CsrOp *a, double *out, int64_t ldo, const double *B, int64_t ldb, const double *X,
                    int64_t ldx, int64_t kw) {
    hipStream_t s = A.ctx->stream;
    if (a) {
        spmm_epi(a->m, X, ldx, out, ldo, kw, SPMV_RESID, SpmmEpi{B, ldb, nullptr}, s);
        return;
    }
    A.apply_block(out, ldo, X, ldx, kw);
    vec_sub_cols(out, ldo, B, ldb, out, ldo, A.nrows, kw, s);
}

}  // namespace

void pcg_block_impl(LinOp &A, LinOp *M, const double *B, int64_t ldb, double *X, int64_t ldx, int64_t k,
                    int64_t max_iter, double rel_tol, double abs_tol, double *hist, int64_t ld_hist, int64_t *iters) {
    if (k <= 0) return;
    hipStream_t s = A.ctx->stream;
    const int64_t n = A.nrows;
    BlockWs w(n, k, 4);
    const int64_t ld = w.ld;
    double *R = w.block(0), *Z = w.block(1), *P = w.block(2), *AP = w.block(3);
    double *Zp = M ? Z : R;  // identity preconditioner: z is r itself
    auto *a = dynamic_cast<CsrOp *>(&A);
    std::vector<int64_t> col(w.kmax);  // slot -> column of the chunk
    std::vector<double> bn(w.kmax), tol(w.kmax);
    std::vector<char> stop(w.kmax);
    for (int64_t c0 = 0; c0 < k; c0 += MG_BLOCK_COLS) {
        const int64_t kw = std::min<int64_t>(MG_BLOCK_COLS, k - c0);
        const double *Bc = B + c0 * ldb;
        double *Xc = X + c0 * ldx;
        double *histc = hist ? hist + c0 * ld_hist : nullptr;
        int64_t *itc = iters + c0;
        int64_t na = kw;  // active slots [0, na)
        // slot s takes the last active slot's column (R, and P / rz once they live)
        auto drop = [&](int64_t sl, bool live) {
            const int64_t last = na - 1;
            if (sl != last) {
                vec_copy(R + sl * ld, R + last * ld, n, s);
                if (live) {
                    vec_copy(P + sl * ld, P + last * ld, n, s);
                    FAMG_CHECK_HIP(hipMemcpyAsync(w.rz() + sl, w.rz() + last, sizeof(double), hipMemcpyDeviceToDevice, s));
                }
                col[sl] = col[last];
                bn[sl] = bn[last];
                tol[sl] = tol[last];
                w.h_map.p[sl] = w.h_map.p[last];
            }
            na--;
        };
        // descending, so the slot moved in has been looked at already
        auto compact = [&](bool live) {
            const int64_t before = na;
            for (int64_t sl = before; sl-- > 0;)
                if (stop[sl]) drop(sl, live);
            if (na != before) w.upload_map(na, s);
        };
        for (int64_t sl = 0; sl < kw; sl++) {
            col[sl] = sl;
            w.h_map.p[sl] = (int32_t)sl;
        }
        w.upload_map(kw, s);
        residual_block(A, a, R, ld, Bc, ldb, Xc, ldx, kw);
        cg_dot_cols(Bc, ldb, Bc, ldb, n, kw, w.partials(), s);
        cg_final_cols(CG_FINAL_STORE, w.partials(), w.res(), nullptr, kw, s);
        cg_dot_cols(R, ld, R, ld, n, kw, w.partials(), s);
        cg_final_cols(CG_FINAL_STORE, w.partials(), w.res() + kw, nullptr, kw, s);
        w.fetch(2 * kw, s);
        for (int64_t sl = 0; sl < kw; sl++) {
            bn[sl] = std::sqrt(w.h_res.p[sl]);
            tol[sl] = std::max(rel_tol * bn[sl], abs_tol);
            stop[sl] = !(std::sqrt(w.h_res.p[kw + sl]) > tol[sl]);
            if (stop[sl]) itc[sl] = 0;
        }
        compact(false);
        if (na == 0) continue;
        if (M) M->apply_block(Z, ld, R, ld, na);
        vec_copy_cols(P, ld, Zp, ld, n, na, s);
        cg_dot_cols(R, ld, Zp, ld, n, na, w.partials(), s);
        cg_final_cols(CG_FINAL_STORE, w.partials(), w.rz(), nullptr, na, s);
        for (int64_t it = 1; it <= max_iter && na > 0; it++) {
            if (a) spmm_epi(a->m, P, ld, AP, ld, na, SPMV_SET, SpmmEpi{}, s);
            else A.apply_block(AP, ld, P, ld, na);
            cg_dot_cols(P, ld, AP, ld, n, na, w.partials(), s);
            cg_final_cols(CG_FINAL_ALPHA, w.partials(), w.alpha(), w.rz(), na, s);
            cg_update_cols(Xc, ldx, w.map.get(), P, AP, R, ld, w.alpha(), n, na, w.partials(), s);
            cg_final_cols(CG_FINAL_STORE, w.partials(), w.res(), nullptr, na, s);
            w.fetch(na, s);
            for (int64_t sl = 0; sl < na; sl++) {
                const double rn = std::sqrt(w.h_res.p[sl]);
                if (histc) histc[col[sl] * ld_hist + it - 1] = rn / bn[sl];
                stop[sl] = rn <= tol[sl];
                if (stop[sl]) itc[col[sl]] = it;
            }
            compact(true);
            if (na == 0 || it == max_iter) break;  // the last iteration's z, beta and p are never read
            if (M) M->apply_block(Z, ld, R, ld, na);
            cg_dot_cols(R, ld, Zp, ld, n, na, w.partials(), s);
            cg_final_cols(CG_FINAL_BETA, w.partials(), w.beta(), w.rz(), na, s);
            cg_xpay_cols(P, ld, Zp, ld, w.beta(), n, na, s);
        }
        for (int64_t sl = 0; sl < na; sl++) itc[col[sl]] = max_iter + 1;
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
    }
}

void stationary_block_impl(LinOp &A, LinOp &M, const double *B, int64_t ldb, double *X, int64_t ldx, int64_t k,
                           int64_t max_iter, double rel_tol, double *hist, int64_t ld_hist, int64_t *iters) {
    if (k <= 0) return;
    hipStream_t s = A.ctx->stream;
    const int64_t n = A.nrows;
    BlockWs w(n, k, 2);
    const int64_t ld = w.ld;
    double *R = w.block(0), *Z = w.block(1);
    auto *a = dynamic_cast<CsrOp *>(&A);
    // Nothing but X carries over from sweep to sweep, so the slots stay in column
    // order: a column that stops is closed up (R's columns behind it move down
    // one) and R = B - A X runs as one SpMM per run of adjacent active columns.
    std::vector<int64_t> col(w.kmax);
    std::vector<double> bn(w.kmax);
    std::vector<char> stop(w.kmax);
    for (int64_t c0 = 0; c0 < k; c0 += MG_BLOCK_COLS) {
        const int64_t kw = std::min<int64_t>(MG_BLOCK_COLS, k - c0);
        const double *Bc = B + c0 * ldb;
        double *Xc = X + c0 * ldx;
        double *histc = hist ? hist + c0 * ld_hist : nullptr;
        int64_t *itc = iters + c0;
        int64_t na = kw;
        for (int64_t sl = 0; sl < kw; sl++) {
            col[sl] = sl;
            w.h_map.p[sl] = (int32_t)sl;
        }
        w.upload_map(kw, s);
        cg_dot_cols(Bc, ldb, Bc, ldb, n, kw, w.partials(), s);
        cg_final_cols(CG_FINAL_STORE, w.partials(), w.res(), nullptr, kw, s);
        w.fetch(kw, s);
        for (int64_t sl = 0; sl < kw; sl++) bn[sl] = std::sqrt(w.h_res.p[sl]);
        for (int64_t it = 1; na > 0; it++) {
            for (int64_t s0 = 0; s0 < na;) {
                int64_t s1 = s0 + 1;
                while (s1 < na && col[s1] == col[s1 - 1] + 1) s1++;
                residual_block(A, a, R + s0 * ld, ld, Bc + col[s0] * ldb, ldb, Xc + col[s0] * ldx, ldx, s1 - s0);
                s0 = s1;
            }
            cg_dot_cols(R, ld, R, ld, n, na, w.partials(), s);
            cg_final_cols(CG_FINAL_STORE, w.partials(), w.res(), nullptr, na, s);
            w.fetch(na, s);
            bool any = false;
            for (int64_t sl = 0; sl < na; sl++) {
                const double rel = std::sqrt(w.h_res.p[sl]) / bn[sl];
                if (histc) histc[col[sl] * ld_hist + it - 1] = rel;
                stop[sl] = rel < rel_tol || it >= max_iter;
                if (stop[sl]) {
                    itc[col[sl]] = it;
                    any = true;
                }
            }
            if (any) {
                int64_t dst = 0;
                for (int64_t sl = 0; sl < na; sl++) {
                    if (stop[sl]) continue;
                    if (dst != sl) {
                        vec_copy(R + dst * ld, R + sl * ld, n, s);
                        col[dst] = col[sl];
                        bn[dst] = bn[sl];
                        w.h_map.p[dst] = w.h_map.p[sl];
                    }
                    dst++;
                }
                na = dst;
                w.upload_map(na, s);
            }
            if (na == 0) break;
            M.apply_block(Z, ld, R, ld, na);
            cg_add_cols(Xc, ldx, w.map.get(), Z, ld, n, na, s);
        }
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
    }
}

// ------------------------------------------------------- coupled block CG

void RankChol::factor(const double *G, int64_t ldg, int64_t k, double rank_tol) {
    sc.assign(k, 0.0);
    cand.clear();
    order.clear();
    for (int64_t j = 0; j < k; j++) {
        const double g = G[j * ldg + j];
        if (g > 0.0) {  // a zero or converged direction, a non-SPD A or M, a NaN: dropped
            cand.push_back(j);
            sc[j] = 1.0 / std::sqrt(g);
        }
    }
    nc = (int64_t)cand.size();
    C.assign(nc * nc, 0.0);
    L.assign(nc * nc, 0.0);
    std::vector<double> dg(nc, 1.0);
    std::vector<char> taken(nc, 0);
    for (int64_t a = 0; a < nc; a++)
        for (int64_t b = 0; b < nc; b++) {
            const int64_t i = cand[a], j = cand[b];
            C[a * nc + b] = a == b ? 1.0 : ((0.5 * (G[i * ldg + j] + G[j * ldg + i])) * sc[i]) * sc[j];
        }
    for (int64_t t = 0; t < nc; t++) {
        int64_t p = -1;
        for (int64_t a = 0; a < nc; a++)
            if (!taken[a] && (p < 0 || dg[a] > dg[p])) p = a;  // ties: the lower index
        if (p < 0 || !(dg[p] > rank_tol)) break;
        const double lpp = std::sqrt(dg[p]);
        L[p * nc + t] = lpp;
        taken[p] = 1;
        order.push_back(p);
        for (int64_t a = 0; a < nc; a++) {
            if (taken[a]) continue;
            double s = C[a * nc + p];
            for (int64_t u = 0; u < t; u++) s -= L[a * nc + u] * L[p * nc + u];
            const double l = s / lpp;
            L[a * nc + t] = l;
            dg[a] -= l * l;
        }
    }
}

void RankChol::solve(const double *Y, int64_t ldy, int64_t k, int64_t m, double *out) const {
    const int64_t r = rank();
    std::vector<double> z(std::max<int64_t>(1, r));
    std::fill(out, out + k * m, 0.0);
    for (int64_t j = 0; j < m; j++) {
        for (int64_t t = 0; t < r; t++) {
            const int64_t a = order[t];
            double s = sc[cand[a]] * Y[cand[a] * ldy + j];
            for (int64_t u = 0; u < t; u++) s -= L[a * nc + u] * z[u];
            z[t] = s / L[a * nc + t];
        }
        for (int64_t t = r; t-- > 0;) {
            double s = z[t];
            for (int64_t u = t + 1; u < r; u++) s -= L[order[u] * nc + t] * z[u];
            z[t] = s / L[order[t] * nc + t];
        }
        for (int64_t t = 0; t < r; t++) out[j * k + cand[order[t]]] = sc[cand[order[t]]] * z[t];
    }
}

void block_cg_impl(LinOp &A, LinOp *M, const double *B, int64_t ldb, double *X, int64_t ldx, int64_t k,
                   int64_t max_iter, double rel_tol, double abs_tol, double rank_tol, double *hist, int64_t ld_hist,
                   int64_t *ranks, int64_t *iters) {
    if (k <= 0) return;
    FAMG_REQUIRE(k <= BCG_MAX_W, AMG_ERR_UNSUPPORTED, "block CG: more than 32 columns");
    if (!(rank_tol > 0.0)) rank_tol = 0x1p-26;
    hipStream_t s = A.ctx->stream;
    const int64_t n = A.nrows, ld = std::max<int64_t>(1, n);
    DevBuf<double> blocks((size_t)4 * ld * k), scal((size_t)k * (VEC_DOT_PARTIALS + 2)), coef(2 * BCG_MAX_W * BCG_MAX_W);
    PinnedBuf<double> h_res(2 * (size_t)k), h_gram(2 * BCG_MAX_W * BCG_MAX_W), h_coef(2 * BCG_MAX_W * BCG_MAX_W);
    BcgWork gw;
    gw.reserve(*A.ctx, n);
    double *R = blocks.get(), *Z = R + ld * k, *P = Z + ld * k, *Q = P + ld * k;
    double *Zp = M ? Z : R;  // identity preconditioner: z is r itself
    double *partials = scal.get(), *res = partials + k * VEC_DOT_PARTIALS;
    double *d_alpha = coef.get(), *d_beta = d_alpha + BCG_MAX_W * BCG_MAX_W;
    double *h_alpha = h_coef.p, *h_beta = h_alpha + BCG_MAX_W * BCG_MAX_W;
    const size_t coef_bytes = (size_t)k * 8 * ceil_div(k, 8) * sizeof(double);
    auto *a = dynamic_cast<CsrOp *>(&A);
    std::vector<double> bn(k), tol(k), sol(k * k);
    RankChol ch;
    // the squared column norms of V into res[off ..], no synchronise
    auto norms = [&](const double *V, int64_t ldv, int64_t off) {
        cg_dot_cols(V, ldv, V, ldv, n, k, partials, s);
        cg_final_cols(CG_FINAL_STORE, partials, res + off, nullptr, k, s);
    };
    auto fetch = [&](int64_t cnt) {
        FAMG_CHECK_HIP(hipMemcpyAsync(h_res.p, res, cnt * sizeof(double), hipMemcpyDeviceToHost, s));
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
    };
    residual_block(A, a, R, ld, B, ldb, X, ldx, k);
    norms(B, ldb, 0);
    norms(R, ld, k);
    fetch(2 * k);
    bool done = true;
    for (int64_t c = 0; c < k; c++) {
        bn[c] = std::sqrt(h_res.p[c]);
        tol[c] = std::max(abs_tol, rel_tol * bn[c]);
        done = done && std::sqrt(h_res.p[k + c]) <= tol[c];
    }
    if (done) {
        *iters = 0;
        return;
    }
    if (M) M->apply_block(Z, ld, R, ld, k);
    vec_copy_cols(P, ld, Zp, ld, n, k, s);
    for (int64_t it = 1; it <= max_iter; it++) {
        if (a) spmm_epi(a->m, P, ld, Q, ld, k, SPMV_SET, SpmmEpi{}, s);
        else A.apply_block(Q, ld, P, ld, k);
        // [G | S] = P^T [Q | R]: synchronisation 1
        const int ldg = bcg_gram(P, ld, k, Q, ld, k, R, ld, k, n, gw, h_gram.p, s);
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
        ch.factor(h_gram.p, ldg, k, rank_tol);
        ch.solve(h_gram.p + k, ldg, k, k, sol.data());
        if (ranks) ranks[it - 1] = ch.rank();
        bcg_pack_coef(sol.data(), k, k, h_alpha);
        FAMG_CHECK_HIP(hipMemcpyAsync(d_alpha, h_alpha, coef_bytes, hipMemcpyHostToDevice, s));
        bcg_gemm("bcg_update", X, ldx, X, ldx, P, ld, d_alpha, k, k, n, +1, s);
        bcg_gemm("bcg_update", R, ld, R, ld, Q, ld, d_alpha, k, k, n, -1, s);
        norms(R, ld, 0);
        fetch(k);  // synchronisation 2
        done = true;
        for (int64_t c = 0; c < k; c++) {
            const double rn = std::sqrt(h_res.p[c]);
            if (hist) hist[c * ld_hist + it - 1] = bn[c] == 0.0 ? rn : rn / bn[c];
            done = done && rn <= tol[c];
        }
        if (done) {
            *iters = it;
            return;
        }
        if (ch.rank() == 0 || it == max_iter) break;  // no direction left; the last z, beta and p are never read
        if (M) M->apply_block(Z, ld, R, ld, k);
        // T = Q^T Z: synchronisation 3 (the factor of G serves beta too)
        const int ldt = bcg_gram(Q, ld, k, Zp, ld, k, nullptr, 0, 0, n, gw, h_gram.p, s);
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
        ch.solve(h_gram.p, ldt, k, k, sol.data());
        bcg_pack_coef(sol.data(), k, k, h_beta);
        FAMG_CHECK_HIP(hipMemcpyAsync(d_beta, h_beta, coef_bytes, hipMemcpyHostToDevice, s));
        bcg_gemm("bcg_dir", P, ld, Zp, ld, P, ld, d_beta, k, k, n, -1, s);
    }
    *iters = max_iter + 1;
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
}

void CompositeOp::apply(double *out, const double *rhs) {
    std::lock_guard<std::mutex> lk(mtx);
    hipStream_t s = ctx->stream;
    const int64_t n = nrows;
    if (ws.size() < (size_t)std::max<int64_t>(1, n)) ws.resize(std::max<int64_t>(1, n));
    vec_fill(out, 0.0, n, s);
    vec_copy(ws.get(), rhs, n, s);
    auto step = [&](LinOp &c) {
        c.apply_in_place(ws.get());
        vec_add_inplace(out, ws.get(), n, s);
        residual(*A, ws.get(), rhs, out);
    };
    for (size_t k = comps.size(); k-- > 0;) step(*comps[k]);
    for (size_t k = 1; k < comps.size(); k++) step(*comps[k]);
}

void CompositeOp::apply_block(double *out, int64_t ldo, const double *rhs, int64_t ldr, int64_t k) {
    if (flag(FLAG_BLOCK_CYCLE) == 0 || k <= 0) {
        LinOp::apply_block(out, ldo, rhs, ldr, k);
        return;
    }
    std::lock_guard<std::mutex> lk(mtx);
    FAMG_REQUIRE(out != rhs, AMG_ERR_INVALID, "composite apply: out must not alias rhs");
    FAMG_REQUIRE(ldo >= nrows && ldr >= nrows, AMG_ERR_INVALID, "composite apply: leading dimension too small");
    hipStream_t s = ctx->stream;
    const int64_t n = nrows;
    // chunks of MG_BLOCK_COLS columns, as the multigrid takes them: bounds the workspace
    const int64_t kmax = std::min<int64_t>(k, MG_BLOCK_COLS);
    const size_t need = (size_t)std::max<int64_t>(1, n) * kmax;
    if (bws.size() < 2 * need) bws.resize(2 * need);
    double *R = bws.get(), *Z = bws.get() + need;  // the residual block, a component's result
    auto *a = dynamic_cast<CsrOp *>(A.get());
    for (int64_t c0 = 0; c0 < k; c0 += MG_BLOCK_COLS) {
        const int64_t kw = std::min<int64_t>(MG_BLOCK_COLS, k - c0);
        double *o = out + c0 * ldo;
        const double *b = rhs + c0 * ldr;
        if (n > 0)  // OUT = +0.0
            FAMG_CHECK_HIP(hipMemset2DAsync(o, ldo * sizeof(double), 0, n * sizeof(double), kw, s));
        vec_copy_cols(R, n, b, ldr, n, kw, s);
        auto step = [&](LinOp &c) {
            c.apply_block(Z, n, R, n, kw);  // apply_in_place: copy to scratch, then apply
            vec_add_cols(o, ldo, Z, n, n, kw, s);
            if (a) {
                spmm_epi(a->m, o, ldo, R, n, kw, SPMV_RESID, SpmmEpi{b, ldr, nullptr}, s);
            } else {
                A->apply_block(R, n, o, ldo, kw);
                vec_sub_cols(R, n, b, ldr, R, n, n, kw, s);
            }
        };
        for (size_t q = comps.size(); q-- > 0;) step(*comps[q]);
        for (size_t q = 1; q < comps.size(); q++) step(*comps[q]);
    }
}

}  // namespace famg

namespace {

LinOp &need_op(const amg_linop *h) {
    FAMG_REQUIRE(h && h->op, AMG_ERR_INVALID, "null amg_linop handle");
    return *h->op;
}

SolveOps single_gpu_ops(LinOp &a, LinOp *m) {
    SolveOps o;
    o.ctx = a.ctx;
    o.n = a.nrows;
    o.n_alloc = a.nrows;
    o.A = [&a](double *out, double *x) { a.apply(out, x); };
    o.resid = [&a](double *r, const double *b, double *x) { residual(a, r, b, x); };
    if (m) o.M = [m](double *out, const double *r) { m->apply(out, r); };
    Ctx *ctx = a.ctx;
    const int64_t n = a.nrows;
    o.dot = [ctx, n](const double *u, const double *v) { return vec_dot(u, v, n, *ctx); };
    return o;
}

// the block drivers' argument checks that need no handle (before the handle
// checks, as in amg_adaptive_build) ...
void block_solve_args(const double *B, const double *X, int64_t k, const double *hist, int64_t ld_hist,
                      int64_t max_iter, const int64_t *iters) {
    FAMG_REQUIRE(B && X && iters, AMG_ERR_INVALID, "block solve: null B, X or iters");
    FAMG_REQUIRE(k >= 0, AMG_ERR_INVALID, "block solve: negative column count");
    FAMG_REQUIRE(!hist || ld_hist >= max_iter, AMG_ERR_INVALID, "block solve: ld_hist below max_iter");
    FAMG_REQUIRE(B != X, AMG_ERR_INVALID, "block solve: B must not alias X");
}

// ... and the ones that need the operators
void block_solve_ops(LinOp &a, LinOp *m, const double *B, int64_t ldb, const double *X, int64_t ldx, int64_t k) {
    auto dist = [](const LinOp &o) { return o.kind() == Kind::DistCsr || o.kind() == Kind::DistMultigrid; };
    FAMG_REQUIRE(!dist(a) && !(m && dist(*m)), AMG_ERR_UNSUPPORTED,
                 "block solve: distributed operators have no block cycle (amg_dist_pcg_solve per column)");
    FAMG_REQUIRE(a.nrows == a.ncols && (!m || (m->nrows == a.nrows && m->ncols == a.nrows)), AMG_ERR_DIM,
                 "solver dims");
    const int64_t n = a.nrows;
    FAMG_REQUIRE(ldb >= n && ldx >= n, AMG_ERR_INVALID, "block solve: leading dimension too small");
    if (k > 0 && n > 0) {  // the two blocks' extents must not overlap
        const double *be = B + (k - 1) * ldb + n, *xe = X + (k - 1) * ldx + n;
        FAMG_REQUIRE(be <= X || xe <= B, AMG_ERR_INVALID, "block solve: B must not alias X");
    }
}

}  // namespace

extern "C" {

amg_status amg_composite_create(const amg_linop *A, amg_linop *const *components, int64_t ncomponents,
                                amg_linop **out) {
    return guard([&] {
        LinOp &a = need_op(A);
        FAMG_REQUIRE(out && ncomponents >= 1 && components, AMG_ERR_INVALID, "need at least one component");
        FAMG_REQUIRE(a.nrows == a.ncols, AMG_ERR_DIM, "Composite needs a square operator");
        auto c = std::make_shared<CompositeOp>();
        c->ctx = a.ctx;
        c->A = A->op;
        c->nrows = c->ncols = a.nrows;
        for (int64_t k = 0; k < ncomponents; k++) {
            LinOp &p = need_op(components[k]);
            FAMG_REQUIRE(p.nrows == a.nrows && p.ncols == a.nrows, AMG_ERR_DIM, "component dims");
            FAMG_REQUIRE(p.ctx == a.ctx, AMG_ERR_INVALID, "component on another context");
            c->comps.push_back(components[k]->op);
        }
        *out = new amg_linop{c};
    });
}

amg_status amg_composite_push(amg_linop *composite, const amg_linop *component) {
    return guard([&] {
        need_op(composite);
        auto c = std::dynamic_pointer_cast<CompositeOp>(composite->op);
        FAMG_REQUIRE(c, AMG_ERR_INVALID, "not a Composite");
        LinOp &p = need_op(component);
        FAMG_REQUIRE(p.nrows == c->nrows && p.ncols == c->nrows, AMG_ERR_DIM, "component dims");
        std::lock_guard<std::mutex> lk(c->mtx);
        c->comps.push_back(component->op);
    });
}

amg_status amg_composite_ncomponents(const amg_linop *composite, int64_t *n) {
    return guard([&] {
        auto *c = dynamic_cast<CompositeOp *>(&need_op(composite));
        FAMG_REQUIRE(c && n, AMG_ERR_INVALID, "not a Composite");
        *n = (int64_t)c->comps.size();
    });
}

amg_status amg_stationary_solve(amg_linop *A, amg_linop *M, const double *b, double *x, int64_t max_iter,
                                double rel_tol, double *hist, int64_t *iters) {
    return guard([&] {
        LinOp &a = need_op(A);
        LinOp &m = need_op(M);
        FAMG_REQUIRE(b && x && iters && max_iter > 0, AMG_ERR_INVALID, "bad argument");
        FAMG_REQUIRE(a.nrows == a.ncols && m.nrows == a.nrows, AMG_ERR_DIM, "solver dims");
        a.ctx->set_device();
        *iters = stationary_impl(single_gpu_ops(a, &m), b, x, max_iter, rel_tol, hist);
    });
}

amg_status amg_pcg_solve(amg_linop *A, amg_linop *M, const double *b, double *x, int64_t max_iter,
                         double rel_tol, double abs_tol, double *hist, int64_t *iters) {
    return guard([&] {
        LinOp &a = need_op(A);
        FAMG_REQUIRE(b && x && iters && max_iter >= 0, AMG_ERR_INVALID, "bad argument");
        LinOp *m = M ? &need_op(M) : nullptr;
        FAMG_REQUIRE(a.nrows == a.ncols && (!m || m->nrows == a.nrows), AMG_ERR_DIM, "solver dims");
        a.ctx->set_device();
        *iters = pcg_impl(single_gpu_ops(a, m), b, x, max_iter, rel_tol, abs_tol, hist);
    });
}

amg_status amg_pcg_solve_block(amg_linop *A, amg_linop *M, const double *B, int64_t ldb, double *X, int64_t ldx,
                               int64_t k, int64_t max_iter, double rel_tol, double abs_tol, double *hist,
                               int64_t ld_hist, int64_t *iters) {
    return guard([&] {
        block_solve_args(B, X, k, hist, ld_hist, max_iter, iters);
        FAMG_REQUIRE(max_iter >= 0, AMG_ERR_INVALID, "block solve: negative max_iter");
        LinOp &a = need_op(A);
        LinOp *m = M ? &need_op(M) : nullptr;
        block_solve_ops(a, m, B, ldb, X, ldx, k);
        if (k == 0) return;
        a.ctx->set_device();
        pcg_block_impl(a, m, B, ldb, X, ldx, k, max_iter, rel_tol, abs_tol, hist, ld_hist, iters);
    });
}

amg_status amg_stationary_solve_block(amg_linop *A, amg_linop *M, const double *B, int64_t ldb, double *X,
                                      int64_t ldx, int64_t k, int64_t max_iter, double rel_tol, double *hist,
                                      int64_t ld_hist, int64_t *iters) {
    return guard([&] {
        block_solve_args(B, X, k, hist, ld_hist, max_iter, iters);
        FAMG_REQUIRE(max_iter > 0, AMG_ERR_INVALID, "block solve: max_iter must be positive");
        LinOp &a = need_op(A);
        LinOp &m = need_op(M);
        block_solve_ops(a, &m, B, ldb, X, ldx, k);
        if (k == 0) return;
        a.ctx->set_device();
        stationary_block_impl(a, m, B, ldb, X, ldx, k, max_iter, rel_tol, hist, ld_hist, iters);
    });
}

amg_status amg_block_cg_solve(amg_linop *A, amg_linop *M, const double *B, int64_t ldb, double *X, int64_t ldx,
                              int64_t k, int64_t max_iter, double rel_tol, double abs_tol, double rank_tol,
                              double *hist, int64_t ld_hist, int64_t *ranks, int64_t *iters) {
    return guard([&] {
        FAMG_REQUIRE(B && X && iters, AMG_ERR_INVALID, "block CG: null B, X or iters");
        FAMG_REQUIRE(k >= 0, AMG_ERR_INVALID, "block CG: negative column count");
        FAMG_REQUIRE(k <= BCG_MAX_W, AMG_ERR_UNSUPPORTED,
                     "block CG: more than 32 columns (the k x k coupling cannot be chunked)");
        FAMG_REQUIRE(max_iter >= 0, AMG_ERR_INVALID, "block CG: negative max_iter");
        FAMG_REQUIRE(!hist || ld_hist >= max_iter, AMG_ERR_INVALID, "block CG: ld_hist below max_iter");
        FAMG_REQUIRE(rank_tol < 1.0, AMG_ERR_INVALID, "block CG: rank_tol must be below 1 (<= 0: the default 2^-26)");
        FAMG_REQUIRE(B != X, AMG_ERR_INVALID, "block CG: B must not alias X");
        LinOp &a = need_op(A);
        LinOp *m = M ? &need_op(M) : nullptr;
        block_solve_ops(a, m, B, ldb, X, ldx, k);
        if (k == 0) return;
        a.ctx->set_device();
        block_cg_impl(a, m, B, ldb, X, ldx, k, max_iter, rel_tol, abs_tol, rank_tol, hist, ld_hist, ranks, iters);
    });
}

amg_status amg_block_gram(amg_ctx *ctx, const double *X, int64_t ldx, int64_t w, const double *Y1, int64_t ld1,
                          int64_t m1, const double *Y2, int64_t ld2, int64_t m2, int64_t n, double *C) {
    return guard([&] {
        FAMG_REQUIRE(X && Y1 && C, AMG_ERR_INVALID, "block gram: null X, Y1 or C");
        FAMG_REQUIRE(w >= 1 && m1 >= 1 && m2 >= 0 && n >= 0, AMG_ERR_INVALID,
                     "block gram: need w >= 1, m1 >= 1, m2 >= 0 and n >= 0");
        FAMG_REQUIRE(w <= BCG_MAX_W && m1 <= BCG_MAX_W && m2 <= BCG_MAX_W, AMG_ERR_UNSUPPORTED,
                     "block gram: more than 32 columns in a block");
        FAMG_REQUIRE(m2 == 0 || Y2, AMG_ERR_INVALID, "block gram: null Y2 with m2 > 0");
        FAMG_REQUIRE(ldx >= n && ld1 >= n && (m2 == 0 || ld2 >= n), AMG_ERR_INVALID,
                     "block gram: leading dimension too small");
        FAMG_REQUIRE(ctx, AMG_ERR_INVALID, "null context");
        ctx->ctx.set_device();
        hipStream_t s = ctx->ctx.stream;
        BcgWork gw;
        gw.reserve(ctx->ctx, n);
        PinnedBuf<double> h(2 * BCG_MAX_W * BCG_MAX_W);
        const int ldc = bcg_gram(X, ldx, w, Y1, ld1, m1, m2 ? Y2 : nullptr, ld2, m2, n, gw, h.p, s);
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
        for (int64_t j = 0; j < m1 + m2; j++)
            for (int64_t i = 0; i < w; i++) C[j * w + i] = h.p[i * ldc + j];
    });
}

amg_status amg_block_gemm_update(amg_ctx *ctx, double *Y, int64_t ldy, const double *X, int64_t ldx, const double *C,
                                 int64_t w, int64_t m, int64_t n, int32_t sign) {
    return guard([&] {
        FAMG_REQUIRE(X && Y && C, AMG_ERR_INVALID, "block gemm update: null Y, X or C");
        FAMG_REQUIRE(w >= 1 && m >= 1 && n >= 0, AMG_ERR_INVALID, "block gemm update: need w >= 1, m >= 1 and n >= 0");
        FAMG_REQUIRE(w <= BCG_MAX_W && m <= BCG_MAX_W, AMG_ERR_UNSUPPORTED,
                     "block gemm update: more than 32 columns in a block");
        FAMG_REQUIRE(sign == 1 || sign == -1, AMG_ERR_INVALID, "block gemm update: sign must be +1 or -1");
        FAMG_REQUIRE(ldx >= n && ldy >= n, AMG_ERR_INVALID, "block gemm update: leading dimension too small");
        if (n > 0) {  // the two blocks' extents must not overlap
            const double *xe = X + (w - 1) * ldx + n, *ye = Y + (m - 1) * ldy + n;
            FAMG_REQUIRE(xe <= Y || ye <= X, AMG_ERR_INVALID, "block gemm update: X must not alias Y");
        }
        FAMG_REQUIRE(ctx, AMG_ERR_INVALID, "null context");
        ctx->ctx.set_device();
        hipStream_t s = ctx->ctx.stream;
        DevBuf<double> cd(BCG_MAX_W * BCG_MAX_W);
        PinnedBuf<double> h(BCG_MAX_W * BCG_MAX_W);
        bcg_pack_coef(C, w, m, h.p);
        FAMG_CHECK_HIP(hipMemcpyAsync(cd.get(), h.p, (size_t)m * 8 * ceil_div(w, 8) * sizeof(double),
                                      hipMemcpyHostToDevice, s));
        bcg_gemm("bcg_update", Y, ldy, Y, ldy, X, ldx, cd.get(), w, m, n, sign, s);
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
    });
}

}  // extern "C"
