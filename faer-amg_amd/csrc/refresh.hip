// refresh.hip -- numeric re-setup of a smoothed-aggregation hierarchy: the same
// sparsity pattern, new matrix values (amg_sa_refresh).
//
// sa_build's patterns are all structural: the tentative P writes `cd` entries per
// row, spgemm keeps every hashed column, the smoothing fix-ups work on given
// patterns and the transpose is a permutation.  A refresh therefore keeps the
// aggregates and every pattern and recomputes only numbers.  The first refresh of
// a hierarchy runs the symbolic passes once (spgemm, transpose) and records the
// patterns of the intermediates and the transpose permutations; later ones run
//  * k_spgemm_refill   C's values on a frozen pattern: no hash table, no rank sort,
//                      no atomics; C's sorted columns staged in LDS and searched
//                      there; 64 / G entries of A's row in flight when B's rows
//                      hold at most G entries (G = 4 for A P with three candidates)
//  * k_transpose_refill  R.val[q] = P.val[perm[q]]
// and the existing fix-ups (k_smooth_fix, k_add_into).  Every C entry starts at
// 0.0 and accumulates fma(a_e, b, acc) in ascending order of the entries e of A's
// row: k_spgemm_numeric's and the CPU oracle's values bit for bit.
#include <algorithm>
#include <chrono>
#include <cstring>

#include "famg.hpp"

namespace famg {

// --------------------------------------------------------- frozen-pattern SpGEMM

// position of column j in the ascending list c[0, n), -1 if absent
template <typename I>
__device__ __forceinline__ I find_col(const int32_t *c, I n, int32_t j) {
    I lo = 0, hi = n;
    while (lo < hi) {
        const I mid = (lo + hi) >> 1;
        if (c[mid] < j) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && c[lo] == j) ? lo : (I)-1;
}

// One wave per C row.  G lanes share an entry e of A's row and take one entry each
// of B's row acol[e] (G < 64: B's rows hold at most G entries, checked; G == 64: the
// lanes stride over B's row), so 64 / G entries of A are loaded and searched at
// once.  Their products then enter the accumulators group by group in ascending e
// with a barrier between groups: within a group the columns are distinct, so each C
// entry's fma chain runs in A's order.  A row of more than CAP columns is searched
// and accumulated in global memory (visible across the wave's lanes after the
// barrier's workgroup fence).  bad: 1 a product column missing from C, 2 a B row
// beyond G -- nothing is stored for such a product.
template <int G, int CAP>
__global__ __launch_bounds__(64) void k_spgemm_refill(const int64_t *__restrict__ arp, const int32_t *__restrict__ acol,
                                                      const double *__restrict__ aval,
                                                      const int64_t *__restrict__ brp, const int32_t *__restrict__ bcol,
                                                      const double *__restrict__ bval, int64_t m,
                                                      const int64_t *__restrict__ crp, const int32_t *__restrict__ ccol,
                                                      double *cval, int *bad) {
    __shared__ int32_t scol[CAP];
    __shared__ double acc[CAP];
    constexpr int T = 64 / G;
    const int lane = threadIdx.x, g = lane / G, lig = lane % G;
    for (int64_t row = blockIdx.x; row < m; row += gridDim.x) {
        const int64_t c0 = crp[row], clen = crp[row + 1] - c0;
        const bool staged = clen <= CAP;
        if (staged) {
            for (int t = lane; t < (int)clen; t += 64) {
                scol[t] = ccol[c0 + t];
                acc[t] = 0.0;
            }
        } else {
            for (int64_t t = lane; t < clen; t += 64) cval[c0 + t] = 0.0;
        }
        __syncthreads();
        const int64_t a0 = arp[row], a1 = arp[row + 1];
        for (int64_t eb = a0; eb < a1; eb += T) {
            if constexpr (G == 64) {
                const int32_t k = acol[eb];
                const double a = aval[eb];
                for (int64_t f = brp[k] + lane; f < brp[k + 1]; f += 64) {
                    const int32_t j = bcol[f];
                    if (staged) {
                        const int p = find_col<int>(scol, (int)clen, j);
                        if (p < 0) *bad = 1;
                        else acc[p] = fma(a, bval[f], acc[p]);
                    } else {
                        const int64_t p = find_col<int64_t>(ccol + c0, clen, j);
                        if (p < 0) *bad = 1;
                        else cval[c0 + p] = fma(a, bval[f], cval[c0 + p]);
                    }
                }
                __syncthreads();
            } else {
                const int64_t e = eb + g;
                int64_t p = -1;
                double a = 0.0, b = 0.0;
                if (e < a1) {
                    const int32_t k = acol[e];
                    const int64_t b0 = brp[k], b1 = brp[k + 1];
                    if (b1 - b0 > G) *bad = 2;
                    else if (b0 + lig < b1) {
                        const int32_t j = bcol[b0 + lig];
                        a = aval[e];
                        b = bval[b0 + lig];
                        p = staged ? (int64_t)find_col<int>(scol, (int)clen, j) : find_col<int64_t>(ccol + c0, clen, j);
                        if (p < 0) *bad = 1;
                    }
                }
                const int groups = (int)(a1 - eb < T ? a1 - eb : T);
                for (int gg = 0; gg < groups; gg++) {
                    if (g == gg && p >= 0) {
                        if (staged) acc[p] = fma(a, b, acc[p]);
                        else cval[c0 + p] = fma(a, b, cval[c0 + p]);
                    }
                    __syncthreads();
                }
            }
        }
        if (staged)
            for (int t = lane; t < (int)clen; t += 64) cval[c0 + t] = acc[t];
        __syncthreads();
    }
}

// out[0] / out[1] = the longest row of the patterns with row pointers rpa (na rows) / rpb (nb rows)
__global__ void k_refill_max_len(const int64_t *rpa, int64_t na, const int64_t *rpb, int64_t nb,
                                 unsigned long long *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long va = i < na ? (unsigned long long)(rpa[i + 1] - rpa[i]) : 0ull;
    unsigned long long vb = i < nb ? (unsigned long long)(rpb[i + 1] - rpb[i]) : 0ull;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long oa = __shfl_xor(va, off), ob = __shfl_xor(vb, off);
        va = va > oa ? va : oa;
        vb = vb > ob ? vb : ob;
    }
    if ((threadIdx.x & 63) == 0) {
        if (va) atomicMax(out, va);
        if (vb) atomicMax(out + 1, vb);
    }
}

constexpr int REFILL_LDS_CAP = 4096;  // columns of a C row staged in LDS (spgemm's own limit of distinct columns)

template <int G, int CAP>
static void launch_refill(const GpuCsr &A, const GpuCsr &B, GpuCsr &C, int *bad, hipStream_t s) {
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(A.nrows, 256 * 32));
    hipLaunchKernelGGL((k_spgemm_refill<G, CAP>), dim3(grid), dim3(64), 0, s, A.rp64.get(), A.col.get(), A.val.get(),
                       B.rp64.get(), B.col.get(), B.val.get(), A.nrows, C.rp64.get(), C.col.get(), C.val.get(), bad);
}

template <int G>
static void launch_refill_cap(int64_t maxc, const GpuCsr &A, const GpuCsr &B, GpuCsr &C, int *bad, hipStream_t s) {
    if (maxc <= 256) launch_refill<G, 256>(A, B, C, bad, s);
    else if (maxc <= 1024) launch_refill<G, 1024>(A, B, C, bad, s);
    else launch_refill<G, REFILL_LDS_CAP>(A, B, C, bad, s);  // longer rows: searched in global memory
}

void spgemm_refill(const GpuCsr &A, const GpuCsr &B, GpuCsr &C) {
    FAMG_REQUIRE(A.ncols == B.nrows, AMG_ERR_DIM, "spgemm_refill: A.ncols != B.nrows");
    FAMG_REQUIRE(C.nrows == A.nrows && C.ncols == B.ncols, AMG_ERR_DIM, "spgemm_refill: C is not A.nrows x B.ncols");
    FAMG_REQUIRE(A.ctx == B.ctx && A.ctx == C.ctx, AMG_ERR_INVALID, "spgemm_refill: operands of different contexts");
    if (!A.nrows) return;
    Ctx &ctx = *A.ctx;
    hipStream_t s = ctx.stream;
    DevBuf<unsigned long long> mx(2);
    DevBuf<int> bad(1);
    FAMG_CHECK_HIP(hipMemsetAsync(mx.get(), 0, 2 * sizeof(unsigned long long), s));
    FAMG_CHECK_HIP(hipMemsetAsync(bad.get(), 0, sizeof(int), s));
    const int64_t rows = std::max(B.nrows, C.nrows);
    hipLaunchKernelGGL(k_refill_max_len, dim3((unsigned)ceil_div(rows, 256)), dim3(256), 0, s, B.rp64.get(), B.nrows,
                       C.rp64.get(), C.nrows, mx.get());
    unsigned long long h[2] = {0, 0};
    FAMG_CHECK_HIP(hipMemcpyAsync(h, mx.get(), sizeof(h), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    const int64_t maxb = (int64_t)h[0], maxc = (int64_t)h[1];
    if (maxb <= 4) launch_refill_cap<4>(maxc, A, B, C, bad.get(), s);
    else if (maxb <= 16) launch_refill_cap<16>(maxc, A, B, C, bad.get(), s);
    else launch_refill_cap<64>(maxc, A, B, C, bad.get(), s);
    FAMG_CHECK_HIP(hipGetLastError());
    int hb = 0;
    FAMG_CHECK_HIP(hipMemcpyAsync(&hb, bad.get(), sizeof(int), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    FAMG_REQUIRE(hb != 2, AMG_ERR_INVALID, "spgemm_refill: a row of B is longer than the measured maximum");
    FAMG_REQUIRE(hb == 0, AMG_ERR_INVALID, "spgemm_refill: a column of the product is missing from C's pattern");
}

// ------------------------------------------------------------- transpose refill

// thread per row i of P: entry e = (i, j) sits in R's row j at column i
__global__ void k_transpose_perm(const int64_t *prp, const int32_t *pcol, int64_t m, const int64_t *rrp,
                                 const int32_t *rcol, int64_t rrows, int32_t *perm, int *bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    for (int64_t e = prp[i]; e < prp[i + 1]; e++) {
        const int64_t j = pcol[e];
        if (j < 0 || j >= rrows) { *bad = 1; continue; }
        const int64_t r0 = rrp[j];
        const int64_t p = find_col<int64_t>(rcol + r0, rrp[j + 1] - r0, (int32_t)i);
        if (p < 0) *bad = 1;
        else perm[r0 + p] = (int32_t)e;
    }
}

__global__ void k_transpose_refill(const double *__restrict__ pval, const int32_t *__restrict__ perm, int64_t nnz,
                                   double *rval, int *bad) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nnz) return;
    const int64_t src = perm[q];
    if (src < 0 || src >= nnz) *bad = 1;
    else rval[q] = pval[src];
}

static void check_flag(DevBuf<int> &bad, hipStream_t s, const char *msg) {
    int h = 0;
    FAMG_CHECK_HIP(hipGetLastError());
    FAMG_CHECK_HIP(hipMemcpyAsync(&h, bad.get(), sizeof(int), hipMemcpyDeviceToHost, s));
    FAMG_CHECK_HIP(hipStreamSynchronize(s));
    FAMG_REQUIRE(h == 0, AMG_ERR_INVALID, msg);
}

void transpose_perm(const GpuCsr &P, const GpuCsr &R, int32_t *perm) {
    FAMG_REQUIRE(R.nrows == P.ncols && R.ncols == P.nrows && R.nnz == P.nnz, AMG_ERR_DIM,
                 "transpose_perm: R does not have the shape of P^T");
    FAMG_REQUIRE(P.nnz < (int64_t(1) << 31), AMG_ERR_UNSUPPORTED, "transpose_perm: nnz >= 2^31");
    hipStream_t s = P.ctx->stream;
    DevBuf<int> bad(1);
    FAMG_CHECK_HIP(hipMemsetAsync(bad.get(), 0, sizeof(int), s));
    // an entry of R no entry of P lands on keeps -1, which the refill refuses
    if (P.nnz) FAMG_CHECK_HIP(hipMemsetAsync(perm, 0xff, P.nnz * sizeof(int32_t), s));
    if (P.nrows)
        hipLaunchKernelGGL(k_transpose_perm, dim3((unsigned)ceil_div(P.nrows, 256)), dim3(256), 0, s, P.rp64.get(),
                           P.col.get(), P.nrows, R.rp64.get(), R.col.get(), R.nrows, perm, bad.get());
    check_flag(bad, s, "transpose_perm: R's pattern is not the transpose of P's");
}

void transpose_refill(const GpuCsr &P, GpuCsr &R, const int32_t *perm) {
    FAMG_REQUIRE(R.nrows == P.ncols && R.ncols == P.nrows && R.nnz == P.nnz, AMG_ERR_DIM,
                 "transpose_refill: R does not have the shape of P^T");
    hipStream_t s = P.ctx->stream;
    DevBuf<int> bad(1);
    FAMG_CHECK_HIP(hipMemsetAsync(bad.get(), 0, sizeof(int), s));
    if (P.nnz)
        hipLaunchKernelGGL(k_transpose_refill, dim3((unsigned)ceil_div(P.nnz, 256)), dim3(256), 0, s, P.val.get(),
                           perm, P.nnz, R.val.get(), bad.get());
    check_flag(bad, s, "transpose_refill: the permutation points outside P");
}

// ------------------------------------------------------------------ the refresh

__global__ void k_pattern_differs(const int64_t *rpa, const int64_t *rpb, int64_t n1, const int32_t *ca,
                                  const int32_t *cb, int64_t nnz, int *bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if ((i < n1 && rpa[i] != rpb[i]) || (i < nnz && ca[i] != cb[i])) *bad = 1;
}

static void require_same_pattern(const GpuCsr &a, const GpuCsr &b) {
    FAMG_REQUIRE(a.nrows == b.nrows && a.ncols == b.ncols && a.nnz == b.nnz, AMG_ERR_INVALID,
                 "sa_refresh: the matrix does not have the shape and entry count of the build's");
    hipStream_t s = a.ctx->stream;
    DevBuf<int> bad(1);
    FAMG_CHECK_HIP(hipMemsetAsync(bad.get(), 0, sizeof(int), s));
    const int64_t work = std::max(a.nrows + 1, a.nnz);
    hipLaunchKernelGGL(k_pattern_differs, dim3((unsigned)ceil_div(work, 256)), dim3(256), 0, s, a.rp64.get(),
                       b.rp64.get(), a.nrows + 1, a.col.get(), b.col.get(), a.nnz, bad.get());
    check_flag(bad, s, "sa_refresh: the matrix's row pointers or column indices differ from the build's");
}

// dst = src's pattern (device copies of rp64 / col), with uninitialised values or none
static void pattern_clone(const GpuCsr &src, GpuCsr &dst, bool with_values) {
    hipStream_t s = src.ctx->stream;
    dst = GpuCsr{};
    dst.ctx = src.ctx;
    dst.nrows = src.nrows;
    dst.ncols = src.ncols;
    dst.nnz = src.nnz;
    dst.rp64.resize(src.nrows + 1);
    dst.col.resize(src.nnz, 4);
    if (with_values) dst.val.resize(src.nnz, 2);
    FAMG_CHECK_HIP(hipMemcpyAsync(dst.rp64.get(), src.rp64.get(), (src.nrows + 1) * sizeof(int64_t),
                                  hipMemcpyDeviceToDevice, s));
    if (src.nnz)
        FAMG_CHECK_HIP(hipMemcpyAsync(dst.col.get(), src.col.get(), src.nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
}

static int64_t pattern_bytes(const GpuCsr &p) { return (int64_t)p.rp64.bytes() + (int64_t)p.col.bytes(); }

// C = A B: on the pattern `frozen` by the refill kernel, or (frozen empty) by spgemm,
// whose pattern is then kept in frozen.  C is not finalized.
static void product(const GpuCsr &A, const GpuCsr &B, GpuCsr &C, GpuCsr &frozen, bool record) {
    if (record) {
        spgemm(A, B, C, false);
        pattern_clone(C, frozen, false);
    } else {
        pattern_clone(frozen, C, true);
        spgemm_refill(A, B, C);
    }
}

static CsrPtr wrap_csr(Ctx *ctx, GpuCsr &&m) {
    auto p = make_csr(ctx);
    p->m = std::move(m);
    p->nrows = p->m.nrows;
    p->ncols = p->m.ncols;
    return p;
}

namespace {
struct StageClock {  // FAMG_SA_LOG=1: stage wall times, the stream drained at every lap
    bool on;
    hipStream_t s;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double lap() {
        if (!on) return 0.0;
        FAMG_CHECK_HIP(hipStreamSynchronize(s));
        const auto t1 = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return ms;
    }
};
}  // namespace

void sa_refresh(MultigridOp &mg, const CsrPtr &A, const double *nn_in, int64_t ld, int64_t k, int64_t *info8) {
    FAMG_REQUIRE(mg.sa_rec, AMG_ERR_UNSUPPORTED, "sa_refresh: only a multigrid that amg_sa_build made keeps its aggregates");
    SaRecord &rec = *mg.sa_rec;
    const SaConfig &cfg = rec.cfg;
    FAMG_REQUIRE(A && nn_in, AMG_ERR_INVALID, "sa_refresh: null argument");
    FAMG_REQUIRE(A->ctx == mg.ctx, AMG_ERR_INVALID, "sa_refresh: the matrix lives on another context");
    FAMG_REQUIRE(k == rec.k, AMG_ERR_INVALID, "sa_refresh: the near-null space must have the build's column count");
    FAMG_REQUIRE(ld >= A->nrows, AMG_ERR_INVALID, "sa_refresh: near-null leading dimension < n");
    Ctx *ctx = mg.ctx;
    const size_t NS = rec.aggs.size();  // coarsening steps
    // the installed operators, in the caller's numbering: their patterns are the frozen ones
    std::vector<CsrPtr> oldA, oldR, oldP;
    {
        std::lock_guard<std::mutex> lk(mg.mtx);
        FAMG_REQUIRE(mg.levels.size() == NS + 1, AMG_ERR_UNSUPPORTED, "sa_refresh: levels were added to the hierarchy");
        for (size_t l = 0; l <= NS; l++) {
            oldA.push_back(std::dynamic_pointer_cast<CsrOp>(mg.levels[l].origA()));
            FAMG_REQUIRE(oldA.back(), AMG_ERR_UNSUPPORTED, "sa_refresh: a level operator is not a CSR matrix");
            if (l == NS) break;
            oldR.push_back(std::dynamic_pointer_cast<CsrOp>(mg.levels[l].origR()));
            oldP.push_back(std::dynamic_pointer_cast<CsrOp>(mg.levels[l].origP()));
            FAMG_REQUIRE(oldR.back() && oldP.back(), AMG_ERR_UNSUPPORTED, "sa_refresh: a transfer is not a CSR matrix");
        }
    }
    if (A != oldA[0]) require_same_pattern(A->m, oldA[0]->m);
    const bool record = !rec.pat;
    std::shared_ptr<SaRefreshPatterns> pat = record ? std::make_shared<SaRefreshPatterns>() : rec.pat;
    if (record) pat->steps.resize(NS);
    const int64_t cd = cfg.candidate_dimension;
    std::vector<LinOpPtr> As{A}, Ss, Rs, Ps;
    int64_t cur_ld = A->nrows;
    std::vector<double> nn(A->nrows * k);
    for (int64_t c = 0; c < k; c++) std::memcpy(nn.data() + c * cur_ld, nn_in + c * ld, A->nrows * sizeof(double));
    static const bool log_on = env_is_one("FAMG_SA_LOG");
    StageClock clk{log_on, ctx->stream};
    CsrPtr cur = A;
    for (size_t l = 0; l < NS; l++) {
        SaRefreshPatterns::Step &st = pat->steps[l];
        const int64_t bs = rec.bss[l], n = cur->nrows, na = rec.naggs[l];
        double ms[5] = {0, 0, 0, 0, 0};  // tentative P, P smoothing, transpose, RAP, coarse near-null
        clk.lap();
        std::vector<double> cnn(na * cd * k);
        CsrPtr P = sa_tentative_block(ctx, n / bs, bs, rec.aggs[l].data(), na, nn.data(), cur_ld, k, cd, cnn.data());
        ms[0] = clk.lap();
        if (record) {
            st.ap.resize(cfg.smoothing_steps);
            st.s.resize(cfg.smoothing_steps);
        }
        for (int64_t q = 0; q < cfg.smoothing_steps; q++) {
            GpuCsr S;
            if (bs == 1) {  // smooth_interpolation: the fix-up in place on A P
                product(cur->m, P->m, S, st.ap[q], record);
                smooth_interp_fixup(S, P->m, cur->diagonal(), 0.66);
            } else {  // block_jacobi_smooth
                CsrPtr Dinv = block_jacobi_dinv(*cur, bs, 0.66);
                GpuCsr AP;
                product(cur->m, P->m, AP, st.ap[q], record);
                product(Dinv->m, AP, S, st.s[q], record);
                csr_add_into(S, P->m);
                csr_finalize(S);
            }
            P = wrap_csr(ctx, std::move(S));
        }
        ms[1] = clk.lap();
        GpuCsr T;
        if (record) {
            transpose(P->m, T);
            FAMG_REQUIRE(P->m.nnz < (int64_t(1) << 31), AMG_ERR_UNSUPPORTED, "sa_refresh: nnz >= 2^31");
            st.perm.resize(P->m.nnz);
            transpose_perm(P->m, T, st.perm.get());
        } else {
            pattern_clone(oldR[l]->m, T, true);
            transpose_refill(P->m, T, st.perm.get());
            csr_finalize(T);
        }
        CsrPtr R = wrap_csr(ctx, std::move(T));
        ms[2] = clk.lap();
        GpuCsr AP, C;
        product(cur->m, P->m, AP, st.rap_ap, record);
        if (record) {
            spgemm(R->m, AP, C, false);
        } else {
            pattern_clone(oldA[l + 1]->m, C, true);
            spgemm_refill(R->m, AP, C);
        }
        csr_finalize(C);
        CsrPtr Ac = wrap_csr(ctx, std::move(C));
        ms[3] = clk.lap();
        nn_postprocess(*Ac, 3, cnn.data(), na * cd, k);
        ms[4] = clk.lap();
        if (clk.on)
            fprintf(stderr,
                    "famg sa refresh level %lld: n %lld aggregates %lld record %d ms: tentative %.3f smoothing %.3f"
                    " transpose %.3f rap %.3f nearnull %.3f\n",
                    (long long)l, (long long)n, (long long)na, record ? 1 : 0, ms[0], ms[1], ms[2], ms[3], ms[4]);
        Rs.push_back(R);
        Ps.push_back(P);
        As.push_back(Ac);
        nn.swap(cnn);
        cur_ld = na * cd;
        cur = Ac;
    }
    for (size_t l = 0; l <= NS; l++) {
        auto M = std::static_pointer_cast<CsrOp>(As[l]);
        if (l == NS) Ss.push_back(make_coarse_chol(*M));
        else Ss.push_back(sa_make_smoother(cfg, M, rec.aggs[l].data(), rec.naggs[l], rec.bss[l]));
    }
    if (clk.on)
        fprintf(stderr, "famg sa refresh smoothers: levels %lld ms: smoothers %.3f\n", (long long)(NS + 1), clk.lap());
    if (record) {
        pat->bytes = 0;
        for (auto &st : pat->steps) {
            for (auto &p : st.ap) pat->bytes += pattern_bytes(p);
            for (auto &p : st.s) pat->bytes += pattern_bytes(p);
            pat->bytes += pattern_bytes(st.rap_ap) + (int64_t)st.perm.bytes();
        }
    }
    FAMG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    // every stage succeeded: commit
    mg.install_operators(As, Ss, Rs, Ps);
    rec.pat = pat;
    if (info8) {
        const int64_t v[8] = {record ? 1 : 0, pat->bytes, (int64_t)NS + 1, (int64_t)NS, 0, 0, 0, 0};
        std::copy(v, v + 8, info8);
    }
}

}  // namespace famg
