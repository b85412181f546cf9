// fine.hip -- the fine level of a box hierarchy whose operator is the constant
// 7-point stencil (C2: A_0 of the 256^3 Laplacian): the cycle's four fine
// launches as TWO marching kernels.
//
// Down (multigrid.rs:341-342 with the first Jacobi step folded): the residual
// from the zero guess r = f - A (d f), the restriction f_c = R r and the next
// level's first step d_c f_c stream f in, r out, r in again, f_c and d_c f_c
// out: 440 MB at 256^3.  k_fine_rr computes r per fine plane in LDS, so r never
// reaches HBM: f in, f_c and d_c f_c out, 172 MB.
//
// Up (multigrid.rs:349-350 and 361-369, the zero-guess step folded):
// v = d f + P v_c, then one Jacobi step z = v + d (f - A v) stream f and v_c
// in, v out, then v and f in again and z out: 704 MB.  k_fine_pj computes v per
// fine plane (with its one-point x/y halo), keeps it in registers and LDS, and
// writes only z: f, v_c and z cross HBM once, 285 MB.
//
// Both march: a workgroup takes an (x, y) tile through a run of jper planes (one
// round of workgroups over the chip), with the planes two steps ahead in
// flight in registers.  Every sum is the unfused kernels' fma chain over the
// same operands (spmv_dia_kernel's constant 7-point RESID0 / JACOBI,
// k_gtc_restrict_march, k_gtc_interp ADD0 with a one-value d), so the results
// are bitwise the four-launch cycle's (test_fine_fused_bitwise).
//
// fine_resid_restrict_ok / fine_interp_jacobi_ok are the whole decision
// (MultigridOp::level_shape asks them): a level that passes launches the
// kernel here, every other level takes the four-launch form.
#include <algorithm>
#include <type_traits>

#include "famg.hpp"

namespace famg {

// A workgroup barrier that orders LDS only: __syncthreads() also waits for every
// outstanding global load, which would drain the next planes' register prefetch
// at each plane step
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Timing experiments only (a library built with -DFAMG_FINE_TIMING, `make TIMING=1`):
// the environment variable FAMG_FINE_DBG, read at every launch, switches parts of
// the fused kernels off -- the results are wrong.  The shipped library has neither
// the variable nor the branches.
#ifdef FAMG_FINE_TIMING
#define FINE_DBG(a, bits) (((a).dbg & (bits)) != 0)
#define FINE_DBG_FIELD int dbg;  // the bits of FAMG_FINE_DBG
#define FINE_DBG_READ(a) (a).dbg = (int)env_int("FAMG_FINE_DBG", 0)
#else
#define FINE_DBG(a, bits) false
#define FINE_DBG_FIELD
#define FINE_DBG_READ(a) (void)0
#endif

typedef double dbl2_t __attribute__((ext_vector_type(2)));
typedef double dbl2u_t __attribute__((ext_vector_type(2), aligned(8)));  // 8-B aligned 16-B loads

// k_fine_rr: r = f - A (d f), f_c = R r and d_c f_c (SETDF) in one marching
// launch.  A workgroup takes a 32 x 8 coarse tile through a run of jper coarse
// planes, walking the fine planes p = 2 Zb - 1 .. 2 Ze once; every coarse row
// adds the entries of its R row that lie in plane p to the fma chain of the
// coarse plane they belong to (p = 2Z - 1, 2Z, 2Z + 1, 2Z + 2: two chains in
// flight per row), complete at p = 2Z + 2.  The work per fine plane:
//   R's terms without value-table lookups or masks: every class's entries lie in
//     the 32 slots (dz, dy, dx) a 2 x 2 x 2 box smoothed by the 7-point stencil
//     reaches (4 at dz = -1, 12 at dz = 0, 12 at dz = 1, 4 at dz = 2), so each
//     class is 32 fp64 weights in LDS (gtc.wt, +0.0 where the class has no
//     entry) and a plane adds 4 or 12 fma terms per chain: an absent slot adds
//     fma(+0.0, r, acc) = acc (r finite, the accumulator never -0.0), so every
//     chain is the class's entries in ascending (dz, dy, dx) order, bitwise
//     k_gtc_restrict_march's; the two chains of a plane interleave;
//   g = d f once per point, when a plane arrives (the seven-point sum is
//     spmv_dia_kernel's fma chain over d x_j): the z neighbours and the centre
//     from the lane's registers (every lane keeps the same 16-B units of the
//     window through the march), only the plane itself in LDS (two slots);
//   windows start at an odd x (2 X0 - 3 for f, 2 X0 - 1 for r), so a coarse
//     row's four r values per (dz, dy) are two aligned 16-B LDS reads;
//   the class ids and d_c codes of the next coarse plane load with the f plane
//     two steps ahead (no LDS staging, no wait of their own).
// Three workgroups per CU.  Even nx: a unit (x, x + 1) with x odd straddles the
// grid only at x = -1 and x = nx - 1, loaded from the clamped pair and shifted.
constexpr int R2_TX = 32, R2_TY = 8;                        // coarse tile
constexpr int R2_UX = R2_TX + 3, R2_UY = 2 * R2_TY + 4;     // f/g window: 35 units x 20 rows (x from 2 X0 - 3, y from 2 Y0 - 2)
constexpr int R2_NU = R2_UX * R2_UY, R2_PU = (R2_NU + 255) / 256;  // 700 units, 3 per lane
constexpr int R2_RX = R2_TX + 1, R2_RY = 2 * R2_TY + 2;     // r window: 33 units x 18 rows (x from 2 X0 - 1, y from 2 Y0 - 1)
constexpr int R2_NR = R2_RX * R2_RY;                        // 594
constexpr int R2_WS = 34;                                   // LDS doubles per class (32 weights, padded against bank repeats)
constexpr int R2_CMAX = 32;                                 // classes (LDS: 8.7 KB)

struct FineRr2Args {
    const uint8_t *cls;  // R's class per coarse row
    const double *wt;    // nclass x 32 weights (the 32-slot pattern)
    int nclass;
    int nx, ny, nz, cx, cy, cz;
    int ntx, nty, jper;
    const double *f;
    double *fc, *dfc;
    const uint8_t *dcc;  // the coarse level's d: codes into dtc, or one value dkc
    const double *dtc;
    double dkc;
    int dmode;  // 0 one value, 1 codes
    double dk;  // the fine level's one-value d
    double cst[7];
    FINE_DBG_FIELD  // 1 skips the R sums, 2 the residual
};

struct Rr2Set {
    dbl2_t F[R2_PU], G[R2_PU];  // f (shifted, 0.0 outside the grid) and d f of one plane at the lane's units
};

__global__ __launch_bounds__(256, 3) void k_fine_rr(FineRr2Args a) {
    __shared__ __attribute__((aligned(16))) double gs[2 * 2 * R2_NU];   // d f of planes p, p + 1
    __shared__ __attribute__((aligned(16))) double rs2[2 * 2 * R2_NR];  // r of planes p, p - 1
    __shared__ double sdt[256];
    extern __shared__ __attribute__((aligned(16))) double sw[];  // the classes' weights, R2_WS per class
    const int tid = threadIdx.x;
    const int t = xcd_remap(blockIdx.x, gridDim.x);
    const int ntxy = a.ntx * a.nty;
    const int chunk = t / ntxy, txy = t - chunk * ntxy;
    const int X0 = (txy % a.ntx) * R2_TX, Y0 = (txy / a.ntx) * R2_TY;
    const int Zb = chunk * a.jper, Ze = min(Zb + a.jper, a.cz);
    const int64_t cpl = (int64_t)a.cx * a.cy, fpl = (int64_t)a.nx * a.ny;
    for (int b = tid; b < a.nclass * 32; b += 256) sw[(b >> 5) * R2_WS + (b & 31)] = a.wt[b];
    if (a.dmode == 1) sdt[tid] = a.dtc[tid];
    // the lane's units: load offset in a plane (32-bit), shift code, residual slot
    int off[R2_PU], ri[R2_PU];
    bool sa[R2_PU], sb[R2_PU], sc[R2_PU], rin[R2_PU], v0[R2_PU], v1[R2_PU];
#pragma unroll
    for (int u = 0; u < R2_PU; u++) {
        const int q = tid + 256 * u, ux = q % R2_UX, uy = q / R2_UX;
        const int x = 2 * X0 - 3 + 2 * ux, y = 2 * Y0 - 2 + uy;
        const bool yin = q < R2_NU && (unsigned)y < (unsigned)a.ny;
        const bool any = yin && x >= -1 && x <= a.nx - 1;
        sa[u] = any && x >= 0 && x + 1 < a.nx;  // both points: (f[x], f[x + 1])
        sb[u] = any && x == a.nx - 1;           // loaded (nx - 2, nx - 1): (.y, 0)
        sc[u] = any && x == -1;                 // loaded (0, 1): (0, .x)
        off[u] = any ? y * a.nx + min(max(x, 0), a.nx - 2) : 0;
        rin[u] = q < R2_NU && ux >= 1 && ux <= R2_RX && uy >= 1 && uy <= R2_RY;
        ri[u] = rin[u] ? (uy - 1) * R2_RX + ux - 1 : 0;
        v0[u] = yin && x >= 0 && x < a.nx;
        v1[u] = yin && x + 1 >= 0 && x + 1 < a.nx;
    }
    // the lane's coarse row
    const int lx = tid % R2_TX, ly = tid / R2_TX, X = X0 + lx, Y = Y0 + ly;
    const bool live = X < a.cx && Y < a.cy;
    const int64_t Jxy = live ? (int64_t)Y * a.cx + X : 0;
    const int p0 = 2 * Zb - 1, p1 = 2 * Ze;
    auto fetch = [&](int p, Rr2Set &S) {
        const double *fz = a.f + (int64_t)min(max(p, 0), a.nz - 1) * fpl;
#pragma unroll
        for (int u = 0; u < R2_PU; u++) S.F[u] = *reinterpret_cast<const dbl2u_t *>(fz + off[u]);
    };
    // class id and d_c code of coarse plane Z (clamped: a plane past the run is never used)
    int ncls = 0, ndc = 0;
    auto fetch_cls = [&](int Z) {
        const int64_t J = (int64_t)min(Z, a.cz - 1) * cpl + Jxy;
        ncls = a.cls[J];
        if (a.dmode == 1) ndc = a.dcc[J];
    };
    // the arrived plane: shift / zero in place, d f beside it
    auto settle = [&](int p, Rr2Set &S) {
        const bool pin = (unsigned)p < (unsigned)a.nz;
#pragma unroll
        for (int u = 0; u < R2_PU; u++) {
            const dbl2_t v = S.F[u];
            const double x0 = sa[u] ? v.x : sb[u] ? v.y : 0.0;
            const double x1 = sa[u] ? v.y : sc[u] ? v.x : 0.0;
            S.F[u] = pin ? dbl2_t{x0, x1} : dbl2_t{0.0, 0.0};
            S.G[u] = a.dk * S.F[u];
        }
    };
    auto publish = [&](int p, const Rr2Set &S) {
        double *g = gs + (p & 1) * 2 * R2_NU;
#pragma unroll
        for (int u = 0; u < R2_PU; u++) {
            const int q = tid + 256 * u;
            if (q < R2_NU) *reinterpret_cast<dbl2_t *>(g + 2 * q) = S.G[u];
        }
    };
    Rr2Set S0, S1, S2, S3;  // plane p0 + k in set k mod 4
    fetch(p0 - 1, S3);
    fetch(p0, S0);
    fetch(p0 + 1, S1);
    fetch_cls(Zb);
    settle(p0 - 1, S3);
    settle(p0, S0);
    publish(p0, S0);
    fetch(p0 + 2, S2);
    __syncthreads();

    double acc[2] = {0.0, 0.0};
    int cb[2] = {0, 0}, dq[2] = {0, 0};  // per chain: its class's weights in sw, its d_c code
    // step p: Sm = plane p - 1 (its G), S0 = p, S1 = p + 1 (arrived), S3 = p + 3 (issued here; the set of p - 1)
    auto step = [&](int p, Rr2Set &Sm, Rr2Set &Sp, Rr2Set &S1p, Rr2Set &S3p, auto ph) {
        constexpr int PH = decltype(ph)::value;
        constexpr int sn = (PH >> 1) & 1, so = sn ^ 1, gn = PH & 1, go = 2 + (PH & 1);
        settle(p + 1, S1p);
        publish(p + 1, S1p);  // the slot of p - 1: its in-plane reads ended before the last barrier
        const double *g0 = gs + (p & 1) * 2 * R2_NU;
        double *rp = rs2 + (p & 1) * 2 * R2_NR;
        const bool pin = (unsigned)p < (unsigned)a.nz;
#pragma unroll
        for (int u = 0; u < R2_PU; u++) {
            if (!rin[u] || FINE_DBG(a, 2)) continue;
            const int q = tid + 256 * u;
            const dbl2_t ym = *reinterpret_cast<const dbl2_t *>(g0 + 2 * (q - R2_UX));
            const dbl2_t yp = *reinterpret_cast<const dbl2_t *>(g0 + 2 * (q + R2_UX));
            const double xl = g0[2 * q - 1], xr = g0[2 * q + 2];
            const dbl2_t gm = Sm.G[u], gc = Sp.G[u], gp = S1p.G[u];
            const double y0[7] = {gm.x, ym.x, xl, gc.x, gc.y, yp.x, gp.x};
            const double y1[7] = {gm.y, ym.y, gc.x, gc.y, xr, yp.y, gp.y};
            double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
            for (int k = 0; k < 7; k++) {
                acc0 = fma(a.cst[k], y0[k], acc0);
                acc1 = fma(a.cst[k], y1[k], acc1);
            }
            const dbl2_t b = Sp.F[u];
            *reinterpret_cast<dbl2_t *>(rp + 2 * ri[u]) =
                dbl2_t{pin && v0[u] ? b.x - acc0 : 0.0, pin && v1[u] ? b.y - acc1 : 0.0};
        }
        fetch(min(p + 3, p1 + 1), S3p);  // in flight two planes
        const int Zn = (p + 1) >> 1, Zo = Zn - 1;
        const bool nl = Zn < Ze, ol = Zo >= Zb;
        if (gn == 0 && nl) {  // chain n starts: its class (loaded two steps ago); the next one's load
            cb[sn] = ncls * R2_WS;
            dq[sn] = ndc;
            acc[sn] = 0.0;
            fetch_cls(Zn + 1);
        }
        lds_barrier();
        if (!live || FINE_DBG(a, 1)) return;
        // r(p) at the 4 x 4 positions (dy, dx) in -1..2 of the anchor (2X, 2Y): units lx, lx + 1 of rows 2 ly + dy
        double w[16];
#pragma unroll
        for (int dy = 0; dy < 4; dy++) {
            const double *rr = rp + 2 * ((2 * ly + dy) * R2_RX + lx);
            const dbl2_t m0 = *reinterpret_cast<const dbl2_t *>(rr);
            const dbl2_t m1 = *reinterpret_cast<const dbl2_t *>(rr + 2);
            w[4 * dy + 0] = m0.x;
            w[4 * dy + 1] = m0.y;
            w[4 * dy + 2] = m1.x;
            w[4 * dy + 3] = m1.y;
        }
        // the slots of a plane group: 4 (dz = -1, 2) or 12 (dz = 0, 1), as w indices
        constexpr int P4[4] = {5, 6, 9, 10};
        constexpr int P12[12] = {1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14};
        constexpr int NN = (gn == 0) ? 4 : 12, NO = (go == 3) ? 4 : 12;
        constexpr int ON = (gn == 0) ? 0 : 4, OO = (go == 2) ? 16 : 28;
        double wn[NN], wo[NO];
        if (nl) {
#pragma unroll
            for (int k = 0; k < NN; k += 2) {
                const dbl2_t v = *reinterpret_cast<const dbl2_t *>(sw + cb[sn] + ON + k);
                wn[k] = v.x;
                wn[k + 1] = v.y;
            }
        }
        if (ol) {
#pragma unroll
            for (int k = 0; k < NO; k += 2) {
                const dbl2_t v = *reinterpret_cast<const dbl2_t *>(sw + cb[so] + OO + k);
                wo[k] = v.x;
                wo[k + 1] = v.y;
            }
        }
        double an = acc[sn], ao = acc[so];
#pragma unroll
        for (int k = 0; k < 12; k++) {
            if (nl && k < NN) an = fma(wn[k], w[NN == 4 ? P4[k % 4] : P12[k]], an);
            if (ol && k < NO) ao = fma(wo[k], w[NO == 4 ? P4[k % 4] : P12[k]], ao);
        }
        acc[sn] = an;
        acc[so] = ao;
        if (go == 3 && ol) {
            const int64_t J = (int64_t)Zo * cpl + Jxy;
            a.fc[J] = ao;
            const double dd = a.dmode == 0 ? a.dkc : sdt[dq[so]];
            a.dfc[J] = dd * ao;  // vec_mul(_coded)'s product
        }
    };
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    using P2 = std::integral_constant<int, 2>;
    using P3 = std::integral_constant<int, 3>;
    int p = p0;
    for (; p + 3 <= p1; p += 4) {
        step(p, S3, S0, S1, S3, P0{});
        step(p + 1, S0, S1, S2, S0, P1{});
        step(p + 2, S1, S2, S3, S1, P2{});
        step(p + 3, S2, S3, S0, S2, P3{});
    }
    if (p < p1) {
        step(p, S3, S0, S1, S3, P0{});
        step(p + 1, S0, S1, S2, S0, P1{});
    }
}

// k_fine_pj: v = d f + P v_c, then z = v + d (f - A v), in one marching launch.
// A workgroup of 1024 lanes takes a 256 x 16 fine (x, y) tile through a run of
// jper planes; the coarse planes P reads sit in an LDS ring of four slots.  It
// works on 16-B units -- two x-adjacent fine points, x even, in one box, so one
// coarse window anchor -- the way k_fine_rr cuts its plane work:
//   per lane three units of the 68 x 18 v window (x from x0 - 2, y from y0 - 1):
//     f and the two class bytes of a unit in one load each (16 B, 2 B);
//   v of planes z - 1, z, z + 1 stay in the lane's registers (the Jacobi sum's
//     z neighbours and centre), only plane z in LDS for the in-plane neighbours
//     (two slots);
//   P's dictionary decoded per class: its KE = 4 fp64 weights (two 16-B LDS
//     reads) and, per coarse-ring phase, its four coarse-window offsets (one
//     8-B read) -- the fma chain over the KE entries in dictionary order, padding
//     +0.0 terms included, is k_gtc_interp's ADD0 sum;
//   the output tile's 512 units as 16-B stores.
// Bitwise the two launches it replaces (test_fine_fused_bitwise).  Even nx.
constexpr int J2_NT = 1024;                                 // threads per workgroup
constexpr int J2_TX = 256, J2_TY = 16;                      // fine tile (x, y): whole grid rows at 256^3
constexpr int J2_UX = J2_TX / 2 + 2, J2_UY = J2_TY + 2;     // v window: 130 units x 18 rows
constexpr int J2_NU = J2_UX * J2_UY, J2_PU = (J2_NU + J2_NT - 1) / J2_NT;  // 2340 units, 3 per lane
constexpr int J2_CX = J2_TX / 2 + 4, J2_CY = J2_TY / 2 + 4, J2_CPL = J2_CX * J2_CY;  // coarse window 132 x 12
constexpr int J2_CPF = (J2_CPL + J2_NT - 1) / J2_NT;        // coarse points per lane (2)
constexpr int J2_CMAX = 128;                                // classes

struct FinePj2Args {
    const uint8_t *cls;    // P's class id per fine row
    const uint16_t *dict;  // nclass x 4 entries: value index << 8 | slot
    const double *vtab;
    int nclass;
    int nx, ny, nz, cx, cy, cz;
    int ntx, nty, jper;
    const double *vc;  // coarse correction v_c
    const double *f;   // fine rhs
    double *out;       // z
    double dk;
    double cst[7];
    FINE_DBG_FIELD  // 1 no stores, 2 no P sums, 4 no Jacobi sums
};

struct Pj2Set {
    dbl2_t F[J2_PU], V[J2_PU];
    int C[J2_PU];  // the unit's two class bytes (x even: low byte)
};

__global__ __launch_bounds__(J2_NT) void k_fine_pj(FinePj2Args a) {
    __shared__ __attribute__((aligned(16))) double vr[2 * 2 * J2_NU];  // v of planes z, z + 1
    __shared__ double cring[4 * J2_CPL];
    __shared__ __attribute__((aligned(16))) double pw[J2_CMAX * 4];    // per class its 4 weights
    __shared__ __attribute__((aligned(8))) int16_t po[4 * J2_CMAX * 4];  // per ring phase and class: 4 offsets
    const int tid = threadIdx.x;
    const int t = xcd_remap(blockIdx.x, gridDim.x);
    const int ntxy = a.ntx * a.nty;
    const int chunk = t / ntxy, txy = t - chunk * ntxy;
    const int x0 = (txy % a.ntx) * J2_TX, y0 = (txy / a.ntx) * J2_TY;
    const int zb = chunk * a.jper, ze = min(zb + a.jper, a.nz);
    const int cwx0 = (x0 >> 1) - 2, cwy0 = (y0 >> 1) - 2;
    const int64_t fpl = (int64_t)a.nx * a.ny;
    for (int b = tid; b < 4 * a.nclass; b += J2_NT) {
        const uint32_t e = a.dict[b], sl = e & 255u;
        pw[b] = a.vtab[e >> 8];
        const int dzs = (int)(sl / 9u) - 1, dys = (int)((sl / 3u) % 3u) - 1, dxs = (int)(sl % 3u) - 1;
#pragma unroll
        for (int r = 0; r < 4; r++) po[r * 4 * a.nclass + b] = (int16_t)(((r + dzs) & 3) * J2_CPL + dys * J2_CX + dxs);
    }
    // the lane's units: plane offset (32-bit, an in-grid unit for units outside),
    // coarse anchor, whether in the grid / in the output tile
    int off[J2_PU], cb[J2_PU];
    bool inq[J2_PU], jac[J2_PU];
#pragma unroll
    for (int u = 0; u < J2_PU; u++) {
        const int q = tid + J2_NT * u, ux = q % J2_UX, uy = q / J2_UX;
        const int x = x0 - 2 + 2 * ux, y = y0 - 1 + uy;
        inq[u] = q < J2_NU && (unsigned)x < (unsigned)a.nx && (unsigned)y < (unsigned)a.ny;
        jac[u] = inq[u] && ux >= 1 && ux <= J2_TX / 2 && uy >= 1 && uy <= J2_TY;
        off[u] = inq[u] ? y * a.nx + x : 0;
        cb[u] = inq[u] ? ((y >> 1) - cwy0) * J2_CX + (x >> 1) - cwx0 : J2_CX + 1;
    }
    auto fetch = [&](int z, Pj2Set &S) {
        const int zc = min(max(z, 0), a.nz - 1);
        const double *fz = a.f + (int64_t)zc * fpl;
        const uint8_t *cz = a.cls + (int64_t)zc * fpl;
#pragma unroll
        for (int u = 0; u < J2_PU; u++) {
            S.F[u] = *reinterpret_cast<const dbl2_t *>(fz + off[u]);
            S.C[u] = (int)*reinterpret_cast<const uint16_t *>(cz + off[u]);
        }
    };
    auto cfetch = [&](int Z, double (&v)[J2_CPF]) {
        const int64_t cpl = (int64_t)a.cx * a.cy;
#pragma unroll
        for (int u = 0; u < J2_CPF; u++) {
            const int p = tid + J2_NT * u;
            const int X = cwx0 + p % J2_CX, Y = cwy0 + p / J2_CX;
            const bool in = p < J2_CPL && (unsigned)X < (unsigned)a.cx && (unsigned)Y < (unsigned)a.cy &&
                            (unsigned)Z < (unsigned)a.cz;
            v[u] = a.vc[in ? (int64_t)Z * cpl + (int64_t)Y * a.cx + X : 0];
        }
    };
    auto cstore = [&](int Z, const double (&v)[J2_CPF]) {
#pragma unroll
        for (int u = 0; u < J2_CPF; u++) {
            const int p = tid + J2_NT * u;
            const int X = cwx0 + p % J2_CX, Y = cwy0 + p / J2_CX;
            const bool in = (unsigned)X < (unsigned)a.cx && (unsigned)Y < (unsigned)a.cy && (unsigned)Z < (unsigned)a.cz;
            if (p < J2_CPL) cring[(Z & 3) * J2_CPL + p] = in ? v[u] : 0.0;
        }
    };
    // v = d f + P v_c of plane z at the lane's units (0.0 outside the grid)
    auto interp = [&](int z, Pj2Set &S) {
        const bool zin = (unsigned)z < (unsigned)a.nz;
        const int16_t *pz = po + ((z >> 1) & 3) * 4 * a.nclass;
#pragma unroll
        for (int u = 0; u < J2_PU; u++) {
            double vv[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int c = (S.C[u] >> (8 * h)) & 255;
                const dbl2_t w01 = *reinterpret_cast<const dbl2_t *>(pw + 4 * c);
                const dbl2_t w23 = *reinterpret_cast<const dbl2_t *>(pw + 4 * c + 2);
                const uint2 oo = *reinterpret_cast<const uint2 *>(pz + 4 * c);
                const int o0 = (int)(int16_t)(oo.x & 0xffffu), o1 = (int)(int16_t)(oo.x >> 16);
                const int o2 = (int)(int16_t)(oo.y & 0xffffu), o3 = (int)(int16_t)(oo.y >> 16);
                double acc = 0.0;
                if (!FINE_DBG(a, 2)) {
                    acc = fma(w01.x, cring[cb[u] + o0], acc);
                    acc = fma(w01.y, cring[cb[u] + o1], acc);
                    acc = fma(w23.x, cring[cb[u] + o2], acc);
                    acc = fma(w23.y, cring[cb[u] + o3], acc);
                }
                const double fv = h ? S.F[u].y : S.F[u].x;
                vv[h] = (zin && inq[u]) ? a.dk * fv + acc : 0.0;  // d*b (vec_mul's product) + P v_c
            }
            S.V[u] = dbl2_t{vv[0], vv[1]};
        }
    };
    auto publish = [&](int z, const Pj2Set &S) {
        double *g = vr + (z & 1) * 2 * J2_NU;
#pragma unroll
        for (int u = 0; u < J2_PU; u++) {
            const int q = tid + J2_NT * u;
            if (q < J2_NU) *reinterpret_cast<dbl2_t *>(g + 2 * q) = S.V[u];
        }
    };
    // coarse planes zb/2 - 2 .. zb/2 + 1 (those of v(zb - 1) .. v(zb + 1); zb is even)
    const int Zb = zb >> 1;
    {
        double cv[J2_CPF];
        for (int Z = Zb - 2; Z <= Zb + 1; Z++) {
            cfetch(Z, cv);
            cstore(Z, cv);
        }
    }
    Pj2Set S0, S1, S2, S3;  // plane zb + k in set k mod 4
    fetch(zb - 1, S3);
    fetch(zb, S0);
    fetch(zb + 1, S1);
    __syncthreads();
    interp(zb - 1, S3);
    interp(zb, S0);
    publish(zb, S0);
    int cmax = Zb + 2;
    double cp[J2_CPF];
    cfetch(cmax, cp);
    fetch(zb + 2, S2);
    __syncthreads();

    // step z: Sm = z - 1 (its V), Sz = z, S1 = z + 1 (f arrived: its v now), S3 = z + 3 (issued; the set of z - 1)
    auto step = [&](int z, Pj2Set &Sm, Pj2Set &Sz, Pj2Set &S1, Pj2Set &S3) {
        interp(z + 1, S1);
        publish(z + 1, S1);  // the slot of z - 1: its in-plane reads ended before the last barrier
        // z(z) = v + d (f - A v): spmv_dia_kernel's constant 7-point JACOBI sum
        const double *v0 = vr + (z & 1) * 2 * J2_NU;
        const bool zon = z < ze;
        double *oz = a.out + (int64_t)min(z, a.nz - 1) * fpl;
#pragma unroll
        for (int u = 0; u < J2_PU; u++) {
            if (!jac[u] || !zon || FINE_DBG(a, 1)) continue;
            const int q = tid + J2_NT * u;
            if (FINE_DBG(a, 4)) {
                *reinterpret_cast<dbl2_t *>(oz + off[u]) = Sz.V[u];
                continue;
            }
            const dbl2_t ym = *reinterpret_cast<const dbl2_t *>(v0 + 2 * (q - J2_UX));
            const dbl2_t yp = *reinterpret_cast<const dbl2_t *>(v0 + 2 * (q + J2_UX));
            const double xl = v0[2 * q - 1], xr = v0[2 * q + 2];
            const dbl2_t vm = Sm.V[u], vc = Sz.V[u], vp = S1.V[u];
            const double y0[7] = {vm.x, ym.x, xl, vc.x, vc.y, yp.x, vp.x};
            const double y1[7] = {vm.y, ym.y, vc.x, vc.y, xr, yp.y, vp.y};
            double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
            for (int k = 0; k < 7; k++) {
                acc0 = fma(a.cst[k], y0[k], acc0);
                acc1 = fma(a.cst[k], y1[k], acc1);
            }
            const dbl2_t fz = Sz.F[u];
            // streamed out (nontemporal: z is read by the next solve step, not by this cycle)
            __builtin_nontemporal_store(dbl2_t{vc.x + a.dk * (fz.x - acc0), vc.y + a.dk * (fz.y - acc1)},
                                        reinterpret_cast<dbl2_t *>(oz + off[u]));
        }
        cstore(cmax, cp);  // the coarse plane v(z + 2) adds (slot of cmax - 4: unread)
        cmax = ((z + 3) >> 1) + 1;
        cfetch(cmax, cp);
        fetch(min(z + 3, ze), S3);
        lds_barrier();
    };
    for (int z = zb; z < ze; z += 4) {
        step(z, S3, S0, S1, S3);
        step(z + 1, S0, S1, S2, S0);
        step(z + 2, S1, S2, S3, S1);
        step(z + 3, S2, S3, S0, S2);
    }
}

// ------------------------------------------------------------ host side

bool fine_resid_restrict_ok(const GpuCsr &A, const GpuCsr &R, const SpmvEpi &epi, const SpmvEpi &epic) {
    if (flag(FLAG_FINE_FUSE) == 0 || !dia7_cst_dk(A, epi)) return false;
    if (!R.gtc.built() || !R.gtc.r || R.rframe.on() || R.cframe.on() || R.gtc.ntab > 256) return false;
    // k_fine_rr: every class in the 32-slot pattern (gtc.wt), the classes' weights in
    // LDS, 32-bit offsets within a fine plane
    if (!R.gtc.wt.get() || R.gtc.nclass > R2_CMAX || R.gtc.fg[0] * R.gtc.fg[1] >= (int64_t(1) << 31)) return false;
    // the coarse level's d coded (8-bit) or one value: no global load in the plane loop
    if (!epic.y2 || !epic.dc) return false;
    for (int q = 0; q < 3; q++)
        if (R.gtc.fg[q] != A.dia.cst_n[q] || R.gtc.cg[q] != (R.gtc.fg[q] + 1) / 2) return false;
    // even nx: the 16-B units of a window row never straddle the end of a grid row
    // except where the kernels shift them (an odd nx runs the unfused launches)
    if (R.gtc.fg[0] % 2 != 0) return false;
    return A.nrows == R.ncols && R.nrows == R.gtc.cg[0] * R.gtc.cg[1] * R.gtc.cg[2];
}

void fine_resid_restrict(const GpuCsr &A, const GpuCsr &R, const double *f, double dk, double *fc,
                         const SpmvEpi &epic, hipStream_t s) {
    FineRr2Args a{};
    a.cls = R.gtc.cls.get();
    a.wt = R.gtc.wt.get();
    a.nclass = R.gtc.nclass;
    a.nx = (int)R.gtc.fg[0]; a.ny = (int)R.gtc.fg[1]; a.nz = (int)R.gtc.fg[2];
    a.cx = (int)R.gtc.cg[0]; a.cy = (int)R.gtc.cg[1]; a.cz = (int)R.gtc.cg[2];
    a.ntx = (int)ceil_div(a.cx, R2_TX);
    a.nty = (int)ceil_div(a.cy, R2_TY);
    a.f = f;
    a.fc = fc;
    a.dfc = epic.y2;
    // the coarse level's d as the SETDF epilogue reads it (k_gtc_restrict_march)
    if (epic.dc && epic.dk != 0.0 && flag(FLAG_DIA_DK) != 0) {
        a.dmode = 0;
        a.dkc = epic.dk;
    } else {
        a.dmode = 1;
        a.dcc = epic.dc;
        a.dtc = epic.dt;
    }
    a.dk = dk;
    for (int k = 0; k < 7; k++) a.cst[k] = A.dia.cst_v[k];
    FINE_DBG_READ(a);
    const int64_t ntxy = (int64_t)a.ntx * a.nty;
    // occupancy at a typical run length, then the run length for one round of workgroups
    const size_t dyn = (size_t)8 * R2_WS * a.nclass;
    const int per_cu = kernel_occupancy(reinterpret_cast<const void *>(k_fine_rr), 256, dyn);
    const int64_t want = (int64_t)per_cu * std::max(A.ctx ? A.ctx->num_cus : 256, 1);
    a.jper = (int)std::max<int64_t>(1, ceil_div((int64_t)a.cz * ntxy, want));
    if (flag(FLAG_FINE_FUSE) > 1) a.jper = (int)std::max<int64_t>(1, flag(FLAG_FINE_FUSE) / 2);
    const dim3 grid((unsigned)(ntxy * ceil_div(a.cz, a.jper)));
    k_fine_rr<<<grid, dim3(256), dyn, s>>>(a);
    FAMG_CHECK_HIP(hipGetLastError());
    const int64_t n = A.nrows, nc = R.nrows;
    // f in once, f_c and d_c f_c out, R's class ids (1 B per coarse row; a coded d_c: 1 B more);
    // CSR-equivalent: A's RESID0 (x, b = f; r out; d gathered) + R's SETDF
    log_launch("fine-rr", SPMV_KERNEL_DIA, -1, n, 8 * n + 16 * nc + nc + (a.dmode == 1 ? nc : 0),
               (12 * A.nnz + 4 * (n + 1) + 32 * n) + (12 * R.nnz + 4 * (nc + 1) + 8 * n + 16 * nc));
}

bool fine_interp_jacobi_ok(const GpuCsr &A, const GpuCsr &P, const SpmvEpi &epi) {
    if (flag(FLAG_FINE_FUSE) == 0 || !dia7_cst_dk(A, epi)) return false;
    if (!P.gtc.built() || P.gtc.r || P.rframe.on() || P.cframe.on() || P.gtc.ntab > 256) return false;
    // k_fine_pj: four entries per class, the classes' tables in LDS, 32-bit offsets
    // within a fine plane
    if (P.gtc.ke != 4 || P.gtc.nclass > J2_CMAX || P.gtc.fg[0] * P.gtc.fg[1] >= (int64_t(1) << 31)) return false;
    for (int q = 0; q < 3; q++)
        if (P.gtc.fg[q] != A.dia.cst_n[q] || P.gtc.cg[q] != (P.gtc.fg[q] + 1) / 2) return false;
    if (P.gtc.fg[0] % 2 != 0) return false;  // even nx (16-B units of two points in one box)
    return A.nrows == P.nrows && P.ncols == P.gtc.cg[0] * P.gtc.cg[1] * P.gtc.cg[2];
}

void fine_interp_jacobi(const GpuCsr &A, const GpuCsr &P, const double *vc, const double *f, double dk, double *out,
                        hipStream_t s) {
    FinePj2Args a{};
    a.cls = P.gtc.cls.get();
    a.dict = P.gtc.dict.get();
    a.vtab = P.gtc.vtab.get();
    a.nclass = P.gtc.nclass;
    a.nx = (int)P.gtc.fg[0]; a.ny = (int)P.gtc.fg[1]; a.nz = (int)P.gtc.fg[2];
    a.cx = (int)P.gtc.cg[0]; a.cy = (int)P.gtc.cg[1]; a.cz = (int)P.gtc.cg[2];
    a.ntx = (int)ceil_div(a.nx, J2_TX);
    a.nty = (int)ceil_div(a.ny, J2_TY);
    a.vc = vc;
    a.f = f;
    a.out = out;
    a.dk = dk;
    for (int k = 0; k < 7; k++) a.cst[k] = A.dia.cst_v[k];
    FINE_DBG_READ(a);
    const int64_t ntxy = (int64_t)a.ntx * a.nty;
    // one round of workgroups over the chip; an even run of planes per workgroup
    const int per_cu = kernel_occupancy(reinterpret_cast<const void *>(k_fine_pj), J2_NT, 0);
    const int64_t want = (int64_t)per_cu * std::max(A.ctx ? A.ctx->num_cus : 256, 1);
    int jper = (int)std::max<int64_t>(2, ceil_div((int64_t)a.nz * ntxy, want));
    if (flag(FLAG_FINE_FUSE) > 1) jper = (int)flag(FLAG_FINE_FUSE);
    a.jper = jper + (jper & 1);
    const dim3 grid((unsigned)(ntxy * ceil_div(a.nz, a.jper)));
    k_fine_pj<<<grid, dim3(J2_NT), 0, s>>>(a);
    FAMG_CHECK_HIP(hipGetLastError());
    const int64_t n = A.nrows;
    // f and z once, v_c once, the class ids (1 B per row); CSR-equivalent: P's ADD0 + A's JACOBI
    log_launch("fine-pj", SPMV_KERNEL_DIA, -1, n, 8 * n + 8 * P.ncols + 8 * n + n,
               (12 * P.nnz + 4 * (n + 1) + 8 * P.ncols + 16 * n) + (12 * A.nnz + 4 * (n + 1) + 32 * n));
}

}  // namespace famg
