// gpu_csr.hpp -- a CSR matrix on the device and the state of its SpMV storages.
//
// Each storage format is one struct, a member of GpuCsr.  Its default member
// initialisers are the "not built" state, so dropping a storage (and freeing its
// HBM) is the assignment m.x = {}; csr_finalize resets all of them before it
// builds what the matrix takes.
#pragma once

#include <vector>

#include "common.hpp"

namespace famg {

// Plane layout of a rank-local vector of a distributed grid level (dist.hip,
// DESIGN.md 6): the rank owns planes [z0, z0 + nz) of an nx x ny x gz grid
// (local entries [0, nz * pl)), then its ghost planes -- gl whole planes below z0,
// then gh above z0 + nz.  Local plane z in [-gl, nz + gh) starts at entry
// z * pl + (z < 0 ? nz * pl + gl * pl : z >= nz ? gl * pl : 0).
// Off (nx == 0) for single-GPU matrices; a redundant (all-gathered) level is
// the frame with z0 = 0, nz = gz and no ghosts.
struct SlabFrame {
    int64_t nx = 0, ny = 0, gz = 0;  // the global grid
    int64_t z0 = 0, nz = 0;          // owned planes
    int64_t gl = 0, gh = 0;          // ghost planes below / above
    bool on() const { return nx > 0; }
    int64_t pl() const { return nx * ny; }
    int64_t n_own() const { return nz * nx * ny; }
    int64_t add_lo() const { return (nz + gl) * nx * ny; }  // added to z * pl for z < 0
    int64_t add_hi() const { return gl * nx * ny; }         // ... for z >= nz
    // global grid plane of a local entry (ghosts included)
    int64_t plane_of(int64_t c) const {
        const int64_t p = pl(), own = n_own();
        if (c < own) return z0 + c / p;
        const int64_t g = c - own;
        return g < gl * p ? z0 - gl + g / p : z0 + nz + (g - gl * p) / p;
    }
    int64_t in_plane(int64_t c) const {
        const int64_t p = pl(), own = n_own();
        return c < own ? c % p : (c - own) % p;
    }
};

enum SpmvKernel : int {
    SPMV_KERNEL_STREAM = 0, SPMV_KERNEL_SELL = 1, SPMV_KERNEL_VECTOR = 2, SPMV_KERNEL_DIA = 3, SPMV_KERNEL_BSR = 4,
    SPMV_KERNEL_SELLP = 5, SPMV_KERNEL_SCS = 6, SPMV_KERNEL_XS = 7, SPMV_KERNEL_GTC = 8
};

// SELL-64 copy with compressed column indices (sell.hip):
// slice s holds rows [row0[s], row0[s+1]) (<= 64), one lane per row,
// soff[s+1]-soff[s] entry steps; desc[s] = byte offset/128 of its block in
// data | column mode << 30; base = one int32 per step.
struct SellStore {
    DevBuf<int32_t> row0;
    DevBuf<int32_t> soff;
    DevBuf<uint32_t> desc;
    DevBuf<int32_t> base;
    DevBuf<char> data;
    int64_t nslices = 0, steps = 0, bytes = 0;
    int64_t mode_slices[3] = {0, 0, 0};  // slices per column mode (implicit, u16, i32)
    std::vector<int64_t> seg_slc;        // slices of row segment g: [seg_slc[g], seg_slc[g+1])
    bool paired = true;     // step-pair layout (16-B value loads); false: one step per 512-B row
    bool is_short = false;  // coded slices of <= 4 steps in equal pairs (spmv_sell_short_kernel)
    // value codes (sell.hip "value codes"): 0 = fp64 values, else 4/8/16-bit codes
    // into vtab (ntab distinct bit patterns, ascending)
    int vbits = 0;
    int64_t ntab = 0;
    DevBuf<double> vtab;
    bool built() const { return desc.get() != nullptr; }
    int64_t stream_bytes() const { return bytes + 12 * (nslices + 1) + 4 * steps + 8 * ntab; }
};

// DIA codes (dia.hip): cw words of codes per row for the k diagonals off
// (ascending), into the value table vtab
struct DiaStore {
    DevBuf<uint32_t> codes;
    DevBuf<double> vtab;
    int64_t ntab = 0;
    int k = 0, cw = 0, vbits = 0;
    int pat = 0;  // > 32 diagonals: the run pattern (spmv_dia_pat_kernel)
    // 7- or 27-point DIA operator whose every row is the interior stencil truncated
    // at the grid faces (dia_constant): the kernels read no codes
    bool cst = false;
    int cst_n[3] = {0, 0, 0};
    double cst_v[27] = {0};
    std::vector<int> off;
    // row range: the whole matrix (kernel == DIA) or one row segment (seg, e.g.
    // the halo interior of a distributed level) beside SELL
    int64_t r0 = 0, r1 = 0, seg = 0;
    // set when the codes describe a color-permuted SGS copy: stored row p is
    // original row rowid[p] (device array owned by the SgsOp)
    const int32_t *rowid = nullptr;
    bool built() const { return codes.get() != nullptr; }
    int64_t stream_bytes(int64_t nrows) const {
        return cst ? 8 * (int64_t)k : 4 * cw * nrows + 8 * ntab;  // constant: no codes
    }
};

// wave-per-row storage compression (spmv.hip): 8/16-bit value codes (codes, table
// vtab) and 16-bit column offsets from the row (off); the kernel reads the CSR
// arrays for whatever is not compressed
struct VecStore {
    DevBuf<uint8_t> codes;
    DevBuf<int16_t> off;
    DevBuf<double> vtab;
    int64_t ntab = 0;
    int vbits = 0;
    bool o16 = false;
    int wpr = 1;  // waves per row, chosen once for the whole matrix (flag FLAG_VEC_WPR overrides)
    bool built() const { return codes.get() != nullptr || off.get() != nullptr; }
    int64_t stream_bytes(int64_t nrows, int64_t nnz) const {
        return nnz * ((vbits ? vbits / 8 : 8) + (o16 ? 2 : 4)) + 4 * (nrows + 1) + 8 * ntab;
    }
};

// 3x3 block storage (bsr.hip): node-row slices, one 4864-B unit per block step
struct BsrStore {
    DevBuf<char> data;
    DevBuf<int32_t> row0, soff;
    int64_t slices = 0, steps = 0, maxw = 0;
    std::vector<int64_t> seg_slc;
    bool built() const { return data.get() != nullptr; }
    int64_t stream_bytes() const { return steps * (64 * 76) + 8 * (slices + 1); }
};

// pattern SELL with L lanes per row (sellp.hip): values / codes only, columns
// from per-slice offset patterns
struct SellpStore {
    DevBuf<char> vals;
    DevBuf<int64_t> eoff;
    DevBuf<int32_t> row0, pat, offs;  // pat: {offs start, width} per slice
    DevBuf<int32_t> rbase;            // per-row column base (rectangular matrices)
    DevBuf<double> vtab;
    int64_t slices = 0, elems = 0, ntab = 0, meta_bytes = 0, stream = 0;
    int L = 0, vbits = 0;
    std::vector<int64_t> seg_slc;
    bool built() const { return vals.get() != nullptr; }
    int64_t stream_bytes() const { return stream; }
};

// stencil-class storage (scs.hip): one 8/16-bit class id per row, a
// dictionary of class stencils over the union of the rows' offsets
struct ScsStore {
    DevBuf<char> cls;
    DevBuf<double> dict;
    DevBuf<int32_t> offs;
    int64_t k = 0, nclass = 0;
    int64_t kr = 0;    // offsets before the padding to a multiple of 8 (the x-staged walk stops there)
    int64_t seg = -1;  // >= 0: only this row segment (a distributed level's halo interior) beside SELL
    int ib = 0;
    bool lanes = false;  // one row per wave (few long rows: spmv_scs_lanes_kernel)
    // x-staged stencil classes on a 3-D grid (spmv_xscs_kernel): per tile of
    // xt[0] x xt[1] x xt[2] grid points its x window (tile + halo xr) in LDS;
    // xlo[k] = the window offset of stencil offset k
    bool staged = false;
    int xt[3] = {0, 0, 0}, xr[3] = {0, 0, 0};
    int xws = 0;          // LDS row stride of the window (>= wx; padded against bank conflicts)
    int xtile_src = 0;    // how the tile was chosen: TuneSource (tuning.hpp)
    bool xfdiv = false;   // the tile's float-reciprocal divisions checked exact (xscs_set_tile)
    bool xsplit = false;  // few long rows: eight lanes per row (spmv_xscs_split_kernel)
    DevBuf<int32_t> xlo;
    std::vector<int> xsteps;  // (dx, dy, dz) of each of the k offsets
    bool built() const { return cls.get() != nullptr; }
    int64_t stream_bytes(int64_t nrows) const { return ib * nrows + 8 * k * nclass + 4 * k; }
};

// grid-transfer classes (gtc.hip) for R/P of a 2x2x2-box hierarchy: an overlay
// on the finalized storage used for the modes it supports (gtc_supports)
struct GtcStore {
    bool on = false, r = false;
    DevBuf<uint8_t> cls;
    DevBuf<uint16_t> dict;  // nclass x ke entries: value index << 8 | step slot
    DevBuf<double> vtab;    // the distinct values (<= 256)
    int ke = 0, nce = 0, ntab = 0, nclass = 0;
    // R: per class its value at each of the 32 slots (dz, dy, dx) a 2 x 2 x 2 box
    // smoothed by the 7-point stencil reaches, +0.0 where the class has no entry
    // (fine.hip k_fine_rr); empty when some class has an entry outside them
    DevBuf<double> wt;
    int64_t fg[3] = {0, 0, 0}, cg[3] = {0, 0, 0};
    bool built() const { return on; }
    int64_t stream_bytes(int64_t nrows) const { return nrows + 2 * (int64_t)nce + 8 * (int64_t)ntab; }
};

// wide grid-transfer classes (gtx.hip): 16-bit class per row, dictionary of
// (window offset, fp64 value) entries in global memory -- every box level
struct GtxStore {
    bool on = false, r = false;
    DevBuf<uint16_t> cls;
    DevBuf<int32_t> dptr, dlen, doff;
    DevBuf<double> dval;
    int64_t nclass = 0, nent = 0;
    int tile[3] = {0, 0, 0}, win[3] = {0, 0, 0}, lo[3] = {0, 0, 0};
    int64_t fg[3] = {0, 0, 0}, cg[3] = {0, 0, 0};
    bool fdiv = false;  // the window's float-reciprocal divisions checked exact (at build)
    bool built() const { return on; }
    int64_t stream_bytes(int64_t nrows) const { return 2 * nrows + 12 * nent + 8 * nclass; }
};

// x-staged SELL (xsell.hip): per group of 4096 rows the x chunks staged in LDS,
// per slice fp64 values + 16-bit LDS indices (or 32-bit columns: escape slices)
struct XsStore {
    DevBuf<char> data;
    DevBuf<uint32_t> desc;
    DevBuf<int32_t> soff, coff, chunks;
    int64_t groups = 0, bytes = 0, steps = 0, chunk_total = 0, escape_slices = 0;
    int64_t maxw = 0;  // widest slice (the burst kernel's batch: 7 or 8 steps)
    bool built() const { return data.get() != nullptr; }
    int64_t stream_bytes() const {
        return bytes + 8 * (int64_t)(desc.size() + 1) + 4 * chunk_total + 4 * (groups + 1);
    }
};

// A CSR matrix resident on the device.  rp64 (int64 row pointers) always
// exists and is what setup kernels (SpGEMM, transpose, extraction) read;
// rp32 + the stream schedule exist when nnz < 2^31 and are what SpMV reads
// (12 B per entry + 4 B per row of index/value traffic).
struct GpuCsr {
    Ctx *ctx = nullptr;
    int64_t nrows = 0, ncols = 0, nnz = 0;
    DevBuf<int64_t> rp64;
    DevBuf<int32_t> rp32;
    DevBuf<int32_t> col;   // padded by 4 entries (16-B vector loads)
    DevBuf<double> val;    // padded by 2 entries
    DevBuf<int32_t> sched; // stream-SpMV row blocks: nblocks+1 row starts
    int64_t nblocks = 0;
    // Row segments (SGS colors, halo boundary/interior): [seg_rows[g], seg_rows[g+1]).
    // Schedule blocks and SELL slices never straddle a segment.
    std::vector<int64_t> seg_rows, seg_blk;
    // the storages: csr_finalize resets all of them, builds what the matrix takes
    // and drops a loser with m.x = {}; gtc / gtx are overlays attached afterwards
    SellStore sell;
    DiaStore dia;
    VecStore vec;
    BsrStore bsr;
    SellpStore sellp;
    ScsStore scs;
    GtcStore gtc;
    GtxStore gtx;
    XsStore xs;
    // gtc_attach / gtx_attach ran since the last finalize (attach_box_transfers retries nothing)
    bool tried_gtc = false, tried_gtx = false;
    // policy inputs, kept across finalize
    bool no_bsr = false;    // e.g. a color-permuted SGS copy
    bool bsr_pin = false;   // a renumbered copy of a 3x3-block matrix: take the block storage whenever it builds
    int8_t kind_pin = -1;   // a renumbered copy: 0 one-lane storages (SELL / x-staged) whenever they build, 1 wave-per-row, 2 CSR-stream
    bool no_sellp = false;  // e.g. a color-permuted SGS copy (swept in SGS mode)
    // grid hint: the rows are the points of an nx x ny x nz grid, x fastest (0 = none);
    // set by the stencil generators, the box hierarchy and amg_csr_set_grid
    // (grid_src 1), else inferred at finalize from the stencil offsets (grid_src 2)
    int64_t grid[3] = {0, 0, 0};
    int grid_src = 0;
    // rank-local matrix of a distributed grid level (dist.hip): its rows are the
    // owned planes of rframe, its columns the local vector of cframe.  The
    // x-staged classes and grid-transfer classes then stage ghost planes through
    // the frame, and their launches split into interior / boundary z-tile ranges
    // (segments 1 / 0, 2) so the interior runs while the halo is in flight.
    SlabFrame rframe, cframe;
    // a renumbered copy (reorder.hip): rows in a new order, each row's entries in
    // the original's stored order with renamed columns -- storages that reorder a
    // row's entries (DIA, stencil / grid-transfer classes, pattern and aligned SELL)
    // are not built, so every row sum stays the original's; col_orig = new column ->
    // original column (the 3x3-block build merges a node's rows by original column)
    bool order_fixed = false;
    std::vector<int32_t> col_orig;
    int kernel = 0;  // SpmvKernel chosen at finalize
    bool spmv_ready() const { return rp32.get() != nullptr && sched.get() != nullptr; }
    int64_t index_bytes() const { return 12 * nnz + 4 * (nrows + 1); }
    // matrix bytes one SpMV streams with the chosen kernel (data + metadata)
    int64_t stream_bytes() const {
        switch (kernel) {
        case SPMV_KERNEL_SELL: return sell.stream_bytes();
        case SPMV_KERNEL_VECTOR: return vec.stream_bytes(nrows, nnz);
        case SPMV_KERNEL_DIA: return dia.stream_bytes(nrows);
        case SPMV_KERNEL_BSR: return bsr.stream_bytes();
        case SPMV_KERNEL_SELLP: return sellp.stream_bytes();
        case SPMV_KERNEL_SCS: return scs.stream_bytes(nrows);
        case SPMV_KERNEL_XS: return xs.stream_bytes();
        default: return index_bytes();
        }
    }
};

}  // namespace famg
