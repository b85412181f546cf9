"""The 3x3-block SpMV kernels (bsr.hip, spmm.hip spmm_bsr3_kernel) at their slice,
batch and grid edges, against the oracle's fma chain (bitwise) and a high-precision
host reference (the order-free bound of tests/test_gpu_row_per_wave.py).

Every operator is synthetic (numpy, fixed seeds), uploaded with
SparseMatOp.from_arrays, and takes the block storage by the library's own rule
(blocks >= 70 % filled, fewer bytes than the alternative): full 3x3 blocks of
distinct random values under random sorted node columns, every node row of a slice
at the slice's width but three ragged rows (one empty, one of a single block, one a
block shorter than its slice) in three slices.  Each GPU test asserts kernel == "bsr"
and stream_bytes == steps * 4864 + 8 (slices + 1), steps the sum over slices of the
longest node row, computed here from the CSR arrays.

Matrices (N node rows, 3 N dof rows; slices / block steps; kernel forms reached under
the flag pairs (bsr_kernel, bsr_long) = (default, default), (0, -1), (1, -1), (2, -1),
(3, -1), (0, 0)):
  short        N = 933 square, widths 1 2 3 4 5 7 8 9 15 16 17 31 32 0 6, last slice 37
               live lanes; 15 slices / 156 steps; bsr3<1>, bsr3p<4,false>, <2,true>,
               <4,true> (maxw = 32), bsr3l<1>; spmm_bsr3 k = 1, 3, 8, 11 (15 slices:
               no multiple of its 4-wave workgroups)
  short-holes  short with entries (0,1), (1,0) of one off-diagonal block in five
               removed (zero-filled value slots); as short
  long         N = 897 square, widths 1 7 8 9 15 16 17 23 24 25 33 40 64 65 0, the last
               slice one live lane of an empty row; 15 slices / 347 steps; maxw = 65, so
               flags 1..3 fall back to bsr3<1>; bsr3l<1> walks 1..9 eight-step groups
  long-default 65 x 869 node blocks (R-shaped), widths 160 and 48, the second slice one
               live lane; 2 slices / 208 steps >= 48 per slice: bsr3l<1> at default flags,
               bsr3<1> under (k, -1)
  tall         the short row structure over 65 node columns (P-shaped); as short
  grid4        N = 4095 * 64 + 17 square, width 1 but every 97th slice cycling 2..9;
               4096 slices / 4282 steps, 2.47 M entries: the 4-wave forms bsr3<4>,
               bsr3p<4,true>, bsr3l<4>; runs (default, default), (3, -1), (0, 0) and
               k = 3 set only
spmm_bsr3 takes the JACOBI epilogue on square operators only (the C ABI refuses it
otherwise), so tall runs set, add and resid k-wide and asserts the refusal.

Signed zero.  Dof row 0 of the first block-shorter node row of short, short-holes, long
and tall holds values -1e-200 against x = 1e-200: every product underflows to -0.0.  The
oracle's chain (and every CSR / SELL kernel, which stores only the row's entries) ends
at -0.0; the block storage walks one more (padding) step of that row, fma(+0.0, 1e-200,
-0.0) = +0.0, and gives +0.0.  That row is compared by value, every other row as int64
bit patterns; both signs are asserted.

Also here: SPMV_SETDF on block storage (a plan entry bsr3 / SETDF, bitwise the cycle
with the separate d * f pass), the coded-diagonal branch of BsrRow::load (a two-level
cycle around `short` with a diagonal smoother of 16 distinct values, bitwise the same
steps made one by one through the C ABI), and the SpMV of a renumbered block copy.

Times on an MI355X (pytest call durations, uploads and references included): short
0.54 s, short-holes 0.01, long 0.10, long-default 0.01, tall 0.07, grid4 0.49, coded
diagonal 0.07, renumbered copy (28^3, 368 slices / 9612 steps) 0.62, SETDF (60^3) 7.4 s
per smoother within the whole suite (the hierarchy build and the oracle's arrays are most
of it).  grid4 costs about as much as the five small matrices together and less than a
tenth of the SETDF cases, so its widths were not trimmed.
"""
import time

import numpy as np
import pytest

from test_gpu_row_per_wave import (MODES, PAD, Case, T, check_csr, device_block, fa, kwide_mismatches, row_sums,
                                   run_modes, values)

gpu = pytest.mark.gpu
STEP = 4864  # bytes of one block step: 64 lanes x (9 values + one node column)
TINY = 1e-200

SHORT_W = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 0, 6)
LONG_W = (1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 33, 40, 64, 65, 0)
GRID4_SLICES = 4096
PAIRS = ((None, None), (0, -1), (1, -1), (2, -1), (3, -1), (0, 0))
GRID4_PAIRS = ((None, None), (3, -1), (0, 0))
# the ragged node rows of a slice: lane -> its block count from the slice's width w
RAGGED = ((5, lambda w: 0), (11, lambda w: 1), (20, lambda w: w - 1))


# ------------------------------------------------------------------ builders

def node_pattern(N, NC, widths, seed, ragged=()):
    """Node-level CSR (nrp, ncol) of N node rows over NC node columns.  Slice k (64 node
    rows, the last one what remains) has width widths[k]: each of its node rows holds
    that many blocks, but lanes 5, 11 and 20 of the slices named in `ragged` hold 0, 1 and
    w - 1.  A node row's L columns are one uniform draw from each of L equal strata of
    [0, NC): sorted, distinct, and no two rows alike.  Node column 0 is pinned into node
    row 0 and node column NC - 1 into the last block of the first full row of the widest
    slice."""
    rng = np.random.default_rng(seed)
    widths = np.asarray(widths, np.int64)
    assert (len(widths) - 1) * 64 < N <= len(widths) * 64 and widths.max() <= NC
    lens = np.repeat(widths, 64)[:N].copy()
    for k in ragged:
        assert widths[k] >= 3 and 64 * k + 20 < N
        for lane, f in RAGGED:
            lens[64 * k + lane] = f(int(widths[k]))
    nrp = np.concatenate(([0], np.cumsum(lens)))
    rows = np.repeat(np.arange(N), lens)
    j = np.arange(nrp[-1]) - nrp[rows]
    L = lens[rows]
    lo, hi = j * NC // L, (j + 1) * NC // L
    ncol = lo + np.floor(rng.random(nrp[-1]) * (hi - lo)).astype(np.int64)
    assert lens[0] > 0
    ncol[nrp[0]] = 0
    kw = int(np.argmax(widths))
    ncol[nrp[64 * kw + 1] - 1] = NC - 1  # lane 0 of that slice is never ragged
    return nrp, ncol


def expand3(nrp, ncol):
    """The dof CSR pattern of full 3x3 blocks on a node pattern."""
    N = len(nrp) - 1
    L = np.diff(nrp)
    dlen = np.repeat(3 * L, 3)  # entries of dof rows 3I, 3I + 1, 3I + 2
    rp = np.concatenate(([0], np.cumsum(dlen)))
    seg = (3 * ncol[:, None] + np.arange(3)[None, :]).ravel()  # node row I: seg[3 nrp[I] : 3 nrp[I + 1]]
    src = np.arange(rp[-1]) - np.repeat(rp[:-1], dlen) + np.repeat(np.repeat(3 * nrp[:-1], 3), dlen)
    assert len(rp) == 3 * N + 1
    return rp, seg[src]


def punch_holes(rp, col, val):
    """test_bsr_storage_bitwise's gap recipe: entries (0,1) and (1,0) of the off-diagonal
    blocks with (I + J) % 5 == 0 removed."""
    row = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    I, J = row // 3, col // 3
    hole = ((I + J) % 5 == 0) & (I != J) & (((row % 3 == 0) & (col % 3 == 1)) | ((row % 3 == 1) & (col % 3 == 0)))
    keep = ~hole
    rp2 = np.concatenate(([0], np.cumsum(np.bincount(row[keep], minlength=len(rp) - 1))))
    return rp2, col[keep], val[keep], int(hole.sum())


def block_shape(c):
    """(blocks of every node row, width of every slice, steps, fill) from the CSR arrays
    of an operator of one row segment, its entries in any order: a node row's blocks are
    the distinct node columns of its three dof rows together, a slice (64 node rows) is
    as wide as its longest node row, steps is the sum of the widths -- the layout
    bsr.hip documents -- and fill = entries / (9 blocks)."""
    assert c.n % 3 == 0 and c.ncols % 3 == 0
    N = c.n // 3
    node = np.repeat(np.arange(c.n), c.lens) // 3
    pairs = np.unique(node * (c.ncols // 3) + c.col // 3)
    blocks = np.bincount(pairs // (c.ncols // 3), minlength=N)
    widths = np.maximum.reduceat(blocks, np.arange(0, N, 64))
    return blocks, widths, int(widths.sum()), c.nnz / (9.0 * blocks.sum())


def make_case(name, N, NC, widths, seed, ragged=(), holes=False):
    nrp, ncol = node_pattern(N, NC, widths, seed, ragged)
    rp, col = expand3(nrp, ncol)
    val = values(int(rp[-1]), 0, seed + 1)
    under = None
    if ragged:  # the underflow row: dof row 0 of the block-shorter node row of the first ragged slice
        Iu = 64 * ragged[0] + RAGGED[2][0]
        under = 3 * Iu
        e = slice(rp[under], rp[under + 1])
        val[e] = -TINY * (1.0 + 0.001 * np.arange(rp[under + 1] - rp[under]))
    if holes:
        rp, col, val, removed = punch_holes(rp, col, val)
        assert removed > 0
    c = Case(name, 3 * N, rp, col, val, seed + 2, ncols=3 * NC)
    if under is not None:
        c.x[c.col[c.rp[under]:c.rp[under + 1]]] = TINY
        if holes:  # (the hole recipe leaves 2 of 3 entries per block of a row: every node column stays)
            J = np.unique(c.col[c.rp[under]:c.rp[under + 1]] // 3)
            c.x[(3 * J[:, None] + np.arange(3)[None, :]).ravel()] = TINY
    c.under, c.N, c.NC, c.want_widths = under, N, NC, np.asarray(widths, np.int64)
    c.blocks, c.widths, c.steps, c.fill = block_shape(c)
    c.slices = len(c.widths)
    return c


_cases = {}


def bsr_case(name):
    if name in _cases:
        return _cases[name]
    if name in ("short", "short-holes"):
        N = 14 * 64 + 37
        c = make_case(name, N, N, SHORT_W, 401, ragged=(6, 10, 12), holes=name == "short-holes")
    elif name == "long":
        N = 14 * 64 + 1
        c = make_case(name, N, N, LONG_W, 411, ragged=(3, 8, 13))
    elif name == "long-default":
        c = make_case(name, 65, 869, (160, 48), 421)
    elif name == "tall":
        c = make_case(name, 14 * 64 + 37, 65, np.minimum(SHORT_W, 32), 431, ragged=(6, 10, 12))
    else:
        assert name == "grid4"
        w = np.ones(GRID4_SLICES, np.int64)
        idx = np.arange(0, GRID4_SLICES, 97)
        w[idx] = 2 + np.arange(len(idx)) % 8
        N = (GRID4_SLICES - 1) * 64 + 17
        c = make_case(name, N, N, w, 441)
    _cases[name] = c
    return c


SMALL = ("short", "short-holes", "long", "long-default", "tall")
KWIDE = ("short", "long", "tall")


# ------------------------------------------------------------------ GPU side

def oracle_modes(c):
    """The oracle's ascending-column fma chain (O.Csr.spmv) with the epilogues of
    spmv_dev.hpp's epi_value, one rounding per operation, no contraction; once per case."""
    if getattr(c, "_oracle", None) is None:
        import oracle as O
        ax = O.Csr.from_arrays(c.n, c.ncols, c.rp, c.col, c.val).spmv(c.x[:c.ncols])
        t = c.b - ax
        t = c.d * t
        c._oracle = {"set": ax, "add": c.y0 + ax, "resid": c.b - ax, "jacobi": c.x[:c.n] + t}
    return c._oracle


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def check_bitwise(c, mode, y, tag):
    """y against the oracle as int64 bit patterns; the underflow row by value, its signs
    as the module docstring states them."""
    ref = oracle_modes(c)[mode]
    keep = np.ones(c.n, bool)
    if c.under is not None:
        keep[c.under] = False
        assert y[c.under] == ref[c.under], (c.name, tag, mode, "underflow row")
        if mode == "set":
            assert ref[c.under] == 0.0 and np.signbit(ref[c.under]), (c.name, "the oracle keeps -0.0")
            assert y[c.under] == 0.0 and not np.signbit(y[c.under]), (c.name, tag, "block storage gives +0.0")
    bad = np.flatnonzero(bits(y)[keep] != bits(ref)[keep])
    assert len(bad) == 0, (c.name, tag, mode, len(bad), np.flatnonzero(keep)[bad[:8]])


def assert_block_storage(A, c):
    info = A.spmv_info()
    assert info["kernel"] == "bsr", info
    assert info["stream_bytes"] == c.steps * STEP + 8 * (c.slices + 1), (info, c.steps, c.slices)
    return info


class flag_pairs:
    """Iterate (bsr_kernel, bsr_long) pairs (None: the default read with get_flag);
    the defaults are restored on exit."""

    def __init__(self, pairs):
        self.pairs = pairs

    def __enter__(self):
        F = fa()
        self.k0, self.l0 = F.get_flag("bsr_kernel"), F.get_flag("bsr_long")
        return self

    def __iter__(self):
        F = fa()
        for k, lg in self.pairs:
            F.set_flag("bsr_kernel", self.k0 if k is None else k)
            F.set_flag("bsr_long", self.l0 if lg is None else lg)
            yield "default" if k is None else (k, lg)

    def __exit__(self, *exc):
        F = fa()
        F.set_flag("bsr_kernel", self.k0)
        F.set_flag("bsr_long", self.l0)


def kwide_rect_mismatches(ctx, A, c, ks, modes, seed=14):
    """kwide_mismatches of test_gpu_row_per_wave.py for an operator that need not be
    square and a choice of modes: the entries of amg_csr_spmm_epilogue (X of ncols rows,
    Y and B of n; leading dimensions above them, the padding rows untouched) that differ
    in bits from amg_csr_spmv_epilogue of their column."""
    import torch
    rng = np.random.default_rng(seed)
    kmax = max(ks)
    X = rng.uniform(-1, 1, (c.ncols, kmax))
    B, Y0 = (rng.uniform(-1, 1, (c.n, kmax)) for _ in range(2))
    d = T(c.d)
    bad = 0
    for k in ks:
        xbuf, Xv = device_block(X[:, :k], c.ncols + 3)
        bbuf, Bv = device_block(B[:, :k], c.n + 1)
        for mode in modes:
            ybuf, Yv = device_block(Y0[:, :k], c.n + 5)
            A.spmm_epilogue(mode, Xv, Yv, Bv, d)
            ctx.synchronize()
            for j in range(k):
                y1 = T(Y0[:, j])
                A.spmv_epilogue(mode, Xv[:, j].contiguous(), y1, Bv[:, j].contiguous(), d)
                ctx.synchronize()
                bad += int((Yv[:, j].contiguous().view(dtype=torch.int64) != y1.view(dtype=torch.int64)).sum())
            assert bool((ybuf[:, c.n:] == PAD).all()) and bool((xbuf[:, c.ncols:] == PAD).all())
            assert bool((bbuf[:, c.n:] == PAD).all())
    return bad


def run_case(ctx, name, pairs, kwide):
    t0 = time.time()
    c = bsr_case(name)
    A = c.upload(ctx)
    assert_block_storage(A, c)
    c.worst = (0.0, None, 0)
    first = None
    with flag_pairs(pairs) as fp:
        for tag in fp:
            out = run_modes(ctx, A, c)  # (asserts: the same call twice gives the same bits)
            for mode in MODES:
                c.check(mode, out[mode])
                check_bitwise(c, mode, out[mode], tag)
                if first is not None:
                    assert np.array_equal(bits(out[mode]), bits(first[mode])), (name, tag, mode, "differs from default")
            first = first or out
            if kwide == "all":
                bad = kwide_mismatches(ctx, A)
                assert bad == 0, (name, tag, bad)
            elif kwide is not None:
                bad = kwide_rect_mismatches(ctx, A, c, *kwide)
                assert bad == 0, (name, tag, bad)
    print(f"block storage {name}: {c.slices} slices, {c.steps} steps, fill {c.fill:.3f}, "
          "max error / tolerance %.3g (%s, a row of %d entries)" % c.worst, f"{time.time() - t0:.2f} s")


@gpu
@pytest.mark.parametrize("name", SMALL)
def test_bsr_kernels(ctx, name):
    """Every kernel form (six flag pairs) in four modes: bitwise the oracle's chain (the
    underflow row by value), within the order-free bound, empty rows exact, all flag
    settings and repeated calls the same bits; on short, long and tall every column of the
    k-wide call (k = 1, 3, 8, 11, four modes) bitwise the single-vector call."""
    if name != "tall":
        run_case(ctx, name, PAIRS, "all" if name in KWIDE else None)
        return
    # amg_csr_spmm_epilogue takes JACOBI (x_i of every row) on square operators only:
    # tall runs the three modes it takes and asserts the fourth is refused, not run
    run_case(ctx, name, PAIRS, ((1, 3, 8, 11), ("set", "add", "resid")))
    c = bsr_case(name)
    A = c.upload(ctx)
    _, Xv = device_block(np.zeros((c.ncols, 1)), c.ncols + 3)
    _, Yv = device_block(np.zeros((c.n, 1)), c.n + 5)
    with pytest.raises(fa().AmgError, match="square"):
        A.spmm_epilogue("jacobi", Xv, Yv, Yv, T(c.d))


@gpu
def test_bsr_four_wave_grid(ctx):
    """grid4: 4096 slices, the smallest count that takes the 4-wave workgroups of
    spmv_bsr3_kernel and spmv_bsr3l_kernel (sl = blk * 4 + wave under xcd_remap, the last
    slice 17 live lanes); (default, default), (3, -1), (0, 0); k = 3 set k-wide."""
    run_case(ctx, "grid4", GRID4_PAIRS, ((3,), ("set",)))


# ------------------------------------------------- SETDF, coded diagonal, renumbered copy

def _weights(S, nn):
    return [1.0 / float(nn[:, c] @ (S @ nn[:, c])) for c in range(nn.shape[1])]


def _elasticity_sa(ctx, elements, smoother):
    """test_gpu_sa.py's C5-path hierarchy on the shuffled Q1 elasticity stand-in."""
    F = fa()
    H = F.elasticity_q1(elements, seed=3, permute=True)
    A, S = H.upload(ctx), H.to_scipy()
    nn = F.constant_candidates(S.shape[0], 3)
    mg = F.smoothed_aggregation(A, nn, weights=_weights(S, nn), block_size=3, candidate_dimension=3,
                                coarsest_dim=150, smoother=smoother)
    return A, mg


def _downloaded_case(name, M, seed):
    """A Case on the arrays a device operator hands back (rows in their stored order)."""
    n, ncols = M.dims()
    rp, col, val = M.arrays()
    c = Case(name, n, rp, col, val, seed, ncols=ncols)
    c.blocks, c.widths, c.steps, c.fill = block_shape(c)
    c.slices = len(c.widths)
    return c


def _cycle(ctx, mg, bd):
    import torch
    z = torch.empty_like(bd)
    mg.apply(z, bd)
    ctx.synchronize()
    return z.cpu().numpy()


# R_0 of the stand-in takes the block storage (fewer bytes than 12 B per entry: its node
# rows differ in length, and a slice is as wide as its longest) at 60^3, 61^3, 62^3, 63^3
# and 64^3 elements and at none of 16 x 12 x 12, 20 x 16 x 16, 24^3, 28^3, 32^3, 40^3,
# 48^3, 56^3, 57^3, 58^3, 59^3, where R_0 is CSR-stream and the plans hold no SETDF at
# all: 60^3 (669780 rows, R_0 51378 x 669780) is the smallest cube that qualifies
SETDF_ELEMENTS = (60, 60, 60)


@gpu
@pytest.mark.parametrize("smoother", ["l1", "jacobi"])
def test_bsr_restrict_setdf(ctx, smoother):
    """SPMV_SETDF on block storage (y2 = d * y beside y, the next level's first Jacobi
    step from zero): smoothed aggregation on elasticity_q1(60^3), block size 3 -- the
    smallest cube whose R_0 is block-stored (SETDF_ELEMENTS above).  The plan holds
    a bsr3 / SETDF entry; the cycle is bitwise the one with set_restrict_df(False), whose
    plan is one launch longer, and within 1e-11 of the oracle cycle on the same arrays."""
    import oracle as O
    from test_gpu_parity import oracle_levels_from_gpu
    import torch
    t0 = time.time()
    A, mg = _elasticity_sa(ctx, SETDF_ELEMENTS, smoother)
    R0 = mg.level(0)[2]
    assert_block_storage(R0, _downloaded_case("R_0", R0, 451))
    plan = mg.cycle_plan()
    setdf = [p for p in plan if p["mode"] == "SETDF"]
    print("plan:", [(p["level"], p["role"], p["mode"], p["name"]) for p in plan])
    assert setdf and all(p["name"] == "bsr3" and p["role"] == "restrict" for p in setdf), plan
    b = np.random.default_rng(12).uniform(-1, 1, A.nrows)
    bd = torch.as_tensor(b, device="cuda:0")
    z = _cycle(ctx, mg, bd)
    try:
        mg.set_restrict_df(False)
        plan_off = mg.cycle_plan()
        assert not any(p["mode"] == "SETDF" for p in plan_off) and len(plan_off) == len(plan) + 1, plan_off
        z_off = _cycle(ctx, mg, bd)
    finally:
        mg.set_restrict_df(True)
    assert np.array_equal(bits(z), bits(z_off))
    zref = O.Multigrid(oracle_levels_from_gpu(mg, smoother)).apply(b)
    err = np.linalg.norm(z - zref) / np.linalg.norm(zref)
    print(f"SETDF {smoother}: {mg.levels()} levels, |z - oracle| / |oracle| = {err:.2e}, {time.time() - t0:.1f} s")
    assert err <= 1e-11


@gpu
def test_bsr_coded_diagonal(ctx):
    """BsrRow::load's dc branch (the smoother diagonal as 8-bit codes into a table): a
    two-level Multigrid around `short` (aggregates of 64 rows, an identity coarse operator)
    whose level-0 smoother is a diagonal drawn from 16 values.  The plan shows the codes
    were built (vec_mul_coded) and the post-smoothing step on bsr3 / JACOBI; under every
    flag pair the cycle is bitwise the same steps made one by one through
    amg_csr_spmv_epilogue, which passes d itself."""
    import scipy.sparse as sp
    import torch
    F = fa()
    c = bsr_case("short")
    A = c.upload(ctx)
    assert_block_storage(A, c)
    n, nc = c.n, (c.n + 63) // 64
    rng = np.random.default_rng(461)
    d = rng.uniform(0.1, 0.2, 16)[rng.integers(0, 16, n)]
    P = sp.csr_matrix((np.ones(n), (np.arange(n), np.arange(n) // 64)), shape=(n, nc))
    Pd, Rd = F.SparseMatOp.from_scipy(ctx, P), F.SparseMatOp.from_scipy(ctx, P.T.tocsr())
    Ac = F.SparseMatOp.from_scipy(ctx, sp.identity(nc, format="csr"))
    Cc = F.CoarseCholesky(Ac)
    mg = F.Multigrid(A, F.diag(ctx, d))
    mg.add_level(Ac, Cc, Rd, Pd)
    f, dd = T(c.b), T(d)
    with flag_pairs(PAIRS) as fp:
        for tag in fp:
            plan = [(p["level"], p["role"], p["mode"], p["name"]) for p in mg.cycle_plan()]
            assert (0, "smooth", "-", "vec_mul_coded") in plan and (0, "smooth", "JACOBI", "bsr3") in plan, plan
            assert (0, "resid", "RESID", "bsr3") in plan, plan
            z = torch.empty_like(f)
            mg.apply(z, f)
            ctx.synchronize()
            t = dd * f  # the first Jacobi step from zero
            r, fc, vc, out = torch.empty_like(f), T(np.zeros(nc)), T(np.zeros(nc)), torch.empty_like(f)
            A.spmv_epilogue("resid", t, r, f)
            Rd.apply(fc, r)
            Cc.apply(vc, fc)
            Pd.spmv_epilogue("add", vc, t)
            A.spmv_epilogue("jacobi", t, out, f, dd)
            ctx.synchronize()
            assert torch.equal(z.view(dtype=torch.int64), out.view(dtype=torch.int64)), tag


RENUMBERED_ELEMENTS = (28, 28, 28)  # 70644 rows: a level is renumbered from 65536 rows (27^3: 63504)


@gpu
def test_bsr_renumbered_copy(ctx):
    """The renumbered copy the cycle runs (reorder.hip: nodes renumbered, every row's
    entries in their original order, blocks merged by original column) on the shuffled
    stand-in at 28^3, the smallest cube with the 65536 rows a renumbered level needs:
    reordered(0), block-stored, and its SpMV in four modes within the order-free bound on
    its own downloaded arrays."""
    import torch
    A, mg = _elasticity_sa(ctx, RENUMBERED_ELEMENTS, "l1")
    mg.set_reorder(2)
    _cycle(ctx, mg, torch.zeros(A.nrows, dtype=torch.float64, device="cuda:0"))  # renumbers at the first apply
    assert mg.reordered(0)
    Ar = mg.run_level(0)[0]
    c = _downloaded_case("renumbered", Ar, 471)
    assert c.n == A.nrows >= 65536 and c.nnz == A.nnz
    assert_block_storage(Ar, c)
    with flag_pairs(((None, None), (3, -1), (0, 0))) as fp:
        for tag in fp:
            for mode, y in run_modes(ctx, Ar, c).items():
                c.check(mode, y)
    print(f"renumbered copy: {c.slices} slices, {c.steps} steps, fill {c.fill:.3f}, "
          "max error / tolerance %.3g (%s, a row of %d entries)" % c.worst)


# ------------------------------------------------------- host-only checks

@pytest.mark.parametrize("name", SMALL + ("grid4",))
def test_builders_and_tolerances_on_the_host(name):
    """The builders give sorted, in-range CSR of the intended block shape (per-slice
    widths, predicted steps, fill, the ragged rows, the pinned node columns, the bytes
    that let the storage rule take the blocks), and a plain double evaluation of the sums
    lies within the tolerances of the reference: the bound is checked against the
    reference, not against a kernel."""
    c = bsr_case(name)
    check_csr(c)
    assert c.n == 3 * c.N and c.ncols == 3 * c.NC and len(c.x) == max(c.n, c.ncols)
    assert c.slices == (c.N + 63) // 64 == len(c.want_widths)
    assert np.array_equal(c.widths, c.want_widths) and c.steps == int(c.want_widths.sum())
    assert len(np.unique(c.val)) == c.nnz  # no value codes
    assert c.fill >= 0.7
    nc = c.col // 3
    assert nc.min() == 0 and nc.max() == c.NC - 1
    # fewer bytes than 12 B per entry + 4 B per row (what the rule compares with when no SELL copy exists)
    assert c.steps * STEP + 8 * (c.slices + 1) < 12 * c.nnz + 4 * (c.n + 1)
    if name in ("short", "short-holes", "tall"):
        assert c.N == 14 * 64 + 37 and c.widths.max() == 32 and (c.widths == 0).any()
        assert c.steps == 156
    if name == "short-holes":
        assert c.nnz < bsr_case("short").nnz and c.fill < 1.0
        assert np.array_equal(c.blocks, bsr_case("short").blocks)
    else:
        assert c.fill == 1.0
    if name == "long":
        assert c.N == 14 * 64 + 1 and c.widths.max() == 65 and c.widths[-1] == 0 and c.steps == 347
    if name == "long-default":
        assert (c.N, c.NC) == (65, 869) and c.widths.min() >= 48 and c.steps >= 48 * c.slices
    if name == "tall":
        assert c.NC == 65 and c.n > c.ncols
    if name == "grid4":
        assert c.slices == GRID4_SLICES and c.N % 64 == 17 and set(c.widths.tolist()) == set(range(1, 10))
    if c.under is not None:
        # three slices with an empty node row, one of a single block and one a block short
        ragged = [k for k in range(c.N // 64) if c.blocks[64 * k + 5] == 0 and c.widths[k] >= 3]
        assert len(ragged) == 3 and c.under // 3 == 64 * ragged[0] + 20
        for k in ragged:
            assert c.blocks[64 * k + 11] == 1 and c.blocks[64 * k + 20] == c.widths[k] - 1
            full = np.delete(c.blocks[64 * k:64 * k + 64], [5, 11, 20])
            assert np.all(full == c.widths[k])
        assert c.blocks[c.under // 3] == c.widths[c.under // 3 // 64] - 1
        e = slice(c.rp[c.under], c.rp[c.under + 1])
        assert np.all(c.val[e] < 0) and np.all(c.x[c.col[e]] == TINY)
        assert np.all(c.val[e] * c.x[c.col[e]] == 0.0) and np.all(np.signbit(c.val[e] * c.x[c.col[e]]))
    prod = c.val * c.x[c.col]
    s = np.zeros(c.n)
    live = c.lens > 0
    s[live] = np.add.reduceat(prod, c.rp[:-1][live])
    plain = {"set": s, "add": c.y0 + s, "resid": c.b - s, "jacobi": c.x[:c.n] + c.d * (c.b - s)}
    for mode in MODES:
        c.check(mode, plain[mode])


def test_reference_of_a_rectangular_case():
    """Case.ncols: the row sums of an R-shaped and a P-shaped operator against exact
    rational arithmetic on a few rows (x is max(n, ncols) long, the Jacobi operand x_i
    its first n entries)."""
    from fractions import Fraction
    for name in ("long-default", "tall"):
        c = bsr_case(name)
        s, S = row_sums(c.rp, c.col, c.val, c.x)
        ref, _ = c.reference()["jacobi"]
        for i in (0, 7, c.n - 1):
            t = [Fraction(float(c.val[e])) * Fraction(float(c.x[c.col[e]])) for e in range(c.rp[i], c.rp[i + 1])]
            exact = sum(t, Fraction(0))
            mag = sum((abs(q) for q in t), Fraction(0))
            assert abs(Fraction(float(s[i])) - exact) <= mag * Fraction(1, 2 ** 50)
            jac = Fraction(float(c.x[i])) + Fraction(float(c.d[i])) * (Fraction(float(c.b[i])) - exact)
            assert abs(Fraction(float(ref[i])) - jac) <= (abs(jac) + mag) * Fraction(1, 2 ** 50)
