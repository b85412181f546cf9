"""The eight-lanes-per-row x-staged class kernel (scs.hip spmv_xscs_split_kernel).

x-staged levels of few long rows (fewer than 131072 rows, at least 256 padded
offsets, 16-bit class ids) split every row over eight adjacent lanes: lane j takes the
offset pairs (2 (j + 8 s), 2 (j + 8 s) + 1), s = 0, 1, ..., sums them with fma in
ascending s, and the eight partial sums meet in a fixed tree (lanes 1, 2, 4 apart).
That is not the oracle's sequential order, so the checks are those of
test_gpu_row_per_wave.py: a long-double reference and the per-row bound E_i = 2 n_i u S_i
(valid for any summation order) plus one rounding per epilogue operation.  Bitwise on
top: the same call twice, every tile (one pass, several passes, fewer than 128 rows per
tile), every k-wide call per column; with FAMG_XSCS_SPLIT=0 the operator is back on
one lane per row and bitwise the oracle's CSR sums.

Operators: a full-box stencil with one random value per offset, truncated at the grid
faces, on odd extents (numpy, fixed seeds, SparseMatOp.from_arrays and the grid hint).
    shape 1  (20, 18, 14), radii (3, 3, 3): 343 offsets, k = 344 = 16 * 21 + 8 (the
             last step covers half a group), 343 classes
    shape 2  (22, 15, 11), radii (4, 3, 2): 315 offsets, k = 320 = 16 * 20 (a whole
             number of steps), 315 classes
No extent is a multiple of a tile extent used here, so partial tiles occur everywhere.
"""
import numpy as np
import pytest

import oracle as O
from test_gpu_parity import _epilogues_bitwise, apply_dev, fa, oracle_levels_from_gpu
from test_gpu_row_per_wave import MODES, Case, apply3_mismatches, check_csr, kwide_mismatches, run_modes

gpu = pytest.mark.gpu

# name: (grid, radii, offsets, padded offsets k, classes)
SHAPES = {
    "half-step": ((20, 18, 14), (3, 3, 3), 343, 344, 343),
    "whole-steps": ((22, 15, 11), (4, 3, 2), 315, 320, 315),
}
# shape 1's tiles: 64 rows (a 512-thread workgroup), 128 (one pass), 256 (two passes), 1024 (eight)
TILES = ("4,4,4", "8,8,2", "16,8,2", "16,8,8")

_cases = {}


def box_stencil(grid, radii, seed):
    """CSR of the full-box stencil: offset (dx, dy, dz) carries one random value,
    entries leaving the grid are dropped; columns ascending in every row."""
    nx, ny, nz = grid
    rx, ry, rz = radii
    n = nx * ny * nz
    d = np.array([(dx, dy, dz) for dz in range(-rz, rz + 1) for dy in range(-ry, ry + 1)
                  for dx in range(-rx, rx + 1)])
    K = len(d)
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.5, 1.5, K) * rng.choice((-1.0, 1.0), K)
    assert len(np.unique(v)) == K
    i = np.arange(n)
    X, Y, Z = (i % nx)[:, None] + d[None, :, 0], (i // nx % ny)[:, None] + d[None, :, 1], \
        (i // (nx * ny))[:, None] + d[None, :, 2]
    keep = (X >= 0) & (X < nx) & (Y >= 0) & (Y < ny) & (Z >= 0) & (Z < nz)
    col = (Z * ny + Y) * nx + X
    rp = np.concatenate(([0], np.cumsum(keep.sum(axis=1))))
    return rp, col[keep], np.broadcast_to(v, col.shape)[keep]


def case(name):
    if name not in _cases:
        grid, radii, _, _, _ = SHAPES[name]
        rp, col, val = box_stencil(grid, radii, 400 + len(name))
        _cases[name] = Case("split-" + name, int(np.prod(grid)), rp, col, val, 500 + len(name))
    return _cases[name]


def upload(ctx, name, lanes=8):
    """The operator with its grid hint; asserts the storage every test here is about."""
    c = case(name)
    A = fa().SparseMatOp.from_arrays(ctx, c.n, c.n, c.rp, c.col, c.val)
    A.set_grid(*SHAPES[name][0])
    info = A.spmv_info()
    assert info["kernel"] == "classes" and info["xstaged"] and info["row_lanes"] == lanes, info
    _, _, _, kp, classes = SHAPES[name]
    assert (info["classes"], info["class_offsets"], info["class_id_bits"]) == (classes, kp, 16), info
    return c, A, info


def dense_terms(c):
    """Products a_ij x_j of every row at its offset's position among the sorted
    offsets, padded to a multiple of 8 (absent terms 0.0: fma(+0.0, finite, acc) = acc)."""
    rows = np.repeat(np.arange(c.n), c.lens)
    offs = np.unique(c.col - rows)
    kp = (len(offs) + 7) // 8 * 8
    P = np.zeros((c.n, kp))
    P[rows, np.searchsorted(offs, c.col - rows)] = c.val * c.x[c.col]
    return P


def eight_chain_sums(P):
    """Row sums in the kernel's order, in plain double (rounded products, no fma)."""
    n, k = P.shape
    part = []
    for j in range(8):
        acc = np.zeros(n)
        s = 0
        while 2 * (j + 8 * s) < k:
            acc = acc + P[:, 2 * (j + 8 * s)]
            acc = acc + P[:, 2 * (j + 8 * s) + 1]
            s += 1
        part.append(acc)
    for m in (1, 2, 4):  # lane l += lane l ^ m; lane 0 holds the row sum
        part = [part[l] + part[l ^ m] for l in range(8)]
    return part[0]


# ------------------------------------------------------------------ host-only

@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_and_eight_chain_order_on_the_host(name):
    """k, the class count and the routing rule's inputs of each shape, computed from
    the CSR arrays; the eight-chain order evaluated in plain double lies within the
    tolerances of the reference (the bound is not mis-derived) and differs from the
    sequential sum in some row (the checks below would notice the other kernel)."""
    grid, radii, K, kp, classes = SHAPES[name]
    c = case(name)
    check_csr(c)
    rows = np.repeat(np.arange(c.n), c.lens)
    offs = np.unique(c.col - rows)
    assert len(offs) == K == np.prod([2 * r + 1 for r in radii]) and (K + 7) // 8 * 8 == kp
    assert 256 <= kp <= 1024 and (kp % 16 == 8) == (name == "half-step")
    assert 1024 <= c.n < 131072 and K * c.n <= 2 * c.nnz and len(np.unique(c.val)) > 256
    seen = {((c.col[c.rp[i]:c.rp[i + 1]] - i).tobytes(), c.val[c.rp[i]:c.rp[i + 1]].tobytes()) for i in range(c.n)}
    assert len(seen) == classes > 256  # 16-bit class ids
    # partial tiles: under the x extents the tile timing tries (8, 16) and under every forced tile
    assert grid[0] % 8 and grid[0] % 16
    if name == "half-step":
        assert all(any(e % int(t) for e, t in zip(grid, tile.split(","))) for tile in TILES)
    P = dense_terms(c)
    s8 = eight_chain_sums(P)
    seq = np.zeros(c.n)
    for k in range(P.shape[1]):
        seq = seq + P[:, k]
    assert np.any(s8 != seq)
    plain = {"set": s8, "add": c.y0 + s8, "resid": c.b - s8, "jacobi": c.x + c.d * (c.b - s8)}
    for mode in MODES:
        c.check(mode, plain[mode])


# ------------------------------------------------------------------------ GPU

@gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_split_modes_and_kwide(ctx, name):
    """Four modes against the reference within the per-row tolerance, each twice with
    the same bits; amg_csr_spmm_epilogue and a 3-column apply bitwise per column."""
    c, A, info = upload(ctx, name)
    c.worst = (0.0, None, 0)
    for mode, y in run_modes(ctx, A, c).items():
        c.check(mode, y)
    print(f"eight lanes per row ({name}): tile {info['tile']} ({info['tile_source']}), "
          "max error / tolerance %.3g (%s, a row of %d entries)" % c.worst)
    bad_k, bad_a = kwide_mismatches(ctx, A), apply3_mismatches(ctx, A)
    assert bad_k == 0 and bad_a == 0, (name, bad_k, bad_a)


@gpu
def test_split_tiles_give_identical_bits(ctx, monkeypatch):
    """Shape 1 under forced tiles of 64, 128, 256 and 1024 rows (FAMG_XSCS_TILE, read
    at every build): a partial workgroup, one pass, two and eight passes over the
    window.  Every mode within the tolerance and bitwise the same under every tile."""
    name = "half-step"
    first = None
    try:
        for tile in TILES:
            monkeypatch.setenv("FAMG_XSCS_TILE", tile)
            c, A, info = upload(ctx, name)
            assert info["tile"] == tuple(int(t) for t in tile.split(",")) and info["tile_source"] == "env", info
            out = run_modes(ctx, A, c)
            for mode, y in out.items():
                c.check(mode, y)
            if first is None:
                first = out
            for mode in MODES:
                assert np.array_equal(out[mode].view(np.int64), first[mode].view(np.int64)), (tile, mode)
    finally:
        monkeypatch.delenv("FAMG_XSCS_TILE", raising=False)


@gpu
def test_switch_restores_one_lane_per_row(ctx, monkeypatch):
    """FAMG_XSCS_SPLIT=0 (read at every build): shape 1 reports one lane per row and
    all four epilogues are bitwise the oracle's CSR sums; without the switch the same
    arrays are back on eight lanes."""
    monkeypatch.setenv("FAMG_XSCS_SPLIT", "0")
    try:
        _, A, _ = upload(ctx, "half-step", lanes=1)
        _epilogues_bitwise(ctx, A, 31)
    finally:
        monkeypatch.delenv("FAMG_XSCS_SPLIT", raising=False)
    upload(ctx, "half-step", lanes=8)


@gpu
def test_split_level_in_a_cycle(ctx, no_tail):
    """A two-level Multigrid around shape 1 (aggregates of 64 rows, an identity coarse
    operator): the residual and the Jacobi step of level 0 run on the x-staged classes
    of the matrix, and one V-cycle is within 1e-11 of the oracle."""
    import scipy.sparse as sp
    F = fa()
    c, A, _ = upload(ctx, "half-step")
    n = c.n
    nc = (n + 63) // 64
    P = sp.csr_matrix((np.ones(n), (np.arange(n), np.arange(n) // 64)), shape=(n, nc))
    Pd, Rd = F.SparseMatOp.from_scipy(ctx, P), F.SparseMatOp.from_scipy(ctx, P.T.tocsr())
    Ac = F.SparseMatOp.from_scipy(ctx, sp.identity(nc, format="csr"))
    mg = F.Multigrid(A, F.new_jacobi(A))
    mg.add_level(Ac, F.CoarseCholesky(Ac), Rd, Pd)
    assert mg.level(0)[0].spmv_info()["row_lanes"] == 8
    plan = mg.cycle_plan()
    print("plan:", [(p["level"], p["role"], p["mode"], p["name"]) for p in plan])
    own = [p for p in plan if p["level"] == 0 and p["mode"] in ("RESID", "JACOBI")]
    assert {p["mode"] for p in own} == {"RESID", "JACOBI"} and all(p["name"] == "xscs" for p in own), plan
    b = np.random.default_rng(47).uniform(-1, 1, n)
    z = apply_dev(ctx, mg, b, n)
    zref = O.Multigrid(oracle_levels_from_gpu(mg, "jacobi")).apply(b)
    assert np.linalg.norm(z - zref) <= 1e-11 * np.linalg.norm(zref)
