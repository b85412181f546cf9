"""The dictionary walks of the class kernels (scs.hip spmv_xscs_kernel, gtx.hip
k_gtx_interp / k_gtx_restrict) on grids small enough that nearly every wave mixes
classes, on odd extents and partial tiles, and on shapes with class-uniform waves:
a walk may be regrouped, retiled or rescheduled, never summed differently, so
every check here is bitwise against the oracle's CSR row sums.
"""
import numpy as np
import pytest

import oracle as O
from test_gpu_parity import H, T, _epilogues_bitwise, apply_dev, fa, oracle_levels_from_gpu

pytestmark = pytest.mark.gpu


def _operator(ctx, gen, dims):
    return (fa().SparseMatOp.laplace3d_7pt(ctx, *dims) if gen == "7pt"
            else fa().SparseMatOp.aniso27(ctx, *dims, 1.0, 1.0, 0.01))


def _rows_per_lane(info):
    t = info["tile"]
    rows = t[0] * t[1] * t[2]
    return 1 if rows <= 256 else 2 if rows <= 512 else 4


def test_stencil_class_walks_bitwise(ctx, monkeypatch):
    """x-staged stencil classes of small box hierarchies: the 27-point (24, 20, 18)
    hierarchy (A_1 = 12 x 10 x 9 rows, 125 offsets: on the class-uniform path 7
    blocks of 16, one of 8 and 5 single steps), the 7-point (48, 40, 36) one (A_1
    with 33 offsets) -- no tile of these has an interior beyond the boundary layers,
    so nearly every wave mixes classes -- and 7-point (64, 48, 40) with room for
    class-uniform waves.  The last case forces 8 x 8 x 8 tiles (FAMG_XSCS_TILE, read
    at every build): two rows per lane whatever the tile timing picks.  On every
    x-staged level all four epilogues are bitwise the oracle's."""
    seen, rl_gt1 = 0, 0
    for gen, dims, tile in (("27pt", (24, 20, 18), None), ("7pt", (48, 40, 36), None), ("7pt", (64, 48, 40), None),
                            ("7pt", (48, 40, 36), "8,8,8")):
        if tile:
            monkeypatch.setenv("FAMG_XSCS_TILE", tile)
        else:
            monkeypatch.delenv("FAMG_XSCS_TILE", raising=False)
        A = _operator(ctx, gen, dims)
        mg = fa().sa_build_box(A, dims, (2, 2, 2), coarsest_dim=60)
        for l in range(1, mg.levels() - 1):
            Al = mg.level(l)[0]
            info = Al.spmv_info()
            if not info["xstaged"]:
                continue
            rl = _rows_per_lane(info)
            print(gen, dims, tile, "level", l, Al.dims(), "tile", info["tile"], "rows/lane", rl, "classes",
                  info["classes"], "offsets", info["class_offsets"], "id bits", info["class_id_bits"])
            seen += 1
            rl_gt1 += rl > 1
            _epilogues_bitwise(ctx, Al, 300 + l)
    monkeypatch.delenv("FAMG_XSCS_TILE", raising=False)
    assert seen >= 2, seen
    assert rl_gt1 >= 1, "no x-staged level with more than one row per lane"


def _blocks(M):
    """Padded row lengths of M (the dictionary pads a class to 4-entry groups) as 4-entry
    groups and 8-entry blocks."""
    n = np.diff(np.asarray(M.arrays()[0]))
    p = (n + 3) // 4 * 4
    return p // 4, (p + 7) // 8


GTX_SHAPES = [("7pt", (24, 20, 18)), ("27pt", (21, 19, 17)), ("7pt", (192, 48, 48))]


@pytest.fixture(scope="module")
def gtx_hierarchies(ctx):
    """The hierarchies of GTX_SHAPES with the wide grid-transfer classes wherever they
    build (gtx_time = 0, restored), each with the oracle's V-cycle result: built once."""
    out = {}
    keep = fa().get_flag("dense_tail")
    fa().set_flag("dense_tail", 0)  # every level runs (as the no_tail fixture)
    fa().set_flag("gtx_time", 0)
    try:
        for gen, dims in GTX_SHAPES:
            A = _operator(ctx, gen, dims)
            mg = fa().sa_build_box(A, dims, (2, 2, 2), coarsest_dim=60)
            b = np.random.default_rng(45).uniform(-1, 1, A.nrows)
            zref = O.Multigrid(oracle_levels_from_gpu(mg, "jacobi")).apply(b)
            out[(gen, dims)] = (A, mg, b, zref)
        yield out
    finally:
        fa().set_flag("gtx_time", 2)
        fa().set_flag("dense_tail", keep)


def _gtx_ops(mg):
    for l in range(mg.levels() - 1):
        _, _, R, P = mg.level(l)
        for w, M in (("R", R), ("P", P)):
            if M.spmv_info()["gtc_kind"] == "gtx":
                yield l, w, M


def test_grid_transfer_walks_cover_block_residues(ctx, gtx_hierarchies):
    """The row lengths the grid-transfer tests below walk, from the operators' CSR
    arrays: a row of exactly one 4-entry group, and every residue of the rows' 8-entry
    blocks modulo 2 and 3 (on P also of the 4-entry groups modulo 2) -- a walk in blocks
    of 8 entries, unrolled by two or run 1-2 blocks ahead of its sums, then meets every
    first and last trip it has."""
    one_group = False
    res = {("R", 8, 3): set(), ("R", 8, 2): set(), ("P", 8, 3): set(), ("P", 8, 2): set(), ("P", 4, 2): set()}
    for (gen, dims), (_, mg, _, _) in gtx_hierarchies.items():
        for l, w, M in _gtx_ops(mg):
            g4, b8 = _blocks(M)
            one_group = one_group or bool(np.any(g4 == 1))
            for (ww, be, s), r in res.items():
                if ww == w:
                    r.update(int(v) for v in np.unique((b8 if be == 8 else g4) % s))
    assert one_group, "no row of exactly one 4-entry group"
    for (w, be, s), r in res.items():
        assert r == set(range(s)), (w, be, s, r)


@pytest.mark.parametrize("gen,dims", GTX_SHAPES)
def test_grid_transfer_walks_bitwise(ctx, gtx_hierarchies, gen, dims):
    """Wide grid-transfer classes on odd extents and partial tiles (7-point
    (24, 20, 18), 27-point (21, 19, 17): every wave mixes classes) and on 7-point
    (192, 48, 48), whose level-1 operators have class-uniform waves: y = P v_c,
    y += P v_c and f_c = R r bitwise the oracle's CSR sums; the cycle with the SETDF
    epilogue bitwise the one with the separate d*f pass, bitwise repeatable, and
    within 1e-11 of the oracle."""
    A, mg, b, zref = gtx_hierarchies[(gen, dims)]
    seen = set()
    rng = np.random.default_rng(5)
    for l, w, M in _gtx_ops(mg):
        seen.add((l, w))
        OM = O.Csr.from_arrays(*M.dims(), *M.arrays())
        m, n = M.dims()
        x, y0 = rng.standard_normal(n), rng.standard_normal(m)
        ax = OM.spmv(x)
        assert np.array_equal(apply_dev(ctx, M, x, m), ax), (l, w, M.spmv_info())
        if w == "P":
            yd = T(y0)
            M.spmv_epilogue("add", T(x), yd)
            assert np.array_equal(H(yd), y0 + ax), (l, w, M.spmv_info())
    assert (1, "R") in seen and (1, "P") in seen, seen
    assert any(p["mode"] == "SETDF" for p in mg.cycle_plan())
    z = apply_dev(ctx, mg, b, A.nrows)
    z_again = apply_dev(ctx, mg, b, A.nrows)
    assert np.array_equal(z.view(np.int64), z_again.view(np.int64))
    mg.set_restrict_df(False)
    try:
        assert not any(p["mode"] == "SETDF" for p in mg.cycle_plan())
        z0 = apply_dev(ctx, mg, b, A.nrows)
    finally:
        mg.set_restrict_df(True)
    assert np.array_equal(z.view(np.int64), z0.view(np.int64))
    assert np.linalg.norm(z - zref) <= 1e-11 * np.linalg.norm(zref)


def test_stencil_class_cycle_repeatable(ctx, no_tail):
    """One V-cycle over x-staged levels run twice: bitwise equal outputs, within 1e-11
    of the oracle."""
    dims = (48, 40, 36)
    A = _operator(ctx, "7pt", dims)
    mg = fa().sa_build_box(A, dims, (2, 2, 2), coarsest_dim=60)
    assert any(mg.level(l)[0].spmv_info()["xstaged"] for l in range(1, mg.levels() - 1))
    b = np.random.default_rng(46).uniform(-1, 1, A.nrows)
    z = apply_dev(ctx, mg, b, A.nrows)
    z_again = apply_dev(ctx, mg, b, A.nrows)
    assert np.array_equal(z.view(np.int64), z_again.view(np.int64))
    zref = O.Multigrid(oracle_levels_from_gpu(mg, "jacobi")).apply(b)
    assert np.linalg.norm(z - zref) <= 1e-11 * np.linalg.norm(zref)
