"""The fused fine-level launches of fine.hip (k_fine_rr, k_fine_pj) on the tile
paths test_fine_fused_bitwise does not reach: a second and third x tile of
k_fine_pj (nx > 256), a last tile a few points wide in x and in y, and odd
ny / nz (a partial box in y and z).  Every shape has an even nx and at least
65,536 rows (a fused fine level needs both) and is the smallest that reaches
its path:
  (520, 16, 8)   three fine x tiles of 256, the last 8 wide; coarse 260 x 8 x 4:
                 nine coarse x tiles of 32, the last 4 wide
  (130, 33, 17)  odd ny, nz; coarse 65 x 17 x 9: the last coarse x tile is one
                 column wide
  (258, 34, 10)  two fine x tiles, the last 2 wide; three y tiles of 16, the
                 last 2 rows
  (66, 63, 51)   odd ny, nz on more than one tile in y
The V-cycle with the fused launches is bitwise the unfused one (fine_fuse = 0)
for the default run length and for runs of 2, 6 and 1000 planes.  Last, a
hierarchy whose transfers the fused kernels cannot take (trilinear P) runs the
four-launch form."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(520, 16, 8), (130, 33, 17), (258, 34, 10), (66, 63, 51)]
FUSE = (0, 1, 2, 6, 1000)


def fa():
    import faer_amg_amd
    return faer_amg_amd


def T(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, np.float64), device="cuda:0")


def H(t):
    import torch
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def bits(a):
    return a.view(np.int64)


def build(ctx, dims):
    A = fa().SparseMatOp.laplace3d_7pt(ctx, *dims)
    mg = fa().sa_build_box(A, dims, (2, 2, 2), coarsest_dim=100)
    b = T(np.random.default_rng(11).uniform(-1, 1, int(np.prod(dims))))
    return A, mg, b


def fine_names(mg):
    return [p["name"] for p in mg.cycle_plan() if p["level"] == 0]


def apply_with(ctx, mg, b, ff):
    """One V-cycle with flag fine_fuse = ff: the result and the fine level's plan names."""
    import torch
    fa().set_flag("fine_fuse", ff)
    z = torch.full_like(b, np.nan)
    mg.apply(z, b)
    ctx.synchronize()
    return H(z), fine_names(mg)


@pytest.mark.parametrize("dims", SHAPES)
def test_fine_tiles_bitwise(ctx, dims):
    """Every run length of the fused launches against the unfused cycle, bitwise;
    the plan names fine-rr and fine-pj exactly when the flag is non-zero."""
    assert dims[0] % 2 == 0 and int(np.prod(dims)) >= 65536
    _, mg, b = build(ctx, dims)
    outs = {}
    try:
        for ff in FUSE:
            outs[ff], names = apply_with(ctx, mg, b, ff)
            print(dims, "fine_fuse", ff, names)
            assert ("fine-pj" in names) == (ff != 0) and ("fine-rr" in names) == (ff != 0), (ff, names)
    finally:
        fa().set_flag("fine_fuse", 1)
    assert np.isfinite(outs[0]).all()
    for ff in FUSE[1:]:
        assert np.array_equal(bits(outs[ff]), bits(outs[0])), ff


def test_fine_tiles_coded_diagonal(ctx):
    """Flag dia_dk = 0 reads every Jacobi diagonal through its 1-B codes.  The
    fused launches need the fine level's one-value d, so with the flag off the
    fine level runs unfused whatever fine_fuse says (the plan shows it); k_fine_rr
    reads d_c through its codes (dmode 1) under the default flags, because the
    coarse level's d is not one value: asserted through the launch's plan bytes,
    which then hold the code byte per coarse row.  All four combinations give the
    same bits."""
    dims = (258, 34, 10)
    outs = {}
    try:
        for dk in (1, 0):
            fa().set_flag("dia_dk", dk)
            _, mg, b = build(ctx, dims)
            for ff in (0, 1):
                outs[dk, ff], names = apply_with(ctx, mg, b, ff)
                print(dims, "dia_dk", dk, "fine_fuse", ff, names)
                fused = "fine-pj" in names and "fine-rr" in names
                assert fused == (dk == 1 and ff == 1), (dk, ff, names)
                if fused:
                    # dmode 1: the launch's bytes are f in, f_c and d_c f_c out, the class
                    # byte and the d_c code byte per coarse row (a one-value d_c: no code byte)
                    n = int(np.prod(dims))
                    nc = int(np.prod([(d + 1) // 2 for d in dims]))
                    rr = [p for p in mg.cycle_plan() if p["level"] == 0 and p["name"] == "fine-rr"]
                    assert len(rr) == 1 and rr[0]["bytes"] == 8 * n + 18 * nc, (rr, n, nc)
    finally:
        fa().set_flag("dia_dk", 1)
        fa().set_flag("fine_fuse", 1)
    for key, z in outs.items():
        assert np.array_equal(bits(z), bits(outs[1, 0])), key


def test_fine_tiles_graph_replay(ctx):
    """The fused launches replayed from the captured graph against the eager cycle."""
    import torch
    dims = (130, 33, 17)
    _, mg, b = build(ctx, dims)
    try:
        mg.set_graph(False)
        z0, names = apply_with(ctx, mg, b, 1)
        assert "fine-pj" in names and "fine-rr" in names, names
        mg.set_graph(True)
        zs = [torch.full_like(b, np.nan) for _ in range(3)]  # the capture, then replays
        for z in zs:
            mg.apply(z, b)
        ctx.synchronize()
    finally:
        mg.set_graph(True)
    for z in zs:
        assert np.array_equal(bits(H(z)), bits(z0))


def lin1d(n):
    """Linear interpolation from the (n + 1) // 2 coarse points at the even fine
    indices: weight 1 on them, 1/2 and 1/2 between two, the upper 1/2 dropped
    where it would leave the coarse grid."""
    import scipy.sparse as sp
    x = np.arange(n)
    ev, od = x[x % 2 == 0], x[x % 2 == 1]
    rows = np.concatenate([ev, od, od])
    cols = np.concatenate([ev // 2, od // 2, od // 2 + 1])
    vals = np.concatenate([np.ones(ev.size), np.full(2 * od.size, 0.5)])
    keep = cols < (n + 1) // 2
    return sp.csr_matrix((vals[keep], (rows[keep], cols[keep])), shape=(n, (n + 1) // 2))


def trilinear(dims):
    import scipy.sparse as sp
    nx, ny, nz = dims
    return sp.kron(lin1d(nz), sp.kron(lin1d(ny), lin1d(nx))).tocsr()


def test_fine_unfusable_transfers(ctx):
    """The fusing predicates reject transfers the fused kernels cannot take.  A
    three-level hierarchy on the 7-point Laplacian 64 x 32 x 32 (the smallest DIA
    fine level with an even nx) with trilinear P, R = P^T and Galerkin coarse
    operators: grids, frames, the constant stencil and the one-value d all pass,
    but P's rows hold up to eight entries (k_fine_pj walks four) and R's reach
    (dz, dy, dx) = (-1, -1, -1), outside the 32 slots of k_fine_rr's weights.  So
    with fine_fuse = 1 the fine level takes the four-launch form (the plan names
    neither fused launch), bitwise the fine_fuse = 0 cycle, and within 1e-11 of
    the oracle's cycle over the same levels (test_fine_fused_bitwise's bound)."""
    import oracle as O
    F = fa()
    dims = [(64, 32, 32), (32, 16, 16), (16, 8, 8)]
    A = [F.SparseMatOp.laplace3d_7pt(ctx, *dims[0])]
    A[0].set_grid(*dims[0])
    R, P = [], []
    for l in (0, 1):
        P.append(F.SparseMatOp.from_scipy(ctx, trilinear(dims[l])))
        R.append(F.transpose(P[l]))
        A.append(F.galerkin_rap(R[l], A[l], P[l]))
        A[l + 1].set_grid(*dims[l + 1])
    mg = F.Multigrid(A[0], F.new_jacobi(A[0], 0.66))
    mg.add_level(A[1], F.new_jacobi(A[1], 0.66), R[0], P[0])
    mg.add_level(A[2], F.CoarseCholesky(A[2]), R[1], P[1])
    b = T(np.random.default_rng(11).uniform(-1, 1, A[0].nrows))
    outs = {}
    try:
        for ff in (0, 1):
            outs[ff], names = apply_with(ctx, mg, b, ff)
            print(dims[0], "trilinear, fine_fuse", ff, names)
            assert "fine-rr" not in names and "fine-pj" not in names, (ff, names)
    finally:
        fa().set_flag("fine_fuse", 1)
    assert np.isfinite(outs[0]).all()
    assert np.array_equal(bits(outs[1]), bits(outs[0]))
    levels = []
    for l in range(3):
        lev = {"A": O.Csr.from_arrays(*A[l].dims(), *A[l].arrays()), "smoother": "chol" if l == 2 else "jacobi"}
        if l < 2:
            lev["R"] = O.Csr.from_arrays(*R[l].dims(), *R[l].arrays())
            lev["P"] = O.Csr.from_arrays(*P[l].dims(), *P[l].arrays())
        levels.append(lev)
    zref = O.Multigrid(levels).apply(H(b))
    err = np.linalg.norm(outs[1] - zref) / np.linalg.norm(zref)
    print("trilinear V-cycle rel err vs oracle", err)
    assert err <= 1e-11
