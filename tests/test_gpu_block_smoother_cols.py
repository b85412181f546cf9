"""The k-wide BlockSmoother apply (block.hip k_block_apply_cols, flag
block_smoother_cols) and what runs through it: the block V-cycle of a
smoother="block" hierarchy, Composite, the block PCG loop and smooth_vectors.

Column by column is the definition of correct: every column of a block apply is
compared bit for bit (torch.equal) with the single-vector apply of that column.
Blocks are column-major torch views; where the leading dimension is above n the
padding rows hold 7.5 and must stay untouched.  Against the restatement
(np_oracle.block_smoother) the tolerances are those of
tests/test_gpu_parity.py for the single apply: 1e-13 relative for scalar blocks,
1e-12 for block_size = 3.
"""
import numpy as np
import pytest

import np_oracle as N
import oracle as O

pytestmark = pytest.mark.gpu
PAD = 7.5
KS = (2, 7, 8, 9, 33)
KMAX = max(KS)


def fa():
    import faer_amg_amd
    return faer_amg_amd


def device_block(X, ld=None):
    """X (numpy n x k) as a column-major torch device view with leading dimension ld."""
    import torch
    n, k = X.shape
    ld = n if ld is None else ld
    buf = torch.full((k, ld), PAD, dtype=torch.float64, device="cuda:0")
    buf[:, :n] = torch.as_tensor(np.ascontiguousarray(X.T), device="cuda:0")
    return buf, buf[:, :n].t()


def box_partition(dims, box):
    nx, ny, nz = dims
    bx, by, bz = box
    cx, cy = -(-nx // bx), -(-ny // by)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (x // bx + cx * (y // by + cy * (z // bz))).ravel().astype(np.int64)


def irregular_partition(sizes, m, rng, empty_id=None):
    """Blocks of the given sizes, then random ones below 90 rows, membership scattered;
    empty_id: an aggregate id that owns no node (the ids above it move up by one)."""
    sizes = list(sizes)
    while sum(sizes) < m:
        sizes.append(int(rng.integers(1, 90)))
    ids = np.repeat(np.arange(len(sizes)), sizes)[:m]
    if empty_id is not None:
        ids = ids + (ids >= empty_id)
    return rng.permutation(ids).astype(np.int64)


OPERATORS = ("box7", "irregular27", "big7", "vector3")
_built = {}


def operator(ctx, name):
    """name -> dict(A, B, S (scipy), part, block_size, tol, R (n x KMAX rhs), cols (the
    KMAX single applies, device vectors)): built once, shared, never written."""
    import scipy.sparse as sps
    import torch
    if name in _built:
        return _built[name]
    F = fa()
    rng = np.random.default_rng({"box7": 61, "irregular27": 62, "big7": 63, "vector3": 64}[name])
    bs, tol = 1, 1e-13
    if name == "box7":  # 2^3 boxes on 6 x 5 x 4: the boxes of the last y layer are cut
        S = O.laplace3d_7pt(6, 5, 4).to_scipy()
        part = box_partition((6, 5, 4), (2, 2, 2))
    elif name == "irregular27":  # a block above one chunk, singletons, a chunk bound at exactly 256, an empty id
        S = O.aniso27(14, 12, 10).to_scipy()
        part = irregular_partition([300, 1, 1, 57, 128, 256, 3], S.shape[0], rng, empty_id=4)
        assert 4 not in part and part.max() > 4
    elif name == "big7":  # one block of 1030 rows: the first width class below 8
        S = O.laplace3d_7pt(11, 10, 10).to_scipy()
        part = irregular_partition([1030], S.shape[0], rng)
    else:  # the coupled operator of test_block_smoother_vector
        L = O.laplace3d_7pt(6, 5, 4).to_scipy()
        Loff = L - sps.diags(L.diagonal())
        K = rng.standard_normal((3, 3))
        K = K + K.T
        D = np.diag([20.0, 25.0, 30.0])
        S = (sps.kron(-Loff, -K) + sps.kron(sps.identity(L.shape[0]), D)).tocsr()
        part = box_partition((6, 5, 4), (3, 2, 2))
        bs, tol = 3, 1e-12
    S = S.tocsr()
    S.sort_indices()
    A = F.SparseMatOp.from_scipy(ctx, S)
    B = F.BlockSmoother(A, part, block_size=bs)
    n = S.shape[0]
    R = rng.uniform(-1, 1, (n, KMAX))
    cols = []
    for c in range(KMAX):
        z = torch.full((n,), np.nan, dtype=torch.float64, device="cuda:0")
        B.apply(z, torch.as_tensor(np.ascontiguousarray(R[:, c]), device="cuda:0"))
        ctx.synchronize()
        cols.append(z)
    _built[name] = dict(A=A, B=B, S=S, part=part, block_size=bs, tol=tol, R=R, cols=cols, n=n)
    return _built[name]


# ------------------------------------------------------------- the bare smoother

@pytest.mark.parametrize("name", OPERATORS)
def test_block_apply_is_bitwise_the_single_apply(ctx, name):
    """k = 2, 7, 8, 9, 33 (groups of 8 with tails of 1, 7 and a lone narrow group), leading
    dimensions n and n + 3, out of place and in place."""
    import torch
    op = operator(ctx, name)
    B, n, R, cols = op["B"], op["n"], op["R"], op["cols"]
    assert fa().get_flag("block_smoother_cols") == 1
    for k in KS:
        for pad in (0, 3):
            rbuf, Rv = device_block(R[:, :k], n + pad)
            obuf, Ov = device_block(np.full((n, k), np.nan), n + pad)
            B.apply(Ov, Rv)
            ctx.synchronize()
            for c in range(k):
                assert torch.equal(Ov[:, c], cols[c]), (name, k, pad, c)
            assert bool((obuf[:, n:] == PAD).all()) and bool((rbuf[:, n:] == PAD).all())
            assert torch.equal(Rv, torch.as_tensor(R[:, :k], device="cuda:0"))
            B.apply_in_place(Rv)
            ctx.synchronize()
            for c in range(k):
                assert torch.equal(Rv[:, c], cols[c]), (name, k, pad, c, "in place")
            assert bool((rbuf[:, n:] == PAD).all())


@pytest.mark.parametrize("name", OPERATORS)
def test_block_apply_against_the_restatement(ctx, name):
    op = operator(ctx, name)
    B, n, R = op["B"], op["n"], op["R"]
    ref = N.block_smoother(op["S"], op["part"], block_size=op["block_size"])
    _, Rv = device_block(R[:, :9])
    _, Ov = device_block(np.full((n, 9), np.nan))
    B.apply(Ov, Rv)
    ctx.synchronize()
    Z = Ov.cpu().numpy()
    for c in range(9):
        zr = ref(R[:, c])
        err = np.linalg.norm(Z[:, c] - zr) / np.linalg.norm(zr)
        print(f"{name} column {c}: rel err vs restatement {err:.2e}")
        assert err <= op["tol"], (name, c, err)


def test_info_and_width_classes(ctx):
    """amg_block_smoother_info: the shape of each operator; big7 has chunks in the
    8-wide class and in a narrower one, so its block apply runs two widths."""
    for name in OPERATORS:
        op = operator(ctx, name)
        info = op["B"].info()
        sizes = np.bincount(op["part"]) * op["block_size"]
        print(name, info)
        assert info["nblocks"] == len(sizes)  # ids that own no node count as (empty) blocks
        assert info["max_block"] == sizes.max()
        assert info["inverse_bytes"] == 8 * int((sizes.astype(np.int64) ** 2).sum())
        assert sum(info["chunks_by_width"].values()) == info["nchunks"] >= 1
    w = operator(ctx, "box7")["B"].info()
    assert w["nchunks"] == 1 and w["chunks_by_width"] == {8: 1, 4: 0, 2: 0, 1: 0}  # 120 rows: one chunk
    w = operator(ctx, "irregular27")["B"].info()["chunks_by_width"]
    assert w[8] >= 3 and w[4] == w[2] == w[1] == 0  # 300 rows: above a chunk, still 8 wide
    w = operator(ctx, "big7")["B"].info()["chunks_by_width"]
    assert w[8] >= 1 and w[4] == 1 and w[2] == w[1] == 0  # 1030 rows: 4 wide; the 70 others 8 wide


@pytest.mark.parametrize("name", ["irregular27", "big7"])
def test_flag_is_bitwise_neutral(ctx, name):
    import torch
    F = fa()
    op = operator(ctx, name)
    B, n, R = op["B"], op["n"], op["R"]
    _, Rv = device_block(R[:, :9], n + 3)
    out = {}
    try:
        for on in (0, 1):
            F.set_flag("block_smoother_cols", on)
            assert F.get_flag("block_smoother_cols") == on
            _, Ov = device_block(np.full((n, 9), np.nan), n + 1)
            B.apply(Ov, Rv)
            ctx.synchronize()
            out[on] = Ov
    finally:
        F.set_flag("block_smoother_cols", 1)
    assert torch.equal(out[0], out[1])
    assert torch.equal(out[1][:, 8], op["cols"][8])


# --------------------------------------------------------------- the block cycle

def hierarchy(ctx):
    if "mg" not in _built:
        dims = (8, 6, 5)
        A = fa().SparseMatOp.laplace3d_7pt(ctx, *dims)
        mg = fa().sa_build_box(A, dims, (2, 2, 2), coarsest_dim=10, smoother="block")
        assert mg.levels() >= 2 and mg.level(0)[1].kind == "block"
        _built["mg"] = (A, mg, box_partition(dims, (2, 2, 2)))
    return _built["mg"]


def block_vs_columns(ctx, op, n, k, seed):
    """op.apply on an n x k block (ld > n) against k single applies, bit for bit."""
    import torch
    Bh = np.random.default_rng(seed).uniform(-1, 1, (n, k))
    bbuf, Bv = device_block(Bh, n + 8)
    obuf, Ov = device_block(np.full((n, k), np.nan), n + 16)
    op.apply(Ov, Bv)
    ctx.synchronize()
    for c in range(k):
        z = torch.empty(n, dtype=torch.float64, device="cuda:0")
        op.apply(z, Bv[:, c].contiguous())
        ctx.synchronize()
        assert torch.equal(Ov[:, c], z), (k, c, float((Ov[:, c] - z).abs().max()))
    assert bool((obuf[:, n:] == PAD).all()) and bool((bbuf[:, n:] == PAD).all())
    assert torch.equal(Bv, torch.as_tensor(Bh, device="cuda:0"))


@pytest.mark.parametrize("tail", [4096, 0])
def test_multigrid_block_apply_is_bitwise_the_column_cycles(ctx, tail):
    """Nine columns through the block V-cycle: the zero-guess smoothing step applies the
    BlockSmoother out of place, the post-smoothing in place on the residual block.  Without
    the dense tail the BlockSmoother of level 1 runs too."""
    F = fa()
    A, mg, _ = hierarchy(ctx)
    try:
        F.set_flag("dense_tail", tail)
        block_vs_columns(ctx, mg, A.nrows, 9, seed=65)
    finally:
        F.set_flag("dense_tail", 4096)


def test_multigrid_block_plan_lists_the_k_wide_launches(ctx, no_tail):
    """ceil(9 / 8) = 2 BlockSmoother launches per smoothing step where there were 9."""
    F = fa()
    _, mg, _ = hierarchy(ctx)
    plans = {}
    try:
        for on in (0, 1):
            F.set_flag("block_smoother_cols", on)
            plans[on] = [p for p in mg.block_plan(9) if p["role"] == "smooth" and p["name"].startswith("block")]
    finally:
        F.set_flag("block_smoother_cols", 1)
    n0, n1 = len(plans[0]), len(plans[1])
    print("smoothing records: flag 0", n0, "flag 1", n1, sorted({p["level"] for p in plans[1]}))
    assert n0 > 0 and n1 * 9 == n0 * 2, (n0, n1)
    assert {p["name"] for p in plans[0]} == {"block"}
    assert {p["name"] for p in plans[1]} == {"block_cols"}
    assert {p["level"] for p in plans[1]} == set(range(mg.levels() - 1))
    # bytes: the inverses and the index once per group, the vectors per column
    for l in range(mg.levels() - 1):
        Bl = mg.level(l)[1]
        nl, inv = Bl.nrows, Bl.info()["inverse_bytes"]
        got = sorted(p["bytes"] for p in plans[1] if p["level"] == l)
        visits = len(got) // 2
        assert got == sorted([inv + 8 * nl + 16 * nl * 1, inv + 8 * nl + 16 * nl * 8] * visits), (l, got)


# ----------------------------------------------------------------- the consumers

@pytest.mark.parametrize("pc", ["multigrid", "block"])
def test_pcg_solve_block_is_the_column_solves(ctx, pc):
    import torch
    F = fa()
    A, mg, part = hierarchy(ctx)
    M = mg if pc == "multigrid" else F.BlockSmoother(A, part)
    n, k = A.nrows, 3
    Bh = np.random.default_rng(66).uniform(-1, 1, (n, k))
    _, Bv = device_block(Bh, n + 2)
    _, Xv = device_block(np.zeros((n, k)), n + 5)
    its, hists = F.pcg_solve_block(A, M, Bv, Xv, max_iter=200, rel_tol=1e-10)
    ctx.synchronize()
    for c in range(k):
        x = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        it, hist = F.pcg_solve(A, M, Bv[:, c].contiguous(), x, max_iter=200, rel_tol=1e-10)
        ctx.synchronize()
        assert 0 < it < 200 and it == its[c], (pc, c, it, its[c])
        assert np.array_equal(hist, hists[c])
        assert torch.equal(Xv[:, c], x), (pc, c)


def test_stationary_solve_block_is_the_column_solves(ctx):
    import torch
    F = fa()
    A, _, part = hierarchy(ctx)
    M = F.BlockSmoother(A, part)
    n, k = A.nrows, 3
    Bh = np.random.default_rng(69).uniform(-1, 1, (n, k))
    _, Bv = device_block(Bh, n + 2)
    _, Xv = device_block(np.zeros((n, k)), n + 5)
    its, hists = F.stationary_solve_block(A, M, Bv, Xv, max_iter=12, rel_tol=1e-12)
    ctx.synchronize()
    for c in range(k):
        x = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        it, hist = F.stationary_solve(A, M, Bv[:, c].contiguous(), x, max_iter=12, rel_tol=1e-12)
        ctx.synchronize()
        assert it == its[c] > 0 and np.array_equal(hist, hists[c])
        assert torch.equal(Xv[:, c], x), c


def test_block_cg_with_a_block_smoother_is_flag_neutral(ctx):
    """The coupled block CG is not its column solves; the flag must not change its bits."""
    import torch
    F = fa()
    A, _, part = hierarchy(ctx)
    M = F.BlockSmoother(A, part)
    n, k = A.nrows, 9
    Bh = np.random.default_rng(70).uniform(-1, 1, (n, k))
    _, Bv = device_block(Bh, n + 2)
    res = {}
    try:
        for on in (0, 1):
            F.set_flag("block_smoother_cols", on)
            _, Xv = device_block(np.zeros((n, k)), n + 5)
            it, hist, _ = F.block_cg_solve(A, M, Bv, Xv, max_iter=200, rel_tol=1e-10)
            ctx.synchronize()
            res[on] = (it, hist, Xv)
    finally:
        F.set_flag("block_smoother_cols", 1)
    assert 0 < res[1][0] < 200 and res[0][0] == res[1][0]
    assert np.array_equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def test_host_blocks_through_the_c_abi(ctx):
    """amg_linop_apply on a host block (staged whole, one k-wide apply): the device bits."""
    op = operator(ctx, "irregular27")
    B, R, cols = op["B"], op["R"], op["cols"]
    Z = B.apply(np.zeros((op["n"], 9), order="F"), np.asfortranarray(R[:, :9]))
    for c in range(9):
        assert np.array_equal(Z[:, c], cols[c].cpu().numpy()), c


def test_composite_of_block_smoother_and_multigrid(ctx):
    F = fa()
    A, mg, part = hierarchy(ctx)
    comp = F.Composite(A, [F.BlockSmoother(A, part), mg])
    block_vs_columns(ctx, comp, A.nrows, 9, seed=67)


def test_smooth_vectors_with_a_block_smoother(ctx):
    F = fa()
    A, _, part = hierarchy(ctx)
    B = F.BlockSmoother(A, part)
    X0 = np.random.default_rng(68).standard_normal((A.nrows, 9))
    res = {}
    try:
        for on in (0, 1):
            F.set_flag("block_smoother_cols", on)
            res[on] = F.smooth_vectors(A, B, X0=X0, iters=3)
    finally:
        F.set_flag("block_smoother_cols", 1)
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert res[1][0].shape == X0.shape and np.all(np.isfinite(res[1][1])) and np.all(res[1][1] > 0.0)
