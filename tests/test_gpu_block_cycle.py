"""The block V-cycle (ops.hip MultigridOp::apply_block, solve.cpp
CompositeOp::apply_block), its k-wide kernels (spmm_epi, dense_gemm_cols) and the
adaptive build (amg_adaptive_build).

Column by column is the definition of correct: every k-wide result is compared
bit for bit with the single-vector entry point applied to each column.  Blocks
are column-major torch views with a leading dimension above n whose padding rows
hold 7.5 and must stay untouched.  Tolerances where bits cannot be asked for are
those of tests/test_gpu_nearnull.py (1e-12 on orthonormal bases, 1e-10 relative
on convergence factors) and the cycle tolerance 1e-11.
"""
import numpy as np
import pytest

gpu = pytest.mark.gpu
PAD = 7.5


def fa():
    import faer_amg_amd
    return faer_amg_amd


def device_block(X, ld=None, pad=PAD):
    """X (numpy n x k) as a column-major torch device view with leading dimension ld."""
    import torch
    n, k = X.shape
    ld = n if ld is None else ld
    buf = torch.full((k, ld), pad, dtype=torch.float64, device="cuda:0")
    buf[:, :n] = torch.as_tensor(np.ascontiguousarray(X.T), device="cuda:0")
    return buf, buf[:, :n].t()


def T(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


# ------------------------------------------------- 1. SpMM with the epilogues

MODES = ("set", "add", "resid", "jacobi")


def spmm_epi_vs_spmv(ctx, A, ks=(1, 3, 8, 11)):
    """Every mode and k: each column of amg_csr_spmm_epilogue is bitwise
    amg_csr_spmv_epilogue of that column; ldx, ldy, ldb > n with the padding intact."""
    import torch
    m, n = A.dims()
    rng = np.random.default_rng(12)
    kmax = max(ks)
    X, B, Y0 = rng.uniform(-1, 1, (n, kmax)), rng.uniform(-1, 1, (m, kmax)), rng.uniform(-1, 1, (m, kmax))
    d = T(rng.uniform(0.1, 0.2, m))
    for k in ks:
        xbuf, Xv = device_block(X[:, :k], n + 3)
        bbuf, Bv = device_block(B[:, :k], m + 1)
        for mode in MODES:
            if mode == "jacobi" and m != n:
                continue
            ybuf, Yv = device_block(Y0[:, :k], m + 5)
            A.spmm_epilogue(mode, Xv, Yv, Bv, d)
            ctx.synchronize()
            for c in range(k):
                y1 = T(Y0[:, c])
                A.spmv_epilogue(mode, Xv[:, c].contiguous(), y1, Bv[:, c].contiguous(), d)
                ctx.synchronize()
                assert torch.equal(Yv[:, c], y1), (A.spmv_info()["kernel"], mode, k, c)
            assert bool((ybuf[:, m:] == PAD).all()) and bool((xbuf[:, n:] == PAD).all())
            assert bool((bbuf[:, m:] == PAD).all())


def storage(M):
    """What serves the operator's launches (amg_csr_spmv_info: a grid-transfer overlay
    first, as spmv and spmm_epi take it, else the finalized storage)."""
    info = M.spmv_info()
    return info["kernel"], info


# The compressed storages are built from a minimum size up (DIA codes from 65536
# rows, classes / pattern SELL from 1024, 3x3 blocks where they stream fewer bytes):
# the small operators below take value-coded SELL-64 or CSR-stream (k-wide kernels of
# their own) and are compared all the same; the storage assertions sit on the
# smallest operators that were seen to get the intended storage.

@gpu
def test_spmm_epilogue_dia(ctx):
    for A in (fa().SparseMatOp.laplace3d_7pt(ctx, 12, 11, 10), fa().SparseMatOp.aniso27(ctx, 8, 8, 8, 1.0, 1.0, 0.01)):
        print("small grid operator:", storage(A)[0])
        spmm_epi_vs_spmv(ctx, A)
    A = fa().SparseMatOp.laplace3d_7pt(ctx, 42, 41, 40)  # 68880 rows, ragged against the 256-row blocks
    kind, info = storage(A)
    assert kind == "dia" and info["dia_diagonals"] == 7, info
    spmm_epi_vs_spmv(ctx, A)
    A27 = fa().SparseMatOp.aniso27(ctx, 48, 48, 32, 1.0, 1.0, 0.01)
    kind, info = storage(A27)
    assert kind == "dia" and info["dia_diagonals"] == 27, info
    spmm_epi_vs_spmv(ctx, A27, ks=(3, 11))


@gpu
def test_spmm_epilogue_box_levels(ctx):
    """A_1, P_0 and R_0 of the 16^3 box hierarchy: CSR-stream (512 rows are below every
    compressed storage's minimum) and the 8-bit grid-transfer classes."""
    dims = (16, 16, 16)
    A = fa().SparseMatOp.laplace3d_7pt(ctx, *dims)
    mg = fa().sa_build_box(A, dims, (2, 2, 2), coarsest_dim=10)
    A1 = mg.level(1)[0]
    P0 = mg.level(0)[3]
    k1, i1 = storage(A1)
    kp, ip = storage(P0)
    print(f"16^3: A_1 {k1} classes={i1['classes']}  P_0 {kp} gtc={ip['gtc_kind']}")
    spmm_epi_vs_spmv(ctx, A1)
    spmm_epi_vs_spmv(ctx, P0)
    spmm_epi_vs_spmv(ctx, mg.level(0)[2], ks=(3, 11))  # R_0
    assert k1 == "csr-stream", i1
    assert kp == "gtc" and ip["gtc_kind"] == "gtc", ip


@gpu
def test_spmm_epilogue_classes_and_pattern_sell(ctx):
    """The 128^3 box hierarchy (as test_spmm_compressed_storages builds it): stencil
    classes and pattern SELL, on the smallest operators that have them.  Its class
    levels all run one row per lane (measured: levels 1 and 2; the one-row-per-wave
    kernel needs an operator of >= 256 offsets without a grid, which no hierarchy
    built here has): spmm_scs_lanes_kernel and its epilogues are checked on banded
    operators in tests/test_gpu_row_per_wave.py."""
    F = fa()
    dims = (128, 128, 128)
    A = F.SparseMatOp.laplace3d_7pt(ctx, *dims)
    mg = F.sa_build_box(A, dims, (2, 2, 2), coarsest_dim=500)
    try:
        F.set_flag("dense_tail", 0)  # the plan of every level
        plan = mg.cycle_plan()
    finally:
        F.set_flag("dense_tail", 4096)
    lanes = sorted({p["level"] for p in plan if p["name"] == "scs_lanes"})
    per_lane = sorted({p["level"] for p in plan if p["name"] in ("scs", "xscs")})
    print("class levels: one row per lane", per_lane, "one row per wave", lanes)
    assert per_lane
    for l in sorted({per_lane[-1]} | set(lanes[-1:])):
        M = mg.level(l)[0]
        assert storage(M)[0] == "classes", storage(M)[1]
        spmm_epi_vs_spmv(ctx, M, ks=(3, 11))
    sellp = [M for l in range(1, mg.levels()) for M in mg.level(l)[0:1] + mg.level(l)[2:4]
             if M is not None and storage(M)[0] == "sellp"]
    print("pattern-SELL operators:", [M.dims() for M in sellp])
    assert sellp
    for M in sorted(sellp, key=lambda M: M.nrows)[:2]:
        spmm_epi_vs_spmv(ctx, M, ks=(3, 11))


@gpu
def test_grid_transfer_overlay_is_served_first(ctx):
    """R_0 / P_0 of a 64 x 48 x 40 box hierarchy carry the 8-bit grid-transfer classes over
    pattern SELL with several lanes per row, which rounds differently: the k-wide call
    and the block cycle take the overlay, as the single-vector call does."""
    dims = (64, 48, 40)
    A = fa().SparseMatOp.laplace3d_7pt(ctx, *dims)
    mg = fa().sa_build_box(A, dims, (2, 2, 2), coarsest_dim=100)
    _, _, R0, P0 = mg.level(0)
    assert R0.nrows == 15360
    for M in (R0, P0):
        kind, info = storage(M)
        assert kind == "gtc" and info["gtc_kind"] == "gtc", info
        spmm_epi_vs_spmv(ctx, M, ks=(3, 11))
    lvl0 = [(p["role"], p["name"]) for p in mg.block_plan(3) if p["level"] == 0 and p["role"] in ("restrict", "interp")]
    assert lvl0 == [("restrict", "spmm_gtc"), ("interp", "spmm_gtc")], lvl0
    block_vs_columns(ctx, mg, A.nrows, 5)


@gpu
def test_spmm_epilogue_sell_and_csr_stream(ctx):
    F = fa()
    try:
        F.set_value_codes(False)
        A = F.SparseMatOp.random7(ctx, 9, 8, 7)
        kind, info = storage(A)
        print(f"random7 without value codes: {kind} value_bits={info['value_bits']}")
        assert kind == "sell" and info["value_bits"] == 0
        spmm_epi_vs_spmv(ctx, A)
    finally:
        F.set_value_codes(True)
    try:
        F.set_spmv_format("csr")
        A = F.SparseMatOp.random7(ctx, 9, 8, 7)
        assert storage(A)[0] == "csr-stream"
        spmm_epi_vs_spmv(ctx, A)
        # a row of more than 2048 entries: the whole workgroup reduces it, column after column
        import scipy.sparse as sp
        n = 2600
        M = sp.lil_matrix((n, n))
        M.setdiag(4.0 + np.arange(n) % 3)
        M[0, :] = np.random.default_rng(17).uniform(-1, 1, n)
        M[5, 1:40] = -0.25
        M = M.tocsr()
        M.sort_indices()
        assert M.getnnz(axis=1).max() > 2048
        L = F.SparseMatOp.from_scipy(ctx, M)
        assert storage(L)[0] == "csr-stream"
        spmm_epi_vs_spmv(ctx, L, ks=(3, 11))
    finally:
        F.set_spmv_format("auto")
    # 16-bit value codes (the random coefficients: more than 256 distinct values)
    A = F.SparseMatOp.random7(ctx, 9, 8, 7)
    kind, info = storage(A)
    assert kind == "sell" and info["value_bits"] == 16, info
    spmm_epi_vs_spmv(ctx, A)


@gpu
def test_spmm_epilogue_blocks(ctx):
    A = fa().elasticity_q1((4, 3, 3), seed=11).upload(ctx)
    print("elasticity (4, 3, 3):", storage(A)[0])
    spmm_epi_vs_spmv(ctx, A)
    A = fa().elasticity_q1((12, 10, 10), seed=3).upload(ctx)
    assert storage(A)[0] == "bsr"
    spmm_epi_vs_spmv(ctx, A)


@gpu
def test_spmm_epilogue_xsell(ctx):
    # x-staged SELL is built from 512 row groups of 4096 up: the 128^3 operator of test_spmm_xsell_and_pattern_sell
    A = fa().SparseMatOp.random7(ctx, 128, 128, 128, seed=3, window=4096)
    assert storage(A)[0] == "xsell"
    spmm_epi_vs_spmv(ctx, A)


# ------------------------------------------------------- 2. dense_gemm_cols

@gpu
@pytest.mark.parametrize("dims", [(5, 5, 5), (6, 5, 5)])
def test_coarse_cholesky_block_apply(ctx, dims):
    """dense_gemm_cols: odd n sums in k_gemv's order, even n in k_gemv2's."""
    import torch
    F = fa()
    A = F.SparseMatOp.laplace3d_7pt(ctx, *dims)
    n = A.nrows
    assert n % 2 == dims[0] % 2
    S = F.CoarseCholesky(A)
    B = np.random.default_rng(13).uniform(-1, 1, (n, 11))
    bbuf, Bv = device_block(B, n + 3)
    obuf, Ov = device_block(np.zeros((n, 11)), n + 1)
    S.apply(Ov, Bv)
    ctx.synchronize()
    for c in range(11):
        z = torch.empty(n, dtype=torch.float64, device="cuda:0")
        S.apply(z, Bv[:, c].contiguous())
        ctx.synchronize()
        assert torch.equal(Ov[:, c], z), c
    assert bool((obuf[:, n:] == PAD).all())
    # and it is the solve: A (S b) = b
    res = A.to_scipy() @ Ov.cpu().numpy() - B
    assert np.max(np.abs(res)) <= 1e-10


# ------------------------------------------- 3. block cycle = column cycles

def block_vs_columns(ctx, op, n, k, seed=14, flags=(1, 0)):
    """op.apply on an n x k block (ld > n) against k single applies, bit for bit, with
    the block cycle on and off."""
    import torch
    F = fa()
    B = np.random.default_rng(seed).uniform(-1, 1, (n, k))
    bbuf, Bv = device_block(B, n + 8)
    cols = []
    for c in range(k):
        z = torch.empty(n, dtype=torch.float64, device="cuda:0")
        op.apply(z, Bv[:, c].contiguous())
        ctx.synchronize()
        cols.append(z)
    try:
        for on in flags:
            F.set_flag("block_cycle", on)
            obuf, Ov = device_block(np.zeros((n, k)), n + 16)
            op.apply(Ov, Bv)
            ctx.synchronize()
            for c in range(k):
                assert torch.equal(Ov[:, c], cols[c]), (on, k, c, float((Ov[:, c] - cols[c]).abs().max()))
            assert bool((obuf[:, n:] == PAD).all()) and bool((bbuf[:, n:] == PAD).all())
            assert torch.equal(Bv, T(B))
    finally:
        F.set_flag("block_cycle", 1)
    return cols


_built = {}


def box16(ctx, smoother):
    if ("box", smoother) not in _built:
        dims = (16, 16, 16)
        A = fa().SparseMatOp.laplace3d_7pt(ctx, *dims)
        _built["box", smoother] = (A, fa().sa_build_box(A, dims, (2, 2, 2), coarsest_dim=10, smoother=smoother))
    return _built["box", smoother]


def elasticity_sa(ctx, which=0, elements=(4, 4, 3)):
    """(c): smoothed aggregation of elasticity_q1((4, 4, 3)), L1, block size 3, coarsest_dim 60
    (CSR-stream levels at that size; (12, 10, 10) elements give 3x3-block storage)."""
    if ("el", which, elements) not in _built:
        F = fa()
        if ("elA", elements) not in _built:
            _built["elA", elements] = F.elasticity_q1(elements, seed=11).upload(ctx)
        A = _built["elA", elements]
        nn = F.constant_candidates(A.nrows, 3)
        if which == 1:  # a second hierarchy over the same matrix: another candidate block
            nn = np.asfortranarray(nn * (1.0 + 0.25 * np.sin(np.arange(A.nrows))[:, None]))
        _built["el", which, elements] = (A, F.smoothed_aggregation(A, nn, block_size=3, candidate_dimension=3,
                                                                   coarsest_dim=60, smoother="l1"))
    return _built["el", which, elements]


@gpu
@pytest.mark.parametrize("tail", [0, 64])
@pytest.mark.parametrize("mu,steps", [(1, 1), (2, 2)])
def test_block_cycle_box_jacobi(ctx, mu, steps, tail):
    F = fa()
    A, mg = box16(ctx, "jacobi")
    assert mg.levels() == 4 and mg.level(2)[0].nrows == 64
    try:
        F.set_flag("dense_tail", tail)
        mg.with_cycle_type(mu).with_smoothing_steps(steps)
        if tail and mu == 1:  # level 2 and below run as the dense tail
            assert max(p["level"] for p in mg.block_plan(3)) == 2
            assert [p["name"] for p in mg.block_plan(3) if p["level"] == 2] == ["gemm_cols"]
        for k in (3, 8, 11, 33):  # 33 crosses the 32-column chunk
            block_vs_columns(ctx, mg, A.nrows, k)
    finally:
        F.set_flag("dense_tail", 4096)
        mg.with_cycle_type(1).with_smoothing_steps(1)


@gpu
def test_block_cycle_box_sgs(ctx):
    """A smoother without a k-wide form runs per column inside the block cycle."""
    A, mg = box16(ctx, "sgs")
    assert mg.level(0)[1].kind == "sgs"
    print("SGS block plan:", [p["name"] for p in mg.block_plan(5)])
    block_vs_columns(ctx, mg, A.nrows, 5)


@gpu
def test_block_cycle_elasticity(ctx):
    A, mg = elasticity_sa(ctx)
    assert mg.levels() >= 2
    block_vs_columns(ctx, mg, A.nrows, 5)
    A, mg = elasticity_sa(ctx, elements=(12, 10, 10))  # the same on 3x3-block storage
    assert mg.levels() >= 2 and mg.level(0)[0].spmv_info()["kernel"] == "bsr"
    assert any(p["name"] == "spmm_bsr3" for p in mg.block_plan(5))
    block_vs_columns(ctx, mg, A.nrows, 5)


@gpu
def test_block_cycle_renumbered_fine_level(ctx):
    """(d) 30^3 elements with option 5 forced to 2: the fine level runs renumbered
    (k-wide gather / scatter) and P_0 is CSR-stream."""
    F = fa()
    H = F.elasticity_q1((30, 30, 30), seed=3, permute=True)
    A = H.upload(ctx)
    nn = F.constant_candidates(A.nrows, 3)
    mg = F.smoothed_aggregation(A, nn, block_size=3, candidate_dimension=3, coarsest_dim=150, smoother="l1")
    mg.set_reorder(2)
    assert mg.reordered(0)
    plan = mg.block_plan(3)
    names = [p["name"] for p in plan]
    assert names[0] == "perm_gather_cols" and names[-1] == "perm_scatter_cols", names
    assert [p["name"] for p in plan if p["level"] == 0 and p["role"] == "interp"] == ["spmm_stream"]
    block_vs_columns(ctx, mg, A.nrows, 3)


@gpu
def test_block_composite(ctx):
    F = fa()
    A, mg0 = elasticity_sa(ctx, 0)
    _, mg1 = elasticity_sa(ctx, 1)
    comp = F.Composite(A, [mg0, mg1])
    block_vs_columns(ctx, comp, A.nrows, 5)
    # in place and from host blocks: the same bits
    import torch
    B = np.random.default_rng(14).uniform(-1, 1, (A.nrows, 5))
    cols = block_vs_columns(ctx, comp, A.nrows, 5, flags=(1,))
    ibuf, Iv = device_block(B, A.nrows + 8)
    comp.apply_in_place(Iv)
    ctx.synchronize()
    Hh = comp.apply(np.zeros_like(B, order="F"), np.asfortranarray(B))
    for c in range(5):
        assert torch.equal(Iv[:, c], cols[c])
        assert np.array_equal(Hh[:, c], cols[c].cpu().numpy())
    assert bool((ibuf[:, A.nrows:] == PAD).all())


# ------------------------------------------------------------ 4. launch plan

@gpu
def test_block_plan_box(ctx, no_tail):
    """Hierarchy (a) without its dense tail: block_plan(8) has as many records as
    block_plan(1), block_plan(16) at most twice as many, and every A / R / P record
    costs less than 8 single-column ones.  Its levels run on value-coded SELL-64, the
    8-bit grid-transfer classes and CSR-stream: each has its k-wide launch."""
    A, mg = box16(ctx, "jacobi")
    p1, p8, p16 = mg.block_plan(1), mg.block_plan(8), mg.block_plan(16)
    print("block_plan records: k=1", len(p1), "k=8", len(p8), "k=16", len(p16))
    print("k=1:", [p["name"] for p in p1])
    assert len(p8) == len(p1), ([p["name"] for p in p1], [p["name"] for p in p8])
    assert len(p16) <= 2 * len(p1)
    arp = 0
    for a, b in zip(p1, p8):
        assert (a["level"], a["role"], a["name"]) == (b["level"], b["role"], b["name"])
        if a["kernel"] >= 0:  # an A / R / P launch: the matrix is read once for the 8 columns
            arp += 1
            assert b["bytes"] < 8 * a["bytes"], (a, b)
    assert arp >= 3 * (mg.levels() - 1)


@gpu
@pytest.mark.parametrize("elements", [(4, 4, 3), (12, 10, 10)])
def test_block_plan_fused_storages(ctx, elements):
    """On (c) and on its 3x3-block sibling: an A / R / P record of a storage with an SpMM
    kernel appears once per group of 8 columns per visit, and costs less than its columns."""
    _, mg = elasticity_sa(ctx, elements=elements)
    p1 = mg.block_plan(1)
    fused = [p for p in p1 if p["name"].startswith("spmm_")]
    print(elements, "k=1 plan:", [(p["level"], p["role"], p["name"]) for p in p1])
    assert fused and {p["name"] for p in fused} <= {"spmm_dia", "spmm_scs", "spmm_bsr3", "spmm_sellp", "spmm_sell",
                                                     "spmm_xsell", "spmm_stream", "spmm_gtc"}
    if elements == (12, 10, 10):
        assert any(p["name"] == "spmm_bsr3" and p["level"] == 0 for p in fused)
        p8 = mg.block_plan(8)
        for a, b in zip([p for p in p1 if p["name"] == "spmm_bsr3"], [p for p in p8 if p["name"] == "spmm_bsr3"]):
            assert b["bytes"] < 8 * a["bytes"] and b["rows"] == a["rows"], (a, b)
    key = lambda p: (p["level"], p["role"], p["mode"], p["name"])
    for k in (5, 11, 33):
        pk = mg.block_plan(k)
        groups = sum(-(-min(32, k - c0) // 8) for c0 in range(0, k, 32))  # ceil(kw / 8) per 32-column chunk
        for kk in {key(p) for p in fused}:
            n1 = sum(1 for p in p1 if key(p) == kk)
            nk = sum(1 for p in pk if key(p) == kk)
            assert nk == groups * n1, (k, kk, n1, nk)


# ---------------------------------- 5. smooth_vectors with multigrid / composite

def np_thin_qr(X):
    Q, R = np.linalg.qr(X)
    s = np.where(np.diag(R) < 0, -1.0, 1.0)
    return Q * s, R * s[:, None]


def np_cfs(S, pc, X):
    AW = S @ X
    EV = X - pc(AW)
    return np.sqrt(np.einsum("ij,ij->j", EV, S @ EV)) / np.sqrt(np.einsum("ij,ij->j", X, AW))


def np_smooth(S, pc, X0, iters):
    """smooth_vector (adaptivity.rs:307-390); pc maps an n x k block to M^-1 block."""
    X = np_thin_qr(np_thin_qr(X0)[0])[0]
    for _ in range(iters):
        X = np_thin_qr(X - pc(S @ X))[0]
    return X, np_cfs(S, pc, X)


def column_apply(pc):
    """The handle applied one column at a time (k = 1 calls: never the block cycle)."""
    def f(B):
        out = np.zeros_like(B, order="F")
        for c in range(B.shape[1]):
            out[:, c] = pc.apply(np.zeros(B.shape[0]), np.ascontiguousarray(B[:, c]))
        return out
    return f


@gpu
@pytest.mark.parametrize("kind", ["multigrid", "composite"])
def test_smooth_vectors_block_preconditioner(ctx, kind):
    F = fa()
    dims = (12, 11, 10)
    A = F.SparseMatOp.laplace3d_7pt(ctx, *dims)
    S = A.to_scipy().tocsr()
    mg = F.sa_build_box(A, dims, (2, 2, 2), coarsest_dim=50)
    pc = mg if kind == "multigrid" else F.Composite(A, [mg, F.new_l1(A)])
    X0 = np.random.default_rng(15).standard_normal((S.shape[0], 5))
    Xr, cr = np_smooth(S, column_apply(pc), X0, 3)
    X, cfs = F.smooth_vectors(A, pc, X0=X0, iters=3)
    dx, dc = np.max(np.abs(X - Xr)), np.max(np.abs(cfs / cr - 1.0))
    print(f"smooth_vectors {kind}: |X-Xref|={dx:.2e} |cfs/ref-1|={dc:.2e} cfs={cfs}")
    assert dx <= 1e-12
    assert dc <= 1e-10
    X2, cfs2 = F.smooth_vectors(A, pc, X0=X0, iters=3)
    assert np.array_equal(X, X2) and np.array_equal(cfs, cfs2)


# ------------------------------------------------------------ 6. adaptive build

@gpu
def test_adaptive_build_is_its_composition(ctx, dev):
    import torch
    F = fa()
    A = F.elasticity_q1((4, 4, 3), seed=11).upload(ctx)
    n, dim, iters = A.nrows, 4, 6
    sa = dict(block_size=3, strength_depth=1, coarsest_dim=60)
    comp, cfs = F.adaptive_build(A, dim=dim, seed=0, max_components=3, test_iters=iters, **sa)
    assert comp.kind == "composite" and comp.ncomponents() == 3 and cfs.shape == (2, dim)
    # the same steps from the pieces (adaptivity.rs:56-70, 108-115, 117-162)
    X0 = np.random.default_rng(0).standard_normal((n, dim))
    Xs, _ = F.find_near_null(A, dim - 1, iters=iters, block_size=3, strength_depth=1, X0=X0[:, 1:])
    Bk = np.empty((n, dim), order="F")
    Bk[:, 0] = 1.0
    Bk[:, 1:] = Xs
    Q, _ = F.thin_qr(ctx, Bk)
    mgs = [F.smoothed_aggregation(A, Q, weights=F.create_weights(A, Q), **sa)]
    ref = F.Composite(A, [mgs[0]])
    cref = np.zeros((2, dim))
    for m in (1, 2):
        basis, cref[m - 1] = F.smooth_vectors(A, ref, X0=X0, iters=iters // (2 * m - 1))
        mgs.append(F.smoothed_aggregation(A, basis, weights=cref[m - 1], **sa))
        ref.push(mgs[-1])
    b = torch.as_tensor(np.random.default_rng(16).uniform(-1.0, 1.0, n), device=dev)
    z, zr = torch.empty_like(b), torch.empty_like(b)
    comp.apply(z, b)
    ref.apply(zr, b)
    ctx.synchronize()
    dz = float((z - zr).norm() / zr.norm())
    dc = np.max(np.abs(cfs / cref - 1.0))
    print(f"adaptive build vs composition: |z-zref|/|zref|={dz:.2e} (bits equal: {torch.equal(z, zr)}) "
          f"|cfs/ref-1|={dc:.2e}\ncfs={cfs}")
    assert dz <= 1e-11
    assert dc <= 1e-10
    its = {}
    for name, pc in (("none", None), ("1", F.Composite(A, mgs[:1])), ("2", F.Composite(A, mgs[:2])), ("3", comp)):
        x = torch.zeros_like(b)
        its[name], _ = F.pcg_solve(A, pc, b, x, max_iter=200 if pc is not None else 5000, rel_tol=1e-8)
        ctx.synchronize()
    print(f"pcg iterations: unpreconditioned {its['none']}, 1 / 2 / 3 components {its['1']} / {its['2']} / {its['3']}")
    assert its["3"] <= 200
    assert its["3"] <= its["none"]


# ------------------------------------------- argument checks on live handles

@gpu
def test_leading_dimensions_checked_on_live_handles(ctx):
    """ld < n needs the operator's n: the same statuses, nothing launched."""
    import torch
    import ctypes as C
    F = fa()
    L = F.lib()
    INVALID = 1
    A = F.SparseMatOp.laplace3d_7pt(ctx, 6, 5, 4)
    n = A.nrows
    mg = F.sa_build_box(A, (6, 5, 4), (2, 2, 2), coarsest_dim=20)
    X = torch.zeros((3, n), dtype=torch.float64, device="cuda:0")
    Y = torch.zeros((3, n), dtype=torch.float64, device="cuda:0")
    px, py = C.c_void_p(X.data_ptr()), C.c_void_p(Y.data_ptr())
    assert L.amg_csr_spmm_epilogue(A.h, 0, px, n - 1, py, n, None, 0, None, 3) == INVALID
    assert b"leading dimension" in L.amg_last_error()
    assert L.amg_csr_spmm_epilogue(A.h, 0, px, n, py, n - 1, None, 0, None, 3) == INVALID
    assert L.amg_csr_spmm_epilogue(A.h, 2, px, n, py, n, px, n - 1, None, 3) == INVALID
    assert L.amg_csr_spmm_epilogue(A.h, 2, px, n, py, n, None, 0, None, 3) == INVALID      # RESID without B
    assert L.amg_csr_spmm_epilogue(A.h, 3, px, n, py, n, px, n, None, 3) == INVALID       # JACOBI without d
    assert L.amg_csr_spmm_epilogue(A.h, 0, px, n, px, n, None, 0, None, 3) == INVALID      # X == Y
    assert L.amg_csr_spmm_epilogue(A.h, 0, px, n, py, n, None, 0, None, 0) == 0            # k = 0: nothing to do
    assert L.amg_multigrid_apply(mg.h, py, n - 1, px, n, 3, 1) == INVALID
    assert L.amg_multigrid_apply(mg.h, py, n, px, n - 1, 3, 1) == INVALID
    assert L.amg_multigrid_apply(mg.h, px, n, px, n, 3, 1) == INVALID                     # out aliases rhs
    assert L.amg_multigrid_block_plan(A.h, 3, None, 0, C.byref(C.c_int64())) == INVALID   # not a multigrid
    x0 = np.zeros((n, 4), order="F")
    cfg = F.AdaptiveConfig()
    out = C.c_void_p()
    assert L.amg_adaptive_build(A.h, x0.ctypes.data_as(C.c_void_p), n - 1, 4, C.byref(cfg), None, C.byref(out)) == INVALID
    assert b"leading dimension" in L.amg_last_error()
    assert L.amg_adaptive_build(mg.h, x0.ctypes.data_as(C.c_void_p), n, 4, C.byref(cfg), None, C.byref(out)) == INVALID
    ctx.synchronize()
