"""amg_sa_refresh: the numeric re-setup of a smoothed-aggregation hierarchy for a
matrix with the build's sparsity pattern and new values.

The reference of every comparison is the composition of the setup pieces on the
recorded aggregates -- sa_tentative_block(sa_aggregates(l)), block_jacobi or
smooth_interpolation, transpose, galerkin_rap, nn_postprocess feeding the next level
-- which test_gpu_sa.py::test_sa_build_equals_composition pins to amg_sa_build.  All
comparisons are bitwise (rowptr, columns, values by bit pattern; V-cycles by bit
pattern): the refill kernels keep spgemm's order of accumulation, and no storage of
these small levels is chosen by timing, so two builds of one matrix agree to the bit.
"""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu


def fa():
    import faer_amg_amd
    return faer_amg_amd


def bits(v):
    return np.asarray(v, np.float64).view(np.int64)


def same_csr(X, Y):
    a, b = X.arrays(), Y.arrays()
    return (X.dims() == Y.dims() and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            and np.array_equal(bits(a[2]), bits(b[2])))


def scaled(S, seed):
    """D S D with a random positive diagonal: S's pattern entry for entry, still SPD."""
    d = np.random.default_rng(seed).uniform(0.5, 2.0, S.shape[0])
    T = S.copy()
    T.data = S.data * d[np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))] * d[S.indices]
    return T


def weights(S, nn):
    return [1.0 / float(nn[:, c] @ (S @ nn[:, c])) for c in range(nn.shape[1])]


def compose(ctx, A, nn, mg, bs, cd):
    """The hierarchy of the setup pieces on mg's recorded aggregates:
    (As, Rs, Ps, [(agg, naggs, block size)] per coarsening step)."""
    F = fa()
    As, Rs, Ps, parts = [A], [], [], []
    cur = A
    for l in range(mg.levels() - 1):
        agg, na = mg.sa_aggregates(l)
        P, cnn = F.sa_tentative_block(ctx, agg, na, nn, block_size=bs, candidate_dimension=cd)
        P = F.block_jacobi(cur, P, bs) if bs > 1 else F.smooth_interpolation(cur, P)
        R = F.transpose(P)
        Ac = F.galerkin_rap(R, cur, P)
        nn = F.nn_postprocess(Ac, cnn, 3)
        parts.append((agg, na, bs))
        As.append(Ac)
        Rs.append(R)
        Ps.append(P)
        cur, bs = Ac, cd
    return As, Rs, Ps, parts


def assert_hierarchy(mg, comp):
    As, Rs, Ps, _ = comp
    assert mg.levels() == len(As)
    for l in range(mg.levels()):
        Al, _, Rl, Pl = mg.level(l)
        assert same_csr(Al, As[l]), f"A of level {l}"
        if l + 1 < mg.levels():
            assert same_csr(Pl, Ps[l]), f"P of level {l}"
            assert same_csr(Rl, Rs[l]), f"R of level {l}"


def composed_multigrid(mg, comp, smoother):
    """amg_multigrid_create / add_level over comp's operators with the smoothers
    amg_sa_build gives them (SGS: L1 where mg's level fell back to it)."""
    F = fa()
    As, Rs, Ps, parts = comp

    def make(l):
        if l + 1 == len(As):
            return F.CoarseCholesky(As[l])
        if smoother == "jacobi":
            return F.new_jacobi(As[l], 0.66)
        if smoother == "l1":
            return F.new_l1(As[l])
        if smoother == "sgs":
            return F.SymGaussSeidel(As[l]) if mg.level(l)[1].kind == "sgs" else F.new_l1(As[l])
        if smoother == "block":
            agg, na, bs = parts[l]
            return F.BlockSmoother(As[l], agg, na, block_size=bs)
        assert smoother == "chebyshev"
        return F.new_chebyshev(As[l])

    out = F.Multigrid(As[0], make(0))
    for l in range(1, len(As)):
        out.add_level(As[l], make(l), Rs[l - 1], Ps[l - 1])
    return out


def vcycle(ctx, mg, b, z=None):
    import torch
    z = torch.empty_like(b) if z is None else z
    mg.apply(z, b)
    ctx.synchronize()
    return z.cpu().numpy().copy()


def rhs(n, seed=12, k=None):
    import torch
    r = np.random.default_rng(seed).uniform(-1, 1, n if k is None else (k, n))
    t = torch.as_tensor(r, device="cuda:0")
    return t if k is None else t.T  # column-major n x k


_cache = {}


def elasticity(ctx, elements=(5, 4, 4), coarsest=150, smoother="l1"):
    """The Q1 elasticity stand-in, its build and two matrices of the same pattern:
    D A D and the generator at another contrast."""
    key = (elements, coarsest, smoother)
    if key not in _cache:
        F = fa()
        H = F.elasticity_q1(elements, seed=11)
        S = H.to_scipy().tocsr()
        nn = F.constant_candidates(S.shape[0], 3)
        A = H.upload(ctx)
        S2 = scaled(S, 3)
        S3 = F.elasticity_q1(elements, contrast=2.0, seed=11).to_scipy().tocsr()
        assert np.array_equal(S3.indptr, S.indptr) and np.array_equal(S3.indices, S.indices)
        assert not np.array_equal(S3.data, S.data)
        _cache[key] = dict(S=S, nn=nn, A=A, S2=S2, A2=F.SparseMatOp.from_scipy(ctx, S2),
                           A3=F.SparseMatOp.from_scipy(ctx, S3))
    return _cache[key]


def build_elasticity(ctx, p, coarsest, smoother="l1"):
    return fa().smoothed_aggregation(p["A"], p["nn"], weights=weights(p["S"], p["nn"]), block_size=3,
                                     candidate_dimension=3, coarsest_dim=coarsest, smoother=smoother)


# ---------------------------------------------------------------- 1: block path

def test_block_path_equals_composition(ctx):
    """Block size 3, three constant candidates: after refresh(A') every level's P, R
    and A_c are the composition on the recorded aggregates, bit for bit -- for D A D
    (the recording refresh) and for the generator at another contrast (a reusing one)."""
    p = elasticity(ctx)
    mg = build_elasticity(ctx, p, 150)
    assert mg.levels() >= 2
    info = mg.refresh(p["A2"], p["nn"])
    assert info["recorded"] and info["record_bytes"] > 0 and info["levels"] == mg.levels()
    assert_hierarchy(mg, compose(ctx, p["A2"], p["nn"], mg, 3, 3))
    info = mg.refresh(p["A3"], p["nn"])
    assert not info["recorded"] and info["record_bytes"] > 0
    assert_hierarchy(mg, compose(ctx, p["A3"], p["nn"], mg, 3, 3))


# --------------------------------------------------------------- 2: scalar path

def test_scalar_path_equals_composition(ctx):
    """Block size 1 through smooth_interpolation on every level (one of the two
    candidates kept; keeping both fails in amg_sa_build itself, whose MIS leaves
    one-node aggregates here): amg_gen_random_7pt on 12 x 11 x 10 with two seeds, the
    same pattern with other values; two random candidates; at least three levels."""
    F = fa()
    cd = 1
    dims = (12, 11, 10)
    A = F.SparseMatOp.random7(ctx, *dims, seed=42, window=-1)
    A2 = F.SparseMatOp.random7(ctx, *dims, seed=43, window=-1)
    a, a2 = A.arrays(), A2.arrays()
    assert np.array_equal(a[0], a2[0]) and np.array_equal(a[1], a2[1]) and not np.array_equal(a[2], a2[2])
    n = A.nrows
    nn = np.asfortranarray(np.random.default_rng(6).uniform(0.5, 1.5, (n, 2)))
    nn2 = np.asfortranarray(np.random.default_rng(7).uniform(0.5, 1.5, (n, 2)))
    mg = F.smoothed_aggregation(A, nn, block_size=1, candidate_dimension=cd, coarsest_dim=20, smoother="jacobi")
    assert mg.levels() >= 3
    for which in range(2):  # the recording refresh, then a reusing one
        info = mg.refresh(A2, nn2)
        assert info["recorded"] == (which == 0)
        assert_hierarchy(mg, compose(ctx, A2, nn2, mg, 1, cd))


# ------------------------------------------------ 3: recorded path, round trip

def test_reuse_equals_record_and_round_trip(ctx):
    p = elasticity(ctx)
    mg = build_elasticity(ctx, p, 150)
    b = rhs(p["S"].shape[0])
    built = [[X.arrays() if X is not None and i != 1 else None for i, X in enumerate(mg.level(l))]
             for l in range(mg.levels())]
    z_built = vcycle(ctx, mg, b)

    def snapshot():
        return [[X.arrays() if X is not None and i != 1 else None for i, X in enumerate(mg.level(l))]
                for l in range(mg.levels())]

    def same(s, t):
        return all((x is None and y is None) or
                   (np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(bits(x[2]), bits(y[2])))
                   for ls, lt in zip(s, t) for x, y in zip(ls, lt))

    assert mg.refresh(p["A2"], p["nn"])["recorded"]
    first = snapshot()
    z_first = vcycle(ctx, mg, b)
    assert not same(first, built)
    assert not mg.refresh(p["A2"], p["nn"])["recorded"]
    assert same(snapshot(), first)
    assert np.array_equal(bits(vcycle(ctx, mg, b)), bits(z_first))
    assert not mg.refresh(p["A"], p["nn"])["recorded"]  # back to the build's matrix
    assert same(snapshot(), built)
    assert np.array_equal(bits(vcycle(ctx, mg, b)), bits(z_built))


def test_earlier_level_handles_keep_the_old_operators(ctx):
    """The aliasing rule of amg.h: handles from amg_multigrid_get_level before the
    refresh keep the hierarchy they were taken from."""
    p = elasticity(ctx)
    mg = build_elasticity(ctx, p, 150)
    A1 = mg.level(1)[0]
    _, _, R0, P0 = mg.level(0)
    before = [X.arrays() for X in (A1, R0, P0)]
    mg.refresh(p["A2"], p["nn"])
    for X, old in zip((A1, R0, P0), before):
        assert all(np.array_equal(u, v) for u, v in zip(X.arrays(), old))
    assert not np.array_equal(mg.level(1)[0].arrays()[2], before[0][2])
    assert same_csr(mg.level(0)[0], p["A2"])


# ------------------------------------------------------------- 4: stale state

STALE = dict(elements=(6, 5, 5), coarsest=12)


@pytest.mark.parametrize("reorder", [1, 2])
@pytest.mark.parametrize("graph", [True, False])
def test_no_stale_state_after_refresh(ctx, graph, reorder):
    """Apply with fixed (out, rhs) pointers, refresh, apply with the same pointers: the
    cycle is the one of a multigrid composed from the pieces for A' -- no graph captured
    before the refresh, no dense tail, renumbered copy or diagonal code of the old
    values survives.  Three levels with a middle one of at most 4096 rows (the dense
    tail); also the block apply with k = 3."""
    import torch
    F = fa()
    p = elasticity(ctx, STALE["elements"])
    mg = build_elasticity(ctx, p, STALE["coarsest"])
    assert mg.levels() >= 3 and mg.level(1)[0].nrows <= 4096
    mg.set_graph(graph)
    mg.set_reorder(reorder)
    n = p["S"].shape[0]
    b, z = rhs(n), torch.empty(n, dtype=torch.float64, device="cuda:0")
    B = rhs(n, seed=13, k=3)
    Z = torch.empty((3, n), dtype=torch.float64, device="cuda:0").T
    z_old = vcycle(ctx, mg, b, z)
    mg.apply(Z, B)
    ctx.synchronize()
    mg.refresh(p["A2"], p["nn"])
    comp = compose(ctx, p["A2"], p["nn"], mg, 3, 3)
    ref = composed_multigrid(mg, comp, "l1")
    ref.set_graph(graph)
    ref.set_reorder(reorder)
    z_ref = vcycle(ctx, ref, b)
    for _ in range(2):  # the capture and its replay
        z_new = vcycle(ctx, mg, b, z)
        assert np.array_equal(bits(z_new), bits(z_ref))
    assert not np.array_equal(z_new, z_old)
    Zr = torch.empty((3, n), dtype=torch.float64, device="cuda:0").T
    ref.apply(Zr, B)
    mg.apply(Z, B)
    ctx.synchronize()
    assert np.array_equal(bits(Z.cpu().numpy()), bits(Zr.cpu().numpy()))
    assert np.array_equal(bits(Z.cpu().numpy()[:, 0]), bits(vcycle(ctx, mg, B[:, 0].contiguous())))


# --------------------------------------------------------------- 5: smoothers

@pytest.mark.parametrize("smoother", ["jacobi", "l1", "sgs", "block", "chebyshev"])
def test_smoothers_rebuilt(ctx, smoother):
    p = elasticity(ctx, STALE["elements"])
    mg = build_elasticity(ctx, p, STALE["coarsest"], smoother)
    b = rhs(p["S"].shape[0])
    z_old = vcycle(ctx, mg, b)
    mg.refresh(p["A2"], p["nn"])
    ref = composed_multigrid(mg, compose(ctx, p["A2"], p["nn"], mg, 3, 3), smoother)
    z = vcycle(ctx, mg, b)
    assert np.array_equal(bits(z), bits(vcycle(ctx, ref, b)))
    assert not np.array_equal(z, z_old)


# ----------------------------------------------------- 6: failure is atomic

def test_failure_leaves_the_hierarchy_intact(ctx):
    F = fa()
    p = elasticity(ctx, STALE["elements"])
    S, nn = p["S"], p["nn"]
    mg = build_elasticity(ctx, p, STALE["coarsest"])
    b = rhs(S.shape[0])
    z0 = vcycle(ctx, mg, b)
    levels0 = [mg.level(l)[0].arrays() for l in range(mg.levels())]

    def unchanged():
        assert np.array_equal(bits(vcycle(ctx, mg, b)), bits(z0))
        for l, old in enumerate(levels0):
            assert all(np.array_equal(u, v) for u, v in zip(mg.level(l)[0].arrays(), old))

    def refused(A_new, near_null, status):
        with pytest.raises(F.AmgError) as e:
            mg.refresh(A_new, near_null)
        assert e.value.status == status, str(e.value)
        unchanged()

    # one column index changed (row 7's last entry moves one column up, or down at the edge)
    bad = p["S2"].copy()
    e = bad.indptr[8] - 1
    bad.indices[e] += 1 if bad.indices[e] + 1 < S.shape[0] else -1
    refused(F.SparseMatOp.from_arrays(ctx, *S.shape, bad.indptr, bad.indices, bad.data), nn, 1)
    # a zeroed diagonal block: block_jacobi's AMG_ERR_NOT_SPD
    zero = p["S2"].copy()
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    zero.data[(rows // 3 == 4) & (zero.indices // 3 == 4)] = 0.0
    refused(F.SparseMatOp.from_arrays(ctx, *S.shape, zero.indptr, zero.indices, zero.data), nn, 4)
    # another candidate count, another size
    refused(p["A2"], np.asfortranarray(nn[:, :2]), 1)
    small = F.SparseMatOp.laplace3d_7pt(ctx, 4, 4, 4)
    refused(small, np.ones((64, 3), order="F"), 1)
    # the failures recorded nothing; a good refresh still works and a bad one after it is refused too
    assert mg.refresh(p["A2"], nn)["recorded"]
    z0 = vcycle(ctx, mg, b)
    levels0 = [mg.level(l)[0].arrays() for l in range(mg.levels())]
    refused(F.SparseMatOp.from_arrays(ctx, *S.shape, zero.indptr, zero.indices, zero.data), nn, 4)
    # a hierarchy amg_sa_build did not make
    L = F.SparseMatOp.laplace3d_7pt(ctx, 8, 8, 8)
    box = F.sa_build_box(L, (8, 8, 8), (2, 2, 2), coarsest_dim=30)
    bb = rhs(512)
    zb = vcycle(ctx, box, bb)
    with pytest.raises(F.AmgError) as e:
        box.refresh(L, np.ones((512, 1), order="F"))
    assert e.value.status == 3
    assert np.array_equal(bits(vcycle(ctx, box, bb)), bits(zb))
    hand = composed_multigrid(mg, compose(ctx, p["A2"], nn, mg, 3, 3), "l1")
    with pytest.raises(F.AmgError) as e:
        hand.refresh(p["A2"], nn)
    assert e.value.status == 3
