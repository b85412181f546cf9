"""The device strength graph at BFS depth > 1 (csrc/sagraph.hip: k_ball,
ball_pattern_device, strength_graph_device with a depth; amg_set_sa_setup(1) at any
strength_depth).

The ball primitive: amg_pattern_ball_device equals the pattern of (pattern(A) + I)^depth
with the diagonal removed, computed here with scipy in int64 (entries reset to 1 after
every product) or, for the dense bands, with a float32 matmul whose sums (<= 2049) are
exact.  The cases meet the wave kernel's cap of 256 members exactly, pass it by a few,
meet the workgroup kernel's cap of 4096 exactly and pass it (AMG_ERR_UNSUPPORTED, never a
truncated ball).

The strength graph at depth 2 and 3, checked two ways as tests/test_gpu_sa_device.py
checks depth 1.  Bitwise against `restated_strength_graph` below: that file's
restatement with the candidates of a row taken from its ball and everything else the
same.  And against the host amg_strength_graph(depth): the same pattern, weights within
rtol 1e-14 -- the bound derived there still holds: a node pair still merges at most bs^2
terms, the division by gmax is unchanged and pow(t, 4.0) against (t*t)*(t*t) differs per
dof edge as before.

End to end under the policy: amg_sa_build at strength_depth 2 and 3 reports level 0 built
on the device and is the device pieces composed (bitwise), its V-cycle within the
existing 1e-11 of oracle/amg_oracle.c on the same hierarchy; a level whose ball passes
the cap falls back to the host (reason 2) and builds policy 0's hierarchy bitwise;
amg_find_near_null returns an orthonormal basis; the default policy afterwards builds
what it built before."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import oracle as O

pytestmark = pytest.mark.gpu

UNSUPPORTED = 3


def fa():
    import faer_amg_amd
    return faer_amg_amd


@pytest.fixture
def device_setup():
    fa().set_sa_setup(1)
    try:
        yield
    finally:
        fa().set_sa_setup(0)


# ------------------------------------------------------------------ references

def ball_ref(S, depth):
    """Pattern of (pattern(S) + I)^depth without its diagonal, as CSR with sorted columns."""
    n = S.shape[0]
    M = sp.csr_matrix((np.ones(S.nnz, np.int64), S.indices, S.indptr), shape=S.shape) + sp.identity(n, np.int64, "csr")
    M.data[:] = 1
    if n <= 5000 and M.nnz > 200 * n:  # a dense band: float32 sums of <= n ones are exact
        D = M.toarray().astype(np.float32)
        R = D
        for _ in range(depth - 1):
            R = ((R @ D) > 0).astype(np.float32)
        R = R > 0
        np.fill_diagonal(R, False)
        B = sp.csr_matrix(R)
    else:
        R = M
        for _ in range(depth - 1):
            R = (R @ M).tocsr()
            R.data[:] = 1  # int64 counts never grow: no wrap at any depth
        B = R.tolil()
        B.setdiag(0)
        B = B.tocsr()
        B.eliminate_zeros()
    B.sort_indices()
    return B


def restated_strength_graph(A, nn, w, block_size=1, cand=None):
    """tests/test_gpu_sa_device.py's restatement (sa_oracle.strength_graph with
    wt = (t*t)*(t*t) for math.pow(t, 4.0)); the candidates of row i are the columns of
    row i of `cand` other than i (None: A itself, depth 1)."""
    A = (A if cand is None else cand).tocsr()
    n = A.shape[0]
    NN = np.asarray(nn, np.float64).reshape(n, -1).tolist()
    k = len(NN[0])
    w = [float(v) for v in w]

    def vnorm(i):
        s = 0.0
        for c in range(k):
            s += (NN[i][c] * w[c]) * NN[i][c]
        return max(s, 1e-30)

    vn = [vnorm(i) for i in range(n)]
    rp, ci = A.indptr, A.indices
    dof = []
    for i in range(n):
        cand_i = []
        for j in (int(j) for j in ci[rp[i]:rp[i + 1]] if j != i):
            a, b = min(i, j), max(i, j)
            x = 0.0
            for c in range(k):
                x += (NN[a][c] * w[c]) * NN[b][c]
            rho2 = (x * x) / (vn[a] * vn[b])
            cand_i.append((2.0 * math.sqrt(max(1.0 - rho2, 0.0)), j))
        cand_i.sort()
        out = []
        if cand_i:
            cand_i = cand_i[:max(len(cand_i) // 2, 1)]
            dmin, dmax = cand_i[0][0], cand_i[-1][0]
            for d, j in cand_i:
                if abs(dmax - dmin) < 1e-12:
                    wt = 1.0
                else:
                    t = (dmax - d) / (dmax - dmin + 1e-12)
                    wt = (t * t) * (t * t)
                out.append((j, wt))
            out.sort(key=lambda e: e[0])
        dof.append(out)
    if block_size == 1:
        return _lists_to_csr(dof, n)
    nnodes = n // block_size
    node, lmax = [], []
    for I in range(nnodes):
        cat = []
        for r in range(block_size):
            cat += [(j // block_size, v) for j, v in dof[I * block_size + r]]
        cat.sort(key=lambda e: e[0])  # stable: (dof ascending, column ascending) within an id
        out = []
        for j, v in cat:
            if out and out[-1][0] == j:
                out[-1] = (j, out[-1][1] + v)
            else:
                out.append((j, v))
        node.append(out)
        lmax.append(max([v for _, v in out], default=0.0))
    gmax = max(lmax)
    return _lists_to_csr([[(j, v / gmax) for j, v in out if j != I] for I, out in enumerate(node)], nnodes)


def _lists_to_csr(lists, n):
    rp = np.zeros(n + 1, np.int64)
    for i, l in enumerate(lists):
        rp[i + 1] = rp[i] + len(l)
    ci = np.array([j for l in lists for j, _ in l], np.int64)
    va = np.array([v for l in lists for _, v in l], np.float64)
    return sp.csr_matrix((va, ci, rp), shape=(n, n))


# ------------------------------------------------------------------ patterns

def _banded(n, hb):
    """SPD, rows of up to 2 hb off-diagonal entries; its depth-d ball is the band of d hb."""
    i = np.arange(n)
    d = np.abs(i[:, None] - i[None, :])
    M = np.where((d > 0) & (d <= hb), -1.0 / (1.0 + d), 0.0)
    M[i, i] = 1.0 - M.sum(axis=1)
    S = sp.csr_matrix(M)
    S.sort_indices()
    return S


def _tiny():
    """6 rows: row 0 stores its diagonal only, row 1 one off-diagonal entry (keep = 1)."""
    rows = {0: [0], 1: [1, 4], 2: [0, 1, 2, 3, 5], 3: [1, 2, 3, 4], 4: [0, 2, 3, 4, 5], 5: [2, 3, 4, 5]}
    r = [i for i, cs in rows.items() for _ in cs]
    c = [j for cs in rows.values() for j in cs]
    v = [4.0 if i == j else -1.0 for i, j in zip(r, c)]
    S = sp.csr_matrix((v, (r, c)), shape=(6, 6))
    S.sort_indices()
    return S


def _laplace7(nx, ny, nz):
    e = lambda m: sp.diags([-np.ones(m - 1), -np.ones(m - 1)], [-1, 1])  # noqa: E731
    I = sp.identity
    S = (sp.kron(sp.kron(I(nz), I(ny)), e(nx)) + sp.kron(sp.kron(I(nz), e(ny)), I(nx))
         + sp.kron(sp.kron(e(nz), I(ny)), I(nx)) + 6.0 * sp.identity(nx * ny * nz)).tocsr()
    S.sort_indices()
    return S


def _random_asym(n=400, density=0.015, seed=31):
    """Asymmetric, a stored diagonal everywhere but row 7, which stores nothing at all."""
    rng = np.random.default_rng(seed)
    M = rng.random((n, n)) < density
    np.fill_diagonal(M, True)
    M[7, :] = False
    S = sp.csr_matrix(M.astype(np.float64))
    S.sort_indices()
    return S


def _stride(n=1 << 15, links=(1, 3, 1024, 2048, 4096, 8192)):
    """i ~ i +- s for every stride s (no wrap), with a diagonal: column ids of a ball differ by
    multiples of 1024, which a masked hash would send to one slot."""
    i = np.arange(n)
    r, c = [i], [i]
    for s in links:
        r += [i[:-s], i[s:]]
        c += [i[:-s] + s, i[s:] - s]
    r, c = np.concatenate(r), np.concatenate(c)
    S = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))
    S.sort_indices()
    return S


def _star(hubs=70, leaves=70):
    """Node 0, `hubs` hubs tied to it, `leaves` leaves per hub: graph Laplacian + I (SPD)."""
    n = 1 + hubs + hubs * leaves
    r, c = [], []
    for h in range(hubs):
        hub = 1 + h
        r += [0, hub]
        c += [hub, 0]
        for l in range(leaves):
            leaf = 1 + hubs + h * leaves + l
            r += [hub, leaf]
            c += [leaf, hub]
    Adj = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))
    S = (sp.diags(np.asarray(Adj.sum(axis=1)).ravel() + 1.0) - Adj).tocsr()
    S.sort_indices()
    return S


_pat = {}


def pattern(ctx, name):
    """(A on the device, scipy A), built once per name."""
    if name not in _pat:
        kind, *arg = name.split(":")
        if kind == "lap":
            S = _laplace7(*(int(v) for v in arg[0].split("x")))
        elif kind == "tiny":
            S = _tiny()
        elif kind == "rand":
            S = _random_asym()
        elif kind == "band":
            S = _banded(int(arg[0]), int(arg[1]))
        elif kind == "stride":
            S = _stride()
        else:
            S = _star()
        _pat[name] = (fa().SparseMatOp.from_scipy(ctx, S), S)
    return _pat[name]


def ball_arrays(ctx, name, depth):
    A, S = pattern(ctx, name)
    B = fa().pattern_ball_device(A, depth)
    assert B.dims() == S.shape
    rp, ci, va = B.arrays()
    assert (va == 1.0).all()
    return rp, ci, S


# ------------------------------------------------------------------ the ball primitive

def check_ball(ctx, name, depth):
    rp, ci, S = ball_arrays(ctx, name, depth)
    R = ball_ref(S, depth)
    assert np.array_equal(rp, R.indptr)
    assert np.array_equal(ci, R.indices)
    return np.diff(rp), R


@pytest.mark.parametrize("depth", [2, 3, 5])
@pytest.mark.parametrize("dims,longest", [("5x4x3", 59), ("9x8x7", 209)])
def test_ball_seven_point(ctx, dims, longest, depth):
    sizes, _ = check_ball(ctx, "lap:" + dims, depth)
    if depth == 5:
        assert sizes.max() == longest  # the wave kernel alone (<= 256)
    assert sizes.max() <= 256


def test_ball_tiny_diagonal_only_row(ctx):
    sizes, _ = check_ball(ctx, "tiny", 2)
    assert sizes[0] == 0  # row 0 stores only its diagonal: an empty ball
    assert sizes[1] > 1


def test_ball_random_asymmetric(ctx):
    sizes, R = check_ball(ctx, "rand", 2)
    assert (R != R.T).nnz > 0
    assert sizes[7] == 0 and np.diff(pattern(ctx, "rand")[1].indptr)[7] == 0  # the row that stores nothing


def test_ball_meets_the_wave_cap(ctx):
    sizes, _ = check_ball(ctx, "band:640:64", 2)
    assert sizes.max() == 256 and (sizes == 256).sum() == 384


def test_ball_both_kernels_in_one_call(ctx):
    sizes, _ = check_ball(ctx, "band:640:65", 2)
    assert sizes.max() == 260 and (sizes > 256).sum() == 386 and (sizes <= 256).sum() == 254


def test_ball_workgroup_rows(ctx):
    sizes, _ = check_ball(ctx, "band:640:100", 2)
    assert sizes.min() == 200 and sizes.max() == 400 and (sizes > 256).sum() == 526


def test_ball_depth3_past_the_wave_cap(ctx):
    sizes, _ = check_ball(ctx, "band:640:43", 3)
    assert sizes.max() == 258


def test_ball_meets_the_workgroup_cap(ctx):
    sizes, _ = check_ball(ctx, "band:4200:1024", 2)
    assert sizes.max() == 4096 and (sizes == 4096).sum() == 104


def test_ball_past_the_workgroup_cap_is_refused(ctx):
    A, S = pattern(ctx, "band:4200:1025")
    sizes = np.diff(ball_ref(S, 2).indptr)
    assert (sizes > 4096).sum() == 106
    with pytest.raises(fa().AmgError) as e:
        fa().pattern_ball_device(A, 2)
    assert e.value.status == UNSUPPORTED and "4096" in str(e.value)


@pytest.mark.parametrize("depth,lo,hi", [(2, 33, 65), (3, 100, 187)])
def test_ball_stride_graph(ctx, depth, lo, hi):
    sizes, _ = check_ball(ctx, "stride", depth)
    assert sizes.min() == lo and sizes.max() == hi


def test_ball_star(ctx):
    A, S = pattern(ctx, "star")
    assert S.shape[0] == 4971
    with pytest.raises(fa().AmgError) as e:
        fa().pattern_ball_device(A, 2)  # row 0 reaches all 4970 others
    assert e.value.status == UNSUPPORTED
    rp, ci, _ = ball_arrays(ctx, "star", 1)
    P = S.copy().tolil()
    P.setdiag(0)
    P = P.tocsr()
    P.eliminate_zeros()
    P.sort_indices()
    assert np.array_equal(rp, P.indptr) and np.array_equal(ci, P.indices)  # depth 1: the pattern itself


@pytest.mark.parametrize("name,depth", [("band:640:65", 2), ("stride", 3), ("rand", 2)])
def test_ball_twice_the_same(ctx, name, depth):
    a = ball_arrays(ctx, name, depth)[:2]
    b = ball_arrays(ctx, name, depth)[:2]
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_ball_dimension_error(ctx):
    S = sp.csr_matrix(np.ones((3, 4)))
    with pytest.raises(fa().AmgError) as e:
        fa().pattern_ball_device(fa().SparseMatOp.from_scipy(ctx, S), 2)
    assert e.value.status == 2  # AMG_ERR_DIM


# ------------------------------------------------------------------ strength graph

CASES = ("elast_const", "elast_rand", "laplace", "tiny")
_cache = {}


def case(ctx, name):
    """(A on the device, scipy A, near-null, weights, block size), built once."""
    if name in _cache:
        return _cache[name]
    F = fa()
    if name.startswith("elast"):
        H = F.elasticity_q1((4, 3, 3), seed=11)
        A, S, bs = H.upload(ctx), H.to_scipy(), 3
        if name == "elast_const":  # distances tie throughout (the 1.0 branch where a row keeps one value)
            nn = F.constant_candidates(S.shape[0], 3)
            w = [1.0 / float(nn[:, c] @ (S @ nn[:, c])) for c in range(3)]
        else:  # the power branch; the kept pattern is asymmetric
            rng = np.random.default_rng(21)
            nn, w = rng.standard_normal((S.shape[0], 4)), rng.uniform(0.5, 2.0, 4)
    elif name == "laplace":
        A = F.SparseMatOp.laplace3d_7pt(ctx, 5, 4, 3)
        S, bs = A.to_scipy(), 1
        nn, w = np.random.default_rng(3).standard_normal((S.shape[0], 2)), [1.0, 0.5]
    elif name.startswith("band65"):
        A, S = pattern(ctx, "band:640:65")
        bs = 1 if name == "band65_bs1" else 2
        rng = np.random.default_rng(5)
        nn, w = rng.standard_normal((640, 2)), rng.uniform(0.5, 2.0, 2)
    elif name == "band4200":
        A, S = pattern(ctx, "band:4200:1024")
        bs = 1
        rng = np.random.default_rng(6)
        nn, w = rng.standard_normal((4200, 2)), rng.uniform(0.5, 2.0, 2)
    else:
        S, bs = _tiny(), 1
        A = F.SparseMatOp.from_scipy(ctx, S)
        nn, w = np.random.default_rng(9).standard_normal((6, 2)), [1.0, 0.7]
    _cache[name] = (A, S, np.asfortranarray(nn), list(w), bs)
    return _cache[name]


_ref = {}


def restated(ctx, name, depth):
    """The restated graph of a case at a depth, computed once and left unchanged."""
    if (name, depth) not in _ref:
        _, S, nn, w, bs = case(ctx, name)
        S = S.tocsr()
        S.sort_indices()
        _ref[name, depth] = restated_strength_graph(S, nn, w, bs, cand=ball_ref(S, depth))
    return _ref[name, depth]


def check_against_host(ctx, name, depth, D):
    A, S, nn, w, bs = case(ctx, name)
    G = fa().strength_graph(A, nn, w, depth=depth, block_size=bs)
    rp, ci, va = D.arrays()
    assert D.dims() == G.shape
    assert np.array_equal(rp, G.indptr) and np.array_equal(ci, G.indices)
    assert np.allclose(va, G.data, rtol=1e-14, atol=0.0)


STRENGTH = [(n, d) for n in CASES for d in (2, 3)] + [("band65_bs1", 2), ("band65_bs2", 2)]


@pytest.mark.parametrize("name,depth", STRENGTH)
def test_strength_graph_device_depth(ctx, name, depth):
    A, S, nn, w, bs = case(ctx, name)
    D = fa().strength_graph_device(A, nn, w, block_size=bs, depth=depth)
    rp, ci, va = D.arrays()
    R = restated(ctx, name, depth)
    assert np.array_equal(rp, R.indptr) and np.array_equal(ci, R.indices)
    assert np.array_equal(va.view(np.int64), R.data.view(np.int64))
    check_against_host(ctx, name, depth, D)
    if name == "tiny":
        assert rp[1] - rp[0] == 0  # the diagonal-only row has no candidates at any depth


def test_strength_graph_device_depth_at_the_cap(ctx):
    """Banded 4200 / 1024 at depth 2 (rows of exactly 4096 candidates): too slow to restate in
    pure Python, so against the host graph alone."""
    A, S, nn, w, bs = case(ctx, "band4200")
    D, info = fa().strength_graph_device(A, nn, w, block_size=bs, depth=2, info=True)
    assert info["longest_ball"] == 4096 and info["block_rows"] == 4200 and info["wave_rows"] == 0
    check_against_host(ctx, "band4200", 2, D)


def test_strength_graph_device_depth_info(ctx):
    A, S, nn, w, bs = case(ctx, "band65_bs2")
    D, info = fa().strength_graph_device(A, nn, w, block_size=bs, depth=2, info=True)
    sizes = np.diff(ball_ref(S, 2).indptr)
    assert info["longest_ball"] == 260
    assert info["wave_rows"] == 254 and info["block_rows"] == 386  # both ball kernels ran
    assert info["ball_entries"] == sizes.sum()
    assert info["dof_entries"] == np.maximum(sizes // 2, 1).sum()
    assert info["node_edges"] == D.nnz
    # two calls: the same bits
    E = fa().strength_graph_device(A, nn, w, block_size=bs, depth=2)
    assert all(np.array_equal(u, v) for u, v in zip(D.arrays(), E.arrays()))


def test_strength_graph_device_depth_one_is_todays(ctx):
    A, S, nn, w, bs = case(ctx, "elast_rand")
    a = fa().strength_graph_device(A, nn, w, block_size=bs).arrays()
    b = fa().strength_graph_device(A, nn, w, block_size=bs, depth=1).arrays()
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    r = restated_strength_graph(S, nn, w, bs)
    assert np.array_equal(a[2].view(np.int64), r.data.view(np.int64))


def test_strength_graph_device_byte_budget(ctx):
    A, S, nn, w, bs = case(ctx, "laplace")
    with pytest.raises(fa().AmgError) as e:
        fa().strength_graph_device(A, nn, w, block_size=bs, depth=2, max_bytes=1)
    assert e.value.status == UNSUPPORTED and "byte budget" in str(e.value)
    sizes = np.diff(ball_ref(S, 2).indptr)
    need = 4 * sizes.sum() + 8 * (S.shape[0] + 1) + 12 * np.maximum(sizes // 2, 1).sum()
    fa().strength_graph_device(A, nn, w, block_size=bs, depth=2, max_bytes=int(need))  # exactly enough
    with pytest.raises(fa().AmgError):
        fa().strength_graph_device(A, nn, w, block_size=bs, depth=2, max_bytes=int(need) - 1)


def test_strength_graph_device_ball_cap(ctx):
    A, S = pattern(ctx, "star")
    nn = np.asfortranarray(np.random.default_rng(2).standard_normal((S.shape[0], 2)))
    with pytest.raises(fa().AmgError) as e:
        fa().strength_graph_device(A, nn, [1.0, 0.5], depth=2)
    assert e.value.status == UNSUPPORTED and "4096" in str(e.value)


@pytest.mark.parametrize("name,depth", [("elast_rand", 2), ("laplace", 3), ("band65_bs2", 2)])
def test_aggregate_device_on_depth_graphs(ctx, name, depth):
    A, S, nn, w, bs = case(ctx, name)
    D = fa().strength_graph_device(A, nn, w, block_size=bs, depth=depth)
    agg_d, na_d, _ = fa().aggregate_mis_device(D)
    agg_r, na_r = fa().aggregate_mis(restated(ctx, name, depth))
    assert na_d == na_r and np.array_equal(agg_d, agg_r)


# ------------------------------------------------------------------ end to end

def weights(S, nn):
    return [1.0 / float(nn[:, c] @ (S @ nn[:, c])) for c in range(nn.shape[1])]


def build_elast(ctx, depth, elements=(5, 4, 4), coarsest=150):
    H = fa().elasticity_q1(elements, seed=11)
    A, S = H.upload(ctx), H.to_scipy()
    nn = fa().constant_candidates(S.shape[0], 3)
    mg = fa().smoothed_aggregation(A, nn, weights=weights(S, nn), block_size=3, candidate_dimension=3,
                                   coarsest_dim=coarsest, smoother="l1", strength_depth=depth)
    return A, S, nn, mg


def build_laplace(ctx, depth):
    A = fa().SparseMatOp.laplace3d_7pt(ctx, 9, 8, 7)
    S = A.to_scipy()
    nn = np.asfortranarray(1.0 + 0.1 * np.random.default_rng(8).random((S.shape[0], 1)))
    mg = fa().smoothed_aggregation(A, nn, weights=weights(S, nn), block_size=1, candidate_dimension=1,
                                   coarsest_dim=40, smoother="l1", strength_depth=depth)
    return A, S, nn, mg


def hierarchy_arrays(mg):
    out = []
    for l in range(mg.levels()):
        Al, _, Rl, Pl = mg.level(l)
        out += [Al.arrays()] + ([Rl.arrays(), Pl.arrays()] if Rl is not None else [])
    return out


def vcycle_within_oracle(ctx, mg, n):
    import torch
    levels = []
    nl = mg.levels()
    for l in range(nl):
        Al, _, Rl, Pl = mg.level(l)
        d = {"A": O.Csr.from_arrays(*Al.dims(), *Al.arrays()), "smoother": "chol" if l == nl - 1 else "l1"}
        if Rl is not None:
            d["R"] = O.Csr.from_arrays(*Rl.dims(), *Rl.arrays())
            d["P"] = O.Csr.from_arrays(*Pl.dims(), *Pl.arrays())
        levels.append(d)
    b = np.random.default_rng(12).uniform(-1, 1, n)
    zref = O.Multigrid(levels).apply(b)
    bd = torch.as_tensor(b, device="cuda:0")
    z = torch.empty_like(bd)
    mg.apply(z, bd)
    ctx.synchronize()
    assert np.linalg.norm(z.cpu().numpy() - zref) <= 1e-11 * np.linalg.norm(zref)


def test_sa_build_depth2_elasticity_is_the_device_pieces(ctx, device_setup):
    A, S, nn, mg = build_elast(ctx, 2)
    assert mg.levels() >= 2
    info = mg.sa_level_info(0)
    assert info[5] == 1 and info[6] == 0 and info[7] > 0  # on the device, no reason, a ball was counted
    assert info[:3] == (S.shape[0], 3, S.shape[0] // 3)
    G, gi = fa().strength_graph_device(A, nn, weights(S, nn), block_size=3, depth=2, info=True)
    assert info[4] == G.nnz and info[7] == gi["longest_ball"]
    agg, na, ai = fa().aggregate_mis_device(G)
    assert not ai["fallback"] and info[3] == na
    P, _ = fa().sa_tentative_block(ctx, agg, na, nn, block_size=3)
    Ps = fa().block_jacobi(A, P, 3)
    Ac = fa().galerkin_rap(fa().transpose(Ps), A, Ps)
    A1, _, _, _ = mg.level(1)
    _, _, _, P0 = mg.level(0)
    for X, Y in ((P0, Ps), (A1, Ac)):
        assert all(np.array_equal(u, v) for u, v in zip(X.arrays(), Y.arrays()))
    vcycle_within_oracle(ctx, mg, S.shape[0])
    with pytest.raises(fa().AmgError):
        mg.sa_level_info(mg.levels() - 1)  # one record per coarsening step


def test_sa_build_depth3_seven_point_is_the_device_pieces(ctx, device_setup):
    A, S, nn, mg = build_laplace(ctx, 3)
    assert mg.levels() >= 2
    info = mg.sa_level_info(0)
    assert info[5] == 1 and info[6] == 0
    assert info[7] == np.diff(ball_ref(S, 3).indptr).max()
    G = fa().strength_graph_device(A, nn, weights(S, nn), block_size=1, depth=3)
    agg, na, ai = fa().aggregate_mis_device(G)
    assert not ai["fallback"] and info[3] == na
    P, _ = fa().sa_tentative_block(ctx, agg, na, nn, block_size=1)
    Ps = fa().smooth_interpolation(A, P, 0.66)
    Ac = fa().galerkin_rap(fa().transpose(Ps), A, Ps)
    A1, _, _, _ = mg.level(1)
    _, _, _, P0 = mg.level(0)
    for X, Y in ((P0, Ps), (A1, Ac)):
        assert all(np.array_equal(u, v) for u, v in zip(X.arrays(), Y.arrays()))
    vcycle_within_oracle(ctx, mg, S.shape[0])


def build_star(ctx):
    A, S = pattern(ctx, "star")
    nn = fa().constant_candidates(S.shape[0], 1)
    return fa().smoothed_aggregation(A, nn, weights=weights(S, nn), block_size=1, candidate_dimension=1,
                                     max_levels=2, smoother="l1", strength_depth=2)


def test_sa_build_ball_past_the_cap_keeps_the_host(ctx):
    assert fa().get_sa_setup() == 0
    host = build_star(ctx)
    assert host.levels() == 2
    assert host.sa_level_info(0)[5:7] == (0, 1)  # on the host by policy
    fa().set_sa_setup(1)
    try:
        dev = build_star(ctx)
    finally:
        fa().set_sa_setup(0)
    info = dev.sa_level_info(0)
    assert info[5] == 0 and info[6] == 2 and info[7] > 4096  # the ball cap; the count is a lower bound
    a, b = hierarchy_arrays(host), hierarchy_arrays(dev)
    assert len(a) == len(b) == 4  # A_0, R_0, P_0, A_1
    for x, y in zip(a, b):
        assert all(np.array_equal(u, v) for u, v in zip(x, y))


def test_find_near_null_device_depth2(ctx, device_setup):
    H = fa().elasticity_q1((5, 4, 4), seed=11)
    A = H.upload(ctx)
    X, cfs = fa().find_near_null(A, 3, iters=10, seed=4, block_size=3, strength_depth=2)
    X = np.asarray(X)
    assert np.max(np.abs(X.T @ X - np.eye(3))) <= 1e-12
    assert np.all(np.isfinite(cfs)) and np.all(cfs > 0)


def test_policy_flipped_back_builds_the_host_hierarchy_at_depth2(ctx):
    """Host policy before, device policy in between, host policy after, all at depth 2: the
    first and the last hierarchies are bitwise equal (the policy leaves nothing behind)."""
    assert fa().get_sa_setup() == 0
    before = hierarchy_arrays(build_elast(ctx, 2)[3])
    fa().set_sa_setup(1)
    try:
        between = build_elast(ctx, 2)[3]
        assert between.sa_level_info(0)[5] == 1
    finally:
        fa().set_sa_setup(0)
    mg = build_elast(ctx, 2)[3]
    assert mg.sa_level_info(0)[5:8] == (0, 1, 0)
    after = hierarchy_arrays(mg)
    assert len(before) == len(after) >= 3
    for a, b in zip(before, after):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
