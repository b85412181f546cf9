"""The device SA setup (csrc/sagraph.hip; amg_set_sa_setup(1)): the strength graph
and the MIS aggregation on the GPU.

Strength graph, checked two ways.  Bitwise against `restated_strength_graph` below:
oracle/sa_oracle.py::strength_graph's algorithm at depth 1 with its one expression
math.pow(t, 4.0) replaced by (t*t)*(t*t), which is what the device computes (every
other step is IEEE-exact on both sides).  And against the host amg_strength_graph:
the same pattern, weights within rtol 1e-14 -- pow(t, 4.0) and (t*t)*(t*t) differ by
<= 3 * 2^-53 + 0.52 ULP per dof edge; up to 9 merged terms and the division by gmax
stay under ~45 * 2^-53 ~ 5e-15.

Aggregation: amg_aggregate_mis_device equals the host amg_aggregate_mis exactly on the
same graph (the parallel rule decides what the greedy sweep decides; the tail is the
host's own code).

End to end under the policy: amg_sa_build is the device pieces composed (bitwise),
its V-cycle within the existing 1e-11 of oracle/amg_oracle.c on the same hierarchy,
PCG beats CG, amg_find_near_null returns an orthonormal basis, and the default policy
afterwards builds what it built before."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import oracle as O

pytestmark = pytest.mark.gpu


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


# ------------------------------------------------------------------ restatement

def restated_strength_graph(A, nn, w, block_size=1):
    """sa_oracle.strength_graph at depth 1 with wt = (t*t)*(t*t) for math.pow(t, 4.0)."""
    A = A.tocsr()
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
        cand = []
        for j in (int(j) for j in ci[rp[i]:rp[i + 1]] if j != i):
            a, b = min(i, j), max(i, j)
            x = 0.0
            for c in range(k):
                x += (NN[a][c] * w[c]) * NN[b][c]
            rho2 = (x * x) / (vn[a] * vn[b])
            cand.append((2.0 * math.sqrt(max(1.0 - rho2, 0.0)), j))
        cand.sort()
        out = []
        if cand:
            cand = cand[:max(len(cand) // 2, 1)]
            dmin, dmax = cand[0][0], cand[-1][0]
            for d, j in cand:
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


# ------------------------------------------------------------------ cases

def _banded(n, hb):
    """SPD, rows of up to 2 hb off-diagonal entries (beyond one wave's 256 candidates at hb = 160)."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    d = np.abs(i - j)
    M = np.where((d > 0) & (d <= hb), -1.0 / (1.0 + d), 0.0)
    M[np.arange(n), np.arange(n)] = 1.0 - M.sum(axis=1)
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


CASES = ("elast_const", "elast_rand", "laplace", "band_bs1", "band_bs2", "tiny")
_cache = {}


def case(ctx, name):
    """(A on the device, scipy A, near-null, weights, block size, host strength graph), built once."""
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
    elif name.startswith("band"):
        S, bs = _banded(640, 160), (1 if name == "band_bs1" else 2)
        A = F.SparseMatOp.from_scipy(ctx, S)
        rng = np.random.default_rng(5)
        nn, w = rng.standard_normal((640, 2)), rng.uniform(0.5, 2.0, 2)
    else:
        S, bs = _tiny(), 1
        A = F.SparseMatOp.from_scipy(ctx, S)
        nn, w = np.random.default_rng(9).standard_normal((6, 2)), [1.0, 0.7]
    nn = np.asfortranarray(nn)
    G = F.strength_graph(A, nn, w, depth=1, block_size=bs)
    _cache[name] = (A, S, nn, list(w), bs, G)
    return _cache[name]


# ------------------------------------------------------------------ strength graph

@pytest.mark.parametrize("name", CASES)
def test_strength_graph_device(ctx, name):
    A, S, nn, w, bs, G = case(ctx, name)
    D = fa().strength_graph_device(A, nn, w, block_size=bs)
    assert D.dims() == G.shape
    rp, ci, va = D.arrays()
    R = restated_strength_graph(S, nn, w, bs)
    assert np.array_equal(rp, R.indptr) and np.array_equal(ci, R.indices)
    assert np.array_equal(va.view(np.int64), R.data.view(np.int64))
    assert np.array_equal(rp, G.indptr) and np.array_equal(ci, G.indices)
    assert np.allclose(va, G.data, rtol=1e-14, atol=0.0)
    if name == "elast_rand":
        P = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=G.shape)
        assert (P != P.T).nnz > 0  # asymmetric pattern
    if name.startswith("band"):
        assert np.diff(S.indptr).max() - 1 > 256  # rows beyond one wave's candidates
    if name == "tiny":
        assert rp[1] - rp[0] == 0 and rp[2] - rp[1] == 1


def test_strength_graph_device_memory_kinds(ctx):
    """near_null from host memory and from device memory: the same bits."""
    import torch
    A, S, nn, w, bs, G = case(ctx, "elast_rand")
    a = fa().strength_graph_device(A, nn, w, block_size=bs).arrays()
    nd = torch.as_tensor(np.ascontiguousarray(nn.T), device="cuda:0").t()  # column-major n x k on the device
    assert nd.stride(0) == 1 and nd.is_cuda
    b = fa().strength_graph_device(A, nd, w, block_size=bs).arrays()
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    hn = torch.as_tensor(np.ascontiguousarray(nn.T)).t()  # the same block as a host tensor
    c = fa().strength_graph_device(A, hn, w, block_size=bs).arrays()
    assert all(np.array_equal(u, v) for u, v in zip(a, c))


# ------------------------------------------------------------------ aggregation

def agg_equal(ctx, G, max_passes=0):
    G = G.tocsr()
    G.sort_indices()
    agg_h, na_h = fa().aggregate_mis(G)
    Gd = fa().SparseMatOp.from_scipy(ctx, G)
    agg_d, na_d, info = fa().aggregate_mis_device(Gd, max_passes)
    assert na_d == na_h
    assert np.array_equal(agg_d, agg_h)
    return info


@pytest.mark.parametrize("name", CASES)
def test_aggregate_device_on_strength_graphs(ctx, name):
    G = case(ctx, name)[5]
    info = agg_equal(ctx, G)
    assert not info["fallback"] and info["passes"] >= 1 and info["roots"] >= 1
    # and on the device-built graph where it lies
    A, S, nn, w, bs, _ = case(ctx, name)
    D = fa().strength_graph_device(A, nn, w, block_size=bs)
    agg_d, na_d, _ = fa().aggregate_mis_device(D)
    agg_r, na_r = fa().aggregate_mis(restated_strength_graph(S, nn, w, bs))
    assert na_d == na_r and np.array_equal(agg_d, agg_r)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_aggregate_device_random_asymmetric(ctx, seed):
    """400 nodes, density 0.015, weights from {1/4, 1/2, 3/4} (tie-heavy degrees), an empty row."""
    rng = np.random.default_rng(100 + seed)
    n = 400
    M = (rng.random((n, n)) < 0.015) * rng.choice([0.25, 0.5, 0.75], size=(n, n))
    np.fill_diagonal(M, 0.0)
    M[7, :] = 0.0    # listed by others, lists nobody
    M[:, 11] = 0.0   # listed by nobody
    G = sp.csr_matrix(M)
    assert (G != G.T).nnz > 0 and np.diff(G.indptr).min() == 0
    info = agg_equal(ctx, G)
    assert not info["fallback"]


def _sync_rounds(G):
    """Rounds of the parallel rule when every round reads the previous round's states."""
    G = G.tocsr()
    n = G.shape[0]
    deg = np.array([G.data[G.indptr[i]:G.indptr[i + 1]].sum() for i in range(n)])
    T = G.T.tocsr()
    H = []
    for v in range(n):
        us = T.indices[T.indptr[v]:T.indptr[v + 1]]
        H.append([u for u in us if u != v and (deg[u] > deg[v] or (deg[u] == deg[v] and u < v))])
    state = np.zeros(n, np.int8)
    rounds = 0
    while (state == 0).any():
        new = state.copy()
        for v in np.flatnonzero(state == 0):
            s = state[H[v]]
            if (s == 1).any():
                new[v] = 2
            elif (s == 2).all():
                new[v] = 1
        state = new
        rounds += 1
    return rounds


def test_aggregate_device_grid_unit_weights(ctx):
    """12^3 7-point adjacency, unit weights: priority is by index among equal degrees; tens of passes."""
    e = lambda m: sp.diags([np.ones(m - 1), np.ones(m - 1)], [-1, 1])  # noqa: E731
    I = sp.identity(12)
    G = (sp.kron(sp.kron(I, I), e(12)) + sp.kron(sp.kron(I, e(12)), I) + sp.kron(sp.kron(e(12), I), I)).tocsr()
    assert G.shape == (1728, 1728) and set(np.unique(G.data)) == {1.0}
    info = agg_equal(ctx, G)
    rounds = _sync_rounds(G)
    # a pass sees at least what a synchronous round sees (decisions are final and made in place)
    assert rounds >= 10 and not info["fallback"]
    assert 2 <= info["passes"] <= rounds, (info, rounds)


def test_aggregate_device_path_graph_falls_back(ctx):
    """A 200-node path needs about one pass per node; past max_passes = 8 the host sweep
    runs on the downloaded graph: the same aggregates."""
    n = 200
    G = sp.diags([np.ones(n - 1), np.ones(n - 1)], [-1, 1]).tocsr()
    info = agg_equal(ctx, G, max_passes=8)
    assert info["fallback"] and info["passes"] == 8
    assert info["roots"] >= n // 3
    full = agg_equal(ctx, G)  # the default budget decides it on the device
    assert not full["fallback"] and full["passes"] > 8 and full["roots"] == info["roots"]


# ------------------------------------------------------------------ end to end

def elasticity(ctx, elements, seed=11):
    H = fa().elasticity_q1(elements, seed=seed)
    return H.upload(ctx), H.to_scipy()


def weights(S, nn):
    return [1.0 / float(nn[:, c] @ (S @ nn[:, c])) for c in range(nn.shape[1])]


def build(ctx, elements, coarsest=150):
    A, S = elasticity(ctx, elements)
    nn = fa().constant_candidates(S.shape[0], 3)
    mg = fa().smoothed_aggregation(A, nn, weights=weights(S, nn), block_size=3, candidate_dimension=3,
                                   coarsest_dim=coarsest, smoother="l1")
    return A, S, nn, mg


def hierarchy_arrays(mg):
    out = []
    for l in range(mg.levels()):
        Al, _, Rl, Pl = mg.level(l)
        out += [Al.arrays()] + ([Rl.arrays(), Pl.arrays()] if Rl is not None else [])
    return out


def test_sa_build_device_equals_composition(ctx, device_setup):
    """Under the policy amg_sa_build's first level is the device pieces composed: bitwise in P_0 and A_1."""
    A, S, nn, mg = build(ctx, (5, 4, 4))
    assert mg.levels() >= 2
    G = fa().strength_graph_device(A, nn, weights(S, nn), block_size=3)
    agg, na, info = fa().aggregate_mis_device(G)
    assert not info["fallback"]
    P, cnn = fa().sa_tentative_block(ctx, agg, na, nn, block_size=3)
    Ps = fa().block_jacobi(A, P, 3)
    Ac = fa().galerkin_rap(fa().transpose(Ps), A, Ps)
    A1, _, _, _ = mg.level(1)
    _, _, R0, P0 = mg.level(0)
    for X, Y in ((P0, Ps), (A1, Ac)):
        assert all(np.array_equal(u, v) for u, v in zip(X.arrays(), Y.arrays()))
    assert R0.dims() == (na * 3, S.shape[0])


def test_sa_device_vcycle_parity_and_pcg(ctx, device_setup):
    """Elasticity (8,6,6), L1, built under the policy: one V-cycle within 1e-11 of the oracle
    on the same hierarchy; PCG to 1e-8 in fewer iterations than unpreconditioned CG."""
    import torch
    A, S, nn, mg = build(ctx, (8, 6, 6))
    n = S.shape[0]
    assert mg.levels() >= 2
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
    x = torch.zeros_like(bd)
    itp, _ = fa().pcg_solve(A, mg, bd, x, max_iter=300, rel_tol=1e-8)
    itc, _ = fa().pcg_solve(A, None, bd, torch.zeros_like(bd), max_iter=3000, rel_tol=1e-8)
    assert itp < itc
    assert np.linalg.norm(b - S @ x.cpu().numpy()) <= 1e-7 * np.linalg.norm(b)


def test_find_near_null_device(ctx, device_setup):
    A, S = elasticity(ctx, (5, 4, 4))
    X, cfs = fa().find_near_null(A, 3, iters=10, seed=4, block_size=3)
    X = np.asarray(X)
    assert np.max(np.abs(X.T @ X - np.eye(3))) <= 1e-12
    assert np.all(np.isfinite(cfs)) and np.all(cfs > 0)


def test_policy_flipped_back_builds_the_host_hierarchy(ctx):
    """Host policy before, device policy in between, host policy after: the first and the last
    hierarchies are bitwise equal (the policy leaves nothing behind)."""
    assert fa().get_sa_setup() == 0
    before = hierarchy_arrays(build(ctx, (5, 4, 4))[3])
    fa().set_sa_setup(1)
    try:
        between = hierarchy_arrays(build(ctx, (5, 4, 4))[3])
    finally:
        fa().set_sa_setup(0)
    after = hierarchy_arrays(build(ctx, (5, 4, 4))[3])
    assert len(before) == len(after) and len(between) >= 3
    for a, b in zip(before, after):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
