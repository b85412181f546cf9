"""The modularity partitioner on the device (csrc/partition.hip).

amg_partition_modularity_device equals the host amg_partition_modularity exactly --
aggregates, counts, rounds, improvement passes, swaps -- on uploaded graphs (the
cases of tests/modularity_restated.py, which tests/test_partition_host.py pins to
the restatement) and on amg_strength_graph_device output; past the pass budget and
past the row-length bound the host finishes with the same result.  Under
amg_set_sa_partitioner(1), for both setup policies, amg_sa_build is the pieces
composed (bitwise), its V-cycle is within the existing 1e-11 of oracle/amg_oracle.c
on the same downloaded hierarchy, and PCG converges; a cf-128 partition gives the
BlockSmoother blocks of about 128 rows; the default policy afterwards builds what
it built before."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import modularity_restated as R
import oracle as O

pytestmark = pytest.mark.gpu


def fa():
    import faer_amg_amd
    return faer_amg_amd


@pytest.fixture
def modularity():
    fa().set_sa_partitioner(1)
    try:
        yield
    finally:
        fa().set_sa_partitioner(0)
        fa().set_sa_setup(0)


def both(ctx, G, **cfg):
    """host and device partitions of the scipy graph G, asserted equal; the device info"""
    F = fa()
    G = G.tocsr()
    agg_h, na_h, ih = F.partition_modularity(G, **cfg)
    Gd = F.SparseMatOp.from_scipy(ctx, G)
    agg_d, na_d, idev = F.partition_modularity_device(Gd, **cfg)
    assert na_d == na_h
    assert np.array_equal(agg_d, agg_h)
    for key in ("rounds", "improvement_passes", "swaps", "min_agg", "max_agg"):
        assert idev[key] == ih[key], key
    return idev


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_device_partitioner_equals_host(ctx, name):
    make, cfg = R.CASES[name]
    info = both(ctx, R.to_scipy(make()), **cfg)
    assert not info["fallback"]
    assert info["passes"] >= info["rounds"] and info["max_passes_in_round"] <= info["passes"]
    if info["rounds"]:
        assert info["max_passes_in_round"] >= 1


def _random_coefficient_operator(m, seed):
    """7-point operator on m^3 with random positive edge coefficients, shifted to be SPD"""
    rng = np.random.default_rng(seed)
    G = R.to_scipy(R.grid_rows(m, m, m, lower_only=True))
    G.data = rng.uniform(0.1, 10.0, G.nnz)
    W = G + G.T
    A = sp.diags(np.asarray(W.sum(axis=1)).ravel() + 0.01) - W
    A = A.tocsr()
    A.sort_indices()
    return A


def test_device_partitioner_on_device_strength_graphs(ctx):
    F = fa()
    S = _random_coefficient_operator(12, 31)
    A = F.SparseMatOp.from_scipy(ctx, S)
    rng = np.random.default_rng(3)
    nn, w = np.asfortranarray(rng.standard_normal((S.shape[0], 2))), [1.0, 0.5]
    H = F.elasticity_q1((6, 6, 6), seed=11)
    E, Es = H.upload(ctx), H.to_scipy()
    en, ew = np.asfortranarray(rng.standard_normal((Es.shape[0], 4))), list(rng.uniform(0.5, 2.0, 4))
    for op, cand, wts, bs in ((A, nn, w, 1), (E, en, ew, 3)):
        Gd = F.strength_graph_device(op, cand, wts, block_size=bs)
        agg_d, na_d, idev = F.partition_modularity_device(Gd)
        G = Gd.to_scipy()
        assert (G != G.T).nnz > 0  # each row keeps its strongest half: not symmetric
        agg_h, na_h, ih = F.partition_modularity(G)
        assert na_d == na_h and np.array_equal(agg_d, agg_h)
        assert (idev["rounds"], idev["improvement_passes"], idev["swaps"]) == \
            (ih["rounds"], ih["improvement_passes"], ih["swaps"])
        assert not idev["fallback"]
        n = G.shape[0]
        assert math.floor(n / 8.0) - 2 <= na_d <= n / 8.0


def test_pass_budget_of_one_finishes_on_the_host(ctx):
    G = R.to_scipy(R.grid_rows(12, 12, 12))
    info = both(ctx, G, max_passes=1)
    assert info["fallback"] and info["passes"] == 1 and info["max_passes_in_round"] == 1
    full = both(ctx, G)
    assert not full["fallback"] and full["max_passes_in_round"] > 1


def test_hub_row_takes_the_wave_proposals(ctx):
    """Node 0 lists 300 neighbours: past the 64 entries one lane proposes for."""
    rows = R.hub_rows()
    assert len(rows[0]) == 300
    info = both(ctx, R.to_scipy(rows))
    assert not info["fallback"] and info["max_agg"] > 1
    both(ctx, R.to_scipy(rows), coarsening_factor=32.0, agg_size_penalty=0.0)


def test_row_beyond_the_bound_partitions_on_the_host(ctx):
    """A 4100-entry row: the device function hands the graph to the host partitioner."""
    rows = R.hub_rows(n=4200, spokes=4100)
    info = both(ctx, R.to_scipy(rows), coarsening_factor=64.0, max_improvement_iters=2)
    assert info["fallback"] and info["passes"] == 0


def _arrow(n):
    """SPD with one dof row of n - 1 off-diagonal entries (beyond the device strength graph's 4096)"""
    T = sp.diags([-np.ones(n - 1), -np.ones(n - 1)], [-1, 1]).tolil()
    T[0, 1:] = -0.001
    T[1:, 0] = -0.001
    T = T.tocsr()
    A = (T + sp.diags(-np.asarray(T.sum(axis=1)).ravel() + 0.5)).tocsr()
    A.sort_indices()
    return A


def hierarchy_arrays(mg):
    out = []
    for l in range(mg.levels()):
        Al, _, Rl, Pl = mg.level(l)
        out += [Al.arrays()] + ([Rl.arrays(), Pl.arrays()] if Rl is not None else [])
    return out


def test_sa_build_row_beyond_the_bound_keeps_the_host_path(ctx, modularity):
    F = fa()
    S = _arrow(4200)
    assert np.diff(S.indptr).max() - 1 > 4096
    A = F.SparseMatOp.from_scipy(ctx, S)
    nn = np.ones((4200, 1))
    host = hierarchy_arrays(F.smoothed_aggregation(A, nn, coarsest_dim=1000, smoother="l1"))
    F.set_sa_setup(1)
    dev = hierarchy_arrays(F.smoothed_aggregation(A, nn, coarsest_dim=1000, smoother="l1"))
    assert len(host) == len(dev) >= 3
    for a, b in zip(host, dev):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))


def _elasticity_build(ctx, elements, coarsest):
    F = fa()
    H = F.elasticity_q1(elements, seed=11)
    A, S = H.upload(ctx), H.to_scipy()
    nn = F.constant_candidates(S.shape[0], 3)
    w = [1.0 / float(nn[:, c] @ (S @ nn[:, c])) for c in range(3)]
    mg = F.smoothed_aggregation(A, nn, weights=w, block_size=3, candidate_dimension=3, coarsest_dim=coarsest,
                                smoother="l1")
    return A, S, nn, w, mg


@pytest.mark.parametrize("setup", [0, 1])
def test_sa_build_under_modularity(ctx, modularity, setup):
    """amg_sa_build's first level is the pieces composed (bitwise in P_0 and A_1); one V-cycle
    within 1e-11 of the oracle on the downloaded hierarchy; PCG to 1e-8 beats plain CG."""
    import torch
    F = fa()
    F.set_sa_setup(setup)
    A, S, nn, w, mg = _elasticity_build(ctx, (8, 6, 6), 100)
    n = S.shape[0]
    nl = mg.levels()
    assert nl >= 2
    if setup:
        agg, na, info = F.partition_modularity_device(F.strength_graph_device(A, nn, w, block_size=3))
        assert not info["fallback"]
    else:
        agg, na, info = F.partition_modularity(F.strength_graph(A, nn, w, depth=1, block_size=3))
    nnodes = n // 3
    assert math.floor(nnodes / 8.0) - 2 <= na <= nnodes / 8.0
    P, _ = F.sa_tentative_block(ctx, agg, na, nn, block_size=3)
    Ps = F.block_jacobi(A, P, 3)
    Ac = F.galerkin_rap(F.transpose(Ps), A, Ps)
    A1, _, _, _ = mg.level(1)
    _, _, R0, P0 = mg.level(0)
    for X, Y in ((P0, Ps), (A1, Ac)):
        assert all(np.array_equal(u, v) for u, v in zip(X.arrays(), Y.arrays()))
    assert R0.dims() == (na * 3, n)
    levels = []
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
    itp, _ = F.pcg_solve(A, mg, bd, x, max_iter=300, rel_tol=1e-8)
    itc, _ = F.pcg_solve(A, None, bd, torch.zeros_like(bd), max_iter=3000, rel_tol=1e-8)
    assert itp < itc
    assert np.linalg.norm(b - S @ x.cpu().numpy()) <= 1e-7 * np.linalg.norm(b)


@pytest.mark.parametrize("setup", [0, 1])
def test_find_near_null_under_modularity(ctx, modularity, setup):
    F = fa()
    F.set_sa_setup(setup)
    H = F.elasticity_q1((5, 4, 4), seed=11)
    X, cfs = F.find_near_null(H.upload(ctx), 3, iters=10, seed=4, block_size=3)
    X = np.asarray(X)
    assert np.max(np.abs(X.T @ X - np.eye(3))) <= 1e-12
    assert np.all(np.isfinite(cfs)) and np.all(cfs > 0)


def test_block_smoother_on_a_cf128_partition(ctx):
    """20^3 grid at cf 128: about 62 blocks of about 128 rows; the BlockSmoother over them is SPD."""
    F = fa()
    n, cf = 8000, 128.0
    Gd = F.SparseMatOp.from_scipy(ctx, R.to_scipy(R.grid_rows(20, 20, 20)))
    agg, na, pinfo = F.partition_modularity_device(Gd, coarsening_factor=cf)
    assert not pinfo["fallback"]
    assert math.floor(n / cf) - 2 <= na <= n / cf  # so the mean block has 128 .. 133.4 rows
    A = F.SparseMatOp.laplace3d_7pt(ctx, 20, 20, 20)
    blk = F.BlockSmoother(A, agg, na)
    info = blk.info()
    assert info["nblocks"] == na
    assert info["max_block"] == pinfo["max_agg"] >= 128  # the largest is at least the mean
    M = blk.to_sparse().to_scipy().tocsr()
    assert abs(M - M.T).max() <= 1e-12 * abs(M).max()
    for a in range(na):
        idx = np.flatnonzero(agg == a)
        assert np.linalg.eigvalsh(M[idx][:, idx].toarray()).min() > 0.0


def test_partitioner_policy_reset_builds_what_it_built(ctx):
    """MIS before, modularity in between, MIS after: the first and the last hierarchies are
    bitwise equal, and the one in between has other aggregates."""
    F = fa()
    assert F.get_sa_partitioner()[0] == 0
    before = hierarchy_arrays(_elasticity_build(ctx, (5, 4, 4), 150)[4])
    F.set_sa_partitioner(1)
    try:
        between = hierarchy_arrays(_elasticity_build(ctx, (5, 4, 4), 150)[4])
    finally:
        F.set_sa_partitioner(0)
    after = hierarchy_arrays(_elasticity_build(ctx, (5, 4, 4), 150)[4])
    assert len(before) == len(after) and len(between) >= 3
    for a, b in zip(before, after):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert between[1][0].shape != before[1][0].shape or not np.array_equal(between[1][1], before[1][1])
