"""Classical coarsening on the device (csrc/lsinterp.hip).

The gfx950 search kernel returns the host search's bits -- sets, weights, errors and
the per-size "none" flags -- on short lists (Gram matrix in LDS), on lists that
cross 64 candidates (entries recomputed from the staged rows), at k = 1 (singular
Gram matrices: the pseudo-inverse path) and k = 8, and on rows past a lowered list
cap, which take the host fallback and are counted, and on lists of 130 and 200
candidates at k = 16 (the 129..256 bin: one wave per block).  The candidate lists
have no device form: amg_ls_candidates runs the library's host BFS over the downloaded
pattern, and is checked here against the restated BFS; amg_ls_interpolation builds
the same P with the search on either side, unit rows for the C-points, and its Galerkin product is the numpy triple
product.  amg_cr_split keeps its invariants and its reported reduction is recomputed
from public pieces; amg_classical_build is its pieces composed, runs within the
project's tolerances of the C oracle on the downloaded hierarchy, beats the level-0
smoother under PCG, is the same hierarchy with the search on either side, and goes
through the block cycle bit for bit.  The levels below the first coarsening -- built
from Galerkin operators, with post-processed near-null vectors and long lists -- are
covered at 8^3: the whole hierarchy goes through the oracle and is the same with the
search on either side."""
import numpy as np
import pytest
import scipy.sparse as sp

import classical_restated as R

pytestmark = pytest.mark.gpu

M = 8  # the grid of the search cases: 7-point M^3


def fa():
    import faer_amg_amd
    return faer_amg_amd


@pytest.fixture(scope="module")
def grid():
    """7-point 8^3: matrix rows, the index-order MIS as C-points, candidate lists at
    depths 2 and 5, the thin-QR near-null [1, x, y, z]."""
    rows = R.laplace_rows(M, M, M)
    pt = R.index_order_mis(R.grid_rows(M, M, M))
    return {"rows": rows, "pt": pt, "nn": R.qr_near_null(M, M, M),
            "lists2": R.candidates(rows, pt, 2), "lists5": R.candidates(rows, pt, 5)}


def same_bits(host, device):
    for name, h, d in zip(("count", "cols", "w", "err"), host[:4], device[:4]):
        assert h.dtype == d.dtype and h.shape == d.shape, name
        assert h.tobytes() == d.tobytes(), name


def both(ctx, lists, nn, d, mi=3, max_list=0):
    F = fa()
    L = R.lists_to_scipy(lists)
    host = F.ls_search(L, nn, d, mi, where=0)
    device = F.ls_search(L, nn, d, mi, where=1, ctx=ctx, max_list=max_list)
    same_bits(host, device)
    assert host[4]["subsets"] == device[4]["subsets"]
    return host, device


def test_device_search_equals_host_on_short_lists(ctx, grid):
    host, device = both(ctx, grid["lists2"], grid["nn"], np.ones(4))
    nf = int((grid["pt"] != 1).sum())
    assert device[4] == {"device_rows": nf, "host_rows": 0, "longest_list": 6, "subsets": host[4]["subsets"]}
    assert (host[0][grid["pt"] != 1, 0] == 1).all()  # every F row found a singleton


def test_device_search_equals_host_across_64_candidates(ctx, grid):
    """The F rows of the slab z = 0 at depth 5: lists of 34..81 candidates, so both the
    Gram-in-LDS launches (<= 64) and the recomputing ones run; C(34, 2) = 561 and most
    other subset counts are no multiple of 64."""
    lists = [l if i < M * M else [] for i, l in enumerate(grid["lists5"])]
    lens = [len(l) for l in lists if l]
    assert min(lens) <= 64 < max(lens)
    assert any((n * (n - 1) // 2) % 64 for n in lens)
    host, device = both(ctx, lists, grid["nn"], np.array([1.0, 0.5, 2.0, 0.25]))
    assert device[4]["device_rows"] == len(lens) and device[4]["host_rows"] == 0
    assert (host[0][:M * M][grid["pt"][:M * M] != 1, 0] == 1).all()


@pytest.mark.parametrize("k", [1, 8])
def test_device_search_equals_host_for_k(ctx, grid, k):
    n = M ** 3
    if k == 1:  # a constant column: every Gram matrix of r >= 2 is singular
        nn, d = np.full((n, 1), 1.0), np.array([1.0])
    else:
        nn = np.asfortranarray(np.random.default_rng(8).uniform(0.5, 1.5, (n, k)))
        d = np.linspace(0.5, 2.0, k)
    host, _ = both(ctx, grid["lists2"], nn, d)
    if k == 1:
        f = grid["pt"] != 1
        assert (host[0][f, 0] == 1).all() and (host[2][f, 0, 0] == 1.0).all() and (host[3][f, 0] == 0.0).all()


def test_rows_past_the_list_cap_take_the_host_fallback(ctx, grid):
    lens = np.array([len(l) for l in grid["lists2"]])
    assert (lens > 4).any() and ((lens > 0) & (lens <= 4)).any()
    _, device = both(ctx, grid["lists2"], grid["nn"], np.ones(4), max_list=4)
    assert device[4]["host_rows"] == int((lens > 4).sum())
    assert device[4]["device_rows"] == int(((lens > 0) & (lens <= 4)).sum())


def test_device_search_with_four_per_row(ctx, grid):
    both(ctx, grid["lists2"], grid["nn"], np.ones(4), mi=4)


def test_device_search_equals_host_in_the_longest_bin(ctx):
    """Lists of 130 and 200 candidates at k = 16: the 129..256 launch, whose staged rows
    (200 x 16 doubles) leave room for one wave per block; C(200, 3) = 1 313 400 subsets."""
    n, k = 264, 16
    nn = np.asfortranarray(np.random.default_rng(16).uniform(0.5, 1.5, (n, k)))
    lists = [[] for _ in range(n)]
    lists[0] = list(range(64, 264))
    lists[1] = list(range(70, 200))
    lists[2] = [64, 100, 263]
    host, device = both(ctx, lists, nn, np.linspace(0.5, 2.0, k))
    assert device[4]["device_rows"] == 3 and device[4]["host_rows"] == 0 and device[4]["longest_list"] == 200
    assert host[0][0, 0] == 1


def test_device_search_rejects_what_it_cannot_take(ctx, grid):
    F = fa()
    L = R.lists_to_scipy(grid["lists2"])
    with pytest.raises(F.AmgError, match="k <= 16") as e:
        F.ls_search(L, np.ones((M ** 3, 17)), np.ones(17), 3, where=1, ctx=ctx)
    assert e.value.status == 3
    with pytest.raises(F.AmgError, match="needs a context"):
        F.ls_search(L, grid["nn"], np.ones(4), 3, where=1)


@pytest.mark.parametrize("depth", [2, 5])
def test_candidate_lists_equal_the_restated_bfs(ctx, grid, depth):
    F = fa()
    A = F.SparseMatOp.from_scipy(ctx, R.to_scipy(grid["rows"]))
    got = F.ls_candidates(A, grid["pt"], depth)
    want = R.lists_to_scipy(grid["lists%d" % depth])
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert (got.data == 1.0).all()


def test_candidate_lists_on_a_shuffled_numbering(ctx):
    F = fa()
    A = F.SparseMatOp.random7(ctx, 10, 10, 10, seed=3, window=0)
    S = A.to_scipy().tocsr()
    S.sort_indices()
    rows = [[(int(j), 1.0) for j in S.indices[S.indptr[i]:S.indptr[i + 1]]] for i in range(S.shape[0])]
    pt = R.index_order_mis(rows)
    got = F.ls_candidates(A, pt, 3)
    want = R.lists_to_scipy(R.candidates(rows, pt, 3))
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)


def test_ls_interpolation_is_the_pieces_and_its_rap_is_the_triple_product(ctx, grid):
    F = fa()
    n, pt, nn = M ** 3, grid["pt"], grid["nn"]
    As = R.to_scipy(grid["rows"])
    A = F.SparseMatOp.from_scipy(ctx, As)
    d = np.ones(4)
    cfg = dict(search_depth=1, depth_ls=1, max_interp=3)
    Ph, cnn_h, err_h = F.ls_interpolation(A, pt, nn, d, where=0, **cfg)
    Pd, cnn_d, err_d = F.ls_interpolation(A, pt, nn, d, where=1, **cfg)
    P = Ph.to_scipy().tocsr()
    Pdev = Pd.to_scipy().tocsr()
    assert np.array_equal(P.indptr, Pdev.indptr) and np.array_equal(P.indices, Pdev.indices)
    assert P.data.tobytes() == Pdev.data.tobytes() and err_h.tobytes() == err_d.tobytes()
    cpts = np.flatnonzero(pt == 1)
    assert P.shape == (n, len(cpts))
    assert np.array_equal(cnn_h, nn[cpts]) and np.array_equal(cnn_d, cnn_h)
    # the restatement's rows: unit rows for the C-points, the accepted weights elsewhere
    res = R.search(grid["lists2"], nn, d, 3)
    coarse = {int(c): q for q, c in enumerate(cpts)}
    for i in range(n):
        cols, vals = P.indices[P.indptr[i]:P.indptr[i + 1]], P.data[P.indptr[i]:P.indptr[i + 1]]
        if pt[i] == 1:
            assert cols.tolist() == [coarse[i]] and vals.tolist() == [1.0] and err_h[i] == 0.0
            continue
        found, btb = res[i]
        size = R.accept(found, btb, 1.2)
        assert size > 0
        assert cols.tolist() == [coarse[j] for j in found[size - 1][0]]
        assert vals.tobytes() == np.array(found[size - 1][1]).tobytes()
        assert err_h[i] == found[size - 1][2]
    # A_c = R (A P) from the device SpGEMMs against numpy: the same pattern, 1e-12 |row|_inf
    Ac = F.galerkin_rap(F.transpose(Ph), A, Ph).to_scipy().tocsr()
    ref = (P.T @ As @ P).tocsr()
    Ac.sort_indices()
    ref.sort_indices()
    assert np.array_equal(Ac.indptr, ref.indptr) and np.array_equal(Ac.indices, ref.indices)
    rowmax = np.abs(ref).max(axis=1).toarray().ravel()
    assert (np.abs(Ac.data - ref.data) <= 1e-12 * np.repeat(rowmax, np.diff(ref.indptr))).all()


# ------------------------------------------------------------------ the split, the level, the hierarchy

def _problem(ctx, m):
    """7-point m^3, the near-null [1, x, y, z] after a thin QR, create_weights"""
    F = fa()
    A = F.SparseMatOp.laplace3d_7pt(ctx, m, m, m)
    nn = R.qr_near_null(m, m, m)
    w = np.asarray(F.create_weights(A, nn), np.float64)
    return A, nn, w


def test_cr_split_invariants_and_its_reduction_from_public_pieces(ctx):
    import torch
    F = fa()
    m = 10
    n = m ** 3
    A, nn, w = _problem(ctx, m)
    G = F.strength_graph(A, nn, w, depth=1)
    cfg = F.ClassicalConfig()
    pt, nc, info = F.cr_split(A, G)
    print("cr_split 10^3:", {k: v for k, v in info.items() if k != "c_round"}, "C", nc,
          "F", int((pt == 0).sum()), "N", int((pt == 2).sum()))
    cpts = np.flatnonzero(pt == 1)
    assert nc == len(cpts) and 0 < nc < n and set(np.unique(pt)) <= {0, 1, 2}
    assert (np.diff(cpts) > 0).all()  # sorted and unique by construction of the labels
    assert info["stop"] in ("converged", "no_new_c", "max_cr_iters", "zero_vector")
    rounds = info["rounds"]
    assert 1 <= rounds <= cfg.max_cr_iters and len(info["c_per_round"]) == rounds
    assert info["c_per_round"][-1] == nc and (np.diff([0] + info["c_per_round"]) > 0).all()
    cround = info["c_round"]
    assert ((cround >= 0) == (pt == 1)).all() and cround.max() == rounds - 1
    assert [int((cround == r).sum()) for r in range(rounds)] == np.diff([0] + info["c_per_round"]).tolist()
    # the C-points of one round are independent in the graph: the one chosen first clears every
    # node its row lists, so (the graph is not symmetric) no two of a round list each other
    G = G.tocsr()
    listed = [set(G.indices[G.indptr[i]:G.indptr[i + 1]].tolist()) for i in range(n)]
    for i in cpts:
        assert not any(cround[j] == cround[i] and int(i) in listed[j] for j in listed[i])
    if info["stop"] == "converged":
        assert info["reduction"] <= cfg.target_convergence
    # the last round's reduction again, from public pieces
    S = A.to_scipy().tocsr()
    isf = (pt != 1).astype(float)
    Af = sp.diags(isf) @ S @ sp.diags(isf) + sp.diags(1.0 - isf)
    Afd = F.SparseMatOp.from_scipy(ctx, Af.tocsr())
    part, nparts, _ = F.partition_modularity(G, coarsening_factor=cfg.smoother_coarsening_factor)
    Mf = F.BlockSmoother(Afd, part, nparts)
    u = torch.as_tensor(isf, device="cuda:0")
    start = float(torch.linalg.vector_norm(u))
    t, z = torch.empty_like(u), torch.empty_like(u)
    for _ in range(cfg.relax_steps):
        Afd.apply(t, u)
        Mf.apply(z, t)
        ctx.synchronize()
        u = u - z
    red = (float(torch.linalg.vector_norm(u)) / start) ** (1.0 / cfg.relax_steps)
    assert abs(red - info["reduction"]) <= 1e-10 * red


def test_cr_split_guards(ctx):
    F = fa()
    A, nn, w = _problem(ctx, 6)
    G = F.strength_graph(A, nn, w, depth=1)
    _, _, one = F.cr_split(A, G, max_cr_iters=1, target_convergence=1e-9)
    assert one["rounds"] == 1 and one["stop"] == "max_cr_iters"
    pt, nc, many = F.cr_split(A, G, max_cr_iters=50, target_convergence=1e-9)
    assert many["stop"] in ("no_new_c", "zero_vector", "converged") and many["rounds"] < 50
    with pytest.raises(F.AmgError):
        F.cr_split(A, G, relax_steps=0)


def _hierarchy(mg):
    out = []
    for l in range(mg.levels()):
        Al, _, Rl, Pl = mg.level(l)
        out += [Al.arrays()] + ([Rl.arrays(), Pl.arrays()] if Rl is not None else [])
    return out


BUILD8 = dict(coarsest_dim=100)


@pytest.fixture(scope="module")
def built8(ctx):
    """The whole hierarchy of 7-point 8^3 (levels 512, 423, 148, 22), the search on the device"""
    F = fa()
    A, nn, w = _problem(ctx, M)
    return A, nn, w, F.classical_build(A, nn, w, where=1, **BUILD8)


def _oracle_parity(ctx, A, mg, seed):
    """One V-cycle within 1e-11 of the C oracle on the downloaded hierarchy and rho_k over
    10 stationary cycles within 1e-8 (+ the noise floor of the residual); the oracle levels."""
    import torch
    import oracle as O
    F = fa()
    n, nl = A.nrows, mg.levels()
    levels = []
    for l in range(nl):
        Al, _, Rl, Pl = mg.level(l)
        d = {"A": O.Csr.from_arrays(*Al.dims(), *Al.arrays()), "smoother": "chol" if l == nl - 1 else "l1"}
        if Rl is not None:
            d["R"] = O.Csr.from_arrays(*Rl.dims(), *Rl.arrays())
            d["P"] = O.Csr.from_arrays(*Pl.dims(), *Pl.arrays())
        levels.append(d)
    b = np.random.default_rng(seed).uniform(-1, 1, n)
    zref = O.Multigrid(levels).apply(b)
    bd = torch.as_tensor(b, device="cuda:0")
    z = torch.empty_like(bd)
    mg.apply(z, bd)
    ctx.synchronize()
    assert np.linalg.norm(z.cpu().numpy() - zref) <= 1e-11 * np.linalg.norm(zref)
    x = torch.zeros_like(bd)
    it, hist = F.stationary_solve(A, mg, bd, x, max_iter=11, rel_tol=1e-300)
    _, it_o, hist_o = O.stationary_solve(levels[0]["A"], O.Multigrid(levels), b, max_iter=11, rel_tol=1e-300)
    S = A.to_scipy()
    floor = np.finfo(float).eps * abs(S).sum(axis=1).max() * float(torch.max(torch.abs(x))) / np.max(np.abs(b))
    assert it == it_o == 11
    assert np.all(np.abs(hist - hist_o) <= 1e-8 * hist_o + floor)
    assert hist[-1] < hist[0]
    return b, bd, S


def test_whole_hierarchy_vcycle_parity(ctx, built8):
    """Every level of the 8^3 hierarchy, the ones built from Galerkin operators included,
    through the oracle: V-cycle 1e-11, rho_k 1e-8."""
    A, _, _, mg = built8
    assert mg.levels() >= 3
    _oracle_parity(ctx, A, mg, 21)


def test_whole_hierarchy_is_the_same_with_the_search_on_either_side(ctx, built8):
    """where 0 and where 1: every A, R and P of every level bit for bit (two coarsenings at
    least, so lists on Galerkin levels and near-null vectors after amg_nn_postprocess)."""
    F = fa()
    A, nn, w, mg = built8
    other = F.classical_build(A, nn, w, where=0, **BUILD8)
    host, dev = _hierarchy(other), _hierarchy(mg)
    assert len(host) == len(dev) >= 7  # A_0, and R, P, A per coarsening
    for a, b in zip(host, dev):
        assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))
    assert all(d["device_rows"] == 0 for d in other.classical_info)
    assert [d["host_rows"] + d["device_rows"] for d in other.classical_info] == \
        [d["host_rows"] + d["device_rows"] for d in mg.classical_info]


def test_classical_build_level_is_the_pieces_composed(ctx, built8):
    """P_0 and A_1 of amg_classical_build are amg_cr_split, amg_ls_interpolation and
    amg_galerkin_rap(P^T, A, P) of the pieces, bit for bit."""
    F = fa()
    A, nn, w, mg = built8
    sizes = [mg.level(l)[0].nrows for l in range(mg.levels())]
    print("classical 8^3: levels", sizes, mg.classical_info)
    assert mg.levels() >= 3 and all(a > b for a, b in zip(sizes, sizes[1:])) and sizes[-1] <= 100
    info = mg.classical_info  # one entry per coarsening: what ran where
    assert [d["rows"] for d in info] == sizes[:-1] and [d["coarse_rows"] for d in info] == sizes[1:]
    for d in info:
        assert d["device_rows"] + d["host_rows"] + d["coarse_rows"] <= d["rows"] and d["cr_rounds"] >= 1
        assert d["host_rows"] == 0 or d["longest_list"] > 256
    G = F.strength_graph(A, nn, w, depth=1)
    pt, nc, _ = F.cr_split(A, G)
    P, cnn, _ = F.ls_interpolation(A, pt, nn, w, where=1)
    assert P.ls_info["device_rows"] == mg.classical_info[0]["device_rows"] == int((pt != 1).sum())
    assert P.ls_info["host_rows"] == 0 and P.ls_info["longest_list"] == mg.classical_info[0]["longest_list"]
    Ac = F.galerkin_rap(F.transpose(P), A, P)
    A1, _, _, _ = mg.level(1)
    _, _, R0, P0 = mg.level(0)
    for X, Y in ((P0, P), (A1, Ac)):
        assert all(np.array_equal(u, v) for u, v in zip(X.arrays(), Y.arrays()))
    assert R0.dims() == (nc, M ** 3) and A1.dims() == (nc, nc)


# One coarsening at 16^3.  The Galerkin operators fill in (operator complexity 9.2 over the
# five levels 4096, 2537, 1066, 410, 10 this problem gets at the defaults), a depth-3 ball
# on a coarse level holds hundreds of C-points and the search there enumerates C(L, 3)
# subsets per row: the whole hierarchy takes minutes, on either side.  The whole hierarchy
# is built at 8^3 (test_classical_build_level_is_the_pieces_composed).
BUILD16 = dict(coarsest_dim=300, max_levels=2)


@pytest.fixture(scope="module")
def built16(ctx):
    F = fa()
    A, nn, w = _problem(ctx, 16)
    return A, nn, w, F.classical_build(A, nn, w, where=1, **BUILD16)


def test_classical_build_vcycle_parity_and_pcg(ctx, built16):
    """7-point 16^3: one V-cycle within 1e-11 of the C oracle on the downloaded hierarchy,
    rho_k over 10 stationary cycles within 1e-8, PCG to 1e-8 in fewer iterations than
    with the level-0 smoother alone."""
    import torch
    import oracle as O
    F = fa()
    A, nn, w, mg = built16
    n, nl = A.nrows, mg.levels()
    assert nl >= 2
    sizes = [mg.level(l)[0].nrows for l in range(nl)]
    nnz = [mg.level(l)[0].nnz for l in range(nl)]
    print("classical 16^3: levels", sizes, "operator complexity %.3f" % (sum(nnz) / nnz[0]))
    assert all(a > b for a, b in zip(sizes, sizes[1:]))
    b, bd, S = _oracle_parity(ctx, A, mg, 12)
    x = torch.zeros_like(bd)
    itp, _ = F.pcg_solve(A, mg, bd, x, max_iter=300, rel_tol=1e-8)
    its, _ = F.pcg_solve(A, F.new_l1(A), bd, torch.zeros_like(bd), max_iter=3000, rel_tol=1e-8)
    print("classical 16^3: PCG iterations", itp, "with the hierarchy,", its, "with L1 alone")
    assert itp < its
    assert np.linalg.norm(b - S @ x.cpu().numpy()) <= 1e-7 * np.linalg.norm(b)


def test_classical_build_host_and_device_search_give_the_same_hierarchy(ctx, built16):
    F = fa()
    A, nn, w, mg = built16
    host = _hierarchy(F.classical_build(A, nn, w, where=0, **BUILD16))
    dev = _hierarchy(mg)
    assert len(host) == len(dev) == 4  # A_0, R_0, P_0, A_1
    for a, b in zip(host, dev):
        assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


def test_block_cycle_through_the_classical_hierarchy(ctx, built16):
    """k = 8 columns through the block cycle: every column is the single-vector cycle, bit for bit."""
    import torch
    A, _, _, mg = built16
    n, k = A.nrows, 8
    B = torch.as_tensor(np.random.default_rng(3).uniform(-1, 1, (k, n)), device="cuda:0").T  # column-major n x k
    Z = torch.zeros((k, n), dtype=torch.float64, device="cuda:0").T
    mg.apply(Z, B)
    ctx.synchronize()
    for c in range(k):
        z = torch.empty(n, dtype=torch.float64, device="cuda:0")
        mg.apply(z, B[:, c].contiguous())
        ctx.synchronize()
        assert torch.equal(Z[:, c], z), c


def test_classical_build_rejects_what_it_cannot_take(ctx):
    F = fa()
    A, nn, w = _problem(ctx, 4)
    with pytest.raises(F.AmgError, match="above 4") as e:
        F.classical_build(A, nn, w, max_interp=5)
    assert e.value.status == 3
    with pytest.raises(F.AmgError, match="no aggregates") as e:
        F.classical_build(A, nn, w, smoother=3)
    assert e.value.status == 3
    mg = F.classical_build(A, nn, w, max_levels=1)  # no coarsening: the Cholesky solve alone
    assert mg.levels() == 1
    mg = F.classical_build(A, nn, w, coarsest_dim=1000)  # as amg_sa_build: one coarsening at least
    assert mg.levels() == 2
