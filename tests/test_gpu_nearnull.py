"""The device near-null search (nearnull.hip: amg_thin_qr, amg_smooth_vectors,
amg_create_weights, amg_find_near_null) against numpy restatements of
adaptivity.rs:264-390, 434-443.

The restatement of the thin QR is np.linalg.qr with the columns of Q flipped so
that R's diagonal is positive (Q is then unique for a full-rank block).

Tolerances: 1e-12 absolute on orthonormal-column quantities (the project's bound
for LAPACK-compared bases, tests/test_gpu_sa.py); R to 1e-12 of its largest
entry; convergence factors to 1e-10 relative.  Every test prints the figures it
asserts on.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

gpu = pytest.mark.gpu
TOL = 1e-12


def fa():
    import faer_amg_amd
    return faer_amg_amd


def np_thin_qr(X):
    Q, R = np.linalg.qr(X)
    s = np.where(np.diag(R) < 0, -1.0, 1.0)
    return Q * s, R * s[:, None]


def np_smooth(S, pc, X0, iters):
    """smooth_vector (adaptivity.rs:307-390); pc maps an n x k block to M^-1 block."""
    X = np_thin_qr(np_thin_qr(X0)[0])[0]
    for _ in range(iters):
        X = np_thin_qr(X - pc(S @ X))[0]
    return X, np_cfs(S, pc, X)


def np_cfs(S, pc, X):
    AW = S @ X
    EV = X - pc(AW)
    return np.sqrt(np.einsum("ij,ij->j", EV, S @ EV)) / np.sqrt(np.einsum("ij,ij->j", X, AW))


def handle_apply(pc):
    def f(B):
        B = np.asfortranarray(B)
        return pc.apply(np.zeros_like(B, order="F"), B)
    return f


def device_block(X, ld=None, pad=7.5):
    """X (numpy n x k) as a column-major torch device view with leading dimension ld."""
    import torch
    n, k = X.shape
    ld = n if ld is None else ld
    buf = torch.full((k, ld), pad, dtype=torch.float64, device="cuda:0")
    buf[:, :n] = torch.as_tensor(np.ascontiguousarray(X.T), device="cuda:0")
    return buf, buf[:, :n].t()


# ------------------------------------------------------------------ CPU only


def test_block_arguments_rejected_without_a_device():
    """The argument checks run before anything touches a device."""
    L = fa().lib()
    x = np.zeros((70, 65), order="F")
    p = x.ctypes.data_as(C.c_void_p)
    assert L.amg_thin_qr(None, p, 70, 70, 65, None, 0) == 3      # k = 65: UNSUPPORTED
    assert L.amg_thin_qr(None, p, 70, 10, 20, None, 0) == 2      # n < k: DIM
    assert L.amg_thin_qr(None, p, 9, 10, 5, None, 0) == 1        # ld < n: INVALID
    assert L.amg_thin_qr(None, p, 70, 70, 0, None, 0) == 1       # k = 0
    assert L.amg_thin_qr(None, None, 70, 70, 4, None, 0) == 1    # null block
    assert L.amg_thin_qr(None, p, 70, 70, 4, None, 0) == 1       # null context
    assert b"null context" in L.amg_last_error()
    assert L.amg_smooth_vectors(None, None, p, 70, 4, 1, None, 0) == 1
    assert L.amg_create_weights(None, p, 70, 4, p, 0) == 1
    assert L.amg_find_near_null(None, p, 70, 4, 1, 1, 1, None, 0) == 1


# ------------------------------------------------------------------ thin QR


@gpu
@pytest.mark.parametrize("n,k,where,pad", [(64, 64, "host", 0), (4099, 1, "host", 0), (4099, 3, "device", 0),
                                           (4099, 17, "device", 5), (4099, 33, "host", 0), (70001, 64, "device", 0)])
def test_thin_qr_against_lapack(ctx, n, k, where, pad):
    X = np.random.default_rng(1).standard_normal((n, k))
    Qr, Rr = np_thin_qr(X)
    if where == "host":
        Q, R = fa().thin_qr(ctx, np.asfortranarray(X))
    else:
        buf, view = device_block(X, n + pad)
        Qd, R = fa().thin_qr(ctx, view, in_place=True)
        ctx.synchronize()
        assert Qd.data_ptr() == buf.data_ptr()
        Q = Qd.cpu().numpy()
        assert bool((buf[:, n:] == 7.5).all())  # the padding rows of an ld > n buffer are untouched
    dq, dr = np.max(np.abs(Q - Qr)), np.max(np.abs(R - Rr)) / np.max(np.abs(Rr))
    orth = np.max(np.abs(Q.T @ Q - np.eye(k)))
    print(f"thin_qr n={n} k={k} {where}: |Q-Qref|={dq:.2e} |R-Rref|/max={dr:.2e} |QtQ-I|={orth:.2e}")
    assert dq <= TOL
    assert dr <= TOL
    assert orth <= TOL
    assert np.all(np.tril(R, -1) == 0.0) and np.all(np.diag(R) > 0.0)


def ill_conditioned(n, k):
    rng = np.random.default_rng(2)
    U = np.linalg.qr(rng.standard_normal((n, k)))[0]
    V = np.linalg.qr(rng.standard_normal((k, k)))[0]
    return np.asfortranarray(U @ np.diag(np.logspace(0, -10, k)) @ V.T)


@gpu
@pytest.mark.parametrize("n,k", [(3000, 16), (4099, 33)])
def test_thin_qr_ill_conditioned_takes_the_fallback(ctx, n, k):
    X = ill_conditioned(n, k)
    Q, R = fa().thin_qr(ctx, X)
    orth = np.max(np.abs(Q.T @ Q - np.eye(k)))
    res = np.linalg.norm(Q @ R - X) / np.linalg.norm(X)
    print(f"thin_qr kappa=1e10 n={n} k={k}: |QtQ-I|={orth:.2e} |QR-X|_F/|X|_F={res:.2e}")
    assert orth <= TOL
    assert res <= TOL
    assert np.all(np.tril(R, -1) == 0.0) and np.all(np.diag(R) > 0.0)


@gpu
def test_thin_qr_rank_deficient_is_invalid(ctx):
    X = np.asfortranarray(np.random.default_rng(3).standard_normal((500, 6)))
    X[:, 4] = X[:, 1]
    with pytest.raises(fa().AmgError) as e:
        fa().thin_qr(ctx, X)
    assert e.value.status == 1 and "rank deficient" in str(e.value)


@gpu
def test_thin_qr_errors_and_determinism(ctx):
    F = fa()
    with pytest.raises(F.AmgError) as e:
        F.thin_qr(ctx, np.zeros((70, 65), order="F"))
    assert e.value.status == 3
    with pytest.raises(F.AmgError) as e:
        F.thin_qr(ctx, np.zeros((10, 20), order="F"))
    assert e.value.status == 2
    x = np.ones((10, 5), order="F")
    assert F.lib().amg_thin_qr(ctx.h, x.ctypes.data_as(C.c_void_p), 9, 10, 5, None, 0) == 1
    X = np.asfortranarray(np.random.default_rng(4).standard_normal((4099, 33)))
    Q1, R1 = F.thin_qr(ctx, X.copy(order="F"))
    Q2, R2 = F.thin_qr(ctx, X.copy(order="F"))
    assert np.array_equal(Q1, Q2) and np.array_equal(R1, R2)
    Y = ill_conditioned(3000, 16)
    Q1, R1 = F.thin_qr(ctx, Y.copy(order="F"))
    Q2, R2 = F.thin_qr(ctx, Y.copy(order="F"))
    assert np.array_equal(Q1, Q2) and np.array_equal(R1, R2)


# ------------------------------------------------------------ smooth_vectors

_matrices = {}


def matrix(ctx, name):
    """(operator, scipy copy), built once per session."""
    if name not in _matrices:
        F = fa()
        if name == "lap765":
            A = F.SparseMatOp.laplace3d_7pt(ctx, 7, 6, 5)
        elif name == "lap121110":
            A = F.SparseMatOp.laplace3d_7pt(ctx, 12, 11, 10)
        else:
            A = F.SparseMatOp.random7(ctx, 9, 8, 7)
        _matrices[name] = (A, A.to_scipy().tocsr())
    return _matrices[name]


def diag_pc(A, S, kind):
    if kind == "l1":
        return fa().new_l1(A), 1.0 / np.asarray(abs(S).sum(axis=1)).ravel()
    return fa().new_jacobi(A, 0.66), 0.66 / S.diagonal()


@gpu
@pytest.mark.parametrize("iters", [0, 1, 10])
@pytest.mark.parametrize("kind", ["l1", "jacobi"])
@pytest.mark.parametrize("name,k", [("lap765", 4), ("lap121110", 16), ("random7", 8)])
def test_smooth_vectors_diagonal(ctx, name, k, kind, iters):
    A, S = matrix(ctx, name)
    pc, d = diag_pc(A, S, kind)
    X0 = np.random.default_rng(5).standard_normal((S.shape[0], k))
    apply = lambda B: d[:, None] * B
    Xr, cr = np_smooth(S, apply, X0, iters)
    X, cfs = fa().smooth_vectors(A, pc, X0=X0, iters=iters)
    dx = np.max(np.abs(X - Xr))
    dc = np.max(np.abs(cfs / cr - 1.0))
    dn = np.max(np.abs(cfs / np_cfs(S, apply, X) - 1.0))
    print(f"smooth_vectors {name} k={k} {kind} iters={iters}: |X-Xref|={dx:.2e} "
          f"|cfs/ref-1|={dc:.2e} |cfs/numpy(X)-1|={dn:.2e} cfs in [{cfs.min():.3f}, {cfs.max():.3f}]")
    assert dx <= TOL
    assert dc <= 1e-10
    assert dn <= 1e-10
    X2, cfs2 = fa().smooth_vectors(A, pc, X0=X0, iters=iters)
    assert np.array_equal(X, X2) and np.array_equal(cfs, cfs2)


@gpu
def test_smooth_vectors_device_block_and_seed(ctx):
    """A torch device start block gives the host path's bits; seed draws default_rng(seed)."""
    A, S = matrix(ctx, "lap765")
    pc = fa().new_l1(A)
    X0 = np.random.default_rng(6).standard_normal((S.shape[0], 4))
    Xh, ch = fa().smooth_vectors(A, pc, X0=X0, iters=3)
    _, view = device_block(X0)
    Xd, cd = fa().smooth_vectors(A, pc, X0=view, iters=3)
    ctx.synchronize()
    assert np.array_equal(Xd.cpu().numpy(), Xh) and np.array_equal(cd, ch)
    assert np.array_equal(view.cpu().numpy(), X0)  # the start block is left alone
    Xs, cs = fa().smooth_vectors(A, pc, k=4, iters=3, seed=6)
    assert np.array_equal(Xs, Xh) and np.array_equal(cs, ch)


@gpu
@pytest.mark.parametrize("kind", ["sgs", "block"])
def test_smooth_vectors_generic_preconditioner(ctx, kind):
    A, S = matrix(ctx, "lap765")
    if kind == "sgs":
        pc = fa().SymGaussSeidel(A)
    else:
        x, y, z = np.meshgrid(np.arange(7), np.arange(6), np.arange(5), indexing="ij")
        box = (x // 2) + 4 * ((y // 2) + 3 * (z // 2))  # 2 x 2 x 2 boxes, row = x + 7 (y + 6 z)
        part = np.transpose(box, (2, 1, 0)).ravel()
        pc = fa().BlockSmoother(A, part)
    X0 = np.random.default_rng(7).standard_normal((S.shape[0], 4))
    Xr, cr = np_smooth(S, handle_apply(pc), X0, 3)
    X, cfs = fa().smooth_vectors(A, pc, X0=X0, iters=3)
    dx, dc = np.max(np.abs(X - Xr)), np.max(np.abs(cfs / cr - 1.0))
    print(f"smooth_vectors {kind}: |X-Xref|={dx:.2e} |cfs/ref-1|={dc:.2e}")
    assert dx <= TOL
    assert dc <= 1e-10


# ------------------------------------------- weights, find_near_null, end to end


@gpu
def test_create_weights(ctx):
    H = fa().elasticity_q1((4, 3, 3), seed=11)
    A, S = H.upload(ctx), H.to_scipy()
    X = np.asfortranarray(np.random.default_rng(8).standard_normal((S.shape[0], 5)))
    w = fa().create_weights(A, X)
    ref = np.array([1.0 / float(X[:, c] @ (S @ X[:, c])) for c in range(5)])
    print(f"create_weights: max rel err {np.max(np.abs(w / ref - 1.0)):.2e}")
    assert np.allclose(w, ref, rtol=1e-12, atol=0.0)
    _, view = device_block(X)
    assert np.array_equal(fa().create_weights(A, view), w)
    X[:, 2] *= -0.0  # x^T A x = 0 is not positive
    with pytest.raises(fa().AmgError) as e:
        fa().create_weights(A, X)
    assert e.value.status == 4


@gpu
def test_find_near_null_is_its_composition(ctx):
    F = fa()
    H = F.elasticity_q1((4, 4, 3), seed=11)
    A = H.upload(ctx)
    n, k, iters = A.nrows, 6, 5
    X0 = np.random.default_rng(0).standard_normal((n, k))
    X, cfs = F.find_near_null(A, k, iters=iters, seed=0, block_size=3, strength_depth=1)
    basis, _ = F.smooth_vectors(A, F.new_l1(A), X0=X0, iters=iters)
    w = F.create_weights(A, basis)
    agg, na = F.aggregate_mis(F.strength_graph(A, basis, w, depth=1, block_size=3))
    B = F.BlockSmoother(A, agg, na, block_size=3)
    Xc, cc = F.smooth_vectors(A, B, X0=X0, iters=iters)
    dx, dc = np.max(np.abs(X - Xc)), np.max(np.abs(cfs / cc - 1.0))
    print(f"find_near_null vs composition: |X-Xc|={dx:.2e} |cfs/cc-1|={dc:.2e} aggregates={na} cfs={cfs}")
    assert dx <= TOL
    assert dc <= 1e-10
    assert np.max(np.abs(X.T @ X - np.eye(k))) <= TOL


@gpu
def test_end_to_end_scaled_laplacian(ctx, dev):
    """A bare SPD matrix -> found candidates -> SA hierarchy -> PCG.  The constant
    vector is no near-null vector of S A S; the search finds S^-1 1."""
    import torch
    F = fa()
    L = F.SparseMatOp.laplace3d_7pt(ctx, 12, 11, 10).to_scipy().tocsr()
    n = L.shape[0]
    s = 10.0 ** np.random.default_rng(9).uniform(-1.0, 1.0, n)
    M = (sp.diags(s) @ L @ sp.diags(s)).tocsr()
    M.sort_indices()
    A = F.SparseMatOp.from_scipy(ctx, M)
    X, cfs = F.find_near_null(A, 3, iters=20, seed=0)
    mg = F.smoothed_aggregation(A, X, weights=F.create_weights(A, X), coarsest_dim=100)
    mgc = F.smoothed_aggregation(A, F.constant_candidates(n, 1), coarsest_dim=100)
    b = torch.as_tensor(np.random.default_rng(10).uniform(-1.0, 1.0, n), device=dev)
    its = {}
    for name, pc in (("found", mg), ("constant", mgc), ("none", None)):
        x = torch.zeros_like(b)
        its[name], hist = F.pcg_solve(A, pc, b, x, max_iter=5000, rel_tol=1e-8)
        ctx.synchronize()
        res = np.linalg.norm(b.cpu().numpy() - M @ x.cpu().numpy()) / np.linalg.norm(b.cpu().numpy())
        print(f"pcg {name}: {its[name]} iterations, true residual {res:.2e}")
        if name == "found":
            assert its[name] <= 5000 and res <= 1e-7
    print(f"end to end: iterations {its}, stage-2 cfs {cfs}")
    assert its["found"] <= its["none"]
