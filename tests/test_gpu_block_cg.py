"""The coupled block CG (amg_block_cg_solve; solve.cpp block_cg_impl, kernels in
bcg.hip) and its two kernel primitives (amg_block_gram, amg_block_gemm_update).

The checker of the solver is `model_bcg` below: a numpy float64 restatement of the
algorithm in include/amg.h.  It computes A on the host from amg_csr_download; M is
the library's existing block apply of the same handle (tested elsewhere, not the
code under test).  The model's reductions (the Gram products and the norms) exist in
two summation orders -- plain `@`, and row blocks of 64 (8 at n = 27, where one block of 64
would be the plain order again) summed in order -- and the
spread between the two runs is the yardstick of every comparison that is not a
bound: the GPU's reduction tree is a third order, not a worse one, and is allowed
100 times the spread (the 100 covers the amplification that two orders only sample)
with a floor of 1e-12.

Blocks are column-major torch views with ldb = n + 3 and ldx = n + 1 (odd leading
dimensions: columns that are only 8-byte aligned); the padding holds 7.5 and must
stay untouched.  B is normals (seed 5) with: k >= 3: column 1 zero with a zero
guess; k > 3: the last column equals column 2 and column 3 is scaled by 1e-9;
k >= 8: column 5 = 2 col 0 - 3 col 4.  A random guess keeps the same relations, so
the start residual has them too: the first rank is k minus the dropped columns.
These inputs put every pivot of the rank-revealing Cholesky either at O(1) or at
rounding level, a factor 100 and more from rank_tol = 2^-26 on either side (asserted
of the model first): between summation orders a pivot moves by a relative n k eps /
pivot at the most, so the kept set cannot differ.

The kernel primitives are checked against numpy longdouble references with derived
bounds: |C - C_ref| <= 4 n eps (|X|^T |Y|) for the Gram product (n products, each
rounded once, summed in some order: n eps would do for one order, 4 covers the
blocked tree's partial sums), |Y - Y_ref| <= (w + 2) eps (|Y0| + |X| |C|) for the
update (an fma chain of w terms and one addition).
"""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu
PAD = 7.5
INVALID, DIM, UNSUPPORTED = 1, 2, 3
EPS = np.finfo(np.float64).eps
RANK_TOL = 2.0 ** -26

GRIDS = {
    "3": (3, 3, 3),            # n = 27: below one wave, fewer rows than columns at k = 32
    "12x11x10": (12, 11, 10),  # n = 1320
    "17": (17, 17, 17),        # n = 4913, odd: ragged last block
    "72x64x64": (72, 64, 64),  # n = 294912 > 1024 * 256: several 64-row steps per workgroup of the Gram kernel
}
PRECS = ("none", "jacobi", "mg", "mg_cheby")
CASES = [(g, p) for g in GRIDS for p in PRECS]


def fa():
    import faer_amg_amd
    return faer_amg_amd


def ks_of(grid):
    return (11,) if grid == "72x64x64" else (1, 3, 8, 11, 32)


def T(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def device_block(X, ld):
    """X (numpy n x k) as a column-major torch device view with leading dimension ld."""
    import torch
    n, k = X.shape
    buf = torch.full((k, ld), PAD, dtype=torch.float64, device="cuda:0")
    buf[:, :n] = torch.as_tensor(np.ascontiguousarray(X.T), device="cuda:0")
    return buf, buf[:, :n].t()


def rhs_block(n, k, random_guess, seed=5):
    """(B, X0): the columns described in the module docstring."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, k))
    X0 = rng.standard_normal((n, k)) if random_guess else np.zeros((n, k))
    if k >= 3:
        B[:, 1] = 0.0
        X0[:, 1] = 0.0
    if k > 3:  # the guess with its column: tol_3 = 1e-8 ||B_3|| is out of fp64's reach from an O(1) start residual
        B[:, 3] *= 1e-9
        X0[:, 3] *= 1e-9
    if k >= 8:
        B[:, 5] = 2.0 * B[:, 0] - 3.0 * B[:, 4]
        X0[:, 5] = 2.0 * X0[:, 0] - 3.0 * X0[:, 4]
    if k > 3:
        B[:, k - 1] = B[:, 2]
        X0[:, k - 1] = X0[:, 2]
    return B, X0


def dropped_at_start(k):
    return 3 if k >= 8 else 2 if k > 3 else 1 if k == 3 else 0


# ------------------------------------------------------------------ the model

def gram_plain(X, Y):
    return X.T @ Y


def block_rows(n):
    """Row blocks of 64; at n <= 64 one such block is the plain order again, so 8 there."""
    return 64 if n > 64 else 8


def gram_blocked(X, Y):
    """X^T Y as row blocks of 64 summed in order."""
    n = X.shape[0]
    rows = block_rows(n)
    nb = -(-n // rows)
    Xp = np.zeros((nb * rows, X.shape[1]))
    Yp = np.zeros((nb * rows, Y.shape[1]))
    Xp[:n] = X
    Yp[:n] = Y
    part = Xp.reshape(nb, rows, -1).transpose(0, 2, 1) @ Yp.reshape(nb, rows, -1)
    return np.cumsum(part, axis=0)[-1]


def colnorm_plain(R):
    return np.sqrt((R * R).sum(axis=0))


def colnorm_blocked(R):
    n = R.shape[0]
    rows = block_rows(n)
    nb = -(-n // rows)
    Rp = np.zeros((nb * rows, R.shape[1]))
    Rp[:n] = R
    part = (Rp * Rp).reshape(nb, rows, -1).sum(axis=1)
    return np.sqrt(np.cumsum(part, axis=0)[-1])


class RankChol:
    """G^+ of include/amg.h: symmetrise, drop g_jj <= 0, unit diagonal, Cholesky with
    diagonal pivoting stopped at the first pivot <= rank_tol.  `seen`: every accepted
    pivot and every diagonal left when it stopped."""

    def __init__(self, G, rank_tol):
        k = G.shape[0]
        Gs = 0.5 * (G + G.T)
        d = np.diag(G)
        self.k = k
        self.cand = [j for j in range(k) if d[j] > 0.0]
        nc = len(self.cand)
        self.sc = np.zeros(k)
        self.sc[self.cand] = 1.0 / np.sqrt(d[self.cand])
        s = self.sc[self.cand]
        Cm = (Gs[np.ix_(self.cand, self.cand)] * s[:, None]) * s[None, :]
        np.fill_diagonal(Cm, 1.0)
        L = np.zeros((nc, nc))
        dg = np.ones(nc)
        left = list(range(nc))
        self.order, self.seen = [], []
        for t in range(nc):
            p = max(left, key=lambda a: (dg[a], -a))  # ties: the lower index
            if not dg[p] > rank_tol:
                break
            self.seen.append(dg[p])
            lpp = np.sqrt(dg[p])
            L[p, t] = lpp
            left.remove(p)
            self.order.append(p)
            if left:
                col = (Cm[left, p] - L[left, :t] @ L[p, :t]) / lpp
                L[left, t] = col
                dg[left] -= col * col
        self.seen += [dg[a] for a in left]
        self.Lr = L[np.ix_(self.order, range(len(self.order)))]  # r x r lower triangular, pivot order
        self.rank = len(self.order)

    def solve(self, Y):
        import scipy.linalg as sl
        out = np.zeros((self.k, Y.shape[1]))
        if self.rank:
            idx = [self.cand[a] for a in self.order]
            z = sl.solve_triangular(self.Lr, self.sc[idx][:, None] * Y[idx], lower=True)
            z = sl.solve_triangular(self.Lr.T, z, lower=False)
            out[idx] = self.sc[idx][:, None] * z
        return out


def one_blas_thread():
    """The model's products are small: a threaded BLAS only adds its wake-up time to each."""
    try:
        import threadpoolctl
        return threadpoolctl.threadpool_limits(1)
    except ImportError:
        import contextlib
        return contextlib.nullcontext()


def model_bcg(S, Mapply, B, X0, max_iter, rel_tol, abs_tol=0.0, rank_tol=RANK_TOL, blocked=False):
    """The algorithm of include/amg.h in numpy float64.  S: scipy CSR of A; Mapply: Z = M R
    (None: identity).  Returns a dict: iters, hist (m x k), ranks (m), X, seen (pivots)."""
    with one_blas_thread():
        return _model_bcg(S, Mapply, B, X0, max_iter, rel_tol, abs_tol, rank_tol, blocked)


def _model_bcg(S, Mapply, B, X0, max_iter, rel_tol, abs_tol, rank_tol, blocked):
    gram = gram_blocked if blocked else gram_plain
    norm = colnorm_blocked if blocked else colnorm_plain
    k = B.shape[1]
    X = X0.copy()
    R = B - S @ X
    bn = norm(B)
    tol = np.maximum(abs_tol, rel_tol * bn)
    out = dict(iters=0, hist=[], ranks=[], seen=[], X=X)
    if np.all(norm(R) <= tol):
        return out
    Z = R if Mapply is None else Mapply(R)
    P = Z.copy()
    out["iters"] = max_iter + 1
    for it in range(1, max_iter + 1):
        Q = S @ P
        GS = gram(P, np.hstack([Q, R]))
        ch = RankChol(GS[:, :k], rank_tol)
        out["seen"] += ch.seen
        alpha = ch.solve(GS[:, k:])
        out["ranks"].append(ch.rank)
        X += P @ alpha
        R -= Q @ alpha
        rn = norm(R)
        out["hist"].append(np.where(bn == 0.0, rn, rn / np.where(bn == 0.0, 1.0, bn)))
        if np.all(rn <= tol):
            out["iters"] = it
            break
        if ch.rank == 0 or it == max_iter:
            break
        Z = R if Mapply is None else Mapply(R)
        P = Z - P @ ch.solve(gram(Q, Z))
    out["hist"] = np.array(out["hist"]).reshape(-1, k)
    out["ranks"] = np.array(out["ranks"], np.int64)
    return out


def rel_spread(a, b):
    """max |a - b| / max(|a|, |b|) over the entries (0 where both are 0)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.maximum(np.abs(a), np.abs(b))
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(den > 0.0, np.abs(a - b) / den, 0.0)
    return float(q.max()) if q.size else 0.0


# ------------------------------------------------------------------ operators

_ops = {}


def operators(ctx, grid, prec):
    """(A, scipy A, M) of a case, built once per session."""
    F = fa()
    if grid not in _ops:
        if grid == "elasticity":
            A = F.elasticity_q1((4, 4, 4)).upload(ctx)
        else:
            A = F.SparseMatOp.laplace3d_7pt(ctx, *GRIDS[grid])
        _ops[grid] = {"A": A, "S": A.to_scipy().tocsr()}
    d = _ops[grid]
    A = d["A"]
    if prec not in d:
        if prec == "none":
            d[prec] = None
        elif prec == "jacobi":
            d[prec] = F.new_jacobi(A, 0.66)
        elif prec in ("mg", "mg_cheby"):
            d[prec] = F.sa_build_box(A, GRIDS[grid], (2, 2, 2), coarsest_dim=10 if grid == "3" else 100,
                                     smoother="jacobi" if prec == "mg" else "chebyshev")
        else:  # "sa_l1": the general operator's hierarchy
            nn = F.constant_candidates(A.nrows, 3)
            d[prec] = F.smoothed_aggregation(A, nn, block_size=3, candidate_dimension=3, coarsest_dim=20,
                                             smoother="l1")
    return A, d["S"], d[prec]


def block_apply(ctx, M):
    """Z = M R through the handle's block apply (host in, host out)."""
    if M is None:
        return None

    def f(R):
        import torch
        n, k = R.shape
        rb = T(R.T).t()  # column-major n x k
        zb = torch.zeros((k, n), dtype=torch.float64, device="cuda:0").t()
        M.apply(zb, rb)
        ctx.synchronize()
        return np.ascontiguousarray(zb.cpu().numpy())
    return f


def run_gpu(ctx, A, M, B, X0, **kw):
    """One amg_block_cg_solve on padded blocks; checks the padding and B; returns (iters, hist, ranks, X)."""
    import torch
    n = B.shape[0]
    bbuf, Bv = device_block(B, n + 3)
    xbuf, Xv = device_block(X0, n + 1)
    iters, hist, ranks = fa().block_cg_solve(A, M, Bv, Xv, **kw)
    ctx.synchronize()
    assert bool((bbuf[:, n:] == PAD).all()) and bool((xbuf[:, n:] == PAD).all())
    assert torch.equal(Bv, T(B))
    return iters, hist, ranks, Xv.cpu().numpy().copy()


def bits(h):
    return np.ascontiguousarray(h, np.float64).view(np.uint64)


def check_case(ctx, A, S, M, B, X0, label, max_iter=400, rel_tol=1e-8, model_iters=None):
    """The per-case checks of a converging solve; returns (gpu iters, model iters).
    model_iters: the model stops there, unconverged, and ranks and history are compared over
    those iterations only (n = 294912 without a multigrid: 186 iterations of the numpy model
    take 20 s per summation order); the solve itself still runs to convergence."""
    n, k = B.shape
    Mapply = block_apply(ctx, M)
    cap = max_iter if model_iters is None else model_iters
    m1 = model_bcg(S, Mapply, B, X0, cap, rel_tol)
    m2 = model_bcg(S, Mapply, B, X0, cap, rel_tol, blocked=True)
    bn = np.linalg.norm(B, axis=0)
    tol = rel_tol * bn
    # of the model first: it converges, its true residual is within tolerance, its
    # pivots are far from rank_tol, its two orders agree on ranks and count
    assert m2["iters"] == m1["iters"], (label, m1["iters"], m2["iters"])
    assert np.array_equal(m1["ranks"], m2["ranks"]), label
    for m in (m1, m2):
        seen = np.array(m["seen"])
        assert not np.any((seen > RANK_TOL / 100.0) & (seen < RANK_TOL * 100.0)), (label, seen)
        if model_iters is None:
            assert m["iters"] <= max_iter, (label, m["iters"])
            assert np.all(np.linalg.norm(B - S @ m["X"], axis=0) <= tol), label
        else:
            assert m["iters"] == model_iters + 1 and len(m["ranks"]) == model_iters, (label, m["iters"])
    spread = rel_spread(m1["hist"], m2["hist"])
    htol = max(100.0 * spread, 1e-12)

    iters, hist, ranks, X = run_gpu(ctx, A, M, B, X0, max_iter=max_iter, rel_tol=rel_tol)
    c = min(len(ranks), len(m1["ranks"]))
    print(f"{label}: iters gpu {iters} model {m1['iters']}, ranks[0] {ranks[:1]}, model spread {spread:.2e}, "
          f"gpu-model {rel_spread(hist[:c], m1['hist'][:c]):.2e}")
    # ranks
    if m1["iters"] > 0:  # (n = 27 has no room for more than 27 directions)
        assert m1["ranks"][0] == min(n, k - dropped_at_start(k)), (label, m1["ranks"])
        assert ranks[0] == min(n, k - dropped_at_start(k)), (label, ranks)
    assert np.array_equal(ranks[:c], m1["ranks"][:c]), (label, ranks, m1["ranks"])
    # iterations and history
    if model_iters is None:
        assert abs(iters - m1["iters"]) <= 1, (label, iters, m1["iters"])
    else:
        assert model_iters < iters <= max_iter and c == model_iters, (label, iters)
    assert hist.shape == (iters, k) and len(ranks) == iters
    assert np.all(np.abs(hist[:c] - m1["hist"][:c]) <= htol * np.abs(m1["hist"][:c])), \
        (label, rel_spread(hist[:c], m1["hist"][:c]), htol)
    # the true residual, on the host
    true = np.linalg.norm(B - S @ X, axis=0)
    print(f"{label}: true residual / tol up to {float(np.max(true / np.where(tol > 0, tol, 1.0))):.3f}")
    assert np.all(true <= 2.0 * tol), (label, true / np.where(tol > 0, tol, 1.0))
    if k >= 3:  # the zero column with a zero guess stays zero (every alpha row times a zero direction)
        assert not X[:, 1].any()
    # two calls give equal bits
    iters2, hist2, ranks2, X2 = run_gpu(ctx, A, M, B, X0, max_iter=max_iter, rel_tol=rel_tol)
    assert iters2 == iters and np.array_equal(ranks2, ranks)
    assert np.array_equal(bits(hist2), bits(hist)) and np.array_equal(bits(X2), bits(X))
    return iters, m1["iters"]


# ------------------------------------------------------------------ the solver

@gpu
@pytest.mark.parametrize("grid,prec", CASES)
def test_block_cg_against_the_model(ctx, grid, prec):
    F = fa()
    A, S, M = operators(ctx, grid, prec)
    n = A.nrows
    for k in ks_of(grid):
        for random_guess in (False, True):
            B, X0 = rhs_block(n, k, random_guess)
            label = f"{grid} {prec} k={k} guess={'random' if random_guess else 'zero'}"
            slow_model = grid == "72x64x64" and prec in ("none", "jacobi")
            it_gpu, it_model = check_case(ctx, A, S, M, B, X0, label, model_iters=10 if slow_model else None)
            if grid in ("12x11x10", "17") and prec == "jacobi" and k >= 8:
                # the coupling gain: fewer iterations than the slowest column alone
                import torch
                single = []
                for c in range(k):
                    x1 = T(X0[:, c])
                    it1, _ = F.pcg_solve(A, M, T(B[:, c]), x1, max_iter=400, rel_tol=1e-8)
                    single.append(it1)
                ctx.synchronize()
                print(f"{label}: coupled {it_gpu} (model {it_model}) against single solves up to {max(single)}")
                assert it_gpu <= it_model + 1
                assert it_model < max(single), (label, it_model, single)


@gpu
def test_block_cg_general_operator(ctx):
    """amg_gen_elasticity_q1(4, 4, 4) (block 3, a general storage: A P through the general
    SpMM), SA hierarchy with the L1 smoother, k = 8."""
    A, S, M = operators(ctx, "elasticity", "sa_l1")
    for random_guess in (False, True):
        B, X0 = rhs_block(A.nrows, 8, random_guess)
        check_case(ctx, A, S, M, B, X0, f"elasticity sa_l1 k=8 guess={'random' if random_guess else 'zero'}")


@gpu
@pytest.mark.parametrize("grid,prec", [("12x11x10", "none"), ("17", "jacobi"), ("17", "mg")])
def test_block_cg_not_converged_after_three(ctx, grid, prec):
    """max_iter = 3 on cases that need more: iters = 4, three history rows, X the model's third iterate."""
    A, S, M = operators(ctx, grid, prec)
    n = A.nrows
    Mapply = block_apply(ctx, M)
    for k in (1, 8, 32):
        B, X0 = rhs_block(n, k, k == 8)
        m1 = model_bcg(S, Mapply, B, X0, 3, 1e-8)
        m2 = model_bcg(S, Mapply, B, X0, 3, 1e-8, blocked=True)
        assert m1["iters"] == 4 and m2["iters"] == 4 and len(m1["hist"]) == 3
        iters, hist, ranks, X = run_gpu(ctx, A, M, B, X0, max_iter=3, rel_tol=1e-8)
        assert iters == 4 and hist.shape == (3, k) and len(ranks) == 3
        assert np.array_equal(ranks, m1["ranks"])
        htol = max(100.0 * rel_spread(m1["hist"], m2["hist"]), 1e-12)
        assert np.all(np.abs(hist - m1["hist"]) <= htol * np.abs(m1["hist"])), rel_spread(hist, m1["hist"])
        # X: per column, relative to the iterate's norm
        xn = np.linalg.norm(m1["X"], axis=0)
        xn[xn == 0.0] = 1.0
        xs = float((np.linalg.norm(m1["X"] - m2["X"], axis=0) / xn).max())
        xtol = max(100.0 * xs, 1e-12)
        assert np.all(np.linalg.norm(X - m1["X"], axis=0) / xn <= xtol), (k, xs)
    # max_iter = 0: nothing but the start residual is looked at
    iters, hist, ranks, X = run_gpu(ctx, A, M, B, X0, max_iter=0, rel_tol=1e-8)
    assert iters == 1 and hist.shape == (0, 32) and np.array_equal(X, X0)


@gpu
def test_block_cg_starts_within_tolerance(ctx):
    A, S, M = operators(ctx, "12x11x10", "jacobi")
    n = A.nrows
    Xs = np.random.default_rng(3).standard_normal((n, 4))
    B = np.asarray(S @ Xs)
    iters, hist, ranks, X = run_gpu(ctx, A, M, B, Xs, max_iter=10, rel_tol=1e-8)
    assert iters == 0 and hist.shape == (0, 4) and len(ranks) == 0 and np.array_equal(X, Xs)
    # a rank_tol of the caller's: column 1 = column 0 + 0.1 noise has a pivot near 0.01, kept by
    # the default and dropped at 0.5; whatever is dropped, R stays B - A X to rounding
    B, X0 = rhs_block(n, 3, False)
    B[:, 1] = B[:, 0] + 0.1 * np.random.default_rng(4).standard_normal(n)
    _, _, ranks_d, _ = run_gpu(ctx, A, M, B, X0, max_iter=20, rel_tol=1e-8)
    _, hist_h, ranks_h, Xh = run_gpu(ctx, A, M, B, X0, max_iter=20, rel_tol=1e-8, rank_tol=0.5)
    assert ranks_d[0] == 3 and ranks_h[0] == 2
    bn = np.linalg.norm(B, axis=0)
    assert np.all(np.abs(np.linalg.norm(B - S @ Xh, axis=0) - hist_h[-1] * bn) <= 1e-10 * bn)


@gpu
def test_block_cg_live_handle_errors(ctx):
    import torch
    F = fa()
    L = F.lib()
    dims = (8, 8, 8)
    n = 512
    A = F.SparseMatOp.laplace3d_7pt(ctx, *dims)
    J = F.new_jacobi(A, 0.66)
    mg = F.sa_build_box(A, dims, (2, 2, 2), coarsest_dim=100, smoother="jacobi")
    B = torch.ones((33, n), dtype=torch.float64, device="cuda:0")
    X = torch.zeros((33, n), dtype=torch.float64, device="cuda:0")
    it = np.full(1, -7, np.int64)
    ranks = np.full(5, -7, np.int64)
    vp = C.c_void_p

    def bcg(a, m, ldb=n, ldx=n, k=3):
        return L.amg_block_cg_solve(a.h, None if m is None else m.h, vp(B.data_ptr()), ldb, vp(X.data_ptr()), ldx, k,
                                    5, 1e-8, 0.0, 0.0, None, 0, ranks.ctypes.data_as(vp),
                                    it.ctypes.data_as(C.POINTER(C.c_int64)))

    assert bcg(A, J, ldx=n - 1) == INVALID and b"leading dimension" in L.amg_last_error()
    assert bcg(A, J, ldb=n - 1) == INVALID
    assert bcg(A, J, k=33) == UNSUPPORTED and b"32 columns" in L.amg_last_error()
    # overlapping extents: X one column into B's block
    assert L.amg_block_cg_solve(A.h, None, vp(B.data_ptr()), n, vp(B.data_ptr() + 8 * n), n, 2, 5, 1e-8, 0.0, 0.0, None,
                                0, None, it.ctypes.data_as(C.POINTER(C.c_int64))) == INVALID
    assert b"alias" in L.amg_last_error()
    # a non-square A (the interpolation of the hierarchy), a preconditioner of other dimensions -> DIM
    Pl = mg.level(0)[3]
    assert Pl.nrows != Pl.ncols
    assert bcg(Pl, None) == DIM
    A2 = F.SparseMatOp.laplace3d_7pt(ctx, 4, 4, 4)
    assert bcg(A, F.new_jacobi(A2, 0.66)) == DIM
    # a distributed multigrid (one loopback rank) as M or A -> UNSUPPORTED
    hub = F.LoopbackHub(1)
    comm = F.Comm(ctx, hub=hub, rank=0)
    splits = F.slab_splits(F.box_level_dims(dims, (2, 2, 2), mg.levels()), 1)
    F.set_flag("dense_tail", 0)  # as tests/test_gpu_dist.py builds its distributed cycles
    try:
        dm = F.DistMultigrid(comm, mg, splits, agglomerate_rows=100)
    finally:
        F.set_flag("dense_tail", 4096)
    assert bcg(A, dm) == UNSUPPORTED and b"distributed" in L.amg_last_error()
    assert bcg(dm, None) == UNSUPPORTED
    ctx.synchronize()
    assert not bool(X.any()) and (it == -7).all() and (ranks == -7).all()  # nothing ran
    # k = 0 with live handles: OK, nothing touched
    assert bcg(A, J, k=0) == 0
    assert (it == -7).all() and (ranks == -7).all() and not bool(X.any())


# ------------------------------------------------------------------ the kernels

NS = (1, 63, 64, 65, 4097, 70001)
SHAPES = ((1, 1, 0), (7, 5, 3), (16, 16, 16), (17, 32, 1), (32, 32, 32))


def scaled_normals(rng, n, k):
    return rng.standard_normal((n, k)) * 10.0 ** rng.uniform(-3, 3, k)


@gpu
@pytest.mark.parametrize("n", NS)
def test_block_gram_kernel(ctx, n):
    import torch
    L = fa().lib()
    vp = C.c_void_p
    rng = np.random.default_rng(100 + n)
    for w, m1, m2 in SHAPES:
        X, Y1, Y2 = scaled_normals(rng, n, w), scaled_normals(rng, n, m1), scaled_normals(rng, n, m2)
        xb, Xv = device_block(X, n + 3)
        y1b, Y1v = device_block(Y1, n + 1)
        y2b, Y2v = device_block(Y2, n + 5) if m2 else (None, None)
        m = m1 + m2
        out = []
        for _ in range(2):
            buf = np.full(w * m + 8, PAD)
            st = L.amg_block_gram(ctx.h, vp(Xv.data_ptr()), n + 3, w, vp(Y1v.data_ptr()), n + 1, m1,
                                  vp(Y2v.data_ptr()) if m2 else None, n + 5 if m2 else 0, m2, n,
                                  buf.ctypes.data_as(vp))
            assert st == 0, L.amg_last_error()
            assert (buf[w * m:] == PAD).all()
            out.append(buf[:w * m].reshape((w, m), order="F").copy())
        ctx.synchronize()
        assert np.array_equal(bits(out[0]), bits(out[1]))  # two calls, equal bits
        Y = np.hstack([Y1, Y2])
        ref = (X.astype(np.longdouble).T @ Y.astype(np.longdouble))
        bound = 4.0 * n * EPS * (np.abs(X).T @ np.abs(Y))
        err = np.abs(out[0].astype(np.longdouble) - ref).astype(np.float64)
        print(f"gram n={n} (w, m1, m2)=({w}, {m1}, {m2}): max err / bound {float((err / bound).max()):.3f}")
        assert np.all(err <= bound), (n, w, m1, m2, float((err / bound).max()))
        # the wrapper gives the same bits
        assert np.array_equal(bits(fa().block_gram(ctx, Xv, Y1v, Y2v)), bits(out[0]))
        # operands untouched, padding included
        for b_, h_ in ((xb, X), (y1b, Y1)) + (((y2b, Y2),) if m2 else ()):
            assert bool((b_[:, n:] == PAD).all()) and torch.equal(b_[:, :n], T(h_.T))


@gpu
@pytest.mark.parametrize("n", NS)
def test_block_gemm_update_kernel(ctx, n):
    import torch
    F = fa()
    rng = np.random.default_rng(200 + n)
    for j, (w, m, _) in enumerate(SHAPES):
        for sign in ((1, -1) if j % 2 == 0 else (-1, 1)):
            X, Y0 = scaled_normals(rng, n, w), scaled_normals(rng, n, m)
            Cm = scaled_normals(rng, w, m)
            xb, Xv = device_block(X, n + 3)
            res = []
            for _ in range(2):
                yb, Yv = device_block(Y0, n + 1)
                F.block_gemm_update(ctx, Yv, Xv, Cm, sign)
                ctx.synchronize()
                assert bool((yb[:, n:] == PAD).all())  # rows past n untouched
                res.append(Yv.cpu().numpy().copy())
            assert np.array_equal(bits(res[0]), bits(res[1]))
            ref = Y0.astype(np.longdouble) + sign * (X.astype(np.longdouble) @ Cm.astype(np.longdouble))
            bound = (w + 2) * EPS * (np.abs(Y0) + np.abs(X) @ np.abs(Cm))
            err = np.abs(res[0].astype(np.longdouble) - ref).astype(np.float64)
            print(f"update n={n} (w, m)=({w}, {m}) sign={sign}: max err / bound {float((err / bound).max()):.3f}")
            assert np.all(err <= bound), (n, w, m, sign, float((err / bound).max()))
            assert bool((xb[:, n:] == PAD).all()) and torch.equal(xb[:, :n], T(X.T))
