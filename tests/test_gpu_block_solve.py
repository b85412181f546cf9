"""The block solve drivers (amg_pcg_solve_block, amg_stationary_solve_block;
solve.cpp pcg_block_impl / stationary_block_impl, kernels in pcg.hip).

The single-vector drivers are the definition of correct: for every column the
block call's X, iteration count and residual history are compared bit for bit
with amg_pcg_solve / amg_stationary_solve on copies of that column.  Nothing here
has a tolerance.

Blocks are column-major torch views with ldb = n + 3 and ldx = n + 1 (odd leading
dimensions: columns that are only 8-byte aligned); the padding rows hold 7.5 and
must stay untouched.  The columns are chosen so that they stop at different
iterations: column 0 is the lowest sine mode of the grid (an eigenvector of A and
of Jacobi A: CG from a zero guess stops after one iteration), column 1 is zero
(with a zero guess: 0 iterations, X never written -- a nonzero guess for b = 0
makes amg_pcg_solve divide by ||b|| = 0, so that column's guess is zero in the
random-guess cases too), the last column repeats an earlier one, the rest are
normals.  Half the cases start from a random guess, half from zero; with a random
guess and k >= 11, columns 3 and 4 start near their solution (rhs_block), so the
stationary sweeps stop apart at rel_tol = 1e-2 too.
Histories are compared as bit patterns (a zero column's stationary history is
0/0).
"""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu
PAD = 7.5
INVALID, DIM, UNSUPPORTED = 1, 2, 3

GRIDS = {
    "3": (3, 3, 3),           # n = 27: below one 256-thread block
    "17": (17, 17, 17),       # n = 4913, odd: one stride trip, ragged last block
    "72x64x64": (72, 64, 64)  # n = 294912 > 1024 * 256: the second trip of the dots' grid-stride loop
}
PRECS = ("none", "jacobi", "mg", "composite")
CASES = [(g, p) for g in GRIDS for p in PRECS if not (g == "3" and p == "composite")]


def fa():
    import faer_amg_amd
    return faer_amg_amd


def ks_of(grid):
    return (11,) if grid == "72x64x64" else (1, 3, 11, 33)  # 11: over the 8-column SpMM group; 33: over the 32-column chunk


def device_block(X, ld):
    """X (numpy n x k) as a column-major torch device view with leading dimension ld."""
    import torch
    n, k = X.shape
    buf = torch.full((k, ld), PAD, dtype=torch.float64, device="cuda:0")
    buf[:, :n] = torch.as_tensor(np.ascontiguousarray(X.T), device="cuda:0")
    return buf, buf[:, :n].t()


def T(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def sine_mode(dims):
    nx, ny, nz = dims
    s = [np.sin(np.pi * (np.arange(m) + 1) / (m + 1)) for m in (nx, ny, nz)]
    return (s[2][:, None, None] * s[1][None, :, None] * s[0][None, None, :]).ravel()


def laplace_apply(dims, v):
    """The 7-point Laplacian (6, -1; Dirichlet) applied on the host."""
    nx, ny, nz = dims
    u = v.reshape(nz, ny, nx)
    out = 6.0 * u
    out[:, :, 1:] -= u[:, :, :-1]
    out[:, :, :-1] -= u[:, :, 1:]
    out[:, 1:, :] -= u[:, :-1, :]
    out[:, :-1, :] -= u[:, 1:, :]
    out[1:, :, :] -= u[:-1, :, :]
    out[:-1, :, :] -= u[1:, :, :]
    return out.ravel()


def rhs_block(dims, k, random_guess, seed=5):
    """(B, X0): the columns described in the module docstring."""
    n = int(np.prod(dims))
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, k))
    X0 = rng.standard_normal((n, k)) if random_guess else np.zeros((n, k))
    B[:, 0] = sine_mode(dims)
    if k >= 3:
        B[:, 1] = 0.0
        X0[:, 1] = 0.0
    if k >= 11 and random_guess:
        # guesses near the solution, so that the stationary sweeps stop apart at
        # rel_tol = 1e-2: b = A x0 + delta g gives ||b - A x0|| / ||b|| ~ delta / 6.5
        # (||A y|| ~ sqrt(42) ||y|| for a normal y): column 3 starts below the
        # tolerance, column 4 a few sweeps above it
        for c, delta in ((3, 1e-3), (4, 0.3)):
            B[:, c] = laplace_apply(dims, X0[:, c]) + delta * B[:, c]
    if k > 3:
        B[:, k - 1] = B[:, 2]
        X0[:, k - 1] = X0[:, 2]
    return B, X0, (2 if k > 3 else None)


_ops = {}


def operators(ctx, grid, prec):
    """A and the preconditioner of a case, built once per session."""
    F = fa()
    dims = GRIDS[grid]
    if grid not in _ops:
        _ops[grid] = {"A": F.SparseMatOp.laplace3d_7pt(ctx, *dims)}
    d = _ops[grid]
    A = d["A"]
    if prec not in d:
        if prec == "none":
            d[prec] = None
        elif prec == "jacobi":
            d[prec] = F.new_jacobi(A, 0.66)
        elif prec == "mg":
            d[prec] = F.sa_build_box(A, dims, (2, 2, 2), coarsest_dim=10 if grid == "3" else 100, smoother="jacobi")
        else:
            d[prec] = F.Composite(A, [operators(ctx, grid, "mg")[1], F.new_l1(A)])
    return A, d[prec]


def bits(h):
    return np.ascontiguousarray(h, np.float64).view(np.uint64)


def check_columns(ctx, solve_block, solve_one, dims, k, random_guess, expect=None):
    """One block call against k single calls; returns the per-column iteration counts."""
    import torch
    n = int(np.prod(dims))
    B, X0, dup = rhs_block(dims, k, random_guess)
    bbuf, Bv = device_block(B, n + 3)
    xbuf, Xv = device_block(X0, n + 1)
    iters, hists = solve_block(Bv, Xv)
    ctx.synchronize()
    assert bool((bbuf[:, n:] == PAD).all()) and bool((xbuf[:, n:] == PAD).all())
    assert torch.equal(Bv, T(B))
    for c in range(k):
        b1, x1 = T(B[:, c]), T(X0[:, c])
        it1, h1 = solve_one(b1, x1)
        ctx.synchronize()
        assert int(iters[c]) == it1, (k, c, int(iters[c]), it1)
        assert torch.equal(Xv[:, c], x1), (k, c)
        assert len(hists[c]) == len(h1) and np.array_equal(bits(hists[c]), bits(h1)), (k, c)
    if dup is not None:
        assert int(iters[k - 1]) == int(iters[dup]) and torch.equal(Xv[:, k - 1], Xv[:, dup])
        assert np.array_equal(bits(hists[k - 1]), bits(hists[dup]))
    if expect:
        expect(iters, hists, Xv, X0)
    return [int(v) for v in iters]


@gpu
@pytest.mark.parametrize("grid,prec", CASES)
def test_pcg_block_is_bitwise_the_single_solves(ctx, grid, prec):
    F = fa()
    dims = GRIDS[grid]
    A, M = operators(ctx, grid, prec)
    for j, k in enumerate(ks_of(grid)):
        random_guess = (j + PRECS.index(prec)) % 2 == 1

        def expect(iters, hists, Xv, X0, k=k, random_guess=random_guess):
            if k >= 3:  # the zero column: within tolerance at the start, X never written
                assert int(iters[1]) == 0 and len(hists[1]) == 0 and not bool(Xv[:, 1].any())
            if not random_guess and prec in ("none", "jacobi"):
                assert int(iters[0]) == 1, iters  # the eigenvector column

        its = check_columns(ctx, lambda Bv, Xv: F.pcg_solve_block(A, M, Bv, Xv, max_iter=200, rel_tol=1e-8),
                            lambda b, x: F.pcg_solve(A, M, b, x, max_iter=200, rel_tol=1e-8), dims, k, random_guess,
                            expect)
        print(f"{grid} {prec} k={k} guess={'random' if random_guess else 'zero'}: iters {sorted(set(its))}")
        if prec in ("mg", "composite"):
            assert max(its) <= 200, its  # every column converged
        if grid == "17" and prec == "jacobi" and k >= 3 and not random_guess:
            # the precondition of this test: the columns stop at >= 3 different iterations
            assert len(set(its)) >= 3, its

        def expect3(iters, hists, Xv, X0):
            for c in range(len(iters)):
                assert int(iters[c]) <= 4
                if int(iters[c]) == 4:  # not converged: max_iter + 1, exactly max_iter history entries
                    assert len(hists[c]) == 3

        its3 = check_columns(ctx, lambda Bv, Xv: F.pcg_solve_block(A, M, Bv, Xv, max_iter=3, rel_tol=1e-8),
                             lambda b, x: F.pcg_solve(A, M, b, x, max_iter=3, rel_tol=1e-8), dims, k, random_guess,
                             expect3)
        if grid != "3" and prec in ("none", "jacobi") and k > 3:
            assert 4 in its3, its3  # the random columns cannot converge in 3 iterations


@gpu
@pytest.mark.parametrize("grid,prec", [c for c in CASES if c[1] != "none"])
@pytest.mark.parametrize("rel_tol", [1e-300, 1e-2])
def test_stationary_block_is_bitwise_the_single_solves(ctx, grid, prec, rel_tol):
    F = fa()
    dims = GRIDS[grid]
    A, M = operators(ctx, grid, prec)
    seen = set()
    for j, k in enumerate(ks_of(grid)):
        random_guess = (j + PRECS.index(prec)) % 2 == 0
        its = check_columns(ctx, lambda Bv, Xv: F.stationary_solve_block(A, M, Bv, Xv, max_iter=6, rel_tol=rel_tol),
                            lambda b, x: F.stationary_solve(A, M, b, x, max_iter=6, rel_tol=rel_tol), dims, k,
                            random_guess)
        assert all(1 <= v <= 6 for v in its), its
        if rel_tol == 1e-300:
            assert set(its) == {6}, its
        seen |= set(its)
    print(f"{grid} {prec} rel_tol={rel_tol}: sweeps {sorted(seen)}")
    if rel_tol == 1e-2 and grid != "72x64x64":  # (its one k has a random guess under "mg" only)
        assert len(seen) >= 2 and 1 in seen, seen  # columns stop at different sweeps


@gpu
def test_block_solve_live_handle_errors(ctx):
    import torch
    F = fa()
    L = F.lib()
    dims = (8, 8, 8)
    n = 512
    A = F.SparseMatOp.laplace3d_7pt(ctx, *dims)
    J = F.new_jacobi(A, 0.66)
    mg = F.sa_build_box(A, dims, (2, 2, 2), coarsest_dim=100, smoother="jacobi")
    B = torch.ones((3, n), dtype=torch.float64, device="cuda:0")
    X = torch.zeros((3, n), dtype=torch.float64, device="cuda:0")
    it = np.full(3, -7, np.int64)
    pit = it.ctypes.data_as(C.c_void_p)
    vp = C.c_void_p

    def pcg(a, m, ldb=n, ldx=n, k=3):
        return L.amg_pcg_solve_block(a.h, None if m is None else m.h, vp(B.data_ptr()), ldb, vp(X.data_ptr()), ldx, k,
                                     5, 1e-8, 0.0, None, 0, pit)

    def stat(a, m, ldb=n, ldx=n, k=3):
        return L.amg_stationary_solve_block(a.h, m.h, vp(B.data_ptr()), ldb, vp(X.data_ptr()), ldx, k, 5, 1e-8, None, 0,
                                            pit)

    for f in (pcg, stat):
        assert f(A, J, ldx=n - 1) == INVALID and b"leading dimension" in L.amg_last_error()
        assert f(A, J, ldb=n - 1) == INVALID
    # overlapping extents: X one column into B's block
    assert L.amg_pcg_solve_block(A.h, None, vp(B.data_ptr()), n, vp(B.data_ptr() + 8 * n), n, 2, 5, 1e-8, 0.0, None, 0,
                                 pit) == INVALID
    assert b"alias" in L.amg_last_error()
    # a multigrid as A, a preconditioner of other dimensions -> DIM
    A2 = F.SparseMatOp.laplace3d_7pt(ctx, 4, 4, 4)
    J2 = F.new_jacobi(A2, 0.66)
    assert pcg(mg, J2) == DIM and stat(mg, J2) == DIM
    assert pcg(A, J2) == DIM
    # a distributed multigrid (one loopback rank) as M -> UNSUPPORTED
    hub = F.LoopbackHub(1)
    comm = F.Comm(ctx, hub=hub, rank=0)
    splits = F.slab_splits(F.box_level_dims(dims, (2, 2, 2), mg.levels()), 1)
    F.set_flag("dense_tail", 0)  # as tests/test_gpu_dist.py builds its distributed cycles
    try:
        dm = F.DistMultigrid(comm, mg, splits, agglomerate_rows=100)
    finally:
        F.set_flag("dense_tail", 4096)
    assert pcg(A, dm) == UNSUPPORTED and b"distributed" in L.amg_last_error()
    assert stat(A, dm) == UNSUPPORTED
    assert pcg(dm, None) == UNSUPPORTED
    ctx.synchronize()
    assert not bool(X.any()) and (it == -7).all()  # nothing ran
    # k = 0 with live handles: OK, nothing touched
    assert pcg(A, J, k=0) == 0 and stat(A, J, k=0) == 0
    assert (it == -7).all()


def write_mfem_laplace(d, name, nx, ny, k, rng):
    """A 5-point Laplacian on nx x ny as an MFEM bundle (the files tests/test_io.py
    writes: symmetric coordinate .mtx, .bdy with a count line, .coords, .rhs)."""
    import os
    n = nx * ny
    ent = []
    for j in range(ny):
        for i in range(nx):
            r = i + nx * j
            ent.append((r, r, 4.0))
            if i:
                ent.append((r, r - 1, -1.0))
            if j:
                ent.append((r, r - nx, -1.0))
    with open(os.path.join(d, name + ".mtx"), "w") as f:
        f.write("%%MatrixMarket matrix coordinate real symmetric\n")
        f.write(f"{n} {n} {len(ent)}\n")
        for r, c, v in ent:
            f.write(f"{r + 1} {c + 1} {v!r}\n")
    bdy = [0, nx - 1, n - 1]
    with open(os.path.join(d, name + ".bdy"), "w") as f:
        f.write(f"{len(bdy)}\n" + "".join(f"{b}\n" for b in bdy))
    with open(os.path.join(d, name + ".coords"), "w") as f:
        for r in range(n):
            f.write(f"{float(r % nx)!r} {float(r // nx)!r}\n")
    with open(os.path.join(d, name + ".rhs"), "w") as f:
        for v in rng.standard_normal(n * k):
            f.write(f"{float(v)!r}\n")


@gpu
def test_mfem_rhs_columns_in_one_solve(ctx, tmp_path):
    """The loader's n x 2 rhs block through one amg_pcg_solve_block."""
    import torch
    F = fa()
    write_mfem_laplace(str(tmp_path), "sys", 9, 7, 2, np.random.default_rng(8))
    S = F.MfemSystem(str(tmp_path), "sys", True)
    assert S.rhs_cols == 2 and S.n == 60
    A = S.matrix.upload(ctx)
    M = F.new_jacobi(A, 0.66)
    n = S.n
    bbuf, Bv = device_block(S.rhs, n + 3)
    xbuf, Xv = device_block(np.zeros((n, 2)), n + 1)
    iters, hists = F.pcg_solve_block(A, M, Bv, Xv, max_iter=100, rel_tol=1e-10)
    ctx.synchronize()
    for c in range(2):
        b1, x1 = T(S.rhs[:, c]), T(np.zeros(n))
        it1, h1 = F.pcg_solve(A, M, b1, x1, max_iter=100, rel_tol=1e-10)
        ctx.synchronize()
        assert int(iters[c]) == it1 and 1 <= it1 <= 100
        assert torch.equal(Xv[:, c], x1) and np.array_equal(bits(hists[c]), bits(h1))
    assert bool((bbuf[:, n:] == PAD).all()) and bool((xbuf[:, n:] == PAD).all())
