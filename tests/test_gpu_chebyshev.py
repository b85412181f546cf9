"""The Chebyshev polynomial smoother (csrc/cheby.hip): the operator
against a numpy restatement of its definition, the polynomial it is, its k-wide
form bit for bit, the eigenvalue bound, and its place in the V-cycle, the block
cycle and the solve drivers.

Tolerances: 1e-11 (max-norm, relative) wherever the device and numpy sum the rows
of A in different orders -- the project's cycle tolerance; bits
wherever two device paths compute the same thing; 1e-13 for the dense tail
(test_dense_tail's bound); the bound's brackets are derived in DESIGN.md 14.
"""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu
PAD = 7.5
OK, INVALID, DIM, NOT_SPD = 0, 1, 2, 4


def fa():
    import faer_amg_amd
    return faer_amg_amd


# --------------------------------------------- the definition, restated in numpy

def cheby_coeffs(lmax, lmin, m):
    """c1[k], c2[k] of DESIGN.md 14 (the same expressions in the same order)."""
    theta = (lmax + lmin) / 2.0
    delta = (lmax - lmin) / 2.0
    sigma = theta / delta
    rho = 1.0 / sigma
    c1, c2 = [0.0], [1.0 / theta]
    for _ in range(1, m):
        rk = 1.0 / (2.0 * sigma - rho)
        c1.append(rk * rho)
        c2.append(2.0 * rk / delta)
        rho = rk
    return c1, c2, sigma


def np_cheby(S, lmax, lmin, m, b):
    """z = S b of the definition; b a vector or an n x k block."""
    dinv = 1.0 / S.diagonal()
    if b.ndim == 2:
        dinv = dinv[:, None]
    c1, c2, _ = cheby_coeffs(lmax, lmin, m)
    d = c2[0] * (dinv * b)
    x = d.copy()
    r = b
    for k in range(1, m):
        r = r - S @ d
        d = (c1[k] * d) + (c2[k] * (dinv * r))
        x = x + d
    return x


def np_lanczos(S, iters):
    """Largest Ritz value of `iters` Lanczos steps on D^-1 A in the D inner product
    from q_i = ((i * 2654435761) mod 2^32) / 2^32 - 0.5."""
    n = S.shape[0]
    dg = S.diagonal()
    q = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 32)).astype(np.float64) / 2.0**32 - 0.5
    q = q / np.sqrt(q @ (dg * q))
    qp, beta, al, be = None, 0.0, [], []
    for j in range(iters):
        w = S @ q
        a = q @ w
        al.append(a)
        if j + 1 == iters:
            break
        w = w / dg - a * q
        if j > 0:
            w = w - beta * qp
        beta = np.sqrt(w @ (dg * w))
        if not beta > 1e-13 * abs(a):
            break
        be.append(beta)
        qp, q = q, w / beta
    T = np.diag(al) + np.diag(be[:len(al) - 1], 1) + np.diag(be[:len(al) - 1], -1)
    return float(np.linalg.eigvalsh(T)[-1])


def row_sum_bound(S):
    return float((np.asarray(abs(S).sum(axis=1)).ravel() / S.diagonal()).max())


def lam_true(S):
    """lambda_max(D^-1 A), dense."""
    s = 1.0 / np.sqrt(S.diagonal())
    return float(np.linalg.eigvalsh(s[:, None] * S.toarray() * s[None, :])[-1])


def maxrel(z, ref):
    return float(np.max(np.abs(z - ref)) / np.max(np.abs(ref)))


# --------------------------------------------------------------------- operators

_ops = {}


def operator(ctx, name):
    """(handle, scipy CSR, lambda_max(D^-1 A)); built once, never changed."""
    if name not in _ops:
        F = fa()
        if name == "elasticity":  # block 3, a general storage
            A = F.elasticity_q1((4, 4, 4)).upload(ctx)
        else:  # 7-point nx x ny x nz
            A = F.SparseMatOp.laplace3d_7pt(ctx, *name)
        S = A.to_scipy().tocsr()
        _ops[name] = (A, S, lam_true(S))
    return _ops[name]


SMALL = (5, 4, 3)   # n = 60: less than one wave
ODD = (11, 9, 7)    # n = 693: odd, every 16-B path has a tail
OPERATORS = [SMALL, ODD, "elasticity"]


def T(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def device_block(X, ld, pad=PAD):
    """X (numpy n x k) as a column-major torch device view with leading dimension ld."""
    import torch
    n, k = X.shape
    buf = torch.full((k, ld), pad, dtype=torch.float64, device="cuda:0")
    buf[:, :n] = torch.as_tensor(np.ascontiguousarray(X.T), device="cuda:0")
    return buf, buf[:, :n].t()


def apply_dev(ctx, op, b):
    import torch
    z = torch.empty(len(b), dtype=torch.float64, device="cuda:0")
    op.apply(z, T(b))
    ctx.synchronize()
    return z.cpu().numpy()


# ------------------------------------------------------- 1. apply against numpy

@gpu
@pytest.mark.parametrize("name", OPERATORS, ids=str)
def test_apply_against_numpy(ctx, name):
    F = fa()
    A, S, lt = operator(ctx, name)
    n = A.nrows
    b = np.random.default_rng(21).uniform(-1, 1, n)
    lmax = lt * (1 + 1e-12)
    for ratio in (4.0, 30.0):
        for m in (1, 2, 3, 6):
            Sm = F.new_chebyshev(A, steps=m, eig_ratio=ratio, lambda_max=lmax)
            assert Sm.kind == "chebyshev" and Sm.dims() == (n, n)
            z = apply_dev(ctx, Sm, b)
            ref = np_cheby(S, lmax, lmax / ratio, m, b)
            info = F.chebyshev_info(Sm)
            zi = np_cheby(S, info["lambda_max"], info["lambda_min"], info["steps"], b)
            e, ei = maxrel(z, ref), maxrel(z, zi)
            print(f"{name} ratio {ratio} m {m}: |z-ref| {e:.2e}  from info {ei:.2e}")
            assert info["lambda_max"] == lmax and info["lambda_min"] == lmax / ratio and info["steps"] == m
            assert e <= 1e-11 and ei <= 1e-11
            # symmetric: transpose_apply is apply; apply_in_place goes through a scratch copy
            import torch
            zt = torch.empty(n, dtype=torch.float64, device="cuda:0")
            Sm.transpose_apply(zt, T(b))
            zp = T(b).clone()
            Sm.apply_in_place(zp)
            ctx.synchronize()
            assert np.array_equal(zt.cpu().numpy(), z) and np.array_equal(zp.cpu().numpy(), z)


# ---------------------------------------------------------- 2. the polynomial

@gpu
def test_the_polynomial(ctx):
    """Z = S I through one block apply (k = 60: two chunks of the 32-column block
    workspace).  Z is symmetric, and I - Z A = T_m((theta - lambda)/delta) / T_m(sigma)
    of D^-1 A: with the spectrum inside (0, lambda_max] every eigenvalue lies in
    [-1/T_m(sigma), 1)."""
    F = fa()
    A, S, lt = operator(ctx, SMALL)
    n = A.nrows
    Ad = S.toarray()
    Lc = np.linalg.cholesky(Ad)
    lmax = lt * (1 + 1e-12)
    for ratio in (4.0, 30.0):
        for m in (1, 2, 3, 5):
            Sm = F.new_chebyshev(A, steps=m, eig_ratio=ratio, lambda_max=lmax)
            bbuf, Bv = device_block(np.eye(n), n + 2)
            obuf, Ov = device_block(np.zeros((n, n)), n + 4)
            Sm.apply(Ov, Bv)
            ctx.synchronize()
            Z = Ov.cpu().numpy()
            assert bool((obuf[:, n:] == PAD).all()) and bool((bbuf[:, n:] == PAD).all())
            asym = np.max(np.abs(Z - Z.T)) / np.max(np.abs(Z))
            sigma = cheby_coeffs(lmax, lmax / ratio, m)[2]
            bound = 1.0 / np.cosh(m * np.arccosh(sigma))
            Zs = 0.5 * (Z + Z.T)
            ev = 1.0 - np.linalg.eigvalsh(Lc.T @ Zs @ Lc)  # eig(I - Z A) = 1 - eig(L^T Z L), A = L L^T
            print(f"ratio {ratio} m {m}: asym {asym:.1e}  eig(I - ZA) in [{ev.min():.6f}, {ev.max():.6f}]  "
                  f"-1/T_m(sigma) = {-bound:.6f}")
            assert asym <= 1e-13
            assert ev.min() >= -bound - 1e-10 and ev.max() < 1.0
            assert maxrel(Z, np_cheby(S, lmax, lmax / ratio, m, np.eye(n))) <= 1e-11


# --------------------------------------------------------- 3. k-wide, bitwise

@gpu
@pytest.mark.parametrize("name,pads", [(SMALL, (8, 16)), (ODD, (8, 16)), (ODD, (9, 17)), ("elasticity", (8, 16))],
                         ids=str)
def test_block_apply_bitwise(ctx, name, pads):
    """Every column of a block apply is the single apply of that column, bit for bit,
    with the padding rows of the blocks intact.  Leading dimensions n + 8 / n + 16 make
    the columns of the odd operator 8-B aligned only (the scalar kernels) against the
    16-B single apply; n + 9 / n + 17 make them 16-B aligned with an odd last row."""
    import torch
    F = fa()
    A, S, lt = operator(ctx, name)
    n = A.nrows
    B = np.random.default_rng(22).uniform(-1, 1, (n, 33))
    for m in (1, 2, 4):
        Sm = F.new_chebyshev(A, steps=m)
        cols = []
        for c in range(33):
            z = torch.empty(n, dtype=torch.float64, device="cuda:0")
            Sm.apply(z, T(B[:, c]))
            ctx.synchronize()
            cols.append(z)
        for k in (1, 3, 8, 11, 33):  # 33 crosses the 32-column chunk
            bbuf, Bv = device_block(B[:, :k], n + pads[0])
            obuf, Ov = device_block(np.zeros((n, k)), n + pads[1])
            Sm.apply(Ov, Bv)
            ctx.synchronize()
            for c in range(k):
                assert torch.equal(Ov[:, c], cols[c]), (name, m, k, c, float((Ov[:, c] - cols[c]).abs().max()))
            assert bool((obuf[:, n:] == PAD).all()) and bool((bbuf[:, n:] == PAD).all())
            assert torch.equal(Bv, T(B[:, :k]))


# ----------------------------------------------------------------- 4. the bound

@gpu
@pytest.mark.parametrize("dims", [(5, 5, 5), (9, 7, 5), (11, 11, 11)], ids=str)
def test_bound_brackets_the_spectrum(ctx, dims):
    """The defaults (10 Lanczos steps, boost 1.1) on 7-point operators: the restatement
    gives lambda_max / lambda_true = 1.072, 1.045, 1.017 and ritz / lambda_true = 0.986,
    0.968, 0.940 on the CPU."""
    F = fa()
    A, S, lt = operator(ctx, dims)
    info = F.chebyshev_info(F.new_chebyshev(A))
    rr = np_lanczos(S, 10)
    print(f"{dims}: lambda_max/true {info['lambda_max'] / lt:.4f}  ritz/true {info['ritz'] / lt:.4f}  "
          f"(restatement {min(1.1 * rr, row_sum_bound(S)) / lt:.4f}, {rr / lt:.4f})  G {info['row_sum_bound']:.4f}")
    assert lt <= info["lambda_max"] <= 1.1 * lt * (1 + 1e-12)
    assert 0.9 * lt <= info["ritz"] <= lt * (1 + 1e-12)
    assert info["eig_iters"] == 10 and info["steps"] == 2
    assert info["lambda_min"] == info["lambda_max"] / 20.0


@gpu
@pytest.mark.parametrize("name", OPERATORS + [(5, 5, 5)], ids=str)
def test_bound_definition(ctx, name):
    F = fa()
    A, S, lt = operator(ctx, name)
    G = row_sum_bound(S)
    for boost, iters in ((1.1, 10), (1.0, 4), (1.3, 64)):
        info = F.chebyshev_info(F.new_chebyshev(A, boost=boost, eig_iters=iters))
        print(f"{name} boost {boost} iters {iters}: {info}  lambda_true {lt:.6f}")
        assert info["lambda_max"] == min(boost * info["ritz"], info["row_sum_bound"])
        assert info["ritz"] <= lt * (1 + 1e-12) <= info["row_sum_bound"] * (1 + 1e-12)
        assert abs(info["row_sum_bound"] - G) <= 1e-13 * G
        assert 1 <= info["eig_iters"] <= iters
    i0 = F.chebyshev_info(F.new_chebyshev(A, eig_iters=0))
    assert i0["lambda_max"] == i0["row_sum_bound"] and abs(i0["row_sum_bound"] - G) <= 1e-13 * G
    assert i0["ritz"] == 0.0 and i0["eig_iters"] == 0
    ig = F.chebyshev_info(F.new_chebyshev(A, lambda_max=1.75, eig_ratio=7.0, steps=3))
    assert ig["lambda_max"] == 1.75 and ig["lambda_min"] == 1.75 / 7.0 and ig["ritz"] == 0.0
    assert ig["eig_iters"] == 0 and ig["steps"] == 3


# ------------------------------------------------------------------ 5. V-cycle

def np_levels(mg):
    """Per level (A, R, P, smoother) downloaded from the device hierarchy; the smoother
    is the restatement with the level's chebyshev_info, the coarsest a dense solve."""
    F = fa()
    out = []
    for l in range(mg.levels()):
        Al, Sl, Rl, Pl = mg.level(l)
        S = Al.to_scipy().tocsr()
        if l == mg.levels() - 1:
            assert Sl.kind == "coarse"
            Ad = S.toarray()
            out.append((S, None, None, lambda r, Ad=Ad: np.linalg.solve(Ad, r)))
        else:
            assert Sl.kind == "chebyshev", Sl.kind
            i = F.chebyshev_info(Sl)
            out.append((S, Rl.to_scipy().tocsr(), Pl.to_scipy().tocsr(),
                        lambda r, S=S, i=i: np_cheby(S, i["lambda_max"], i["lambda_min"], i["steps"], r)))
    return out


def np_cycle(levels, l, v, f, mu, steps):
    """cycle of multigrid.rs:269-380 with smooth() as v <- v + S (f - A v)."""
    A, R, P, sm = levels[l]
    if l == len(levels) - 1:
        return sm(f)
    for _ in range(steps):
        v = v + sm(f - A @ v)
    fc = R @ (f - A @ v)
    vc = np.zeros(len(fc))
    for _ in range(mu):
        vc = np_cycle(levels, l + 1, vc, fc, mu, steps)
    v = v + P @ vc
    for _ in range(steps):
        v = v + sm(f - A @ v)
    return v


_hier = {}


def hierarchy(ctx, which):
    if which not in _hier:
        F = fa()
        if which == "box":
            dims = (16, 16, 16)
            A = F.SparseMatOp.laplace3d_7pt(ctx, *dims)
            _hier[which] = (A, F.sa_build_box(A, dims, (2, 2, 2), coarsest_dim=10, smoother=4))
        else:
            A = F.elasticity_q1((5, 5, 5)).upload(ctx)
            nn = F.constant_candidates(A.nrows, 3)
            _hier[which] = (A, F.smoothed_aggregation(A, nn, block_size=3, candidate_dimension=3, coarsest_dim=20,
                                                      smoother=4, chebyshev_steps=3))
    return _hier[which]


@gpu
@pytest.mark.parametrize("which,mu,steps", [("box", 1, 1), ("box", 2, 2), ("elasticity", 1, 1)])
def test_vcycle_against_numpy(ctx, which, mu, steps):
    import torch
    F = fa()
    A, mg = hierarchy(ctx, which)
    n = A.nrows
    nl = mg.levels()
    assert nl >= 3, nl
    want = 3 if which == "elasticity" else 2
    assert all(F.chebyshev_info(mg.level(l)[1])["steps"] == want for l in range(nl - 1))
    b = np.random.default_rng(23).uniform(-1, 1, n)
    try:
        mg.with_cycle_type(mu).with_smoothing_steps(steps)
        mg.set_graph(False)
        z = apply_dev(ctx, mg, b)
        ref = np_cycle(np_levels(mg), 0, np.zeros(n), b, mu, steps)
        e = maxrel(z, ref)
        print(f"{which} mu {mu} steps {steps}: {nl} levels, |z - numpy cycle| {e:.2e}")
        assert e <= 1e-11
        # graph replay (captured at the first apply, replayed at the second) equals eager
        mg.set_graph(True)
        zg = torch.empty(n, dtype=torch.float64, device="cuda:0")
        bd = T(b)
        for _ in range(2):
            mg.apply(zg, bd)
        ctx.synchronize()
        assert np.array_equal(zg.cpu().numpy(), z)
        # the dense tail (built through cycle(), as for SGS) against every level run
        if mu == 1:
            assert max(p["level"] for p in mg.cycle_plan()) < nl - 1  # the tail is on
            F.set_flag("dense_tail", 0)
            z0 = apply_dev(ctx, mg, b)
            assert max(p["level"] for p in mg.cycle_plan()) == nl - 1
            et = float(np.linalg.norm(z - z0) / np.linalg.norm(z0))
            print(f"dense tail on vs off: {et:.2e}")
            assert et <= 1e-13
    finally:
        F.set_flag("dense_tail", 4096)
        mg.with_cycle_type(1).with_smoothing_steps(1)
        mg.set_graph(True)


# -------------------------------------------------------------- 6. block cycle

@gpu
@pytest.mark.parametrize("tail", [0, 4096])
def test_block_cycle(ctx, tail):
    """On the 16^3 hierarchy with k = 11: every column is the single cycle bit for bit;
    the block plan holds as many cheby_* records as the single cycle's (one k-wide
    launch each, none per column) and every A / R / P launch is one k-wide spmm_*."""
    import torch
    F = fa()
    A, mg = hierarchy(ctx, "box")
    n, k = A.nrows, 11
    B = np.random.default_rng(24).uniform(-1, 1, (n, k))
    try:
        F.set_flag("dense_tail", tail)
        cols = []
        for c in range(k):
            z = torch.empty(n, dtype=torch.float64, device="cuda:0")
            mg.apply(z, T(B[:, c]))
            ctx.synchronize()
            cols.append(z)
        bbuf, Bv = device_block(B, n + 8)
        obuf, Ov = device_block(np.zeros((n, k)), n + 16)
        mg.apply(Ov, Bv)
        ctx.synchronize()
        for c in range(k):
            assert torch.equal(Ov[:, c], cols[c]), (c, float((Ov[:, c] - cols[c]).abs().max()))
        assert bool((obuf[:, n:] == PAD).all()) and bool((bbuf[:, n:] == PAD).all())
        p1, pk = mg.cycle_plan(), mg.block_plan(k)
        ch1 = [(p["level"], p["name"]) for p in p1 if p["name"].startswith("cheby_")]
        chk = [(p["level"], p["name"]) for p in pk if p["name"].startswith("cheby_")]
        print(f"tail {tail}: cheby records single {len(ch1)} block {len(chk)}; block plan:",
              [(p["level"], p["name"]) for p in pk])
        assert ch1 and chk == ch1
        nlev = len({l for l, _ in ch1})
        assert len(ch1) == 4 * nlev  # steps 2: first + last, before and after the coarse visit
        mats = [p for p in pk if p["kernel"] >= 0]
        assert mats and all(p["name"].startswith("spmm_") for p in mats), [p["name"] for p in mats]
        # the bytes of the records (n = rows): first 8n + 24nk, last 8n + 32nk
        for p in pk:
            if p["name"] == "cheby_first":
                assert p["bytes"] == 8 * p["rows"] + 24 * p["rows"] * k
            if p["name"] == "cheby_step":
                assert p["bytes"] == 8 * p["rows"] + 32 * p["rows"] * k
    finally:
        F.set_flag("dense_tail", 4096)


@gpu
def test_launch_record_bytes(ctx, no_tail):
    """steps 3 (first, step, last) and steps 1 (x only) through a two-level multigrid's plan."""
    F = fa()
    dims = (6, 5, 4)
    A = F.SparseMatOp.laplace3d_7pt(ctx, *dims)
    n = A.nrows
    box = F.sa_build_box(A, dims, (2, 2, 2), coarsest_dim=20, smoother="jacobi")
    _, _, R, P = box.level(0)
    Ac, Sc = box.level(1)[0], box.level(1)[1]
    for m, want in ((3, [("cheby_first", 32), ("cheby_step", 48), ("cheby_step", 40)]), (1, [("cheby_first", 24)])):
        mg = F.Multigrid(A, F.new_chebyshev(A, steps=m))
        mg.add_level(Ac, Sc, R, P)
        pre = [(p["name"], p["bytes"]) for p in mg.cycle_plan() if p["name"].startswith("cheby_")][:len(want)]
        assert pre == [(name, per_row * n) for name, per_row in want], pre
        blk = [(p["name"], p["bytes"]) for p in mg.block_plan(5) if p["name"].startswith("cheby_")][:len(want)]
        assert blk == [(name, (8 + (per_row - 8) * 5) * n) for name, per_row in want], blk


# -------------------------------------------------------------------- 7. solves

@gpu
def test_solves(ctx):
    """elasticity_q1((6, 6, 6)), SA with coarsest_dim 60 (the default 1000 would leave one
    level: a direct solve), rel_tol 1e-8: PCG with the Chebyshev hierarchy converges in
    no more iterations than with the L1 hierarchy (the restatement on a numpy SA
    hierarchy of the same operator: 30 against 69), and the block driver is bitwise the single solves."""
    import torch
    F = fa()
    A = F.elasticity_q1((6, 6, 6)).upload(ctx)
    n = A.nrows
    nn = F.constant_candidates(n, 3)
    sa = dict(block_size=3, candidate_dimension=3, coarsest_dim=60)
    mg_c = F.smoothed_aggregation(A, nn, smoother=4, **sa)
    mg_l = F.smoothed_aggregation(A, nn, smoother="l1", **sa)
    assert mg_c.levels() >= 2 and mg_c.level(0)[1].kind == "chebyshev"
    B = np.random.default_rng(25).uniform(-1, 1, (n, 3))
    its = {}
    xs = []
    for name, mg in (("chebyshev", mg_c), ("l1", mg_l)):
        x = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        its[name], hist = F.pcg_solve(A, mg, T(B[:, 0]), x, max_iter=200, rel_tol=1e-8)
        ctx.synchronize()
        res = np.linalg.norm(B[:, 0] - A.to_scipy() @ x.cpu().numpy()) / np.linalg.norm(B[:, 0])
        print(f"pcg {name}: {its[name]} iterations, true residual {res:.2e}")
        assert its[name] <= 200 and res <= 1e-7
    assert its["chebyshev"] <= its["l1"]
    singles = []
    for c in range(3):
        x = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        it, hist = F.pcg_solve(A, mg_c, T(B[:, c]), x, max_iter=200, rel_tol=1e-8)
        ctx.synchronize()
        singles.append((x, int(it), np.array(hist)))
    bbuf, Bv = device_block(B, n + 8)
    xbuf, Xv = device_block(np.zeros((n, 3)), n + 16)
    itb, histb = F.pcg_solve_block(A, mg_c, Bv, Xv, max_iter=200, rel_tol=1e-8)
    ctx.synchronize()
    for c in range(3):
        assert torch.equal(Xv[:, c], singles[c][0]), c
        assert int(itb[c]) == singles[c][1]
        assert np.array_equal(np.array(histb[c]), singles[c][2])
    assert bool((xbuf[:, n:] == PAD).all()) and bool((bbuf[:, n:] == PAD).all())


# -------------------------------------------------------------------- 8. errors

@gpu
def test_errors(ctx):
    F = fa()
    L = F.lib()
    A, S, lt = operator(ctx, SMALL)
    out = C.c_void_p()

    def create(op, **kw):
        cfg = F.ChebyshevConfig(**kw)
        st = L.amg_chebyshev_create(op.h, C.byref(cfg), C.byref(out))
        return st, L.amg_last_error()

    R = F.SparseMatOp.from_scipy(ctx, S[:40, :].tocsr())
    st, msg = create(R)
    assert st == DIM and b"square" in msg
    # an explicit zero on the diagonal, and a row without a diagonal entry
    rp, ci = np.array([0, 2, 4, 5]), np.array([0, 1, 0, 1, 2])
    Z = F.SparseMatOp.from_arrays(ctx, 3, 3, rp, ci, np.array([2.0, -1.0, -1.0, 0.0, 2.0]))
    st, msg = create(Z)
    assert st == NOT_SPD and b"diagonal" in msg
    Nn = F.SparseMatOp.from_arrays(ctx, 3, 3, rp, ci, np.array([2.0, -1.0, -1.0, -3.0, 2.0]))
    assert create(Nn)[0] == NOT_SPD
    Mi = F.SparseMatOp.from_arrays(ctx, 3, 3, np.array([0, 2, 3, 4]), np.array([0, 1, 0, 2]),
                                   np.array([2.0, -1.0, -1.0, 2.0]))
    assert create(Mi)[0] == NOT_SPD
    for bad in (dict(steps=0), dict(eig_ratio=1.0), dict(boost=0.5), dict(eig_iters=65), dict(eig_iters=-1),
                dict(lambda_max=-1.0)):
        st, msg = create(A, **bad)
        assert st == INVALID and b"chebyshev" in msg, (bad, msg)
    assert out.value is None
    info = np.zeros(6)
    J = F.new_jacobi(A)  # kept alive: destroying a handle resets the thread's last error
    assert L.amg_chebyshev_info(J.h, info.ctypes.data_as(C.c_void_p)) == INVALID
    assert b"not a Chebyshev" in L.amg_last_error()
    with pytest.raises(F.AmgError):
        F.sa_build_box(A, SMALL, (2, 2, 2), coarsest_dim=10, smoother=5)
    # a null config is the defaults
    assert L.amg_chebyshev_create(A.h, None, C.byref(out)) == OK and out.value
    D = F.LinOp(out, ctx)
    assert F.chebyshev_info(D) == F.chebyshev_info(F.new_chebyshev(A))
    assert F.chebyshev_info(D)["steps"] == 2 and F.chebyshev_info(D)["eig_iters"] == 10
