"""The row-per-wave SpMV kernels against a high-precision host reference.

Two kernel families put one wavefront (or 2 or 4) on a row and finish with a lane
butterfly: the wave-per-row CSR kernel (spmv.hip spmv_vector_kernel: 6 storage
variants x 3 waves per row x 7 modes) and the one-row-per-wave stencil-class
kernels (scs.hip spmv_scs_lanes_kernel, spmm.hip spmm_scs_lanes_kernel).  Every
operator here is synthetic (numpy, fixed seeds) and uploaded with
SparseMatOp.from_arrays; every test asserts the storage it depends on.

Reference: row sums in np.longdouble (>= 63 mantissa bits; exact Fraction sums
where the platform's long double is no wider than double), epilogues in the same
precision.  With u = 2^-53, n_i the stored entries of row i, S_i = sum_j |a_ij||x_j|
and E_i = 2 n_i u S_i (spmv_bound of test_gpu_parity.py, valid for any summation
order; padding terms fma(+0.0, finite, acc) round nothing) the per-row tolerances
are one rounding per operation of epi_value (spmv_dev.hpp):
    set     E_i
    add     E_i + u |ref_i|
    resid   E_i + u |ref_i|
    jacobi  |d_i| E_i + 2 u (|x_i| + |d_i| (|b_i| + S_i))
plus 1e-300; an empty row must come out exact (0, y0, b, fl(x + fl(d b))).

Bitwise on top: the same call twice gives the same bits; every k-wide result
(amg_csr_spmm_epilogue with leading dimensions above n and untouched padding rows,
k in (1, 3, 8, 11); A.apply on 3 columns) equals the single-vector call column by
column.

The host-only tests at the end need no GPU; the scs-* cases call
amg_grid_from_offsets and so, like tests/test_capi.py, need the built library.  They
check the builders and check the tolerances against a plain double evaluation of the
same sums.
"""
import numpy as np
import pytest

gpu = pytest.mark.gpu
U = 2.0 ** -53
LD = np.longdouble
LD_OK = np.finfo(LD).nmant >= 63
MODES = ("set", "add", "resid", "jacobi")
PAD = 7.5


def fa():
    import faer_amg_amd
    return faer_amg_amd


def T(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda:0")


# ------------------------------------------------------------------ reference

def row_sums(rp, col, val, x):
    """(sum_j a_ij x_j, sum_j |a_ij| |x_j|) of every row, as np.longdouble."""
    n = len(rp) - 1
    s, S = np.zeros(n, LD), np.zeros(n, LD)
    live = np.diff(rp) > 0
    if not live.any():
        return s, S
    if LD_OK:
        assert np.finfo(np.longdouble).nmant >= 63
        prod = val.astype(LD) * x[col].astype(LD)
        starts = rp[:-1][live]  # empty rows hold no entries: consecutive live starts bound one row each
        s[live] = np.add.reduceat(prod, starts)
        S[live] = np.add.reduceat(np.abs(prod), starts)
        return s, S
    from fractions import Fraction
    for i in np.flatnonzero(live):
        t = [Fraction(float(val[e])) * Fraction(float(x[col[e]])) for e in range(rp[i], rp[i + 1])]
        s[i], S[i] = float(sum(t)), float(sum(abs(q) for q in t))
    return s, S


class Case:
    """A CSR operator with its vectors, the reference of every mode and its tolerance.
    ncols (default n: square) sizes x; the Jacobi epilogue reads x_i of every row, so x
    of an operator with more rows than columns is drawn n long."""

    def __init__(self, name, n, rp, col, val, seed, forced=False, expect=None, ncols=None):
        self.name, self.n, self.forced, self.expect = name, n, forced, expect or {}
        self.ncols = n if ncols is None else ncols
        self.rp, self.col, self.val = rp.astype(np.int64), col.astype(np.int64), val.astype(np.float64)
        rng = np.random.default_rng(seed)
        self.x, self.b, self.y0 = (rng.uniform(-1, 1, m) for m in (max(n, self.ncols), n, n))
        self.d = rng.uniform(0.1, 0.2, n)
        self.lens = np.diff(self.rp)
        self._ref = None
        self.worst = (0.0, None, 0)  # largest error / tolerance check() saw, its mode and the row's entries

    @property
    def nnz(self):
        return int(self.rp[-1])

    def reference(self):
        """{mode: (ref, tol)} in np.longdouble; computed once."""
        if self._ref is None:
            s, S = row_sums(self.rp, self.col, self.val, self.x)
            x, b, y0, d = (v.astype(LD) for v in (self.x[:self.n], self.b, self.y0, self.d))
            E = 2 * self.lens.astype(LD) * LD(U) * S
            tiny = LD(1e-300)
            ref = {"set": s, "add": y0 + s, "resid": b - s, "jacobi": x + d * (b - s)}
            tol = {"set": E + tiny,
                   "add": E + LD(U) * np.abs(ref["add"]) + tiny,
                   "resid": E + LD(U) * np.abs(ref["resid"]) + tiny,
                   "jacobi": np.abs(d) * E + 2 * LD(U) * (np.abs(x) + np.abs(d) * (np.abs(b) + S)) + tiny}
            self._ref = {m: (ref[m], tol[m]) for m in MODES}
        return self._ref

    def empty_exact(self, mode):
        """What an empty row holds, rounded as the kernel rounds it (acc = +0.0)."""
        e = self.lens == 0
        x, b, y0, d = self.x[:self.n][e], self.b[e], self.y0[e], self.d[e]
        return {"set": np.zeros(int(e.sum())), "add": y0 + 0.0, "resid": b - 0.0, "jacobi": x + d * (b - 0.0)}[mode]

    def check(self, mode, y):
        """max error / tolerance of y (asserted <= 1); empty rows exact."""
        ref, tol = self.reference()[mode]
        assert np.all(np.isfinite(y)), (self.name, mode)
        ratio = np.abs(y.astype(LD) - ref) / tol
        worst = int(np.argmax(ratio))
        assert ratio[worst] <= 1, (self.name, mode, worst, int(self.lens[worst]), float(ratio[worst]))
        assert np.array_equal(y[self.lens == 0], self.empty_exact(mode)), (self.name, mode, "empty rows")
        self.worst = max(self.worst, (float(ratio[worst]), mode, int(self.lens[worst])), key=lambda t: t[0])
        return float(ratio[worst])

    def upload(self, ctx):
        F = fa()
        try:
            if self.forced:
                F.set_spmv_format("vector")
            return F.SparseMatOp.from_arrays(ctx, self.n, self.ncols, self.rp, self.col, self.val)
        finally:
            F.set_spmv_format("auto")


def check_csr(c):
    """Sorted, in-range CSR with strictly ascending columns in every row."""
    assert c.rp[0] == 0 and len(c.rp) == c.n + 1 and np.all(np.diff(c.rp) >= 0)
    assert len(c.col) == len(c.val) == c.nnz
    assert c.col.min() >= 0 and c.col.max() < c.ncols
    inner = np.ones(c.nnz, bool)
    inner[c.rp[:-1][c.lens > 0]] = False  # the first entry of a row has no predecessor in it
    assert np.all(np.diff(c.col)[inner[1:]] > 0)
    assert np.all(np.isfinite(c.val))


# ------------------------------------------------------- 1. wave-per-row CSR

# row lengths on both sides of every 64-entry chunk edge of 1, 2 and 4 waves per row and
# of the 4x unrolled loop (it needs more than 3 * 64 * WPR entries: 192, 384, 768)
EDGES = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1100)
N_RAGGED = 2051  # odd, no multiple of 4: the last workgroup has dead row slots at 1 and 2 waves per row


def ragged_pattern(n, every, fill, seed):
    """Row i takes the next length of EDGES when i % every == 0, else a mid length
    drawn from fill; the last row has n - 1 > 2048 entries.  Columns random, sorted."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(fill[0], fill[1] + 1, n)
    idx = np.arange(0, n, every)
    lens[idx] = np.asarray(EDGES)[np.arange(len(idx)) % len(EDGES)]
    lens[n - 1] = n - 1
    rp = np.concatenate(([0], np.cumsum(lens)))
    col = np.concatenate([np.sort(rng.choice(n, int(k), replace=False)) for k in lens])
    return rp, col


def values(nnz, table, seed):
    """nnz values from a table of `table` distinct ones (0: all distinct)."""
    rng = np.random.default_rng(seed)
    if table == 0:
        v = rng.uniform(0.5, 1.5, nnz) * rng.choice((-1.0, 1.0), nnz)
        assert len(np.unique(v)) == nnz
        return v
    tab = rng.uniform(0.5, 1.5, table) * rng.choice((-1.0, 1.0), table)
    v = tab[rng.integers(0, table, nnz)]
    v[:table] = tab  # every table value is present
    return v


def far_rows(n, seed, plus=None):
    """n rows, nearly all empty; 20 long rows from row 0 and 20 up to the last row.
    plus None: columns anywhere (offsets beyond +-32767).  Else every offset lies
    within +-32767 but the largest, exactly +plus in row 0; the smallest is exactly
    -32767, in row n - 1."""
    rng = np.random.default_rng(seed)
    long_lens = [k for k in EDGES if k] + [3000] * 20
    rows = list(range(20)) + list(range(n - 20, n))
    lens = np.zeros(n, np.int64)
    cols = {}
    for r, k in zip(rows, long_lens):
        if plus is None:
            c = rng.choice(n, k, replace=False)
        else:
            lo, hi = max(0, r - 32767), min(n - 1, r + 32767)
            c = rng.choice(np.arange(lo, hi + 1), k, replace=False)
            pin = plus if r == 0 else r - 32767 if r == n - 1 else None
            if pin is not None and pin not in c:
                c[0] = pin
        cols[r] = np.sort(c)
        lens[r] = k
    rp = np.concatenate(([0], np.cumsum(lens)))
    return rp, np.concatenate([cols[r] for r in rows])


_cases = {}


def vec_case(name):
    """The operators of sections 1.1-1.3 (built once per process).
    expect: value bits and bytes per column entry (2: 16-bit offsets, 4: int32)."""
    if name in _cases:
        return _cases[name]
    if name.startswith("ragged"):  # 1.1 / 1.2: 16-bit offsets, three value widths
        table, vbits = {"ragged-v8": (200, 8), "ragged-v16": (5000, 16), "ragged-fp64": (0, 0)}[name]
        rp, col = ragged_pattern(N_RAGGED, 3, (150, 330), 101)
        avg = rp[-1] / N_RAGGED
        assert 256 <= avg < 512 and rp[-1] > 65536, avg  # the default policy picks the kernel, 2 waves per row
        c = Case(name, N_RAGGED, rp, col, values(rp[-1], table, 102), 103, expect={"vbits": vbits, "obytes": 2})
    elif name == "long-v16":  # 1.1: average length >= 512, 4 waves per row
        rp, col = ragged_pattern(N_RAGGED, 2, (500, 900), 111)
        assert rp[-1] / N_RAGGED >= 512
        c = Case(name, N_RAGGED, rp, col, values(rp[-1], 5000, 112), 113, expect={"vbits": 16, "obytes": 2})
    elif name.startswith("far"):  # 1.2: int32 columns, three value widths, forced format
        table, vbits = {"far-v8": (200, 8), "far-v16": (5000, 16), "far-fp64": (0, 0)}[name]
        rp, col = far_rows(33000, 121)
        assert rp[-1] > 65536 and np.abs(col - np.repeat(np.arange(33000), np.diff(rp))).max() > 32767
        c = Case(name, 33000, rp, col, values(rp[-1], table, 122), 123, forced=True,
                 expect={"vbits": vbits, "obytes": 4})
    else:  # 1.3: the int16 boundary
        plus, obytes = {"edge-32767": (32767, 2), "edge-32768": (32768, 4)}[name]
        n = 33001
        rp, col = far_rows(n, 131, plus=plus)
        rows = np.repeat(np.arange(n), np.diff(rp))
        off = col - rows
        assert off.max() == plus and off.min() == -32767
        assert np.sum(np.abs(off) > 32767) == (1 if plus == 32768 else 0)
        c = Case(name, n, rp, col, values(rp[-1], 5000, 132), 133, forced=True,
                 expect={"vbits": 16, "obytes": obytes})
    _cases[name] = c
    return c


VEC_CASES = ("ragged-v8", "ragged-v16", "ragged-fp64", "long-v16", "far-v8", "far-v16", "far-fp64",
             "edge-32767", "edge-32768")


def vector_column_bytes(info, c):
    """Bytes per column entry of the wave-per-row storage, from its streamed bytes
    (GpuCsr::stream_bytes: nnz (value + column bytes) + 4 (n + 1) + 8 table entries)."""
    per_entry, rem = divmod(info["stream_bytes"] - 4 * (c.n + 1) - 8 * info["value_table"], c.nnz)
    assert rem == 0, info
    return per_entry - (info["value_bits"] // 8 if info["value_bits"] else 8)


def run_modes(ctx, A, c):
    """Every mode through spmv_epilogue, twice (same bits); {mode: y}."""
    import torch
    xd, bd, dd = T(c.x), T(c.b), T(c.d)
    out = {}
    for mode in MODES:
        ys = []
        for _ in range(2):
            y = T(c.y0)
            A.spmv_epilogue(mode, xd, y, bd, dd)
            ctx.synchronize()
            ys.append(y)
        assert torch.equal(ys[0], ys[1]), (c.name, mode, "not repeatable")
        out[mode] = ys[0].cpu().numpy()
    return out


def device_block(X, ld):
    """X (numpy n x k) as a column-major torch device view with leading dimension ld."""
    import torch
    n, k = X.shape
    buf = torch.full((k, ld), PAD, dtype=torch.float64, device="cuda:0")
    buf[:, :n] = torch.as_tensor(np.ascontiguousarray(X.T), device="cuda:0")
    return buf, buf[:, :n].t()


def kwide_mismatches(ctx, A, ks=(1, 3, 8, 11), seed=12):
    """spmm_epi_vs_spmv of test_gpu_block_cycle.py, counting: the entries of
    amg_csr_spmm_epilogue (every mode and k, ldx, ldy, ldb > n) that differ in bits
    from amg_csr_spmv_epilogue of their column.  The padding rows stay untouched."""
    import torch
    n = A.nrows
    rng = np.random.default_rng(seed)
    kmax = max(ks)
    X, B, Y0 = (rng.uniform(-1, 1, (n, kmax)) for _ in range(3))
    d = T(rng.uniform(0.1, 0.2, n))
    bad = 0
    for k in ks:
        xbuf, Xv = device_block(X[:, :k], n + 3)
        bbuf, Bv = device_block(B[:, :k], n + 1)
        for mode in MODES:
            ybuf, Yv = device_block(Y0[:, :k], n + 5)
            A.spmm_epilogue(mode, Xv, Yv, Bv, d)
            ctx.synchronize()
            for c in range(k):
                y1 = T(Y0[:, c])
                A.spmv_epilogue(mode, Xv[:, c].contiguous(), y1, Bv[:, c].contiguous(), d)
                ctx.synchronize()
                bad += int((Yv[:, c].contiguous().view(dtype=torch.int64) != y1.view(dtype=torch.int64)).sum())
            assert bool((ybuf[:, n:] == PAD).all()) and bool((xbuf[:, n:] == PAD).all())
            assert bool((bbuf[:, n:] == PAD).all())
    return bad


def apply3_mismatches(ctx, A, seed=13):
    """A.apply on a 3-column block against A.apply of every column, in differing bits."""
    import torch
    n = A.nrows
    X = np.random.default_rng(seed).uniform(-1, 1, (n, 3))
    xbuf, Xv = device_block(X, n + 3)
    ybuf, Yv = device_block(np.zeros((n, 3)), n + 5)
    A.apply(Yv, Xv)
    ctx.synchronize()
    bad = 0
    for c in range(3):
        y1 = torch.empty(n, dtype=torch.float64, device="cuda:0")
        A.apply(y1, Xv[:, c].contiguous())
        ctx.synchronize()
        bad += int((Yv[:, c].contiguous().view(dtype=torch.int64) != y1.view(dtype=torch.int64)).sum())
    assert bool((ybuf[:, n:] == PAD).all()) and bool((xbuf[:, n:] == PAD).all())
    return bad


@gpu
@pytest.mark.parametrize("name", VEC_CASES)
def test_vector_kernel(ctx, name):
    """Sections 1.1-1.4: ragged rows around every chunk edge, the six storage variants,
    the int16 offset boundary; 1, 2, 4 and the automatic waves per row; four modes
    against the reference, repeatable, and the k-wide calls bitwise per column."""
    F = fa()
    c = vec_case(name)
    A = c.upload(ctx)
    info = A.spmv_info()
    assert info["kernel"] == "vector", info
    assert info["value_bits"] == c.expect["vbits"], info
    assert vector_column_bytes(info, c) == c.expect["obytes"], info
    c.worst = (0.0, None, 0)
    try:
        for w in (1, 2, 4, 0):
            F.set_flag("vec_wpr", w)
            for mode, y in run_modes(ctx, A, c).items():
                c.check(mode, y)
            bad = kwide_mismatches(ctx, A) + apply3_mismatches(ctx, A)
            assert bad == 0, (name, w, bad)
    finally:
        F.set_flag("vec_wpr", 0)
    print(f"wave-per-row {name}: value bits {info['value_bits']}, column bytes {c.expect['obytes']}, "
          "max error / tolerance %.3g (%s, a row of %d entries)" % c.worst)


def _level0(plan):
    return [p for p in plan if p["level"] == 0]


def _jacobi_cycle(ctx, mg, b, all_vector):
    """One V-cycle of mg with the zero-guess fold on and off against the oracle at
    1e-11.  Level 0's launches on A (smoothing, residual) carry name `vector` in
    modes RESID0 / JACOBI with the fold and RESID / JACOBI without; all_vector: so do
    R's SET and P's ADD0 / ADD (no grid-transfer overlay in front of them)."""
    import oracle as O
    from test_gpu_parity import apply_dev, oracle_levels_from_gpu
    zref = O.Multigrid(oracle_levels_from_gpu(mg, "jacobi")).apply(b)
    for fold in (True, False):
        mg.set_fold_zero_guess(fold)
        plan = mg.cycle_plan()
        print(f"jacobi, fold {fold}:", [(p["level"], p["role"], p["mode"], p["name"]) for p in plan])
        lv0 = [p for p in _level0(plan) if p["mode"] != "-"]  # ("-": the unfolded d * f pass)
        assert [p["mode"] for p in lv0] == (["RESID0", "SET", "ADD0", "JACOBI"] if fold
                                            else ["RESID", "SET", "ADD", "JACOBI"]), lv0
        assert [p["role"] for p in lv0] == ["resid", "restrict", "interp", "smooth"], lv0
        on_vector = lv0 if all_vector else [lv0[0], lv0[3]]
        assert all(p["name"] == "vector" for p in on_vector), lv0
        z = apply_dev(ctx, mg, b, len(b))
        assert np.linalg.norm(z - zref) <= 1e-11 * np.linalg.norm(zref), fold
    mg.set_fold_zero_guess(True)


@gpu
def test_vector_vcycle_fold_and_sgs(ctx):
    """Section 1.5: RESID0 / ADD0 (the folded zero-guess step; wave-per-row levels fold
    under flag fold_xscs) and SGS colour segments on the wave-per-row kernel, on the
    20 x 16 x 12 box hierarchy of test_vcycle_forced_sell, against the oracle at 1e-11.
    sa_build_box puts the grid-transfer overlay in front of R_0 and P_0 whatever the
    format, so there only A_0's RESID0 runs on the kernel; the same A_0, R_0, P_0, A_1
    uploaded again as a two-level Multigrid with A_0's grid hint cleared have no
    overlay, and R_0's SET and P_0's ADD0 run on the kernel too."""
    import oracle as O
    from test_gpu_parity import apply_dev, oracle_levels_from_gpu
    F = fa()
    dims = (20, 16, 12)
    fold_flag = F.get_flag("fold_xscs")
    try:
        F.set_spmv_format("vector")
        F.set_flag("fold_xscs", 1)
        A = F.SparseMatOp.laplace3d_7pt(ctx, *dims)
        assert A.spmv_info()["kernel"] == "vector"
        b = np.random.default_rng(12).uniform(-1, 1, A.nrows)
        mg = F.sa_build_box(A, dims, (2, 2, 2), coarsest_dim=200)
        _jacobi_cycle(ctx, mg, b, all_vector=False)

        def again(M):
            return F.SparseMatOp.from_arrays(ctx, *M.dims(), *M.arrays())
        A0, R0, P0, A1 = again(A), again(mg.level(0)[2]), again(mg.level(0)[3]), again(mg.level(1)[0])
        A0.set_grid(0, 0, 0)  # a cleared hint: nothing is inferred, add_level attaches no overlay
        m2 = F.Multigrid(A0, F.new_jacobi(A0, 0.66))
        m2.add_level(A1, F.CoarseCholesky(A1), R0, P0)
        for M in m2.level(0)[0:1] + m2.level(0)[2:4]:  # (an overlay would report "gtc")
            assert M.spmv_info()["kernel"] == "vector", M.spmv_info()
        _jacobi_cycle(ctx, m2, b, all_vector=True)

        ms = F.sa_build_box(A, dims, (2, 2, 2), coarsest_dim=200, smoother="sgs")
        levels = oracle_levels_from_gpu(ms, "sgs")
        assert levels[0]["smoother"] == "sgs"
        assert F.sgs_info(ms.level(0)[1])["kernel"] == "vector"
        plan = ms.cycle_plan()
        print("sgs:", [(p["level"], p["role"], p["mode"], p["name"]) for p in plan])
        own = [p for p in _level0(plan) if p["role"] in ("smooth", "resid") and p["mode"] != "-"]
        assert {"SGS", "RESID"} <= {p["mode"] for p in own} and all(p["name"] == "vector" for p in own), own
        z = apply_dev(ctx, ms, b, A.nrows)
        zref = O.Multigrid(levels).apply(b)
        assert np.linalg.norm(z - zref) <= 1e-11 * np.linalg.norm(zref)
    finally:
        F.set_spmv_format("auto")
        F.set_flag("fold_xscs", fold_flag)


@gpu
def test_vector_sgs_colour_segments(ctx):
    """Section 1.5: the colour sweeps of SymGaussSeidel on aniso27(9, 8, 7) under the
    forced format (8 colour segments, row_begin != 0, 16-bit row + off columns of the
    colour-permuted copy) against the oracle's SGS, as test_sgs_matches_oracle."""
    import oracle as O
    from test_gpu_parity import apply_dev, gpu_csr
    F = fa()
    try:
        F.set_spmv_format("vector")
        OA = O.aniso27(9, 8, 7)
        A = gpu_csr(ctx, OA)
        S = F.SymGaussSeidel(A)
        assert A.spmv_info()["kernel"] == "vector" and S.sweep_storage()["kernel"] == "vector"
        color, nc = O.greedy_coloring(OA)
        assert S.ncolors == nc == 8
        r = np.random.default_rng(5).standard_normal(OA.nrows)
        e = apply_dev(ctx, S, r, OA.nrows)
        eref = O.sgs_apply(OA, color, nc, r)
        assert np.linalg.norm(e - eref) <= 1e-13 * np.linalg.norm(eref)
    finally:
        F.set_spmv_format("auto")


# ------------------------------------- 2. one-row-per-wave stencil classes

def banded_two_class(n, J, seed):
    """Offsets 2j, |j| <= J.  Rows where the whole stencil fits take values
    v[i mod 2][j] (two classes, 2 (2J + 1) distinct values); every other row holds
    one diagonal entry of one shared value (a third class)."""
    rng = np.random.default_rng(seed)
    K = 2 * J + 1
    offs = 2 * np.arange(-J, J + 1)
    v = rng.uniform(0.5, 1.5, (2, K)) * rng.choice((-1.0, 1.0), (2, K))
    assert len(np.unique(v)) == 2 * K
    i = np.arange(n)
    inner = (i - 2 * J >= 0) & (i + 2 * J < n)
    lens = np.where(inner, K, 1)
    rp = np.concatenate(([0], np.cumsum(lens)))
    col = np.empty(rp[-1], np.int64)
    val = np.empty(rp[-1])
    ii = i[inner]
    pos = rp[:-1][inner][:, None] + np.arange(K)[None, :]
    col[pos] = ii[:, None] + offs[None, :]
    val[pos] = v[ii % 2]
    col[rp[:-1][~inner]] = i[~inner]
    val[rp[:-1][~inner]] = 2.75
    return rp, col, val


def banded_truncated(n, J, seed):
    """Offsets 2j, |j| <= J, one random value per offset, rows truncated at the
    matrix edges: rows 2m and 2m + 1 near an edge share a class, J + J + 1 classes."""
    rng = np.random.default_rng(seed)
    K = 2 * J + 1
    offs = 2 * np.arange(-J, J + 1)
    v = rng.uniform(0.5, 1.5, K) * rng.choice((-1.0, 1.0), K)
    assert len(np.unique(v)) == K
    c = np.arange(n)[:, None] + offs[None, :]
    keep = (c >= 0) & (c < n)
    rp = np.concatenate(([0], np.cumsum(keep.sum(axis=1))))
    return rp, c[keep], np.broadcast_to(v, c.shape)[keep]


# name: (builder, n, J, classes, padded offsets, class id bits).  K = 2J + 1 offsets are
# padded to a multiple of 8; a lane takes the offset pairs 2q, 2q + 1 of every 128-offset
# block, so 264 leaves the third block live in 4 lanes, and 528 / 1024 enter the k-wide
# kernel's 512-offset steps (1024: the kernel's eight-block maximum).
SCS_SHAPES = {
    "a": (banded_two_class, 2048, 128, 3, 264, 8),
    "b": (banded_truncated, 1536, 140, 281, 288, 16),
    "c": (banded_two_class, 3072, 260, 3, 528, 8),
    "d": (banded_truncated, 4096, 511, 1023, 1024, 16),
}


def scs_case(name):
    if ("scs", name) not in _cases:
        build, n, J, _, _, _ = SCS_SHAPES[name]
        rp, col, val = build(n, J, 200 + ord(name))
        _cases["scs", name] = Case("classes-" + name, n, rp, col, val, 300 + ord(name))
    return _cases["scs", name]


def two_level(ctx, A):
    """A two-level Multigrid around A (aggregates of 64 rows, an identity coarse
    operator): only its launch plans are read."""
    import scipy.sparse as sp
    F = fa()
    n = A.nrows
    nc = n // 64
    P = sp.csr_matrix((np.ones(n), (np.arange(n), np.arange(n) // 64)), shape=(n, nc))
    Pd, Rd = F.SparseMatOp.from_scipy(ctx, P), F.SparseMatOp.from_scipy(ctx, P.T.tocsr())
    Ac = F.SparseMatOp.from_scipy(ctx, sp.identity(nc, format="csr"))
    mg = F.Multigrid(A, F.new_jacobi(A))
    mg.add_level(Ac, F.CoarseCholesky(Ac), Rd, Pd)
    return mg


@gpu
@pytest.mark.parametrize("name", sorted(SCS_SHAPES))
def test_class_lanes_kernels(ctx, name):
    """Section 2.  Shapes (final): (a) J = 128, n = 2048, 3 classes, 264 padded offsets,
    8-bit ids; (b) J = 140, n = 1536, 281 classes, 288, 16-bit; (c) J = 260, n = 3072,
    3 classes, 528; (d) J = 511, n = 4096, 1023 classes, 1024.  The launch names
    scs_lanes / spmm_scs come from the plans of a two-level Multigrid around the
    operator.  Four modes against the reference, repeatable; amg_csr_spmm_epilogue
    and a 3-column apply bitwise per column."""
    _, n, J, classes, kp, bits = SCS_SHAPES[name]
    c = scs_case(name)
    A = c.upload(ctx)
    info = A.spmv_info()
    assert info["kernel"] == "classes" and not info["xstaged"] and info["grid_source"] == "none", info
    assert (info["classes"], info["class_offsets"], info["class_id_bits"]) == (classes, kp, bits), info
    mg = two_level(ctx, A)
    plan, bplan = mg.cycle_plan(), mg.block_plan(3)
    print("plan:", [(p["level"], p["role"], p["mode"], p["name"]) for p in plan])
    print("block plan:", [(p["level"], p["role"], p["mode"], p["name"]) for p in bplan])
    for pl, want in ((plan, "scs_lanes"), (bplan, "spmm_scs")):
        own = [p for p in _level0(pl) if p["mode"] in ("RESID", "JACOBI")]
        assert {p["mode"] for p in own} == {"RESID", "JACOBI"} and all(p["name"] == want for p in own), pl
    c.worst = (0.0, None, 0)
    for mode, y in run_modes(ctx, A, c).items():
        c.check(mode, y)
    print(f"stencil classes ({name}): {info['classes']} classes, {info['class_offsets']} offsets, "
          "max error / tolerance %.3g (%s, a row of %d entries)" % c.worst)
    bad_k, bad_a = kwide_mismatches(ctx, A), apply3_mismatches(ctx, A)
    print(f"stencil classes ({name}): k-wide entries differing from the per-column call: "
          f"spmm_epilogue {bad_k}, apply {bad_a}")
    assert bad_k == 0 and bad_a == 0, (name, bad_k, bad_a)


# ------------------------------------------------------- host-only checks

@pytest.mark.parametrize("name", VEC_CASES + tuple("scs-" + k for k in sorted(SCS_SHAPES)))
def test_builders_and_tolerances_on_the_host(name):
    """The builders give sorted, in-range CSR of the intended shape, and a plain double
    evaluation (numpy products, np.add.reduceat sums, the epilogue in double) lies
    within the tolerances of the reference: a mis-derived bound would show here."""
    c = scs_case(name[4:]) if name.startswith("scs-") else vec_case(name)
    check_csr(c)
    if name.startswith("scs-"):
        _, n, J, classes, kp, _ = SCS_SHAPES[name[4:]]
        offs = np.unique(c.col - np.repeat(np.arange(c.n), c.lens))
        K = len(offs)
        assert K == 2 * J + 1 and (K + 7) // 8 * 8 == kp and 256 <= kp <= 1024
        assert c.n >= 1024 and K * c.n <= 2 * c.nnz and len(np.unique(c.val)) > 256
        assert 1 not in offs and fa().grid_from_offsets(offs, c.n) is None
        rows = {}
        for i in range(c.n):
            e = slice(c.rp[i], c.rp[i + 1])
            rows.setdefault(((c.col[e] - i).tobytes(), c.val[e].tobytes()), i)
        assert len(rows) == classes
    else:
        assert (c.lens == 0).any() and c.lens.max() > 2048
        if not c.forced:
            assert c.nnz >= 256 * c.n and set(EDGES) <= set(c.lens.tolist())
    prod = c.val * c.x[c.col]
    s = np.zeros(c.n)
    live = c.lens > 0
    s[live] = np.add.reduceat(prod, c.rp[:-1][live])
    plain = {"set": s, "add": c.y0 + s, "resid": c.b - s, "jacobi": c.x + c.d * (c.b - s)}
    for mode in MODES:
        c.check(mode, plain[mode])


def test_reference_against_exact_fractions():
    """The reference's row sums against exact rational arithmetic on a short ragged
    operator: within 2^-60 S_i (long double) or rounded once (the Fraction path)."""
    from fractions import Fraction
    rng = np.random.default_rng(7)
    n = 40
    lens = rng.integers(0, 70, n)
    lens[3] = 0
    rp = np.concatenate(([0], np.cumsum(lens)))
    col = np.concatenate([np.sort(rng.choice(200, int(k), replace=False)) for k in lens])
    val, x = rng.standard_normal(rp[-1]), rng.standard_normal(200)
    s, S = row_sums(rp, col, val, x)
    for i in range(n):
        t = [Fraction(float(val[e])) * Fraction(float(x[col[e]])) for e in range(rp[i], rp[i + 1])]
        exact, mag = sum(t, Fraction(0)), sum((abs(q) for q in t), Fraction(0))
        hi = float(s[i])
        lo = float(s[i] - LD(hi))  # a long double is the exact sum of two doubles
        err = abs(Fraction(hi) + Fraction(lo) - exact)
        assert err <= mag * Fraction(1, 2 ** (60 if LD_OK else 53)), (i, float(err))
        assert abs(Fraction(float(S[i])) - mag) <= mag * Fraction(1, 2 ** 50)
