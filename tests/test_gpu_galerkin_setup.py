"""The Galerkin setup kernels (spgemm.hip, the scan of blas1.hip) at their table,
sort and scan edges.

Every case is compared twice:
  1. bitwise against the oracle: rowptr and col equal, val.view(int64) equal
     (signed zeros count; explicit zeros from cancellation stay in the pattern);
  2. where the operands fit densely, against the product in np.longdouble:
       |C - C_ld| <= (K + 1) 2^-53 (|A| |B|) + K 2^-1075   elementwise,
     K the longest row of A.  The first term is the rounding of K fma steps;
     the second is the absolute error of K roundings in the subnormal range
     (the standard model with underflow), below 1e-320 and needed only by the
     products that underflow on purpose.
SpMV of a result: |y - y_ld|_i <= 2 nnz_i 2^-53 sum_j |t_ij x_j|, y_ld the row
sums in np.longdouble.

The selectors of spgemm() are restated here (sym_table, num_table) only to say
where a case sits: every case asserts its product bound and its true maximum of
distinct columns, computed in numpy, before the GPU is called.  hash_slot
restates the hash only to construct colliding inputs.
"""
import time

import numpy as np
import pytest
import scipy.sparse as sp

import oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
ETA = LD(2) ** -1075  # zero in fp64


def fa():
    import faer_amg_amd
    return faer_amg_amd


# ------------------------------------------------------------------ helpers

def values(rng, n):
    """Normals over sixteen decades: the order of accumulation shows."""
    return rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)


def from_rows(ncols, rows):
    """CSR from a list of (sorted columns, values) per row, stored as given
    (explicit zeros and signed zeros kept)."""
    rp = np.zeros(len(rows) + 1, np.int64)
    for i, (c, _) in enumerate(rows):
        assert np.all(np.diff(c) > 0)
        rp[i + 1] = rp[i] + len(c)
    ci = np.concatenate([np.asarray(c, np.int64) for c, _ in rows] + [np.zeros(0, np.int64)])
    va = np.concatenate([np.asarray(v, np.float64) for _, v in rows] + [np.zeros(0)])
    return sp.csr_matrix((va, ci, rp), shape=(len(rows), ncols))


def gpu(ctx, S):
    return fa().SparseMatOp.from_scipy(ctx, S)


def orc(S):
    return O.Csr.from_scipy(S)


def same_bits(a, b):
    """Two (rowptr, col, val) triples are the same arrays, values by bit pattern."""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            and np.array_equal(a[2].view(np.int64), b[2].view(np.int64)))


def assert_bitwise(G, Oc):
    assert tuple(G.dims()) == tuple(Oc.dims()[:2])
    g, o = G.arrays(), Oc.arrays()
    assert np.array_equal(g[0], o[0])
    assert np.array_equal(g[1], o[1])
    assert np.array_equal(g[2].view(np.int64), o[2].view(np.int64))


def product_row_counts(A, B):
    """Per row of A: the sum of the picked B rows' lengths, and the number of
    distinct columns of the product row."""
    blen = np.diff(B.indptr).astype(np.int64)
    pa = sp.csr_matrix((np.ones(A.nnz, np.int64), A.indices, A.indptr), shape=A.shape)
    pb = sp.csr_matrix((np.ones(B.nnz, np.int64), B.indices, B.indptr), shape=B.shape)
    return pa @ blen, np.diff((pa @ pb).indptr)  # positive terms only: nothing cancels


def product_bound_and_count(A, B):
    """(product bound, true maximum of distinct columns): what spgemm's two selectors see."""
    ub, cnt = product_row_counts(A, B)
    return int(ub.max(initial=0)), int(cnt.max(initial=0))


def sym_table(bound, ncols):
    b = min(bound, ncols)
    return 64 if b <= 32 else 256 if b <= 128 else 1024 if b <= 512 else 8192


def num_table(count):
    return 64 if count <= 32 else 256 if count <= 128 else 1024 if count <= 512 else 4096 if count <= 2048 else 8192


def hash_slot(j, tbl):
    return (np.asarray(j).astype(np.uint32) * np.uint32(2654435761)) & np.uint32(tbl - 1)


def assert_dense_product(A, B, carr, rows=None):
    """Comparison 2: rows `rows` (default all) of C against the long-double
    product of the dense operands.  Only the columns some entry of B holds are
    laid out densely; C may have no entry elsewhere."""
    assert np.finfo(LD).eps <= 2.0 ** -63  # a reference with bits to spare
    rows = np.arange(A.shape[0]) if rows is None else np.asarray(rows)
    used = np.unique(B.indices)
    assert len(rows) <= 64 and len(used) <= 16384
    K = int(np.diff(A.indptr).max(initial=0))
    Bd = np.zeros((B.shape[0], len(used)), LD)
    Bd[np.repeat(np.arange(B.shape[0]), np.diff(B.indptr)), np.searchsorted(used, B.indices)] = B.data
    Ba = np.abs(Bd)
    rp, ci, va = carr
    for i in rows:
        ref = np.zeros(len(used), LD)
        mag = np.zeros(len(used), LD)
        for e in range(A.indptr[i], A.indptr[i + 1]):
            ref += LD(A.data[e]) * Bd[A.indices[e]]
            mag += abs(LD(A.data[e])) * Ba[A.indices[e]]
        got = np.zeros(len(used), LD)
        cols = ci[rp[i]:rp[i + 1]]
        pos = np.searchsorted(used, cols)
        assert np.all(pos < len(used)) and np.array_equal(used[pos], cols)
        got[pos] = va[rp[i]:rp[i + 1]]
        assert np.all(np.abs(got - ref) <= (K + 1) * U * mag + K * ETA), i


def assert_apply(op, r, c, v, rng):
    """op.apply(x) against the long-double row sums of the COO triple (r, c, v)."""
    m, n = op.dims()
    x = rng.standard_normal(n)
    y = np.full(m, np.nan)
    op.apply(y, x)
    t = v.astype(LD) * x[c].astype(LD)
    ref = np.zeros(m, LD)
    mag = np.zeros(m, LD)
    np.add.at(ref, r, t)
    np.add.at(mag, r, np.abs(t))
    nnz_i = np.bincount(r, minlength=m)
    assert np.all(np.abs(y - ref) <= 2 * nnz_i * U * mag)
    assert np.all(y[nnz_i == 0] == 0)


def assert_apply_arrays(op, rng):
    """The SpMV storage built by csr_finalize matches the arrays the operator downloads."""
    rp, ci, va = op.arrays()
    assert_apply(op, np.repeat(np.arange(len(rp) - 1), np.diff(rp)), ci, va, rng)


def check_product(ctx, A, B, rng, expect, dense_rows=None, dense=True, apply=True):
    """expect = (product bound, max distinct columns, symbolic table, numeric
    table), asserted from the inputs before the GPU runs."""
    ub, cnt = product_bound_and_count(A, B)
    assert (ub, cnt, sym_table(ub, B.shape[1]), num_table(cnt)) == tuple(expect)
    GA, GB = gpu(ctx, A), gpu(ctx, B)
    a0, b0 = GA.arrays(), GB.arrays()
    C = fa().spgemm(GA, GB)
    assert_bitwise(C, O.spgemm(orc(A), orc(B)))
    assert same_bits(GA.arrays(), a0) and same_bits(GB.arrays(), b0)
    if dense:
        assert_dense_product(A, B, C.arrays(), dense_rows)
    if apply:
        assert_apply_arrays(C, rng)
    return C


def stacked_operands(rng, lens, ncols, cols=None):
    """B: len(lens) rows; row r holds the first lens[r] of one set of sorted
    random columns (so the union is the longest row).  A: three rows, the
    middle one empty, the others picking every row of B."""
    d = len(lens)
    if cols is None:
        cols = np.sort(rng.choice(ncols, size=max(lens), replace=False))
    B = from_rows(ncols, [(np.sort(cols[:n]), values(rng, n)) for n in lens])
    pick = np.arange(d)
    A = from_rows(d, [(pick, values(rng, d)), (pick[:0], np.zeros(0)), (pick, values(rng, d))])
    return A, B


# ------------------------------------------------------------- SpGEMM tables

@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("c", [32, 33, 128, 129, 512, 513, 2048, 2049, 4096])
def test_spgemm_table_cutoffs(ctx, c, d):
    """d rows of B with the same c columns out of 3c: the product has c distinct
    columns (numeric cut-offs 32 | 128 | 512 | 2048, and 4096, the last count
    accepted) and the bound is d c: with d = 1 the symbolic selector sits on the
    same cut-offs (32 | 128 | 512), with d = 2 it sees twice the count and the
    two selectors disagree."""
    rng = np.random.default_rng(1000 * d + c)
    A, B = stacked_operands(rng, [c] * d, 3 * c)
    sym = {1: {32: 64, 33: 256, 128: 256, 129: 1024, 512: 1024},
           2: {32: 256, 33: 256, 128: 1024, 129: 1024}}[d].get(c, 8192)
    num = {32: 64, 33: 256, 128: 256, 129: 1024, 512: 1024, 513: 4096, 2048: 4096}.get(c, 8192)
    check_product(ctx, A, B, rng, (d * c, c, sym, num))


@pytest.mark.parametrize("bound,sym", [(32, 64), (33, 256), (128, 256), (129, 1024), (512, 1024), (513, 8192)])
def test_spgemm_symbolic_cutoffs_unequal_rows(ctx, bound, sym):
    """The symbolic cut-offs with two rows of B of ceil(bound/2) and
    floor(bound/2) columns, the shorter within the longer: the bound is `bound`
    (odd ones included) and the count ceil(bound/2), which past bound 32 lies in
    a smaller numeric table."""
    rng = np.random.default_rng(bound)
    hi, lo = (bound + 1) // 2, bound // 2
    A, B = stacked_operands(rng, [hi, lo], 3 * bound)
    num = {16: 64, 17: 64, 64: 256, 65: 256, 256: 1024, 257: 1024}[hi]
    check_product(ctx, A, B, rng, (bound, hi, sym, num))


@pytest.mark.parametrize("ncols,nb,per,sym,num", [(32, 8, 20, 64, 64), (33, 8, 20, 256, 256), (128, 9, 100, 256, 256)])
def test_spgemm_symbolic_table_clamped_by_ncols(ctx, ncols, nb, per, sym, num):
    """A large product bound (nb rows of `per` columns each) over a B of few
    columns: min(bound, B.ncols) picks the small symbolic table, and every
    column of B appears in the product row (load factor 1/2 at ncols 32)."""
    rng = np.random.default_rng(ncols)
    while True:
        rows = [np.sort(rng.choice(ncols, size=per, replace=False)) for _ in range(nb)]
        if len(np.unique(np.concatenate(rows))) == ncols:
            break
    B = from_rows(ncols, [(c, values(rng, per)) for c in rows])
    pick = np.arange(nb)
    A = from_rows(nb, [(pick, values(rng, nb)), (pick[:0], np.zeros(0)), (pick[::2], values(rng, len(pick[::2])))])
    assert sym_table(nb * per, 2 ** 31) > sym  # what the bound alone would pick
    check_product(ctx, A, B, rng, (nb * per, ncols, sym, num))


@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("tbl", [64, 256, 1024, 4096, 8192])
def test_spgemm_colliding_keys(ctx, tbl, d):
    """Rows that fill the numeric TBL table to its limit of TBL/2 keys with
    colliding ones.  B rows 0 and 1: the TBL/2 multiples of TBL, every one in
    slot 0 (probe chains up to TBL/2 long).  B rows 2 and 3: TBL/2 columns from
    the last 16 slots, so the chain runs over the end of the table and wraps to
    slot 0.  Rows of A pick d of the two rows of a kind: with d = 1 the bound is
    TBL/2 and the symbolic pass probes the same table (64, 256, 1024, 8192)
    with the same keys; with d = 2 each entry sums two products."""
    rng = np.random.default_rng(tbl + d)
    half = tbl // 2
    zero = np.arange(half, dtype=np.int64) * tbl
    assert np.all(hash_slot(zero, tbl) == 0)
    cand = np.arange(tbl * tbl // 16 + 64 * tbl, dtype=np.int64)
    last = cand[hash_slot(cand, tbl) >= tbl - 16][:half]
    assert len(last) == half and np.all(hash_slot(last, tbl) >= tbl - 16)
    ncols = int(max(zero[-1], last[-1])) + 1
    B = from_rows(ncols, [(zero, values(rng, half)), (zero, values(rng, half)),
                          (last, values(rng, half)), (last, values(rng, half))])
    pick = lambda a: (np.arange(a, a + d), values(rng, d))  # noqa: E731
    A = from_rows(4, [pick(0), (np.zeros(0, np.int64), np.zeros(0)), pick(2),
                      (np.array([1]), values(rng, 1)), (np.array([3]), values(rng, 1))])
    sym = {1: {64: 64, 256: 256, 1024: 1024}, 2: {64: 256, 256: 1024}}[d].get(tbl, 8192)
    small = tbl < 8192  # TBL 8192: 33 M columns; the dense and SpMV checks left out
    check_product(ctx, A, B, rng, (d * half, half, sym, tbl), dense=small, apply=small)


def test_spgemm_cancellation_and_signed_zeros(ctx):
    """Pairs that cancel exactly leave explicit +0.0 entries in the pattern;
    products that underflow (-1e-200 * 1e-200) leave -0.0, and the bits of both
    zeros are compared."""
    rng = np.random.default_rng(7)
    n, c = 120, 40
    cols = np.sort(rng.choice(n, size=c, replace=False))
    v = values(rng, c)
    tiny = 1e-200 * np.where(rng.random(c) < 0.5, 1.0, -1.0)
    tiny[:2] = (1e-200, -1e-200)
    B = from_rows(n, [(cols, v), (cols, v), (cols, tiny)])
    A = from_rows(3, [(np.array([0, 1]), np.array([1.0, -1.0])),
                      (np.array([2]), np.array([-1e-200])),
                      (np.zeros(0, np.int64), np.zeros(0)),
                      (np.array([0, 1, 2]), np.array([2.0, -2.0, -1e-200])),
                      (np.array([0, 2]), np.array([1.0, 1e-200]))])
    C = check_product(ctx, A, B, rng, (3 * c, c, 256, 256))
    rp, ci, va = C.arrays()
    assert np.array_equal(np.diff(rp), [c, c, 0, c, c])  # every structural entry kept
    bits = va.view(np.int64)
    assert np.all(bits[:c] == 0)  # x - x = +0.0
    neg0 = np.int64(-2 ** 63)
    assert np.array_equal(bits[c:2 * c] == neg0, tiny > 0) and np.all((bits[c:2 * c] == 0) == (tiny < 0))
    assert np.array_equal(bits[2 * c:3 * c] == neg0, tiny > 0)  # fma(-1e-200, tiny, +0.0)
    assert np.array_equal(va[3 * c:], v)  # 1e-400 vanishes beside v


def test_spgemm_mixed_rows_under_grid_stride(ctx):
    """5000 rows of A over 4096 workgroups: one product row of 2049 columns puts
    every row into the 8192 numeric table, among rows of 1 to 8 columns, empty
    rows of A and rows of A that pick only empty rows of B."""
    rng = np.random.default_rng(11)
    nb, ncols, m = 200, 6200, 5000
    brows = [(np.sort(rng.choice(ncols, size=2049, replace=False)), values(rng, 2049))]
    for r in range(1, nb):
        k = 0 if r % 5 == 0 else int(rng.integers(1, 5))
        brows.append((np.sort(rng.choice(ncols, size=k, replace=False)), values(rng, k)))
    B = from_rows(ncols, brows)
    empty_b = np.arange(5, nb, 5)
    short_b = np.setdiff1d(np.arange(1, nb), empty_b)
    arows = []
    for i in range(m):
        if i == 4500:
            pick = np.array([0])
        elif i % 7 == 3:
            pick = np.zeros(0, np.int64)
        elif i % 7 == 5:
            pick = np.sort(rng.choice(empty_b, size=2, replace=False))
        else:
            pick = np.sort(rng.choice(short_b, size=int(rng.integers(1, 3)), replace=False))
        arows.append((pick, values(rng, len(pick))))
    A = from_rows(nb, arows)
    cnt = product_row_counts(A, B)[1]
    assert cnt[4500] == 2049 and np.all(np.delete(cnt, 4500) <= 8) and np.sum(cnt == 0) > 1400
    sample = np.concatenate([[4500, 3, 5, 4095, 4096, 4097, 4999], rng.choice(m, size=40, replace=False)])
    check_product(ctx, A, B, rng, (2049, 2049, 8192, 8192), dense_rows=np.unique(sample))


@pytest.mark.parametrize("which", ["B-empty", "A-empty"])
def test_spgemm_empty_products(ctx, which):
    rng = np.random.default_rng(13)
    A = sp.random(37, 21, density=0.2, random_state=rng, format="csr")
    B = sp.random(21, 45, density=0.2, random_state=rng, format="csr")
    if which == "B-empty":
        B = sp.csr_matrix((21, 45))
    else:
        A = sp.csr_matrix((37, 21))
    C = fa().spgemm(gpu(ctx, A), gpu(ctx, B))
    assert_bitwise(C, O.spgemm(orc(A), orc(B)))
    rp, ci, va = C.arrays()
    assert C.nnz == 0 and C.dims() == (37, 45) and len(ci) == 0 and np.array_equal(rp, np.zeros(38, np.int64))
    y = np.full(37, np.nan)
    C.apply(y, rng.standard_normal(45))
    assert np.all(y == 0)


def test_spgemm_row_limit(ctx):
    """4096 distinct columns is the last count spgemm takes (test_spgemm_table_cutoffs);
    4097 is refused with AMG_ERR_UNSUPPORTED, and the context stays usable."""
    rng = np.random.default_rng(17)
    A, B = stacked_operands(rng, [4097], 3 * 4097)
    assert product_bound_and_count(A, B) == (4097, 4097)
    with pytest.raises(fa().AmgError) as ei:
        fa().spgemm(gpu(ctx, A), gpu(ctx, B))
    assert ei.value.status == 3 and "4096" in str(ei.value)
    A, B = stacked_operands(rng, [40, 40], 120)
    check_product(ctx, A, B, rng, (80, 40, 256, 256))


def test_spgemm_scan_over_two_chunks(ctx):
    """2049 rows of A: the row counts' scan runs over two blocks of 2048."""
    rng = np.random.default_rng(19)
    A = sp.random(2049, 50, density=0.06, random_state=rng, format="csr")
    B = sp.random(50, 60, density=0.1, random_state=rng, format="csr")
    A.data[:] = values(rng, A.nnz)
    B.data[:] = values(rng, B.nnz)
    C = fa().spgemm(gpu(ctx, A), gpu(ctx, B))
    assert_bitwise(C, O.spgemm(orc(A), orc(B)))
    assert_apply_arrays(C, rng)


# ----------------------------------------------------------------- transpose

def check_transpose(ctx, S, rng):
    """Bitwise the oracle's transpose; the same bits from a second call (the
    scatter is atomic, the sort hides it); transposed twice bitwise the input;
    T x within the SpMV bound of A^T x."""
    G = gpu(ctx, S)
    T = fa().transpose(G)
    assert_bitwise(T, O.transpose(orc(S)))
    assert same_bits(fa().transpose(G).arrays(), T.arrays())
    TT = fa().transpose(T)
    assert TT.dims() == G.dims() and same_bits(TT.arrays(), G.arrays())
    assert_apply(T, S.indices, np.repeat(np.arange(S.shape[0]), np.diff(S.indptr)), S.data, rng)
    return T


def columns_matrix(rng, nrows, lens):
    """nrows x len(lens) matrix whose column j has exactly lens[j] entries, at random rows."""
    r = np.concatenate([rng.choice(nrows, size=n, replace=False) for n in lens])
    c = np.repeat(np.arange(len(lens)), lens)
    S = sp.csr_matrix((values(rng, len(r)), (r, c)), shape=(nrows, len(lens)))
    S.sort_indices()
    assert np.array_equal(np.bincount(S.indices, minlength=len(lens)), lens) and S.nnz == len(r)
    return S


@pytest.mark.parametrize("nrows,longest", [(2100, 2048), (2100, 2049), (8300, 8192)])
def test_transpose_long_rows(ctx, nrows, longest):
    """The longest transposed row at the caps of the two LDS sorts: 2048 (the
    2048-entry sort, full), 2049 (the first length in the 8192-entry sort) and
    8192 (that sort full, 96 KiB of LDS), beside empty, one-entry and short rows."""
    rng = np.random.default_rng(longest)
    lens = [3, longest, 0, 1, 500, 0, min(longest - 1, 2047), 2]
    assert max(lens) == longest
    check_transpose(ctx, columns_matrix(rng, nrows, lens), rng)


def test_transpose_row_longer_than_lds_sort(ctx):
    """A transposed row of 8193 entries, one more than the largest LDS sort
    holds: ranked out of place against a copy of the scattered row."""
    # Measured on an MI355X, this one transpose (8300 x 6, 10746 entries):
    # 3.37 s with the one-lane insertion sort in global memory this branch used
    # to be (this test, which transposes the matrix three more times, took
    # 10.3 s), 0.028 s with the parallel rank sort (the test: 0.09 s).
    rng = np.random.default_rng(8193)
    S = columns_matrix(rng, 8300, [3, 8193, 0, 1, 500, 2049])
    G = gpu(ctx, S)
    fa().transpose(gpu(ctx, S[:64]))  # kernels loaded before the clock starts
    ctx.synchronize()
    t0 = time.perf_counter()
    fa().transpose(G)
    ctx.synchronize()
    print(f"transpose with an 8193-entry row: {time.perf_counter() - t0:.4f} s")
    check_transpose(ctx, S, rng)


@pytest.mark.parametrize("ncols", [2048, 2049, 524288, 524289])
def test_transpose_scan_edges(ctx, ncols):
    """The scan of the column counts at one block of 2048 | two, and at 256
    block sums (one pass of the top-level scan) | 257 (it loops, with a carry);
    the last column always holds an entry."""
    rng = np.random.default_rng(ncols)
    rows = []
    for _ in range(3):
        c = rng.choice(ncols - 1, size=1666, replace=False)
        rows.append((np.sort(np.append(c, ncols - 1)), values(rng, 1667)))
    S = from_rows(ncols, rows)
    assert S.nnz == 5001 and S.indices.max() == ncols - 1
    check_transpose(ctx, S, rng)


def test_transpose_short_rows_under_grid_stride(ctx):
    """5000 transposed rows over 4096 workgroups: rows of 0, 1 and 2 entries
    (the first two skip the sort) between rows of 10 to 30."""
    rng = np.random.default_rng(23)
    lens = np.array([(0, 1, 2, int(rng.integers(10, 31)))[j % 4] for j in range(5000)])
    assert lens[4096] == 0 and lens[4097] == 1 and lens[4999] > 2
    check_transpose(ctx, columns_matrix(rng, 40, lens), rng)


# ----------------------------------- interpolation smoothing and the Galerkin product

def unstructured_spd(rng, n):
    """Graph Laplacian of a random sparse symmetric graph plus a positive
    diagonal spread over six decades."""
    G = sp.random(n, n, density=3.0 / n, random_state=rng, format="coo")
    keep = G.row != G.col
    W = sp.csr_matrix((rng.uniform(0.1, 1.0, keep.sum()) * 10.0 ** rng.integers(-2, 3, keep.sum()),
                       (G.row[keep], G.col[keep])), shape=(n, n))
    W = W + W.T
    A = (sp.diags(np.asarray(W.sum(axis=1)).ravel() + 10.0 ** rng.uniform(-3, 3, n)) - W).tocsr()
    A.sort_indices()
    return A


def test_sa_level_on_unstructured_graph(ctx):
    """One smoothed-aggregation level on a matrix that is no stencil, with
    singleton aggregates and one of 2200 nodes: tentative P, smoothed P,
    R = P^T (a row beyond the 2048-entry sort) and R A P (a wide row) bitwise
    the oracle's; P, R and A_c multiply as their downloaded arrays do, so the
    storage finalized after the in-place rewrite of P's values is current."""
    rng = np.random.default_rng(29)
    n = 6000
    A = unstructured_spd(rng, n)
    sizes = [1] * 40 + [2200]
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(1, 9)), n - sum(sizes)))
    sizes = rng.permutation(sizes)
    na = len(sizes)
    agg = rng.permutation(np.repeat(np.arange(na), sizes))
    nn = 1.0 + 0.1 * rng.standard_normal(n)
    OA, GA = orc(A), gpu(ctx, A)
    OPt, ocnn = O.sa_tentative(agg, na, nn)
    Pt, cnn = fa().sa_tentative(ctx, agg, na, nn)
    assert np.array_equal(cnn.view(np.int64), ocnn.view(np.int64))
    assert_bitwise(Pt, OPt)
    OP = O.smooth_interpolation(OA, OPt, 0.66)
    longest = np.bincount(OP.arrays()[1], minlength=na).max()
    assert 2200 <= longest <= 8192 and na < 4096
    P = fa().smooth_interpolation(GA, Pt, 0.66)
    assert_bitwise(P, OP)
    R = fa().transpose(P)
    OR = O.transpose(OP)
    assert_bitwise(R, OR)
    Ac = fa().galerkin_rap(R, GA, P)
    OAc = O.rap(OR, OA, OP)
    assert_bitwise(Ac, OAc)
    assert np.diff(OAc.arrays()[0]).max() > 512
    for op in (P, R, Ac):
        assert_apply_arrays(op, rng)


def small_level(rng, n=30):
    A = unstructured_spd(rng, n)
    agg = np.arange(n) // 3
    OPt, _ = O.sa_tentative(agg, n // 3, np.ones(n))
    return A, OPt.to_scipy()


def assert_good_call(ctx, A, Pt):
    assert_bitwise(fa().smooth_interpolation(gpu(ctx, A), gpu(ctx, Pt), 0.66),
                   O.smooth_interpolation(orc(A), orc(Pt), 0.66))


def test_setup_dimension_errors(ctx):
    rng = np.random.default_rng(31)
    A, Pt = small_level(rng)
    GA, GP = gpu(ctx, A), gpu(ctx, Pt)
    R = fa().transpose(GP)
    with pytest.raises(fa().AmgError) as ei:  # non-square A
        fa().smooth_interpolation(gpu(ctx, A[:, :29]), gpu(ctx, Pt[:29]), 0.66)
    assert ei.value.status == 2
    assert_good_call(ctx, A, Pt)
    with pytest.raises(fa().AmgError) as ei:  # R.nrows != P.ncols
        fa().galerkin_rap(gpu(ctx, Pt.T.tocsr()[:9]), GA, GP)
    assert ei.value.status == 2
    assert_bitwise(fa().galerkin_rap(R, GA, GP), O.rap(orc(Pt.T.tocsr()), orc(A), orc(Pt)))
    with pytest.raises(fa().AmgError) as ei:  # A.ncols != B.nrows
        fa().spgemm(GA, gpu(ctx, Pt[:29]))
    assert ei.value.status == 2
    assert_bitwise(fa().spgemm(GA, GP), O.spgemm(orc(A), orc(Pt)))


def test_smooth_interpolation_diagonal_threshold(ctx):
    """The smoothing needs a_ii > 1e-6: 1e-6 itself is refused, the next larger
    decimal passes and matches the oracle; a row without a diagonal entry is
    refused.  The oracle is not called on the refused inputs."""
    rng = np.random.default_rng(37)
    A, Pt = small_level(rng)
    A = A.tolil()

    def with_diag(i, d):
        M = A.copy()
        M[i, i] = d
        M = M.tocsr()
        M.sort_indices()
        return M

    with pytest.raises(fa().AmgError) as ei:
        fa().smooth_interpolation(gpu(ctx, with_diag(7, 1e-6)), gpu(ctx, Pt), 0.66)
    assert ei.value.status == 1
    ok = with_diag(7, 1.0000001e-6)
    assert ok[7, 7] > 1e-6
    assert_good_call(ctx, ok, Pt)
    M = A.tocsr().tocoo()
    keep = ~((M.row == 11) & (M.col == 11))
    nodiag = sp.csr_matrix((M.data[keep], (M.row[keep], M.col[keep])), shape=M.shape)
    assert nodiag.nnz == M.nnz - 1
    with pytest.raises(fa().AmgError) as ei:
        fa().smooth_interpolation(gpu(ctx, nodiag), gpu(ctx, Pt), 0.66)
    assert ei.value.status == 1
    assert_good_call(ctx, A.tocsr(), Pt)
