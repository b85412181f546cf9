"""The frozen-pattern kernels of the numeric re-setup (refresh.hip) at their edges:
amg_spgemm_refill bitwise against amg_spgemm's values on the same pattern, and the
transpose refill against amg_transpose.

The launch picks the lanes per A entry from B's longest row (<= 4: four lanes, 16
entries of A in flight; <= 16: sixteen lanes; else the whole wave strides over B's
row) and the LDS staging from C's longest row (256, 1024 or 4096 columns; a longer
row is searched in global memory).  Every case says which of these it sits in and
checks that in numpy before the GPU is called.  Each C row of a case is a union of
B rows plus further B rows inside that union, so most C entries accumulate several
products and the order of accumulation shows in the bits (values over sixteen
decades).
"""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

STAGE_CAP = 4096  # REFILL_LDS_CAP of refresh.hip
SMALL = [0, 1, 32, 33, 64, 65, 128, 129, 256]
MID = [257, 512, 513, 1024]
BIG = [1025, 2048, 2049, 4096]


def fa():
    import faer_amg_amd
    return faer_amg_amd


def values(rng, n):
    """Normals over sixteen decades: the order of accumulation shows."""
    return rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)


def bits(v):
    return np.asarray(v, np.float64).view(np.int64)


def operands(widths, lengths, seed, ncols=6000):
    """A (one row per entry of lengths, plus an empty row and a row that picks only an
    empty row of B) and B (rows of at most max(widths) entries, one of exactly every
    width, row 0 empty) such that row i of A B has lengths[i] distinct columns."""
    rng = np.random.default_rng(seed)
    w = max(widths)
    brows = [np.zeros(0, np.int64)]  # row 0 of B: empty, picked by every row of A
    arows = []
    for L in lengths:
        cols = np.sort(rng.choice(ncols, L, replace=False))
        picked = [0]
        for c0 in range(0, L, w):  # the union: chunks of w columns
            picked.append(len(brows))
            brows.append(cols[c0:c0 + w])
        for _ in range(min(40, 2 * L)):  # and rows inside it: longer accumulation chains
            picked.append(len(brows))
            brows.append(np.sort(rng.choice(cols, min(L, int(rng.choice(widths))), replace=False)))
        arows.append(np.array(picked, np.int64))
    arows.append(np.zeros(0, np.int64))     # an empty row of A
    arows.append(np.array([0], np.int64))   # a row of A whose product is empty
    for wd in widths:                       # a B row of exactly every width
        brows.append(np.sort(rng.choice(ncols, wd, replace=False)))
    arows.append(np.arange(len(brows) - len(widths), len(brows), dtype=np.int64))

    def csr(rows, nc):
        rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        ci = np.concatenate(rows + [np.zeros(0, np.int64)])
        return sp.csr_matrix((values(rng, len(ci)), ci, rp), shape=(len(rows), nc))

    B = csr(brows, ncols)
    A = csr(arows, B.shape[0])
    return A, B


def lanes_per_entry(B):
    m = int(np.diff(B.indptr).max(initial=0))
    return 4 if m <= 4 else 16 if m <= 16 else 64


def stage_table(Cp):
    m = int(np.diff(Cp.indptr).max(initial=0))
    return 256 if m <= 256 else 1024 if m <= 1024 else STAGE_CAP


def garbage(pattern):
    """The pattern with values the refill must overwrite everywhere."""
    G = sp.csr_matrix((np.full(pattern.nnz, np.nan), pattern.indices.copy(), pattern.indptr.copy()),
                      shape=pattern.shape)
    return G


def check_refill(ctx, A, B, expect_lengths=None):
    F = fa()
    Ag, Bg = F.SparseMatOp.from_scipy(ctx, A), F.SparseMatOp.from_scipy(ctx, B)
    ref = F.spgemm(Ag, Bg)
    rp, ci, va = ref.arrays()
    if expect_lengths is not None:
        assert list(np.diff(rp)[:len(expect_lengths)]) == list(expect_lengths)
    Cg = F.SparseMatOp.from_scipy(ctx, garbage(sp.csr_matrix((va, ci, rp), shape=(A.shape[0], B.shape[1]))))
    F.spgemm_refill(Ag, Bg, Cg)
    r2, c2, v2 = Cg.arrays()
    assert np.array_equal(r2, rp) and np.array_equal(c2, ci)
    assert np.array_equal(bits(v2), bits(va))
    return Ag, Bg, (rp, ci, va)


CASES = [(w, ls) for w in ((1,), (1, 3), (1, 64), (3, 65)) for ls in (SMALL, MID, BIG)] + \
        [(w, SMALL) for w in ((4,), (2, 5), (16,), (9, 17))]


@pytest.mark.parametrize("widths,lengths", CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(max(v)))
def test_refill_matches_spgemm(ctx, widths, lengths):
    A, B = operands(widths, lengths, seed=sum(widths) + len(lengths))
    blen = np.diff(B.indptr)
    assert blen.min() == 0 and blen.max() == max(widths) and all(wd in blen for wd in widths)
    assert lanes_per_entry(B) == (4 if max(widths) <= 4 else 16 if max(widths) <= 16 else 64)
    assert 0 in np.diff(A.indptr)
    Ag, Bg, (rp, ci, va) = check_refill(ctx, A, B, lengths)
    assert stage_table(sp.csr_matrix((va, ci, rp), shape=(A.shape[0], B.shape[1]))) == \
        (256 if max(lengths) <= 256 else 1024 if max(lengths) <= 1024 else STAGE_CAP)
    # the result serves an SpMV: the refill rebuilt the storage of what it wrote
    F = fa()
    import torch
    Cg = F.SparseMatOp.from_scipy(ctx, garbage(sp.csr_matrix((va, ci, rp), shape=(A.shape[0], B.shape[1]))))
    F.spgemm_refill(Ag, Bg, Cg)
    x = torch.ones(B.shape[1], dtype=torch.float64, device="cuda:0")
    y = torch.empty(A.shape[0], dtype=torch.float64, device="cuda:0")
    Cg.apply(y, x)
    ctx.synchronize()
    assert np.all(np.isfinite(y.cpu().numpy()))


@pytest.mark.parametrize("widths", [(1, 3), (3, 65)], ids=["four-lanes", "whole-wave"])
def test_superset_pattern_and_rows_past_the_staging_cap(ctx, widths):
    """C's pattern a strict superset of the product: the extra entries end +0.0.  One row
    is padded to STAGE_CAP + 1 columns and one to 5000, past the LDS staging: they are
    searched and accumulated in global memory."""
    F = fa()
    lengths = [0, 1, 33, 129, 513, 4096]
    A, B = operands(widths, lengths, seed=77)
    Ag, Bg = F.SparseMatOp.from_scipy(ctx, A), F.SparseMatOp.from_scipy(ctx, B)
    rp, ci, va = F.spgemm(Ag, Bg).arrays()
    ref = sp.csr_matrix((va, ci, rp), shape=(A.shape[0], B.shape[1]))
    rng = np.random.default_rng(5)
    target = {0: 3, 2: 40, 4: STAGE_CAP + 1, 5: 5000}  # row -> padded length
    rows = []
    for i in range(ref.shape[0]):
        have = ref.indices[ref.indptr[i]:ref.indptr[i + 1]]
        if i in target:
            rest = np.setdiff1d(np.arange(ref.shape[1]), have)
            have = np.sort(np.concatenate([have, rng.choice(rest, target[i] - len(have), replace=False)]))
        rows.append(have)
    prp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    pci = np.concatenate(rows)
    sup = sp.csr_matrix((np.full(len(pci), np.nan), pci, prp), shape=ref.shape)
    assert np.diff(prp).max() == 5000 and STAGE_CAP + 1 in np.diff(prp) and sup.nnz > ref.nnz
    Cg = F.SparseMatOp.from_scipy(ctx, sup)
    F.spgemm_refill(Ag, Bg, Cg)
    r2, c2, v2 = Cg.arrays()
    assert np.array_equal(r2, prp) and np.array_equal(c2, pci)
    expect = np.zeros(len(pci))  # +0.0 where the product has no entry
    for i in range(ref.shape[0]):
        have = ref.indices[ref.indptr[i]:ref.indptr[i + 1]]
        expect[prp[i] + np.searchsorted(rows[i], have)] = ref.data[ref.indptr[i]:ref.indptr[i + 1]]
    assert np.array_equal(bits(v2), bits(expect))


@pytest.mark.parametrize("widths", [(1, 3), (3, 65)], ids=["four-lanes", "whole-wave"])
def test_missing_column_is_an_error(ctx, widths):
    """A product column absent from C: AMG_ERR_INVALID through the device flag.  The
    arrays around C's values are untouched (C's own handle keeps its pattern), and the
    same operands refill a complete pattern afterwards."""
    F = fa()
    lengths = [1, 33, 300, 1500]
    A, B = operands(widths, lengths, seed=9)
    Ag, Bg = F.SparseMatOp.from_scipy(ctx, A), F.SparseMatOp.from_scipy(ctx, B)
    rp, ci, va = F.spgemm(Ag, Bg).arrays()
    for row in (0, 2, 3):  # drop the last column of one row at a time (row 0 becomes empty)
        drop = rp[row + 1] - 1
        keep = np.ones(len(ci), bool)
        keep[drop] = False
        rp2 = rp.copy()
        rp2[row + 1:] -= 1
        Cg = F.SparseMatOp.from_scipy(ctx, sp.csr_matrix((np.full(keep.sum(), np.nan), ci[keep], rp2),
                                                         shape=(A.shape[0], B.shape[1])))
        with pytest.raises(F.AmgError) as e:
            F.spgemm_refill(Ag, Bg, Cg)
        assert e.value.status == 1 and "missing from C" in str(e.value)
        r3, c3, _ = Cg.arrays()
        assert np.array_equal(r3, rp2) and np.array_equal(c3, ci[keep])
    check_refill(ctx, A, B)
    # shapes and aliasing
    with pytest.raises(F.AmgError) as e:
        F.spgemm_refill(Ag, Bg, Ag)
    assert e.value.status == 1
    with pytest.raises(F.AmgError) as e:
        F.spgemm_refill(Ag, Bg, Bg)
    assert e.value.status == 1


def test_transpose_refill(ctx):
    """R.val[q] = P.val[perm[q]] on a P with empty columns, empty rows and one column of
    9000 entries (the transpose's own long-row edge): amg_transpose's values bit for bit,
    for the values perm was made from and for new ones."""
    F = fa()
    rng = np.random.default_rng(21)
    m, n = 9500, 700
    rows = []
    long_rows = set(rng.choice(m, 9000, replace=False).tolist())
    for i in range(m):
        if i % 97 == 5 and i not in long_rows:
            rows.append(np.zeros(0, np.int64))  # an empty row
            continue
        c = rng.choice(np.arange(20, n - 30), int(rng.integers(0, 4)), replace=False)  # columns 0..19, n-30.. stay empty
        if i in long_rows:
            c = np.append(c, 650 + 25)  # column 675: 9000 entries
        rows.append(np.unique(c))
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ci = np.concatenate(rows)
    P = sp.csr_matrix((values(rng, len(ci)), ci, rp), shape=(m, n))
    counts = np.bincount(ci, minlength=n)
    assert counts.max() == 9000 and (counts == 0).sum() >= 40 and 0 in np.diff(rp)
    Pg = F.SparseMatOp.from_scipy(ctx, P)
    Rg = F.transpose(Pg)
    rrp, rci, rva = Rg.arrays()
    perm = F.transpose_perm(Pg, Rg)
    assert perm.dtype == np.int32 and np.array_equal(np.sort(perm), np.arange(P.nnz))
    assert np.array_equal(bits(P.data[perm]), bits(rva))
    # new values on the same pattern
    P2 = sp.csr_matrix((values(rng, P.nnz), P.indices, P.indptr), shape=P.shape)
    P2g = F.SparseMatOp.from_scipy(ctx, P2)
    R2g = F.SparseMatOp.from_scipy(ctx, sp.csr_matrix((np.full(len(rci), np.nan), rci, rrp), shape=(n, m)))
    F.transpose_refill(P2g, R2g, perm)
    ref = F.transpose(P2g).arrays()
    got = R2g.arrays()
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert np.array_equal(bits(got[2]), bits(ref[2]))
    # a permutation entry outside P, and an R that is not P's transpose
    bad = perm.copy()
    bad[3] = P.nnz
    with pytest.raises(F.AmgError) as e:
        F.transpose_refill(P2g, R2g, bad)
    assert e.value.status == 1
    other = P.T.tocsr().copy()
    other.sort_indices()
    row = other.indices[other.indptr[675]:other.indptr[676]]
    row[-1] = np.setdiff1d(np.arange(m), row).max()  # an entry P does not have in column 675
    with pytest.raises(F.AmgError) as e:
        F.transpose_perm(Pg, F.SparseMatOp.from_arrays(ctx, n, m, other.indptr, other.indices, other.data))
    assert e.value.status == 1
