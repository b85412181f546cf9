"""The host pieces of classical coarsening (csrc/classical_host.cpp, csrc/ls_pinned.hpp;
DESIGN.md 18) against the plain-Python restatement in tests/classical_restated.py:
amg_cr_mis integer for integer; the host amg_ls_search set for set and bit for bit in
weights and errors, with amg_ls_accept; a known answer; properties checked with numpy
linalg, independent of the pinned solvers; edge rows; the C ABI.  No GPU.  The device
search: tests/test_gpu_classical.py."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import classical_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "faer-amg_amd", "libfaer_amg_amd.so")
HDR = os.path.join(ROOT, "include", "amg.h")
NEW = ("amg_classical_config_default", "amg_cr_mis", "amg_cr_split", "amg_ls_candidates", "amg_ls_search",
       "amg_ls_accept", "amg_ls_interpolation", "amg_classical_build")
OK, INVALID, DIM, UNSUPPORTED = 0, 1, 2, 3
M = 8


def fa():
    import faer_amg_amd
    return faer_amg_amd


@pytest.fixture(scope="module")
def case2():
    """7-point 8^3, C = the index-order MIS of the matrix graph, depth 2, near-null = thin
    QR of [1, x, y, z], unit weights: the restatement's result and the library's."""
    rows = R.laplace_rows(M, M, M)
    pt = R.index_order_mis(R.grid_rows(M, M, M))
    lists = R.candidates(rows, pt, 2)
    nn = R.qr_near_null(M, M, M)
    d = np.ones(4)
    want = R.search(lists, nn, d, 3)
    got = fa().ls_search(R.lists_to_scipy(lists), nn, d, 3)
    return {"pt": pt, "lists": lists, "nn": nn, "d": d, "want": want, "got": got}


# ------------------------------------------------------------------ 1. cr_mis

def _random_graph(n, seed):
    """asymmetric, weights from three values so that degrees tie often"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        nb = sorted(set(int(j) for j in rng.integers(0, n, rng.integers(0, 6)) if j != i))
        rows.append([(j, float(rng.choice([0.25, 0.5, 1.0]))) for j in nb])
    return rows


@pytest.mark.parametrize("name", ["grid6", "random_ties", "masked", "no_candidates"])
def test_cr_mis_equals_the_restatement(name):
    if name == "random_ties":
        rows = _random_graph(300, 11)
        mask = np.ones(300, bool)
    else:
        rows = R.grid_rows(6, 6, 6)
        mask = np.ones(216, bool)
        if name == "masked":
            mask[np.random.default_rng(5).choice(216, 70, replace=False)] = False
        if name == "no_candidates":
            mask[:] = False
    got = fa().cr_mis(R.to_scipy(rows), mask)
    want = R.cr_mis(rows, mask)
    assert got.tolist() == want
    if name == "no_candidates":
        assert want == []
        return
    assert mask[got].all() and len(set(want)) == len(want)
    when = {i: t for t, i in enumerate(want)}
    for i in want:  # independent: no node a chosen node lists is chosen after it (the graph may be asymmetric)
        assert not any(when.get(j, -1) > when[i] for j, _ in rows[i])
    if name == "random_ties":  # the ties are there: equal degrees among the chosen
        assert len(want) > 20


def test_cr_mis_leaves_the_mask_alone_and_clears_non_candidates_too():
    # path 0-1-2 with 1 masked out: 0 and 2 are both chosen; the mask array is not written
    rows = [[(1, 1.0)], [(0, 1.0), (2, 1.0)], [(1, 1.0)]]
    mask = np.array([1, 0, 1], np.uint8)
    assert fa().cr_mis(R.to_scipy(rows), mask).tolist() == [0, 2]
    assert mask.tolist() == [1, 0, 1]


# ------------------------------------------------------------------ 2. the host search

def test_host_search_equals_the_restatement_bitwise(case2):
    count, cols, w, err, info = case2["got"]
    R.check_against(count, cols, w, err, case2["want"], 3)
    lens = [len(l) for l in case2["lists"] if l]
    assert min(lens) >= 3 and max(lens) <= 6
    per_row = [sum(len(list(itertools.combinations(range(n), r))) for r in (1, 2, 3)) for n in lens]
    assert info == {"device_rows": 0, "host_rows": M ** 3, "longest_list": max(lens), "subsets": sum(per_row)}


def test_acceptance_equals_the_restatement(case2):
    count, _, _, err, _ = case2["got"]
    chosen = fa().ls_accept(case2["nn"], case2["d"], count, err, tau=1.2)
    want = [R.accept(found, btb, 1.2) for found, btb in case2["want"]]
    assert chosen.tolist() == want
    f = case2["pt"] != 1
    assert (chosen[~f] == 0).all()
    assert np.bincount(chosen[f], minlength=4).tolist() == [0, 4, 252, 0]


def test_acceptance_keeps_the_reference_nan_rule():
    """A slightly negative accepted error: pow gives NaN, the comparison is false and
    nothing larger is accepted (interpolation/mod.rs:496-506)."""
    nn = np.ones((1, 1))
    count = np.array([[1, 2, 3]], np.int32)
    err = np.array([[-1e-18, -1.0, -2.0]])
    assert fa().ls_accept(nn, [1.0], count, err).tolist() == [1]
    err = np.array([[0.5, 0.4, 0.01]])  # 0.4 < 0.5^1.2 = 0.435; 0.01 < 0.4^1.2
    assert fa().ls_accept(nn, [1.0], count, err).tolist() == [3]
    count = np.array([[0, 2, 0]], np.int32)  # a missing size is skipped; dr counts from the accepted size
    err = np.array([[0.0, 0.3, 0.0]])  # 0.3 < 1^2.4
    assert fa().ls_accept(nn, [1.0], count, err).tolist() == [2]


# ------------------------------------------------------------------ 3. a known answer

def test_constant_near_null_gives_one_unit_weight(case2):
    """One constant column 1.0 with weight 1.0, so every Gram entry is exactly 1: all
    singletons tie at err 0 and the first wins with weight exactly 1.0; 0 < 0^1.2 is
    false, so no pair or triple replaces it and P 1 = 1 exactly.  (With a weight whose
    products round, e.g. 0.37, a triple's error comes out as -2.2e-19 and the
    reference's rule accepts it: the rule is kept, the test pins exact inputs.)"""
    n = M ** 3
    one = np.ones((n, 1))
    count, cols, w, err, _ = fa().ls_search(R.lists_to_scipy(case2["lists"]), one, [1.0], 3)
    chosen = fa().ls_accept(one, [1.0], count, err)
    for i in range(n):
        if case2["pt"][i] == 1:
            assert chosen[i] == 0 and not count[i].any()
            continue
        assert chosen[i] == 1
        assert count[i, 0] == 1 and cols[i, 0, 0] == case2["lists"][i][0]
        assert w[i, 0, 0] == 1.0 and err[i, 0] == 0.0


# ------------------------------------------------------------------ 4. independent of the pinned solvers

def _numpy_subset(G, g, btb):
    """constrained_subset_qp with numpy linalg: (p, err) or None"""
    def valid(p):
        return (np.isfinite(p).all() and (p >= 1e-10).all() and p.sum() <= 1 + 1e-12
                and (p >= 1e-2 * p.max()).all())
    r = len(g)
    lam, V = np.linalg.eigh(G)
    keep = np.abs(lam) > r * np.finfo(float).eps * np.abs(lam).max()
    p = V[:, keep] @ ((V[:, keep].T @ g) / lam[keep])
    if not valid(p):
        K = np.ones((r + 1, r + 1))
        K[:r, :r] = G
        K[r, r] = 0.0
        try:
            p = np.linalg.solve(K, np.append(g, 1.0))[:r]
        except np.linalg.LinAlgError:
            return None
        if not valid(p):
            return None
    return p, btb + p @ G @ p - 2 * g @ p


def test_search_properties_with_numpy_linalg(case2):
    count, cols, w, err, _ = case2["got"]
    nn, d, lists, pt = case2["nn"], case2["d"], case2["lists"], case2["pt"]
    for i in range(M ** 3):
        cand = lists[i]
        if not cand:
            continue
        vf, Vc = nn[i], nn[cand]
        gram, gvec, btb = (Vc * d) @ Vc.T, (Vc * d) @ vf, (vf * d) @ vf
        for s in range(3):
            r = s + 1
            best = None
            for idx in itertools.combinations(range(len(cand)), r):
                ix = list(idx)
                res = _numpy_subset(gram[np.ix_(ix, ix)], gvec[ix], btb)
                if res is not None and (best is None or res[1] < best):
                    best = res[1]
            if count[i, s] == 0:
                continue
            p, c = w[i, s, :r], cols[i, s, :r]
            ix = [cand.index(int(j)) for j in c]  # columns are C-points inside the ball
            assert (pt[c] == 1).all() and (np.diff(c) > 0).all()
            assert abs(err[i, s] - (btb + p @ gram[np.ix_(ix, ix)] @ p - 2 * gvec[ix] @ p)) <= 1e-12 * btb
            assert (p >= 1e-10).all() and (p >= 1e-2 * p.max()).all() and p.sum() <= 1 + 1e-12
            # no feasible same-size subset of the brute force is better by more than 1e-9 btb
            assert best is None or err[i, s] <= best + 1e-9 * btb


# ------------------------------------------------------------------ 5. edge rows

def _search_rows(lists, nn, d, mi=3):
    got = fa().ls_search(R.lists_to_scipy(lists), nn, d, mi)
    R.check_against(*got[:4], R.search(lists, nn, d, mi), mi)
    return got


def test_edge_rows_short_lists_and_no_candidate():
    rng = np.random.default_rng(2)
    nn = np.asfortranarray(rng.uniform(0.5, 1.5, (6, 3)))
    lists = [[], [3], [3, 4], [], [], []]  # no candidate, L = 1, L = 2 with max_interp 3
    count, cols, w, err, _ = _search_rows(lists, nn, np.ones(3))
    assert not count[0].any() and (cols[0] == -1).all()
    assert count[1, 1] == 0 and count[1, 2] == 0 and count[2, 2] == 0
    assert fa().ls_accept(nn, np.ones(3), count, err)[0] == 0  # an empty row of P


@pytest.mark.parametrize("k", [1, 8])
def test_edge_rows_k(k):
    rng = np.random.default_rng(k)
    nn = np.asfortranarray(rng.uniform(0.5, 1.5, (12, k)))
    lists = [[6, 7, 8, 9, 10, 11] if i < 6 else [] for i in range(12)]
    _search_rows(lists, nn, np.linspace(0.5, 2.0, k))


def test_duplicate_candidate_takes_the_pseudo_inverse_path():
    rng = np.random.default_rng(4)
    nn = np.asfortranarray(rng.uniform(0.5, 1.5, (5, 3)))
    nn[3] = nn[2]  # candidates 2 and 3 are the same vector: their Gram matrix is singular
    nn[0] = 0.5 * nn[2] + 0.25 * nn[4]
    lists = [[2, 3, 4], [], [], [], []]
    count, cols, w, err, _ = _search_rows(lists, nn, np.ones(3))
    G = np.array([[nn[2] @ nn[2]] * 2] * 2)
    assert np.linalg.matrix_rank(G) == 1
    p = R.pinv_solve(G.tolist(), [float(nn[2] @ nn[0])] * 2)
    assert abs(p[0] - p[1]) <= 1e-15 and np.isfinite(p).all()  # the minimum-norm solution


def test_max_interp_five_is_unsupported_and_four_works():
    F = fa()
    nn = np.asfortranarray(np.random.default_rng(6).uniform(0.5, 1.5, (8, 2)))
    lists = [[4, 5, 6, 7]] + [[]] * 7
    with pytest.raises(F.AmgError, match="above 4") as e:
        F.ls_search(R.lists_to_scipy(lists), nn, np.ones(2), 5)
    assert e.value.status == UNSUPPORTED
    _search_rows(lists, nn, np.ones(2), mi=4)


# ------------------------------------------------------------------ 6. the C ABI

def test_classical_symbols_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(amg_[a-z0-9_]+)\s*\(", src))
    exported = set(re.findall(r" T (amg_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()))
    for name in NEW:
        assert name in declared, name
        assert name in exported, name
        assert name in fa().SIGNATURES, name
    for name in ("ClassicalConfig", "cr_mis", "cr_split", "ls_candidates", "ls_search", "ls_accept", "ls_interpolation",
                 "classical_build"):
        assert callable(getattr(fa(), name)), name


def test_classical_config_default_and_layout():
    F = fa()
    c = F.ClassicalConfig()
    assert C.sizeof(c) == 104
    assert (c.search_depth, c.depth_ls, c.max_interp, c.tau_threshold) == (1, 2, 3, 1.2)
    assert (c.target_convergence, c.relax_steps, c.smoother_coarsening_factor, c.max_cr_iters) == (0.3, 5, 256.0, 20)
    assert (c.coarsest_dim, c.max_levels, c.omega, c.smoother, c.chebyshev_steps, c.where) == (1000, 0, 0.66, 1, 0, 1)
    assert F.lib().amg_classical_config_default(None) == INVALID


def test_classical_arguments_rejected_without_a_device():
    F = fa()
    L = F.lib()
    lists = F.HostCsr(F._host_csr_from_scipy(R.lists_to_scipy([[1], []])))
    nn = np.asfortranarray(np.ones((2, 1)))
    d = np.ones(1)
    count, cols = np.full(6, -3, np.int32), np.full(18, -3, np.int64)
    w, err = np.full(18, -3.0), np.full(6, -3.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def search(lists_h=lists.h, nnp=p(nn), ld=2, k=1, mi=3, where=0, max_list=0, out=p(count)):
        return L.amg_ls_search(None, lists_h, nnp, ld, k, p(d), mi, where, max_list, out, p(cols), p(w), p(err), None)

    assert search(lists_h=None) == INVALID and b"null argument" in L.amg_last_error()
    assert search(nnp=None) == INVALID
    assert search(out=None) == INVALID
    assert search(mi=0) == INVALID and b"max_interp" in L.amg_last_error()
    assert search(mi=5) == UNSUPPORTED
    assert search(k=0) == INVALID
    assert search(ld=1) == INVALID and b"leading dimension" in L.amg_last_error()
    assert search(where=2) == INVALID and b"where" in L.amg_last_error()
    assert search(where=1) == INVALID and b"needs a context" in L.amg_last_error()
    assert search(max_list=-1) == INVALID
    bad = np.asfortranarray(np.array([[1.0], [np.inf]]))
    assert search(nnp=p(bad)) == INVALID and b"not finite" in L.amg_last_error()
    rect = F.HostCsr(F._host_csr_from_scipy(R.to_scipy([[(1, 1.0)], []], ncols=3)))
    assert search(lists_h=rect.h) == DIM
    assert (count == -3).all() and (cols == -3).all() and (w == -3).all() and (err == -3).all()
    assert search() == OK  # info4 is optional
    assert count.tolist() == [1, 0, 0, 0, 0, 0] and cols[0] == 1 and w[0] == 1.0

    g = F.HostCsr(F._host_csr_from_scipy(R.to_scipy([[(1, 1.0)], [(0, 1.0)]])))
    mask, cp, nnew = np.ones(2, np.uint8), np.zeros(2, np.int64), C.c_int64(-3)
    assert L.amg_cr_mis(None, p(mask), p(cp), C.byref(nnew)) == INVALID
    assert L.amg_cr_mis(g.h, None, p(cp), C.byref(nnew)) == INVALID
    assert L.amg_cr_mis(g.h, p(mask), None, C.byref(nnew)) == INVALID
    assert L.amg_cr_mis(g.h, p(mask), p(cp), None) == INVALID
    assert L.amg_cr_mis(rect.h, p(mask), p(cp), C.byref(nnew)) == DIM
    assert nnew.value == -3
    assert L.amg_cr_mis(g.h, p(mask), p(cp), C.byref(nnew)) == OK and nnew.value == 1 and cp[0] == 0

    ch = np.zeros(2, np.int32)
    assert L.amg_ls_accept(2, p(nn), 2, 1, p(d), 3, 1.2, None, p(err), p(ch)) == INVALID
    assert L.amg_ls_accept(2, p(nn), 1, 1, p(d), 3, 1.2, p(count), p(err), p(ch)) == INVALID
    assert L.amg_ls_candidates(None, p(mask), 2, None) == INVALID and b"null amg_linop" in L.amg_last_error()
    assert L.amg_ls_interpolation(None, p(mask), p(nn), 2, 1, p(d), None, None, None, None, None) == INVALID
    assert L.amg_cr_split(None, g.h, None, p(mask), None, C.byref(nnew), None) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    assert L.amg_classical_build(None, p(nn), 2, 1, p(d), None, None, None) == INVALID
