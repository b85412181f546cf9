"""Plain-Python restatement of the host pieces of classical coarsening:
the C-point MIS with a candidate mask, the BFS candidate lists, the least-squares
subset search with the pinned arithmetic of csrc/ls_pinned.hpp, and the acceptance
rule.  Written from the reference (partitioners/mod.rs:395-423, :695-718;
interpolation/mod.rs:312-356, :387-510) and the pins stated in ls_pinned.hpp, with
Python floats (IEEE doubles, one rounding per operation, no fused multiply-add) and
plain loops: no numpy reductions, so every sum runs in the order the library states.
Shared by tests/test_classical_host.py and tests/test_gpu_classical.py."""
import itertools
import math

import numpy as np

EPS = 2.220446049250313e-16
FEAS_TOL, MIN_ABS, MIN_REL = 1e-12, 1e-10, 1e-2
JACOBI_SWEEPS = 16


# ------------------------------------------------------------------ graphs

def grid_rows(nx, ny, nz, w=1.0):
    """7-point grid graph, rows of (neighbour, weight), ascending; x fastest."""
    rows = []
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                r = []
                for dz, dy, dx in ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (1, 0, 0)):
                    X, Y, Z = x + dx, y + dy, z + dz
                    if 0 <= X < nx and 0 <= Y < ny and 0 <= Z < nz:
                        r.append((X + nx * (Y + ny * Z), w))
                rows.append(r)
    return rows


def laplace_rows(nx, ny, nz):
    """The 7-point Laplacian (diagonal 6, off-diagonals -1), rows ascending."""
    rows = grid_rows(nx, ny, nz, -1.0)
    return [sorted(r + [(i, 6.0)]) for i, r in enumerate(rows)]


def to_scipy(rows, ncols=None):
    import scipy.sparse as sp
    n = len(rows)
    rp = np.zeros(n + 1, np.int64)
    ci, va = [], []
    for i, r in enumerate(rows):
        for j, w in r:
            ci.append(j)
            va.append(w)
        rp[i + 1] = len(ci)
    return sp.csr_matrix((np.array(va, np.float64), np.array(ci, np.int64), rp), shape=(n, ncols or n))


def index_order_mis(rows):
    """Greedy independent set in index order: point types (1 = C, 0 = F)."""
    n = len(rows)
    state = [0] * n  # 0 undecided, 1 C, 2 covered
    for i in range(n):
        if state[i] == 0:
            state[i] = 1
            for j, _ in rows[i]:
                if j != i and state[j] == 0:
                    state[j] = 2
    return np.array([1 if s == 1 else 0 for s in state], np.int8)


# ------------------------------------------------------------------ MIS with a mask

def cr_mis(rows, candidates):
    f = [bool(c) for c in candidates]
    deg = []
    for i, r in enumerate(rows):
        if not f[i]:
            continue
        s = 0.0
        for j, w in r:
            if f[j]:
                s += w
        deg.append((-s, i))
    deg.sort()
    chosen = []
    for _, i in deg:
        if f[i]:
            f[i] = False
            chosen.append(i)
            for j, _ in rows[i]:
                f[j] = False
    return chosen


# ------------------------------------------------------------------ candidate lists

def candidates(rows, point_type, depth):
    """Per non-C row the C-points within BFS depth `depth` (the centre included)."""
    out = []
    for i in range(len(rows)):
        if point_type[i] == 1:
            out.append([])
            continue
        seen = {i}
        frontier = [i]
        for _ in range(depth):
            nxt = []
            for j in frontier:
                for c, _ in rows[j]:
                    if c not in seen:
                        seen.add(c)
                        nxt.append(c)
            frontier = nxt
        out.append(sorted(j for j in seen if point_type[j] == 1))
    return out


def lists_to_scipy(lists):
    return to_scipy([[(j, 1.0) for j in r] for r in lists])


# ------------------------------------------------------------------ the pinned solvers

def finite(x):
    return (x - x) == 0.0


def gram_entry(a, b, d):
    s = 0.0
    for c in range(len(d)):
        s += (a[c] * d[c]) * b[c]
    return s


def validate(p):
    max_w = 0.0
    total = 0.0
    ok = True
    for x in p:
        if not finite(x) or x < MIN_ABS:
            ok = False
        max_w = max_w if max_w > x else x
        total += x
    if not ok:
        return False
    if total > 1.0 + FEAS_TOL:
        return False
    thr = MIN_REL * max_w
    return all(not (x < thr) for x in p)


def eval_err(G, p, g, btb):
    r = len(p)
    quad = 0.0
    lin = 0.0
    for i in range(r):
        t = 0.0
        for j in range(r):
            t += G[i][j] * p[j]
        quad += p[i] * t
    for i in range(r):
        lin += g[i] * p[i]
    return (btb + quad) - 2.0 * lin


def pinv_solve(G, g):
    r = len(g)
    A = [list(row) for row in G]
    V = [[1.0 if i == j else 0.0 for j in range(r)] for i in range(r)]
    for _ in range(JACOBI_SWEEPS):
        off2 = 0.0
        diag2 = 0.0
        for i in range(r):
            diag2 += A[i][i] * A[i][i]
            for j in range(i + 1, r):
                off2 += A[i][j] * A[i][j]
        if off2 <= 1e-32 * (2.0 * off2 + diag2):
            break
        if not finite(off2):
            break
        for p in range(r - 1):
            for q in range(p + 1, r):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                at = abs(theta) + math.sqrt(theta * theta + 1.0)
                t = -1.0 / at if theta < 0.0 else 1.0 / at
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                A[p][p] = A[p][p] - t * apq
                A[q][q] = A[q][q] + t * apq
                A[p][q] = 0.0
                A[q][p] = 0.0
                for k in range(r):
                    if k != p and k != q:
                        akp, akq = A[k][p], A[k][q]
                        A[k][p] = c * akp - s * akq
                        A[p][k] = A[k][p]
                        A[k][q] = s * akp + c * akq
                        A[q][k] = A[k][q]
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    lmax = 0.0
    for i in range(r):
        a = abs(A[i][i])
        lmax = lmax if lmax > a else a
    thr = float(r) * EPS * lmax
    z = []
    for i in range(r):
        y = 0.0
        for j in range(r):
            y += V[j][i] * g[j]
        if not finite(A[i][i]):
            z.append(math.nan)
        else:
            z.append(0.0 if abs(A[i][i]) <= thr else y / A[i][i])
    out = []
    for j in range(r):
        s = 0.0
        for i in range(r):
            s += V[j][i] * z[i]
        out.append(s)
    return out


def _div(a, b):
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def kkt_solve(G, g):
    r = len(g)
    n = r + 1
    M = [[0.0] * (n + 1) for _ in range(n)]
    for i in range(n):
        for j in range(n + 1):
            if j == n:
                M[i][j] = g[i] if i < r else 1.0
            elif i < r and j < r:
                M[i][j] = G[i][j]
            else:
                M[i][j] = 0.0 if (i == r and j == r) else 1.0
    for c in range(n):
        piv = c
        best = abs(M[c][c])
        for i in range(c + 1, n):
            if abs(M[i][c]) > best:
                best = abs(M[i][c])
                piv = i
        if piv != c:
            M[c], M[piv] = M[piv], M[c]
        for i in range(c + 1, n):
            f = _div(M[i][c], M[c][c])
            for j in range(c + 1, n + 1):
                M[i][j] = M[i][j] - f * M[c][j]
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        s = M[i][n]
        for j in range(i + 1, n):
            s = s - M[i][j] * x[j]
        x[i] = _div(s, M[i][i])
    return x[:r]


def subset_qp(G, g, btb):
    """constrained_subset_qp: (weights, err) or None."""
    p = pinv_solve(G, g)
    if not validate(p):
        p = kkt_solve(G, g)
        if not validate(p):
            return None
    return p, eval_err(G, p, g, btb)


# ------------------------------------------------------------------ the search

def search_row(i, cand, nn, d, max_interp):
    """The best subset of each size for row i: a list of max_interp entries, each
    None or (cols, weights, err)."""
    k = len(d)
    vf = [float(nn[i, c]) for c in range(k)]
    vc = [[float(nn[j, c]) for c in range(k)] for j in cand]
    L = len(cand)
    g = [gram_entry(vc[l], vf, d) for l in range(L)]
    btb = gram_entry(vf, vf, d)
    gram = {}
    out = []
    for r in range(1, max_interp + 1):
        best = None
        for idx in itertools.combinations(range(L), r):
            G = [[0.0] * r for _ in range(r)]
            for a in range(r):
                for b in range(a, r):
                    key = (idx[a], idx[b])
                    if key not in gram:
                        gram[key] = gram_entry(vc[idx[a]], vc[idx[b]], d)
                    G[a][b] = gram[key]
                    G[b][a] = gram[key]
            res = subset_qp(G, [g[t] for t in idx], btb)
            if res is not None and (best is None or res[1] < best[2]):
                best = ([cand[t] for t in idx], res[0], res[1])
        out.append(best)
    return out, btb


def search(lists, nn, d, max_interp):
    nn = np.asarray(nn, np.float64)
    if nn.ndim == 1:
        nn = nn[:, None]
    d = [float(x) for x in d]
    return [search_row(i, lists[i], nn, d, max_interp) for i in range(len(lists))]


def accept(found, btb, tau):
    """The accepted size (0: none) by ls_interp_weights' rule."""
    acc_err, acc_size = btb, 0
    for r, best in enumerate(found, start=1):
        if best is None:
            continue
        dr = float(r - acc_size)
        try:
            bound = math.pow(acc_err, tau * dr)
        except (ValueError, OverflowError):
            bound = math.nan  # a negative accepted error: NaN, nothing larger is accepted
        if best[2] < bound:
            acc_err, acc_size = best[2], r
    return acc_size


def check_against(count, cols, w, err, results, max_interp):
    """Library output (ls_search) equals the restatement's: sets exactly, weights and
    errors bit for bit."""
    for i, (found, _) in enumerate(results):
        for s, best in enumerate(found):
            if best is None:
                assert count[i, s] == 0, (i, s)
                assert (cols[i, s] == -1).all() and (w[i, s] == 0).all() and err[i, s] == 0
                continue
            r = s + 1
            assert count[i, s] == r, (i, s)
            assert cols[i, s, :r].tolist() == best[0], (i, s)
            assert (cols[i, s, r:] == -1).all()
            assert np.array(best[1]).tobytes() == w[i, s, :r].tobytes(), (i, s, best[1], w[i, s, :r])
            assert np.float64(best[2]).tobytes() == err[i, s].tobytes(), (i, s, best[2], err[i, s])


def qr_near_null(nx, ny, nz):
    """Thin QR of [1, x, y, z] on the grid (numpy), n x 4."""
    n = nx * ny * nz
    idx = np.arange(n)
    B = np.stack([np.ones(n), (idx % nx).astype(float), ((idx // nx) % ny).astype(float),
                  (idx // (nx * ny)).astype(float)], axis=1)
    Q, _ = np.linalg.qr(B)
    return np.asfortranarray(Q)
