"""The modularity partitioner restated in plain Python lists, from the rules of
DESIGN.md 17 (not from the C++): what amg_partition_modularity and
amg_partition_modularity_device must reproduce integer for integer.

A graph is a list of rows, a row a list of (column, strength) in stored order
(columns ascending, no self loops, not necessarily symmetric).  Python floats
are IEEE doubles and CPython fuses no multiply-add, so the arithmetic below is
the library's (-ffp-contract=off) bit for bit."""
import math

M64 = (1 << 64) - 1


def mix(i, j):
    """splitmix64 finaliser of (i << 32) | j"""
    z = (((i << 32) | j) + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def size_cost(s, cf, pen):
    u = 4.0 * (abs(float(s) - cf) / cf)
    return ((u * u) * (u * u)) * pen


def candidate_edges(rows, rs, size, inv_total, cf, pen):
    """keys (-w, mix, i, j): ascending key order is the edge order"""
    keys = []
    for i, row in enumerate(rows):
        for j, s in row:
            if not i > j:
                continue
            w = s - (inv_total * rs[i]) * rs[j]
            t = float(size[i] + size[j]) - cf
            if size[i] + size[j] > cf:
                w = w - pen * (t * t)
            else:
                w = w + pen * (t * t)
            keys.append((-w, mix(i, j), i, j))
    return keys


def serial_matching(keys, nv, target):
    """mate per vertex (-1: unmatched): the sorted sweep, stopped once more than
    `target` pairs are taken"""
    mate = [-1] * nv
    pairs = 0
    for _, _, i, j in sorted(keys):
        if mate[i] < 0 and mate[j] < 0:
            mate[i], mate[j] = j, i
            pairs += 1
            if pairs > target:
                break
    return mate, pairs


def pass_matching(keys, nv, target):
    """The locally dominant form: (mate, passes).  Every live vertex picks its first
    live incident edge; an edge picked at both ends is matched.  More than
    target + 1 pairs are cut back to the first target + 1 of the order."""
    at = [[] for _ in range(nv)]
    for k in keys:
        at[k[2]].append(k)
        at[k[3]].append(k)
    mate = [-1] * nv
    passes = 0
    while True:
        pick = {}
        for v in range(nv):
            if mate[v] >= 0:
                continue
            live = [k for k in at[v] if mate[k[2]] < 0 and mate[k[3]] < 0]
            if live:
                pick[v] = min(live)
        if not pick:
            break
        passes += 1
        for v, k in pick.items():
            u = k[3] if k[2] == v else k[2]
            if pick.get(u) == k:
                mate[v] = u
    matched = sorted(k for k in keys if mate[k[2]] == k[3])
    for k in matched[target + 1:]:
        mate[k[2]] = mate[k[3]] = -1
    return mate, passes


def contract(rows, rs, size, node_to_v, mate):
    nv = len(rows)
    newid = [0] * nv
    q = 0
    for v in range(nv):  # ascending smallest member
        if mate[v] < 0 or v < mate[v]:
            newid[v] = q
            q += 1
        else:
            newid[v] = newid[mate[v]]
    nrows, nrs, nsize = [], [], []
    for v in range(nv):
        if not (mate[v] < 0 or v < mate[v]):
            continue
        members = [v] if mate[v] < 0 else [v, mate[v]]
        sums, order = {}, []
        for m in members:  # ascending old id; entries in stored order
            for j, s in rows[m]:
                c = newid[j]
                if c in sums:
                    sums[c] = sums[c] + s
                else:
                    sums[c] = s
                    order.append(c)
        nrows.append([(c, sums[c]) for c in sorted(order)])
        nrs.append(rs[v] if mate[v] < 0 else rs[v] + rs[mate[v]])
        nsize.append(size[v] if mate[v] < 0 else size[v] + size[mate[v]])
    return nrows, nrs, nsize, [newid[x] for x in node_to_v]


def improvement_pass(rows, agg, size, cf, pen):
    """one pass: the swaps accepted, or None when nothing was proposed"""
    props = []
    for i, row in enumerate(rows):
        src = agg[i]
        if size[src] <= 1:
            continue
        best = None
        for dst in sorted({agg[j] for j, _ in row if agg[j] != src}):
            tin = tout = 0.0
            for j, s in row:
                if agg[j] == src:
                    tin += s
                elif agg[j] == dst:
                    tout += s
            dq = (tout - tin) + pen * ((size_cost(size[dst], cf, pen) + size_cost(size[src], cf, pen))
                                       - (size_cost(size[dst] + 1, cf, pen) + size_cost(size[src] - 1, cf, pen)))
            if dq > 0.0 and (best is None or dq > best[0]):  # ascending dst: ties keep the smaller id
                best = (dq, dst)
        if best is not None:
            props.append((-best[0], i, best[1]))
    if not props:
        return None
    props.sort()
    alive_nodes = [True] * len(rows)
    alive_aggs = [True] * len(size)
    swaps = 0
    for _, v, to in props:
        frm = agg[v]
        if alive_nodes[v] and alive_aggs[to] and alive_aggs[frm]:
            agg[v] = to
            size[frm] -= 1
            size[to] += 1
            swaps += 1
            alive_aggs[to] = alive_aggs[frm] = False
            alive_nodes[v] = False
            for j, _ in rows[v]:
                alive_nodes[j] = False
                alive_aggs[agg[j]] = False
    return swaps


def partition(rows, cf=8.0, pen=1.0, max_improvement_iters=100, check_passes=False):
    """dict: agg_of, naggs, rounds, improvement_passes, swaps, stalled (a round found no
    pair), pass_counts (per round, with check_passes: the pass form, checked against the
    serial sweep)"""
    n = len(rows)
    base_rs = []
    for row in rows:
        s = 0.0
        for _, w in row:
            s += w
        base_rs.append(0.0 if s < 0.0 else s)
    total = 0.0
    for s in base_rs:
        total += s
    inv_total = 1.0 / total
    cur, rs, size, node_to_v = [list(r) for r in rows], list(base_rs), [1] * n, list(range(n))
    rounds, stalled, pass_counts = 0, False, []
    while n / len(cur) < cf:
        nv = len(cur)
        keys = candidate_edges(cur, rs, size, inv_total, cf, pen)
        if not keys:
            stalled = True
            break
        target = math.ceil(nv - n / cf) + 1
        mate, _ = serial_matching(keys, nv, target)
        if check_passes:
            mate2, passes = pass_matching(keys, nv, target)
            assert mate2 == mate
            pass_counts.append(passes)
        cur, rs, size, node_to_v = contract(cur, rs, size, node_to_v, mate)
        rounds += 1
    agg = node_to_v
    improvement_passes = swaps = 0
    for _ in range(max_improvement_iters):
        got = improvement_pass(rows, agg, size, cf, pen)
        if got is None:
            break
        improvement_passes += 1
        swaps += got
    ren = {}
    for a in agg:  # numbered by smallest node
        if a not in ren:
            ren[a] = len(ren)
    return {"agg_of": [ren[a] for a in agg], "naggs": len(ren), "rounds": rounds,
            "improvement_passes": improvement_passes, "swaps": swaps, "stalled": stalled,
            "pass_counts": pass_counts}


# ---- the graphs the tests share

def grid_rows(nx, ny, nz, lower_only=False):
    """7-point grid, unit strengths; lower_only keeps the neighbours j < i"""
    rows = []
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                i = x + nx * (y + ny * z)
                nb = []
                if z > 0:
                    nb.append(i - nx * ny)
                if y > 0:
                    nb.append(i - nx)
                if x > 0:
                    nb.append(i - 1)
                if not lower_only:
                    if x + 1 < nx:
                        nb.append(i + 1)
                    if y + 1 < ny:
                        nb.append(i + nx)
                    if z + 1 < nz:
                        nb.append(i + nx * ny)
                rows.append([(j, 1.0) for j in nb])
    return rows


def random_rows(n, seed, degree=5):
    """asymmetric, strengths drawn from four values: tie-heavy"""
    import random
    rng = random.Random(seed)
    rows = []
    for i in range(n):
        nb = set()
        while len(nb) < degree:
            j = rng.randrange(n)
            if j != i:
                nb.add(j)
        rows.append([(j, rng.choice((0.25, 0.5, 0.75, 1.0))) for j in sorted(nb)])
    return rows


def path_rows(n):
    return [[(j, 1.0) for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)]


def isolated_rows():
    """a path of 10 (nodes 3..12) among isolated nodes"""
    rows = [[] for _ in range(16)]
    for i in range(3, 13):
        rows[i] = [(j, 1.0) for j in (i - 1, i + 1) if 3 <= j <= 12]
    return rows


def hub_rows(n=400, spokes=300):
    """node 0 lists `spokes` neighbours (a row past the one-lane proposal limit); the
    rest form a ring with a link back to the hub"""
    rows = [[(j, 0.5 + 0.25 * (j % 3)) for j in range(1, spokes + 1)]]
    for i in range(1, n):
        nb = sorted({0, 1 + (i - 2) % (n - 1), 1 + i % (n - 1)} - {i})
        rows.append([(j, 1.0 if j else 0.5) for j in nb])
    return rows


def to_scipy(rows):
    import numpy as np
    import scipy.sparse as sp
    indptr = np.zeros(len(rows) + 1, np.int64)
    for i, r in enumerate(rows):
        indptr[i + 1] = indptr[i] + len(r)
    indices = np.array([j for r in rows for j, _ in r], np.int64)
    data = np.array([s for r in rows for _, s in r], np.float64)
    return sp.csr_matrix((data, indices, indptr), shape=(len(rows), len(rows)))


CASES = {
    "grid12_sym": (lambda: grid_rows(12, 12, 12), dict()),
    "grid12_lower": (lambda: grid_rows(12, 12, 12, lower_only=True), dict()),
    "random600": (lambda: random_rows(600, 7), dict()),
    "path64": (lambda: path_rows(64), dict()),
    "isolated": (isolated_rows, dict()),
    "two_nodes": (lambda: [[(1, 1.0)], [(0, 1.0)]], dict()),
    "grid12_cf2": (lambda: grid_rows(12, 12, 12), dict(coarsening_factor=2.0)),
    "grid12_cf2p5": (lambda: grid_rows(12, 12, 12), dict(coarsening_factor=2.5)),
    "grid16_cf128": (lambda: grid_rows(16, 16, 16), dict(coarsening_factor=128.0)),
    "grid12_pen0": (lambda: grid_rows(12, 12, 12), dict(agg_size_penalty=0.0)),
}
_cache = {}


def case(name):
    """(rows, cfg, restated result), computed once"""
    if name not in _cache:
        make, cfg = CASES[name]
        rows = make()
        _cache[name] = (rows, cfg, partition(rows, cf=cfg.get("coarsening_factor", 8.0),
                                             pen=cfg.get("agg_size_penalty", 1.0)))
    return _cache[name]
