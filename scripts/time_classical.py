#!/usr/bin/env python3
"""Classical coarsening on the 7-point m^3 Laplacian: the least-squares
search on the device against the host function, amg_classical_build's stage times, and
amg_sa_build on the same matrix and near-null beside it.

Near-null: the thin QR of [1, x, y, z]; weights: create_weights.  The C/F split is
amg_cr_split on the depth-1 strength graph at the defaults.

search: the candidate lists at every depth of --depths (3 and the reference's 5); per
depth the rows searched are every --stride-th non-C row (stride 1: all of them; the
stride is reported); host (OpenMP, the threads of OMP_NUM_THREADS) and device alternate
in one process, host first, `reps` (3) runs each; per run torch.cuda.synchronize(), the
call, host perf_counter around it (amg_ls_search returns after its own synchronise).
The device time includes the uploads, the binning sort and the downloads.  Reported:
every run's seconds, the median, min and max, the subsets enumerated and subsets per
second, and that the two outputs are the same bytes.  --level-stages also times the
level-0 stages of amg_classical_build one by one (strength graph, CR split,
amg_ls_interpolation with depth 3 and the search where --where says, the RAP): the
Galerkin operators fill in, so the deeper levels of a large grid have candidate lists
of hundreds of C-points and a whole hierarchy is built at small sizes only.

build: amg_classical_build with the search where --where says, `reps` builds, the
FAMG_SA_LOG=1 line of every level (graph, cr, candidates, search, assemble, rap,
nearnull; CR rounds), levels, rows per level, operator complexity (sum of nnz over the
levels / the fine nnz) and the PCG iterations to rel_tol 1e-8 for one standard-normal
right-hand side; amg_sa_build (defaults: depth-1 strength, MIS aggregates, --sa-cd
candidates kept per aggregate, default 1 as amg_sa_config_default) with the same
smoother (L1) and coarsest_dim beside it.

The measurement runs in a fresh child process under its own `timeout` (the parent never
touches the GPU), and nothing is retried:

  python scripts/time_classical.py [--m 64] [--depths 3,5] [--strides 1,64] [--where 1]
                                   [--sa-cd 1] [--level-stages] [--coarsest-dim 1000] [--max-levels 0] [--skip-search] [--skip-build] [--limit 900] [--out FILE]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "faer-amg_amd"))


def log(msg):
    print(f"[time_classical] {msg}", file=sys.stderr, flush=True)


def near_null(m):
    n = m ** 3
    idx = np.arange(n)
    B = np.stack([np.ones(n), (idx % m).astype(float), ((idx // m) % m).astype(float),
                  (idx // (m * m)).astype(float)], axis=1)
    Q, _ = np.linalg.qr(B)
    return np.asfortranarray(Q)


def parse_log(text, tag):
    levels = []
    for line in text.splitlines():
        m = re.match(r"famg %s level (\d+): (.*) ms: (.*)$" % tag, line)
        if not m:
            continue
        d = {"level": int(m.group(1)), "counts": m.group(2)}
        toks = m.group(3).split()
        d["ms"] = {toks[i]: float(toks[i + 1]) for i in range(0, len(toks), 2)}
        levels.append(d)
    return levels


def captured(fn):
    """fn() with the library's stderr lines captured: (result, seconds, text)"""
    import torch
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tf:
        os.dup2(tf.fileno(), 2)
        try:
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            t = time.perf_counter() - t
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tf.seek(0)
        return out, t, tf.read().decode()


def stats(ts):
    return {"all_s": ts, "median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts))}


def child(args):
    os.environ["FAMG_SA_LOG"] = "1"
    import scipy.sparse as sp
    import torch
    import faer_amg_amd as fa
    if not torch.cuda.is_available():
        sys.exit("time_classical.py needs a GPU")
    ctx = fa.Context(0)
    m = args.m
    A = fa.SparseMatOp.laplace3d_7pt(ctx, m, m, m)
    n = A.nrows
    nn = near_null(m)
    w = np.asarray(fa.create_weights(A, nn), np.float64)
    res = {"device": torch.cuda.get_device_name(0), "m": m, "rows": n, "nnz": A.nnz,
           "omp_threads": os.environ.get("OMP_NUM_THREADS"), "reps": args.reps}
    if not args.skip_search:
        t = time.perf_counter()
        G = fa.strength_graph(A, nn, w, depth=1)
        t_graph = time.perf_counter() - t
        t = time.perf_counter()
        pt, nc, info = fa.cr_split(A, G)
        t_cr = time.perf_counter() - t
        log(f"split: {nc} C-points of {n}, {info['rounds']} rounds, reduction {info['reduction']:.4f} "
            f"({info['stop']}), graph {t_graph:.2f} s, CR {t_cr:.2f} s")
        res["split"] = {"c_points": nc, "rounds": info["rounds"], "reduction": info["reduction"], "stop": info["stop"],
                        "c_per_round": info["c_per_round"], "strength_graph_s": t_graph, "cr_split_s": t_cr}
        if args.level_stages:  # the level-0 stages of amg_classical_build, one by one
            torch.cuda.synchronize()
            t = time.perf_counter()
            P, _, _ = fa.ls_interpolation(A, pt, nn, w, where=args.where)
            torch.cuda.synchronize()
            t_interp = time.perf_counter() - t
            t = time.perf_counter()
            Ac = fa.galerkin_rap(fa.transpose(P), A, P)
            torch.cuda.synchronize()
            t_rap = time.perf_counter() - t
            res["level0"] = {"ls_interpolation_s": t_interp, "where": args.where, "rap_s": t_rap,
                             "coarse_rows": Ac.nrows, "coarse_nnz": Ac.nnz, "p_nnz": P.nnz}
            log(f"level 0: interpolation {t_interp:.2f} s, RAP {t_rap:.2f} s, A_c {Ac.nrows} rows {Ac.nnz} nnz")
            del P, Ac
        res["search"] = []
        for depth, stride in zip(args.depths, args.strides):
            t = time.perf_counter()
            lists = fa.ls_candidates(A, pt, depth).tocsr()
            t_lists = time.perf_counter() - t
            lens = np.diff(lists.indptr)
            rows = np.flatnonzero(lens > 0)[::stride]
            keep = np.zeros(n, bool)
            keep[rows] = True
            sub = sp.diags(keep.astype(float)).tocsr() @ lists
            sub.eliminate_zeros()
            sub = sub.tocsr()
            runs = {0: [], 1: []}
            outs = {}
            for r in range(args.reps):
                for where in (0, 1):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    out = fa.ls_search(sub, nn, w, 3, where=where, ctx=ctx)
                    runs[where].append(time.perf_counter() - t)
                    outs[where] = out
                    log(f"depth {depth} run {r} {'device' if where else 'host'}: {runs[where][-1]:.3f} s")
            same = all(a.tobytes() == b.tobytes() for a, b in zip(outs[0][:4], outs[1][:4]))
            subsets = outs[1][4]["subsets"]
            entry = {"depth": depth, "stride": stride, "rows_searched": int(len(rows)),
                     "non_c_rows": int((lens > 0).sum()), "list_min": int(lens[rows].min()),
                     "list_mean": float(lens[rows].mean()), "list_max": int(lens[rows].max()),
                     "candidate_lists_s": t_lists, "subsets": subsets, "same_bytes": bool(same),
                     "device_info": outs[1][4], "host": stats(runs[0]), "device": stats(runs[1])}
            for side in ("host", "device"):
                entry[side]["subsets_per_s"] = subsets / entry[side]["median_s"]
            entry["speedup_median"] = entry["host"]["median_s"] / entry["device"]["median_s"]
            res["search"].append(entry)
    if not args.skip_build:
        b = torch.as_tensor(np.random.default_rng(7).standard_normal(n), device="cuda:0")

        def describe(mg, runs, tag):
            nl = mg.levels()
            nnz = [mg.level(l)[0].nnz for l in range(nl)]
            x = torch.zeros_like(b)
            it, _ = fa.pcg_solve(A, mg, b, x, max_iter=1000, rel_tol=1e-8)
            d = stats([r[0] for r in runs])
            d.update({"levels": nl, "level_rows": [mg.level(l)[0].nrows for l in range(nl)],
                      "operator_complexity": sum(nnz) / nnz[0], "pcg_iterations": int(it),
                      "level_logs": [parse_log(r[1], tag) for r in runs]})
            return d

        cl, sa = [], []
        for r in range(args.reps):
            mg_c, t, text = captured(lambda: fa.classical_build(A, nn, w, where=args.where, coarsest_dim=args.coarsest_dim,
                                                                max_levels=args.max_levels))
            cl.append((t, text))
            log(f"classical build {r}: {t:.3f} s, {mg_c.levels()} levels")
            mg_s, t, text = captured(lambda: fa.smoothed_aggregation(A, nn, weights=w, candidate_dimension=args.sa_cd,
                                                                     coarsest_dim=args.coarsest_dim, smoother="l1"))
            sa.append((t, text))
            log(f"sa build {r}: {t:.3f} s, {mg_s.levels()} levels")
        res["classical_build"] = describe(mg_c, cl, "classical")
        res["classical_build"]["where"] = args.where
        res["sa_build"] = describe(mg_s, sa, "sa")
        res["sa_build"]["candidate_dimension"] = args.sa_cd
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--depths", default="3,5")
    ap.add_argument("--strides", default="1,64", help="per depth: every stride-th non-C row is searched")
    ap.add_argument("--where", type=int, default=1, help="the search of the builds: 0 host, 1 device")
    ap.add_argument("--sa-cd", type=int, default=1, help="candidate_dimension of the amg_sa_build beside it")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--coarsest-dim", type=int, default=1000)
    ap.add_argument("--max-levels", type=int, default=0, help="of the classical build (0: unlimited)")
    ap.add_argument("--level-stages", action="store_true",
                    help="also time amg_ls_interpolation and the RAP of level 0 on their own")
    ap.add_argument("--skip-search", action="store_true")
    ap.add_argument("--skip-build", action="store_true")
    ap.add_argument("--limit", type=int, default=900, help="seconds (the child's timeout)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.depths = [int(v) for v in args.depths.split(",")]
    args.strides = [int(v) for v in args.strides.split(",")]
    if len(args.strides) != len(args.depths):
        sys.exit("one stride per depth")
    if args.child:
        child(args)
        return
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child"] + \
          [a for a in sys.argv[1:] if a != "--child"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(p.stdout)
    sys.stdout.flush()
    if p.returncode != 0:  # a fault, an abort or the time limit: start nothing more on the GPU
        sys.exit(f"exit status {p.returncode}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(l for l in p.stdout.splitlines() if l.startswith("{")) + "\n")


if __name__ == "__main__":
    main()
