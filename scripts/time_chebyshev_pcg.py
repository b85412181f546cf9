#!/usr/bin/env python3
"""PCG on the C5 stand-in with the L1 hierarchy against Chebyshev hierarchies.

Q1 elasticity on elements^3 (default 80: 1.57M rows), nodes shuffled within windows of
4096 (bench.py --problem elast), general SA with block size 3 and three constant
candidates, coarsest_dim 1000.  One SA setup: the L1 hierarchy is amg_sa_build's; the
Chebyshev hierarchies (steps 2 and 3, the default bound) are assembled over the same
A_l / R_l / P_l and coarse solve with amg_chebyshev_create smoothers, which is what
amg_sa_build(smoother = 4) builds from them.
  single: amg_pcg_solve, one standard-normal right-hand side, zero guess, rel_tol 1e-8
  block:  amg_pcg_solve_block, k = 8 right-hand sides
Method: per repetition X is zeroed, then torch.cuda.synchronize(), the call,
torch.cuda.synchronize(), host perf_counter around the pair; one warm-up of every
configuration, then `reps` (5) repetitions alternating the configurations; the median
of each.  Reports iterations, total ms and ms per iteration (block: per iteration of its
slowest column).  Prints one JSON object.

The measurement runs in a fresh child process under its own `timeout` (the parent never
touches the GPU), and nothing is retried:

  python scripts/time_chebyshev_pcg.py [--elements 80] [--limit 900] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "faer-amg_amd"))


def log(msg):
    print(f"[time_chebyshev_pcg] {msg}", file=sys.stderr, flush=True)


def child(elements, k, reps):
    import torch
    import faer_amg_amd as fa
    if not torch.cuda.is_available():
        sys.exit("time_chebyshev_pcg.py needs a GPU")
    ctx = fa.Context(0)
    t0 = time.perf_counter()
    A = fa.elasticity_q1((elements,) * 3, contrast=1.0, nu=0.3, seed=42, permute=4096).upload(ctx)
    n = A.nrows
    log(f"operator: {n} rows, {A.nnz} nnz, {time.perf_counter() - t0:.1f} s")
    t0 = time.perf_counter()
    nn = fa.constant_candidates(n, 3)
    mg_l1 = fa.smoothed_aggregation(A, nn, block_size=3, candidate_dimension=3, coarsest_dim=1000, smoother="l1")
    nl = mg_l1.levels()
    log(f"SA setup: {nl} levels, {time.perf_counter() - t0:.1f} s")
    levels = [mg_l1.level(l) for l in range(nl)]

    def chebyshev_hierarchy(steps):
        t = time.perf_counter()
        sm = [fa.new_chebyshev(levels[l][0], steps=steps) for l in range(nl - 1)]
        mg = fa.Multigrid(A, sm[0])
        for l in range(1, nl):
            mg.add_level(levels[l][0], sm[l] if l < nl - 1 else levels[l][1], levels[l - 1][2], levels[l - 1][3])
        info = [fa.chebyshev_info(s) for s in sm]
        log(f"chebyshev steps {steps}: smoothers in {time.perf_counter() - t:.2f} s, lambda_max per level "
            f"{[round(i['lambda_max'], 4) for i in info]}")
        return mg, info

    mg_c2, info2 = chebyshev_hierarchy(2)
    mg_c3, _ = chebyshev_hierarchy(3)
    configs = [("l1", mg_l1), ("chebyshev_2", mg_c2), ("chebyshev_3", mg_c3)]
    rng = np.random.default_rng(7)
    b = torch.as_tensor(rng.standard_normal(n), device="cuda:0")
    x = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    B = torch.as_tensor(rng.standard_normal((k, n)), device="cuda:0").t()  # column-major n x k
    X = torch.zeros((k, n), dtype=torch.float64, device="cuda:0").t()
    kw = dict(max_iter=1000, rel_tol=1e-8)

    def timed(f, out):
        out.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    res = {"device": torch.cuda.get_device_name(0), "elements": elements, "rows": n, "nnz": A.nnz, "levels": nl,
           "level_rows": [lv[0].nrows for lv in levels], "fine_level_renumbered": {},
           "chebyshev_lambda_max": [i["lambda_max"] for i in info2],
           "chebyshev_ritz": [i["ritz"] for i in info2], "chebyshev_row_sum_bound": [i["row_sum_bound"] for i in info2],
           "method": "host perf_counter around the call between torch.cuda.synchronize(); median of %d alternated "
                     "repetitions after 1 warm-up" % reps,
           "single": {}, "block": {}, "columns": k}
    for mode, run in (("single", lambda mg: fa.pcg_solve(A, mg, b, x, **kw)),
                      ("block", lambda mg: fa.pcg_solve_block(A, mg, B, X, **kw))):
        out = x if mode == "single" else X
        ts = {name: [] for name, _ in configs}
        its = {}
        for name, mg in configs:  # warm-up: workspaces, renumbering, graph capture
            t, r = timed(lambda: run(mg), out)
            log(f"{mode} warm-up {name}: {t:.1f} ms")
        for _ in range(reps):
            for name, mg in configs:
                t, r = timed(lambda: run(mg), out)
                ts[name].append(t)
                its[name] = int(r[0]) if mode == "single" else [int(v) for v in r[0]]
        for name, mg in configs:
            it = its[name] if mode == "single" else max(its[name])
            med = float(np.median(ts[name]))
            res[mode][name] = {"iterations": its[name], "total_ms": med, "ms_per_iteration": med / max(it, 1),
                               "all_ms": ts[name]}
            res["fine_level_renumbered"][name] = bool(mg.reordered(0))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=80, help="elements per edge (80: 1.57M rows)")
    ap.add_argument("--columns", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=900, help="seconds (the child's timeout)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.elements, args.columns, args.reps)
        return
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child",
           "--elements", str(args.elements), "--columns", str(args.columns), "--reps", str(args.reps)]
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
