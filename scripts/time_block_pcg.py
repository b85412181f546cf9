#!/usr/bin/env python3
"""Block PCG against k consecutive single solves (amg_pcg_solve_block vs amg_pcg_solve).

7-point Laplacian on edge^3 (default 128), the sa_build_box Jacobi hierarchy as the
preconditioner, k = 8 standard-normal right-hand sides, zero guesses, rel_tol 1e-8.
  baseline: k consecutive pcg_solve calls (the single-vector driver, whose code this
            library has had all along), one per column, same process, same hierarchy
  block:    one pcg_solve_block call over the k columns
Method: per repetition X is zeroed, then torch.cuda.synchronize(), the call(s),
torch.cuda.synchronize(), host perf_counter around the pair; one warm-up of each
side, then `reps` (5) repetitions alternating the two sides; the median of each.
Also checks that the two sides agree bit for bit and prints the iteration counts.
Prints one JSON object per edge.

Each edge runs in a fresh child process under its own `timeout` (the parent never
touches the GPU), and nothing is retried:

  python scripts/time_block_pcg.py [--edges 128,256] [--limit 300] [--out FILE]
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


def child(edge, k, reps, block_cycle):
    import torch
    import faer_amg_amd as fa
    if not torch.cuda.is_available():
        sys.exit("time_block_pcg.py needs a GPU")
    ctx = fa.Context(0)
    fa.set_flag("block_cycle", block_cycle)
    dims = (edge,) * 3
    A = fa.SparseMatOp.laplace3d_7pt(ctx, *dims)
    mg = fa.sa_build_box(A, dims, (2, 2, 2), coarsest_dim=1000, smoother="jacobi")
    n = A.nrows
    B = torch.as_tensor(np.random.default_rng(7).standard_normal((k, n)), device="cuda:0").t()  # column-major n x k
    Xb = torch.zeros((k, n), dtype=torch.float64, device="cuda:0").t()
    Xs = torch.zeros((k, n), dtype=torch.float64, device="cuda:0").t()
    cols = [(B[:, c], Xs[:, c]) for c in range(k)]  # contiguous column views
    kw = dict(max_iter=200, rel_tol=1e-8)

    def singles():
        return [fa.pcg_solve(A, mg, b, x, **kw) for b, x in cols]

    def block():
        return fa.pcg_solve_block(A, mg, B, Xb, **kw)

    def timed(f, X):
        X.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    timed(singles, Xs), timed(block, Xb)  # warm-up: workspaces, graph capture
    ts, tb = [], []
    for _ in range(reps):
        t, rs = timed(singles, Xs)
        ts.append(t)
        t, rb = timed(block, Xb)
        tb.append(t)
    its_s = [int(r[0]) for r in rs]
    its_b = [int(v) for v in rb[0]]
    res = {
        "device": torch.cuda.get_device_name(0), "edge": edge, "rows": n, "columns": k, "levels": mg.levels(),
        "block_cycle_flag": block_cycle,
        "method": "host perf_counter around the call(s) between torch.cuda.synchronize(); median of %d after 1 warm-up" % reps,
        "singles_ms": float(np.median(ts)), "block_ms": float(np.median(tb)),
        "singles_all_ms": ts, "block_all_ms": tb,
        "iters_singles": its_s, "iters_block": its_b,
        "bitwise_equal": bool(torch.equal(Xs, Xb)) and its_s == its_b and
        all(np.array_equal(rs[c][1], rb[1][c]) for c in range(k)),
    }
    res["ratio_singles_over_block"] = res["singles_ms"] / res["block_ms"]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", default="128")
    ap.add_argument("--columns", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds per edge (the child's timeout)")
    ap.add_argument("--block-cycle", type=int, default=1, choices=[0, 1],
                    help="flag 11: how the preconditioner takes the block (1 = one block cycle, the default; "
                         "0 = one graph-replayed cycle per column)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.columns, args.reps, args.block_cycle)
        return
    lines = []
    for edge in (int(e) for e in args.edges.split(",")):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(edge),
               "--columns", str(args.columns), "--reps", str(args.reps), "--block-cycle", str(args.block_cycle)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:  # a fault, an abort or the time limit: start nothing more on the GPU
            sys.exit(f"edge {edge}: exit status {p.returncode}")
        lines += [l for l in p.stdout.splitlines() if l.startswith("{")]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
