#!/usr/bin/env python3
"""Coupled block CG against the independent block PCG (amg_block_cg_solve vs amg_pcg_solve_block).

Two problems, k standard-normal right-hand sides (seed 7), zero guesses, rel_tol 1e-8:
  box:   7-point Laplacian on edge^3 (default 128), the sa_build_box Jacobi hierarchy
  elast: the C5 stand-in, Q1 elasticity on elements^3 (default 80), nodes shuffled within
         windows of 4096, general SA (block size 3, three constant candidates, coarsest_dim
         1000) with the L1 smoother and with the default Chebyshev smoother
  baseline: one pcg_solve_block call (k independent recurrences, the code this library had)
  coupled:  one block_cg_solve call
Method: per repetition X is zeroed, then torch.cuda.synchronize(), the call,
torch.cuda.synchronize(), host perf_counter around the pair; one warm-up of each side,
then `reps` (5) repetitions alternating the two sides; the median of each.  Reports the
iteration counts (baseline: of its slowest column), the ranks of the coupled solve, ms in
total and per iteration, and the worst true relative residual of both answers.  Prints one
JSON object per (problem, hierarchy, k).

--trace: one warm-up and one coupled solve per k and nothing else, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python scripts/time_block_cg.py --child box --trace):
the launches are k_bcg_gram_partial + k_gram_final ("bcg_gram") and k_bcg_gemm
("bcg_update", "bcg_dir").

Each problem runs in a fresh child process under its own `timeout` (the parent never
touches the GPU), and nothing is retried:

  python scripts/time_block_cg.py [--problems box,elast] [--columns 8,32] [--limit 900] [--out FILE]
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
    print(f"[time_block_cg] {msg}", file=sys.stderr, flush=True)


def child(problem, size, ks, reps, trace):
    import torch
    import faer_amg_amd as fa
    if not torch.cuda.is_available():
        sys.exit("time_block_cg.py needs a GPU")
    ctx = fa.Context(0)
    t0 = time.perf_counter()
    if problem == "box":
        dims = (size,) * 3
        A = fa.SparseMatOp.laplace3d_7pt(ctx, *dims)
        configs = [("box_jacobi", fa.sa_build_box(A, dims, (2, 2, 2), coarsest_dim=1000, smoother="jacobi"))]
    else:
        A = fa.elasticity_q1((size,) * 3, contrast=1.0, nu=0.3, seed=42, permute=4096).upload(ctx)
        nn = fa.constant_candidates(A.nrows, 3)
        sa = dict(block_size=3, candidate_dimension=3, coarsest_dim=1000)
        configs = [("sa_l1", fa.smoothed_aggregation(A, nn, smoother="l1", **sa)),
                   ("sa_chebyshev", fa.smoothed_aggregation(A, nn, smoother="chebyshev", **sa))]
    n = A.nrows
    log(f"{problem} {size}: {n} rows, {A.nnz} nnz, hierarchies {[m.levels() for _, m in configs]} levels, "
        f"{time.perf_counter() - t0:.1f} s")
    kw = dict(max_iter=1000, rel_tol=1e-8)
    for k in ks:
        B = torch.as_tensor(np.random.default_rng(7).standard_normal((k, n)), device="cuda:0").t()  # column-major n x k
        X = torch.zeros((k, n), dtype=torch.float64, device="cuda:0").t()
        R = torch.zeros((k, n), dtype=torch.float64, device="cuda:0").t()
        bn = torch.linalg.vector_norm(B, dim=0)

        def timed(f):
            X.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, r

        def true_residual():
            A.apply(R, X)
            ctx.synchronize()
            return float((torch.linalg.vector_norm(B - R, dim=0) / bn).max())

        for name, mg in configs:
            sides = {"independent": lambda: fa.pcg_solve_block(A, mg, B, X, **kw),
                     "coupled": lambda: fa.block_cg_solve(A, mg, B, X, **kw)}
            if trace:
                for _ in range(2):
                    t, r = timed(sides["coupled"])
                print(json.dumps({"problem": problem, "hierarchy": name, "rows": n, "columns": k, "iterations": r[0],
                                  "coupled_ms": t}), flush=True)
                continue
            ts = {s: [] for s in sides}
            out = {}
            for s, f in sides.items():  # warm-up: workspaces, graph capture
                t, _ = timed(f)
                log(f"{name} k={k} warm-up {s}: {t:.1f} ms")
            for _ in range(reps):
                for s, f in sides.items():
                    t, r = timed(f)
                    ts[s].append(t)
                    out[s] = (r, true_residual())
            its_i = [int(v) for v in out["independent"][0][0]]
            it_c = int(out["coupled"][0][0])
            ranks = [int(v) for v in out["coupled"][0][2]]
            med = {s: float(np.median(ts[s])) for s in sides}
            print(json.dumps({
                "device": torch.cuda.get_device_name(0), "problem": problem, "size": size, "hierarchy": name, "rows": n,
                "nnz": A.nnz, "columns": k,
                "method": "host perf_counter around the call between torch.cuda.synchronize(); median of %d "
                          "alternated repetitions after 1 warm-up" % reps,
                "independent": {"iterations_min": min(its_i), "iterations_max": max(its_i), "total_ms": med["independent"],
                                "ms_per_iteration": med["independent"] / max(max(its_i), 1),
                                "all_ms": ts["independent"], "true_rel_residual_max": out["independent"][1]},
                "coupled": {"iterations": it_c, "ranks_min": min(ranks) if ranks else None,
                            "ranks_last": ranks[-1] if ranks else None, "total_ms": med["coupled"],
                            "ms_per_iteration": med["coupled"] / max(it_c, 1), "all_ms": ts["coupled"],
                            "true_rel_residual_max": out["coupled"][1],
                            "host_synchronisations_per_iteration": 3},
                "ratio_independent_over_coupled": med["independent"] / med["coupled"],
            }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="box,elast")
    ap.add_argument("--edge", type=int, default=128)
    ap.add_argument("--elements", type=int, default=80)
    ap.add_argument("--columns", default="8,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=900, help="seconds per problem (the child's timeout)")
    ap.add_argument("--trace", action="store_true", help="one warm-up and one coupled solve per k (for a kernel trace)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help="run this problem in this process (what the parent starts)")
    args = ap.parse_args()
    ks = [int(v) for v in args.columns.split(",")]
    if args.child:
        child(args.child, args.edge if args.child == "box" else args.elements, ks, args.reps, args.trace)
        return
    lines = []
    for problem in args.problems.split(","):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", problem,
               "--edge", str(args.edge), "--elements", str(args.elements), "--columns", args.columns,
               "--reps", str(args.reps)] + (["--trace"] if args.trace else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:  # a fault, an abort or the time limit: start nothing more on the GPU
            sys.exit(f"{problem}: exit status {p.returncode}")
        lines += [l for l in p.stdout.splitlines() if l.startswith("{")]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
