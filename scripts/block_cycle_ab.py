#!/usr/bin/env python3
"""A/B of the block V-cycle against the column-by-column path (flag 11).

Times mg.apply on a 32-column device block with flag block_cycle = 1 (one block
cycle, k-wide kernels) and = 0 (32 graph-replayed single-vector cycles: the path
before the block cycle existed), alternating the two, on
  (i)  the C5 stand-in of bench.py --problem elast (Q1 elasticity, 80^3 elements,
       nodes shuffled within windows of 4096, L1, block size 3), and
  (ii) the C2 256^3 7-point box hierarchy (Jacobi),
and adaptive_build(dim=8, max_components=2, test_iters=10) on (i) both ways.
Prints one JSON object: times (median of the repeats, device events), the ratio and
the bytes of the block plan against 32 x the single-vector plan.

The caller bounds the run time (--budget seconds per case, checked between
repeats); nothing is retried.  Needs a GPU.

  python scripts/block_cycle_ab.py --cases c5,c2,adaptive --out profiles/block_cycle/ab.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "faer-amg_amd"))


def time_apply(fa, ctx, mg, out, rhs, reps, budget):
    """Median ms of mg.apply(out, rhs) per flag value, the two alternated."""
    import torch
    ts = {1: [], 0: []}
    t_end = time.monotonic() + budget
    for on in (1, 0):  # warm-up of both paths (graph capture, workspaces)
        fa.set_flag("block_cycle", on)
        mg.apply(out, rhs)
        mg.apply(out, rhs)
    ctx.synchronize()
    for _ in range(reps):
        for on in (1, 0):
            fa.set_flag("block_cycle", on)
            mg.apply(out, rhs)  # (a flag change drops the graphs: re-captured here, outside the timing)
            ctx.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            mg.apply(out, rhs)
            e1.record()
            e1.synchronize()
            ctx.synchronize()
            ts[on].append(e0.elapsed_time(e1))
        if time.monotonic() > t_end:
            break
    fa.set_flag("block_cycle", 1)
    return {("block" if on else "columns") + "_ms": float(np.median(v)) for on, v in ts.items()} | {"repeats": len(ts[1])}


def cycle_case(fa, ctx, A, mg, k, reps, budget):
    import torch
    n = A.nrows
    rhs = torch.as_tensor(np.random.default_rng(1).uniform(-1, 1, (k, n)), device="cuda:0").t()
    out = torch.zeros((k, n), dtype=torch.float64, device="cuda:0").t()
    res = time_apply(fa, ctx, mg, out, rhs, reps, budget)
    res["rows"], res["columns"], res["levels"] = n, k, mg.levels()
    res["speedup"] = res["columns_ms"] / res["block_ms"]
    bp, cp = mg.block_plan(k), mg.cycle_plan()
    res["block_plan_bytes"] = int(sum(p["bytes"] for p in bp))
    res["column_plan_bytes"] = int(k * sum(p["bytes"] for p in cp))
    res["block_plan_launches"], res["column_plan_launches"] = len(bp), k * len(cp)
    res["block_plan_matrix_launches"] = sorted({(p["level"], p["role"], p["name"]) for p in bp if p["kernel"] >= 0})
    # the two paths agree bit for bit on this block
    fa.set_flag("block_cycle", 0)
    ref = torch.zeros_like(out)
    mg.apply(ref, rhs)
    fa.set_flag("block_cycle", 1)
    mg.apply(out, rhs)
    ctx.synchronize()
    res["bitwise_equal"] = bool(torch.equal(out, ref))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c5,c2,adaptive")
    ap.add_argument("--columns", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--budget", type=float, default=60.0, help="seconds of timing per case")
    ap.add_argument("--elements", type=int, default=80)
    ap.add_argument("--edge", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import faer_amg_amd as fa
    if not torch.cuda.is_available():
        sys.exit("block_cycle_ab.py needs a GPU")
    ctx = fa.Context(0)
    res = {"device": torch.cuda.get_device_name(0)}
    cases = args.cases.split(",")
    A5 = None
    if "c5" in cases or "adaptive" in cases:
        e = args.elements
        A5 = fa.elasticity_q1((e, e, e), contrast=1.0, nu=0.3, seed=42, permute=4096).upload(ctx)
    if "c5" in cases:
        nn = fa.constant_candidates(A5.nrows, 3)
        mg = fa.smoothed_aggregation(A5, nn, block_size=3, candidate_dimension=3, coarsest_dim=1000, smoother="l1")
        res["c5"] = cycle_case(fa, ctx, A5, mg, args.columns, args.reps, args.budget)
        print("c5", json.dumps(res["c5"]), flush=True)
        del mg
    if "c2" in cases:
        dims = (args.edge,) * 3
        A = fa.SparseMatOp.laplace3d_7pt(ctx, *dims)
        mg = fa.sa_build_box(A, dims, (2, 2, 2), coarsest_dim=1000, smoother="jacobi")
        res["c2"] = cycle_case(fa, ctx, A, mg, args.columns, args.reps, args.budget)
        print("c2", json.dumps(res["c2"]), flush=True)
        del mg, A
    if "adaptive" in cases:
        ad = {}
        for on in (1, 0):
            fa.set_flag("block_cycle", on)
            ctx.synchronize()
            t0 = time.monotonic()
            comp, cfs = fa.adaptive_build(A5, dim=8, seed=0, max_components=2, test_iters=10, block_size=3,
                                          candidate_dimension=3, coarsest_dim=1000)
            ctx.synchronize()
            ad["block_s" if on else "columns_s"] = time.monotonic() - t0
            ad["cfs_block" if on else "cfs_columns"] = [float(v) for v in cfs[0]]
            del comp
        fa.set_flag("block_cycle", 1)
        ad["speedup"] = ad["columns_s"] / ad["block_s"]
        ad["what"] = "adaptive_build(dim=8, max_components=2, test_iters=10), host wall clock incl. both SA setups"
        res["adaptive"] = ad
        print("adaptive", json.dumps(ad), flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
