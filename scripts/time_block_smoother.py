#!/usr/bin/env python3
"""The k-wide BlockSmoother apply (flag block_smoother_cols = 1) against one launch per
column (flag 0, the only form before the flag existed), in the same process.

Cases (--cases, comma separated; each in a fresh child process under its own timeout):
  box      (a) bare smoother, 7-point edge^3 (default 128) with 2^3 boxes
  runs128  (a) bare smoother, the same operator, nodes grouped into runs of 128
  c5       (a) bare smoother, Q1 elasticity elements^3 (default 80), MIS aggregates of
               the depth-1 strength graph, block_size 3
  cycle    (b) one block V-cycle (mg.apply of a 32-column block) of the
               sa_build_box(smoother="block") hierarchy on the 7-point edge^3 operator
  search   (c) find_near_null(k=7, iters=10) and adaptive_build(dim=8, max_components=2,
               test_iters=10) on the elasticity operator, host wall clock
(a) runs k = 8 and k = 32 out of place on device blocks.  (a) and (b) time with device
events, (a) around `inner` (default 20) back-to-back applies, (b) around 5 cycles; one
warm-up of each side, then `reps` (default 7) repetitions alternating flag 1 and flag 0;
median, minimum and maximum of each side.  (a) also
prints the launches' own bytes model (amg.h: the inverses and 8 B of index per row once
per group of 8 columns + 16 B per row and column) and that model's fraction of 8 TB/s.
With --flag0-only the flag is never set (a library without it: the figures of the parent).
Every case checks that both sides give equal bits.  One JSON object per result line.

  python scripts/time_block_smoother.py [--cases box,runs128,c5,cycle,search] [--out FILE]
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
PEAK = 8e12  # bytes / s


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def box_partition(dims, box):
    nx, ny, nz = dims
    bx, by, bz = box
    cx, cy = -(-nx // bx), -(-ny // by)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (x // bx + cx * (y // by + cy * (z // bz))).ravel().astype(np.int64)


def child(args):
    import torch
    import faer_amg_amd as fa
    if not torch.cuda.is_available():
        sys.exit("time_block_smoother.py needs a GPU")
    ctx = fa.Context(0)
    sides = (0,) if args.flag0_only else (1, 0)

    def set_side(on):
        if not args.flag0_only:
            fa.set_flag("block_smoother_cols", on)

    def event_ms(f, inner=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner

    def alternate(f, timer):
        """{side: [times]} after one warm-up of each side.  Setting a flag makes a multigrid
        drop what it built under the old value (graphs, the dense tail): one untimed call
        after every switch rebuilds that outside the timed window."""
        for on in sides:
            set_side(on)
            timer(f)
        ts = {on: [] for on in sides}
        for _ in range(args.reps):
            for on in sides:
                set_side(on)
                f()
                ts[on].append(timer(f))
        set_side(1)
        return ts

    def emit(**kw):
        kw["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(kw), flush=True)

    def report(case, ts, extra):
        res = dict(case=case, reps=args.reps, **extra)
        for on in sides:
            res["flag%d" % on] = stats(ts[on])
        if len(sides) == 2:
            res["ratio_flag0_over_flag1"] = res["flag0"]["median_ms"] / res["flag1"]["median_ms"]
        return res

    def laplace():
        dims = (args.edge,) * 3
        return dims, fa.SparseMatOp.laplace3d_7pt(ctx, *dims)

    def elasticity():
        return fa.elasticity_q1((args.elements,) * 3, seed=3).upload(ctx)

    def bare(case, A, B):
        n = A.nrows
        # without info() (a library before the flag): the inverse bytes from the CSR form's nonzeros
        info = B.info() if hasattr(B, "info") else {"inverse_bytes": 8 * B.to_sparse().nnz, "chunks_by_width": None,
                                                    "max_block": None, "nblocks": None}
        for k in (8, 32):
            R = torch.as_tensor(np.random.default_rng(7).standard_normal((k, n)), device="cuda:0").t()
            out = {}
            for on in sides:
                set_side(on)
                out[on] = torch.zeros((k, n), dtype=torch.float64, device="cuda:0").t()
                B.apply(out[on], R)
            ctx.synchronize()
            Z = torch.empty((k, n), dtype=torch.float64, device="cuda:0").t()
            ts = alternate(lambda: B.apply(Z, R), lambda f: event_ms(f, args.inner))
            groups = -(-k // 8)
            model = {1: groups * (info["inverse_bytes"] + 8 * n) + 16 * n * k, 0: k * (info["inverse_bytes"] + 24 * n)}
            res = report(case, ts, dict(rows=n, columns=k, calls_per_timing=args.inner, info=info["chunks_by_width"],
                                        max_block=info["max_block"], nblocks=info["nblocks"],
                                        inverse_bytes=info["inverse_bytes"],
                                        bitwise_equal=all(bool(torch.equal(out[on], out[sides[0]])) for on in sides)))
            for on in sides:
                res["flag%d" % on]["model_bytes"] = model[on]
                res["flag%d" % on]["fraction_of_8TBs"] = model[on] / (res["flag%d" % on]["median_ms"] * 1e-3) / PEAK
            emit(**res)

    if args.child == "box":
        dims, A = laplace()
        bare("box", A, fa.BlockSmoother(A, box_partition(dims, (2, 2, 2))))
    elif args.child == "runs128":
        dims, A = laplace()
        bare("runs128", A, fa.BlockSmoother(A, np.arange(A.nrows, dtype=np.int64) // 128))
    elif args.child == "c5":
        A = elasticity()
        nn = fa.constant_candidates(A.nrows, 3)
        G = fa.strength_graph_device(A, nn, fa.create_weights(A, nn), block_size=3)
        agg, na, _ = fa.aggregate_mis_device(G)
        del G
        bare("c5", A, fa.BlockSmoother(A, agg, na, block_size=3))
    elif args.child == "cycle":
        dims, A = laplace()
        mg = fa.sa_build_box(A, dims, (2, 2, 2), coarsest_dim=1000, smoother="block")
        n, k = A.nrows, 32
        R = torch.as_tensor(np.random.default_rng(7).standard_normal((k, n)), device="cuda:0").t()
        out = {}
        for on in sides:
            set_side(on)
            out[on] = torch.zeros((k, n), dtype=torch.float64, device="cuda:0").t()
            mg.apply(out[on], R)
        ctx.synchronize()
        Z = torch.empty((k, n), dtype=torch.float64, device="cuda:0").t()
        ts = alternate(lambda: mg.apply(Z, R), lambda f: event_ms(f, 5))
        plan = mg.block_plan(k)
        names = {}
        for p in plan:
            names[p["name"]] = names.get(p["name"], 0) + 1
        emit(**report("cycle", ts, dict(rows=n, columns=k, levels=mg.levels(), plan_launches=names,
                                        plan_bytes=sum(p["bytes"] for p in plan),
                                        plan_block_smoother_bytes=sum(p["bytes"] for p in plan
                                                                      if p["name"].startswith("block")),
                                        bitwise_equal=all(bool(torch.equal(out[on], out[sides[0]])) for on in sides))))
    elif args.child == "search":
        A = elasticity()
        n = A.nrows

        def wall(f):
            ctx.synchronize()
            t0 = time.perf_counter()
            wall.last = f()
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for name, f in (("find_near_null", lambda: fa.find_near_null(A, 7, iters=10, block_size=3)[1]),
                        ("adaptive_build", lambda: fa.adaptive_build(A, dim=8, max_components=2, test_iters=10,
                                                                     block_size=3)[1])):
            cfs = {}
            for on in sides:
                set_side(on)
                wall(f)
                cfs[on] = np.array(wall.last)
            ts = {on: [] for on in sides}
            for _ in range(args.search_reps):
                for on in sides:
                    set_side(on)
                    ts[on].append(wall(f))
            set_side(1)
            res = report(name, ts, dict(rows=n, bitwise_equal=all(np.array_equal(cfs[on], cfs[sides[0]]) for on in sides)))
            res["reps"] = args.search_reps
            emit(**res)
    else:
        sys.exit("unknown case " + args.child)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="box,runs128,c5,cycle,search")
    ap.add_argument("--edge", type=int, default=128)
    ap.add_argument("--elements", type=int, default=80)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--search-reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="(a): applies between one pair of events")
    ap.add_argument("--limit", type=int, default=400, help="seconds per case (the child's timeout)")
    ap.add_argument("--flag0-only", action="store_true", help="never touch the flag (a library without it)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    lines = []
    for case in args.cases.split(","):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", case,
               "--edge", str(args.edge), "--elements", str(args.elements), "--reps", str(args.reps),
               "--search-reps", str(args.search_reps), "--inner", str(args.inner)] + (["--flag0-only"] if args.flag0_only else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        lines += [l for l in p.stdout.splitlines() if l.startswith("{")]
        if args.out:  # after every case: a later one that fails loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        if p.returncode != 0:  # a fault, an abort or the time limit: start nothing more on the GPU
            sys.exit(f"case {case}: exit status {p.returncode}")


if __name__ == "__main__":
    main()
