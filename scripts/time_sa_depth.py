#!/usr/bin/env python3
"""amg_sa_build at strength depth > 1 with the strength graph and the aggregation on the
host (amg_set_sa_setup(0), the default) against the device (amg_set_sa_setup(1): the BFS
balls, the ranking and the MIS passes on the GPU).

Problems: `lap` -- the 7-point Laplacian on size^3 with one constant candidate (block
size 1); `elast` -- the C5 stand-in, Q1 elasticity on size^3 elements, nodes shuffled
within windows of 4096, block size 3, three constant candidates.  General SA,
coarsest_dim 1000, the L1 smoother, strength_depth = --depth.
Method (scripts/time_sa_setup.py's): the policies named by --policies alternate in one
process, `reps` (3) builds each, the host first when it is among them; per build
torch.cuda.synchronize(), the call, torch.cuda.synchronize(), host perf_counter around
the pair.  FAMG_SA_LOG=1 is set for every build: the library's per-level, per-stage wall
times, the longest ball and the reason a level stayed on the host are read from its
stderr.  Reported per policy: every build's seconds with median, min and max; the
strength stage summed over the levels per build (ms) with median, min and max; levels,
rows / aggregates / strength edges / MIS passes / longest ball / reason per level; the
per-level stage times (median, ms); the PCG iterations to rel_tol 1e-8 on the last
hierarchy for one standard-normal right-hand side.  `device_faster` compares the ranges:
true only where the device's maximum lies below the host's minimum.  One JSON object.

The measurement runs in a fresh child process under its own `timeout` (the parent never
touches the GPU), and nothing is retried:

  python scripts/time_sa_depth.py --problem elast --size 40 --depth 3 [--policies 0,1]
                                  [--reps 3] [--limit 600] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "faer-amg_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from time_sa_setup import STAGES, parse_sa_log  # noqa: E402

NAMES = {0: "host", 1: "device"}


def log(msg):
    print(f"[time_sa_depth] {msg}", file=sys.stderr, flush=True)


def spread(values):
    return {"all": [float(v) for v in values], "median": float(np.median(values)), "min": float(min(values)),
            "max": float(max(values))}


def child(problem, size, depth, policies, reps):
    os.environ["FAMG_SA_LOG"] = "1"  # read once, at the first build
    import torch
    import faer_amg_amd as fa
    if not torch.cuda.is_available():
        sys.exit("time_sa_depth.py needs a GPU")
    ctx = fa.Context(0)
    t0 = time.perf_counter()
    if problem == "lap":
        A = fa.SparseMatOp.laplace3d_7pt(ctx, size, size, size)
        bs = 1
    else:
        A = fa.elasticity_q1((size,) * 3, contrast=1.0, nu=0.3, seed=42, permute=4096).upload(ctx)
        bs = 3
    n = A.nrows
    log(f"operator: {n} rows, {A.nnz} nnz, {time.perf_counter() - t0:.1f} s")
    nn = fa.constant_candidates(n, bs)

    def build(policy):
        fa.set_sa_setup(policy)
        sys.stderr.flush()
        saved = os.dup(2)
        with tempfile.TemporaryFile() as tf:
            os.dup2(tf.fileno(), 2)  # the library writes its stage times to fd 2
            try:
                torch.cuda.synchronize()
                t = time.perf_counter()
                mg = fa.smoothed_aggregation(A, nn, block_size=bs, candidate_dimension=bs, coarsest_dim=1000,
                                             smoother="l1", strength_depth=depth)
                torch.cuda.synchronize()
                t = time.perf_counter() - t
            finally:
                os.dup2(saved, 2)
                os.close(saved)
                fa.set_sa_setup(0)
            tf.seek(0)
            levels, smoothers = parse_sa_log(tf.read().decode())
        return mg, t, levels, smoothers

    runs = {p: [] for p in policies}
    last = {}
    for r in range(reps):
        for policy in policies:
            last.pop(policy, None)  # one hierarchy of each policy alive at a time
            mg, t, levels, smoothers = build(policy)
            log(f"build {r} {NAMES[policy]}: {t:.3f} s, {mg.levels()} levels, strength "
                f"{sum(d['strength'] for d in levels):.1f} ms")
            runs[policy].append({"s": t, "levels": levels, "smoothers_ms": smoothers})
            last[policy] = mg
    b = torch.as_tensor(np.random.default_rng(7).standard_normal(n), device="cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "problem": problem, "size": size, "depth": depth, "rows": n,
           "nnz": A.nnz,
           "method": "host perf_counter around amg_sa_build between torch.cuda.synchronize(); the policies "
                     "alternated in one process, host first; %d builds each; FAMG_SA_LOG=1 stage times" % reps,
           "policies": {}}
    for policy in policies:
        rs = runs[policy]
        lv = rs[-1]["levels"]
        stages = [{s: float(np.median([r["levels"][l][s] for r in rs])) for s in STAGES} for l in range(len(lv))]
        x = torch.zeros_like(b)
        it, _ = fa.pcg_solve(A, last[policy], b, x, max_iter=1000, rel_tol=1e-8)
        res["policies"][NAMES[policy]] = {
            "build_s": spread([r["s"] for r in rs]),
            "strength_ms": spread([sum(d["strength"] for d in r["levels"]) for r in rs]),
            "aggregation_ms": spread([sum(d["aggregation"] for d in r["levels"]) for r in rs]),
            "levels": last[policy].levels(),
            "level_rows": [d["n"] for d in lv], "aggregates": [d["aggregates"] for d in lv],
            "strength_edges": [d["edges"] for d in lv], "on_device": [d["device"] for d in lv],
            "reason": [d["reason"] for d in lv], "longest_ball": [d["ball"] for d in lv],
            "passes": [d["passes"] for d in lv], "fallback": [d["fallback"] for d in lv],
            "stage_ms": stages, "pcg_iterations": int(it)}
    P = res["policies"]
    if "host" in P and "device" in P:
        res["device_faster"] = {k: P["device"][k]["max"] < P["host"][k]["min"] for k in ("build_s", "strength_ms")}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problem", choices=("lap", "elast"), default="elast")
    ap.add_argument("--size", type=int, default=40, help="grid points (lap) or elements (elast) per edge")
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--policies", default="0,1", help="0 host, 1 device; '1' times the device alone")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=600, help="seconds (the child's timeout)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    policies = sorted({int(p) for p in args.policies.split(",")})
    if not policies or any(p not in NAMES for p in policies) or args.depth < 1:
        ap.error("policies are 0 and 1, depth >= 1")
    if args.child:
        child(args.problem, args.size, args.depth, policies, args.reps)
        return
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child",
           "--problem", args.problem, "--size", str(args.size), "--depth", str(args.depth),
           "--policies", ",".join(str(p) for p in policies), "--reps", str(args.reps)]
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
