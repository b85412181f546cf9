#!/usr/bin/env python3
"""amg_sa_refresh against amg_sa_build on the C5 stand-in: Q1 elasticity on size^3
elements, nodes shuffled within windows of 4096, block size 3, three constant
candidates, coarsest_dim 1000, the L1 smoother.  A is the mesh at contrast 1, A' the
same mesh (the same pattern) at --contrast.

Method: one process per (setup policy, strength depth).  `reps` (3) times, alternated:
a hierarchy is built on A (untimed); amg_sa_build(A') is timed -- the yardstick, the
parent commit's own figure since the build is unchanged; the first refresh of the
A-hierarchy to A' (it records the patterns) and a later refresh to A' are timed.  Per
call torch.cuda.synchronize(), the call, torch.cuda.synchronize(), host perf_counter
around the pair.  FAMG_SA_LOG=1: the library's stage lines of every timed call are kept.
`faster` compares ranges: true only where the refresh's maximum lies below the build's
minimum.  The two level-0 products A' P and R (A' P) are timed with device events on
the context's stream around amg_spgemm and around amg_spgemm_refill (each call with its
own host synchronisations, 3 repetitions, after one warm-up).  PCG iterations to 1e-8 on
A' for one standard-normal right-hand side: the refreshed hierarchy (frozen aggregates)
and the freshly built one.  One JSON object.

The measurement runs in a fresh child process under its own `timeout` (the parent never
touches the GPU), and nothing is retried:

  python scripts/time_sa_refresh.py --elements 80 --policy 0 --depth 1 [--reps 3]
                                    [--contrast 2.0] [--limit 900] [--out FILE]
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

NAMES = {0: "host", 1: "device"}


def log(msg):
    print(f"[time_sa_refresh] {msg}", file=sys.stderr, flush=True)


def spread(values):
    return {"all": [float(v) for v in values], "median": float(np.median(values)), "min": float(min(values)),
            "max": float(max(values))}


def stage_sums(text):
    """Sum over the levels of every `name value` pair after `ms:` on the library's stage lines."""
    out = {}
    for line in text.splitlines():
        if not line.startswith("famg sa") or " ms: " not in line:
            continue
        for name, v in re.findall(r"([a-z]+) ([0-9.]+)", line.split(" ms: ", 1)[1]):
            out[name] = out.get(name, 0.0) + float(v)
    return out


def child(elements, policy, depth, reps, contrast):
    os.environ["FAMG_SA_LOG"] = "1"  # read once, at the first build
    import torch
    import faer_amg_amd as fa
    if not torch.cuda.is_available():
        sys.exit("time_sa_refresh.py needs a GPU")
    ctx = fa.Context(0)
    t0 = time.perf_counter()
    gen = dict(nu=0.3, seed=42, permute=4096)
    A = fa.elasticity_q1((elements,) * 3, contrast=1.0, **gen).upload(ctx)
    A2 = fa.elasticity_q1((elements,) * 3, contrast=contrast, **gen).upload(ctx)
    n = A.nrows
    log(f"operators: {n} rows, {A.nnz} nnz, {time.perf_counter() - t0:.1f} s")
    nn = fa.constant_candidates(n, 3)

    def timed(f):
        sys.stderr.flush()
        saved = os.dup(2)
        with tempfile.TemporaryFile() as tf:
            os.dup2(tf.fileno(), 2)  # the library writes its stage times to fd 2
            try:
                torch.cuda.synchronize()
                t = time.perf_counter()
                r = f()
                torch.cuda.synchronize()
                t = time.perf_counter() - t
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            tf.seek(0)
            return r, t, stage_sums(tf.read().decode())

    def build(M):
        fa.set_sa_setup(policy)
        try:
            return fa.smoothed_aggregation(M, nn, block_size=3, candidate_dimension=3, coarsest_dim=1000,
                                           smoother="l1", strength_depth=depth)
        finally:
            fa.set_sa_setup(0)

    runs = {"build": [], "first_refresh": [], "later_refresh": []}
    mg = fresh = info = None
    for r in range(reps):
        mg = fresh = None  # one hierarchy of each kind alive at a time
        mg = build(A)
        fresh, t, st = timed(lambda: build(A2))
        runs["build"].append({"s": t, "stage_ms": st})
        info, t1, st1 = timed(lambda: mg.refresh(A2, nn))
        assert info["recorded"]
        runs["first_refresh"].append({"s": t1, "stage_ms": st1})
        info, t2, st2 = timed(lambda: mg.refresh(A2, nn))
        assert not info["recorded"]
        runs["later_refresh"].append({"s": t2, "stage_ms": st2})
        log(f"rep {r}: build {t:.3f} s, first refresh {t1:.3f} s, later refresh {t2:.3f} s")
    res = {"device": torch.cuda.get_device_name(0), "elements": elements, "rows": n, "nnz": A.nnz,
           "policy": NAMES[policy], "depth": depth, "contrast": contrast, "levels": mg.levels(),
           "record_bytes": info["record_bytes"],
           "method": "host perf_counter around each call between torch.cuda.synchronize(); build(A'), first and "
                     "later refresh alternated in one process, %d of each; FAMG_SA_LOG=1 stage sums" % reps}
    for k, rs in runs.items():
        res[k] = {"s": spread([r["s"] for r in rs]),
                  "stage_ms": {s: float(np.median([r["stage_ms"].get(s, 0.0) for r in rs])) for s in rs[-1]["stage_ms"]}}
    res["faster"] = {k: res[k]["s"]["max"] < res["build"]["s"]["min"] for k in ("first_refresh", "later_refresh")}
    # the level-0 products: amg_spgemm against the refill on its pattern, device events
    stream = torch.cuda.ExternalStream(ctx.stream) if ctx.stream else torch.cuda.default_stream()
    _, _, R0, P0 = mg.level(0)

    def events(f):
        ms = []
        for it in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            f()
            e1.record(stream)
            torch.cuda.synchronize()
            if it:
                ms.append(e0.elapsed_time(e1))
        return spread(ms)

    AP = fa.spgemm(A2, P0)
    C = fa.spgemm(R0, AP)
    res["products_ms"] = {"AP_spgemm": events(lambda: fa.spgemm(A2, P0)),
                          "AP_refill": events(lambda: fa.spgemm_refill(A2, P0, AP)),
                          "RAP_spgemm": events(lambda: fa.spgemm(R0, AP)),
                          "RAP_refill": events(lambda: fa.spgemm_refill(R0, AP, C)),
                          "note": "whole calls: amg_spgemm with its symbolic pass, scan, allocation and finalize; "
                                  "amg_spgemm_refill with its row-length pass and the finalize of C"}
    b = torch.as_tensor(np.random.default_rng(7).standard_normal(n), device="cuda:0")
    its = {}
    for name, M in (("refreshed", mg), ("fresh_build", fresh)):
        x = torch.zeros_like(b)
        it, _ = fa.pcg_solve(A2, M, b, x, max_iter=1000, rel_tol=1e-8)
        its[name] = int(it)
    res["pcg_iterations"] = its
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=80)
    ap.add_argument("--policy", type=int, choices=(0, 1), default=0, help="amg_set_sa_setup: 0 host, 1 device")
    ap.add_argument("--depth", type=int, default=1)
    ap.add_argument("--contrast", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=900, help="seconds (the child's timeout)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.elements, args.policy, args.depth, args.reps, args.contrast)
        return
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child",
           "--elements", str(args.elements), "--policy", str(args.policy), "--depth", str(args.depth),
           "--contrast", str(args.contrast), "--reps", str(args.reps)]
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
