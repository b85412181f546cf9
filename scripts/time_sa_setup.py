#!/usr/bin/env python3
"""amg_sa_build on the C5 stand-in with the strength graph and the aggregation on the
host (amg_set_sa_setup(0), the default) against the device (amg_set_sa_setup(1)).

Q1 elasticity on elements^3 (default 80: 1.57M rows), nodes shuffled within windows of
4096 (bench.py --problem elast), general SA with block size 3, three constant
candidates, candidate_dimension 3, coarsest_dim 1000, the L1 smoother -- the setup
scripts/time_chebyshev_pcg.py reports as "SA setup".
Method: the two policies alternate in one process, `reps` (3) builds each, the host
policy first (so the process's first build, which also pays first-use costs, is a host
one); per build torch.cuda.synchronize(), the call, torch.cuda.synchronize(), host
perf_counter around the pair; the median of each policy.  FAMG_SA_LOG=1 is set for
every build: the library's per-level, per-stage wall times are read from its stderr
(the switch synchronises the stream at stage ends, where every stage but the strength
graph and the aggregation already does).  Reported per policy: every build's seconds
and the median, levels, rows / aggregates / strength edges / passes per level, the
per-level stage times (median over the builds, ms), and the PCG iterations to rel_tol
1e-8 on the last hierarchy for one standard-normal right-hand side.  Prints one JSON
object.

The measurement runs in a fresh child process under its own `timeout` (the parent never
touches the GPU), and nothing is retried:

  python scripts/time_sa_setup.py [--elements 80] [--limit 600] [--out FILE]
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

STAGES = ("strength", "aggregation", "tentative", "smoothing", "rap", "nearnull")


def log(msg):
    print(f"[time_sa_setup] {msg}", file=sys.stderr, flush=True)


def parse_sa_log(text):
    """The FAMG_SA_LOG lines of one build: per-level dicts and the smoothers' ms."""
    levels, smoothers = [], None
    for line in text.splitlines():
        m = re.match(r"famg sa level (\d+): (.*) ms: (.*)$", line)
        if m:
            d = {"level": int(m.group(1))}
            toks = m.group(2).split()
            d.update({toks[i]: int(toks[i + 1]) for i in range(0, len(toks), 2)})
            toks = m.group(3).split()
            d.update({toks[i]: float(toks[i + 1]) for i in range(0, len(toks), 2)})
            levels.append(d)
        m = re.match(r"famg sa smoothers: .* smoothers ([0-9.]+)$", line)
        if m:
            smoothers = float(m.group(1))
    return levels, smoothers


def child(elements, reps):
    os.environ["FAMG_SA_LOG"] = "1"  # read once, at the first build
    import torch
    import faer_amg_amd as fa
    if not torch.cuda.is_available():
        sys.exit("time_sa_setup.py needs a GPU")
    ctx = fa.Context(0)
    t0 = time.perf_counter()
    A = fa.elasticity_q1((elements,) * 3, contrast=1.0, nu=0.3, seed=42, permute=4096).upload(ctx)
    n = A.nrows
    log(f"operator: {n} rows, {A.nnz} nnz, {time.perf_counter() - t0:.1f} s")
    nn = fa.constant_candidates(n, 3)

    def build(policy):
        fa.set_sa_setup(policy)
        sys.stderr.flush()
        saved = os.dup(2)
        with tempfile.TemporaryFile() as tf:
            os.dup2(tf.fileno(), 2)  # the library writes its stage times to fd 2
            try:
                torch.cuda.synchronize()
                t = time.perf_counter()
                mg = fa.smoothed_aggregation(A, nn, block_size=3, candidate_dimension=3, coarsest_dim=1000,
                                             smoother="l1")
                torch.cuda.synchronize()
                t = time.perf_counter() - t
            finally:
                os.dup2(saved, 2)
                os.close(saved)
                fa.set_sa_setup(0)
            tf.seek(0)
            levels, smoothers = parse_sa_log(tf.read().decode())
        return mg, t, levels, smoothers

    names = {0: "host", 1: "device"}
    runs = {0: [], 1: []}
    last = {}
    for r in range(reps):
        for policy in (0, 1):
            last.pop(policy, None)  # one hierarchy of each policy alive at a time
            mg, t, levels, smoothers = build(policy)
            log(f"build {r} {names[policy]}: {t:.3f} s, {mg.levels()} levels")
            runs[policy].append({"s": t, "levels": levels, "smoothers_ms": smoothers})
            last[policy] = mg
    b = torch.as_tensor(np.random.default_rng(7).standard_normal(n), device="cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "elements": elements, "rows": n, "nnz": A.nnz,
           "method": "host perf_counter around amg_sa_build between torch.cuda.synchronize(); the two policies "
                     "alternated in one process, host first; median of %d; FAMG_SA_LOG=1 stage times" % reps,
           "policies": {}}
    for policy in (0, 1):
        rs = runs[policy]
        lv = rs[-1]["levels"]
        stages = []
        for l in range(len(lv)):
            stages.append({s: float(np.median([r["levels"][l][s] for r in rs])) for s in STAGES})
        x = torch.zeros_like(b)
        it, _ = fa.pcg_solve(A, last[policy], b, x, max_iter=1000, rel_tol=1e-8)
        res["policies"][names[policy]] = {
            "all_s": [r["s"] for r in rs], "median_s": float(np.median([r["s"] for r in rs])),
            "levels": last[policy].levels(),
            "level_rows": [d["n"] for d in lv], "level_nodes": [d["nodes"] for d in lv],
            "aggregates": [d["aggregates"] for d in lv], "strength_edges": [d["edges"] for d in lv],
            "on_device": [d["device"] for d in lv], "passes": [d["passes"] for d in lv],
            "fallback": [d["fallback"] for d in lv],
            "stage_ms": stages, "stage_total_ms": {s: float(sum(st[s] for st in stages)) for s in STAGES},
            "smoothers_ms": float(np.median([r["smoothers_ms"] for r in rs])),
            "pcg_iterations": int(it)}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=80, help="elements per edge (80: 1.57M rows)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=600, help="seconds (the child's timeout)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.elements, args.reps)
        return
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child",
           "--elements", str(args.elements), "--reps", str(args.reps)]
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
