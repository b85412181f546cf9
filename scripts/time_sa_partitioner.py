#!/usr/bin/env python3
"""The modularity partitioner on the C5 stand-in: host against device,
and amg_sa_build under the MIS aggregates against the modularity aggregates.

Q1 elasticity on elements^3 (default 80: 1.57M rows), nodes shuffled within windows of
4096 (bench.py --problem elast), general SA with block size 3, three constant
candidates, candidate_dimension 3, coarsest_dim 1000, the L1 smoother -- the setup of
scripts/time_sa_setup.py.

Method: one process; the four builds {MIS, modularity} x {host setup, device setup}
alternate, `reps` (3) of each, the host MIS build first (it also pays the process's
first-use costs); per build torch.cuda.synchronize(), the call,
torch.cuda.synchronize(), host perf_counter around the pair; medians, with every
build's seconds kept (the spread).  FAMG_SA_LOG=1 is set for every build: the
per-level stage times, aggregates, partitioner rounds and passes are read from the
library's stderr.  Per configuration: PCG iterations to rel_tol 1e-8 for one
standard-normal right-hand side, and the operator complexity (sum of the levels'
nnz over the fine nnz).

The partitioner alone, on the level-0 graph amg_strength_graph_device leaves on the
device: amg_partition_modularity_device against amg_partition_modularity on the
downloaded copy of the same graph, alternated, median of `reps`.

BlockSmoother blocks: PCG (at most --block-iters iterations) preconditioned by one
BlockSmoother over a coarsening_factor-128 modularity partition of that graph against
one over its MIS aggregates: iterations, seconds, seconds per iteration.

The measurement runs in a fresh child process under its own `timeout` (the parent
never touches the GPU), and nothing is retried:

  python scripts/time_sa_partitioner.py [--elements 80] [--limit 900] [--out FILE]
"""
import argparse
import ctypes as C
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


def log(msg):
    print(f"[time_sa_partitioner] {msg}", file=sys.stderr, flush=True)


def child(elements, reps, block_iters):
    os.environ["FAMG_SA_LOG"] = "1"  # read once, at the first build
    import torch
    import faer_amg_amd as fa
    if not torch.cuda.is_available():
        sys.exit("time_sa_partitioner.py needs a GPU")
    ctx = fa.Context(0)
    t0 = time.perf_counter()
    A = fa.elasticity_q1((elements,) * 3, contrast=1.0, nu=0.3, seed=42, permute=4096).upload(ctx)
    n = A.nrows
    log(f"operator: {n} rows, {A.nnz} nnz, {time.perf_counter() - t0:.1f} s")
    nn = fa.constant_candidates(n, 3)
    b = torch.as_tensor(np.random.default_rng(7).standard_normal(n), device="cuda:0")

    def build(part, setup):
        fa.set_sa_partitioner(part)
        fa.set_sa_setup(setup)
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
                fa.set_sa_partitioner(0)
            tf.seek(0)
            levels, smoothers = parse_sa_log(tf.read().decode())
        return mg, t, levels, smoothers

    configs = [("mis", 0), ("mis", 1), ("modularity", 0), ("modularity", 1)]
    label = lambda c: f"{c[0]}/{'device' if c[1] else 'host'}"  # noqa: E731
    runs = {c: [] for c in configs}
    summary = {}
    for r in range(reps):
        for c in configs:
            mg, t, levels, smoothers = build(*c)
            log(f"build {r} {label(c)}: {t:.3f} s, {mg.levels()} levels")
            runs[c].append({"s": t, "levels": levels, "smoothers_ms": smoothers})
            if r == reps - 1:  # the hierarchy's own figures, then it is released
                x = torch.zeros_like(b)
                torch.cuda.synchronize()
                tp = time.perf_counter()
                it, _ = fa.pcg_solve(A, mg, b, x, max_iter=1000, rel_tol=1e-8)
                torch.cuda.synchronize()
                tp = time.perf_counter() - tp
                nnz = [mg.level(l)[0].nnz for l in range(mg.levels())]
                summary[c] = {"levels": mg.levels(), "pcg_iterations": int(it), "pcg_s": tp,
                              "operator_complexity": float(sum(nnz)) / nnz[0]}
            del mg
    res = {"device": torch.cuda.get_device_name(0), "elements": elements, "rows": n, "nnz": A.nnz,
           "method": "host perf_counter around each call between torch.cuda.synchronize(); the configurations "
                     "alternated in one process, MIS on the host first; median of %d with every run kept; "
                     "FAMG_SA_LOG=1 stage times" % reps,
           "builds": {}}
    for c in configs:
        rs = runs[c]
        lv = rs[-1]["levels"]
        stages = [{s: float(np.median([r["levels"][l][s] for r in rs])) for s in STAGES} for l in range(len(lv))]
        agg_runs = [float(sum(d["aggregation"] for d in r["levels"])) for r in rs]
        d = {"all_s": [r["s"] for r in rs], "median_s": float(np.median([r["s"] for r in rs])),
             "level_nodes": [d["nodes"] for d in lv], "aggregates": [d["aggregates"] for d in lv],
             "on_device": [d["device"] for d in lv], "passes": [d["passes"] for d in lv],
             "fallback": [d["fallback"] for d in lv],
             "aggregation_ms_all": agg_runs, "aggregation_ms_median": float(np.median(agg_runs)),
             "stage_ms": stages, "stage_total_ms": {s: float(sum(st[s] for st in stages)) for s in STAGES}}
        for key in ("rounds", "maxpasses", "improve", "swaps"):
            if key in lv[0]:
                d[key] = [x[key] for x in lv]
        d.update(summary[c])
        res["builds"][label(c)] = d

    # the partitioner alone on the level-0 device graph
    S = A.to_scipy()
    w = [1.0 / float(nn[:, c] @ (S @ nn[:, c])) for c in range(3)]
    del S
    Gd = fa.strength_graph_device(A, nn, w, block_size=3)
    Gs = Gd.to_scipy()
    Gh = fa.HostCsr(fa._host_csr_from_scipy(Gs))
    nodes = Gd.nrows
    vp = C.c_void_p

    def part_host(cfg):
        agg, na, info = np.zeros(nodes, np.int64), C.c_int64(), np.zeros(8, np.int64)
        t = time.perf_counter()
        fa._ck(fa.lib().amg_partition_modularity(Gh.h, C.byref(cfg), agg.ctypes.data_as(vp), C.byref(na),
                                                 info.ctypes.data_as(vp)))
        return time.perf_counter() - t, agg, na.value, info

    def part_dev(cfg):
        agg, na, info = np.zeros(nodes, np.int64), C.c_int64(), np.zeros(8, np.int64)
        torch.cuda.synchronize()
        t = time.perf_counter()
        fa._ck(fa.lib().amg_partition_modularity_device(Gd.h, C.byref(cfg), agg.ctypes.data_as(vp), C.byref(na),
                                                        info.ctypes.data_as(vp)))
        torch.cuda.synchronize()
        return time.perf_counter() - t, agg, na.value, info

    res["partitioner"] = {}
    part128 = None
    for cf in (8.0, 128.0):
        cfg = fa.PartitionerConfig(coarsening_factor=cf)
        th, td = [], []
        for r in range(reps):
            t, agg_h, na_h, ih = part_host(cfg)
            th.append(t)
            t, agg_d, na_d, idev = part_dev(cfg)
            td.append(t)
            log(f"partitioner cf {cf:g} rep {r}: host {th[-1]:.3f} s, device {td[-1]:.3f} s")
        res["partitioner"][f"cf{cf:g}"] = {
            "nodes": nodes, "edges": int(Gs.nnz), "aggregates": int(na_d),
            "equal": bool(na_h == na_d and np.array_equal(agg_h, agg_d)),
            "host_s_all": th, "host_s_median": float(np.median(th)),
            "device_s_all": td, "device_s_median": float(np.median(td)),
            "info_device": [int(v) for v in idev], "info_host": [int(v) for v in ih]}
        if cf == 128.0:
            part128 = (agg_d, na_d)

    # one BlockSmoother as the PCG preconditioner: cf-128 modularity blocks against MIS aggregates
    agg_m, na_m, _ = fa.aggregate_mis_device(Gd)
    res["block_smoother_pcg"] = {}
    for name, (agg, na) in (("mis", (agg_m, na_m)), ("modularity_cf128", part128)):
        blk = fa.BlockSmoother(A, agg, na, block_size=3)
        x = torch.zeros_like(b)
        torch.cuda.synchronize()
        t = time.perf_counter()
        it, hist = fa.pcg_solve(A, blk, b, x, max_iter=block_iters, rel_tol=1e-8)
        relres = hist[-1] if len(hist) else float("nan")  # the last recorded residual figure
        torch.cuda.synchronize()
        t = time.perf_counter() - t
        info = blk.info()
        res["block_smoother_pcg"][name] = {"blocks": int(na), "max_block_rows": int(info["max_block"]),
                                           "inverse_bytes": int(info["inverse_bytes"]), "iterations": int(it),
                                           "converged": bool(it < block_iters), "final": float(relres), "s": t,
                                           "s_per_iteration": t / max(int(it), 1)}
        log(f"block smoother pcg {name}: {it} iterations, {t:.3f} s")
        del blk
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=80, help="elements per edge (80: 1.57M rows)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--block-iters", type=int, default=2000)
    ap.add_argument("--limit", type=int, default=900, help="seconds (the child's timeout)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.elements, args.reps, args.block_iters)
        return
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child",
           "--elements", str(args.elements), "--reps", str(args.reps), "--block-iters", str(args.block_iters)]
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
