#!/usr/bin/env python3
"""A pair map against a target on the device (rnamsm_pair_sweep_f32, rnamsm_pair_precision_f32) over a grid: L in {128, 512,
1024, 4096} on a random float32 map and on an all-zero one (an SS probability map is almost all ~0: every candidate in one bin).  Per cell:
  sweep_ms          ops.pair_sweep with the 1001 thresholds as a SweepTable (workspace and output allocation included; nothing read back)
  precision_ms      ops.pair_precision with k = L and the reference's ten cuts (the masked copy, the 20 launches of the selection, the scan)
  host_hist_ms      the map's and the target's copy to the host plus tests/pair_metrics_truth.sweep_hist (searchsorted + bincount)
  host_broadcast_ms the same with the reference's n x 1001 broadcast (sweep_broadcast), up to L = 1024: at 4096 it is 8.4 M x 1001 booleans
  host_precision_ms the copies plus precision_ranked (a lexsort of every candidate)
The device's integers are checked against the histogram truth in every cell.  Into profiles/pair_metrics_timing.json (or argv[1]).

    python tools/pair_metrics_timing.py [out.json]
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rna-msm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import pair_metrics_truth as T
from rnamsm import metrics, ops

dev = torch.device("cuda:0")
RUNS, HOST_RUNS = 10, 2
TH = metrics.sweep_thresholds()


def timed(fn, runs):
    fn()                                                        # warm-up: code objects, the allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return got, {"best": min(times), "median": statistics.median(times), "runs": runs}


table = ops.sweep_table(TH, dev)
res = {"device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "min_sep": 1, "dtype": "float32", "T": len(TH),
       "cases": []}
for L in (128, 512, 1024, 4096):
    rng = np.random.default_rng(L)
    t = (rng.random((L, L)) < 0.01).astype(np.int8)
    td = torch.from_numpy(t).to(dev)
    cuts = metrics.precision_cuts(L)
    for kind in ("random", "zeros"):
        x = rng.random((L, L), dtype=np.float32) if kind == "random" else np.zeros((L, L), dtype=np.float32)
        xd = torch.from_numpy(x).to(dev)
        counts, sweep = timed(lambda: ops.pair_sweep(xd, td, table, 1), RUNS)
        prec, precision = timed(lambda: ops.pair_precision(xd, td, L, cuts, 1), RUNS)
        want, host_hist = timed(lambda: T.sweep_hist(xd.cpu().numpy(), td.cpu().numpy(), TH, 1), HOST_RUNS)
        want_p, host_prec = timed(lambda: T.precision_ranked(xd.cpu().numpy(), td.cpu().numpy(), L, cuts, 1), HOST_RUNS)
        case = {"L": L, "map": kind, "candidates": L * (L - 1) // 2, "sweep_ms": sweep, "precision_ms": precision, "host_hist_ms": host_hist,
                "host_precision_ms": host_prec,
                "sweep_equals_the_rule": bool(np.array_equal(counts.cpu().numpy(), want)),
                "precision_equals_the_rule": bool(np.array_equal(prec.hits.cpu().numpy(), want_p[0]) and int(prec.count) == want_p[1]),
                "host_hist_over_sweep": host_hist["median"] / sweep["median"], "host_precision_over_precision": host_prec["median"] / precision["median"]}
        if L <= 1024:
            _, host_b = timed(lambda: T.sweep_broadcast(xd.cpu().numpy(), td.cpu().numpy(), TH, 1), HOST_RUNS)
            case["host_broadcast_ms"] = host_b
            case["host_broadcast_over_sweep"] = host_b["median"] / sweep["median"]
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pair_metrics_timing.json")
with open(out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(f"wrote {out}")
