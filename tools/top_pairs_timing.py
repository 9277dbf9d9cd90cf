#!/usr/bin/env python3
"""The top-k ranked pairs on the device (rnamsm_top_pairs_f64) over a grid: L in {128, 512, 1024, 4096}, k in {L/2, L, 2L,
65536}, min_sep 1, a random float64 map and an all-zero map (every candidate a tie: the worst case for the tie pass).  Three columns
per cell, as measured, no bar:
  device_ms      ops.top_pairs on the map where it lies (workspace and output allocation included; nothing is read back)
  host_ms        what a user had before: the map's copy to the host plus the numpy statement of the rule (tests/top_pairs_truth.py:
                 mask, key, one lexsort of every candidate); it does not depend on k and is measured once per map
  topk_ms        for reference only: torch.topk on the device over the masked, flattened map (mask prebuilt).  It has no defined order
                 among equal scores, so it is never a substitute; on the random map its pairs are compared with the rule's.
Also the bytes one select pass streams (the candidates of the upper triangle) and the time nine such passes -- eight digits and the
count -- take at 6.3 TB/s.  The device's output is checked against the numpy statement in every cell.  Into profiles/top_pairs_timing.json
(or the path given).

    python tools/top_pairs_timing.py [out.json]
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

import top_pairs_truth as T
from rnamsm import ops

dev = torch.device("cuda:0")
RUNS, HOST_RUNS, HBM_TBPS, PASSES = 10, 2, 6.3, 9


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


res = {"device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "min_sep": 1, "dtype": "float64",
       "hbm_tbps_assumed": HBM_TBPS, "select_passes": PASSES, "cases": []}
for L in (128, 512, 1024, 4096):
    mask = torch.ones(L, L, dtype=torch.bool, device=dev).triu(1)
    for kind in ("random", "zeros"):
        x = np.random.default_rng(L).standard_normal((L, L)) if kind == "random" else np.zeros((L, L))
        xd = torch.from_numpy(x).to(dev)
        ranked, host = timed(lambda: T.ranked(xd.cpu().numpy(), 1), HOST_RUNS)
        cand = L * (L - 1) // 2
        pass_bytes = 8 * cand
        for k in sorted({L // 2, L, 2 * L, 65536}):
            rec, device = timed(lambda: ops.top_pairs(xd, k, 1), RUNS)
            want_p, want_s, n = T.padded(ranked[0], ranked[1], k)
            exact = bool(int(rec.count) == n and np.array_equal(rec.pairs.cpu().numpy(), want_p)
                         and rec.scores.cpu().numpy().tobytes() == want_s.tobytes())
            kk = min(k, L * L)
            top, topk = timed(lambda: torch.where(mask, xd, float("-inf")).flatten().topk(kk), RUNS)
            idx = top.indices[:n].cpu().numpy()
            same_pairs = bool(np.array_equal(np.stack([idx // L, idx % L], 1), want_p[:n]))
            case = {"L": L, "map": kind, "k": k, "count": n, "candidates": cand, "device_ms": device, "host_ms": host, "topk_ms": topk,
                    "device_equals_the_rule": exact, "topk_pairs_equal_the_rule": same_pairs,
                    "host_over_device": host["median"] / device["median"], "topk_over_device": topk["median"] / device["median"],
                    "pass_bytes": pass_bytes, "hbm_floor_ms_of_the_passes": 1e3 * PASSES * pass_bytes / (HBM_TBPS * 1e12)}
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "top_pairs_timing.json")
with open(out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(f"wrote {out}")
