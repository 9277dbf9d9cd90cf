#!/usr/bin/env python3
"""Mutual-information contacts (rnamsm_msa_mi): the whole device call in both gap modes, rnamsm_msa_invcov on the same
input in the same process (it shares stage 1), and the numpy restatement (tests/mi_truth.mi_ratio_of over counts from a float64
matrix product of the one-hot, exact for these counts, and apc_numpy), at (N, L) = (1024, 512) and (20000, 512), alignments of
A C G U and gaps drawn around two founder sequences.  The device's output is checked against the restatement at each point.
Median of 5 after a warm-up; figures as measured, no bar, into profiles/mi_timing.json.

    python tools/mi_timing.py [N,L ...]
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

import invcov_truth as T
import mi_truth as M
from rnamsm import _lib, ops

shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or [(1024, 512), (20000, 512)]
dev = torch.device("cuda:0")
RUNS = 5


def timed(fn):
    fn()                                                        # warm-up: code objects, the allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return got, {"best": min(times), "median": statistics.median(times), "runs": RUNS}


res = {"device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(),
       "device_ms_include": "workspace allocation and the one wait for K", "cases": []}
for N, L in shapes:
    t = T.mixture_alignment(seed=N + L, N=N, L=L)
    u8 = torch.from_numpy(t).to(dev)
    K = len(T.symbols(t))
    case = {"N": N, "L": L, "K": K, "msa_mi_ms": {}, "numpy_restatement_s": {}, "mi_distance_over_largest_entry": {},
            "mip_distance_over_largest_entry": {}, "exactly_symmetric": {}}
    _, case["msa_invcov_ms"] = timed(lambda: ops.msa_invcov(u8, T.GAP))
    t0 = time.perf_counter()
    flat = (t[:, :, None] == T.symbols(t)[None, None, :]).astype(np.float64).reshape(N, L * K)
    counts = (flat.T @ flat).reshape(L, K, L, K).transpose(0, 2, 1, 3)
    counts_s = time.perf_counter() - t0
    for mode in M.MODES:
        rec, case["msa_mi_ms"][mode] = timed(lambda: ops.msa_mi(u8, T.GAP, gaps=mode))
        t0 = time.perf_counter()
        want = M.mi_ratio_of(M.tables_from_counts(counts, N, mode))
        want_p = M.apc_numpy(M.zero_diagonal(want))
        case["numpy_restatement_s"][mode] = counts_s + time.perf_counter() - t0
        mi, mip = rec.mi.cpu().numpy(), rec.mip.cpu().numpy()
        case["mi_distance_over_largest_entry"][mode] = float(np.abs(mi - want).max() / want.max())
        case["mip_distance_over_largest_entry"][mode] = float(np.abs(mip - want_p).max() / np.abs(want_p).max())
        case["exactly_symmetric"][mode] = bool(np.array_equal(mi, mi.T))
    case["speedup_over_numpy"] = {m: case["numpy_restatement_s"][m] * 1e3 / case["msa_mi_ms"][m]["median"] for m in M.MODES}
    case["workspace_mb"] = _lib.load().rnamsm_msa_mi_workspace_bytes(N, L) / 1e6
    res["cases"].append(case)
    print(json.dumps(case), flush=True)
out = os.path.join(ROOT, "profiles", "mi_timing.json")
with open(out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(f"wrote {out}")
