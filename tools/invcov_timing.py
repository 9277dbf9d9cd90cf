#!/usr/bin/env python3
"""Covariance contacts (rnamsm_msa_invcov): the device against the numpy restatement of the reference's MSA.invcov
(tests/invcov_truth.invcov: one-hot, np.cov, numpy's SVD norm) at (N, L) = (1024, 512) and (20000, 512), alignments of A C G U and
gaps drawn around two founder sequences.  Figures as measured, no bar, into profiles/invcov_timing.json.

    python tools/invcov_timing.py [N,L ...]
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
from rnamsm import _lib, ops

shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or [(1024, 512), (20000, 512)]
dev = torch.device("cuda:0")
RUNS = 5
res = {"device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "cases": []}
for N, L in shapes:
    t = T.mixture_alignment(seed=N + L, N=N, L=L)
    u8 = torch.from_numpy(t).to(dev)
    ops.msa_invcov(u8, T.GAP)                                   # warm-up: code objects, the allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        got = ops.msa_invcov(u8, T.GAP)
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    t0 = time.perf_counter()
    want = T.invcov(t)
    host_s = time.perf_counter() - t0
    got = got.cpu().numpy()
    K = len(T.symbols(t))
    words = -(-N // 64)
    case = {"N": N, "L": L, "K": K,
            "device_ms": {"best": min(times), "median": statistics.median(times), "runs": RUNS,
                          "includes": "workspace allocation and the one wait for K"},
            "numpy_restatement_s": host_s,
            "speedup_over_numpy": host_s * 1e3 / statistics.median(times),
            "and_popcount_word_ops": L * L * K * K * words,
            "max_abs_distance_over_largest_entry": float(np.abs(got - want).max() / want.max()),
            "exactly_symmetric": bool(np.array_equal(got, got.T)),
            "workspace_mb": _lib.load().rnamsm_msa_invcov_workspace_bytes(N, L) / 1e6}
    res["cases"].append(case)
    print(json.dumps(case), flush=True)
out = os.path.join(ROOT, "profiles", "invcov_timing.json")
with open(out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(f"wrote {out}")
