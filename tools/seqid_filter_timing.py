#!/usr/bin/env python3
"""The identity redundancy filter: wall clock of the whole ops.seqid_filter call -- upload excluded, the order's sort,
the pack, every pass with its read-back and the finish included -- median of 7 after a warm-up, at N in {1000, 10 000, 100 000} x
L in {128, 1024}, with num_seqs = 0 (one pass at 90) and num_seqs = 512 (passes from 20 upward until 512 rows are kept).  Inputs:
synthetic mixtures with many near copies (tests/seqid_filter_truth.py: alignment, N / 50 founders, every row a founder with up to a
quarter of its columns redrawn).  Beside it the host implementation (rnamsm.msa.seqid_filter_host, once) where N * L <= 1.3 M, which
is where it finishes in under a minute, with its indices compared to the device's.  The kept count after every pass comes from
kept_at; launches = 3 + 2 * chunks * passes + 3.  Figures as measured, no bar, into profiles/seqid_filter_timing.json.

    python tools/seqid_filter_timing.py [--out FILE] [N,L ...]
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

import seqid_filter_truth as T
from rnamsm import msa, ops

args = sys.argv[1:]
out = os.path.join(ROOT, "profiles", "seqid_filter_timing.json")
if args[:1] == ["--out"]:
    out, args = args[1], args[2:]
shapes = [tuple(int(v) for v in a.split(",")) for a in args] or [(N, L) for N in (1000, 10000, 100000) for L in (128, 1024)]
dev = torch.device("cuda:0")
GAP, RUNS, HOST_MAX = 10, 7, 1300000

res = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "chunk": ops.get_param("seqid_filter_chunk"), "cases": []}
for N, L in shapes:
    a = T.alignment(N, L, N + L, families=max(1, N // 50))
    u8 = torch.from_numpy(a).to(dev)
    for num_seqs in (0, 512):
        rec = ops.seqid_filter(u8, GAP, num_seqs)            # warm-up: code objects, the allocator's blocks
        torch.cuda.synchronize()
        times = []
        for _ in range(RUNS):
            t0 = time.perf_counter()
            rec = ops.seqid_filter(u8, GAP, num_seqs)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        at = rec.kept_at.cpu().numpy()
        thresholds = msa.seqid_thresholds(num_seqs)
        if num_seqs > 0 and rec.indices.numel() >= num_seqs:     # stopped by the count: after the pass that kept the last row
            thresholds = thresholds[:thresholds.index(int(at.max())) + 1]
        chunks = -(-(-(-N // 64) * 64) // res["chunk"])
        case = {"N": N, "L": L, "num_seqs": num_seqs, "ms": {"median": statistics.median(times), "all": times},
                "kept": int(rec.indices.numel()), "passes": len(thresholds),
                "kept_after_pass": {str(t): int(((at >= 0) & (at <= t)).sum()) for t in thresholds},
                "launches": 6 + 2 * chunks * len(thresholds), "read_backs": len(thresholds)}
        if N * L <= HOST_MAX:
            t0 = time.perf_counter()
            hi, hat = msa.seqid_filter_host(a, GAP, num_seqs)
            case["host_s"] = time.perf_counter() - t0
            case["host_equal"] = bool(np.array_equal(hi, rec.indices.cpu().numpy()) and np.array_equal(hat, at))
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    del u8
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(f"wrote {out}")
