#!/usr/bin/env python3
"""Sequence-weighted mutual information (rnamsm_msa_wmi): the whole device call beside rnamsm_msa_mi at the same shape
(the integer popcount route a weighted count cannot use) and beside the same contraction as one torch.matmul of fp64 one-hot
matrices on the device, C = (Y * w)^T Y with Y [N, L * K], at N in {1 k, 10 k, 100 k} x L in {128, 512, 1024}, K = 4 ("pairwise"),
random A C G U with 5 % gaps, weights 1 / (1 .. 50).  msa_wmi is timed twice: the two maps (tiles below the diagonal skipped) and with
want_counts (every tile, the [L, L, 4, 4] counts written), which is the work the matmul does (that call also
counts K with torch.unique to size the counts: one more pass over the tokens and one more wait, inside its time).  The achieved rate counts the fp64
MFMA work issued, 2 * 64 * 64 * (N rounded up to the planes' 1024 rows) per tile, over the WHOLE call (stage 1, the pair kernel, the
correction, the workspace allocation and the one wait included), so it understates the kernel.  Median of 7 after a warm-up;
figures as measured, no bar, into profiles/wmi_timing.json.

    python tools/wmi_timing.py [N,L ...]
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rna-msm_amd"))

import torch

from rnamsm import _lib, ops

shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or [(N, L) for N in (1000, 10000, 100000) for L in (128, 512, 1024)]
dev = torch.device("cuda:0")
RUNS, GAP, K = 7, 10, 4


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


res = {"device": torch.cuda.get_device_name(0), "device_ms_include": "workspace allocation and the one wait for K", "cases": []}
for N, L in shapes:
    gen = torch.Generator(device=dev).manual_seed(N + L)
    u8 = torch.randint(4, 4 + K, (N, L), generator=gen, device=dev, dtype=torch.uint8)
    u8[torch.rand((N, L), generator=gen, device=dev) < 0.05] = GAP
    w = 1.0 / torch.randint(1, 51, (N,), generator=gen, device=dev).to(torch.float64)
    case = {"N": N, "L": L, "K": K}
    _, case["msa_mi_ms"] = timed(lambda: ops.msa_mi(u8, GAP))
    rec, case["msa_wmi_ms"] = timed(lambda: ops.msa_wmi(u8, GAP, "pairwise", w))
    full, case["msa_wmi_counts_ms"] = timed(lambda: ops.msa_wmi(u8, GAP, "pairwise", w, want_counts=True))

    def matmul():
        Y = (u8[:, :, None] == torch.arange(4, 4 + K, device=dev, dtype=torch.uint8)).to(torch.float64).reshape(N, L * K)
        return Y, (Y * w[:, None]).T @ Y

    (Y, _), case["matmul_with_one_hot_ms"] = timed(matmul)
    Yw = (Y * w[:, None]).T.contiguous()
    C, case["matmul_alone_ms"] = timed(lambda: Yw @ Y)
    got = full.wcounts.permute(0, 2, 1, 3).reshape(L * K, L * K)
    case["counts_distance_from_matmul_over_N_eps"] = float(((got - C).abs() / C.clamp_min(1e-300)).max() / (N * 2.0 ** -52))
    case["same_maps_both_routes"] = bool(torch.equal(rec.mi, full.mi))
    tiles = -(-L * K // 64)
    rows = -(-N // 1024) * 1024
    for key, n_tiles in (("msa_wmi_ms", tiles * (tiles + 1) // 2), ("msa_wmi_counts_ms", tiles * tiles)):
        case[key]["tflops_fp64_mfma_issued_over_whole_call"] = 2.0 * 64 * 64 * rows * n_tiles / (case[key]["median"] * 1e-3) / 1e12
    case["matmul_alone_ms"]["tflops"] = 2.0 * N * (L * K) ** 2 / (case["matmul_alone_ms"]["median"] * 1e-3) / 1e12
    case["workspace_mb"] = _lib.load().rnamsm_msa_wmi_workspace_bytes(N, L) / 1e6
    res["cases"].append(case)
    print(json.dumps(case), flush=True)
    del Y, Yw, C, full, rec, got
out = os.path.join(ROOT, "profiles", "wmi_timing.json")
with open(out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(f"wrote {out}")
