#!/usr/bin/env python3
"""Alignment statistics: the tiled pair kernel behind rnamsm_msa_neff against rnamsm_msa_weights, the one-block-per-row
kernel it shares its result with, at (N, L) = (1176, 36), (10000, 512) and (20000, 512), and rnamsm_msa_pdist at (8192, 512).  Wall
milliseconds between device synchronises, best of three after a warm-up, buffers allocated outside the timed region; the byte-compare
rate is N * N * L byte pairs per second for both (the tiled kernel runs only the tiles on or above the diagonal, so its executed
rate is about half of that).  The weights of the two routes are compared bit for bit.  Figures as measured, no bar, into
profiles/msa_stats_timing.json.

    python tools/msa_stats_timing.py [N,L ...]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rna-msm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch

import msa_stats_truth as T
from rnamsm import _lib, ops

shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or [(1176, 36), (10000, 512), (20000, 512)]
PDIST_SHAPE = (8192, 512)
dev = torch.device("cuda:0")
lib = _lib.load()
stream = lambda: torch.cuda.current_stream().cuda_stream      # noqa: E731
RUNS = 3


def best_ms(call):
    call()                                                  # warm-up: code objects
    torch.cuda.synchronize()
    times = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return min(times), times


res = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "cases": []}
for N, L in shapes:
    u8 = torch.from_numpy(T.alignment(N, L, N + L)).to(dev)
    ws = torch.empty(lib.rnamsm_msa_neff_workspace_bytes(N, L), dtype=torch.uint8, device=dev)
    nn = torch.empty(N, dtype=torch.int32, device=dev)
    w_new, w_old = torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.float64, device=dev)
    neff = torch.empty((), dtype=torch.float64, device=dev)
    new_ms, new_all = best_ms(lambda: _lib.check(lib.rnamsm_msa_neff(u8.data_ptr(), N, L, L, 0.2, nn.data_ptr(), w_new.data_ptr(), neff.data_ptr(),
                                                                    ws.data_ptr(), ws.numel(), stream())))
    old_ms, old_all = best_ms(lambda: _lib.check(lib.rnamsm_msa_weights(u8.data_ptr(), N, L, 0.2, w_old.data_ptr(), stream())))
    pairs = float(N) * N * L
    case = {"N": N, "L": L, "seqid_cutoff": 0.2,
            "msa_neff_ms": {"best": new_ms, "all": new_all}, "msa_weights_ms": {"best": old_ms, "all": old_all},
            "msa_neff_byte_compares_per_s": pairs / (new_ms * 1e-3), "msa_weights_byte_compares_per_s": pairs / (old_ms * 1e-3),
            "msa_weights_over_msa_neff": old_ms / new_ms, "weights_bit_equal": bool(torch.equal(w_new, w_old)),
            "neff": float(neff.item()), "workspace_mb": ws.numel() / 1e6,
            "bands": -(-(-(-N // 64)) // max(1, (ws.numel() - lib.rnamsm_msa_neff_min_workspace_bytes(N, L)) // (-(-N // 64) * 64 * 8) + 1))}
    res["cases"].append(case)
    print(json.dumps(case), flush=True)
    del ws

N, L = PDIST_SHAPE
u8 = torch.from_numpy(T.alignment(N, L, N + L)).to(dev)
ws = torch.empty(lib.rnamsm_msa_pdist_workspace_bytes(N, L), dtype=torch.uint8, device=dev)
dist = torch.empty((N, N), dtype=torch.float64, device=dev)
ms, all_ms = best_ms(lambda: _lib.check(lib.rnamsm_msa_pdist(u8.data_ptr(), N, L, L, None, dist.data_ptr(), ws.data_ptr(), ws.numel(), stream())))
res["pdist"] = {"N": N, "L": L, "output": "dist float64 [N, N]", "ms": {"best": ms, "all": all_ms},
                "byte_compares_per_s": float(N) * N * L / (ms * 1e-3), "output_gb_per_s": N * N * 8 / (ms * 1e-3) / 1e9,
                "exactly_symmetric": bool(torch.equal(dist, dist.T)), "zero_diagonal": not bool(dist.diagonal().any())}
print(json.dumps(res["pdist"]), flush=True)
out = os.path.join(ROOT, "profiles", "msa_stats_timing.json")
with open(out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(f"wrote {out}")
