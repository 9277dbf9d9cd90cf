#!/usr/bin/env python3
"""RNA-MSM-SS head, several structures per launch: wall time of ONE rnamsm_ss_head_packed call over B structures against B
sequential rnamsm_ss_head calls on the same inputs, same process, same device (16 blocks, random weights; both through the C
ABI on preallocated workspaces and outputs, so neither side pays for an allocation).  Median of --steps after --warmup; per
batch the ratio, the ms per structure and the model FLOPs (2.62 MFLOP per pixel) as a fraction of the 157.3 TF fp32 MFMA peak.
The outputs of the two paths are compared bit for bit on the way.  One JSON document on stdout (and to --out).

    python tools/ss_head_packed_timing.py --out profiles/ss_head_packed_timing.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ss_head_packed_timing.py --hip-only

--hip-only: one packed call per batch and nothing else (no lone calls, no timing loop), so that a kernel trace holds exactly
one launch set per batch and its grid sizes can be read off: sum_b ceil(L_b / 16)^2 blocks per convolution launch.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rna-msm_amd"), os.path.join(ROOT, "tests")]

import numpy as np      # noqa: E402
import torch            # noqa: E402

PEAK_TFLOPS = 157.3
# model FLOPs per pixel: stem 3x3 128 -> 48 (+ bias), 16 x (3x3 + 5x5, 48 -> 48), fc1 48 -> 1 (multiply-add = 2 FLOPs)
FLOP_PER_PIXEL = 2 * 9 * 128 * 48 + 16 * 2 * (9 + 25) * 48 * 48 + 2 * 48
NUM_BLOCKS = 16
MIXED_SEED, MIXED_B = 2024, 32


def batches():
    """(label, [L_b]): B = 16 and 64 at L = 35, 64, 128, 256, and one mixed batch with L drawn from 20..200 (fixed seed)."""
    out = [(f"B={B} L={L}", [L] * B) for L in (35, 64, 128, 256) for B in (16, 64)]
    rng = np.random.RandomState(MIXED_SEED)
    out.append((f"B={MIXED_B} L=20..200 (seed {MIXED_SEED})", [int(v) for v in rng.randint(20, 201, size=MIXED_B)]))
    return out


def wall_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from rnamsm import _lib, ss
    import ss_truth

    dev = torch.device("cuda:0")
    lib = _lib.load()
    model = ss.SSPredictor(NUM_BLOCKS)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in ss_truth.make_state(NUM_BLOCKS, seed=0).items()}, strict=True)
    model = model.eval().to(dev)
    ptrs, _ = model._packed_weights()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for label, Ls in batches():
        B = len(Ls)
        rng = np.random.RandomState(B * 1000 + Ls[0])
        atps, codes = [], []
        for L in Ls:
            a = torch.from_numpy(rng.rand(120, L, L).astype(np.float32)).to(dev)
            atps.append(a / a.sum(-1, keepdim=True))
            codes.append(torch.from_numpy(rng.randint(0, 4, size=L).astype(np.uint8)).to(dev))
        pixels = sum(L * L for L in Ls)
        tiles = sum(((L + 15) // 16) ** 2 for L in Ls)
        out_packed = torch.empty(pixels, device=dev)
        out_lone = torch.empty(pixels, device=dev)
        offs = np.concatenate([[0], np.cumsum([L * L for L in Ls])]).astype(np.int64)
        ws_packed = torch.empty(lib.rnamsm_ss_head_packed_workspace_bytes(B, (ctypes.c_int * B)(*Ls)), dtype=torch.uint8, device=dev)
        ws_lone = torch.empty(lib.rnamsm_ss_head_workspace_bytes(max(Ls)), dtype=torch.uint8, device=dev)
        items = (_lib.SsItem * B)()
        for b, L in enumerate(Ls):
            items[b] = _lib.SsItem(atps[b].data_ptr(), L * L, codes[b].data_ptr(), L, None, out_packed.data_ptr() + 4 * int(offs[b]))

        def packed():
            _lib.check(lib.rnamsm_ss_head_packed(items, B, NUM_BLOCKS, ptrs, ws_packed.data_ptr(), ws_packed.numel(), stream))

        def lone():
            for b, L in enumerate(Ls):
                _lib.check(lib.rnamsm_ss_head(atps[b].data_ptr(), L * L, codes[b].data_ptr(), L, NUM_BLOCKS, ptrs, None,
                                              out_lone.data_ptr() + 4 * int(offs[b]), ws_lone.data_ptr(), ws_lone.numel(), stream))

        row = {"batch": label, "B": B, "L_min": min(Ls), "L_max": max(Ls), "pixels": pixels, "blocks_per_conv_launch": tiles,
               "launches_packed": 2 + 2 * NUM_BLOCKS + (B + 31) // 32, "launches_sequential": B * (2 + 2 * NUM_BLOCKS)}
        if args.hip_only:
            packed()
            torch.cuda.synchronize()
        else:
            seq_ms, seq_min = wall_ms(lone, args.steps, args.warmup)
            pk_ms, pk_min = wall_ms(packed, args.steps, args.warmup)
            same = bool(torch.equal(out_packed.view(torch.int32), out_lone.view(torch.int32)))
            flops = FLOP_PER_PIXEL * pixels
            row.update(sequential_ms=seq_ms, sequential_ms_min=seq_min, packed_ms=pk_ms, packed_ms_min=pk_min,
                       speedup=seq_ms / pk_ms, sequential_ms_per_structure=seq_ms / B, packed_ms_per_structure=pk_ms / B,
                       sequential_frac_fp32_mfma_peak=flops / (seq_ms * 1e-3) / (PEAK_TFLOPS * 1e12),
                       packed_frac_fp32_mfma_peak=flops / (pk_ms * 1e-3) / (PEAK_TFLOPS * 1e12), bit_identical=same)
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    doc = {"what": "RNA-MSM-SS head, 16 blocks, fp32: one rnamsm_ss_head_packed call over B structures against B sequential "
                   "rnamsm_ss_head calls; wall time, median of `steps`",
           "device": torch.cuda.get_device_name(0), "flop_per_pixel": FLOP_PER_PIXEL, "peak_fp32_mfma_tflops": PEAK_TFLOPS,
           "steps": args.steps, "warmup": args.warmup, "rows": rows}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not args.hip_only and not all(r["bit_identical"] for r in rows):
        sys.exit("a packed batch's outputs differ from the lone calls'")


if __name__ == "__main__":
    main()
