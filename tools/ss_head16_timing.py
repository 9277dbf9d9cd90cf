#!/usr/bin/env python3
"""RNA-MSM-SS head, bf16 mode beside fp32: ms per call of rnamsm_ss_head16 and of rnamsm_ss_head in the same process and session
(16 blocks, random weights, the same maps), median of --steps calls, one structure per call at --sizes and one packed call of
--packed-batch structures of L = --packed-L.  Per row: the ratio fp32 / bf16, the run-to-run spread of each head ((max - min) /
median of its calls), whether the bf16 head is faster by more than that spread, and the bf16 head's model FLOPs as a fraction of the
2500 TF bf16 MFMA peak and its time as a multiple of its byte floor (the bytes every launch must move at 6.3 TB/s: the fp32 maps in,
the two fp32 images read and written by every conv, the result out).  One JSON document on stdout (and to --out).

    python tools/ss_head16_timing.py --out profiles/ss_head16_timing.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rna-msm_amd"), os.path.join(ROOT, "tests")]

import numpy as np      # noqa: E402
import torch            # noqa: E402

PEAK_BF16_TFLOPS, PEAK_FP32_TFLOPS, HBM_TBPS = 2500.0, 157.3, 6.3
NUM_BLOCKS = 16
# model FLOPs per pixel: stem 3x3 128 -> 48 (+ bias), 16 x (3x3 + 5x5, 48 -> 48), fc1 48 -> 1 (multiply-add = 2 FLOPs)
FLOP_PER_PIXEL = 2 * 9 * 128 * 48 + NUM_BLOCKS * 2 * (9 + 25) * 48 * 48 + 2 * 48
# bytes per pixel: stem 120 maps in + x out; per block 3x3: x in, t out; 5x5: t in, x in and out; output pass: x in, one float out
BYTES_PER_PIXEL = 4 * (120 + 48 + NUM_BLOCKS * 5 * 48 + 48 + 1)


def gpu_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    med = float(np.median(ms))
    return med, float(min(ms)), float((max(ms) - min(ms)) / med)


def row_of(label, pixels, f32, b16):
    (m32, lo32, sp32), (m16, lo16, sp16) = f32, b16
    flops = FLOP_PER_PIXEL * pixels
    floor_ms = BYTES_PER_PIXEL * pixels / (HBM_TBPS * 1e12) * 1e3
    return dict(label, f32_ms=m32, f32_ms_min=lo32, f32_spread=sp32, bf16_ms=m16, bf16_ms_min=lo16, bf16_spread=sp16,
                ratio_f32_over_bf16=m32 / m16, faster_beyond_spread=bool(m16 * (1 + max(sp32, sp16)) < m32),
                bf16_frac_bf16_mfma_peak=flops / (m16 * 1e-3) / (PEAK_BF16_TFLOPS * 1e12),
                f32_frac_fp32_mfma_peak=flops / (m32 * 1e-3) / (PEAK_FP32_TFLOPS * 1e12),
                byte_floor_ms=floor_ms, bf16_over_byte_floor=m16 / floor_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,512,1024")
    ap.add_argument("--packed-batch", type=int, default=64)
    ap.add_argument("--packed-L", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from rnamsm import ss
    import ss_truth

    dev = torch.device("cuda:0")
    state = ss_truth.make_state(NUM_BLOCKS, seed=0)
    heads = {}
    for mode in ("f32", "bf16"):
        m = ss.SSPredictor(NUM_BLOCKS, gemm_dtype=mode)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
        heads[mode] = m.eval().to(dev)

    def maps(L, seed):
        rng = np.random.RandomState(seed)
        atp = rng.rand(120, L, L).astype(np.float32)
        atp /= atp.sum(-1, keepdims=True)
        codes = ss.base_codes("".join(rng.choice(list("ACGU"), L)))
        return torch.from_numpy(atp).to(dev), torch.from_numpy(codes).to(dev)

    rows = []
    for L in [int(s) for s in args.sizes.split(",") if s]:
        a, codes = maps(L, L)
        t = {mode: gpu_ms(lambda: heads[mode].predict(a, codes), args.steps, args.warmup) for mode in ("f32", "bf16")}
        rows.append(row_of({"case": "lone", "L": L}, L * L, t["f32"], t["bf16"]))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    if args.packed_batch:
        B, L = args.packed_batch, args.packed_L
        members = [maps(L, 1000 + b) for b in range(B)]
        atps, codes = [m[0] for m in members], [m[1] for m in members]
        t = {mode: gpu_ms(lambda: heads[mode].predict_many(atps, codes), args.steps, args.warmup) for mode in ("f32", "bf16")}
        rows.append(row_of({"case": "packed", "B": B, "L": L}, B * L * L, t["f32"], t["bf16"]))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    doc = {"what": "RNA-MSM-SS head, 16 blocks: rnamsm_ss_head16 (bf16 operands, fp32 accumulation) beside rnamsm_ss_head (fp32), one session",
           "device": torch.cuda.get_device_name(0), "flop_per_pixel": FLOP_PER_PIXEL, "bytes_per_pixel": BYTES_PER_PIXEL,
           "peak_bf16_mfma_tflops": PEAK_BF16_TFLOPS, "peak_fp32_mfma_tflops": PEAK_FP32_TFLOPS, "hbm_tbps": HBM_TBPS,
           "steps": args.steps, "rows": rows}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
