#!/usr/bin/env python3
"""RNA-MSM-SS head timing: ms per structure of the HIP head (rnamsm_ss_head, 16 blocks, random weights), its model FLOPs as a
fraction of the 157.3 TF fp32 MFMA peak, the same network in PyTorch eager fp32 on the same device (the reference's
`--device cuda`: MIOpen convolutions plus the NCHW <-> NHWC permutes around every LayerNorm, tests/ss_truth.py), and CPU torch
at the sizes given by --cpu-sizes with the thread count stated.  One JSON document on stdout (and to --out).

    python tools/ss_head_timing.py --out profiles/ss_head_timing.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ss_head_timing.py --hip-only --sizes 512
"""
import argparse
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
    return float(np.median(ms)), float(min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,512,1024")
    ap.add_argument("--cpu-sizes", default="128,512")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from rnamsm import ss
    import ss_truth

    torch.set_num_threads(args.threads)
    dev = torch.device("cuda:0")
    state = ss_truth.make_state(16, seed=0)
    model = ss.SSPredictor(16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    model = model.eval().to(dev)
    rows = []
    for L in [int(s) for s in args.sizes.split(",") if s]:
        rng = np.random.RandomState(L)
        atp = rng.rand(120, L, L).astype(np.float32)
        atp /= atp.sum(-1, keepdims=True)
        seq = "".join(rng.choice(list("ACGU"), L))
        a = torch.from_numpy(atp).to(dev)
        codes = torch.from_numpy(ss.base_codes(seq)).to(dev)
        flops = FLOP_PER_PIXEL * L * L
        med, best = gpu_ms(lambda: model.predict(a, codes), args.steps, args.warmup)
        row = {"L": L, "hip_ms": med, "hip_ms_min": best, "model_gflop": flops / 1e9,
               "hip_frac_fp32_mfma_peak": flops / (med * 1e-3) / (PEAK_TFLOPS * 1e12)}
        if not args.hip_only:
            x = ss_truth.features(atp, seq)
            sd = {k: torch.from_numpy(v).to(dev) for k, v in state.items()}
            xt = torch.from_numpy(x).to(dev, torch.float32)
            with torch.no_grad():
                tmed, _ = gpu_ms(lambda: ss_truth.logits(xt, sd, torch.float32, dev), max(3, args.steps // 2), 1)
            row.update(torch_eager_gpu_ms=tmed, speedup_vs_torch_eager=tmed / med)
            if str(L) in args.cpu_sizes.split(","):
                t0 = time.perf_counter()
                with torch.no_grad():
                    ss_truth.logits(x, state, torch.float32, "cpu")
                row.update(torch_cpu_ms=(time.perf_counter() - t0) * 1e3, torch_cpu_threads=torch.get_num_threads())
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    doc = {"what": "RNA-MSM-SS head, 16 blocks, one structure per call, fp32", "device": torch.cuda.get_device_name(0),
           "flop_per_pixel": FLOP_PER_PIXEL, "peak_fp32_mfma_tflops": PEAK_TFLOPS, "steps": args.steps, "rows": rows}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
