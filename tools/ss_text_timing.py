#!/usr/bin/env python3
"""The `.prob` text of the SS head, host against device: at each L, the median of `--steps` after a warm-up of
  (a) np.savetxt(path, probs, delimiter="\\t") on the host -- what the CLI's writer thread did for every structure;
  (b) the formatter kernel (rnamsm_ss_prob_text, HIP events), the device-to-host copy of its text into pinned memory and the one
      binary write of it -- the writer thread's share is the write, the copy runs on the side stream;
  (c) the SS head itself (16 blocks, random weights) at the same L, in the same run.
The kernel moves 29 bytes per element (4 read, 25 written); its GB/s is reported beside its share of the head.  The bytes of (a)
and (b) are compared on every size.  One JSON document on stdout (and to --out).

    python tools/ss_text_timing.py --out profiles/ss_text_timing.json
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rna-msm_amd"), os.path.join(ROOT, "tests")]

import numpy as np      # noqa: E402
import torch            # noqa: E402


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
    return float(np.median(ms))


def host_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="35,128,512,1024")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from rnamsm import ops, ss
    import ss_truth

    dev = torch.device("cuda:0")
    model = ss.SSPredictor(16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in ss_truth.make_state(16, seed=0).items()}, strict=True)
    model = model.eval().to(dev)
    scratch = tempfile.mkdtemp(prefix="rnamsm_ss_text_")
    path = os.path.join(scratch, "x.prob")
    rows = []
    for L in (int(v) for v in args.sizes.split(",")):
        rng = np.random.RandomState(L)
        atp = rng.exponential(size=(120, L, L)).astype(np.float32)
        atp /= atp.sum(-1, keepdims=True)
        atp = torch.from_numpy(atp).to(dev)
        seq = "".join(rng.choice(list("ACGU"), L))
        probs = model.predict(atp, seq)
        head = gpu_ms(lambda: model.predict(atp, seq), args.steps, args.warmup)
        kernel = gpu_ms(lambda: ops.ss_prob_text(probs), args.steps, args.warmup)
        text, word = ops.ss_prob_text(probs)
        assert int(word.item()) == 0
        pinned = torch.empty(text.shape, dtype=torch.uint8, pin_memory=True)
        copy = gpu_ms(lambda: pinned.copy_(text, non_blocking=True), args.steps, args.warmup)
        torch.cuda.synchronize()
        host_text = pinned.numpy()

        def write():
            with open(path, "wb") as f:
                f.write(memoryview(host_text))

        wr = host_ms(write, args.steps, args.warmup)
        device_bytes = open(path, "rb").read()
        prob = probs.cpu().numpy()
        savetxt = host_ms(lambda: np.savetxt(path, prob, delimiter="\t"), args.steps, 1)
        same = open(path, "rb").read() == device_bytes
        row = {"L": L, "text_bytes": len(device_bytes), "same_bytes": same, "savetxt_ms": savetxt, "kernel_ms": kernel,
               "copy_ms": copy, "write_ms": wr, "head_ms": head, "copy_plus_write_ms": copy + wr,
               "savetxt_over_copy_plus_write": savetxt / (copy + wr), "kernel_over_head": kernel / head,
               "kernel_GBps": 29.0 * L * L / (kernel * 1e-3) / 1e9}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    os.remove(path)
    os.rmdir(scratch)
    doc = {"what": "SS head .prob text: np.savetxt on the host against rnamsm_ss_prob_text + copy + one binary write; median of `steps`",
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "bytes_per_element_moved": 29,
           "bars": {"copy_plus_write_below_savetxt": all(r["copy_plus_write_ms"] < r["savetxt_ms"] for r in rows),
                    "kernel_at_most_5_percent_of_head_at_512_and_1024": all(r["kernel_over_head"] <= 0.05 for r in rows if r["L"] in (512, 1024)),
                    "same_bytes": all(r["same_bytes"] for r in rows)},
           "rows": rows}
    out = json.dumps(doc, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
