#!/usr/bin/env python3
"""The RSA_result tables, host against device: per alignment, K = 3 members, seeded values, the median of `--steps` after a warm-up
(and the spread, min .. max) of
  (a) the host path -- rsa.write_rsa_files: the float64 scaling, K + 1 string tables through np.char.mod and np.savetxt -- what the
      CLI's writer thread did for every alignment;
  (b) the device path -- the formatter (rnamsm_rsa_text, HIP events), the copies of the text, the counts and the ensemble into
      pinned memory, and write_rsa_files(text=...): K + 1 headers and binary writes, the directories included.
The files of (a) and (b) are compared on every size.  A packed batch of 64 alignments of L = 64 is timed the same way, per alignment
(one rnamsm_rsa_text_packed call for the 64).  One JSON document on stdout (and to --out).

    python tools/rsa_text_timing.py --out profiles/rsa_text_timing.json
"""
import argparse
import json
import os
import random
import shutil
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
    return ms


def host_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return ms


def stat(ms, per=1):
    return {"median": float(np.median(ms)) / per, "min": float(np.min(ms)) / per, "max": float(np.max(ms)) / per}


def tree(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="35,128,512,1024")
    ap.add_argument("--models", type=int, default=3)
    ap.add_argument("--batch", default="64x64", help="members x L of the packed batch")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from rnamsm import ops, rsa
    from rnamsm.ss import letter_codes

    dev = torch.device("cuda:0")
    K = args.models
    names = [f"model_pcc_{k}.pt" for k in range(K)]
    scratch = tempfile.mkdtemp(prefix="rnamsm_rsa_text_")
    host_dir, dev_dir = os.path.join(scratch, "host"), os.path.join(scratch, "device")

    def case(L, seed):
        rng = np.random.RandomState(seed)
        return rng.uniform(0.01, 0.99, size=(K, L)).astype(np.float32), "".join(rng.choice(list("ACGU"), L))

    def measure(members, label):
        """members: [(values, seq)] of one formatter call; every figure per alignment."""
        B = len(members)
        ids = [f"x{b}" for b in range(B)]
        draws = random.Random(2022)

        def host_all():
            for i, (v, s) in zip(ids, members):
                rsa.write_rsa_files(v, s, i, host_dir, names, draws)

        host = host_ms(host_all, args.steps, args.warmup)
        vals = [torch.from_numpy(v).to(dev) for v, _ in members]
        lets = [torch.from_numpy(letter_codes(s)).to(dev) for _, s in members]
        run = (lambda: ops.rsa_text(vals[0], lets[0])) if B == 1 else (lambda: ops.rsa_text_packed(vals, lets))
        kernel = gpu_ms(run, args.steps, args.warmup)
        outs = [run()] if B == 1 else run()
        pins = [[torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in o] for o in outs]

        def copies():
            for ps, o in zip(pins, outs):
                for p, t in zip(ps, o):
                    p.copy_(t, non_blocking=True)

        copy = gpu_ms(copies, args.steps, args.warmup)
        torch.cuda.synchronize()
        records = [tuple(p.numpy() for p in ps) for ps in pins]
        assert all(int(r[1][K + 1]) == 0 and int(r[1][K + 2]) == 0 for r in records)

        def device_all():
            for i, (v, s), r in zip(ids, members, records):
                rsa.write_rsa_files(v, s, i, dev_dir, names, draws, text=r)

        writes = host_ms(device_all, args.steps, args.warmup)
        same = tree(host_dir) == tree(dev_dir) and len(tree(host_dir)) >= B * (K + 1)
        a, b = stat(host, B), {k: stat(kernel, B)[k] + stat(copy, B)[k] + stat(writes, B)[k] for k in ("median", "min", "max")}
        row = {"case": label, "members": B, "L": members[0][0].shape[1], "K": K, "same_files": same, "host_path_ms": a,
               "kernel_ms": stat(kernel, B), "copies_ms": stat(copy, B), "header_and_binary_writes_ms": stat(writes, B),
               "device_path_ms": b, "writer_thread_ms": {"before": a["median"], "after": stat(writes, B)["median"]},
               "host_over_device": a["median"] / b["median"]}
        print(json.dumps(row), file=sys.stderr, flush=True)
        return row

    rows = [measure([case(L, L)], f"lone L={L}") for L in (int(v) for v in args.sizes.split(","))]
    nb, lb = (int(v) for v in args.batch.split("x"))
    rows.append(measure([case(lb, 7000 + b) for b in range(nb)], f"packed {nb} x L={lb}, per alignment"))
    shutil.rmtree(scratch)
    doc = {"what": "RSA_result tables: write_rsa_files on the host against rnamsm_rsa_text + three small copies + K + 1 headers and "
                   "binary writes; ms per alignment, median (min .. max) of `steps`",
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "bars": {"writer_thread_time_falls": all(r["writer_thread_ms"]["after"] < r["writer_thread_ms"]["before"] for r in rows),
                    "same_files": all(r["same_files"] for r in rows)},
           "rows": rows}
    out = json.dumps(doc, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
