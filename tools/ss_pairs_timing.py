#!/usr/bin/env python3
"""The predicted structure of the SS head, host against device: at each L, on the head's own output for seeded maps, the median of
`--steps` after a warm-up of
  (a) the host path -- the device-to-host copy of the [L, L] probabilities into pinned memory, ss.secondary_structure, and the two
      np.savetxt tables (`.ct`, `.bpseq`) -- what the CLI's writer thread did for every structure;
  (b) the device path -- the decoding kernel (rnamsm_ss_pairs, HIP events), the copies of the partner vector, the counts and the two
      bodies into pinned memory, and the two binary writes;
  (c) the SS head itself (16 blocks, random weights) at the same L, in the same run.
The files of (a) and (b) are compared on every size.  The all-0.9 matrix at L = 1024 (1022 rounds: the bound on adversarial input) is
timed separately, kernel only.  One JSON document on stdout (and to --out).

    python tools/ss_pairs_timing.py --out profiles/ss_pairs_timing.json
"""
import argparse
import json
import os
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
    scratch = tempfile.mkdtemp(prefix="rnamsm_ss_pairs_")
    host_dir, dev_dir = os.path.join(scratch, "host"), os.path.join(scratch, "device")
    os.makedirs(host_dir)
    os.makedirs(dev_dir)
    rows = []
    for L in (int(v) for v in args.sizes.split(",")):
        rng = np.random.RandomState(L)
        atp = rng.exponential(size=(120, L, L)).astype(np.float32)
        atp /= atp.sum(-1, keepdims=True)
        atp = torch.from_numpy(atp).to(dev)
        seq = "".join(rng.choice(list("ACGU"), L))
        letters = torch.from_numpy(ss.letter_codes(seq)).to(dev)
        probs = model.predict(atp, seq)
        head = gpu_ms(lambda: model.predict(atp, seq), args.steps, args.warmup)
        # (a)
        pinned = torch.empty(probs.shape, dtype=torch.float32, pin_memory=True)
        copy_probs = gpu_ms(lambda: pinned.copy_(probs, non_blocking=True), args.steps, args.warmup)
        torch.cuda.synchronize()
        prob = pinned.numpy()
        above = int((prob[np.triu_indices(L, k=1)] > np.float32(ss.THRESHOLD)).sum())
        if above > 40 * L:          # a map this dense would keep the host's Python loop busy for hours: say so instead
            raise SystemExit(f"L = {L}: {above} pairs above the threshold; the host path cannot be timed on such a map")
        t0 = time.perf_counter()
        pairs = ss.secondary_structure(prob)
        first = 1e3 * (time.perf_counter() - t0)
        decode = first if first > 2000.0 else host_ms(lambda: ss.secondary_structure(prob), args.steps, 0)
        partner_host = np.zeros(L, dtype=int)
        for i, j in pairs:
            partner_host[i], partner_host[j] = j + 1, i + 1
        savetxt = host_ms(lambda: ss._tables_on_host(host_dir, "x", seq, partner_host), args.steps, 1)
        # (b)
        kernel = gpu_ms(lambda: ops.ss_pairs(probs, letters), args.steps, args.warmup)
        outs = ops.ss_pairs(probs, letters)
        pins = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in outs]

        def copies():
            for p, t in zip(pins, outs):
                p.copy_(t, non_blocking=True)

        copy_small = gpu_ms(copies, args.steps, args.warmup)
        torch.cuda.synchronize()
        partner, counts, ct, bp = (p.numpy() for p in pins)
        assert int(counts[3]) == 0
        writes = host_ms(lambda: ss._tables_from_bodies(dev_dir, "x", L, memoryview(ct)[:int(counts[1])], memoryview(bp)[:int(counts[2])]),
                         args.steps, args.warmup)
        same = (all(open(os.path.join(host_dir, "x" + e), "rb").read() == open(os.path.join(dev_dir, "x" + e), "rb").read()
                    for e in (".ct", ".bpseq")) and ss.pairs_from_partner(partner) == pairs)
        a, b = copy_probs + decode + savetxt, kernel + copy_small + writes
        row = {"L": L, "pairs_above_threshold": above, "pairs": len(pairs), "same_files_and_pairs": same,
               "host_copy_probs_ms": copy_probs, "host_decode_ms": decode, "host_savetxt_tables_ms": savetxt, "host_path_ms": a,
               "kernel_ms": kernel, "copy_small_ms": copy_small, "binary_writes_ms": writes, "device_path_ms": b,
               "host_over_device": a / b, "head_ms": head, "kernel_over_head": kernel / head}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    shutil.rmtree(scratch)
    L = 1024
    dense = torch.full((L, L), 0.9, device=dev)
    letters = torch.full((L,), ord("A"), dtype=torch.uint8, device=dev)
    dense_ms = gpu_ms(lambda: ops.ss_pairs(dense, letters), 3, 1)
    dense_pairs = int(ops.ss_pairs(dense, letters)[1][0].item())
    doc = {"what": "SS head structure: D2H of the probabilities + secondary_structure + two np.savetxt tables on the host against "
                   "rnamsm_ss_pairs + four small copies + two binary writes; median of `steps`",
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "bars": {"device_path_at_most_host_path": all(r["device_path_ms"] <= r["host_path_ms"] for r in rows),
                    "same_files_and_pairs": all(r["same_files_and_pairs"] for r in rows)},
           "rows": rows,
           "dense_worst_case": {"L": L, "rounds": L - 2, "kernel_ms": dense_ms, "pairs": dense_pairs}}
    out = json.dumps(doc, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
