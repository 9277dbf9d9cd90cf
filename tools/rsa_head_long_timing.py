#!/usr/bin/env python3
"""RNA-MSM RSA head on long alignments: ms per sequence of rnamsm_rsa_head_long (K = 3 members, random weights, 4 launches) at
L = 1500, 3000 and 4096 against the same three networks in PyTorch eager fp32 on the same device from the normalised input (the
comparison tools/rsa_head_timing.py makes, measured in the same run), and of the tables' text: rnamsm_rsa_text_long plus the copy
of its record to the host against write_rsa_files' host arithmetic and np.savetxt on the same values (wall clock, into a
temporary directory).  Median of --steps after --warmup, with min .. max.  One JSON document on stdout (and to --out).

    python tools/rsa_head_long_timing.py --out profiles/rsa_head_long_timing.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rsa_head_long_timing.py --hip-only --sizes 4096
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rna-msm_amd"), os.path.join(ROOT, "tests")]

import numpy as np      # noqa: E402
import torch            # noqa: E402

HIP_LAUNCHES = 4


def _stats(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


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
    return _stats(ms)


def wall_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t))
    return _stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1500,3000,4096")
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hip-only", action="store_true", help="the long head alone (for a kernel trace)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from rnamsm import rsa
    import rsa_truth as T

    dev = torch.device("cuda:0")
    states = [T.make_state(k) for k in range(args.members)]
    st = T.load_stats("oh")
    ens = rsa.RSAEnsemble([rsa.RSAPredictor.from_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}) for sd in states],
                          {"emb": (st["emb_mu"], st["emb_std"]), "oh": (st["oh_mu"], st["oh_std"])}).eval().to(dev)
    dev_states = [{k: torch.from_numpy(v).to(dev) for k, v in sd.items() if not k.endswith("num_batches_tracked")} for sd in states]
    rows = []
    for L in [int(s) for s in args.sizes.split(",") if s]:
        rng = np.random.RandomState(L)
        emb = (st["emb_mu"] + st["emb_std"] * rng.standard_normal((L, 768))).astype(np.float32)
        seq = "".join(rng.choice(list("ACGU"), L))
        e = torch.from_numpy(emb).to(dev)
        codes = torch.from_numpy(rsa.base_codes(seq)).to(dev)
        letters = torch.from_numpy(rsa.letter_codes(seq)).to(dev)
        with torch.no_grad():
            hip = gpu_ms(lambda: ens.predict_long(e, codes), args.steps, args.warmup)
        row = {"L": L, "members": args.members, "hip_long_ms": hip, "hip_launches": HIP_LAUNCHES}
        if not args.hip_only:
            x = torch.from_numpy(T.features(emb, seq, st)).to(dev)

            def eager():
                return [torch.sigmoid(T.logits_torch(x, sd)) for sd in dev_states]

            with torch.no_grad():
                eag = gpu_ms(eager, args.steps, args.warmup)
                values = ens.predict_long(e, codes)
                err = max(float((values[k] - p).abs().max()) for k, p in enumerate(eager()))
            row.update(torch_eager_ms=eag, eager_over_hip=eag["median"] / hip["median"], max_abs_to_eager=err,
                       not_slower_than_eager=bool(hip["median"] <= eag["median"]))
            host_values = values.cpu().numpy()

            def text_device():
                return [t.cpu() for t in rsa.table_text_long(values, letters)]

            def text_host():
                with tempfile.TemporaryDirectory(prefix="rsa_long_timing_") as d:
                    rsa.write_rsa_files(host_values, seq, "x", d, ens.model_names, random.Random(2022))

            record = text_device()
            assert int(record[1][args.members + 1]) == 0 and int(record[1][args.members + 2]) == 0
            tdev, thost = wall_ms(text_device, args.steps, args.warmup), wall_ms(text_host, args.steps, 1)
            row.update(text_long_device_ms=tdev, text_host_write_rsa_files_ms=thost, host_over_device_text=thost["median"] / tdev["median"])
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    doc = {"what": f"RNA-MSM RSA head on long alignments (rnamsm_rsa_head_long), {args.members} members, one sequence per call, fp32; "
                   f"eager = the same networks from normalised input, one after the other; text: rnamsm_rsa_text_long and the copy of "
                   f"its record to the host (wall clock) against write_rsa_files into a temporary directory",
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "rows": rows}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
