#!/usr/bin/env python3
"""RNA-MSM RSA head timing: ms per sequence of the HIP ensemble (rnamsm_rsa_head, K = 3 members, random weights, 4 launches) and
of the same three networks in PyTorch eager fp32 on the same device (the functional restatement tests/rsa_truth.py, one network
after the other, as the reference's loop over its models runs them), with the launch count of each side.  Median of --steps
after --warmup.  One JSON document on stdout (and to --out).

    python tools/rsa_head_timing.py --out profiles/rsa_head_timing.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rsa_head_timing.py --hip-only --sizes 1024
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rna-msm_amd"), os.path.join(ROOT, "tests")]

import numpy as np      # noqa: E402
import torch            # noqa: E402

HIP_LAUNCHES = 4


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


def eager_launches(fn):
    """Device kernels one call of fn launches, counted by the torch profiler."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="35,128,512,1024")
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hip-only", action="store_true")
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
        with torch.no_grad():
            med, best = gpu_ms(lambda: ens.predict(e, codes), args.steps, args.warmup)
        row = {"L": L, "members": args.members, "hip_ms": med, "hip_ms_min": best, "hip_launches": HIP_LAUNCHES}
        if not args.hip_only:
            x = torch.from_numpy(T.features(emb, seq, st)).to(dev)

            def eager():
                return [torch.sigmoid(T.logits_torch(x, sd)) for sd in dev_states]

            with torch.no_grad():
                tmed, tbest = gpu_ms(eager, args.steps, args.warmup)
                try:
                    n = eager_launches(eager)
                except Exception as exc:       # noqa: BLE001  (profiler not available: the time stands without the count)
                    n = f"not counted: {type(exc).__name__}"
            row.update(torch_eager_ms=tmed, torch_eager_ms_min=tbest, torch_eager_launches=n, eager_over_hip=tmed / med)
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    doc = {"what": f"RNA-MSM RSA head, {args.members} members, one sequence per call, fp32; eager = the same networks from normalised "
                   f"input, one after the other", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "rows": rows}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
