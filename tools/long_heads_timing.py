#!/usr/bin/env python3
"""The pair heads on stitched long alignments (data.long_heads=stitched): what each long entry point costs beyond L = 1024.
Synthetic weights and maps; per L (default 1500 and 3000) the wall time -- a device synchronise on either side, the best and the
median of --repeats runs after one warm-up -- of rnamsm_contact_head_long (120 channels), rnamsm_ss_head_long (--blocks BasicBlocks, default 16),
rnamsm_ss_prob_text_long and rnamsm_ss_pairs_long (on the head's own probabilities and on a helix-plus-noise matrix that needs
rounds), next to the forwards' time of the same L from profiles/long_msa_timing.json.  Figures as measured: no bar.

    python tools/long_heads_timing.py --out profiles/long_heads_timing.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rna-msm_amd"), os.path.join(ROOT, "tests")]

import numpy as np      # noqa: E402
import torch            # noqa: E402


def timed(fn, repeats):
    fn()                                                  # code objects, allocator
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"best_ms": min(ms), "median_ms": statistics.median(ms), "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--lengths", type=int, nargs="+", default=[1500, 3000])
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("long_heads_timing needs a HIP device: there is no CPU path and no number without one")
    from rnamsm import _lib, ops, ss
    import ss_pairs_long_cases as LC
    import ss_truth
    dev = torch.device("cuda:0")
    forwards = {}
    try:
        with open(os.path.join(ROOT, "profiles", "long_msa_timing.json")) as f:
            for case in json.load(f)["cases"]:
                forwards[case["L"]] = min(r["forwards_ms"] for r in case["runs"])
    except (OSError, KeyError, ValueError):
        pass
    predictor = ss.SSPredictor(args.blocks)
    predictor.load_state_dict({k: torch.from_numpy(v) for k, v in ss_truth.make_state(args.blocks, seed=1).items()}, strict=True)
    predictor = predictor.eval().to(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    weight, bias = torch.randn(120, device=dev, generator=gen), torch.zeros(1, device=dev)
    doc = {"device": torch.cuda.get_device_name(0), "ss_blocks": args.blocks, "cases": []}
    for L in args.lengths:
        idx = torch.arange(L, device=dev)
        atp = torch.rand(120, L, L, device=dev, generator=gen).mul_(2.0 / L)
        atp.mul_(((idx[:, None] - idx[None, :]).abs() < 1023).to(atp.dtype))          # +0.0 where no window holds the pair
        codes = torch.from_numpy(np.random.RandomState(L).randint(0, 4, L).astype(np.uint8)).to(dev)
        letters = torch.from_numpy(np.frombuffer(b"ACGU", np.uint8)[codes.cpu().numpy()].copy()).to(dev)
        probs = predictor.predict_long(atp, codes)
        helix = torch.from_numpy(LC.helix_noise(L)).to(dev)
        case = {"L": L, "forwards_ms_from_long_msa_timing": forwards.get(L),
                "contact_head_long": timed(lambda: ops.contact_head_long(atp, weight, bias), args.repeats),
                "ss_head_long": timed(lambda: predictor.predict_long(atp, codes), args.repeats),
                "ss_prob_text_long": timed(lambda: ops.ss_prob_text_long(probs), args.repeats),
                "ss_pairs_long_on_head_probs": timed(lambda: ops.ss_pairs_long(probs, letters), args.repeats),
                "ss_pairs_long_on_helix_noise": timed(lambda: ops.ss_pairs_long(helix, letters), args.repeats),
                "pairs_in_helix_noise": int(ops.ss_pairs_long(helix, letters)[1][0].item()),
                "workspace_mb": {"contact_head_long": _lib.load().rnamsm_contact_head_long_workspace_bytes(L, 120) / 1e6,
                                 "ss_head_long": _lib.load().rnamsm_ss_head_long_workspace_bytes(L) / 1e6,
                                 "ss_pairs_long": _lib.load().rnamsm_ss_pairs_long_workspace_bytes(L) / 1e6,
                                 "prob_text": _lib.load().rnamsm_ss_prob_text_long_bytes(L) / 1e6}}
        doc["cases"].append(case)
        del atp, probs, helix
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
