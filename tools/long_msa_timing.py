#!/usr/bin/env python3
"""Long alignments (data.long_msa=windows): what the windowed forward costs at the shipped size.  Synthetic weights, max_seqlen = 1024,
R = 64 rows, L = 1500 and 3000 body columns, default stride (512): per L the wall time of the windows' forwards (each ended by a
device synchronise), of the stitch calls (rnamsm_stitch_rows + rnamsm_stitch_pairs, device events around each), the peak allocated
memory, and the achieved GB/s of stitch_pairs against the bytes its traffic model says it must move:

    every window element read once:                  n * H * W^2 * 4
    every covered output element written once:       H * covered * 4
    every uncovered output element written once:     H * (L^2 - covered) * 4
    one read and one further write per further call that covers an element (the running sum):  2 * H * sum_k |earlier-covered part of window k| * 4

One process, one GPU, one JSON document on stdout and in --out.

    python tools/long_msa_timing.py --out profiles/long_msa_timing.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rna-msm_amd")]

import numpy as np      # noqa: E402
import torch            # noqa: E402

HBM_STREAM_TBPS = 6.3   # measured float4 copy on this part (csrc/common.h: PEAK_HBM_TBPS)


def pairs_traffic_bytes(L, W, stride, H):
    """The bytes rnamsm_stitch_pairs must move over an alignment's one-window-per-call run (the docstring's model)."""
    from rnamsm import windows
    starts = [s for s, _, _ in windows.plan_windows(L, W, stride)]
    seen = np.zeros((L, L), bool)
    again = 0
    for s in starts:
        again += int(seen[s:s + W, s:s + W].sum())
        seen[s:s + W, s:s + W] = True
    read = len(starts) * W * W + again
    written = L * L + again
    return 4 * H * (read + written), {"windows": len(starts), "covered_pairs": int(seen.sum()), "recovered_pairs": again}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--lengths", type=int, nargs="+", default=[1500, 3000])
    ap.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("long_msa_timing needs a HIP device: there is no CPU path and no number without one")
    from rnamsm import ops, synthetic, windows
    from rnamsm.model import MSATransformer
    dev = torch.device("cuda:0")
    state = synthetic.make_state_dict(seed=0)
    model = MSATransformer(num_layers=10)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    model = model.eval().to(dev)
    W = model.max_seqlen - 1
    stride = windows.default_stride(W)
    H, D = model.num_layers * model.num_attention_heads, model.embed_dim
    doc = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "W": W, "stride": stride, "hbm_stream_tbps": HBM_STREAM_TBPS,
           "cases": []}
    rng = np.random.RandomState(0)
    with torch.no_grad():
        warm = torch.from_numpy(np.concatenate([np.zeros((args.rows, 1)), rng.choice(synthetic.RESIDUE_TOKENS, (args.rows, W))], 1)
                                .astype(np.int64)).to(dev)
        model.checked_forward_one(warm, need_repr=False)                  # code objects, workspace
        for L in args.lengths:
            toks = torch.from_numpy(np.concatenate([np.zeros((args.rows, 1)), rng.choice(synthetic.RESIDUE_TOKENS, (args.rows, L))], 1)
                                    .astype(np.int64)).to(dev)
            plan = windows.plan_windows(L, W, stride)
            model_bytes, counts = pairs_traffic_bytes(L, W, stride, H)
            runs = []
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                emb = torch.empty(L, D, device=dev)
                atp = torch.empty(H, L, L, device=dev)
                fwd_ms, rows_ms, pairs_ms = 0.0, 0.0, 0.0
                t_all = time.perf_counter()
                for k, (s, _, _) in enumerate(plan):
                    win = torch.cat([toks[:, :1], toks[:, 1 + s:1 + s + W]], 1)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = model.checked_forward_one(win, False, need_repr=False)
                    torch.cuda.synchronize()
                    fwd_ms += (time.perf_counter() - t0) * 1e3
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    ev[0].record()
                    ops.stitch_rows(out["emb"].unsqueeze(0), emb, stride, k)
                    ev[1].record()
                    ops.stitch_pairs(out["atp"].unsqueeze(0), atp, stride, k)
                    ev[2].record()
                    torch.cuda.synchronize()
                    rows_ms += ev[0].elapsed_time(ev[1])
                    pairs_ms += ev[1].elapsed_time(ev[2])
                    del out
                total_ms = (time.perf_counter() - t_all) * 1e3
                runs.append({"forwards_ms": fwd_ms, "stitch_rows_ms": rows_ms, "stitch_pairs_ms": pairs_ms, "total_ms": total_ms,
                             "peak_allocated_gb": torch.cuda.max_memory_allocated() / 1e9,
                             "stitch_pairs_gbps": model_bytes / (pairs_ms * 1e-3) / 1e9,
                             "stitch_fraction_of_forwards": (rows_ms + pairs_ms) / fwd_ms})
                finite = bool(torch.isfinite(emb).all()) and bool(torch.isfinite(atp).all())
                del emb, atp
            doc["cases"].append({"L": L, **counts, "stitch_pairs_model_bytes": model_bytes,
                                 "stitch_pairs_bound_ms_at_stream_rate": model_bytes / (HBM_STREAM_TBPS * 1e12) * 1e3,
                                 "outputs_finite": finite, "runs": runs})
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
