"""Timing of the LM head's kernels and of likelihood.scan against the route they replace -> profiles/lm_scan_timing.json.

  head    rnamsm_lm_head on n rows (n = 35, 511, 1023) against MSATransformer.lm_logits + log_softmax + the wild-type subtraction on
          the same n rows; a packed call of 64 members of 63 rows against 64 lone calls
  scan    likelihood.scan against likelihood.masked_marginal_scores on the same 8 query positions, at 64 x 128 and 256 x 512:
          ms per position and torch.cuda.max_memory_allocated

Wall time on one stream with a device sync around every sample: median of --repeats after --warmup, min .. max beside it, the two
arms of a comparison interleaved in one process.  `python bench.py` at the parent commit and at this tree is a run of its own; its
two result lines go into the same JSON under "bench" (--bench-parent / --bench-head: the files holding them).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rna-msm_amd"))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from rnamsm import likelihood, lm, synthetic      # noqa: E402
from rnamsm.model import MSATransformer           # noqa: E402

DEV = "cuda:0"


def timed(fns: dict, repeats: int, warmup: int) -> dict:
    """{name: fn} run in turn, round by round -> {name: {median_ms, min_ms, max_ms}}."""
    samples = {k: [] for k in fns}
    for r in range(warmup + repeats):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                samples[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in samples.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_scan_timing.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-large", action="store_true", help="leave the 256 x 512 scan out")
    ap.add_argument("--bench-parent", default="")
    ap.add_argument("--bench-head", default="")
    args = ap.parse_args()
    state = synthetic.make_state_dict(seed=0)
    model = MSATransformer(num_layers=10)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    model = model.eval().to(DEV)
    head = lm.kernel_of(model)
    V = len(model.vocab)
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup, "head": [], "scan": []}
    rng = np.random.RandomState(0)

    def old_route(x, wt):
        lp = model.lm_logits(x).log_softmax(-1)
        return lp - lp[torch.arange(len(wt), device=DEV), wt].unsqueeze(1)

    with torch.no_grad():
        for n in (35, 511, 1023):
            x = torch.from_numpy(rng.standard_normal((n, 768)).astype(np.float32)).to(DEV)
            wt = torch.from_numpy(rng.randint(0, V, n)).to(DEV)
            t = timed({"lm_head": lambda: head.rows(x, None, wt), "lm_logits_route": lambda: old_route(x, wt)}, args.repeats, args.warmup)
            diff = float((head.rows(x, None, wt)["scores"] - old_route(x, wt)).abs().max())
            result["head"].append({"n": n, **t, "ratio": t["lm_logits_route"]["median_ms"] / t["lm_head"]["median_ms"],
                                   "scores_max_abs_diff": diff})
        xs = [torch.from_numpy(rng.standard_normal((63, 768)).astype(np.float32)).to(DEV) for _ in range(64)]
        wts = [torch.from_numpy(rng.randint(0, V, 63)).to(DEV) for _ in range(64)]
        t = timed({"packed": lambda: head.packed(xs, None, wts), "lone_x64": lambda: [head.rows(x, None, w) for x, w in zip(xs, wts)]},
                  args.repeats, args.warmup)
        same = all(torch.equal(a[k], b[k]) for a, b in zip(head.packed(xs, None, wts), [head.rows(x, None, w) for x, w in zip(xs, wts)])
                   for k in a)
        result["head_packed"] = {"members": 64, "rows_each": 63, **t, "ratio": t["lone_x64"]["median_ms"] / t["packed"]["median_ms"],
                                 "bit_identical": bool(same)}
        for R, C in ((64, 128),) + (() if args.skip_large else ((256, 512),)):
            toks = torch.from_numpy(synthetic.make_tokens(R, C, 5)).to(DEV)
            idx = [int(i) for i in np.linspace(1, C - 1, 8)]
            entry = {"R": R, "C": C, "positions": 8}
            for name, fn in (("scan", lambda: likelihood.scan(model, toks, indices=idx).scores),
                             ("masked_marginal_scores", lambda: likelihood.masked_marginal_scores(model, toks, indices=idx))):
                fn()                                                           # workspace and tables exist from here on
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                t = timed({name: fn}, max(3, args.repeats // 3), 1)[name]
                entry[name] = {**t, "ms_per_position": t["median_ms"] / 8, "max_memory_allocated": torch.cuda.max_memory_allocated()}
            entry["ratio"] = entry["masked_marginal_scores"]["median_ms"] / entry["scan"]["median_ms"]
            entry["scores_max_abs_diff"] = float((likelihood.scan(model, toks, indices=idx).scores
                                                  - likelihood.masked_marginal_scores(model, toks, indices=idx)).abs().max())
            result["scan"].append(entry)
    bench = {}
    for key, path in (("parent", args.bench_parent), ("head", args.bench_head)):
        if path:
            bench[key] = [json.loads(ln) for ln in open(path) if ln.startswith("{")]
    if bench:
        result["bench"] = bench
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
