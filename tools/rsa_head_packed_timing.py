#!/usr/bin/env python3
"""RNA-MSM RSA ensemble, several alignments per launch: wall time of ONE rnamsm_rsa_head_packed call over B embeddings against B
sequential rnamsm_rsa_head calls on the same inputs, same process, same device (K = 3, random weights, one-hot kind; both
through the C ABI on preallocated workspaces and outputs, so neither side pays for an allocation).  Median of --steps after
--warmup; per batch the ratio and the ms per alignment.  The outputs of the two paths are compared bit for bit on the way.  One
JSON document on stdout (and to --out).

    python tools/rsa_head_packed_timing.py --out profiles/rsa_head_packed_timing.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rsa_head_packed_timing.py --hip-only

--hip-only: one packed call per batch and nothing else (no lone calls, no timing loop), so that a kernel trace holds exactly
one launch set per batch and its grid sizes can be read off: sum_b ceil(L_b / 32) x K blocks per launch.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rna-msm_amd"), os.path.join(ROOT, "tests")]

import numpy as np      # noqa: E402
import torch            # noqa: E402

K = 3
MIXED_SEED, MIXED_B = 2024, 32


def batches():
    """(label, [L_b]): B = 16 and 64 at L = 35, 64, 128, 256, and one mixed batch with L drawn from 20..200 (fixed seed)."""
    out = [(f"B={B} L={L}", [L] * B) for L in (35, 64, 128, 256) for B in (16, 64)]
    rng = np.random.RandomState(MIXED_SEED)
    out.append((f"B={MIXED_B} L=20..200 (seed {MIXED_SEED})", [int(v) for v in rng.randint(20, 201, size=MIXED_B)]))
    return out


def wall_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from rnamsm import _lib, rsa
    import rsa_truth

    dev = torch.device("cuda:0")
    lib = _lib.load()
    members = [rsa.RSAPredictor.from_state_dict({k: torch.from_numpy(v) for k, v in rsa_truth.make_state(11 + k).items()})
               for k in range(K)]
    st = rsa_truth.load_stats("oh")
    model = rsa.RSAEnsemble(members, {"emb": (st["emb_mu"], st["emb_std"]), "oh": (st["oh_mu"], st["oh_std"])}).eval().to(dev)
    ptrs, _ = model._packed_weights()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for label, Ls in batches():
        B = len(Ls)
        rng = np.random.RandomState(B * 1000 + Ls[0])
        embs, codes = [], []
        for L in Ls:
            embs.append(torch.from_numpy((st["emb_mu"] + st["emb_std"] * rng.standard_normal((L, 768))).astype(np.float32)).to(dev))
            codes.append(torch.from_numpy(rng.randint(0, 4, size=L).astype(np.uint8)).to(dev))
        positions = sum(Ls)
        tiles = sum((L + 31) // 32 for L in Ls)
        out_packed = torch.empty(K * positions, device=dev)
        out_lone = torch.empty(K * positions, device=dev)
        offs = np.concatenate([[0], np.cumsum([K * L for L in Ls])]).astype(np.int64)
        ws_packed = torch.empty(lib.rnamsm_rsa_head_packed_workspace_bytes(B, (ctypes.c_int * B)(*Ls), K), dtype=torch.uint8, device=dev)
        ws_lone = torch.empty(lib.rnamsm_rsa_head_workspace_bytes(max(Ls), K), dtype=torch.uint8, device=dev)
        items = (_lib.RsaItem * B)()
        for b, L in enumerate(Ls):
            items[b] = _lib.RsaItem(embs[b].data_ptr(), 768, codes[b].data_ptr(), L, out_packed.data_ptr() + 4 * int(offs[b]), None)

        def packed():
            _lib.check(lib.rnamsm_rsa_head_packed(items, B, K, 1, ptrs, ws_packed.data_ptr(), ws_packed.numel(), stream))

        def lone():
            for b, L in enumerate(Ls):
                _lib.check(lib.rnamsm_rsa_head(embs[b].data_ptr(), 768, codes[b].data_ptr(), L, K, 1, ptrs,
                                               out_lone.data_ptr() + 4 * int(offs[b]), None, ws_lone.data_ptr(), ws_lone.numel(), stream))

        row = {"batch": label, "B": B, "L_min": min(Ls), "L_max": max(Ls), "positions": positions, "blocks_per_launch": tiles * K,
               "launches_packed": 4 + (B + 31) // 32, "launches_sequential": 4 * B}
        if args.hip_only:
            packed()
            torch.cuda.synchronize()
        else:
            seq_ms, seq_min = wall_ms(lone, args.steps, args.warmup)
            pk_ms, pk_min = wall_ms(packed, args.steps, args.warmup)
            same = bool(torch.equal(out_packed.view(torch.int32), out_lone.view(torch.int32)))
            row.update(sequential_ms=seq_ms, sequential_ms_min=seq_min, packed_ms=pk_ms, packed_ms_min=pk_min,
                       speedup=seq_ms / pk_ms, sequential_ms_per_alignment=seq_ms / B, packed_ms_per_alignment=pk_ms / B,
                       bit_identical=same)
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    doc = {"what": "RNA-MSM RSA ensemble, K = 3, fp32: one rnamsm_rsa_head_packed call over B alignments against B sequential "
                   "rnamsm_rsa_head calls; wall time, median of `steps`",
           "device": torch.cuda.get_device_name(0), "n_models": K, "steps": args.steps, "warmup": args.warmup, "rows": rows}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not args.hip_only and not all(r["bit_identical"] for r in rows):
        sys.exit("a packed batch's outputs differ from the lone calls'")


if __name__ == "__main__":
    main()
