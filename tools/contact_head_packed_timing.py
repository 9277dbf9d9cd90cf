#!/usr/bin/env python3
"""Contact head, several alignments per launch: wall time of ONE rnamsm_contact_head_packed call over B stripped maps against B
sequential rnamsm_contact_head_atp calls on the same inputs, same process, same device (120 channels, O(1) regression weights; both
through the C ABI on preallocated workspaces and outputs, so neither side pays for an allocation).  Median of --steps after
--warmup with min .. max; per batch the ratio and the ms per alignment.  The outputs of the two paths are compared bit for bit at
every point.  One JSON document on stdout (and to --out).

    python tools/contact_head_packed_timing.py --out profiles/contact_head_packed_timing.json
    python tools/contact_head_packed_timing.py --lone [--lib OTHER/librnamsm_hip.so] --out lone.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/contact_head_packed_timing.py --hip-only

--lone: the lone rnamsm_contact_head on un-stripped [120, C, C] maps at C = 512 and 1024, with this tree's library or, with --lib,
another build of it (an earlier commit's: run the two in turn on one device and compare the figures and the hashes).
--hip-only: one lone call at C = 512 and 1024 and one packed call per batch, nothing else, so that a kernel trace holds exactly
those launch sets and the split between the kernels can be read off.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rna-msm_amd")]

import numpy as np      # noqa: E402
import torch            # noqa: E402

NCH = 120
MIXED_SEED, MIXED_B = 2024, 32
LONE_CS = (512, 1024)                    # --lone: timed
HASH_CS = (2, 9, 34, 257, 258, 300)      # --lone: one call each, for the hash alone (tile seams, the 256-row stride of the sums)


def batches():
    """(label, [L_b]): B = 16 and 64 at L = 35, 64, 128, 256, and one ragged batch with L drawn from 20..300 (fixed seed)."""
    out = [(f"B={B} L={L}", [L] * B) for L in (35, 64, 128, 256) for B in (16, 64)]
    rng = np.random.RandomState(MIXED_SEED)
    out.append((f"B={MIXED_B} L=20..300 (seed {MIXED_SEED})", [int(v) for v in rng.randint(20, 301, size=MIXED_B)]))
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
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def maps_like(shape, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.softmax(torch.randn(shape, generator=g) * 3, -1).to(dev)


def lone_rows(lib_path, dev, w, b, stream, steps, warmup):
    """The lone rnamsm_contact_head of the library at lib_path (bound here by hand: an earlier build lacks the newer symbols)."""
    import hashlib
    lib = ctypes.CDLL(lib_path)
    lib.rnamsm_contact_head.restype = ctypes.c_int
    lib.rnamsm_contact_head.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.rnamsm_contact_head_workspace_bytes.restype = ctypes.c_size_t
    lib.rnamsm_contact_head_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    rows = []
    for C in HASH_CS + LONE_CS:
        maps = maps_like((NCH, C, C), dev, C)
        ws = torch.empty(lib.rnamsm_contact_head_workspace_bytes(C, NCH), dtype=torch.uint8, device=dev)
        out = torch.empty(C - 1, C - 1, device=dev)

        def call():
            rc = lib.rnamsm_contact_head(maps.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), C, NCH,
                                         stream)
            assert rc == 0, rc

        row = {"C": C}
        if C in LONE_CS:
            row["ms"] = wall_ms(call, steps, warmup)
        else:
            call()
        row["sha256"] = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
        del maps
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--lone", action="store_true")
    ap.add_argument("--lib", default="", metavar="LIBRARY")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from rnamsm import _lib

    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(5)
    w = (torch.randn(NCH, generator=g) * 20).to(dev)
    b = torch.tensor([0.3], device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    doc = {"device": torch.cuda.get_device_name(0), "nch": NCH, "steps": args.steps, "warmup": args.warmup}
    if args.lone:
        doc["what"] = ("contact head, lone rnamsm_contact_head on un-stripped [120, C, C] maps; wall time per call, median of `steps` "
                       "with min .. max, and the SHA-256 of the [C-1, C-1] result")
        doc["library"] = args.lib or "this tree's"
        doc["rows"] = lone_rows(args.lib or _lib.LIB_PATH, dev, w, b, stream, args.steps, args.warmup)
    else:
        lib = _lib.load()
        doc["what"] = ("contact head, 120 channels: one rnamsm_contact_head_packed call over B alignments against B sequential "
                       "rnamsm_contact_head_atp calls; wall time, median of `steps` with min .. max")
        rows = []
        if args.hip_only:
            for C in LONE_CS:
                maps = maps_like((NCH, C, C), dev, C)
                ws = torch.empty(lib.rnamsm_contact_head_workspace_bytes(C, NCH), dtype=torch.uint8, device=dev)
                out = torch.empty(C - 1, C - 1, device=dev)
                _lib.check(lib.rnamsm_contact_head(maps.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   C, NCH, stream))
                torch.cuda.synchronize()
                del maps
        for label, Ls in batches():
            B = len(Ls)
            atps = [maps_like((NCH, L, L), dev, 1000 * B + 7 * k + L) for k, L in enumerate(Ls)]
            pixels = sum(L * L for L in Ls)
            out_packed, out_lone = torch.empty(pixels, device=dev), torch.empty(pixels, device=dev)
            offs = np.concatenate([[0], np.cumsum([L * L for L in Ls])]).astype(np.int64)
            ws_packed = torch.empty(lib.rnamsm_contact_head_packed_workspace_bytes(B, (ctypes.c_int * B)(*Ls), NCH), dtype=torch.uint8,
                                    device=dev)
            ws_lone = torch.empty(lib.rnamsm_contact_head_workspace_bytes(max(Ls) + 1, NCH), dtype=torch.uint8, device=dev)
            items = (_lib.ContactItem * B)()
            for k, L in enumerate(Ls):
                items[k] = _lib.ContactItem(atps[k].data_ptr(), L * L, L, out_packed.data_ptr() + 4 * int(offs[k]))

            def packed():
                _lib.check(lib.rnamsm_contact_head_packed(items, B, NCH, w.data_ptr(), b.data_ptr(), ws_packed.data_ptr(),
                                                          ws_packed.numel(), stream))

            def lone():
                for k, L in enumerate(Ls):
                    _lib.check(lib.rnamsm_contact_head_atp(atps[k].data_ptr(), L * L, L, NCH, w.data_ptr(), b.data_ptr(),
                                                           out_lone.data_ptr() + 4 * int(offs[k]), ws_lone.data_ptr(), ws_lone.numel(),
                                                           stream))

            any_long = any(L > 256 for L in Ls)
            row = {"batch": label, "B": B, "L_min": min(Ls), "L_max": max(Ls), "pixels": pixels,
                   "sum_blocks": NCH * sum((L + 255) // 256 for L in Ls), "regress_blocks": sum(((L + 31) // 32) ** 2 for L in Ls),
                   "launches_packed": 2 + any_long + (B + 31) // 32, "launches_sequential": sum(2 + (L > 256) for L in Ls)}
            if args.hip_only:
                packed()
                torch.cuda.synchronize()
            else:
                seq = wall_ms(lone, args.steps, args.warmup)
                pk = wall_ms(packed, args.steps, args.warmup)
                same = bool(torch.equal(out_packed.view(torch.int32), out_lone.view(torch.int32)))
                row.update(sequential_ms=seq, packed_ms=pk, speedup=seq["median"] / pk["median"],
                           sequential_ms_per_alignment=seq["median"] / B, packed_ms_per_alignment=pk["median"] / B,
                           packed_not_slower_within_spread=pk["median"] <= seq["median"] + (seq["max"] - seq["min"]) + (pk["max"] - pk["min"]),
                           bit_identical=same)
            print(json.dumps(row), file=sys.stderr, flush=True)
            rows.append(row)
        doc["rows"] = rows
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not args.hip_only and not args.lone and not all(r["bit_identical"] for r in doc["rows"]):
        sys.exit("outputs differ bit for bit")


if __name__ == "__main__":
    main()
