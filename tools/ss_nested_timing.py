#!/usr/bin/env python3
"""The nested structure decoding: HIP-event time of the whole ss.nested_structure call (every fill launch and the
traceback; the call's own allocations come from the caching allocator, after a warm-up) -- median of 7, at L = 64 x 64 packed,
512, 1024 and 4096.
Inputs: helices on noise (tests/ss_pairs_cases.helix_noise_1024 at 1024; the planted map of tests/ss_nested_truth.py at 4096; a
random sigmoid map elsewhere).  Beside it rnamsm_ss_pairs (its long sibling past 1024) on the same map, and a -O2 build of the host
header's serial model (tests/native/ss_nested_check.cpp, L <= 1024 only), whose partner vector is compared with the device's.
The fill (all its launches) and the traceback are also timed separately: the same launches enqueued by two calls of
rnamsm_ss_nested_phases with an event around each (ops.ss_nested_phase_times), median of 7.  Every case names its input family.
Figures as measured, no bar, into profiles/ss_nested_timing.json.

    python tools/ss_nested_timing.py [--out FILE]
"""
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rna-msm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import ss_nested_truth as T
import ss_pairs_cases as C
from rnamsm import ops, ss

args = sys.argv[1:]
out = os.path.join(ROOT, "profiles", "ss_nested_timing.json")
if args[:1] == ["--out"]:
    out = args[1]
dev = torch.device("cuda:0")
RUNS = 7


def timed(fn):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return res, {"median": statistics.median(times), "min": min(times), "all": times}


def phases(probs, letters):
    ops.ss_nested_phase_times(probs, letters)
    runs = [ops.ss_nested_phase_times(probs, letters)[1:] for _ in range(RUNS)]
    return {"fill_ms": statistics.median(r[0] for r in runs), "traceback_ms": statistics.median(r[1] for r in runs)}


def host_model(exe, prob, seq, tmp):
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        f.write(np.int32(len(seq)).tobytes() + np.float32(0.516).tobytes() + np.int32(3).tobytes() + bytes(ss.letter_codes(seq))
                + np.ascontiguousarray(prob).tobytes())
    text = subprocess.run([exe, src, dst, "3"], check=True, capture_output=True, text=True).stdout
    partner = np.frombuffer(open(dst, "rb").read(), dtype=np.int32, count=len(seq))
    return float(text.split()[1]), partner


res = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "runs": RUNS, "theta": 0.516, "min_loop": 3, "cases": []}
with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "ss_nested_check")
    subprocess.run([shutil.which("g++"), "-std=c++17", "-O2", os.path.join(ROOT, "tests", "native", "ss_nested_check.cpp"), "-o", exe],
                   check=True)
    # 64 structures of L = 64 in one packed call
    maps = [C.random_sigmoid(64, 500 + n, 0.0) for n in range(64)]
    probs = [torch.from_numpy(m).to(dev) for m in maps]
    letters = [torch.from_numpy(ss.letter_codes(C.seq_for(64, n))).to(dev) for n in range(64)]
    got, ms = timed(lambda: ss.nested_structure_many(probs, letters))
    _, ms_pairs = timed(lambda: ss.structure_many(probs, letters))
    case = {"L": 64, "packed": 64, "input": "random sigmoid maps", "decode_ms": ms, **phases(probs, letters), "ss_pairs_ms": ms_pairs, "fill_launches": 1,
            "pairs": int(sum(int(g[1][0]) for g in got))}
    res["cases"].append(case)
    print(json.dumps(case), flush=True)
    for L in (512, 1024, 4096):
        prob = C.helix_noise_1024() if L == 1024 else T.planted_4096()[0] if L == 4096 else C.random_sigmoid(L, L, -1.0)
        seq = C.seq_for(L, L)
        p, l = torch.from_numpy(np.ascontiguousarray(prob)).to(dev), torch.from_numpy(ss.letter_codes(seq)).to(dev)
        got, ms = timed(lambda: ss.nested_structure(p, l))
        _, ms_pairs = timed(lambda: (ss.structure if L <= 1024 else ss.structure_long)(p, l))
        family = "helices on noise (helix_noise_1024)" if L == 1024 else "planted nested helices" if L == 4096 else "random sigmoid map"
        case = {"L": L, "packed": 1, "input": family, "decode_ms": ms, **phases([p], [l]), "ss_pairs_ms": ms_pairs, "fill_launches": -(-L // 64),
                "workspace_bytes": 8 * (-(-L // 64) * 64) ** 2, "pairs": int(got[1][0]), "score": int(got[1][4])}
        if L <= 1024:
            seconds, partner = host_model(exe, prob, seq, tmp)
            case["host_serial_O2_ms"] = 1e3 * seconds
            case["host_equal"] = bool(np.array_equal(partner, got[0].cpu().numpy()))
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(f"wrote {out}")
