#!/usr/bin/env python3
"""A sha256 of every output tensor of the 16-bit 256x256 kernels (gemm16_swp / gemm16_q16s / row_logits16x / row_logits16q /
row_apply16x) on fixed-seed operands, in every regime of their K loops, as JSON on stdout: for an A/B of two commits whose kernels
must not reorder a single sum (profiles/gemm16_core_trace_ab.json).  RNAMSM_LIB_PATH picks the library.
Regimes: nk == 1 (redundant reload), nk == 2, nk >= 3 (clamped reload in steady state), full tile grids and ragged edges.
  plane GEMMs   M 2048 / 2300, N 256 / 1280, K 64 / 128 / 192 (plain bf16, 64-deep tiles: nk 1, 2, 3; f16x3, 32-deep: nk 2, 4, 6 --
                rnamsm_gemm_bf16 takes K % 64 == 0 only, so K = 96 and nk == 1 cannot occur in f16x3); fp32 out with / without
                residual, plane out with / without GELU; lnfold and residual_stats once per format; q16s forced at N = 256
  row_logits16  plain bf16 (q kernel) C 384 / 392 / 512, f16x3 (x kernel: two K tiles per row, nk == 1 cannot occur) C 256 / 264 /
                520; H 1 / 2; R 1 / 2 / 3 / 9 -- the rows per split of every case are computed and 1, 2, >= 3 must all occur
  row_apply16   C 256 (smallest for row_apply16x_kernel, which needs R >= 4) / 300 (no multiple of the key tile), R 1 / 5, fp32 and
                plane outputs
  batched       one framed ragged batch (rnamsm_forward_batch with true_rows; the batched logits call has no C entry point of its own):
                plain bf16, alignments of 3 and 2 rows x 384 columns, so row_logits16q_kernel walks (MSA, head, slab, tile) with a
                scale per MSA; emb, atp and row_attn of both alignments are hashed"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rna-msm_amd"))
import numpy as np, torch
from rnamsm import _lib, ops, synthetic
from rnamsm._lib import ACT_GELU_ERF

lib = _lib.load()
dev = torch.device("cuda:0")
FORMATS = [("bf16", 1, 0), ("f16x3", 3, 1)]
out = {}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def rand(name, shape, scale=1.0):
    return torch.from_numpy((scale * synthetic.normal(name, 41, shape)).astype(np.float32)).to(dev)


def planes(x, split, fmt):
    return ops.split_bf16(x, want_lo=(split == 3), fmt=fmt)


def rec(key, *tensors):
    out[key] = [sha(t) for t in tensors if t is not None]


def gemms(tag, split, fmt, shapes):
    for M, N, K in shapes:
        a, w = planes(rand(f"a.{M}.{K}", (M, K)), split, fmt), planes(rand(f"w.{N}.{K}", (N, K), 0.05), split, fmt)
        b, res = rand(f"b.{N}", (N,), 0.1), rand(f"r.{M}.{N}", (M, N))
        k = f"gemm.{tag}.{M}x{N}x{K}"
        rec(k + ".f32", ops.linear_planes(a, w, b, fmt=fmt))
        rec(k + ".f32.res", ops.linear_planes(a, w, b, residual=res, fmt=fmt))
        rec(k + ".planes", *ops.linear_planes(a, w, b, out_planes=True, scale=0.125, scale_cols=96, fmt=fmt))
        rec(k + ".planes.gelu", *ops.linear_planes(a, w, b, act=ACT_GELU_ERF, out_planes=True, fmt=fmt))


for tag, split, fmt in FORMATS:
    gemms(tag, split, fmt, [(M, N, K) for M in (2048, 2300) for N in (256, 1280) for K in (64, 128, 192)])
    M, N, K = 2300, 768, 128
    a, w = planes(rand("f.a", (M, K)), split, fmt), planes(rand("f.w", (N, K), 0.05), split, fmt)
    stats = torch.stack([rand("f.mean", (M,), 0.1), 1.0 + rand("f.rstd", (M,), 0.1).abs()], 1).contiguous()
    rec(f"lnfold.{tag}", *ops.linear_planes_lnfold(a, w, rand("f.c", (N,)), rand("f.d", (N,)), stats, act=ACT_GELU_ERF, scale=0.125,
                                                   scale_cols=256, fmt=fmt))
    x = rand("f.x", (M, N))
    xpl, part = ops.linear_planes_residual_stats(a, w, rand("f.b", (N,), 0.1), x, fmt=fmt)
    rec(f"residual_stats.{tag}", x, xpl[0], xpl[1], part)
default = lib.rnamsm_get_param(b"gemm16_mfma16")
try:
    _lib.check(lib.rnamsm_set_param(b"gemm16_mfma16", 2))
    gemms("bf16.q16s_forced", 1, 0, [(M, 256, K) for M in (2048, 2300) for K in (64, 128, 192)])
finally:
    _lib.check(lib.rnamsm_set_param(b"gemm16_mfma16", default))

for tag, split, fmt in FORMATS:
    for C in ((384, 392, 512) if split == 1 else (256, 264, 520)):
        for H in (1, 2):
            seen = set()
            for R in (1, 2, 3, 9):
                n = lib.rnamsm_row_logits16_nsplit(R, C, H, split)
                rps = -(-R // n)
                seen |= {min(R, (s + 1) * rps) - s * rps for s in range(n)}
                D = 64 * H
                pl = planes(rand(f"qk.{R}.{C}.{H}", (R * C, 2 * D)), split, fmt)
                partial, _ = ops.row_logits16((pl[0][:, :D], None if pl[1] is None else pl[1][:, :D]),
                                              (pl[0][:, D:], None if pl[1] is None else pl[1][:, D:]), R, C, H, fmt=fmt,
                                              scale=ops.row_scaling(R))
                rec(f"row_logits16.{tag}.R{R}.C{C}.H{H}", partial)
            assert 1 in seen and 2 in seen and any(r >= 3 for r in seen), f"rows per split {sorted(seen)} at C={C} H={H} {tag}: a loop regime is missing"
    H, D = 2, 128
    for C in (256, 300):
        for R in (1, 5):
            ldp = (C + 63) // 64 * 64
            p = rand(f"p.{C}", (H * C, ldp)).abs()
            p[:, C:] = 0
            pp, v = planes(p, split, fmt), planes(rand(f"v.{R}.{C}", (R * C, D)), split, fmt)
            rec(f"row_apply16.{tag}.R{R}.C{C}.f32", ops.row_apply16(pp, v, R, C, H, fmt=fmt, out_scale=1.0 / 4096))
            hi = torch.empty(R * C, D, dtype=torch.int16, device=dev)
            lo = torch.empty(R * C, D, dtype=torch.int16, device=dev) if split == 3 else None
            _lib.check(lib.rnamsm_row_apply16(pp[0].data_ptr(), None if pp[1] is None else pp[1].data_ptr(), ldp, v[0].data_ptr(),
                                              None if v[1] is None else v[1].data_ptr(), D, None, D, R, C, H, 64, 1.0 / 4096,
                                              hi.data_ptr(), None if lo is None else lo.data_ptr(), fmt,
                                              torch.cuda.current_stream().cuda_stream))
            rec(f"row_apply16.{tag}.R{R}.C{C}.planes", hi, lo)
from rnamsm.model import MSATransformer
model = MSATransformer(num_layers=10)
model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(seed=0).items()}, strict=True)
model.gemm_dtype = "bf16"
model = model.eval().to(dev)
msas = [torch.from_numpy(synthetic.make_tokens(r, 384, 50 + i)).to(dev) for i, r in enumerate((3, 2))]
for i, got in enumerate(model.forward_ragged(msas, packed=False)):
    rec(f"forward_batch.true_rows.bf16.msa{i}", got["emb"], got["atp"], got["row_attn"])
torch.cuda.synchronize()
print(json.dumps(out, indent=1))
