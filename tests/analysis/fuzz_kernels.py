#!/usr/bin/env python3
"""Randomised fuzz of the fp32 kernel entry points through rnamsm.ops against fp64 torch arithmetic: ragged row counts,
strided operand / output views (leading dimensions larger than the row), every epilogue combination, random head counts.
  * rnamsm_gemm_bias_act_res      M 1..700, N in 128 k, K in 32 k, lda / ldc / ldr padded, bias / GELU / residual
                                  (also in place) / column scale / zero_rows, both tile widths
  * rnamsm_gemm_lnfold (+ stats)  the same GEMM with LayerNorm folded in, against LayerNorm -> Linear in fp64
  * rnamsm_row_logits + softmax_rows + row_apply,  rnamsm_col_attn_fused        q / k / v as column slices of one wide
                                  activation (ld = 3 H 64 + padding), R 1..300, C 1..300, H 1..12, padded keys
  * rnamsm_gemm_bf16 (plane operands)  M 1..6000 (both sides of the 2048-row kernel switch), N in 128 k up to 1536, K in 64 k,
                                  bf16 / bf16x3 / f16x3, every staging variant ("gemm16_dma" 0..4, "gemm16_mfma16", "gemm_group", "gemm16_dephase"),
                                  fp32 output (+ residual) or plane output (+ GELU / column scale), against the fp64
                                  product of the PLANE VALUES
  * rnamsm_greedy_select / rnamsm_msa_weights   random alignments built from a few mutated founders (ties everywhere), both
                                  greedy schemes ("greedy_fused" 0 / 2), max and min: device rows == host rows, weights bit-equal
With --16 (run16: a separate case stream, so that run()'s seeds replay the cases they always did):
  * rnamsm_row_logits16 + softmax_rows_planes + row_apply16, rnamsm_col_attn16(_prescaled)   R / C biased to the edges of
                                  the dispatch thresholds (256x256 tiles, row_logits16q at C >= 384 with C % 8 == 0, the qb2
                                  rounding rule on R, the slab caps) up to 1024, H 1..12, bf16 or f16x3, "attn16" 1 / 2 / 4 / 5,
                                  "row16_max_rows" 0 / 32, padding masks, plane output, q / k / v as plane views with ld =
                                  3 H 64 + 8 k into buffers whose unused columns and extra rows hold NaN bit patterns -- against
                                  fp64 on the plane values and on the fp32 operands at tests/test_gpu_attn16.py's MODES bars; every
                                  output finite (the kernels clamp tail reads to in-view rows: a NaN is an over-read)
Exit code 1 on any violation.     python tests/analysis/fuzz_kernels.py [--16] [cases [seed]]
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "rna-msm_amd"))

import numpy as np
import torch

from rnamsm import ops
from rnamsm._lib import ACT_GELU_ERF, ACT_NONE

DEV = "cuda:0"


def strided(rows, cols, gen, pad):
    """[rows, cols] view with row stride cols + pad into a larger buffer filled with NaN outside the view."""
    buf = torch.full((rows, cols + pad), float("nan"), device=DEV)
    view = buf[:, :cols]
    view.copy_(torch.randn(rows, cols, device=DEV, generator=gen))
    return view


def rel(a, b):
    return float((a.double() - b).norm() / b.norm().clamp_min(1e-30))


def fuzz_gemm(rng, gen):
    M = int(rng.integers(1, 700))
    N = 128 * int(rng.integers(1, 5))
    K = 32 * int(rng.integers(1, 17))
    a = strided(M, K, gen, 4 * int(rng.integers(0, 4)))
    w = torch.randn(N, K, device=DEV, generator=gen) * 0.1
    bias = torch.randn(N, device=DEV, generator=gen) if rng.random() < 0.8 else None
    act = ACT_GELU_ERF if rng.random() < 0.4 else ACT_NONE
    res_mode = int(rng.integers(0, 3))                  # 0 none, 1 separate, 2 in place
    out = strided(M, N, gen, 4 * int(rng.integers(0, 4)))
    residual = None if res_mode == 0 else (strided(M, N, gen, 4 * int(rng.integers(0, 4))) if res_mode == 1 else out)
    res64 = None if residual is None else residual.double().clone()
    scale_cols = 4 * int(rng.integers(0, N // 4 + 1)) if rng.random() < 0.5 else 0
    scale = float(rng.uniform(0.05, 2.0))
    zero_rows = (torch.rand(M, device=DEV, generator=gen) < 0.2).to(torch.uint8) if (rng.random() < 0.3 and act == ACT_NONE and res_mode == 0) else None
    ops.set_param("gemm_tile", int(rng.integers(0, 3)))
    want = a.double() @ w.double().T
    if bias is not None:
        want = want + bias.double()
    if scale_cols:
        want[:, :scale_cols] *= scale
    if zero_rows is not None:
        want[zero_rows.bool(), :scale_cols] = 0.0
    if act == ACT_GELU_ERF:
        want = torch.nn.functional.gelu(want)
    if res64 is not None:
        want = want + res64
    ops.linear(a, w, bias, act=act, residual=residual, scale=scale, scale_cols=scale_cols, out=out, zero_rows=zero_rows)
    err = rel(out, want)
    return err < 2e-6, f"gemm M={M} N={N} K={K} act={act} res={res_mode} scale_cols={scale_cols} zero_rows={zero_rows is not None}: {err:.2e}"


def fuzz_lnfold(rng, gen):
    M = int(rng.integers(1, 700))
    N = 128 * int(rng.integers(1, 5))
    K = 32 * int(rng.integers(1, 17))
    x = strided(M, K, gen, 4 * int(rng.integers(0, 4)))
    x.mul_(float(rng.uniform(0.2, 3.0))).add_(float(rng.uniform(-1.0, 1.0)))
    w = torch.randn(N, K, device=DEV, generator=gen) * 0.1
    bias = torch.randn(N, device=DEV, generator=gen)
    gamma = 1.0 + 0.1 * torch.randn(K, device=DEV, generator=gen)
    beta = 0.1 * torch.randn(K, device=DEV, generator=gen)
    act = ACT_GELU_ERF if rng.random() < 0.4 else ACT_NONE
    wg, c, d = ops.ln_fold_weights(w, bias, gamma, beta)
    stats = None
    if rng.random() < 0.7:                               # the forward's form: statistics from the producers' partial sums
        stats = ops.row_stats_from_partials(ops.row_partials(x.contiguous()), K)
    ops.set_param("gemm_tile", int(rng.integers(0, 3)))
    out = ops.linear_lnfold(x, wg, c, d, stats=stats, act=act)
    ln = torch.nn.functional.layer_norm(x.double(), (K,), gamma.double(), beta.double(), 1e-5)
    want = ln @ w.double().T + bias.double()
    if act == ACT_GELU_ERF:
        want = torch.nn.functional.gelu(want)
    err = rel(out, want)
    return err < 5e-6, f"lnfold M={M} N={N} K={K} act={act} stats={'partials' if stats is not None else 'self'}: {err:.2e}"


def fuzz_row_attention(rng, gen):
    H = int(rng.integers(1, 13))
    while True:
        R, C = int(rng.integers(1, 301)), int(rng.integers(1, 301))
        if R * C <= 20000:
            break
    ld = 3 * 64 * H + 4 * int(rng.integers(0, 4))
    buf = torch.randn(R * C, ld, device=DEV, generator=gen)
    q, k, v = buf[:, :64 * H], buf[:, 64 * H:128 * H], buf[:, 128 * H:192 * H]
    scaling = 0.125 / math.sqrt(R)
    qs = (q * scaling).contiguous()
    qv = buf.clone()
    qv[:, :64 * H] = qs
    q, k, v = qv[:, :64 * H], qv[:, 64 * H:128 * H], qv[:, 128 * H:192 * H]
    partial, nsplit = ops.row_logits(q, k, R, C, H)
    probs = ops.softmax_rows(partial)
    ctx = ops.row_apply(probs, v, R, C, H)
    q4 = q.double().reshape(R, C, H, 64)
    k4 = k.double().reshape(R, C, H, 64)
    v4 = v.double().reshape(R, C, H, 64)
    logits = torch.einsum("rihd,rjhd->hij", q4, k4)
    p = logits.softmax(-1)
    want = torch.einsum("hij,rjhd->rihd", p, v4).reshape(R * C, H * 64)
    e_p = float((probs.double() - p).abs().max())
    e_c = rel(ctx, want)
    return e_p < 2e-5 and e_c < 2e-5, f"row attention R={R} C={C} H={H} ld={ld} nsplit={nsplit}: probs {e_p:.2e} ctx {e_c:.2e}"


def fuzz_col_attention(rng, gen):
    H = int(rng.integers(1, 13))
    while True:
        R, C = int(rng.integers(1, 301)), int(rng.integers(1, 301))
        if R * C <= 20000:
            break
    ld = 3 * 64 * H + 4 * int(rng.integers(0, 4))
    buf = torch.randn(R * C, ld, device=DEV, generator=gen)
    buf[:, :64 * H] *= 0.125 * 1.5
    q, k, v = buf[:, :64 * H], buf[:, 64 * H:128 * H], buf[:, 128 * H:192 * H]
    mask = None
    if rng.random() < 0.4 and R > 1:
        mask = (torch.rand(R * C, device=DEV, generator=gen) < 0.2)
        mask.view(R, C)[0] = False                      # a column never loses all its keys in the reference's use
        mask = mask.to(torch.uint8)
    ops.set_param("col_dma", int(rng.integers(-1, 2)))
    ops.set_param("col_small", int(rng.integers(0, 2)))
    # (round 4) unmasked cases half the time through the log2-domain entry (rnamsm_col_attn_fused_prescaled: first pass without a
    # running maximum, "col_fast" = 0 keeps the online softmax), now and then with a query whose scores leave exp2's range
    pre = mask is None and rng.random() < 0.5
    if pre:
        ops.set_param("col_fast", int(rng.integers(0, 2)))
        if rng.random() < 0.3 and R >= 4:
            i, c = int(rng.integers(0, R)), int(rng.integers(0, C))
            kk = k.view(R, C, H, 64)[int(rng.integers(0, R)), c, 0]
            q.view(R, C, H, 64)[i, c, 0] = (100.0 if rng.random() < 0.5 else -100.0) * kk / kk.norm()
        qs = buf.clone()
        qs[:, :64 * H] *= 1.4426950408889634
        ctx = ops.col_attn(qs[:, :64 * H], qs[:, 64 * H:128 * H], qs[:, 128 * H:192 * H], R, C, H, prescaled=True)
        ops.set_param("col_fast", 1)
    else:
        ctx = ops.col_attn(q, k, v, R, C, H, pad_mask=mask)
    ops.set_param("col_small", 1)
    q4 = q.double().reshape(R, C, H, 64)
    k4 = k.double().reshape(R, C, H, 64)
    v4 = v.double().reshape(R, C, H, 64)
    s = torch.einsum("ichd,jchd->hcij", q4, k4)
    if mask is not None:
        s = s.masked_fill(mask.view(R, C).bool().T[None, :, None, :], -10000.0)
    if R == 1:
        want = v.double()
    else:
        want = torch.einsum("hcij,jchd->ichd", s.softmax(-1), v4).reshape(R * C, H * 64)
    err = rel(ctx, want)
    return err < 2e-5 and bool(torch.isfinite(ctx).all()), f"col attention R={R} C={C} H={H} ld={ld} masked={mask is not None} prescaled={pre}: {err:.2e}"


def fuzz_planes_gemm(rng, gen):
    M = int(rng.integers(1, 6000)) if rng.random() < 0.7 else int(rng.choice([2047, 2048, 2049, 255, 256, 257, 4096]))
    N = 128 * int(rng.integers(1, 13))
    K = 64 * int(rng.integers(1, 9))
    split, fmt = [(1, 0), (3, 1)][int(rng.integers(0, 2))]
    ht = torch.float16 if fmt == 1 else torch.bfloat16
    knobs = {"gemm16_dma": int(rng.integers(0, 5)), "gemm16_mfma16": int(rng.integers(0, 3)), "gemm_group": int(rng.choice([0, 1, 3, 8])),
             "_legacy_draw": int(rng.integers(0, 3))}               # (the removed "gemm16_dephase" draw: keeps the case stream of a seed)
    knobs.pop("_legacy_draw")
    for k_, v_ in knobs.items():
        ops.set_param(k_, v_)
    a = ops.split_bf16(torch.randn(M, K, device=DEV, generator=gen), want_lo=split == 3, fmt=fmt)
    w = ops.split_bf16(torch.randn(N, K, device=DEV, generator=gen) * 0.05, want_lo=split == 3, fmt=fmt)
    bias = torch.randn(N, device=DEV, generator=gen) * 0.1 if rng.random() < 0.8 else None
    eff = lambda pl: sum(p.view(ht).double() for p in pl if p is not None)
    want = eff(a) @ eff(w).T
    if bias is not None:
        want = want + bias.double()
    form = int(rng.integers(0, 4))                      # 0 fp32 out, 1 fp32 out + residual, 2 planes + GELU, 3 planes + column scale
    if form <= 1:
        residual = strided(M, N, gen, 4 * int(rng.integers(0, 4))) if form == 1 else None
        out = strided(M, N, gen, 4 * int(rng.integers(0, 4)))
        if residual is not None:
            want = want + residual.double()
        ops.linear_planes(a, w, bias, residual=residual, out=out, fmt=fmt)
        err, tol = rel(out, want), (2e-6 if split == 1 else 4e-5 if fmt == 0 else 3e-6)
    else:
        scale_cols = 0
        if form == 2:
            oh, ol = ops.linear_planes(a, w, bias, act=ACT_GELU_ERF, out_planes=True, fmt=fmt)
            want = torch.nn.functional.gelu(want)
        else:
            scale_cols = 4 * int(rng.integers(0, N // 4 + 1))
            oh, ol = ops.linear_planes(a, w, bias, scale=0.25, scale_cols=scale_cols, out_planes=True, fmt=fmt)
            want[:, :scale_cols] *= 0.25
        err, tol = rel(eff((oh, ol)).float(), want), (6e-3 if split == 1 else 4e-5 if fmt == 0 else 3e-6)
    return err < tol, f"planes gemm M={M} N={N} K={K} split={split} fmt={fmt} form={form} {knobs}: {err:.2e} (tol {tol:.0e})"


def fuzz_subsampling(rng, gen):
    from rnamsm.msa import greedy_select, greedy_select_device, msa_weights
    N, L = int(rng.integers(2, 500)), int(rng.integers(1, 120))
    founders = rng.integers(4, 11, size=(int(rng.integers(1, 6)), L))
    rows = founders[rng.integers(0, founders.shape[0], size=N)].copy()
    flips = rng.random((N, L)) < rng.uniform(0.0, 0.2)
    rows[flips] = rng.integers(4, 11, size=int(flips.sum()))
    tokens = np.concatenate([np.zeros((N, 1), dtype=np.int64), rows.astype(np.int64)], axis=1)
    n = int(rng.integers(1, N + 2))
    mode = "max" if rng.random() < 0.5 else "min"
    fused = int(rng.choice([0, 2]))
    ops.set_param("greedy_fused", fused)
    got = greedy_select_device(tokens, n, mode, DEV)
    want = greedy_select(tokens, n, mode)
    ok = np.array_equal(got, want)
    w_dev = msa_weights(tokens, 0.2, device=DEV)
    w_host = msa_weights(tokens, 0.2)
    ok_w = np.array_equal(w_dev, w_host)
    return ok and ok_w, f"sub-sampling N={N} L={L} n={n} {mode} greedy_fused={fused}: rows equal {ok}, weights equal {ok_w}"


def run(cases=40, seed=0, log=print):
    rng = np.random.default_rng(seed)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    bad = 0
    DEFAULT_PLANE_KNOBS = {k_: ops.get_param(k_) for k_ in ("gemm16_dma", "gemm16_mfma16", "gemm_group")}
    try:
        for case in range(cases):
            for fn in (fuzz_gemm, fuzz_lnfold, fuzz_row_attention, fuzz_col_attention, fuzz_planes_gemm, fuzz_subsampling):
                ok, note = fn(rng, gen)
                bad += not ok
                log(f"{'ok ' if ok else 'BAD'} {case:3d} {note}")
    finally:
        ops.set_param("gemm_tile", 0)
        ops.set_param("col_dma", -1)
        ops.set_param("greedy_fused", 1)
        for k_, v_ in DEFAULT_PLANE_KNOBS.items():
            ops.set_param(k_, v_)
    log(f"{6 * cases} kernel cases, {bad} violations")
    return bad


# ---- 16-bit attention entry points (run16) ---------------------------------------------------------------------------
R16 = [1, 3, 4, 5, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 1024]
C16 = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 1016, 1019, 1024]
MODES16 = [(1, 0, 2e-6, 8e-3), (3, 1, 3e-6, 3e-6)]      # (split, fmt, bar vs the plane values, bar vs the fp32 operands): test_gpu_attn16.py
BUDGET16 = 1 << 28                                       # R C H max(R, C): fp64 score tensors of <= 2 GB, a case in tens of ms
NAN16 = {0: 0x7FC0, 1: 0x7E00}                           # quiet-NaN bit patterns of bf16 / fp16
PS16 = 4096.0


def _plane_buffer(x, split, fmt, ld, extra):
    """fp32 [T, n] -> (hi, lo | None) plane views [T, n] with row stride ld into buffers of T + extra rows whose other
    columns and rows hold NaN."""
    T, n = x.shape
    out = []
    for p in ops.split_bf16(x, want_lo=split == 3, fmt=fmt):
        if p is None:
            out.append(None)
            continue
        buf = torch.full((T + extra, ld), NAN16[fmt], dtype=torch.int16, device=DEV)
        buf[:T, :n] = p
        out.append(buf[:T, :n])
    return tuple(out)


def _vals(pl, fmt):
    ht = torch.float16 if fmt == 1 else torch.bfloat16
    v = pl[0].contiguous().view(ht).double()
    return v if pl[1] is None else v + pl[1].contiguous().view(ht).double()


def _cut(pl, a, b):
    return (pl[0][:, a:b], None if pl[1] is None else pl[1][:, a:b])


def _draw16(rng, table):
    return int(rng.choice(table)) if rng.random() < 0.7 else int(rng.integers(1, 1025))


def fuzz_attention16(rng, gen):
    while True:
        R, C = _draw16(rng, R16), _draw16(rng, C16)
        if rng.random() < 0.5 and C % 8 == 0 and C > 1:
            C -= int(rng.integers(1, 8))                 # C % 8 != 0 half the time
        hmax = min(12, BUDGET16 // (R * C * max(R, C)))
        if hmax >= 1:
            break
    H = int(rng.integers(1, hmax + 1))
    D = 64 * H
    T = R * C
    split, fmt, tol_e, tol_f = MODES16[int(rng.integers(0, 2))]
    var, max_rows = int(rng.choice([1, 2, 4, 5])), int(rng.choice([0, 32]))
    masked = rng.random() < 0.4
    pre = split == 1 and not masked and rng.random() < 0.5
    out_planes = rng.random() < 0.5
    ld = 3 * D + 8 * int(rng.integers(0, 4))
    extra = int(rng.integers(1, 65))
    ops.set_param("attn16", var)
    ops.set_param("row16_max_rows", max_rows)
    qkv = torch.randn(T, 3 * D, device=DEV, generator=gen)
    pl = _plane_buffer(qkv, split, fmt, ld, extra)
    key_mask = pad = None
    if masked:
        key_mask = (torch.rand(C, device=DEV, generator=gen) < 0.2)
        key_mask[0] = False
        pad = (torch.rand(R, C, device=DEV, generator=gen) < 0.2)
        pad[0] = False                                   # a column never loses all its keys in the reference's use
    # tied row attention
    scale = ops.row_scaling(R)
    partial, nsplit = ops.row_logits16(_cut(pl, 0, D), _cut(pl, D, 2 * D), R, C, H, fmt=fmt, scale=scale)
    probs, pp = ops.softmax_rows_planes(partial, split=split, fmt=fmt, plane_scale=PS16,
                                        key_mask=None if key_mask is None else key_mask.to(torch.uint8))
    ctx = ops.row_apply16(pp, _cut(pl, 2 * D, 3 * D), R, C, H, fmt=fmt, out_scale=1.0 / PS16)
    e = _vals(pl, fmt).view(R, C, 3, H, 64)
    f = qkv.double().view(R, C, 3, H, 64)
    summed = partial.sum(0).double()
    err_l = rel(summed, scale * torch.einsum("rihd,rjhd->hij", e[:, :, 0], e[:, :, 1]))
    lf = scale * torch.einsum("rihd,rjhd->hij", f[:, :, 0], f[:, :, 1])
    err_lf = rel(summed, lf)
    if key_mask is not None:
        summed = summed.masked_fill(key_mask[None, None, :], -10000.0)
        lf = lf.masked_fill(key_mask[None, None, :], -10000.0)
    err_p = float((probs.double() - torch.softmax(summed, -1)).abs().max())
    p_eff = _vals(pp, fmt)[:, :C].reshape(H, C, C) / PS16
    err_c = rel(ctx, torch.einsum("hij,rjhd->rihd", p_eff, e[:, :, 2]).reshape(T, D))
    err_cf = rel(ctx, torch.einsum("hij,rjhd->rihd", torch.softmax(lf, -1), f[:, :, 2]).reshape(T, D))
    # slabs of more than 32 rows ("row16_max_rows" = 0, or plain bf16, whose slabs are uncapped): fp32 chains of up to 64 R terms.
    # There the logits bars and the context-vs-fp32 bar are at least twice what torch's fp32 arithmetic does on the same operands.
    tol_l, tol_lf, tol_cf = tol_e, tol_f, tol_f
    yl = yc = 0.0
    if -(-R // nsplit) > 32:
        f32 = qkv.view(R, C, 3, H, 64)
        l32 = scale * torch.einsum("rihd,rjhd->hij", f32[:, :, 0], f32[:, :, 1])
        c32 = torch.einsum("hij,rjhd->rihd", torch.softmax(l32.masked_fill(key_mask[None, None, :], -10000.0) if key_mask is not None
                                                           else l32, -1), f32[:, :, 2]).reshape(T, D)
        lf0 = scale * torch.einsum("rihd,rjhd->hij", f[:, :, 0], f[:, :, 1])
        yl = rel(l32, lf0)
        yc = rel(c32, torch.einsum("hij,rjhd->rihd", torch.softmax(lf, -1), f[:, :, 2]).reshape(T, D))
        tol_l, tol_lf, tol_cf = max(tol_e, 2 * yl), max(tol_f, 2 * yl), max(tol_f, 2 * yc)
        del f32, l32, c32, lf0
    ldp = (C + 63) // 64 * 64
    tail_ok = ldp == C or all(int(p[:, C:].abs().max()) == 0 for p in pp if p is not None)
    finite = bool(torch.isfinite(partial).all()) and bool(torch.isfinite(probs).all()) and bool(torch.isfinite(ctx).all()) \
        and bool(torch.isfinite(p_eff).all())
    del partial, probs, pp, ctx, p_eff, summed, lf
    # column attention
    cpl = pl
    if pre:
        qs = qkv.clone()
        qs[:, :D] *= 0.125 * 1.4426950408889634
        cpl = _plane_buffer(qs, split, fmt, ld, extra)
        del qs
    args = (_cut(cpl, 0, D), _cut(cpl, D, 2 * D), _cut(cpl, 2 * D, 3 * D), R, C, H)
    if pre:
        got = ops.col_attn16(*args, fmt=fmt, prescaled=True, out_planes=out_planes)
    else:
        got = ops.col_attn16(*args, fmt=fmt, scale=0.125, pad_mask=None if pad is None else pad.to(torch.uint8),
                             out_planes=out_planes)
    got = _vals(got, fmt) if out_planes else got.double()
    finite = finite and bool(torch.isfinite(got).all())

    def col_ref(q, k, v):
        s_ = torch.einsum("ichd,jchd->hcij", q, k)
        if pad is not None:
            s_ = s_.masked_fill(pad.t()[None, :, None, :], -10000.0)
        return torch.einsum("hcij,jchd->ichd", torch.softmax(s_, -1), v).reshape(T, D)
    ce = _vals(cpl, fmt).view(R, C, 3, H, 64) if pre else e
    qe = ce[:, :, 0] * (0.6931471805599453 if pre else 0.125)
    err_k = rel(got, col_ref(qe, ce[:, :, 1], ce[:, :, 2]))
    err_kf = rel(got, col_ref(0.125 * f[:, :, 0], f[:, :, 1], f[:, :, 2]))
    # P is rounded to the operand format inside the column kernel (3e-3 against the plane values in plain bf16); a plain-bf16
    # plane output adds its own 2^-9 rounding (6e-3: the planes GEMM's plane-output bar above)
    tk = (6e-3 if out_planes else 3e-3) if split == 1 else tol_e
    tkf = tol_f if not (split == 1 and out_planes) else 1e-2
    ok = (err_l < tol_l and err_lf < tol_lf and err_p < 2e-6 and err_c < tol_e and err_cf < tol_cf and err_k < tk and err_kf < tkf
          and tail_ok and finite)
    return ok, (f"attention16 R={R} C={C} H={H} ld={ld}+{extra} split={split} fmt={fmt} attn16={var} row16_max_rows={max_rows} "
                f"nsplit={nsplit} masked={masked} prescaled={pre} planes={out_planes}: logits {err_l:.2e}/{err_lf:.2e} probs {err_p:.2e} "
                f"row ctx {err_c:.2e}/{err_cf:.2e} col ctx {err_k:.2e}/{err_kf:.2e} tail0 {tail_ok} finite {finite}"
                + (f" (torch fp32: logits {yl:.2e} ctx {yc:.2e})" if yl else ""))


def run16(cases=40, seed=0, log=print):
    rng = np.random.default_rng(seed)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    bad = 0
    defaults = {k_: ops.get_param(k_) for k_ in ("attn16", "row16_max_rows")}
    try:
        for case in range(cases):
            ok, note = fuzz_attention16(rng, gen)
            bad += not ok
            log(f"{'ok ' if ok else 'BAD'} {case:3d} {note}")
    finally:
        for k_, v_ in defaults.items():
            ops.set_param(k_, v_)
        torch.cuda.empty_cache()
    log(f"{cases} 16-bit attention cases, {bad} violations")
    return bad


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a != "--16"]
    fn = run16 if "--16" in sys.argv[1:] else run
    n = fn(int(argv[0]) if argv else 40, int(argv[1]) if len(argv) > 1 else 0, log=lambda line: print(line, flush=True))
    sys.exit(1 if n else 0)
