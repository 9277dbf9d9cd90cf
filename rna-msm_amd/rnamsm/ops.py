"""Per-kernel Python entry points over the C ABI (torch tensors in, raw device pointers out).

PyTorch is plumbing here: it allocates HBM and owns the HIP stream; every FLOP runs in
librnamsm_hip.so.  All functions require contiguous float32 tensors on a HIP device and raise
otherwise -- there is no eager fallback.
"""
from __future__ import annotations

import ctypes
import functools
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import ACT_GELU_ERF, ACT_NONE, F32

HEAD_DIM = 64


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _first_tensor(args):
    for a in args:
        if isinstance(a, torch.Tensor):
            return a
        if isinstance(a, (tuple, list)):
            t = _first_tensor(a)
            if t is not None:
                return t
    return None


def _on_operand_device(fn):
    """The library launches on the calling thread's CURRENT device and stream.  A worker thread (the CLI's MSA reader)
    or a model on cuda:1 has operands elsewhere, so every op enters the device of its first tensor operand first;
    `_stream()` then is that device's current stream."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        t = _first_tensor(args)
        if t is None:
            t = _first_tensor(tuple(kwargs.values()))
        if t is None or not t.is_cuda:
            return fn(*args, **kwargs)            # the op itself raises the "no CPU path" error
        with torch.cuda.device(t.device):
            return fn(*args, **kwargs)
    return wrapper


def _dev(t: torch.Tensor, name: str, dtype=torch.float32) -> int:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.RnamsmError(f"{name}: expected a tensor on the HIP device (no CPU path exists)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t.data_ptr()


def _rowmajor(t: torch.Tensor, name: str) -> int:
    """Leading dimension (in elements) of a 2-D view whose last dim is contiguous."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: expected a 2-D tensor with contiguous rows, got strides {t.stride()}")
    return t.stride(0)


def set_param(name: str, value: int) -> None:
    """rnamsm_set_param: in-process A/B knobs (include/rnamsm.h lists them)."""
    _lib.check(_lib.load().rnamsm_set_param(name.encode(), int(value)))


def get_param(name: str) -> int:
    return int(_lib.load().rnamsm_get_param(name.encode()))


@_on_operand_device
def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    D = x.shape[-1]
    x2 = x.contiguous().view(-1, D)
    y = torch.empty_like(x2) if out is None else out
    _lib.check(_lib.load().rnamsm_layernorm(_dev(x2, "x"), _dev(gamma, "gamma"), _dev(beta, "beta"), _dev(y, "out"),
                                            x2.shape[0], D, eps, _stream()))
    return y.view(x.shape)


@_on_operand_device
def layernorm_split(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5, split: int = 3, fmt: int = 1):
    """LayerNorm whose output goes straight into 16-bit planes (hi, lo | None) [T, D]: the A operand of a 16-bit GEMM."""
    D = x.shape[-1]
    x2 = x.contiguous().view(-1, D)
    hi = torch.empty(x2.shape, dtype=torch.int16, device=x2.device)
    lo = torch.empty(x2.shape, dtype=torch.int16, device=x2.device) if split == 3 else None
    _lib.check(_lib.load().rnamsm_layernorm_split(_dev(x2, "x"), _dev(gamma, "gamma"), _dev(beta, "beta"), hi.data_ptr(),
                                                  None if lo is None else lo.data_ptr(), x2.shape[0], D, eps, fmt, _stream()))
    return hi, lo


@_on_operand_device
def linear(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE,
           residual: Optional[torch.Tensor] = None, scale: float = 1.0, scale_cols: int = 0,
           out: Optional[torch.Tensor] = None, zero_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = act((a @ w.T + bias) * (col < scale_cols ? scale : 1)) + residual;  a [M,K], w [N,K].
    zero_rows (uint8 [M]): flagged rows get 0 in the scaled columns (q *= 1 - padding_mask)."""
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    _lib.check(_lib.load().rnamsm_gemm_bias_act_res(
        _dev(a, "a"), _rowmajor(a, "a"), _dev(w.contiguous(), "w"), None if bias is None else _dev(bias, "bias"),
        None if residual is None else _dev(residual, "residual"), 0 if residual is None else _rowmajor(residual, "residual"),
        _dev(out, "out"), _rowmajor(out, "out"), M, N, K, act, scale, scale_cols,
        None if zero_rows is None else _dev(zero_rows, "zero_rows", torch.uint8), F32, _stream()))
    return out


@_on_operand_device
def linear_row_scaled(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], row_factor: torch.Tensor,
                      scale: float = 1.0, scale_cols: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[m, n] = ((a @ w.T + bias)[m, n] * scale) * row_factor[m] for n < scale_cols, (a @ w.T + bias)[m, n] elsewhere
    (rnamsm_gemm_row_scaled: the QKV projection of a ragged batch; the general form of linear(zero_rows=...))."""
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    _lib.check(_lib.load().rnamsm_gemm_row_scaled(
        _dev(a, "a"), _rowmajor(a, "a"), _dev(w.contiguous(), "w"), None if bias is None else _dev(bias, "bias"),
        _dev(out, "out"), _rowmajor(out, "out"), M, N, K, scale, scale_cols, _dev(row_factor, "row_factor"), F32, _stream()))
    return out


@_on_operand_device
def ln_fold_weights(w: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor):
    """LayerNorm(gamma, beta) folded into the Linear (w [N,K], bias) that consumes it: (Wg [N,K], c [N], d [N]) with
    LN(x) w^T + bias = rstd * (x Wg^T - mean * c) + d  (include/rnamsm.h, K1 folded)."""
    w = w.contiguous()
    N, K = w.shape
    wg = torch.empty_like(w)
    c = torch.empty(N, device=w.device, dtype=torch.float32)
    d = torch.empty(N, device=w.device, dtype=torch.float32)
    _lib.check(_lib.load().rnamsm_ln_fold_weights(_dev(w, "w"), None if bias is None else _dev(bias, "bias"),
                                                  _dev(gamma, "gamma"), _dev(beta, "beta"), wg.data_ptr(), c.data_ptr(),
                                                  d.data_ptr(), N, K, _stream()))
    return wg, c, d


@_on_operand_device
def row_partials(x: torch.Tensor) -> torch.Tensor:
    """(sum x, sum (x - slab mean)^2) of every row of x [T, D] per 32-feature slab, slab-major: [D/32, T, 2], the statistics
    format of the folded LayerNorm (include/rnamsm.h, K1 folded)."""
    D = x.shape[-1]
    x2 = x.contiguous().view(-1, D)
    out = torch.empty(D // 32, x2.shape[0], 2, device=x2.device, dtype=torch.float32)
    _lib.check(_lib.load().rnamsm_row_partials(_dev(x2, "x"), out.data_ptr(), x2.shape[0], D, _stream()))
    return out


@_on_operand_device
def linear_residual_stats(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], residual: torch.Tensor,
                          out: Optional[torch.Tensor] = None):
    """(out, row_partials): out = a @ w.T + bias + residual (may be in place: out = residual) and the row partial sums
    [N/32, M, 2] of the stored out -- the producer side of the folded LayerNorm."""
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    part = torch.empty(N // 32, M, 2, device=a.device, dtype=torch.float32)
    _lib.check(_lib.load().rnamsm_gemm_residual_stats(
        _dev(a, "a"), _rowmajor(a, "a"), _dev(w.contiguous(), "w"), None if bias is None else _dev(bias, "bias"),
        _dev(residual, "residual"), _rowmajor(residual, "residual"), _dev(out, "out"), _rowmajor(out, "out"), M, N, K,
        part.data_ptr(), M, F32, _stream()))
    return out, part


@_on_operand_device
def row_stats_from_partials(partials: torch.Tensor, K: int, rows: Optional[int] = None, eps: float = 1e-5,
                            cond_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(mean, rstd) [rows, 2] of the first `rows` rows from their slab partials [K/32, M, 2] (Chan et al.'s combination).
    cond_flag (int32 [1]): bit 1 is set when a row's mean^2 exceeds 1024 (var + eps) -- the folded GEMM then loses more than
    5 bits to cancellation and the caller should use layernorm + linear for that input."""
    M = partials.shape[1]
    rows = M if rows is None else rows
    stats = torch.empty(rows, 2, device=partials.device, dtype=torch.float32)
    _lib.check(_lib.load().rnamsm_row_stats_from_partials(_dev(partials, "partials"), M, rows, K, eps, stats.data_ptr(),
                                                          None if cond_flag is None else _dev(cond_flag, "cond_flag", torch.int32),
                                                          _stream()))
    return stats


@_on_operand_device
def linear_lnfold(x: torch.Tensor, wg: torch.Tensor, c: torch.Tensor, d: torch.Tensor, stats: Optional[torch.Tensor] = None,
                  eps: float = 1e-5, act: int = ACT_NONE, scale: float = 1.0, scale_cols: int = 0,
                  out: Optional[torch.Tensor] = None, cond_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act((rstd * (x @ wg.T - mean * c) + d) * (col < scale_cols ? scale : 1)) = act(Linear(LayerNorm(x)) ...): the GEMM
    reads x itself; (wg, c, d) from ln_fold_weights; (mean, rstd) of row m = stats[m] (row_stats_from_partials; stats may
    cover more rows than x), or summed by the GEMM itself when None (which then also reports the precondition in cond_flag)."""
    M, K = x.shape
    N = wg.shape[0]
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().rnamsm_gemm_lnfold(_dev(x, "x"), _rowmajor(x, "x"), _dev(wg, "wg"), _dev(c, "c"), _dev(d, "d"),
                                              eps, None if stats is None else _dev(stats, "stats"),
                                              None if cond_flag is None else _dev(cond_flag, "cond_flag", torch.int32),
                                              _dev(out, "out"), _rowmajor(out, "out"), M, N, K, act, scale, scale_cols, F32,
                                              _stream()))
    return out


@_on_operand_device
def split_bf16(w: torch.Tensor, want_lo: bool = True, fmt: int = 0):
    """fp32 tensor -> (hi, lo) 16-bit planes (fmt 0 = bf16, 1 = fp16) as int16 tensors of the same shape
    (lo = half(w - hi), None if not wanted)."""
    w = w.contiguous()
    hi = torch.empty(w.shape, dtype=torch.int16, device=w.device)
    lo = torch.empty(w.shape, dtype=torch.int16, device=w.device) if want_lo else None
    _lib.check(_lib.load().rnamsm_split_bf16(_dev(w, "w"), hi.data_ptr(), None if lo is None else lo.data_ptr(),
                                             w.numel(), fmt, _stream()))
    return hi, lo


@_on_operand_device
def linear_bf16(a: torch.Tensor, w_hi: torch.Tensor, w_lo: Optional[torch.Tensor], bias: Optional[torch.Tensor] = None,
                act: int = ACT_NONE, residual: Optional[torch.Tensor] = None, scale: float = 1.0, scale_cols: int = 0,
                out: Optional[torch.Tensor] = None, split: int = 3, fmt: int = 1) -> torch.Tensor:
    """`linear` on the 16-bit matrix cores: split = 1 (bf16 operands) or 3 (hi/lo fp16 split: fmt must be 1 = f16x3)."""
    M, K = a.shape
    N = w_hi.shape[0]
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    _lib.check(_lib.load().rnamsm_gemm_bf16(
        _dev(a, "a"), _rowmajor(a, "a"), _dev(w_hi, "w_hi", torch.int16), None if w_lo is None else _dev(w_lo, "w_lo", torch.int16),
        None if bias is None else _dev(bias, "bias"), None if residual is None else _dev(residual, "residual"),
        0 if residual is None else _rowmajor(residual, "residual"), _dev(out, "out"), _rowmajor(out, "out"), M, N, K, act,
        scale, scale_cols, split, fmt, None, None, None, None, _stream()))
    return out


@_on_operand_device
def row_logits(q: torch.Tensor, k: torch.Tensor, R: int, C: int, H: int, rows_per_chunk: int = 0) -> Tuple[torch.Tensor, int]:
    """q, k: [R*C, *] views with row stride ld; returns (partial [nsplit,H,C,C], nsplit).  rows_per_chunk > 0: one slab
    per reference row chunk (the padded, chunked path: rnamsm_row_logits_chunked)."""
    lib = _lib.load()
    nsplit = (R + rows_per_chunk - 1) // rows_per_chunk if rows_per_chunk > 0 else lib.rnamsm_row_logits_nsplit(R, C, H)
    partial = torch.empty(nsplit, H, C, C, device=q.device, dtype=torch.float32)
    ld = _rowmajor(q, "q")
    assert _rowmajor(k, "k") == ld
    if rows_per_chunk > 0:
        _lib.check(lib.rnamsm_row_logits_chunked(_dev(q, "q"), _dev(k, "k"), ld, _dev(partial, "partial"), R, C, H, HEAD_DIM,
                                                 rows_per_chunk, F32, _stream()))
    else:
        _lib.check(lib.rnamsm_row_logits(_dev(q, "q"), _dev(k, "k"), ld, _dev(partial, "partial"), R, C, H, HEAD_DIM, F32,
                                         _stream()))
    return partial, nsplit


def row_chunks(R: int, C: int, max_tokens_per_msa: int):
    """(number of row chunks, rows per chunk) of the reference's _batched_forward (modules.py:717-750), (0, 0) when it
    takes the direct path."""
    mt = min(int(max_tokens_per_msa), 2 ** 31 - 1)
    n = _lib.load().rnamsm_row_chunks(R, C, mt)
    return (n, max(1, mt // C)) if n else (0, 0)


@_on_operand_device
def softmax_rows(partial: torch.Tensor, out: Optional[torch.Tensor] = None,
                 key_mask: Optional[torch.Tensor] = None, chunk_pad_mask: Optional[torch.Tensor] = None,
                 rows_per_chunk: int = 0, logit_scale: float = 1.0) -> torch.Tensor:
    """key_mask uint8 [C]: direct-path fill.  chunk_pad_mask uint8 [R*C] + rows_per_chunk: the chunked path's per-chunk
    fill (slab c is masked by row c*rows_per_chunk of the padding mask).  logit_scale (direct path): multiplies the summed
    logits first -- where the exact path applies 1/sqrt(R) (rnamsm_softmax_rows_scaled)."""
    nsplit, H, C, _ = partial.shape
    probs = torch.empty(H, C, C, device=partial.device, dtype=torch.float32) if out is None else out
    if chunk_pad_mask is not None:
        _lib.check(_lib.load().rnamsm_softmax_rows_chunked(_dev(partial, "partial"), nsplit, _dev(probs, "probs"), H, C,
                                                           _dev(chunk_pad_mask, "chunk_pad_mask", torch.uint8),
                                                           rows_per_chunk, _stream()))
        return probs
    _lib.check(_lib.load().rnamsm_softmax_rows_scaled(_dev(partial, "partial"), nsplit, _dev(probs, "probs"), H, C,
                                                      None if key_mask is None else _dev(key_mask, "key_mask", torch.uint8),
                                                      float(logit_scale), _stream()))
    return probs


@_on_operand_device
def row_apply(probs: torch.Tensor, v: torch.Tensor, R: int, C: int, H: int,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    ctx = torch.empty(R * C, H * HEAD_DIM, device=v.device, dtype=torch.float32) if out is None else out
    _lib.check(_lib.load().rnamsm_row_apply(_dev(probs, "probs"), _dev(v, "v"), _rowmajor(v, "v"), _dev(ctx, "ctx"),
                                            _rowmajor(ctx, "ctx"), R, C, H, HEAD_DIM, None, None, 0, F32, _stream()))
    return ctx


@_on_operand_device
def col_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, R: int, C: int, H: int,
             out: Optional[torch.Tensor] = None, pad_mask: Optional[torch.Tensor] = None, prescaled: bool = False,
             q_rows: Optional[int] = None) -> torch.Tensor:
    """prescaled: q carries dh^-1/2 * log2(e) (rnamsm_col_attn_fused_prescaled: no running maximum in the first pass)."""
    ctx = torch.empty(R * C, H * HEAD_DIM, device=v.device, dtype=torch.float32) if out is None else out
    ld = _rowmajor(q, "q")
    assert _rowmajor(k, "k") == ld and _rowmajor(v, "v") == ld
    if prescaled:
        assert pad_mask is None
        _lib.check(_lib.load().rnamsm_col_attn_fused_prescaled(_dev(q, "q"), _dev(k, "k"), _dev(v, "v"), ld, _dev(ctx, "ctx"),
                                                               _rowmajor(ctx, "ctx"), R, C, H, HEAD_DIM, R if q_rows is None else q_rows,
                                                               _stream()))
        return ctx
    if q_rows is not None:      # only the first q_rows query rows are computed and stored (rnamsm_col_attn_fused_queries)
        _lib.check(_lib.load().rnamsm_col_attn_fused_queries(_dev(q, "q"), _dev(k, "k"), _dev(v, "v"), ld, _dev(ctx, "ctx"),
                                                             _rowmajor(ctx, "ctx"), R, C, H, HEAD_DIM, q_rows,
                                                             None if pad_mask is None else _dev(pad_mask, "pad_mask", torch.uint8),
                                                             F32, _stream()))
        return ctx
    _lib.check(_lib.load().rnamsm_col_attn_fused(_dev(q, "q"), _dev(k, "k"), _dev(v, "v"), ld, _dev(ctx, "ctx"),
                                                 _rowmajor(ctx, "ctx"), R, C, H, HEAD_DIM,
                                                 None if pad_mask is None else _dev(pad_mask, "pad_mask", torch.uint8),
                                                 None, None, 0, F32, _stream()))
    return ctx


@_on_operand_device
def col_attn_probs(q: torch.Tensor, k: torch.Tensor, R: int, C: int, H: int, pad_mask: Optional[torch.Tensor] = None,
                   scale: float = 1.0) -> torch.Tensor:
    """The probabilities the fused column attention never forms (reference modules.py:905-917), on request:
    fp32 [H, C, R, R] = softmax_j(scale * q_i . k_j) per column and head; q as the QKV GEMM left it (already scaled)."""
    probs = torch.empty(H, C, R, R, device=q.device, dtype=torch.float32)
    ld = _rowmajor(q, "q")
    assert _rowmajor(k, "k") == ld
    _lib.check(_lib.load().rnamsm_col_attn_probs(_dev(q, "q"), _dev(k, "k"), ld, _dev(probs, "probs"), R, C, H, HEAD_DIM,
                                                 None if pad_mask is None else _dev(pad_mask, "pad_mask", torch.uint8),
                                                 scale, F32, _stream()))
    return probs


# ---- 16-bit attention contractions: operands are (hi, lo) int16 plane pairs, lo = None for plain bf16 ---------------
def _pl(t: Optional[torch.Tensor], name: str):
    return None if t is None else _dev(t, name, torch.int16)


@_on_operand_device
def linear_planes(a, w, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE, residual: Optional[torch.Tensor] = None,
                  scale: float = 1.0, scale_cols: int = 0, out: Optional[torch.Tensor] = None, out_planes: bool = False,
                  fmt: int = 0):
    """16-bit GEMM whose A operand is already (hi, lo | None) planes [M, K] (the LDS-DMA kernels): returns fp32 [M, N],
    or (hi, lo | None) planes when out_planes (no residual then)."""
    a_hi, a_lo = a
    w_hi, w_lo = w
    M, K = a_hi.shape
    N = w_hi.shape[0]
    split = 3 if w_lo is not None else 1
    o_hi = o_lo = None
    if out_planes:
        o_hi = torch.empty(M, N, dtype=torch.int16, device=a_hi.device)
        o_lo = torch.empty(M, N, dtype=torch.int16, device=a_hi.device) if split == 3 else None
    elif out is None:
        out = torch.empty(M, N, device=a_hi.device, dtype=torch.float32)
    _lib.check(_lib.load().rnamsm_gemm_bf16(
        None, _rowmajor(a_hi, "a_hi"), _pl(w_hi, "w_hi"), _pl(w_lo, "w_lo"), None if bias is None else _dev(bias, "bias"),
        None if residual is None else _dev(residual, "residual"), 0 if residual is None else _rowmajor(residual, "residual"),
        None if out_planes else _dev(out, "out"), N if out_planes else _rowmajor(out, "out"), M, N, K, act, scale, scale_cols,
        split, fmt, _pl(a_hi, "a_hi"), _pl(a_lo, "a_lo"), None if o_hi is None else o_hi.data_ptr(),
        None if o_lo is None else o_lo.data_ptr(), _stream()))
    return (o_hi, o_lo) if out_planes else out


@_on_operand_device
def linear_planes_lnfold(x, wg, c: torch.Tensor, d: torch.Tensor, stats: torch.Tensor, act: int = ACT_NONE, scale: float = 1.0,
                         scale_cols: int = 0, fmt: int = 0):
    """K1 folded, 16-bit modes: x = (hi, lo | None) planes of the RAW residual stream [M, K]; wg = planes of W * gamma;
    c = row sums of the wg planes' values, d = bias + W beta; stats [M, 2].  Returns the output planes (hi, lo | None)."""
    M, K = x[0].shape
    N = wg[0].shape[0]
    split = 1 if x[1] is None else 3
    ohi = torch.empty(M, N, dtype=torch.int16, device=x[0].device)
    olo = torch.empty(M, N, dtype=torch.int16, device=x[0].device) if split == 3 else None
    _lib.check(_lib.load().rnamsm_gemm16_lnfold(_pl(x[0], "x_hi"), _pl(x[1], "x_lo"), _rowmajor(x[0], "x_hi"), _pl(wg[0], "wg_hi"),
                                                _pl(wg[1], "wg_lo"), _dev(c, "c"), _dev(d, "d"), _dev(stats, "stats"),
                                                ohi.data_ptr(), None if olo is None else olo.data_ptr(), N, M, N, K, act, scale,
                                                scale_cols, split, fmt, _stream()))
    return ohi, olo


@_on_operand_device
def linear_planes_residual_stats(a, w, bias: Optional[torch.Tensor], x: torch.Tensor, fmt: int = 0):
    """x += a w^T + bias in place (fp32) on the 16-bit matrix cores; returns (x planes (hi, lo | None), row_partials
    [N/32, M, 2]) of the new x -- the producer side of the folded LayerNorm in the 16-bit modes."""
    M, K = a[0].shape
    N = w[0].shape[0]
    split = 1 if a[1] is None else 3
    xhi = torch.empty(M, N, dtype=torch.int16, device=x.device)
    xlo = torch.empty(M, N, dtype=torch.int16, device=x.device) if split == 3 else None
    part = torch.empty(N // 32, M, 2, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().rnamsm_gemm16_residual_stats(_pl(a[0], "a_hi"), _pl(a[1], "a_lo"), _rowmajor(a[0], "a_hi"),
                                                        _pl(w[0], "w_hi"), _pl(w[1], "w_lo"),
                                                        None if bias is None else _dev(bias, "bias"), _dev(x, "x"),
                                                        _rowmajor(x, "x"), M, N, K, split, fmt, xhi.data_ptr(),
                                                        None if xlo is None else xlo.data_ptr(), N, part.data_ptr(), M,
                                                        _stream()))
    return (xhi, xlo), part


@_on_operand_device
def row_logits16(q, k, R: int, C: int, H: int, fmt: int = 0, scale: float = 1.0) -> Tuple[torch.Tensor, int]:
    """q, k: (hi, lo) plane views [R*C, *] with row stride ld (halves); returns (partial [nsplit,H,C,C] fp32, nsplit);
    scale multiplies the fp32 logits (q is expected UNSCALED)."""
    lib = _lib.load()
    nsplit = lib.rnamsm_row_logits16_nsplit(R, C, H, 1 if q[1] is None else 3)
    partial = torch.empty(nsplit, H, C, C, device=q[0].device, dtype=torch.float32)
    ld = _rowmajor(q[0], "q_hi")
    _lib.check(lib.rnamsm_row_logits16(_pl(q[0], "q_hi"), _pl(q[1], "q_lo"), _pl(k[0], "k_hi"), _pl(k[1], "k_lo"), ld,
                                       _dev(partial, "partial"), R, C, H, HEAD_DIM, scale, fmt, _stream()))
    return partial, nsplit


@_on_operand_device
def softmax_rows_planes(partial: torch.Tensor, split: int = 3, fmt: int = 1, key_mask: Optional[torch.Tensor] = None,
                        plane_scale: float = 1.0):
    """softmax_rows that also returns P * plane_scale as planes (hi, lo | None) [H*C, ldp], ldp = C rounded up to 64,
    tail zeroed."""
    nsplit, H, C, _ = partial.shape
    ldp = (C + 63) // 64 * 64
    probs = torch.empty(H, C, C, device=partial.device, dtype=torch.float32)
    p_hi = torch.empty(H * C, ldp, device=partial.device, dtype=torch.int16)
    p_lo = torch.empty(H * C, ldp, device=partial.device, dtype=torch.int16) if split == 3 else None
    _lib.check(_lib.load().rnamsm_softmax_rows_planes(
        _dev(partial, "partial"), nsplit, _dev(probs, "probs"), p_hi.data_ptr(), None if p_lo is None else p_lo.data_ptr(),
        ldp, plane_scale, H, C, None if key_mask is None else _dev(key_mask, "key_mask", torch.uint8), fmt, _stream()))
    return probs, (p_hi, p_lo)


@_on_operand_device
def row_apply16(p, v, R: int, C: int, H: int, fmt: int = 0, out_scale: float = 1.0) -> torch.Tensor:
    """p: (hi, lo) planes [H*C, ldp]; v: (hi, lo) plane views [R*C, *]; returns out_scale * P v, fp32 [R*C, H*64]."""
    ctx = torch.empty(R * C, H * HEAD_DIM, device=v[0].device, dtype=torch.float32)
    _lib.check(_lib.load().rnamsm_row_apply16(_pl(p[0], "p_hi"), _pl(p[1], "p_lo"), _rowmajor(p[0], "p_hi"),
                                              _pl(v[0], "v_hi"), _pl(v[1], "v_lo"), _rowmajor(v[0], "v_hi"),
                                              _dev(ctx, "ctx"), _rowmajor(ctx, "ctx"), R, C, H, HEAD_DIM, out_scale, None, None,
                                              fmt, _stream()))
    return ctx


@_on_operand_device
def zero_plane_rows(pl, mask: torch.Tensor, ncols: int) -> None:
    """In place: zero the first ncols halves of the plane rows flagged in mask (uint8 [T]) -- q *= 1 - padding_mask."""
    _lib.check(_lib.load().rnamsm_zero_plane_rows(_pl(pl[0], "hi"), _pl(pl[1], "lo"), _dev(mask, "mask", torch.uint8),
                                                  pl[0].shape[0], ncols, _rowmajor(pl[0], "hi"), _stream()))


@_on_operand_device
def col_attn16(q, k, v, R: int, C: int, H: int, fmt: int = 0, scale: float = 1.0,
               pad_mask: Optional[torch.Tensor] = None, out_planes: bool = False, prescaled: bool = False):
    """q, k, v: (hi, lo) plane views [R*C, *] with a common row stride; returns softmax(scale * q k^T) v, fp32
    [R*C, H*64] (q UNSCALED) -- or, with out_planes, the context as the 16-bit (hi, lo | None) int16 planes the forward's
    out_proj GEMM reads (format = the operands': bf16, or fp16 for fmt 1).  prescaled (bf16 formats, no mask): the q planes
    hold q * scale * log2(e) already (rnamsm_col_attn16_prescaled: what the forward runs); `scale` is then ignored."""
    D = H * HEAD_DIM
    ld = _rowmajor(q[0], "q_hi")
    assert _rowmajor(k[0], "k_hi") == ld and _rowmajor(v[0], "v_hi") == ld
    ctx = None if out_planes else torch.empty(R * C, D, device=v[0].device, dtype=torch.float32)
    c_hi = torch.empty(R * C, D, device=v[0].device, dtype=torch.int16) if out_planes else None
    c_lo = torch.empty(R * C, D, device=v[0].device, dtype=torch.int16) if out_planes and q[1] is not None else None
    if prescaled:
        assert fmt == 0 and pad_mask is None
        _lib.check(_lib.load().rnamsm_col_attn16_prescaled(_pl(q[0], "q_hi"), _pl(q[1], "q_lo"), _pl(k[0], "k_hi"), _pl(k[1], "k_lo"),
                                                           _pl(v[0], "v_hi"), _pl(v[1], "v_lo"), ld,
                                                           None if ctx is None else _dev(ctx, "ctx"), D, R, C, H, HEAD_DIM,
                                                           _pl(c_hi, "ctx_hi"), _pl(c_lo, "ctx_lo"), _stream()))
        return (c_hi, c_lo) if out_planes else ctx
    _lib.check(_lib.load().rnamsm_col_attn16(_pl(q[0], "q_hi"), _pl(q[1], "q_lo"), _pl(k[0], "k_hi"), _pl(k[1], "k_lo"),
                                             _pl(v[0], "v_hi"), _pl(v[1], "v_lo"), ld,
                                             None if ctx is None else _dev(ctx, "ctx"), D,
                                             R, C, H, HEAD_DIM, scale,
                                             None if pad_mask is None else _dev(pad_mask, "pad_mask", torch.uint8),
                                             _pl(c_hi, "ctx_hi"), _pl(c_lo, "ctx_lo"), fmt, _stream()))
    return (c_hi, c_lo) if out_planes else ctx


@_on_operand_device
def col_attn_probs16(q, k, R: int, C: int, H: int, fmt: int = 0, scale: float = 1.0,
                     pad_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """col_attn_probs for the 16-bit modes: q, k are (hi, lo | None) plane views (q UNSCALED)."""
    probs = torch.empty(H, C, R, R, device=q[0].device, dtype=torch.float32)
    ld = _rowmajor(q[0], "q_hi")
    assert _rowmajor(k[0], "k_hi") == ld
    _lib.check(_lib.load().rnamsm_col_attn_probs16(_pl(q[0], "q_hi"), _pl(q[1], "q_lo"), _pl(k[0], "k_hi"), _pl(k[1], "k_lo"),
                                                   ld, _dev(probs, "probs"), R, C, H, HEAD_DIM,
                                                   None if pad_mask is None else _dev(pad_mask, "pad_mask", torch.uint8),
                                                   fmt, scale, _stream()))
    return probs


@_on_operand_device
def embed_ln(tokens: torch.Tensor, embed_tokens: torch.Tensor, embed_positions: torch.Tensor, row_pos: torch.Tensor,
             gamma: torch.Tensor, beta: torch.Tensor, pad_idx: int, eps: float = 1e-5, row_pos_dim: int = 1) -> torch.Tensor:
    """tokens int64 [R,C] -> x [R*C, D]; raises on token / position ids outside the tables.  row_pos: [>= R] scalars per
    alignment row (row_pos_dim 1), or flattened [>= R, D] vectors (row_pos_dim = D: the msm/ variant, msm/model.py:289-292)."""
    R, C = tokens.shape
    D = embed_tokens.shape[1]
    out = torch.empty(R * C, D, device=tokens.device, dtype=torch.float32)
    err = torch.zeros(1, device=tokens.device, dtype=torch.int32)
    _lib.check(_lib.load().rnamsm_embed_ln_rows(
        _dev(tokens.contiguous(), "tokens", torch.int64), _dev(embed_tokens, "embed_tokens"),
        _dev(embed_positions, "embed_positions"), _dev(row_pos, "row_pos"), int(row_pos_dim), _dev(gamma, "gamma"), _dev(beta, "beta"),
        _dev(out, "out"), R, C, D, embed_tokens.shape[0], embed_positions.shape[0], pad_idx, eps,
        _dev(err, "err", torch.int32), _stream()))
    if int(err.item()) != 0:
        raise IndexError("embed_ln: token or position index out of range")
    return out


@_on_operand_device
def pack_outputs(x_final: torch.Tensor, probs_all: torch.Tensor, C: int) -> Tuple[torch.Tensor, torch.Tensor]:
    NL, H = probs_all.shape[0], probs_all.shape[1]
    D = x_final.shape[-1]
    emb = torch.empty(C - 1, D, device=x_final.device, dtype=torch.float32)
    atp = torch.empty(NL * H, C - 1, C - 1, device=x_final.device, dtype=torch.float32)
    _lib.check(_lib.load().rnamsm_pack_outputs(_dev(x_final, "x_final"), _dev(probs_all, "probs_all"), _dev(emb, "emb"),
                                               _dev(atp, "atp"), C, D, NL, H, _stream()))
    return emb, atp


@_on_operand_device
def add(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a + b, fp32, same shape (the residual add of NormalizedResidualBlock around a foreign layer, modules.py:396).  `out` (a
    contiguous fp32 tensor of that shape) may be `a` or `b` itself: the kernel reads an element before it writes it."""
    assert a.shape == b.shape
    if out is None:
        a, b = a.contiguous(), b.contiguous()
        out = torch.empty_like(a, dtype=torch.float32)
    else:
        assert out.shape == a.shape and out.is_contiguous() and a.is_contiguous() and b.is_contiguous()
    _lib.check(_lib.load().rnamsm_add(_dev(a, "a"), _dev(b, "b"), _dev(out, "out"), out.numel(), _stream()))
    return out


@_on_operand_device
def head_mean(probs: torch.Tensor) -> torch.Tensor:
    """probs [H, ...] fp32 -> mean over the head axis [...] (msm/multihead_attention.py:394-397)."""
    probs = probs.contiguous()
    H = probs.shape[0]
    out = torch.empty(probs.shape[1:], device=probs.device, dtype=torch.float32)
    _lib.check(_lib.load().rnamsm_head_mean(_dev(probs, "probs"), _dev(out, "out"), H, out.numel(), _stream()))
    return out


@_on_operand_device
def contact_head(row_attn: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """row_attn [NL, H, C, C] (or [NL*H, C, C]) -> contacts [C-1, C-1] (modules.py:344-366)."""
    C = row_attn.shape[-1]
    nch = row_attn.numel() // (C * C)
    lib = _lib.load()
    ws = torch.empty(lib.rnamsm_contact_head_workspace_bytes(C, nch), dtype=torch.uint8, device=row_attn.device)
    out = torch.empty(C - 1, C - 1, device=row_attn.device, dtype=torch.float32)
    _lib.check(lib.rnamsm_contact_head(_dev(row_attn.contiguous(), "row_attn"), _dev(weight.contiguous().view(-1), "weight"),
                                       _dev(bias.contiguous().view(-1), "bias"), _dev(out, "contacts"), ws.data_ptr(),
                                       ws.numel(), C, nch, _stream()))
    return out


def _contact_operand(fn: str, atp: torch.Tensor, name: str):
    """The operand rules of one alignment, for contact_head_atp and for every member of contact_head_packed: -> (atp, L) as the
    library reads them (maps whose rows or planes do not lie as [L, L] planes at least L*L apart are copied)."""
    _dev(atp, name)
    if atp.dim() != 3 or atp.shape[0] < 1 or atp.shape[1] != atp.shape[2]:
        raise ValueError(f"{fn}: {name} must be [nch, L, L], got {tuple(atp.shape)}")
    L = atp.shape[-1]
    if atp.stride(2) != 1 or atp.stride(1) != L or atp.stride(0) < L * L:
        atp = atp.contiguous()
    return atp, L


def _contact_regression(weight: torch.Tensor, bias: torch.Tensor, nch: int, fn: str):
    weight, bias = weight.contiguous().view(-1), bias.contiguous().view(-1)
    _dev(weight, "weight")
    _dev(bias, "bias")
    if weight.numel() != nch or bias.numel() != 1:
        raise ValueError(f"{fn}: regression of {weight.numel()} weights and {bias.numel()} biases for maps of {nch} channels")
    return weight, bias


class _Route(NamedTuple):
    """Which entry point a lone call runs through: the call itself or its `_long` sibling for a stitched long alignment
    (include/rnamsm.h: RNAMSM_LONG_MAX_L), which for an L both accept gives the bits (bytes) of its namesake."""
    fn: str                        # the public function's name, for the messages; the library's symbol is rnamsm_<fn>
    max_L: int
    size: Optional[str] = None     # the symbol of its size function, where the call asks one

    @property
    def entry(self) -> str:
        return "rnamsm_" + self.fn

    @property
    def long(self) -> bool:
        return self.max_L == _lib.LONG_MAX_L


_CONTACT_ATP = _Route("contact_head_atp", _lib.CONTACT_MAX_L, "rnamsm_contact_head_workspace_bytes")
_CONTACT_LONG = _Route("contact_head_long", _lib.LONG_MAX_L, "rnamsm_contact_head_long_workspace_bytes")


def _contact_atp_run(route: _Route, atp: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    members, _ = _members(route.fn, _contact_operand, 1, route.max_L, (None, None, "alignments"), {"atp": [atp]}, lone=True)
    atp, L = members[0]
    nch = atp.shape[0]
    weight, bias = _contact_regression(weight, bias, nch, route.fn)
    lib = _lib.load()
    # rnamsm_contact_head_workspace_bytes takes the width of the un-stripped maps
    ws = torch.empty(getattr(lib, route.size)(L if route.long else L + 1, nch), dtype=torch.uint8, device=atp.device)
    out = torch.empty(L, L, device=atp.device, dtype=torch.float32)
    _lib.check(getattr(lib, route.entry)(atp.data_ptr(), atp.stride(0), L, nch, weight.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _stream()))
    return out


@_on_operand_device
def contact_head_atp(atp: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """The contact head on the stripped maps (rnamsm_contact_head_atp): atp [nch, L, L] fp32 as forward_one / the packed drivers
    leave it (planes may lie further apart than L*L: a slice of a wider buffer is read in place) -> contacts [L, L], the bits of
    contact_head on the [nch, L+1, L+1] maps they were stripped from."""
    return _contact_atp_run(_CONTACT_ATP, atp, weight, bias)


@_on_operand_device
def contact_head_long(atp: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """contact_head_atp for L up to LONG_MAX_L (rnamsm_contact_head_long); symmetrise and APC run over the whole map."""
    return _contact_atp_run(_CONTACT_LONG, atp, weight, bias)


@_on_operand_device
def contact_head_packed(atps: Sequence[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor) -> List[torch.Tensor]:
    """The contact head over several alignments in one launch set (rnamsm_contact_head_packed): atps[b] [nch, L_b, L_b] fp32, the
    operand rules of contact_head_atp per member (slices of one wider buffer are read in place) -> a list of [L_b, L_b] tensors,
    each bit-identical to contact_head_atp on that member alone.  One workspace and one output allocation per call: the returned
    tensors are views of one buffer."""
    members, device = _members("contact_head_packed", _contact_operand, _lib.CONTACT_MAX_BATCH, _lib.CONTACT_MAX_L,
                               (None, None, "alignments"), {"atp": atps})
    if not members:
        return []
    B, Ls, nch = len(members), [L for _, L in members], members[0][0].shape[0]
    for b, (atp, _) in enumerate(members):
        if atp.shape[0] != nch:
            raise ValueError(f"contact_head_packed: atp[{b}] has {atp.shape[0]} channels, atp[0] {nch}")
    weight, bias = _contact_regression(weight, bias, nch, "contact_head_packed")
    lib = _lib.load()
    ws = torch.empty(lib.rnamsm_contact_head_packed_workspace_bytes(B, (_lib.c_int * B)(*Ls), nch), dtype=torch.uint8, device=device)
    outs = [o.view(L, L) for o, L in zip(_carved([L * L for L in Ls], device, torch.float32), Ls)]
    items = (_lib.ContactItem * B)()
    for b, ((atp, L), o) in enumerate(zip(members, outs)):
        items[b] = _lib.ContactItem(atp.data_ptr(), atp.stride(0), L, o.data_ptr())
    _lib.check(lib.rnamsm_contact_head_packed(items, B, nch, weight.data_ptr(), bias.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return outs


def _want(fn: str, want: str) -> None:
    if want not in ("probs", "logits"):
        raise ValueError(f"{fn}: want must be 'probs' or 'logits', got {want!r}")


def _members(fn: str, rule, cap: int, max_L: Optional[int], nouns, operands, checked: int = 1, lone: bool = False):
    """The prologue of a packed call.  operands: {name: sequence}, the per-member operands in the order `rule` takes them (one
    sequence or two); nouns: what the two sequences and the members are called in the messages.  The counts must match and stay
    within `cap`; then every member goes through rule(fn, *operands, *names) -- names `atp[3]`, or plain `atp` for a lone call -- which
    returns it as the library reads it, L last; its first `checked` tensors must lie on the device of member 0 and, with a max_L, L
    within [1, max_L].  -> (rule's results per member, device); ([], None) for an empty call."""
    names = list(operands)
    seqs = [list(s) for s in operands.values()]
    if len(seqs) == 2 and len(seqs[0]) != len(seqs[1]):
        raise ValueError(f"{fn}: {len(seqs[0])} {nouns[0]} for {len(seqs[1])} {nouns[1]}")
    B = len(seqs[0])
    if not B:
        return [], None
    if B > cap:
        raise ValueError(f"{fn}: {B} {nouns[2]} exceed the limit of {cap} per call")
    device = seqs[0][0].device if isinstance(seqs[0][0], torch.Tensor) else None
    members = []
    for b in range(B):
        m = rule(fn, *(s[b] for s in seqs), *(n if lone else f"{n}[{b}]" for n in names))
        on = [t.device for t in m[:checked]]
        if any(d != device for d in on):
            who = " / ".join(f"{n}[{b}]" for n in names[:checked])
            raise ValueError(f"{fn}: {who} {'lies' if checked == 1 else 'lie'} on {' / '.join(map(str, on))}, {names[0]}[0] on {device}")
        if max_L is not None and not 1 <= m[-1] <= max_L:
            raise ValueError(f"{fn}: {names[0]}[{b}]: L = {m[-1]} outside [1, {max_L}]")
        members.append(m)
    return members, device


def _carved(sizes: Sequence[int], device, dtype, align: int = 1) -> List[torch.Tensor]:
    """One allocation -> a view of sizes[b] elements per member, each starting on a multiple of `align` elements."""
    starts = [0]
    for n in sizes:
        starts.append(starts[-1] + -(-n // align) * align)
    buf = torch.empty(starts[-1], dtype=dtype, device=device)
    return [buf[s:s + n] for s, n in zip(starts, sizes)]


def _ss_operands(fn: str, atp: torch.Tensor, bc: torch.Tensor, name: str, bc_name: str):
    """The operand rules of one structure, for ss_head and for every member of ss_head_packed: -> (atp, base_codes, L) as the
    library reads them (maps whose rows or planes do not lie as [L, L] planes at least L*L apart are copied)."""
    _dev(atp, name)
    if atp.dim() != 3 or atp.shape[0] != 120 or atp.shape[1] != atp.shape[2]:
        raise ValueError(f"{fn}: {name} must be [120, L, L], got {tuple(atp.shape)}")
    L = atp.shape[-1]
    if atp.stride(2) != 1 or atp.stride(1) != L or atp.stride(0) < L * L:
        atp = atp.contiguous()
    _dev(bc, bc_name, torch.uint8)
    if bc.dim() != 1 or bc.shape[0] != L:
        raise ValueError(f"{fn}: {bc.shape[0] if bc.dim() == 1 else tuple(bc.shape)} base codes for {name} of L = {L}")
    return atp, bc.contiguous(), L


def _ss_entries(fn: str, gemm_dtype: str):
    """(lone, lone size, packed, packed size): the entry points of the SS head in the arithmetic `gemm_dtype`."""
    if gemm_dtype not in _lib.SS_GEMM_DTYPES:
        raise ValueError(f"{fn}: gemm_dtype must be one of {', '.join(_lib.SS_GEMM_DTYPES)}, got {gemm_dtype!r}")
    lib, stem = _lib.load(), "rnamsm_ss_head16" if gemm_dtype == "bf16" else "rnamsm_ss_head"
    return tuple(getattr(lib, stem + tail) for tail in ("", "_workspace_bytes", "_packed", "_packed_workspace_bytes"))


@_on_operand_device
def ss_pack_conv16(w: torch.Tensor) -> torch.Tensor:
    """The bf16 planes of a conv weight for rnamsm_ss_head16 (rnamsm_ss_pack_conv16): w fp32, tap-major [kh][kw][out][in],
    contiguous -> the same shape in bf16, each element rounded to nearest even on the device."""
    _dev(w, "w")
    if not w.is_contiguous():
        raise ValueError("ss_pack_conv16: w must be contiguous")
    out = torch.empty(w.shape, device=w.device, dtype=torch.bfloat16)
    _lib.check(_lib.load().rnamsm_ss_pack_conv16(w.data_ptr(), out.data_ptr(), w.numel(), _stream()))
    return out


def _ss_head_run(fn: str, head, head_bytes, atp: torch.Tensor, base_codes: torch.Tensor, ptrs, num_blocks: int, want: str) -> torch.Tensor:
    """The lone SS head through the entry point `head` and its size function (the route: fp32, bf16 or long; the library holds each
    to its own limit of L).  The workspace is 384 L^2 bytes: 6.4 GB at L = 4096."""
    atp, base_codes, L = _ss_operands(fn, atp, base_codes, "atp", "base_codes")
    ws = torch.empty(max(head_bytes(L), 16), dtype=torch.uint8, device=atp.device)
    out = torch.empty(L, L, device=atp.device, dtype=torch.float32)
    ptr = out.data_ptr()
    _lib.check(head(atp.data_ptr(), atp.stride(0), base_codes.data_ptr(), L, num_blocks, ptrs,
                    ptr if want == "logits" else None, ptr if want == "probs" else None, ws.data_ptr(), ws.numel(), _stream()))
    return out


@_on_operand_device
def ss_head(atp: torch.Tensor, base_codes: torch.Tensor, ptrs, num_blocks: int, want: str = "probs",
            gemm_dtype: str = "f32") -> torch.Tensor:
    """RNA-MSM-SS head (rnamsm_ss_head): atp [120, L, L] fp32 (planes may lie further apart than L*L: a slice of a wider
    buffer is read in place), base_codes uint8 [L] (0..3 = A, C, G, U, other = no base), ptrs: the packed weight table
    (ctypes c_void_p array, rnamsm.ss.SSPredictor) -> [L, L] fp32 probabilities (want="probs") or logits (want="logits").
    gemm_dtype="bf16": rnamsm_ss_head16, with ptrs the table whose conv entries are bf16 planes (ss_pack_conv16)."""
    _want("ss_head", want)
    head, head_bytes, _, _ = _ss_entries("ss_head", gemm_dtype)
    return _ss_head_run("ss_head", head, head_bytes, atp, base_codes, ptrs, num_blocks, want)


@_on_operand_device
def ss_head_long(atp: torch.Tensor, base_codes: torch.Tensor, ptrs, num_blocks: int, want: str = "probs") -> torch.Tensor:
    """ss_head for L up to LONG_MAX_L (rnamsm_ss_head_long, exact fp32 only: ptrs is the fp32 weight table)."""
    _want("ss_head_long", want)
    lib = _lib.load()
    return _ss_head_run("ss_head_long", lib.rnamsm_ss_head_long, lib.rnamsm_ss_head_long_workspace_bytes, atp, base_codes, ptrs,
                        num_blocks, want)


@_on_operand_device
def ss_head_packed(atps: Sequence[torch.Tensor], codes: Sequence[torch.Tensor], ptrs, num_blocks: int,
                   want: str = "probs", gemm_dtype: str = "f32") -> List[torch.Tensor]:
    """RNA-MSM-SS head over several structures in one set of launches (rnamsm_ss_head_packed): atps[b] [120, L_b, L_b] fp32,
    codes[b] uint8 [L_b], the operand rules of ss_head per member (slices of one wider buffer are read in place) -> a list of
    [L_b, L_b] tensors, each bit-identical to ss_head on that member alone.  One workspace and one output allocation per call:
    the returned tensors are views of one buffer.  gemm_dtype="bf16": rnamsm_ss_head16_packed, ptrs as for ss_head."""
    _want("ss_head_packed", want)
    _, _, packed, packed_bytes = _ss_entries("ss_head_packed", gemm_dtype)
    members, device = _members("ss_head_packed", _ss_operands, _lib.SS_MAX_BATCH, _lib.SS_MAX_L,
                               ("maps", "base-code rows", "structures"), {"atp": atps, "base_codes": codes})
    if not members:
        return []
    B, Ls = len(members), [L for _, _, L in members]
    ws = torch.empty(packed_bytes(B, (_lib.c_int * B)(*Ls)), dtype=torch.uint8, device=device)
    outs = [o.view(L, L) for o, L in zip(_carved([L * L for L in Ls], device, torch.float32), Ls)]
    items = (_lib.SsItem * B)()
    for b, ((atp, bc, L), o) in enumerate(zip(members, outs)):
        items[b] = _lib.SsItem(atp.data_ptr(), atp.stride(0), bc.data_ptr(), L, o.data_ptr() if want == "logits" else None,
                               o.data_ptr() if want == "probs" else None)
    _lib.check(packed(items, B, num_blocks, ptrs, ws.data_ptr(), ws.numel(), _stream()))
    return outs


def _ss_text_operand(fn: str, probs: torch.Tensor, name: str, max_L: int = _lib.SS_MAX_L):
    """One [L, L] matrix of ss_prob_text / ss_prob_text_packed as the library reads it -> (probs, L)."""
    _dev(probs, name)
    if probs.dim() != 2 or probs.shape[0] != probs.shape[1]:
        raise ValueError(f"{fn}: {name} must be [L, L], got {tuple(probs.shape)}")
    L = probs.shape[0]
    if not 1 <= L <= max_L:
        raise ValueError(f"{fn}: {name}: L = {L} outside [1, {max_L}]")
    return probs.contiguous(), L


_SS_TEXT = _Route("ss_prob_text", _lib.SS_MAX_L, "rnamsm_ss_prob_text_bytes")
_SS_TEXT_LONG = _Route("ss_prob_text_long", _lib.LONG_MAX_L, "rnamsm_ss_prob_text_long_bytes")


def _ss_prob_text_run(route: _Route, probs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    probs, L = _ss_text_operand(route.fn, probs, "probs", route.max_L)
    lib = _lib.load()
    text = torch.empty(getattr(lib, route.size)(L), dtype=torch.uint8, device=probs.device)
    fallback = torch.empty(1, dtype=torch.int32, device=probs.device)
    _lib.check(getattr(lib, route.entry)(probs.data_ptr(), L, text.data_ptr(), fallback.data_ptr(), _stream()))
    return text, fallback


@_on_operand_device
def ss_prob_text(probs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The `.prob` text of [L, L] fp32 probabilities, written on the device (rnamsm_ss_prob_text): -> (uint8 [25 L^2], the
    bytes of np.savetxt(f, probs, delimiter="\\t"); int32 [1], the fallback word: 1 when an element lies outside [0, 1] -- NaN,
    inf and -0.0 included -- and the text is then not to be used)."""
    return _ss_prob_text_run(_SS_TEXT, probs)


@_on_operand_device
def ss_prob_text_long(probs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """ss_prob_text for L up to LONG_MAX_L (rnamsm_ss_prob_text_long) -> (uint8 [25 L^2], the fallback word)."""
    return _ss_prob_text_run(_SS_TEXT_LONG, probs)


@_on_operand_device
def ss_prob_text_packed(probs: Sequence[torch.Tensor]) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """ss_prob_text of every probs[b] ([L_b, L_b]) in one call (rnamsm_ss_prob_text_packed) -> a list of (text, fallback word),
    each exactly what ss_prob_text gives for that matrix alone.  One text and one word allocation per call: the returned tensors
    are views (every text starts on a 16-byte boundary of the buffer)."""
    members, device = _members("ss_prob_text_packed", _ss_text_operand, _lib.SS_MAX_BATCH, None, (None, None, "matrices"),
                               {"probs": probs})
    if not members:
        return []
    B = len(members)
    lib = _lib.load()
    outs = list(zip(_carved([_lib.SS_TEXT_RECORD * L * L for _, L in members], device, torch.uint8, align=16),
                    _carved([1] * B, device, torch.int32)))
    items = (_lib.SsTextItem * B)()
    for b, ((p, L), (text, word)) in enumerate(zip(members, outs)):
        items[b] = _lib.SsTextItem(p.data_ptr(), L, text.data_ptr(), word.data_ptr())
    _lib.check(lib.rnamsm_ss_prob_text_packed(items, B, _stream()))
    return outs


def _ss_pairs_operands(fn: str, probs: torch.Tensor, letters: torch.Tensor, name: str, letters_name: str, max_L: int = _lib.SS_MAX_L):
    """One structure of ss_pairs / ss_pairs_packed / ss_pairs_long as the library reads it -> (probs, letters, L)."""
    probs, L = _ss_text_operand(fn, probs, name, max_L)
    _dev(letters, letters_name, torch.uint8)
    if letters.dim() != 1 or letters.shape[0] != L:
        raise ValueError(f"{fn}: {letters.shape[0] if letters.dim() == 1 else tuple(letters.shape)} letters for {name} of L = {L}")
    return probs, letters.contiguous(), L


@_on_operand_device
def ss_pairs(probs: torch.Tensor, letters: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The structure of [L, L] fp32 probabilities, decoded on the device (rnamsm_ss_pairs); letters uint8 [L]: the sequence's
    characters -> (partner int32 [L]: 0 or the partner's 1-based index; counts int32 [4]: pairs, bytes of the .ct body, bytes of
    the .bpseq body, fallback; the .ct body uint8 [32 L]; the .bpseq body uint8 [12 L]).  Only the first counts[1] / counts[2] bytes
    of the bodies are written; with counts[3] == 1 (a letter of 0 or >= 128) they are not to be used."""
    return _ss_pairs_run(_SS_PAIRS, [probs], [letters])[0]


@_on_operand_device
def ss_pairs_long(probs: torch.Tensor, letters: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """ss_pairs for L up to LONG_MAX_L (rnamsm_ss_pairs_long: several bases per thread), read as ss_pairs' results are."""
    return _ss_pairs_run(_SS_PAIRS_LONG, [probs], [letters])[0]


@_on_operand_device
def ss_pairs_packed(probs: Sequence[torch.Tensor], letters: Sequence[torch.Tensor]):
    """ss_pairs of every (probs[b], letters[b]) in one call (rnamsm_ss_pairs_packed: one workgroup per structure) -> a list of
    (partner, counts, ct body, bpseq body), each byte-identical to ss_pairs on that structure alone.  One allocation per output kind
    and one workspace per call: the returned tensors are views."""
    return _ss_pairs_run(None, probs, letters)


_SS_PAIRS = _Route("ss_pairs", _lib.SS_MAX_L)
_SS_PAIRS_LONG = _Route("ss_pairs_long", _lib.LONG_MAX_L)


def _ss_struct_outputs(members, device, n_counts: int, dbn: bool = False):
    """One allocation per output kind of a structure decoder -- partner [L], counts [n_counts], the .ct body [32 L], the .bpseq body
    [12 L] and, with dbn, the dot-bracket line [L] -> (a tuple of views per member, the arguments (probs, letters, L, *outputs) per
    member as the library takes them)."""
    Ls = [L for _, _, L in members]
    kinds = [_carved(Ls, device, torch.int32), _carved([n_counts] * len(Ls), device, torch.int32),
             _carved([_lib.SS_CT_LINE_MAX * L for L in Ls], device, torch.uint8),
             _carved([_lib.SS_BPSEQ_LINE_MAX * L for L in Ls], device, torch.uint8)] + ([_carved(Ls, device, torch.uint8)] if dbn else [])
    outs = list(zip(*kinds))
    return outs, [(p.data_ptr(), l.data_ptr(), L, *(t.data_ptr() for t in o)) for (p, l, L), o in zip(members, outs)]


def _ss_pairs_run(route: Optional[_Route], probs, letters):
    """route: the lone call's; None: the packed call."""
    fn = route.fn if route else "ss_pairs_packed"
    rule = functools.partial(_ss_pairs_operands, max_L=route.max_L) if route else _ss_pairs_operands
    members, device = _members(fn, rule, _lib.SS_MAX_BATCH, None, ("matrices", "letter rows", "structures"),
                               {"probs": probs, "letters": letters}, checked=2, lone=route is not None)
    if not members:
        return []
    B, Ls = len(members), [L for _, _, L in members]
    lib = _lib.load()
    nbytes = (lib.rnamsm_ss_pairs_long_workspace_bytes(Ls[0]) if route and route.long
              else lib.rnamsm_ss_pairs_workspace_bytes(B, (_lib.c_int * B)(*Ls)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    outs, args = _ss_struct_outputs(members, device, 4)
    if route:
        _lib.check(getattr(lib, route.entry)(*args[0], ws.data_ptr(), ws.numel(), _stream()))
        return outs
    items = (_lib.SsPairsItem * B)(*(_lib.SsPairsItem(*a) for a in args))
    _lib.check(lib.rnamsm_ss_pairs_packed(items, B, ws.data_ptr(), ws.numel(), _stream()))
    return outs


def _ss_nested_params(fn: str, theta: float, min_loop: int) -> Tuple[float, int]:
    theta = float(theta)
    if not 0.0 <= theta < 1.0:                                  # NaN fails both
        raise ValueError(f"{fn}: theta = {theta} outside [0, 1)")
    if int(min_loop) != min_loop or not 0 <= min_loop <= _lib.SS_NESTED_MAX_LOOP:
        raise ValueError(f"{fn}: min_loop = {min_loop} outside [0, {_lib.SS_NESTED_MAX_LOOP}]")
    return theta, int(min_loop)


@_on_operand_device
def ss_nested(probs: torch.Tensor, letters: torch.Tensor, theta: float = _lib.SS_NESTED_THETA, min_loop: int = _lib.SS_NESTED_MIN_LOOP):
    """The nested structure of greatest summed probability above theta, decoded on the device (rnamsm_ss_nested: include/rnamsm.h
    states the arithmetic); probs [L, L] fp32, L up to LONG_MAX_L, letters uint8 [L] -> (partner int32 [L]; counts int32 [5]: pairs,
    bytes of the .ct body, bytes of the .bpseq body, fallback, score; the .ct body uint8 [32 L]; the .bpseq body uint8 [12 L]; the
    dot-bracket line uint8 [L]).  The bodies are read as ss_pairs' are."""
    return _ss_nested_run("ss_nested", [probs], [letters], theta, min_loop, True)[0]


@_on_operand_device
def ss_nested_packed(probs: Sequence[torch.Tensor], letters: Sequence[torch.Tensor], theta: float = _lib.SS_NESTED_THETA,
                     min_loop: int = _lib.SS_NESTED_MIN_LOOP):
    """ss_nested of every (probs[b], letters[b]) in one call (rnamsm_ss_nested_packed: the member is a grid dimension, so the call
    costs the launches of its largest member) -> a list of ss_nested's tuples, each byte-identical to the lone call's.  One
    allocation per output kind and one workspace (8 Lp^2 bytes per member, Lp = L rounded up to 64) per call: the returned tensors
    are views."""
    return _ss_nested_run("ss_nested_packed", probs, letters, theta, min_loop, False)


def _ss_nested_run(fn: str, probs, letters, theta, min_loop, lone: bool, phase_events: Optional[list] = None):
    theta, min_loop = _ss_nested_params(fn, theta, min_loop)
    rule = functools.partial(_ss_pairs_operands, max_L=_lib.LONG_MAX_L)
    members, device = _members(fn, rule, _lib.SS_MAX_BATCH, None, ("matrices", "letter rows", "structures"),
                               {"probs": probs, "letters": letters}, checked=2, lone=lone)
    if not members:
        return []
    B, Ls = len(members), [L for _, _, L in members]
    lib = _lib.load()
    ws = torch.empty(lib.rnamsm_ss_nested_workspace_bytes(B, (_lib.c_int * B)(*Ls)), dtype=torch.uint8, device=device)
    outs, args = _ss_struct_outputs(members, device, 5, dbn=True)
    if lone:
        p, l, L, *o = args[0]
        _lib.check(lib.rnamsm_ss_nested(p, l, L, theta, min_loop, *o, ws.data_ptr(), ws.numel(), _stream()))
        return outs
    items = (_lib.SsNestedItem * B)(*(_lib.SsNestedItem(*a) for a in args))
    if phase_events is not None:          # the same launches in the same order, with an event recorded around each stage
        for phases in (1, 2):
            phase_events.append(_record_event())
            _lib.check(lib.rnamsm_ss_nested_phases(items, B, theta, min_loop, ws.data_ptr(), ws.numel(), phases, _stream()))
        phase_events.append(_record_event())
        return outs
    _lib.check(lib.rnamsm_ss_nested_packed(items, B, theta, min_loop, ws.data_ptr(), ws.numel(), _stream()))
    return outs


def _record_event() -> torch.cuda.Event:
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


@_on_operand_device
def ss_nested_phase_times(probs: Sequence[torch.Tensor], letters: Sequence[torch.Tensor], theta: float = _lib.SS_NESTED_THETA,
                          min_loop: int = _lib.SS_NESTED_MIN_LOOP):
    """ss_nested_packed with the fill and the traceback enqueued by two calls (rnamsm_ss_nested_phases) and an event around each, for
    tools/ss_nested_timing.py -> (ss_nested_packed's results, fill ms, traceback ms).  Synchronises the device."""
    events: list = []
    outs = _ss_nested_run("ss_nested_phase_times", probs, letters, theta, min_loop, False, events)
    torch.cuda.synchronize()
    return outs, events[0].elapsed_time(events[1]), events[1].elapsed_time(events[2])


def _rsa_operands(fn: str, emb: torch.Tensor, bc: torch.Tensor, name: str, bc_name: str):
    """The operand rules of one alignment, for rsa_head and for every member of rsa_head_packed: -> (emb, row stride, base_codes,
    L) as the library reads them (an embedding whose rows are not contiguous, overlap or do not start at a 16-byte boundary is
    copied)."""
    _dev(emb, name)
    if emb.dim() != 2 or emb.shape[1] != 768:
        raise ValueError(f"{fn}: {name} must be [L, 768], got {tuple(emb.shape)}")
    L = emb.shape[0]
    if emb.stride(1) != 1 or (L > 1 and emb.stride(0) < 768) or emb.data_ptr() % 16:
        emb = emb.contiguous()
    _dev(bc, bc_name, torch.uint8)
    if bc.dim() != 1 or bc.shape[0] != L:
        raise ValueError(f"{fn}: {tuple(bc.shape)} base codes for {name} of L = {L}")
    return emb, emb.stride(0) if L > 1 else 768, bc.contiguous(), L


_RSA_HEAD = _Route("rsa_head", _lib.RSA_MAX_L, "rnamsm_rsa_head_workspace_bytes")
_RSA_HEAD_LONG = _Route("rsa_head_long", _lib.LONG_MAX_L, "rnamsm_rsa_head_long_workspace_bytes")


def _long_range(route: _Route, t, name: str, dim: int) -> None:
    """The range of a long RSA call, before anything else is asked of the operand: a length out of range is wrong on any device."""
    if route.long and isinstance(t, torch.Tensor) and t.dim() == 2 and not 1 <= t.shape[dim] <= route.max_L:
        raise ValueError(f"{route.fn}: {name}: L = {t.shape[dim]} outside [1, {route.max_L}]")


def _rsa_head_run(route: _Route, emb: torch.Tensor, base_codes: torch.Tensor, ptrs, n_models: int, use_onehot: bool, want: str) -> torch.Tensor:
    _want(route.fn, want)
    _long_range(route, emb, "emb", 0)
    emb, stride, base_codes, L = _rsa_operands(route.fn, emb, base_codes, "emb", "base_codes")
    lib = _lib.load()
    ws = torch.empty(max(getattr(lib, route.size)(L, n_models), 16), dtype=torch.uint8, device=emb.device)
    out = torch.empty(n_models, L, device=emb.device, dtype=torch.float32)
    ptr = out.data_ptr()
    _lib.check(getattr(lib, route.entry)(emb.data_ptr(), stride, base_codes.data_ptr(), L, n_models, 1 if use_onehot else 0, ptrs,
                                         ptr if want == "probs" else None, ptr if want == "logits" else None, ws.data_ptr(),
                                         ws.numel(), _stream()))
    return out


@_on_operand_device
def rsa_head(emb: torch.Tensor, base_codes: torch.Tensor, ptrs, n_models: int, use_onehot: bool, want: str = "probs") -> torch.Tensor:
    """RNA-MSM RSA ensemble (rnamsm_rsa_head): emb [L, 768] fp32 (rows may lie further apart than 768 floats: a slice of the
    final representation is read in place), base_codes uint8 [L], ptrs: the packed weight table of the n_models members
    (rnamsm.rsa.RSAEnsemble) -> [n_models, L] fp32 RSA (want="probs") or the pre-sigmoid values (want="logits")."""
    return _rsa_head_run(_RSA_HEAD, emb, base_codes, ptrs, n_models, use_onehot, want)


@_on_operand_device
def rsa_head_long(emb: torch.Tensor, base_codes: torch.Tensor, ptrs, n_models: int, use_onehot: bool, want: str = "probs") -> torch.Tensor:
    """rsa_head for L up to LONG_MAX_L (rnamsm_rsa_head_long: the same four stages on a workspace with 128 tile-sum rows per
    model) -> [n_models, L]; the bits of rsa_head for an L both accept."""
    return _rsa_head_run(_RSA_HEAD_LONG, emb, base_codes, ptrs, n_models, use_onehot, want)


@_on_operand_device
def rsa_head_packed(embs: Sequence[torch.Tensor], codes: Sequence[torch.Tensor], ptrs, n_models: int, use_onehot: bool,
                    want: str = "probs") -> List[torch.Tensor]:
    """RNA-MSM RSA ensemble over several alignments in one set of four launches (rnamsm_rsa_head_packed): embs[b] [L_b, 768] fp32,
    codes[b] uint8 [L_b], the operand rules of rsa_head per member (row slices of one wider buffer are read in place) -> a list of
    [n_models, L_b] tensors, each bit-identical to rsa_head on that member alone.  One workspace and one output allocation per
    call: the returned tensors are views of one buffer."""
    _want("rsa_head_packed", want)
    members, device = _members("rsa_head_packed", _rsa_operands, _lib.RSA_MAX_BATCH, _lib.RSA_MAX_L,
                               ("embeddings", "base-code rows", "alignments"), {"emb": embs, "base_codes": codes})
    if not members:
        return []
    B, Ls = len(members), [m[-1] for m in members]
    lib = _lib.load()
    ws = torch.empty(lib.rnamsm_rsa_head_packed_workspace_bytes(B, (_lib.c_int * B)(*Ls), n_models), dtype=torch.uint8, device=device)
    outs = [o.view(n_models, L) for o, L in zip(_carved([n_models * L for L in Ls], device, torch.float32), Ls)]
    items = (_lib.RsaItem * B)()
    for b, ((emb, stride, bc, L), o) in enumerate(zip(members, outs)):
        items[b] = _lib.RsaItem(emb.data_ptr(), stride, bc.data_ptr(), L,
                                o.data_ptr() if want == "probs" else None, o.data_ptr() if want == "logits" else None)
    _lib.check(lib.rnamsm_rsa_head_packed(items, B, n_models, 1 if use_onehot else 0, ptrs, ws.data_ptr(), ws.numel(), _stream()))
    return outs


def _rsa_text_operands(fn: str, rsa: torch.Tensor, letters: torch.Tensor, name: str, letters_name: str, max_L: int = _lib.RSA_MAX_L):
    """One alignment of rsa_text / rsa_text_packed / rsa_text_long as the library reads it -> (rsa, letters, K, L)."""
    _dev(rsa, name)
    if rsa.dim() != 2:
        raise ValueError(f"{fn}: {name} must be [n_models, L], got {tuple(rsa.shape)}")
    K, L = rsa.shape
    if not 1 <= K <= _lib.RSA_MAX_MODELS:
        raise ValueError(f"{fn}: {name}: {K} members outside [1, {_lib.RSA_MAX_MODELS}]")
    if not 1 <= L <= max_L:
        raise ValueError(f"{fn}: {name}: L = {L} outside [1, {max_L}]")
    _dev(letters, letters_name, torch.uint8)
    if letters.dim() != 1 or letters.shape[0] != L:
        raise ValueError(f"{fn}: {letters.shape[0] if letters.dim() == 1 else tuple(letters.shape)} letters for {name} of L = {L}")
    return rsa.contiguous(), letters.contiguous(), K, L


@_on_operand_device
def rsa_text(rsa: torch.Tensor, letters: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The bodies of the RSA_result tables of the members' [K, L] fp32 RSA, written on the device (rnamsm_rsa_text); letters uint8
    [L]: the sequence's characters -> (text uint8 [(K + 1) x 23 L]: body f -- member f, the ensemble last -- starts at f x 23 L;
    counts int32 [K + 3]: the bytes of each body, the fallback word, the zero word; ens float64 [2, L]: the ensemble's ASA and
    RSA).  Only the first counts[f] bytes of a body are written; with counts[K + 1] == 1 (a value outside [0, 1] or a letter outside
    ACGUT) text and ens are not to be used, and counts[K + 2] == 1 says that an ASA is exactly 0."""
    return _rsa_text_run(_RSA_TEXT, [rsa], [letters])[0]


@_on_operand_device
def rsa_text_long(rsa: torch.Tensor, letters: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """rsa_text for L up to LONG_MAX_L (rnamsm_rsa_text_long: the same kernel, as many passes of 256 positions as L needs), read
    as rsa_text's results are."""
    return _rsa_text_run(_RSA_TEXT_LONG, [rsa], [letters])[0]


@_on_operand_device
def rsa_text_packed(rsa: Sequence[torch.Tensor], letters: Sequence[torch.Tensor]):
    """rsa_text of every (rsa[b], letters[b]) in one call (rnamsm_rsa_text_packed: one workgroup per alignment and table; all the
    members of one K) -> a list of (text, counts, ens), each byte-identical to rsa_text on that alignment alone.  One allocation per
    output kind for the whole group: the returned tensors are views (every text starts on a 16-byte boundary of the buffer)."""
    return _rsa_text_run(None, rsa, letters)


_RSA_TEXT = _Route("rsa_text", _lib.RSA_MAX_L)
_RSA_TEXT_LONG = _Route("rsa_text_long", _lib.LONG_MAX_L)


def _rsa_text_run(route: Optional[_Route], rsa, letters):
    """route: the lone call's; None: the packed call."""
    _fn = route.fn if route else "rsa_text_packed"
    rule = _rsa_text_operands
    if route:
        _long_range(route, rsa[0], "rsa", 1)
        rule = functools.partial(_rsa_text_operands, max_L=route.max_L)
    members, device = _members(_fn, rule, _lib.RSA_MAX_BATCH, None, ("value tables", "letter rows", "alignments"),
                               {"rsa": rsa, "letters": letters}, checked=2, lone=route is not None)
    if not members:
        return []
    B, K = len(members), members[0][2]
    if any(m[2] != K for m in members):
        raise ValueError(f"{_fn}: the alignments of one call share n_models; got {sorted({m[2] for m in members})}")
    Ls = [m[3] for m in members]
    lib = _lib.load()
    outs = list(zip(_carved([(K + 1) * _lib.RSA_TEXT_LINE_MAX * L for L in Ls], device, torch.uint8, align=16),
                    _carved([K + 3] * B, device, torch.int32),
                    (e.view(2, L) for e, L in zip(_carved([2 * L for L in Ls], device, torch.float64), Ls))))
    args = [(r.data_ptr(), l.data_ptr(), L, *(t.data_ptr() for t in o)) for (r, l, _, L), o in zip(members, outs)]
    if route:
        r, l, L, text, counts, ens = args[0]
        _lib.check(getattr(lib, route.entry)(r, l, L, K, text, counts, ens, _stream()))
        return outs
    items = (_lib.RsaTextItem * B)(*(_lib.RsaTextItem(*a) for a in args))
    _lib.check(lib.rnamsm_rsa_text_packed(items, B, K, _stream()))
    return outs


class LMWeights(NamedTuple):
    """The LM head's weights as rnamsm_lm_head reads them: the six tensors in _lib.W_LM's order (kept alive here), the pointer
    table, eps and the shape."""
    tensors: tuple
    ptrs: object
    eps: float
    D: int
    V: int


def lm_weights(dense_w: torch.Tensor, dense_b: torch.Tensor, ln_g: torch.Tensor, ln_b: torch.Tensor, proj_w: torch.Tensor,
               proj_b: torch.Tensor, eps: float = 1e-5) -> LMWeights:
    """Check and pin the weights of the LM head: dense [D, D] + [D], LayerNorm gamma / beta [D], projection [V, D] + [V] (the tied
    embedding rows as they are), fp32 on one HIP device, D a multiple of 64 up to LM_MAX_D, V up to LM_MAX_V."""
    ts = tuple(t.detach().contiguous() for t in (dense_w, dense_b, ln_g, ln_b, proj_w, proj_b))
    for t, name in zip(ts, _lib.W_LM):
        _dev(t, f"lm_head.{name}")
        if t.device != ts[0].device:
            raise ValueError(f"lm_weights: lm_head.{name} lies on {t.device}, lm_head.{_lib.W_LM[0]} on {ts[0].device}")
    D = ts[0].shape[0]
    V = ts[4].shape[0] if ts[4].dim() == 2 else -1
    want = ((D, D), (D,), (D,), (D,), (V, D), (V,))
    for t, name, shape in zip(ts, _lib.W_LM, want):
        if tuple(t.shape) != shape:
            raise ValueError(f"lm_weights: lm_head.{name} is {tuple(t.shape)}, expected {shape}")
    if D % 64 or not 64 <= D <= _lib.LM_MAX_D or not 1 <= V <= _lib.LM_MAX_V:
        raise ValueError(f"lm_weights: D = {D} must be a multiple of 64 in [64, {_lib.LM_MAX_D}] and V = {V} lie in [1, {_lib.LM_MAX_V}]")
    ptrs = (_lib.c_void_p * len(ts))(*(t.data_ptr() for t in ts))
    return LMWeights(ts, ptrs, float(eps), D, V)


def _lm_want(fn: str, want, has_wt: bool) -> tuple:
    if want is None:
        want = _lib.LM_OUTPUTS if has_wt else _lib.LM_OUTPUTS[:2]
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in _lib.LM_OUTPUTS for w in want) or len(set(want)) != len(want):
        raise ValueError(f"{fn}: want must be a non-empty selection of {_lib.LM_OUTPUTS}, got {want!r}")
    if not has_wt and ("scores" in want or "nll" in want):
        raise ValueError(f"{fn}: scores / nll need wt (the wild-type token of every row)")
    return want


def _lm_operands(D: int, fn: str, x: torch.Tensor, rows, name: str, rows_name: str):
    """The operand rules of one member of lm_head_rows / lm_head_packed: -> (x, rows, ld, n) as the library reads them.  x [N, D]
    fp32 is read in place when its rows are contiguous, at least D apart by a multiple of 4 floats and 16-byte aligned (a column
    or row slice of a wider buffer), else copied; rows (None: every row in order) become device int32 and must name rows of x."""
    _dev(x, name)
    if x.dim() != 2 or x.shape[1] != D or x.shape[0] < 1:
        raise ValueError(f"{fn}: {name} must be [N, {D}] with N >= 1, got {tuple(x.shape)}")
    N = x.shape[0]
    if x.stride(1) != 1 or (N > 1 and (x.stride(0) < D or x.stride(0) % 4)) or x.data_ptr() % 16:
        x = x.contiguous()
    ld = x.stride(0) if N > 1 else D
    if rows is None:
        return x, None, ld, N
    rows = torch.as_tensor(rows)
    if rows.dim() != 1 or rows.numel() < 1 or rows.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{fn}: {rows_name} must be a non-empty 1-D int32 / int64 index, got {tuple(rows.shape)} {rows.dtype}")
    lo, hi = int(rows.min()), int(rows.max())           # (a device index costs one read-back: the kernel trusts what it is given)
    if lo < 0 or hi >= N:
        raise IndexError(f"{fn}: {rows_name} reaches [{lo}, {hi}], {name} has rows [0, {N})")
    return x, rows.to(device=x.device, dtype=torch.int32).contiguous(), ld, rows.numel()


def _lm_wt(fn: str, wt, n: int, device, name: str):
    if wt is None:
        return None
    wt = torch.as_tensor(wt)
    if wt.dim() != 1 or wt.numel() != n or wt.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{fn}: {name} must be a 1-D int32 / int64 tensor of {n} tokens, got {tuple(wt.shape)} {wt.dtype}")
    return wt.to(device=device, dtype=torch.int32).contiguous()


def _lm_item(x, ld, rows, wt, n, outs: dict) -> "_lib.LmItem":
    return _lib.LmItem(x.data_ptr(), ld, None if rows is None else rows.data_ptr(), None if wt is None else wt.data_ptr(), n,
                       *(outs[k].data_ptr() if k in outs else None for k in _lib.LM_OUTPUTS))


@_on_operand_device
def lm_head_rows(x: torch.Tensor, rows, wt, weights: LMWeights, want=None) -> dict:
    """The LM head on chosen rows (rnamsm_lm_head): x [N, D] fp32 (a slice of a wider buffer is read in place), rows: the n rows to
    run on (None: all N in order; repeats and any order allowed), wt: the wild-type token of each of the n rows (None: no scores /
    nll), weights: lm_weights(...).  -> {name: tensor} for every name in `want` (default: all the inputs allow): logits, logp,
    scores [n, V], nll [n].  What is not wanted is not computed; a wt outside [0, V) gives a NaN row of scores and nll."""
    members, device = _members("lm_head_rows", functools.partial(_lm_operands, weights.D), 1, _lib.LM_MAX_ROWS,
                               ("feature buffers", "row tables", "members"), {"x": [x], "rows": [rows]}, lone=True)
    x, rows, ld, n = members[0]
    wt = _lm_wt("lm_head_rows", wt, n, device, "wt")
    want = _lm_want("lm_head_rows", want, wt is not None)
    V = weights.V
    outs = {k: torch.empty((n,) if k == "nll" else (n, V), device=device, dtype=torch.float32) for k in want}
    lib = _lib.load()
    ws = torch.empty(lib.rnamsm_lm_head_workspace_bytes(n, weights.D), dtype=torch.uint8, device=device)
    item = _lm_item(x, ld, rows, wt, n, outs)
    _lib.check(lib.rnamsm_lm_head(item, weights.D, V, weights.ptrs, weights.eps, ws.data_ptr(), ws.numel(), _stream()))
    return outs


@_on_operand_device
def lm_head_packed(xs: Sequence[torch.Tensor], rows: Sequence, wts: Sequence, weights: LMWeights, want=None) -> List[dict]:
    """The LM head over several members in one launch set (rnamsm_lm_head_packed): the operand rules of lm_head_rows per member
    (rows[b] / wts[b] may be None; wts all or none) -> a list of {name: tensor}, each tensor bit-identical to lm_head_rows on that
    member alone.  One workspace and one allocation per output kind: the returned tensors are views."""
    xs = list(xs)
    rows = [None] * len(xs) if rows is None else list(rows)
    wts = [None] * len(xs) if wts is None else list(wts)
    members, device = _members("lm_head_packed", functools.partial(_lm_operands, weights.D), _lib.LM_MAX_BATCH, _lib.LM_MAX_ROWS,
                               ("feature buffers", "row tables", "members"), {"x": xs, "rows": rows})
    if not members:
        return []
    B, ns, V = len(members), [m[-1] for m in members], weights.V
    if len(wts) != B:
        raise ValueError(f"lm_head_packed: {len(wts)} wild-type rows for {B} members")
    if sum(ns) > _lib.LM_MAX_ROWS:
        raise ValueError(f"lm_head_packed: {sum(ns)} rows exceed the limit of {_lib.LM_MAX_ROWS} per call")
    has_wt = all(w is not None for w in wts)
    if not has_wt and any(w is not None for w in wts):
        raise ValueError("lm_head_packed: wts must be given for every member or for none")
    wts = [_lm_wt("lm_head_packed", w, n, device, f"wt[{b}]") for b, (w, n) in enumerate(zip(wts, ns))]
    want = _lm_want("lm_head_packed", want, has_wt)
    carved = {k: _carved([n if k == "nll" else n * V for n in ns], device, torch.float32) for k in want}
    outs = [{k: carved[k][b] if k == "nll" else carved[k][b].view(ns[b], V) for k in want} for b in range(B)]
    lib = _lib.load()
    ws = torch.empty(lib.rnamsm_lm_head_packed_workspace_bytes(B, (_lib.c_int * B)(*ns), weights.D), dtype=torch.uint8, device=device)
    items = (_lib.LmItem * B)()
    for b, ((x, r, ld, n), w) in enumerate(zip(members, wts)):
        items[b] = _lm_item(x, ld, r, w, n, outs[b])
    _lib.check(lib.rnamsm_lm_head_packed(items, B, weights.D, V, weights.ptrs, weights.eps, ws.data_ptr(), ws.numel(), _stream()))
    return outs


def _stitch_out(fn: str, out: torch.Tensor, shape: tuple) -> None:
    _dev(out, "out")
    if tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"{fn}: out must be a contiguous {shape} tensor, got {tuple(out.shape)} with strides {out.stride()}")


@_on_operand_device
def stitch_rows(x: torch.Tensor, out: torch.Tensor, stride: int, k0: int = 0) -> torch.Tensor:
    """rnamsm_stitch_rows: x [nb, W, D] fp32 -- the emb of the windows k0 .. k0 + nb - 1 of the plan (L = out.shape[0], W, stride),
    read where they lie (rows and windows may be further apart: a slice of a wider buffer) -- blended into out [L, D].  Calls come
    in ascending k0 and together apply every window once; between them `out` holds running sums."""
    _dev(x, "x")
    if x.dim() != 3 or out.dim() != 2 or x.shape[2] != out.shape[1]:
        raise ValueError(f"stitch_rows: x [nb, W, D] and out [L, D], got {tuple(x.shape)} and {tuple(out.shape)}")
    if x.stride(2) != 1:
        x = x.contiguous()
    nb, W, D = x.shape
    _stitch_out("stitch_rows", out, (out.shape[0], D))
    _lib.check(_lib.load().rnamsm_stitch_rows(x.data_ptr(), x.stride(0), x.stride(1), out.shape[0], W, int(stride), int(k0), nb, D,
                                              out.data_ptr(), _stream()))
    return out


@_on_operand_device
def stitch_pairs(a: torch.Tensor, out: torch.Tensor, stride: int, k0: int = 0, off: int = 0) -> torch.Tensor:
    """rnamsm_stitch_pairs: a [nb, H, W + off, W + off] fp32 -- the maps of the windows k0 .. k0 + nb - 1, read where they lie
    through their own strides, skipping `off` leading rows and columns (0: the stripped atp; 1: maps that still carry <cls>) --
    blended into out [H, L, L]; pairs no window contains come out +0.0.  Calls as for stitch_rows."""
    _dev(a, "a")
    if a.dim() != 4 or out.dim() != 3 or a.shape[1] != out.shape[0] or a.shape[2] != a.shape[3] or out.shape[1] != out.shape[2]:
        raise ValueError(f"stitch_pairs: a [nb, H, W, W] and out [H, L, L], got {tuple(a.shape)} and {tuple(out.shape)}")
    if a.stride(3) != 1:
        a = a.contiguous()
    nb, H, Wo, _ = a.shape
    _stitch_out("stitch_pairs", out, (H, out.shape[1], out.shape[1]))
    plane = a.stride(1) if H > 1 else max(a.stride(1), Wo * a.stride(2))      # (the stride of a dimension of one is not binding)
    _lib.check(_lib.load().rnamsm_stitch_pairs(a.data_ptr(), a.stride(0), plane, a.stride(2), int(off), out.shape[1],
                                               Wo - int(off), int(stride), int(k0), nb, H, out.data_ptr(), _stream()))
    return out


@_on_operand_device
def greedy_select(msa_u8: torch.Tensor, num_seqs: int, mode: str = "max") -> torch.Tensor:
    """msa uint8 [N, L] on the device -> int32 [num_seqs] ascending row indices (utils/align.py:128-148)."""
    if mode not in ("max", "min"):
        raise AssertionError(mode)
    N, L = msa_u8.shape
    lib = _lib.load()
    ws = torch.empty(lib.rnamsm_greedy_select_workspace_bytes(N, L, num_seqs), dtype=torch.uint8, device=msa_u8.device)
    out = torch.empty(num_seqs, dtype=torch.int32, device=msa_u8.device)
    _lib.check(lib.rnamsm_greedy_select(_dev(msa_u8.contiguous(), "msa", torch.uint8), N, L, num_seqs,
                                        1 if mode == "min" else 0, _dev(out, "out", torch.int32), ws.data_ptr(),
                                        ws.numel(), _stream()))
    return out


@_on_operand_device
def msa_weights(msa_u8: torch.Tensor, seqid_cutoff: float = 0.2) -> torch.Tensor:
    """msa uint8 [N, L] on the device -> float64 [N] sequence weights (MSA.weights, utils/align.py:250-253); L <= 32768.
    The reference's pdist runs over the raw character bytes (utils/align.py:121-126); callers here pass TOKEN ids.  The
    two agree for the alphabet that survives from_fasta's regexes (A/C/G/U/X/-, one token per character); characters that
    fall to <unk> would be merged by the token form -- the reader raises for those before this is reached."""
    N, L = msa_u8.shape
    out = torch.empty(N, dtype=torch.float64, device=msa_u8.device)
    _lib.check(_lib.load().rnamsm_msa_weights(_dev(msa_u8.contiguous(), "msa", torch.uint8), N, L, float(seqid_cutoff),
                                              _dev(out, "weights", torch.float64), _stream()))
    return out


@_on_operand_device
def msa_invcov(tokens_u8: torch.Tensor, gap: int, want_counts: bool = False):
    """Covariance contacts (MSA.invcov, utils/align.py:183-193; rnamsm_msa_invcov): tokens uint8 [N, L] on the device (rows may be
    strided: a view with contiguous rows is read where it lies) -> float64 [L, L], exactly symmetric.  N in [2, 2^20], L in [1, 4096],
    at most 16 distinct values other than `gap`; the library refuses anything else and the message names the reason.
    want_counts: also stage 1 -- (map, counts int32 [L, L, K, K], symbols int32 [K] ascending), counts[i, j, a, b] = the number of rows
    with symbols[a] in column i and symbols[b] in column j.  The call waits for the device once (K is read back)."""
    _dev(tokens_u8, "tokens", torch.uint8)
    if tokens_u8.dim() != 2 or (tokens_u8.shape[1] > 1 and tokens_u8.stride(1) != 1) or tokens_u8.stride(0) < tokens_u8.shape[1]:
        tokens_u8 = tokens_u8.contiguous()
    N, L = tokens_u8.shape
    ld = tokens_u8.stride(0) if N > 1 else L
    lib = _lib.load()
    dev = tokens_u8.device
    ws = torch.empty(max(lib.rnamsm_msa_invcov_workspace_bytes(N, L), 256), dtype=torch.uint8, device=dev)
    out = torch.empty((L, L), dtype=torch.float64, device=dev)
    counts = None
    if want_counts:
        vals = torch.unique(tokens_u8[:, :L])
        K = int((vals != int(gap)).sum())
        counts = torch.empty(_lib.INVCOV_META + L * L * K * K * (1 <= K <= _lib.INVCOV_MAX_K), dtype=torch.int32, device=dev)
    _lib.check(lib.rnamsm_msa_invcov(tokens_u8.data_ptr(), N, L, ld, int(gap), out.data_ptr(),
                                     counts.data_ptr() if want_counts else None, ws.data_ptr(), ws.numel(), _stream()))
    if not want_counts:
        return out
    return out, counts[_lib.INVCOV_META:].view(L, L, K, K), counts[1:1 + K]


def _msa_rows(msa_u8: torch.Tensor, name: str):
    """uint8 [N, L] on the device as the alignment statistics read it: (tensor, N, L, ld).  A view with contiguous rows is read where
    it lies (ld = its row stride); anything else is copied."""
    _dev(msa_u8, name, torch.uint8)
    if msa_u8.dim() != 2:
        raise ValueError(f"{name}: expected uint8 [N, L], got {tuple(msa_u8.shape)}")
    if (msa_u8.shape[1] > 1 and msa_u8.stride(1) != 1) or msa_u8.stride(0) < msa_u8.shape[1]:
        msa_u8 = msa_u8.contiguous()
    N, L = msa_u8.shape
    return msa_u8, N, L, (msa_u8.stride(0) if N > 1 else L)


def _aligned_workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


class MsaMi(NamedTuple):
    """What rnamsm_msa_mi writes, on the device; a map that was not asked for is None."""
    mi: Optional[torch.Tensor]     # float64 [L, L]: the mutual information of every pair of columns
    mip: Optional[torch.Tensor]    # float64 [L, L]: apc of mi with a zero diagonal


@_on_operand_device
def msa_mi(tokens_u8: torch.Tensor, gap: int, gaps: str = "pairwise", want=("mi", "mip")) -> MsaMi:
    """Mutual-information contacts (rnamsm_msa_mi): tokens uint8 [N, L] on the device (a view with contiguous rows is read where it
    lies) -> MsaMi.  gaps="pairwise": rows with a gap in either column are left out of that pair; "state": the gap is one more state.
    want: which of "mi", "mip" to make.  mi is exactly symmetric, its diagonal the columns' entropies; mip = apc(mi with a zero
    diagonal), NaN everywhere where that map's total is 0.  N in [2, 2^20], L in [1, 4096], at most 16 distinct values other than
    `gap`; the library refuses anything else.  The call waits for the device once (K is read back)."""
    if gaps not in _lib.MI_GAP_MODES:
        raise ValueError(f"msa_mi: gaps={gaps!r} is not one of {', '.join(map(repr, _lib.MI_GAP_MODES))}")
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in ("mi", "mip") for w in want):
        raise ValueError(f"msa_mi: want={want!r} is not a non-empty choice of 'mi', 'mip'")
    tokens_u8, N, L, ld = _msa_rows(tokens_u8, "msa_mi")
    lib = _lib.load()
    dev = tokens_u8.device
    ws = _aligned_workspace(lib.rnamsm_msa_mi_workspace_bytes(N, L), dev)
    rec = MsaMi(*(torch.empty((L, L), dtype=torch.float64, device=dev) if w in want else None for w in ("mi", "mip")))
    _lib.check(lib.rnamsm_msa_mi(tokens_u8.data_ptr(), N, L, ld, int(gap), _lib.MI_GAP_MODES[gaps],
                                 rec.mi.data_ptr() if rec.mi is not None else None, rec.mip.data_ptr() if rec.mip is not None else None,
                                 ws.data_ptr(), ws.numel(), _stream()))
    return rec


class MsaWmi(NamedTuple):
    """What rnamsm_msa_wmi writes, on the device; wcounts is None unless it was asked for."""
    mi: torch.Tensor                   # float64 [L, L]: the sequence-weighted mutual information of every pair of columns
    mip: torch.Tensor                  # float64 [L, L]: apc of mi with a zero diagonal
    wcounts: Optional[torch.Tensor]    # float64 [L, L, S, S]: the weighted pair counts; S = K ("pairwise") or K + 1 ("state", the gap last)
    wmarg: torch.Tensor                # float64 [L, S]: the weighted column profile, wcounts[i, i, a, a]
    symbols: torch.Tensor              # int32 [K] ascending


@_on_operand_device
def msa_wmi(tokens_u8: torch.Tensor, gap: int, gaps: str = "pairwise", weights: torch.Tensor = None, want_counts: bool = False,
            workspace_bytes: Optional[int] = None) -> MsaWmi:
    """Sequence-weighted mutual information (rnamsm_msa_wmi): msa_mi with row n counted weights[n] times.  tokens uint8 [N, L] on the
    device (a view with contiguous rows is read where it lies), weights float64 [N] on the device, every one finite and > 0 (the
    library refuses anything else and names the first such row) -> MsaWmi.  With every weight 1.0 mi and mip are msa_mi's bit for
    bit.  workspace_bytes: None = the library's default; any size from rnamsm_msa_wmi_min_workspace_bytes(N, L) upward gives the
    same bits in more bands of columns.  want_counts: the counts have to be sized before the call, so K is counted here first
    (torch.unique over the tokens, as ops.msa_invcov does: one more pass and one more wait).  N in [2, 2^20], L in [1, 4096], at most 16 distinct values other than `gap`.  The call
    waits for the device once (K and the weights' verdict are read back)."""
    if gaps not in _lib.MI_GAP_MODES:
        raise ValueError(f"msa_wmi: gaps={gaps!r} is not one of {', '.join(map(repr, _lib.MI_GAP_MODES))}")
    if weights is None:
        raise ValueError("msa_wmi: weights is required (float64 [N] on the device)")
    tokens_u8, N, L, ld = _msa_rows(tokens_u8, "msa_wmi")
    _dev(weights, "weights", torch.float64)
    if weights.dim() != 1 or weights.shape[0] != N:
        raise ValueError(f"msa_wmi: expected {N} weights, got {tuple(weights.shape)}")
    weights = weights.contiguous()
    lib = _lib.load()
    dev = tokens_u8.device
    ws = _aligned_workspace(lib.rnamsm_msa_wmi_workspace_bytes(N, L) if workspace_bytes is None else workspace_bytes, dev)
    S_max = _lib.INVCOV_MAX_K + 1
    mi, mip = (torch.empty((L, L), dtype=torch.float64, device=dev) for _ in range(2))
    wmarg = torch.empty(L * S_max, dtype=torch.float64, device=dev)
    meta = torch.zeros(_lib.INVCOV_META, dtype=torch.int32, device=dev)
    wcounts = None
    if want_counts:
        K = int((torch.unique(tokens_u8[:, :L]) != int(gap)).sum())
        S = K + (gaps == "state")
        wcounts = torch.empty(L * L * S * S * (1 <= K <= _lib.INVCOV_MAX_K), dtype=torch.float64, device=dev)
    _lib.check(lib.rnamsm_msa_wmi(tokens_u8.data_ptr(), N, L, ld, int(gap), _lib.MI_GAP_MODES[gaps], weights.data_ptr(), mi.data_ptr(),
                                  mip.data_ptr(), wcounts.data_ptr() if want_counts else None, wmarg.data_ptr(), meta.data_ptr(),
                                  ws.data_ptr(), ws.numel() if workspace_bytes is None else int(workspace_bytes), _stream()))
    found = int(meta[0].item())
    if want_counts and found != K:      # (both are "the distinct byte values other than gap": they cannot differ)
        raise RuntimeError(f"msa_wmi: the library found {found} symbols, the counts were sized for {K}")
    K = found
    S = K + (gaps == "state")
    return MsaWmi(mi, mip, wcounts.view(L, L, S, S) if want_counts else None, wmarg[:L * S].view(L, S), meta[1:1 + K])


@_on_operand_device
def apc(x: torch.Tensor, zero_diagonal: bool = False) -> torch.Tensor:
    """Average-product correction (the reference's apc, utils/tensor.py:103-113; rnamsm_apc_f64): x float64 [L, L] on the device,
    symmetric or not (a view with contiguous rows is read where it lies) -> x - row sums * column sums / total, float64 [L, L].
    zero_diagonal: the diagonal of x is read as 0.  A total of 0 gives NaN everywhere.  L in [1, 32768]."""
    _dev(x, "x", torch.float64)
    if x.dim() != 2 or x.shape[0] != x.shape[1]:
        raise ValueError(f"apc: expected a square float64 map, got {tuple(x.shape)}")
    L = x.shape[0]
    if (L > 1 and x.stride(1) != 1) or x.stride(0) < L:
        x = x.contiguous()
    lib = _lib.load()
    ws = _aligned_workspace(lib.rnamsm_apc_f64_workspace_bytes(L), x.device)
    out = torch.empty((L, L), dtype=torch.float64, device=x.device)
    _lib.check(lib.rnamsm_apc_f64(x.data_ptr(), L, x.stride(0) if L > 1 else L, int(bool(zero_diagonal)), out.data_ptr(), ws.data_ptr(),
                                  ws.numel(), _stream()))
    return out


class TopPairs(NamedTuple):
    """What rnamsm_top_pairs_f64 / _f32 write, on the device."""
    pairs: torch.Tensor            # int32 [k, 2]: (i, j) of the ranked pairs, 0-based; -1, -1 from row `count` on
    scores: torch.Tensor           # float64 [k]: their values; NaN from row `count` on
    count: torch.Tensor            # int32 scalar: min(k, the number of candidates)


@_on_operand_device
def top_pairs(x: torch.Tensor, k: int, min_sep: int = 1) -> TopPairs:
    """The top-k ranked pairs of a square map (rnamsm_top_pairs_f64 / _f32; include/rnamsm.h states the rule): x float32 or float64
    [L, L] on the device, read where it lies (ld = its row stride; a tensor whose last dimension is not contiguous is refused) ->
    TopPairs.  Candidates are the pairs i < j with j - i >= min_sep whose value is not NaN; larger value first (-0.0 as +0.0), then
    smaller i, then smaller j.  L in [2, 32768], k in [1, 65536], min_sep in [1, 32768]; the library refuses anything else.
    Asynchronous: nothing is read back, count stays on the device."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.RnamsmError("top_pairs: expected a tensor on the HIP device (no CPU path exists)")
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"top_pairs: expected float32 or float64, got {x.dtype}")
    if x.dim() != 2 or x.shape[0] != x.shape[1]:
        raise ValueError(f"top_pairs: expected a square map, got {tuple(x.shape)}")
    L = x.shape[0]
    if L > 1 and x.stride(1) != 1:
        raise ValueError(f"top_pairs: the rows of the map are not contiguous (strides {tuple(x.stride())})")
    lib = _lib.load()
    k, min_sep = int(k), int(min_sep)
    ws = _aligned_workspace(lib.rnamsm_top_pairs_workspace_bytes(L, k), x.device)
    n_rows = min(max(k, 1), _lib.TOP_PAIRS_MAX_K)           # (a k the library refuses still gets real pointers: its message names k)
    rec = TopPairs(torch.empty((n_rows, 2), dtype=torch.int32, device=x.device), torch.empty(n_rows, dtype=torch.float64, device=x.device),
                   torch.empty((), dtype=torch.int32, device=x.device))
    fn = lib.rnamsm_top_pairs_f64 if x.dtype == torch.float64 else lib.rnamsm_top_pairs_f32
    _lib.check(fn(x.data_ptr(), L, x.stride(0) if L > 1 else L, min_sep, k, rec.pairs.data_ptr(), rec.scores.data_ptr(),
                  rec.count.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return rec


def _pair_map_and_target(x, target, what: str):
    """The operand checks pair_sweep and pair_precision share -> (L, ld, ld_t)."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or not isinstance(target, torch.Tensor) or not target.is_cuda:
        raise _lib.RnamsmError(f"{what}: expected the map and the target on the HIP device (no CPU path exists)")
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what}: expected a float32 or float64 map, got {x.dtype}")
    if target.dtype != torch.int8:
        raise TypeError(f"{what}: expected an int8 target, got {target.dtype}")
    if x.dim() != 2 or x.shape[0] != x.shape[1]:
        raise ValueError(f"{what}: expected a square map, got {tuple(x.shape)}")
    if tuple(target.shape) != tuple(x.shape):
        raise ValueError(f"{what}: the target is {tuple(target.shape)}, the map {tuple(x.shape)}")
    if target.device != x.device:
        raise ValueError(f"{what}: the target is on {target.device}, the map on {x.device}")
    L = x.shape[0]
    if L > 1 and x.stride(1) != 1:
        raise ValueError(f"{what}: the rows of the map are not contiguous (strides {tuple(x.stride())})")
    if L > 1 and target.stride(1) != 1:
        raise ValueError(f"{what}: the rows of the target are not contiguous (strides {tuple(target.stride())})")
    return L, (x.stride(0) if L > 1 else L), (target.stride(0) if L > 1 else L)


def _checked_thresholds(thresholds) -> "np.ndarray":
    th = thresholds.detach().cpu().numpy() if isinstance(thresholds, torch.Tensor) else thresholds
    th = np.ascontiguousarray(np.asarray(th, dtype=np.float64))
    if th.ndim != 1:
        raise ValueError(f"pair_sweep: expected a vector of thresholds, got shape {th.shape}")
    if not np.isfinite(th).all():
        raise ValueError(f"pair_sweep: threshold {int(np.flatnonzero(~np.isfinite(th))[0])} is not finite")
    if th.size > 1 and not (th[1:] > th[:-1]).all():
        at = int(np.flatnonzero(~(th[1:] > th[:-1]))[0]) + 1
        raise ValueError(f"pair_sweep: the thresholds are not strictly ascending at index {at} ({th[at - 1]!r}, then {th[at]!r})")
    return th


class SweepTable(NamedTuple):
    """A threshold table that has been checked (finite, strictly ascending) and lies on the device: float64 [T]."""
    values: torch.Tensor


def sweep_table(thresholds, device) -> SweepTable:
    """Checks the thresholds once, on the host, and uploads them: pair_sweep takes the result as it is, so a caller that sweeps many
    maps with one table (the CLI's 1001 values) pays the check and the copy once and its calls read nothing back."""
    return SweepTable(torch.from_numpy(_checked_thresholds(thresholds)).to(device))


@_on_operand_device
def pair_sweep(x: torch.Tensor, target: torch.Tensor, thresholds, min_sep: int = 1, skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The threshold sweep of a pair map against a target (rnamsm_pair_sweep_f64 / _f32; include/rnamsm.h states the rule): x float32
    or float64 [L, L] and target int8 [L, L] on the device, read where they lie (a last dimension that is not contiguous is refused);
    thresholds: a SweepTable (sweep_table: checked and uploaded once; the call is then asynchronous and reads nothing back), or T
    values, strictly ascending and finite, that are checked here on the host before the upload (a device tensor is copied back for
    that check: build a SweepTable instead); T in [1, 4096]; skip: uint8 or bool [L] on the device, non-zero = the position's row and
    column are left out -> int64 [4, T] on the device, the rows tp, fp, tn, fn.  Candidates are the pairs i < j with
    j - i >= min_sep; a candidate is positive iff its target is not 0."""
    L, ld, ld_t = _pair_map_and_target(x, target, "pair_sweep")
    dev = x.device
    if isinstance(thresholds, SweepTable):
        th_dev = thresholds.values
        if th_dev.device != dev:
            raise ValueError(f"pair_sweep: the threshold table is on {th_dev.device}, the map on {dev}")
    else:
        th_dev = torch.from_numpy(_checked_thresholds(thresholds)).to(dev)
    T = int(th_dev.numel())
    skip_ptr = None
    if skip is not None:
        if not isinstance(skip, torch.Tensor) or not skip.is_cuda or skip.dtype not in (torch.uint8, torch.bool):
            raise TypeError("pair_sweep: expected skip as a uint8 or bool tensor on the HIP device")
        if tuple(skip.shape) != (L,):
            raise ValueError(f"pair_sweep: skip is {tuple(skip.shape)}, expected ({L},)")
        skip = skip.contiguous()
        skip_ptr = skip.data_ptr()
    lib = _lib.load()
    ws = _aligned_workspace(lib.rnamsm_pair_sweep_workspace_bytes(T), dev)
    counts = torch.empty((4, max(min(T, _lib.PAIR_SWEEP_MAX_T), 1)), dtype=torch.int64, device=dev)
    fn = lib.rnamsm_pair_sweep_f64 if x.dtype == torch.float64 else lib.rnamsm_pair_sweep_f32
    _lib.check(fn(x.data_ptr(), L, ld, target.data_ptr(), ld_t, skip_ptr, int(min_sep), th_dev.data_ptr(), T, counts.data_ptr(),
                  ws.data_ptr(), ws.numel(), _stream()))
    return counts


class PairPrecision(NamedTuple):
    """What rnamsm_pair_precision_f64 / _f32 count, on the device."""
    hits: torch.Tensor             # int32 [ncuts]: the pairs with a target > 0 among the first min(cuts[c], count) ranked pairs
    count: torch.Tensor            # int32 scalar: min(k, the number of candidates)


@_on_operand_device
def pair_precision(x: torch.Tensor, target: torch.Tensor, k: int, cuts, min_sep: int, max_sep: int = 0,
                   want_pairs: bool = False):
    """The hits among the top-ranked pairs of a map (rnamsm_pair_precision_f64 / _f32; include/rnamsm.h states the rule): x float32
    or float64 [L, L] and target int8 [L, L] on the device, read where they lie (a last dimension that is not contiguous is refused).
    Candidates: i < j, j - i >= min_sep, j - i < max_sep when max_sep > 0, target >= 0, value not NaN; ranked as ops.top_pairs
    ranks.  cuts: ascending integers in [1, k], at most 64 (checked here; a device int32 tensor is checked too, by one copy to the
    host) -> PairPrecision(hits, count); with want_pairs=True -> (PairPrecision, TopPairs), the ranked list beside the counts."""
    L, ld, ld_t = _pair_map_and_target(x, target, "pair_precision")
    k, min_sep, max_sep = int(k), int(min_sep), int(max_sep)
    c = cuts.detach().cpu().numpy() if isinstance(cuts, torch.Tensor) else np.asarray(cuts)
    if c.ndim != 1 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"pair_precision: expected a vector of integer cuts, got shape {c.shape} of {c.dtype}")
    c = c.astype(np.int64)
    if c.size and (c.min() < 1 or c.max() > k):
        raise ValueError(f"pair_precision: cut {int(c[(c < 1) | (c > k)][0])} outside [1, k={k}]")
    if c.size > 1 and (c[1:] < c[:-1]).any():
        raise ValueError("pair_precision: the cuts are not ascending")
    dev = x.device
    cuts_dev = torch.from_numpy(c.astype(np.int32)).to(dev)
    ncuts = int(c.size)
    lib = _lib.load()
    ws = _aligned_workspace(lib.rnamsm_pair_precision_workspace_bytes(L, k, x.element_size()), dev)
    hits = torch.empty(max(min(ncuts, _lib.PAIR_PRECISION_MAX_CUTS), 1), dtype=torch.int32, device=dev)
    count = torch.empty((), dtype=torch.int32, device=dev)
    pairs = scores = None
    if want_pairs:
        n_rows = min(max(k, 1), _lib.TOP_PAIRS_MAX_K)
        pairs = torch.empty((n_rows, 2), dtype=torch.int32, device=dev)
        scores = torch.empty(n_rows, dtype=torch.float64, device=dev)
    fn = lib.rnamsm_pair_precision_f64 if x.dtype == torch.float64 else lib.rnamsm_pair_precision_f32
    _lib.check(fn(x.data_ptr(), L, ld, target.data_ptr(), ld_t, min_sep, max_sep, k, cuts_dev.data_ptr(), ncuts, hits.data_ptr(),
                  count.data_ptr(), pairs.data_ptr() if want_pairs else None, scores.data_ptr() if want_pairs else None, ws.data_ptr(),
                  ws.numel(), _stream()))
    rec = PairPrecision(hits, count)
    return (rec, TopPairs(pairs, scores, count)) if want_pairs else rec


@_on_operand_device
def msa_pdist(msa_u8: torch.Tensor, want: str = "dist"):
    """MSA.pdist (utils/align.py:121-126; rnamsm_msa_pdist): msa uint8 [N, L] on the device -> want="dist": float64 [N, N] =
    mismatches / L, scipy's pdist "hamming" in square form; "counts": int32 [N, N], the mismatches; "both": (dist, counts).  Exactly
    symmetric, the diagonal exactly 0.  N in [1, 16384], L in [1, 32768]; the library refuses anything else."""
    if want not in ("dist", "counts", "both"):
        raise ValueError(f"msa_pdist: want={want!r} is not one of 'dist', 'counts', 'both'")
    msa_u8, N, L, ld = _msa_rows(msa_u8, "msa_pdist")
    lib = _lib.load()
    dev = msa_u8.device
    ws = _aligned_workspace(lib.rnamsm_msa_pdist_workspace_bytes(N, L), dev)
    dist = torch.empty((N, N), dtype=torch.float64, device=dev) if want != "counts" else None
    counts = torch.empty((N, N), dtype=torch.int32, device=dev) if want != "dist" else None
    _lib.check(lib.rnamsm_msa_pdist(msa_u8.data_ptr(), N, L, ld, counts.data_ptr() if counts is not None else None,
                                    dist.data_ptr() if dist is not None else None, ws.data_ptr(), ws.numel(), _stream()))
    return {"dist": dist, "counts": counts, "both": (dist, counts)}[want]


class MsaNeff(NamedTuple):
    """What rnamsm_msa_neff writes, on the device."""
    n_neighbors: torch.Tensor      # int32 [N]: rows within the cutoff, the row itself included
    weights: torch.Tensor          # float64 [N]: 1 / n_neighbors
    neff: torch.Tensor             # float64 scalar: the weights' sum


@_on_operand_device
def msa_neff(msa_u8: torch.Tensor, seqid_cutoff: float = 0.2, workspace_bytes: Optional[int] = None) -> MsaNeff:
    """MSA.weights and MSA.neff("none") (utils/align.py:250-269; rnamsm_msa_neff): msa uint8 [N, L] on the device -> MsaNeff.  The
    weights are msa_weights' values bit for bit, from the tiled pair kernel, without the N x N matrix.  workspace_bytes: None = the
    library's default; any size from rnamsm_msa_neff_min_workspace_bytes(N, L) upward gives the same bits in more bands.
    N in [1, 2^20], L in [1, 32768], seqid_cutoff in [0, 1]."""
    msa_u8, N, L, ld = _msa_rows(msa_u8, "msa_neff")
    lib = _lib.load()
    dev = msa_u8.device
    ws = _aligned_workspace(lib.rnamsm_msa_neff_workspace_bytes(N, L) if workspace_bytes is None else workspace_bytes, dev)
    rec = MsaNeff(torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.float64, device=dev),
                  torch.empty((), dtype=torch.float64, device=dev))
    _lib.check(lib.rnamsm_msa_neff(msa_u8.data_ptr(), N, L, ld, float(seqid_cutoff), rec.n_neighbors.data_ptr(), rec.weights.data_ptr(),
                                   rec.neff.data_ptr(), ws.data_ptr(), ws.numel() if workspace_bytes is None else int(workspace_bytes),
                                   _stream()))
    return rec


@_on_operand_device
def msa_coverage(msa_u8: torch.Tensor, gap: int) -> torch.Tensor:
    """The coverage property (utils/align.py:242-247; rnamsm_msa_coverage): msa uint8 [N, L] on the device -> float64 [L], the share
    of rows whose byte in the column is not `gap`.  N in [1, 2^20], L in [1, 32768]."""
    msa_u8, N, L, ld = _msa_rows(msa_u8, "msa_coverage")
    out = torch.empty(L, dtype=torch.float64, device=msa_u8.device)
    _lib.check(_lib.load().rnamsm_msa_coverage(msa_u8.data_ptr(), N, L, ld, int(gap), out.data_ptr(), _stream()))
    return out


def depth_scaling(R: int) -> float:
    """1/sqrt(R) as the C++ drivers form it -- `1.0f / sqrtf((float)R)` in fp32, both steps correctly rounded -- so that the
    layer-wise mirror modules hand K5 the very same factor (forming it in double and rounding once can differ in the last bit)."""
    import numpy as np
    return float(np.float32(1.0) / np.sqrt(np.float32(R)))


def row_scaling(R: int) -> float:
    """RowSelfAttention.align_scaling (modules.py:713-715)."""
    return (HEAD_DIM ** -0.5) / math.sqrt(R)


class SeqidFilter(NamedTuple):
    """What rnamsm_seqid_filter writes, on the device."""
    indices: torch.Tensor          # int32 [n_kept]: the kept row indices, ascending
    kept_at: torch.Tensor          # int32 [N]: per row the threshold of the pass that kept it, -1 for a row never kept


def seqid_order(msa_u8: torch.Tensor, gap: int) -> torch.Tensor:
    """The order the filter walks the rows in: row 0, then the others by descending number of residues (bytes other than `gap`),
    ties by ascending index -- a stable sort, int32 [N] on the operand's device."""
    nres = (msa_u8 != int(gap)).sum(1)
    N = msa_u8.shape[0]
    if N == 1:
        return torch.zeros(1, dtype=torch.int32, device=msa_u8.device)
    rest = torch.sort(nres[1:], descending=True, stable=True).indices + 1
    return torch.cat([torch.zeros(1, dtype=rest.dtype, device=rest.device), rest]).to(torch.int32)


@_on_operand_device
def seqid_filter(msa_u8: torch.Tensor, gap: int, num_seqs: int, min_seqid: int = 20, max_seqid: int = 90, step: int = 5,
                 order: Optional[torch.Tensor] = None) -> SeqidFilter:
    """The identity redundancy filter (rnamsm_seqid_filter; include/rnamsm.h states the rule): msa uint8 [N, L] on the device (a view
    with contiguous rows is read where it lies) -> SeqidFilter.  A rule of this project's own, modelled on the reference's
    `hhfilter -id 90 -diff num_seqs` and not that binary's algorithm (no per-window count).  num_seqs > 0: passes at min_seqid,
    min_seqid + step, ..., max_seqid until num_seqs rows are kept; 0: one pass at max_seqid.  order: int32 [N] on the device, the
    rows in the order they are walked; None = seqid_order's (row 0, then by descending residues).  Cutting to num_seqs rows is the
    caller's.  N in [1, 2^20], L in [1, 32768]; the call waits for the device (the kept count is read back once per pass)."""
    msa_u8, N, L, ld = _msa_rows(msa_u8, "seqid_filter")
    dev = msa_u8.device
    if order is None:
        order = seqid_order(msa_u8[:, :L], gap)
    _dev(order, "order", torch.int32)
    if order.dim() != 1 or order.shape[0] != N:
        raise ValueError(f"seqid_filter: expected an order of {N} entries, got {tuple(order.shape)}")
    order = order.contiguous()
    lib = _lib.load()
    ws = _aligned_workspace(lib.rnamsm_seqid_filter_workspace_bytes(N, L), dev)
    indices = torch.empty(N, dtype=torch.int32, device=dev)
    kept_at = torch.empty(N, dtype=torch.int32, device=dev)
    n_kept = ctypes.c_int(0)
    _lib.check(lib.rnamsm_seqid_filter(msa_u8.data_ptr(), N, L, ld, int(gap), order.data_ptr(), int(num_seqs), int(min_seqid),
                                       int(max_seqid), int(step), indices.data_ptr(), kept_at.data_ptr(),
                                       ctypes.addressof(n_kept), ws.data_ptr(), ws.numel(), _stream()))
    return SeqidFilter(indices[:n_kept.value], kept_at)
