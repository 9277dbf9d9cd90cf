"""Masked pseudo-likelihood scoring on top of the HIP forward (§8 f4: the reference's utils/likelihood.py).

`sequence_logits` mirrors utils/likelihood.py:39-82 for alignment input: position i of the query (row 0) is replaced by
<mask> in copy i of the MSA, every copy runs the 10-layer forward and the LM head, and the logits at the masked position
are collected.  The copies go through `MSATransformer.forward` in batches of max(1, max_tokens // (R*C)) MSAs, as the
reference does; every FLOP is in librnamsm_hip.so.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib

IntSeq = Union[Sequence[int], np.ndarray, torch.Tensor]


def mask_and_repeat(tokens: torch.Tensor, indices: IntSeq, mask_idx: int) -> torch.Tensor:
    """tokens [R, C] -> [len(indices), R, C] with copy i masked at (row 0, indices[i])  (utils/likelihood.py:18-27)."""
    idx = torch.as_tensor(indices, dtype=torch.long, device=tokens.device)
    out = tokens.unsqueeze(0).repeat(len(idx), 1, 1)
    out[torch.arange(len(idx), device=tokens.device), 0, idx] = mask_idx
    return out


@torch.no_grad()
def sequence_logits(model, tokens: torch.Tensor, mask_positions: bool = True, max_tokens: int = 2 ** 14,
                    indices: Optional[IntSeq] = None) -> torch.Tensor:
    """tokens int64 [R, C] (or [C]: a one-row alignment) on the HIP device, column 0 = <cls>.
    Returns logits [len(indices), vocab] at the query positions `indices` (default: every column after <cls>)."""
    if tokens.dim() == 1:
        tokens = tokens[None]
    assert tokens.dim() == 2
    vocab = model.vocab
    R, C = tokens.shape
    if indices is None:
        indices = torch.arange(int(vocab.prepend_bos), C - int(vocab.append_eos))
    idx = torch.as_tensor(indices, dtype=torch.long, device=tokens.device)
    n = len(idx)
    if not mask_positions:                                                   # utils/likelihood.py:80-81
        out = model(tokens[None], need_logits=True)["logits"]                # [1, R, C, V]
        return out[0, 0, idx]
    masked = mask_and_repeat(tokens, idx, vocab.mask_idx)
    logits = torch.zeros(n, len(vocab), device=tokens.device)
    batch = max(1, max_tokens // (R * C))
    for s in range(0, n, batch):
        out = model(masked[s:s + batch], need_logits=True)["logits"]         # [b, R, C, V]
        b = out.shape[0]
        logits[s:s + b] = out[torch.arange(b, device=out.device), 0, idx[s:s + b]]
    return logits


@torch.no_grad()
def masked_marginal_scores(model, tokens: torch.Tensor, mask_positions: bool = True, max_tokens: int = 2 ** 14,
                           indices: Optional[IntSeq] = None) -> torch.Tensor:
    """log p(token | masked context) - log p(wild type | masked context) per query position and vocabulary entry
    (utils/likelihood.py:86-120 up to its final re-mapping onto the 20 protein letters, which has no RNA counterpart):
    [len(indices), vocab]; the wild-type column is 0."""
    if tokens.dim() == 1:
        tokens = tokens[None]
    vocab = model.vocab
    C = tokens.shape[1]
    if indices is None:
        indices = torch.arange(int(vocab.prepend_bos), C - int(vocab.append_eos))
    idx = torch.as_tensor(indices, dtype=torch.long, device=tokens.device)
    lp = sequence_logits(model, tokens, mask_positions, max_tokens, idx).log_softmax(-1)
    wt = tokens[0, idx]
    return lp - lp[torch.arange(len(idx), device=lp.device), wt].unsqueeze(1)


# ---------------------------------------------------------------------------------------------------------------------------------
# The same scan on the LM head's own kernels (rnamsm.lm / rnamsm_lm_head): the masked copies are built per forward call, the forward
# runs without the full representation, and the head runs on the one row per copy that is asked for, where it lies in `emb`.
class LMScan(NamedTuple):
    """The LM head at n query positions, on the device."""
    logits: torch.Tensor                          # [n, V]
    logp: torch.Tensor                            # [n, V]  log-softmax of the logits
    scores: torch.Tensor                          # [n, V]  logp - logp[wild type]; the wild-type column is exactly 0
    nll: torch.Tensor                             # [n]     -logp[wild type]


def plan_scan_calls(n: int, R: int, C: int, budget: int) -> List[Tuple[int, int]]:
    """The forward calls of a scan over n masked copies of an R x C alignment: [(start, stop)] over the positions, in order, each
    call max(1, budget // (R * C)) copies (forward()'s rule for a batch) but for the last, which takes what is left."""
    if n < 0 or R < 1 or C < 1:
        raise ValueError(f"plan_scan_calls: n = {n}, R = {R}, C = {C}")
    per = max(1, int(budget) // (R * C))
    return [(s, min(s + per, n)) for s in range(0, n, per)]


def _scan_indices(model, tokens: torch.Tensor, indices: Optional[IntSeq]) -> List[int]:
    C = tokens.shape[1]
    if indices is None:
        return list(range(int(model.vocab.prepend_bos), C - int(model.vocab.append_eos)))
    idx = [int(i) for i in (indices.tolist() if isinstance(indices, (torch.Tensor, np.ndarray)) else indices)]
    bad = [i for i in idx if not 1 <= i < C]
    if bad:
        raise ValueError(f"scan: indices {bad} outside [1, {C}): the scan reads a copy's feature from emb, which holds the columns "
                         "behind <cls> only -- likelihood.sequence_logits is the route for column 0")
    return idx


@torch.no_grad()
def scan(model, tokens: torch.Tensor, indices: Optional[IntSeq] = None, mask_positions: bool = True,
         copies_per_call: Optional[int] = None) -> LMScan:
    """Masked pseudo-likelihood scan (utils/likelihood.py:39-120) of the alignment tokens int64 [R, C] (or [C]) on the HIP device:
    for every query column in `indices` (default: every column behind <cls>; each in [1, C)) the LM head's logits, log-probabilities,
    scores against the wild type (row 0's token there) and negative log-likelihood, with that column of row 0 replaced by <mask>.
    At most copies_per_call masked copies exist at a time (default max(1, model.batch_token_budget // (R * C))): a call of more
    than one copy runs through checked_forward_batch, a single copy through checked_forward_one(need_repr=False), and the head then
    runs on exactly the rows emb[b, idx_b - 1] of that call, selected by a row table, not copied.  mask_positions=False: one
    forward of the alignment as it is, the head on row 0's emb.  The forwards run in model.gemm_dtype, the head always in fp32."""
    from . import ops
    from .lm import kernel_of
    if tokens.dim() == 1:
        tokens = tokens[None]
    assert tokens.dim() == 2
    if not tokens.is_cuda:
        raise _lib.RnamsmError("tokens must be on the HIP device (no CPU path exists)")
    R, C = tokens.shape
    idx = _scan_indices(model, tokens, indices)
    head = kernel_of(model)
    V = head.weights().V
    dev = tokens.device
    if not idx:
        e = torch.empty(0, V, device=dev)
        return LMScan(e, e.clone(), e.clone(), torch.empty(0, device=dev))
    tokens = tokens.to(torch.int64)
    idx_dev = torch.tensor(idx, dtype=torch.int64, device=dev)
    wt = tokens[0, idx_dev]
    has_padding = bool((tokens == model.vocab.pad_idx).any())
    if not mask_positions:
        out = model.checked_forward_one(tokens, has_padding, need_repr=False)
        res = head.rows(out["emb"], [i - 1 for i in idx], wt)
        return LMScan(*(res[k] for k in _lib.LM_OUTPUTS))
    per = max(1, model.batch_token_budget // (R * C)) if copies_per_call is None else int(copies_per_call)
    if per < 1:
        raise ValueError(f"scan: copies_per_call = {copies_per_call}")
    chunked = has_padding and _lib.load().rnamsm_row_chunks(R, C, min(int(model.max_tokens_per_msa), 2 ** 31 - 1)) > 0
    batched = per > 1 and not chunked and model.batch_small_msas and (model.gemm_dtype == "f32" or ops.get_param("attn16") != 0)
    if not batched:                                   # forward()'s conditions for a batch: else one copy per call
        per = 1
    parts = []
    mask_idx = model.vocab.mask_idx
    for s, e in plan_scan_calls(len(idx), R, C, per * R * C):
        b = e - s
        if b > 1:
            copies = tokens.unsqueeze(0).repeat(b, 1, 1)
            copies[torch.arange(b, device=dev), 0, idx_dev[s:e]] = mask_idx
            out = model.checked_forward_batch(copies, has_padding)
            feats = out["emb"].view(b * (C - 1), -1)
            rows = [k * (C - 1) + idx[s + k] - 1 for k in range(b)]
        else:
            copies = tokens.clone()
            copies[0, idx[s]] = mask_idx
            out = model.checked_forward_one(copies, has_padding, need_repr=False)
            feats, rows = out["emb"], [idx[s] - 1]
        parts.append(head.rows(feats, rows, wt[s:e]))
        del out, feats, copies                         # at most one call's copies and outputs are resident
    return LMScan(*(torch.cat([p[k] for p in parts], 0) for k in _lib.LM_OUTPUTS))


@torch.no_grad()
def pseudo_perplexity(model, tokens: torch.Tensor, indices: Optional[IntSeq] = None, mask_positions: bool = True,
                      copies_per_call: Optional[int] = None, reduction: str = "mean", log: bool = False) -> float:
    """utils/likelihood.py:139-170 (sequence_pseudo_ppl) for alignment input: the cross entropy of the masked logits against row 0's
    tokens -- the mean (or, reduction="sum", the sum) of scan(...).nll, reduced on the device -- and its exponential unless `log`.
    One scalar is read back."""
    if reduction not in ("mean", "sum"):
        raise ValueError(f"pseudo_perplexity: reduction must be 'mean' or 'sum', got {reduction!r}")
    nll = scan(model, tokens, indices, mask_positions, copies_per_call).nll
    ce = nll.mean() if reduction == "mean" else nll.sum()
    return float((ce if log else ce.exp()).item())
