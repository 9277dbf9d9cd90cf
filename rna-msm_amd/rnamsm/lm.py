"""The LM head as a HIP head of its own (§8 f4: RobertaLMHead of the reference's modules.py plus the log-softmax and wild-type
subtraction of utils/likelihood.py): rnamsm_lm_head on chosen rows of a feature buffer, where they lie.

`LMHeadKernel` pins the weights of `model.lm_head` for the kernels and runs them (`rows`, `packed`).  `LMHead` is the head as the CLI
runs it (data.lm_scores): one `LMResult` per alignment -- "wt": the unmasked marginals from the alignment's own emb, no further
forward; "masked": likelihood.scan, one forward per query position -- and the job that writes `<id>_lm_scores.npy` / `<id>_lm_nll.npy`.
"""
from __future__ import annotations

import os
from typing import List, NamedTuple, Sequence

import numpy as np
import torch

from . import _lib, ops
from .config import LM_SCORES_MODES, check_lm_scores        # noqa: F401  (data.lm_scores)
from .ss import plan_chunks

# rows (sum of L) of one packed call: the head's workspace is D floats per row (96 MB at D = 768), its outputs V + 1 floats per row.
# A bound on one allocation, not a measurement.
LM_CHUNK_ROWS = 32768


def plan_lm_chunks(Ls: Sequence[int], max_rows: int = LM_CHUNK_ROWS, max_batch: int = _lib.LM_MAX_BATCH) -> List[List[int]]:
    """Indices of `Ls` split into consecutive calls of rnamsm_lm_head_packed, in list order: a chunk takes the next alignment as
    long as its sum of L stays within max_rows and its length within max_batch (greedy); an alignment longer than the budget by
    itself is a chunk of its own."""
    return plan_chunks([int(L) for L in Ls], max_rows, max_batch)


class LMHeadKernel:
    """The weights of `model.lm_head` (dense, layer_norm, the tied projection and its bias) as the kernels read them: detached,
    contiguous, re-read whenever a parameter's (data_ptr, _version) changes."""

    def __init__(self, lm_head: torch.nn.Module):
        self.lm_head = lm_head
        self._key = None
        self._weights = None

    def _params(self):
        lm = self.lm_head
        return (lm.dense.weight, lm.dense.bias, lm.layer_norm.weight, lm.layer_norm.bias, lm.weight, lm.bias)

    def weights(self) -> ops.LMWeights:
        params = self._params()
        key = tuple((p.data_ptr(), p._version) for p in params)
        if key != self._key:
            self._weights = ops.lm_weights(*params, eps=self.lm_head.layer_norm.eps)
            self._key = key
        return self._weights

    def rows(self, x: torch.Tensor, rows=None, wt=None, want=None) -> dict:
        return ops.lm_head_rows(x, rows, wt, self.weights(), want)

    def packed(self, xs, rows, wts, want=None) -> List[dict]:
        return ops.lm_head_packed(xs, rows, wts, self.weights(), want)


def kernel_of(model) -> LMHeadKernel:
    """The model's LMHeadKernel, made on first use and kept on the model."""
    k = model.__dict__.get("_lm_head_kernel")
    if k is None or k.lm_head is not model.lm_head:
        k = model.__dict__["_lm_head_kernel"] = LMHeadKernel(model.lm_head)
    return k


class LMResult(NamedTuple):
    """One alignment's result of the LM head, on the device (or, on the writer's side, its host copy)."""
    scores: torch.Tensor                          # [L, V]  log p(token) - log p(wild type) per query position
    nll: torch.Tensor                             # [L]     -log p(wild type)


class LMHead:
    """data.lm_scores in the CLI.  Unlike the other heads this one is handed the alignment's WHOLE token matrix [R, C] (the masked
    scan runs further forwards on it); the wild type is its row 0 behind <cls>."""

    n_tensors = 2
    whole_tokens = True
    skip_suffix = "(masked)"            # behind the class name in the line the CLI prints where stitched_route skips this head

    def __init__(self, model, mode: str):
        if check_lm_scores(mode) == "":
            raise ValueError("LMHead: data.lm_scores is off")
        self.model, self.mode, self.kernel = model, mode, kernel_of(model)

    def _masked(self, tokens: torch.Tensor) -> LMResult:
        from .likelihood import scan
        print(f"data.lm_scores=masked: {tokens.shape[1] - 1} further forwards for this alignment (one per query position)")
        s = scan(self.model, tokens)
        return LMResult(s.scores, s.nll)

    def one(self, emb: torch.Tensor, atp: torch.Tensor, tokens: torch.Tensor) -> LMResult:
        """A lone alignment: "wt" through the lone call on emb where it lies (atp is not read: the heads share one signature)."""
        if self.mode == "masked":
            return self._masked(tokens)
        out = self.kernel.rows(emb, None, tokens[0, 1:], want=("scores", "nll"))
        return LMResult(out["scores"], out["nll"])

    def stitched_route(self, L: int, long_on: bool):
        """On a stitched alignment of L body columns: "wt" keeps one() -- its kernel has no length limit that matters, and no long
        route; "masked" is skipped (the reason named with data.long_heads=stitched on only, as for the other heads)."""
        if self.mode == "wt":
            return self.one
        return "the masked scan would run L forwards per window" if long_on else ""

    def many(self, embs: Sequence[torch.Tensor], atps: Sequence[torch.Tensor], tokens: Sequence[torch.Tensor]) -> List[LMResult]:
        """A group: "wt" in one launch set per chunk of plan_lm_chunks, every member's record the bits of one()."""
        if self.mode == "masked":
            return [self._masked(t) for t in tokens]
        embs, tokens = list(embs), list(tokens)
        out: List[LMResult] = []
        for chunk in plan_lm_chunks([e.shape[0] for e in embs]):
            res = self.kernel.packed([embs[i] for i in chunk], None, [tokens[i][0, 1:] for i in chunk], want=("scores", "nll"))
            out += [LMResult(r["scores"], r["nll"]) for r in res]
        return out

    def flatten(self, rec: LMResult) -> list:
        return [rec.scores, rec.nll]

    def unflatten(self, tensors: Sequence) -> LMResult:
        if len(tensors) != self.n_tensors:
            raise ValueError(f"LMHead: {len(tensors)} tensors for a record of {self.n_tensors}")
        return LMResult(tensors[0], tensors[1])

    def writer_job(self, rec: LMResult, name: str, output_dir):
        """-> (write, tensors): write(host copies) saves <output_dir>/<name>_lm_scores.npy (L, V) and <name>_lm_nll.npy (L,)."""
        p_scores = os.path.join(output_dir, f"{name}_lm_scores.npy")
        p_nll = os.path.join(output_dir, f"{name}_lm_nll.npy")

        def write(scores, nll) -> None:
            np.save(p_scores, scores)
            np.save(p_nll, nll)

        return write, (rec.scores, rec.nll)
