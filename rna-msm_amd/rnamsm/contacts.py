"""The contact head of the language model itself: base-pair probabilities from the row attentions by the reference's symmetrize +
APC + logistic regression (ContactPredictionHead, `contact_head.regression.*` of the trunk's checkpoint).

`predict_many` runs a list of stripped maps (atp [120, L, L], as forward_one and the packed drivers leave them) through as few
launch sets as `plan_contact_chunks` allows (rnamsm_contact_head_packed), every result the bits of the lone call on the un-stripped
maps.  `ContactHead` is the head as the CLI runs it (data.contacts): it makes one `ContactResult` per alignment from the atp where it
lies on the device and turns it into the job that writes `<id>_contacts.npy`.
"""
from __future__ import annotations

import math
import os
from typing import List, NamedTuple, Sequence

import numpy as np
import torch

from . import _lib, ops
from .config import parse_top_pairs_spec
from .ss import long_refusal, plan_chunks

# pixels (sum of L^2) of one packed call: the SS head's budget.  The head's own workspace is 121 floats per position and its
# outputs 4 MB at the budget, so the budget bounds nothing but the size of one output allocation (a condition, not a measurement).
CONTACT_CHUNK_PIXELS = 1024 * 1024


def plan_contact_chunks(Ls: Sequence[int], max_pixels: int = CONTACT_CHUNK_PIXELS,
                        max_batch: int = _lib.CONTACT_MAX_BATCH) -> List[List[int]]:
    """Indices of `Ls` split into consecutive calls of rnamsm_contact_head_packed, in list order: a chunk takes the next alignment
    as long as its sum of L^2 stays within max_pixels and its length within max_batch (greedy); an alignment larger than the budget
    by itself is a chunk of its own."""
    return plan_chunks([int(L) * int(L) for L in Ls], max_pixels, max_batch)


def predict_many(atps: Sequence[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor) -> List[torch.Tensor]:
    """contacts [L_b, L_b] of every atps[b] ([nch, L_b, L_b]), one packed call per chunk of plan_contact_chunks: each the bits of
    ops.contact_head_atp on that member alone."""
    atps = list(atps)
    out: List[torch.Tensor] = []
    for chunk in plan_contact_chunks([a.shape[-1] for a in atps]):
        out += ops.contact_head_packed([atps[i] for i in chunk], weight, bias)
    return out


def top_pairs(x, k: int, min_sep: int = 1, device=None):
    """The top-k ranked pairs of a square pair map (ops.top_pairs; include/rnamsm.h states the rule): x a float32 or float64 [L, L]
    numpy array (moved to `device`) or a tensor on the HIP device -> (pairs int64 [n, 2], scores float64 [n]) as numpy arrays,
    trimmed to n = min(k, the number of candidates).  Candidates: i < j, j - i >= min_sep, not NaN; larger score first, then smaller i,
    then smaller j.  There is no CPU path."""
    if not isinstance(x, torch.Tensor):
        if device is None or torch.device(device).type != "cuda":
            raise _lib.RnamsmError("top_pairs: expected a HIP device for the map (no CPU path exists)")
        x = torch.from_numpy(np.ascontiguousarray(x)).to(device)
    rec = ops.top_pairs(x, k, min_sep)
    n = int(rec.count.item())
    return rec.pairs[:n].cpu().numpy().astype(np.int64), rec.scores[:n].cpu().numpy()


def top_pairs_k(spec, L: int) -> int:
    """data.top_pairs' spec -> k for a map of L positions: "N" = the integer N >= 1; "<x>L" = max(1, ceil(x * L)) with x > 0 read as an
    exact decimal fraction (fractions.Fraction of the string, no float arithmetic: 0.1L at L = 30 is 3)."""
    count, multiple = parse_top_pairs_spec(spec)
    return count if multiple is None else max(1, math.ceil(multiple * int(L)))


def format_top_pairs(pairs, scores, min_sep: int) -> str:
    """The text of a `<id>_<map>_top.txt`: a header, then `i+1 j+1 repr(float(score))` per ranked pair (at most 65536 short lines,
    formatted on the host).  A zero of either sign is printed as 0.0, as the device writes it."""
    lines = [f"# i j score (1-based, j - i >= {int(min_sep)})"]
    lines += [f"{int(i) + 1} {int(j) + 1} {float(s) + 0.0!r}" for (i, j), s in zip(pairs, scores)]
    return "\n".join(lines) + "\n"


class ContactResult(NamedTuple):
    """One alignment's result of the contact head, on the device (or, on the writer's side, its host copy)."""
    contacts: torch.Tensor                        # [L, L]


class ContactHead:
    """data.contacts in the CLI: the regression's weight [nch] and bias [1] on the device (the trunk's own parameters)."""

    n_tensors = 1

    def __init__(self, weight: torch.Tensor, bias: torch.Tensor):
        self.weight, self.bias = weight.detach().contiguous().view(-1), bias.detach().contiguous().view(-1)

    def _one(self, emb: torch.Tensor, atp: torch.Tensor, tokens: torch.Tensor, long: bool) -> ContactResult:
        return ContactResult((ops.contact_head_long if long else ops.contact_head_atp)(atp, self.weight, self.bias))

    def one(self, emb: torch.Tensor, atp: torch.Tensor, tokens: torch.Tensor) -> ContactResult:
        """A lone alignment through the lone call; atp is read where it lies (emb and tokens are not read: the heads share one
        signature)."""
        return self._one(emb, atp, tokens, False)

    def one_long(self, emb: torch.Tensor, atp: torch.Tensor, tokens: torch.Tensor) -> ContactResult:
        """one() on the stitched atp of a long alignment (data.long_heads=stitched), L up to LONG_MAX_L = 4096: the same record
        through rnamsm_contact_head_long.  Symmetrise and APC run over the whole map; a pair no window holds takes part as 0."""
        return self._one(emb, atp, tokens, True)

    def stitched_route(self, L: int, long_on: bool):
        """On a stitched alignment of L body columns: the method that runs this head, or the reason (a str) it is skipped."""
        why = long_refusal(L, long_on)
        return self.one_long if why is None else why

    def many(self, embs: Sequence[torch.Tensor], atps: Sequence[torch.Tensor], tokens: Sequence[torch.Tensor]) -> List[ContactResult]:
        """A group in one launch set per chunk (predict_many): every member's record holds the bits of one()."""
        return [ContactResult(c) for c in predict_many(atps, self.weight, self.bias)]

    def flatten(self, rec: ContactResult) -> list:
        return [rec.contacts]

    def unflatten(self, tensors: Sequence) -> ContactResult:
        if len(tensors) != self.n_tensors:
            raise ValueError(f"ContactHead: {len(tensors)} tensors for a record of {self.n_tensors}")
        return ContactResult(tensors[0])

    def writer_job(self, rec: ContactResult, name: str, output_dir):
        """-> (write, tensors): write(host copy of the contacts) is one np.save of <output_dir>/<name>_contacts.npy."""
        path = os.path.join(output_dir, f"{name}_contacts.npy")

        def write(contacts) -> None:
            np.save(path, contacts)

        return write, (rec.contacts,)
