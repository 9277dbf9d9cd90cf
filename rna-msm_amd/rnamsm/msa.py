"""a2m / FASTA alignment reader and row sub-sampling for the CLI path.

Replaces MSA.from_fasta (utils/align.py:291-317) + A2MDataset.__getitem__ (dataset.py:80-92) for this
path.  Row sub-sampling: the reference defaults to the external `hhfilter` binary (utils/align.py:68-102),
which is not available offline; supported here are `first` (keep the first N rows), the reference's weighted random
`sample-pretrained` (utils/align.py:150-163; weights on the device, the draw by numpy's generator) and its
greedy `diversity-max` / `diversity-min` (utils/align.py:128-148), on the HIP device when one is given
(rnamsm_greedy_select) or on the host -- index-identical to the reference either way.  `seqid-filter` is this project's own
identity redundancy filter (seqid_filter below; rnamsm_seqid_filter on the device, numpy on the host, index-identical): modelled on
what the reference asks of hhfilter (-id 90 -diff num_seqs), not a reproduction of that binary.
"""
from __future__ import annotations

from pathlib import Path
from typing import List, Tuple, Union

import numpy as np

from .alphabet import RNAAlphabet

SAMPLE_METHODS = ("hhfilter", "sample-pretrained", "diversity-max", "diversity-min", "first", "seqid-filter")


def read_fasta_records(path_or_text: Union[str, Path], is_text: bool = False) -> List[Tuple[str, str]]:
    """(description, sequence) records the way the reference's parser (Bio.SeqIO "fasta" = SimpleFastaParser) yields them:
    lines split at newlines only, a record's lines right-stripped and joined, then blanks and carriage returns removed
    (interior tabs stay and are invalid tokens, as there); text before the first '>' is skipped."""
    text = path_or_text if is_text else Path(path_or_text).read_text()
    records: List[Tuple[str, str]] = []
    header, parts = None, []

    def close():
        records.append((header, "".join(parts).replace(" ", "").replace("\r", "")))

    for raw in text.split("\n"):
        if raw[:1] == ">":
            if header is not None:
                close()
            header, parts = raw[1:].rstrip(), []
        elif header is not None:
            parts.append(raw.rstrip())
    if header is not None:
        close()
    return records


def greedy_select(tokens: np.ndarray, num_seqs: int, mode: str = "max") -> np.ndarray:
    """Row indices (sorted) chosen by the reference's greedy max/min mean-Hamming rule
    (utils/align.py:128-148): start from row 0, repeatedly add the row whose mean normalised Hamming
    distance to the rows chosen so far is largest (smallest), first index on ties.

    Candidates with equal mismatch totals are everywhere in real alignments (at step n the totals are integers below
    n*L), and since m/L is inexact in float64 the winner among them is decided by the ORDER of the n additions.  The
    reference takes `.mean(0)` of a [n, candidates] matrix whose reduction axis is the contiguous one (np.delete along
    axis 1 hands back such a layout), i.e. numpy's pairwise summation: 8 interleaved accumulators up to 128 terms, halves
    rounded to multiples of 8 above.  Keeping one float64 per (candidate, step) and reducing along the contiguous step
    axis reproduces exactly that order, so the indices are the reference's (pinned on the shipped 1176-row 2DRB_1
    alignment, where a running sum goes a different way at step 46)."""
    depth = tokens.shape[0]
    if depth <= num_seqs:
        return np.arange(depth)
    body = tokens[:, 1:] if tokens.shape[1] > 1 else tokens
    pick = np.argmax if mode == "max" else np.argmin
    chosen = [0]
    taken = np.zeros(depth, dtype=bool)
    taken[0] = True
    hist = np.empty((depth, num_seqs - 1), dtype=np.float64)        # [candidate, step]: step axis contiguous
    for step in range(1, num_seqs):
        last = body[chosen[-1]]
        hist[:, step - 1] = (body != last[None, :]).mean(1)         # cdist(..., "hamming") = mismatches / L
        cand = np.flatnonzero(~taken)
        best = cand[pick(hist[cand, :step].sum(1) / step)]
        chosen.append(int(best))
        taken[best] = True
    return np.array(sorted(chosen))


def greedy_select_device(tokens: np.ndarray, num_seqs: int, mode: str, device) -> np.ndarray:
    """greedy_select on the HIP device (rnamsm_greedy_select): same indices as the host version, O(N*L) bytes per
    step at HBM/L2 speed instead of numpy speed -- for alignments with 1e4..1e5 rows."""
    import torch
    from . import ops
    if tokens.shape[0] <= num_seqs:
        return np.arange(tokens.shape[0])
    body = tokens[:, 1:] if tokens.shape[1] > 1 else tokens
    u8 = torch.from_numpy(np.ascontiguousarray(body.astype(np.uint8))).to(device)
    return ops.greedy_select(u8, num_seqs, mode).cpu().numpy().astype(np.int64)


def msa_weights(tokens: np.ndarray, seqid_cutoff: float = 0.2, device=None) -> np.ndarray:
    """MSA.weights (utils/align.py:250-253): 1 / number of rows within `seqid_cutoff` normalised Hamming distance (the
    row itself included), float64 [N].  The distances are over the alignment columns (no <cls>); with `device` the O(N^2 L)
    comparison runs on the GPU (rnamsm_msa_weights) -- same integers, same float64 comparison, identical weights."""
    body = np.ascontiguousarray((tokens[:, 1:] if tokens.shape[1] > 1 else tokens).astype(np.uint8))
    if device is not None:
        import torch
        from . import ops
        return ops.msa_weights(torch.from_numpy(body).to(device), seqid_cutoff).cpu().numpy()
    n = body.shape[0]
    counts = np.zeros(n, dtype=np.int64)
    step = max(1, (1 << 24) // max(1, n * body.shape[1]))
    for i0 in range(0, n, step):
        dist = (body[i0:i0 + step, None, :] != body[None, :, :]).mean(-1)       # pdist(.., "hamming") = mismatches / L
        counts[i0:i0 + step] = (dist < seqid_cutoff).sum(1)
    return 1 / counts


def msa_invcov_device(tokens: np.ndarray, gap_idx: int, device):
    """msa_invcov with the map left on the device (a float64 [L, L] tensor): what the CLI's writer copies from."""
    import torch
    from . import _lib, ops
    dev = torch.device(device) if device is not None else None
    if dev is None or dev.type != "cuda":
        raise _lib.RnamsmError(f"msa_invcov: device={device!r} is not a HIP device (no CPU path exists)")
    body = tokens[:, 1:] if tokens.shape[1] > 1 else tokens
    if body.size and (int(body.min()) < 0 or int(body.max()) > 255):
        raise ValueError("msa_invcov: token ids outside [0, 255]")
    return ops.msa_invcov(torch.from_numpy(np.ascontiguousarray(body.astype(np.uint8))).to(dev), int(gap_idx))


def msa_invcov(tokens: np.ndarray, gap_idx: int, device) -> np.ndarray:
    """MSA.invcov (utils/align.py:183-193), the covariance contact map of an alignment: float64 [L, L], the spectral norm of every
    K x K block of the covariance of its one-hot columns (K = the distinct non-gap tokens that occur; a gap is all zeros).  The
    columns are the alignment's (no <cls>, as in msa_weights); token ids stand for the reference's character bytes -- a one-to-one
    recoding permutes every block's rows and columns and leaves its norm unchanged.  On the HIP device only (rnamsm_msa_invcov):
    there is no CPU path, a device that is not one is refused.  N in [2, 2^20], L <= 4096, K in [1, 16]."""
    return msa_invcov_device(tokens, gap_idx, device).cpu().numpy()


def _stats_body_device(tokens: np.ndarray, device, name: str):
    """The alignment's columns (no <cls>, as msa_weights slices them) as uint8 on the HIP device; any other device is refused."""
    import torch
    from . import _lib
    dev = torch.device(device) if device is not None else None
    if dev is None or dev.type != "cuda":
        raise _lib.RnamsmError(f"{name}: device={device!r} is not a HIP device (no CPU path exists)")
    body = tokens[:, 1:] if tokens.shape[1] > 1 else tokens
    if body.size and (int(body.min()) < 0 or int(body.max()) > 255):
        raise ValueError(f"{name}: token ids outside [0, 255]")
    return torch.from_numpy(np.ascontiguousarray(body.astype(np.uint8))).to(dev)


def msa_mi_device(tokens: np.ndarray, gap_idx: int, device, gaps: str = "pairwise"):
    """msa_mi with the two maps left on the device (an ops.MsaMi of float64 [L, L] tensors): what the CLI's writer copies from."""
    from . import ops
    return ops.msa_mi(_stats_body_device(tokens, device, "msa_mi"), int(gap_idx), gaps)


def msa_mi(tokens: np.ndarray, gap_idx: int, device, gaps: str = "pairwise"):
    """Mutual-information contacts of an alignment: (mi, mip), float64 [L, L] each.  mi[i, j] is the mutual information (natural log) of
    columns i and j over the K distinct non-gap tokens that occur, its diagonal the columns' entropies; mip is its average-product
    correction, apc(mi with a zero diagonal) (utils/tensor.py:103-113).  gaps="pairwise": rows with a gap in either column are left
    out of that pair; "state": the gap is a (K+1)-th state.  The columns are the alignment's (no <cls>, as in msa_invcov); a
    one-to-one recoding of the tokens permutes every pair's table and changes the sum's order only.  On the HIP device only
    (rnamsm_msa_mi): there is no CPU path.  N in [2, 2^20], L <= 4096, K in [1, 16]."""
    rec = msa_mi_device(tokens, gap_idx, device, gaps)
    return rec.mi.cpu().numpy(), rec.mip.cpu().numpy()


def msa_mi_weighted_device(tokens: np.ndarray, gap_idx: int, device, gaps: str = "pairwise", weights=None, seqid_cutoff: float = 0.2):
    """msa_mi_weighted with everything left on the device (an ops.MsaWmi): what the CLI's writer copies from.  weights: float64 [N],
    a numpy array or a tensor on the device; None: ops.msa_neff's at seqid_cutoff."""
    import torch
    from . import ops
    u8 = _stats_body_device(tokens, device, "msa_mi_weighted")
    if weights is None:
        weights = ops.msa_neff(u8, seqid_cutoff).weights
    elif not isinstance(weights, torch.Tensor):
        weights = torch.from_numpy(np.array(weights, dtype=np.float64))
    return ops.msa_wmi(u8, int(gap_idx), gaps, weights.to(u8.device))


def msa_mi_weighted(tokens: np.ndarray, gap_idx: int, device, gaps: str = "pairwise", weights=None, seqid_cutoff: float = 0.2):
    """Sequence-weighted mutual-information contacts of an alignment: (mi, mip), float64 [L, L] each -- msa_mi with row n counted
    weights[n] times in every pair's table, so a thousand near-identical copies of one sequence count about once.  weights: float64
    [N], every one finite and > 0; None: MSA.weights (utils/align.py:250-253), 1 / the rows within a normalised Hamming distance of
    seqid_cutoff, from the device (ops.msa_neff, with that call's limits; a cutoff of 0 gives infinite weights, which are refused).
    With every weight 1.0 the maps are msa_mi's bit for bit.  gaps and the columns (no <cls>) are msa_mi's.  On the HIP device only
    (rnamsm_msa_wmi): there is no CPU path.  N in [2, 2^20], L <= 4096, K in [1, 16]."""
    rec = msa_mi_weighted_device(tokens, gap_idx, device, gaps, weights, seqid_cutoff)
    return rec.mi.cpu().numpy(), rec.mip.cpu().numpy()


def msa_pdist(tokens: np.ndarray, device) -> np.ndarray:
    """MSA.pdist (utils/align.py:121-126): the normalised Hamming distance of every pair of rows, float64 [N, N] (scipy's
    squareform(pdist(.., "hamming")): mismatches / L), over the alignment's columns (no <cls>).  Token ids stand for the reference's
    character bytes: a one-to-one recoding changes no distance.  On the HIP device only (rnamsm_msa_pdist); N <= 16384, L <= 32768."""
    from . import ops
    return ops.msa_pdist(_stats_body_device(tokens, device, "msa_pdist"), "dist").cpu().numpy()


def msa_stats_device(tokens: np.ndarray, gap_idx: int, seqid_cutoff: float, device):
    """(ops.MsaNeff, coverage float64 [L]) of an alignment, left on the device: what the CLI's data.msa_stats writes and prints."""
    from . import ops
    u8 = _stats_body_device(tokens, device, "msa_stats")
    return ops.msa_neff(u8, seqid_cutoff), ops.msa_coverage(u8, int(gap_idx))


def msa_neff(tokens: np.ndarray, seqid_cutoff: float = 0.2, normalization="none", device=None) -> float:
    """MSA.neff (utils/align.py:259-269): the sum of the sequence weights at `seqid_cutoff`, divided by 1 ("none"), sqrt(L) ("sqrt"),
    L ("seqlen") or the number given; L = the alignment's columns (no <cls>).  The sum is rnamsm_msa_neff's (one fixed order on the
    device), the division is done here.  On the HIP device only."""
    import math
    from . import ops
    u8 = _stats_body_device(tokens, device, "msa_neff")
    if isinstance(normalization, str):
        if normalization not in ("none", "sqrt", "seqlen"):
            raise ValueError(f"msa_neff: normalization={normalization!r} is not one of 'none', 'sqrt', 'seqlen' or a number")
        normalization = {"none": 1, "sqrt": math.sqrt(u8.shape[1]), "seqlen": u8.shape[1]}[normalization]
    return float(ops.msa_neff(u8, seqid_cutoff).neff.item()) / normalization


def msa_coverage(tokens: np.ndarray, gap_idx: int, device) -> np.ndarray:
    """The coverage property (utils/align.py:242-247): per column the share of rows that hold no gap, float64 [L] (no <cls>).  On the
    HIP device only (rnamsm_msa_coverage)."""
    from . import ops
    return ops.msa_coverage(_stats_body_device(tokens, device, "msa_coverage"), int(gap_idx)).cpu().numpy()


def sample_weights(tokens: np.ndarray, num_seqs: int, rng=None, seqid_cutoff: float = 0.2, device=None) -> np.ndarray:
    """Row indices drawn like MSA.sample_weights (utils/align.py:150-163): row 0 plus num_seqs - 1 of the others without
    replacement with probability proportional to their sequence weight, ascending.  `rng`: a numpy RandomState; None =
    numpy's global one, which is what the reference draws from (seeded by seed_everything(42), RNA_MSM_Inference.py:17)."""
    depth = tokens.shape[0]
    if depth <= num_seqs:
        return np.arange(depth)
    rng = np.random if rng is None else rng
    w = msa_weights(tokens, seqid_cutoff, device)[1:]
    w = w / w.sum()
    idx = rng.choice(depth - 1, size=num_seqs - 1, replace=False, p=w) + 1
    return np.append(0, np.sort(idx))


def check_seqid_filter_args(num_seqs: int, min_seqid: int, max_seqid: int, step: int, prefix: str = "seqid_filter: ") -> None:
    """The filter's limits (include/rnamsm.h); the message names the value.  prefix: what stands in front of the name (the CLI's keys)."""
    for name, value in (("num_seqs", num_seqs), ("min_seqid", min_seqid), ("max_seqid", max_seqid), ("step", step)):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
            raise ValueError(f"{prefix}{name}={value!r} is not an integer")
    if num_seqs < 0:
        raise ValueError(f"{prefix}num_seqs={num_seqs} is negative")
    if min_seqid < 1:
        raise ValueError(f"{prefix}min_seqid={min_seqid} is below 1")
    if not 1 <= max_seqid <= 100:
        raise ValueError(f"{prefix}max_seqid={max_seqid} outside [1, 100]")
    if step < 1:
        raise ValueError(f"{prefix}step={step} is below 1")


def seqid_thresholds(num_seqs: int, min_seqid: int = 20, max_seqid: int = 90, step: int = 5) -> List[int]:
    """The thresholds of the filter's passes: num_seqs > 0: min_seqid, min_seqid + step, ... while below max_seqid, then max_seqid;
    num_seqs == 0, or min_seqid >= max_seqid: max_seqid alone."""
    check_seqid_filter_args(num_seqs, min_seqid, max_seqid, step)
    return (list(range(min_seqid, max_seqid, step)) if num_seqs > 0 else []) + [max_seqid]


def seqid_order(body: np.ndarray, gap: int) -> np.ndarray:
    """The order the filter walks the rows in: row 0, then the others by descending number of residues, ties by ascending index."""
    nres = (body != gap).sum(1)
    return np.concatenate([[0], np.argsort(-nres[1:], kind="stable") + 1]).astype(np.int64)


def seqid_filter_host(body: np.ndarray, gap: int, num_seqs: int, min_seqid: int = 20, max_seqid: int = 90, step: int = 5,
                      order=None) -> Tuple[np.ndarray, np.ndarray]:
    """The identity redundancy filter on the host: body uint8 [N, L] (the alignment's columns, no <cls>) -> (kept row indices
    ascending int64, kept_at int32 [N]: per row the threshold of the pass that kept it, -1 for a row never kept).  The rule is
    include/rnamsm.h's (rnamsm_seqid_filter) -- a rule of this project's own, modelled on the reference's `hhfilter -id 90 -diff
    num_seqs` and not that binary's algorithm -- in integers, vectorised per candidate (one comparison of a row against all rows kept
    so far): index-identical to the device."""
    thresholds = seqid_thresholds(num_seqs, min_seqid, max_seqid, step)
    body = np.ascontiguousarray(body, dtype=np.uint8)
    N, L = body.shape
    order = seqid_order(body, gap) if order is None else np.asarray(order, dtype=np.int64)
    if order.shape != (N,):
        raise ValueError(f"seqid_filter: expected an order of {N} entries, got {order.shape}")
    bad = np.flatnonzero((order < 0) | (order >= N))
    if bad.size:
        raise ValueError(f"seqid_filter: order[{int(bad[0])}] lies outside [0, {N})")
    res = body != gap
    nres = res.sum(1)
    kept_at = np.full(N, -1, dtype=np.int32)
    k_body, k_res, nk = np.empty_like(body), np.empty_like(res), 0
    for t in thresholds:
        for pos, r in enumerate(order):
            if kept_at[r] >= 0 or (nres[r] == 0 and pos != 0):
                continue
            if nk:
                m = k_res[:nk] & res[r]
                both = m.sum(1, dtype=np.int64)
                same = (m & (k_body[:nk] == body[r])).sum(1, dtype=np.int64)
                if ((both > 0) & (100 * same >= t * both)).any():
                    continue
            k_body[nk], k_res[nk], kept_at[r] = body[r], res[r], t
            nk += 1
        if num_seqs > 0 and nk >= num_seqs:
            break
    return np.flatnonzero(kept_at >= 0).astype(np.int64), kept_at


def seqid_filter(tokens: np.ndarray, gap_idx: int, num_seqs: int, min_seqid: int = 20, max_seqid: int = 90, step: int = 5,
                 device=None) -> np.ndarray:
    """Row indices (ascending int64) of the non-redundant rows of an alignment, by the identity redundancy filter: passes at the
    thresholds min_seqid, min_seqid + step, ..., max_seqid (per cent identity over the columns where both rows have a residue) until
    num_seqs rows are kept; num_seqs = 0: one pass at max_seqid.  In a pass the rows are walked longest first behind row 0 and a row
    is kept unless it is that identical to a row already kept.  A rule of this project's own, modelled on the reference's
    `hhfilter -id 90 -diff num_seqs` (utils/align.py:68-102); it does NOT reproduce that binary (whose -diff counts sequences per
    window of 50 columns).  The columns are the alignment's (no <cls>, as in msa_weights).  With `device` (a HIP device) it runs
    there (rnamsm_seqid_filter), else on the host (seqid_filter_host): the same indices either way.  More than num_seqs rows may come
    back; cutting is the caller's."""
    body = tokens[:, 1:] if tokens.shape[1] > 1 else tokens
    if body.size and (int(body.min()) < 0 or int(body.max()) > 255):
        raise ValueError("seqid_filter: token ids outside [0, 255]")
    body = np.ascontiguousarray(body.astype(np.uint8))
    if device is None:
        return seqid_filter_host(body, int(gap_idx), num_seqs, min_seqid, max_seqid, step)[0]
    import torch
    from . import ops
    check_seqid_filter_args(num_seqs, min_seqid, max_seqid, step)
    rec = ops.seqid_filter(torch.from_numpy(body).to(device), int(gap_idx), num_seqs, min_seqid, max_seqid, step)
    return rec.indices.cpu().numpy().astype(np.int64)


def load_msa_tokens(path: Union[str, Path], alphabet: RNAAlphabet, max_seqs_per_msa: int = 512,
                    sample_method: str = "hhfilter", device=None, rng=None, on_full=None, filter_seqid=(20, 90, 5)) -> np.ndarray:
    """.a2m_msa2 file -> int64 tokens [R <= max_seqs, L+1].  With `device` (a HIP device) the sub-sampling arithmetic
    (greedy selection, sequence weights, the redundancy filter) runs on the GPU.  `rng` feeds `sample-pretrained` (see
    sample_weights).  `on_full`: called with the tokens of the alignment as read, every row, before anything is sub-sampled.
    `seqid-filter`: seqid_filter with num_seqs = max_seqs_per_msa and filter_seqid = (min_seqid, max_seqid, step), then the first
    max_seqs_per_msa of the kept rows (all of them where fewer are kept) -- this project's stand-in for the reference's hhfilter
    default, not that binary's selection."""
    if sample_method not in SAMPLE_METHODS:
        raise AssertionError(f"unknown sample_method {sample_method!r}")
    records = read_fasta_records(path)
    tokens = alphabet.encode_a2m_records([seq for _, seq in records])
    if on_full is not None:
        on_full(tokens)
    if max_seqs_per_msa is None or tokens.shape[0] <= max_seqs_per_msa:
        return tokens
    if sample_method == "first":
        return tokens[:max_seqs_per_msa]
    if sample_method in ("diversity-max", "diversity-min"):
        mode = sample_method.split("-")[1]
        if device is not None:
            return tokens[greedy_select_device(tokens, max_seqs_per_msa, mode, device)]
        return tokens[greedy_select(tokens, max_seqs_per_msa, mode)]
    if sample_method == "sample-pretrained":
        return tokens[sample_weights(tokens, max_seqs_per_msa, rng, device=device)]
    if sample_method == "seqid-filter":
        lo, hi, step = filter_seqid
        kept = seqid_filter(tokens, alphabet.tok_to_idx["-"], max_seqs_per_msa, lo, hi, step, device=device)
        return tokens[kept[:max_seqs_per_msa]]
    raise NotImplementedError(
        f"sample_method={sample_method!r} needs the external hhfilter binary of the reference (utils/align.py:68-102); "
        "pre-filter the alignment or pass data.sample_method=seqid-filter (this project's identity filter, not hhfilter's "
        "selection) | first | diversity-max | diversity-min | sample-pretrained")
