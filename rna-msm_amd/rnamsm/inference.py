"""extract_feat: the reference CLI's per-RNA loop (RNA_MSM_Inference.py:90-168) on the HIP path.

For every id in `data.MSA_list` (sorted), reads `<root>/<MSA_path>/<id>.a2m_msa2`, runs the 10-layer forward and
writes `<id>_emb.npy` float32 (L, 768) and `<id>_atp.npy` float32 (120, L, L) -- the NPY v1 C-order files the
downstream SS / RSA predictors consume.  With torch.distributed initialised (one process per GPU),
ids are sharded round-robin over ranks and either written by the rank that computed them (default) or gathered
to rank 0 over RCCL first (`gather_to_rank0=True`).
"""
from __future__ import annotations

import json
import math
import os
import queue
import random
import threading
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import _lib, contacts, lm, metrics, ops, rsa, sharding, ss
from .alphabet import RNAAlphabet
from .config import Config, check_filter_seqid, check_invcov, check_long_heads, check_long_msa, check_mi, check_mi_gaps, check_mi_weights, check_msa_stats, check_ss_gemm_dtype, check_ss_nested, check_target_dir, check_top_pairs
from .model import MSATransformer
from .msa import load_msa_tokens, msa_invcov_device, msa_mi_device, msa_mi_weighted_device, msa_stats_device


def load_checkpoint(model: MSATransformer, path: str, device) -> None:
    """torch.load(path)['state_dict'] with strict key matching (RNA_MSM_Inference.py:133-135)."""
    blob = torch.load(path, map_location="cpu", weights_only=False)
    state = blob["state_dict"] if isinstance(blob, dict) and "state_dict" in blob else blob
    model.load_state_dict(state, strict=True)


def find_msa_files(msa_dir: Path, ids: List[str]) -> Dict[str, Path]:
    """`*.a2m_msa2` files whose stem (up to the first '.') is a requested id (dataset.py:46-64)."""
    if not msa_dir.exists():
        raise FileNotFoundError(msa_dir)
    if not msa_dir.is_dir():
        raise NotADirectoryError(msa_dir)
    wanted = set(ids)
    if not wanted:
        raise ValueError("Passed an empty split file set")
    found = {f.stem.split(".")[0]: f for f in sorted(msa_dir.glob("*.a2m_msa2")) if f.stem.split(".")[0] in wanted}
    if len(found) != len(wanted):
        raise FileNotFoundError(f"{len(wanted) - len(found)} specified split files not found in directory")
    return found


def crop_tokens(tokens: np.ndarray, max_seqlen: int, rng: np.random.RandomState) -> np.ndarray:
    """RandomCropDataset.__getitem__ (dataset.py:142-158): when the alignment (incl. <cls>) is wider than
    max_seqlen keep <cls> plus a random window of max_seqlen - 1 columns."""
    seqlen = tokens.shape[-1]
    if seqlen <= max_seqlen:
        return tokens
    start = rng.randint(1, seqlen - max_seqlen) if seqlen - max_seqlen > 1 else 1
    return np.concatenate([tokens[..., :1], tokens[..., start:start + max_seqlen - 1]], -1)


class _AsyncNpyWriter:
    """Device tensors -> `.npy` files off the critical path: the D2H copy runs on a side stream into pinned buffers and a
    worker thread waits for it and calls np.save, so the GPU starts the next MSA while this one's 126 MB (L = 512) of maps
    are still on their way to disk.  At most `depth` MSAs wait in the queue and `workers` are being written (bounds the pinned memory).  `workers` threads share
    the queue (np.save releases the GIL while it writes: a list of small alignments is bound by the writer, 442 MB for 64 of
    them); an alignment's two files are written by one worker, alignments may finish out of order.  `close()` drains the
    queue and re-raises a worker exception."""

    def __init__(self, device: torch.device, depth: int = 2, workers: int = 2):
        self._stream = torch.cuda.Stream(device)
        self._q: "queue.Queue" = queue.Queue(maxsize=depth)
        self._err: Optional[BaseException] = None
        self._threads = [threading.Thread(target=self._run, name=f"rnamsm-npy-writer-{i}", daemon=True) for i in range(workers)]
        for t in self._threads:
            t.start()

    def _run(self) -> None:
        while True:
            item = self._q.get()
            if item is None:
                return
            event, jobs, done = item
            try:
                if self._err is None:
                    event.synchronize()
                    for path, hosts in jobs:
                        if callable(path):                  # a host-side consumer (a head's text files) instead of a .npy
                            path(*(h.numpy() for h in hosts))
                        else:
                            np.save(path, hosts[0].numpy())
                    done()
            except BaseException as e:                  # noqa: BLE001  (reported by close())
                self._err = e

    def submit(self, jobs, done, after: Optional[torch.cuda.Event] = None) -> None:
        """jobs: [(path, device tensor)], written in this order; a callable in place of the path is called with the host array, or,
        where the job carries a tuple of tensors, with the host array of each; done(): called by the worker after the last file.
        after: an event recorded behind the kernels that produced the tensors -- the copies then wait for THAT point of the compute
        stream only, not for what was enqueued since (the next packed group's forward: the CLI's pipelined pool); None = for
        everything enqueued so far."""
        if after is not None:
            self._stream.wait_event(after)
        else:
            self._stream.wait_stream(torch.cuda.current_stream())
        staged = []
        with torch.cuda.stream(self._stream):
            for path, tensors in jobs:
                hosts = []
                for t in tensors if isinstance(tensors, tuple) else (tensors,):
                    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                    host.copy_(t, non_blocking=True)
                    t.record_stream(self._stream)       # the allocator must not recycle t before the copy has run
                    hosts.append(host)
                staged.append((path, hosts))
            event = torch.cuda.Event()
            event.record(self._stream)
        self._q.put((event, staged, done))              # blocks when `depth` MSAs are already in flight

    def close(self) -> None:
        for _ in self._threads:
            self._q.put(None)
        for t in self._threads:
            t.join()
        if self._err is not None:
            raise self._err


# data.batch_small_msas: which alignments wait for company, and when a group is full.  An alignment of up to SMALL_MSA_TOKENS
# tokens is "small"; a group's frame -- members x max rows x max columns -- stays within FRAME_TOKENS and within twice the real
# tokens, and holds at most GROUP_MEMBERS alignments.  (The limit was 1536 tokens while groups were formed in list order: from
# ~2 k tokens on the padding of an ill-matched frame cost more than the shared launches returned, tools/ragged_batch_timing.py.
# With groups formed by shape -- plan_groups -- frames are tight and 3072 measured x1.82 against x1.54 on a list of 4-24 rows x
# 40-120 columns, tools/cli_throughput.py.)
# (Frames: 16 k tokens / 32 members until the pool existed; a batch of 64 alignments of 8 x 64 runs at 676 k residues/s against
# 649 k for 32 -- GEMM tile quantisation shrinks with the token count, tools/small_batch_knobs.py -- hence 32 k / 64.)
SMALL_MSA_TOKENS, FRAME_TOKENS, GROUP_MEMBERS = 3072, 32768, 64
# ... and within FRAME_MAP_ELEMS = members x (max columns)^2: the maps (row_attn and atp: layers x heads x C^2 floats per member,
# 480 B per element at 10 x 12) scale with C^2, not with the tokens -- 32 shallow alignments of 1 x 1024 would be 16 GB of maps for
# a frame of 32 k tokens, and batching gains nothing at that C.  2^20 elements = 0.5 GB of atp per group: 64 members up to C = 128,
# 16 at C = 256, none above C = 1024 / alone.
FRAME_MAP_ELEMS = 1 << 20


def joins_group(group_shapes: List[tuple], shape: tuple) -> bool:
    """Does a small alignment of `shape` (rows, columns) join the waiting group, or must the group be flushed first?"""
    if len(group_shapes) >= GROUP_MEMBERS:
        return False
    trial = list(group_shapes) + [shape]
    cols = max(s[1] for s in trial)
    frame = len(trial) * max(s[0] for s in trial) * cols
    return frame <= FRAME_TOKENS and frame <= 2 * sum(s[0] * s[1] for s in trial) and len(trial) * cols * cols <= FRAME_MAP_ELEMS


# Without a gather the order in which alignments are computed is free (every alignment has its own files), so the small ones
# of the list wait in a POOL (at most POOL_MSAS of them) and are grouped by shape instead of by list position: sorted by
# (rows, columns) a frame's members are alike, groups fill up to GROUP_MEMBERS / FRAME_TOKENS instead of stopping at the first
# alignment that would pad too much, and a large alignment in between no longer flushes anything.  64 alignments of 2-12 rows
# x 40-80 columns: 12 groups in list order, 4 sorted (tools/cli_throughput.py).
POOL_MSAS = 256


# what one more launch set costs, in tokens of frame (~5.5 ms at ~600 k tokens/s): the padding one more member may add to a frame.
# (Half and a quarter of it -- tighter frames, more groups -- measured the same within 5 % on lists of 64 and 256 alignments.)
GROUP_OVERHEAD_TOKENS = 3300


def _greedy_groups(shapes: List[tuple], order: List[int]) -> List[List[int]]:
    """Fill groups in the given order; an alignment joins the waiting group while joins_group allows it AND the padding it adds
    to the frame costs less than a launch set of its own (GROUP_OVERHEAD_TOKENS)."""
    groups: List[List[int]] = []
    cur: List[int] = []
    rows = cols = 0
    for j in order:
        r, c = shapes[j]
        if cur:
            grown = (len(cur) + 1) * max(rows, r) * max(cols, c) - len(cur) * rows * cols       # what the frame grows by
            if not joins_group([shapes[i] for i in cur], shapes[j]) or grown - r * c > GROUP_OVERHEAD_TOKENS:
                groups.append(sorted(cur))
                cur, rows, cols = [], 0, 0
        cur.append(j)
        rows, cols = max(rows, r), max(cols, c)
    if cur:
        groups.append(sorted(cur))
    return groups


def _clustered_groups(shapes: List[tuple]) -> List[List[int]]:
    """Seed a group with the largest alignment left, then keep adding the one that pads the frame least (joins_group's rule,
    evaluated for all candidates at once) while that padding costs less than a launch set of its own."""
    rc = np.asarray(shapes, dtype=np.int64).reshape(-1, 2)
    tok = rc[:, 0] * rc[:, 1]
    left = np.ones(len(shapes), dtype=bool)
    groups: List[List[int]] = []
    while left.any():
        seed = int(np.flatnonzero(left)[np.argmax(tok[left])])         # (the first of equals)
        left[seed] = False
        g, rows, cols, real = [seed], int(rc[seed, 0]), int(rc[seed, 1]), int(tok[seed])
        while len(g) < GROUP_MEMBERS and left.any():
            frame = (len(g) + 1) * np.maximum(rows, rc[:, 0]) * np.maximum(cols, rc[:, 1])
            ok = left & (frame <= FRAME_TOKENS) & (frame <= 2 * (real + tok))
            ok &= (len(g) + 1) * np.maximum(cols, rc[:, 1]) ** 2 <= FRAME_MAP_ELEMS
            added_padding = frame - len(g) * rows * cols - tok
            ok &= added_padding <= GROUP_OVERHEAD_TOKENS
            if not ok.any():
                break
            best = int(np.argmin(np.where(ok, added_padding, np.iinfo(np.int64).max)))
            left[best] = False
            g.append(best)
            rows, cols, real = max(rows, int(rc[best, 0])), max(cols, int(rc[best, 1])), real + int(tok[best])
        groups.append(sorted(g))
    return groups


def frame_tokens(shapes: List[tuple], groups: List[List[int]]) -> int:
    return sum(len(g) * max(shapes[j][0] for j in g) * max(shapes[j][1] for j in g) for g in groups)


def plan_groups(shapes: List[tuple]) -> List[List[int]]:
    """Partition pooled small alignments (`shapes` = (rows, columns) each) into ragged-batch groups; returns lists of
    positions into `shapes`, every position exactly once, members of a group in ascending position.  Two plans are made -- fill
    greedily in (rows, columns) order; cluster around the largest alignment left -- and the one with the smaller cost (tokens
    of frame, padding included, plus GROUP_OVERHEAD_TOKENS per group) is taken, the first on a tie.  Lists of 64 / 256
    alignments of 2-12 rows x 40-80 columns: 3 / 7 groups, x3.6 / x4.6 against one by one; of 4-24 x 40-120: 6 / 15 groups, x1.9 /
    x2.3 (tools/cli_throughput.py)."""
    if not shapes:
        return []
    plans = [_greedy_groups(shapes, sorted(range(len(shapes)), key=lambda j: (shapes[j][0], shapes[j][1], j))),
             _clustered_groups(shapes)]
    cost = [frame_tokens(shapes, p) + GROUP_OVERHEAD_TOKENS * len(p) for p in plans]
    return plans[0] if cost[0] <= cost[1] else plans[1]


# ---- token-packed groups (exact mode, data.pack_small_msas; round 4): forward_ragged then runs rnamsm_forward_packed, which
# pads nothing, so a group is bounded by what it really holds -- PACKED_TOKENS tokens, PACKED_MEMBERS members, FRAME_MAP_ELEMS map
# elements (sum of C^2) -- and shapes need not match: groups are cut in list order (the gather path keeps its order for free).
# Measured (tools/packed_batch_timing.py, 4-24 rows x 41-121 columns): 4 k tokens 361 k residues/s, 10 k 522 k, 21 k 633 k, 34 k 621 k,
# 49 k 678 k, 66 k 689 k (GEMM tile quantisation and the folded LayerNorm's threshold) against 147 k one by one -- hence 64 k
# tokens / 256 members; and alignments of up to PACKED_SMALL_TOKENS wait for company (16-64 rows x 60-200 columns, ~5 k tokens
# each: x1.4-1.5 packed against alone; framed they lost).
# (round 5: 8192 -> 16384 -- 64 alignments of 16-64 rows x 60-200 columns: 96.2 -> 100.1 MSA/s, f16x3 172.5 -> 180.8, bf16 neutral and
# left at 8192; tools/cli_throughput.py with PACKED_SMALL / PACKED_SMALL_16)
# (PACKED_TOKENS 65536 -> 131072: a 77 k-token list of small alignments as one group instead of two: 385 -> 408 MSA/s)
PACKED_TOKENS, PACKED_MEMBERS, PACKED_SMALL_TOKENS = 131072, 256, 16384
# The CLI's pooled path pipelines its token-packed groups (group g+1 enqueued before group g's error word is read); a pool that would be
# one group of at least this many tokens is dealt into two so that there is something to overlap (RNAMSM_PIPELINE_SPLIT_TOKENS: A/B, 0 = never)
PIPELINE_SPLIT_TOKENS = int(os.environ.get("RNAMSM_PIPELINE_SPLIT_TOKENS", "24576"))
# In a 16-bit arithmetic mode the packed batch runs in that mode too since round 5 (rnamsm_forward_packed: every Linear on the
# 16-bit matrix cores, attention on the exact descriptor kernels), so the same limit applies.  (Round 4 had sent those small
# alignments through the EXACT packed path, with limits of 1024 / 2048 tokens: there was no 16-bit packed batch.)
PACKED_SMALL_TOKENS_16BIT = {"bf16": 8192, "f16x3": 16384}


def r_c_below(shape: tuple, limit: int) -> bool:
    return shape[0] * shape[1] < limit


def joins_packed(group_shapes: List[tuple], shape: tuple) -> bool:
    """Does a small alignment of `shape` join the waiting token-packed group?"""
    trial = list(group_shapes) + [shape]
    return (len(trial) <= PACKED_MEMBERS and sum(r * c for r, c in trial) <= PACKED_TOKENS
            and sum(c * c for _, c in trial) <= FRAME_MAP_ELEMS)


def plan_packed_groups(shapes: List[tuple], fold_min_tokens: int = 0, split_tokens: int = 0, _min_groups: int = 1) -> List[List[int]]:
    """Partition pooled small alignments into token-packed groups, in list order, every position exactly once.  The number of
    groups is the least the three bounds allow; members are then dealt so that the groups hold about the same number of tokens
    (64 + 6 alignments would otherwise run as one full group and one nearly empty launch set).
    fold_min_tokens > 0 (exact mode): alignments of at least that many tokens take the folded LayerNorm, smaller ones do not, and a
    launch set is one or the other -- the two classes are planned separately, so that no group has to be run as two batches
    (MSATransformer.forward_packed would split a mixed one: correct, but two launch sets).
    split_tokens > 0: a pool that would run as ONE group IN ALL, of at least that many tokens, is dealt into two, so that the caller
    has something to pipeline (the second group's forward over the first one's deliveries: +7 % on 64 small alignments; a pool of
    several groups pipelines already, and splitting its smaller class measured -2 %: profiles/r06_cli_pipeline_ab.log)."""
    if not shapes:
        return []
    if split_tokens > 0:
        plan = plan_packed_groups(shapes, fold_min_tokens)
        if len(plan) == 1 and len(shapes) >= 2 and sum(r * c for r, c in shapes) >= split_tokens:
            plan = plan_packed_groups(shapes, 0, 0, 2)
        return plan
    if fold_min_tokens > 0:
        big = [j for j, (r, c) in enumerate(shapes) if r * c >= fold_min_tokens]
        if 0 < len(big) < len(shapes):
            small = [j for j in range(len(shapes)) if r_c_below(shapes[j], fold_min_tokens)]
            return ([[big[j] for j in g] for g in plan_packed_groups([shapes[j] for j in big])]
                    + [[small[j] for j in g] for g in plan_packed_groups([shapes[j] for j in small])])
    tok = [r * c for r, c in shapes]
    k = max(-(-len(shapes) // PACKED_MEMBERS), -(-sum(tok) // PACKED_TOKENS), -(-sum(c * c for _, c in shapes) // FRAME_MAP_ELEMS), _min_groups)
    while True:
        # next-fit with a soft budget of 1/k of the tokens: a group closes once it has reached the budget (the member that crosses
        # it still joins, bounds permitting), or earlier when the next member would break a hard bound
        budget = -(-sum(tok) // k)
        groups: List[List[int]] = [[]]
        t = 0
        for j in range(len(shapes)):
            if groups[-1] and (t >= budget or not joins_packed([shapes[i] for i in groups[-1]], shapes[j])):
                groups.append([])
                t = 0
            groups[-1].append(j)
            t += tok[j]
        if len(groups) <= k:
            return groups
        k = len(groups)             # the hard bounds cut earlier than planned: aim for that many, evenly filled


class _Switches(NamedTuple):
    """Every optional cfg.data.* / cfg.model.* key the CLI loop reads, and what follows from them (read_switches)."""
    gemm_dtype: str             # model.gemm_dtype
    ss_dtype: str               # data.ss_gemm_dtype
    windowing: bool             # data.long_msa=windows
    window_stride: int          # data.window_stride
    long_heads: bool            # data.long_heads=stitched
    invcov_on: bool             # data.invcov
    msa_stats_on: bool          # data.msa_stats
    mi_on: bool                 # data.mi
    mi_gaps: str                # data.mi_gaps
    mi_weighted: bool           # data.mi_weights=seqid
    seqid_cutoff: float         # data.seqid_cutoff where the configuration has one, else the reference's default
    filter_seqid: tuple         # data.filter_min_seqid, data.filter_max_seqid, data.filter_step (sample_method=seqid-filter)
    gathering: bool             # gather_to_rank0 with more than one rank
    ss_path: str                # data.ss_model_path
    rsa_dir: str                # data.rsa_model_dir
    ss_text: bool               # data.ss_prob_text, data.ss_pairs_device, data.rsa_text_device: off under a gather
    ss_pairs: bool
    rsa_text: bool
    contacts: bool              # data.contacts
    lm_mode: str                # data.lm_scores
    exact: bool                 # the model runs in fp32
    packing: bool               # small alignments share token-packed groups (else: padded frames)
    batching: bool              # small alignments share groups at all
    pooled: bool                # ... formed from the pool, by shape, instead of in list order
    small_limit: int            # tokens up to which an alignment waits for company
    top_pairs: str = ""         # data.top_pairs: "" = off, else the spec of the ranked lists' length
    top_pairs_min_sep: int = 1  # data.top_pairs_min_sep
    target_dir: str = ""        # data.target_dir: "" = off, else the directory of the known structures
    target_min_sep: int = 1     # data.target_min_sep
    ss_nested: Optional[tuple] = None      # data.ss_nested: None = off, else (data.ss_nested_threshold, data.ss_nested_min_loop)


def refuse_top_pairs_under_gather(top_pairs: str, gathering: bool) -> None:
    if top_pairs and gathering:
        raise ValueError(f"data.top_pairs={top_pairs!r} is not available with RNAMSM_GATHER_TO_RANK0=1: the ranked lists are made from the "
                         f"maps where they lie on the computing rank's device, and the gather carries no such list; run without the "
                         f"gather (every rank then writes its own files) or without the key")


def refuse_target_dir_under_gather(target_dir: str, gathering: bool) -> None:
    if target_dir and gathering:
        raise ValueError(f"data.target_dir={target_dir!r} is not available with RNAMSM_GATHER_TO_RANK0=1: the counts are made from the "
                         f"maps where they lie on the computing rank's device, and the gather carries no such record; run without the "
                         f"gather (every rank then writes its own files) or without the key")


def refuse_ss_nested_under_gather(on: bool, gathering: bool) -> None:
    if on and gathering:
        raise ValueError("data.ss_nested=true is not available with RNAMSM_GATHER_TO_RANK0=1: the nested structure is decoded from the "
                         "probabilities where they lie on the computing rank's device, and the gather carries no such record; run "
                         "without the gather (every rank then writes its own files) or without the key")


def read_switches(cfg: Config, gathering: bool) -> _Switches:
    """The keys are read and checked here, once, before anything is loaded; the module's limits as they stand at this call."""
    ss_dtype = check_ss_gemm_dtype(getattr(cfg.data, "ss_gemm_dtype", "f32"))
    # data.long_msa=windows: an alignment wider than the model's max_seqlen is not cropped (nothing is drawn for it) and runs as
    # overlapping windows stitched on the device (MSATransformer.forward_windows): its files hold the full L
    windowing = check_long_msa(getattr(cfg.data, "long_msa", "crop")) == "windows"
    window_stride = int(getattr(cfg.data, "window_stride", 0))
    # data.long_heads=stitched: on such an alignment the contact head and the exact-fp32 SS head run on the stitched atp, and the RSA
    # head on the stitched emb, through the long entry points (L <= _lib.LONG_MAX_L); "skip" leaves everything as it was, the printed lines included
    long_heads = check_long_heads(getattr(cfg.data, "long_heads", "skip")) == "stitched"
    # data.invcov: the covariance contact map of every alignment as read -- all rows, all columns -- made on the reader's side and
    # written as <id>_invcov.npy by one more writer job; off, nothing below differs
    invcov_on = check_invcov(getattr(cfg.data, "invcov", False))
    # data.msa_stats: the sequence weights, the coverage and Neff of every alignment as read, made on the reader's side like the map
    # above and written as <id>_weights.npy / <id>_coverage.npy by two more writer jobs; off, nothing below differs
    msa_stats_on = check_msa_stats(getattr(cfg.data, "msa_stats", False))
    seqid_cutoff = float(getattr(cfg.data, "seqid_cutoff", 0.2))
    # data.mi: the mutual-information maps of every alignment as read, made on the reader's side like the two above and written as
    # <id>_mi.npy / <id>_mip.npy by two more writer jobs; off, nothing below differs
    mi_on = check_mi(getattr(cfg.data, "mi", False))
    mi_gaps = check_mi_gaps(getattr(cfg.data, "mi_gaps", "pairwise"))
    # data.mi_weights=seqid: the pair is the sequence-weighted one and goes to <id>_wmi.npy / <id>_wmip.npy instead; the same two
    # tensors per item travel the same way
    mi_weighted = check_mi_weights(getattr(cfg.data, "mi_weights", "none"), mi_on) == "seqid"
    # data.sample_method=seqid-filter: the thresholds of the identity redundancy filter (rnamsm.msa.seqid_filter); the sub-sampling
    # happens behind on_full, so the statistics and maps of the alignment as read see every row whatever the method
    filter_seqid = check_filter_seqid(getattr(cfg.data, "filter_min_seqid", 20), getattr(cfg.data, "filter_max_seqid", 90),
                                      getattr(cfg.data, "filter_step", 5))
    # data.top_pairs: a ranked list of the strongest pairs beside every pair map the run writes, made on the device in the sink; off,
    # nothing below differs.  Under a gather the maps reach rank 0 as host-staged items and the device text outputs are off: refused
    top_pairs, top_pairs_min_sep = check_top_pairs(getattr(cfg.data, "top_pairs", ""), getattr(cfg.data, "top_pairs_min_sep", 1))
    refuse_top_pairs_under_gather(top_pairs, gathering)
    # data.target_dir: the accuracy of every map against a known structure, counted on the device in the sink; off, nothing differs
    target_dir, target_min_sep = check_target_dir(getattr(cfg.data, "target_dir", ""), getattr(cfg.data, "target_min_sep", 1))
    refuse_target_dir_under_gather(target_dir, gathering)
    # data.ss_nested: the nested structure of every alignment the SS head runs on, decoded on the device behind it; off, nothing differs
    nested_theta, nested_loop = getattr(cfg.data, "ss_nested_threshold", 0.516), getattr(cfg.data, "ss_nested_min_loop", 3)
    nested_on = check_ss_nested(getattr(cfg.data, "ss_nested", False), nested_theta, nested_loop, getattr(cfg.data, "ss_model_path", ""))
    refuse_ss_nested_under_gather(nested_on, gathering)
    # data.batch_small_msas: small alignments go through ONE launch set per group (forward_ragged: padded into one
    # frame, every MSA scaled by its own depth); a lone forward of a few hundred tokens costs 5.5 ms on a mostly
    # idle chip.  Groups: by shape from the pool (plan_groups); under gather_to_rank0 the RoundGatherer needs this
    # rank's items in list order, so there only CONSECUTIVE small alignments share a group.
    # (16-bit modes: only with data.batch_small_msas_16bit -- a batch's token count selects the GEMM kernels there, so
    # an alignment's files would depend on its neighbours in the list at the mode's rounding level)
    exact = cfg.model.gemm_dtype == "f32"
    framed16 = bool(getattr(cfg.data, "batch_small_msas_16bit", False)) and ops.get_param("attn16") != 0
    # groups are token-packed (no frame, no padding -- rnamsm_forward_packed, in the model's arithmetic mode), so any small
    # alignments share one -- unless 16-bit framed batches were asked for (data.batch_small_msas_16bit)
    packing = (bool(getattr(cfg.data, "batch_small_msas", True)) and bool(getattr(cfg.data, "pack_small_msas", True))
               and (exact or not framed16))
    batching = bool(getattr(cfg.data, "batch_small_msas", True)) and (exact or framed16 or packing)
    small_limit = (PACKED_SMALL_TOKENS if exact else PACKED_SMALL_TOKENS_16BIT.get(cfg.model.gemm_dtype, 1024)) if packing else SMALL_MSA_TOKENS
    return _Switches(
        gemm_dtype=cfg.model.gemm_dtype, ss_dtype=ss_dtype, windowing=windowing, window_stride=window_stride, long_heads=long_heads,
        invcov_on=invcov_on, msa_stats_on=msa_stats_on, mi_on=mi_on, mi_gaps=mi_gaps, mi_weighted=mi_weighted, seqid_cutoff=seqid_cutoff, filter_seqid=filter_seqid, gathering=gathering, ss_path=getattr(cfg.data, "ss_model_path", ""),
        rsa_dir=getattr(cfg.data, "rsa_model_dir", ""), ss_text=bool(getattr(cfg.data, "ss_prob_text", True)) and not gathering,
        ss_pairs=bool(getattr(cfg.data, "ss_pairs_device", True)) and not gathering,
        rsa_text=bool(getattr(cfg.data, "rsa_text_device", True)) and not gathering, contacts=bool(getattr(cfg.data, "contacts", False)),
        lm_mode=lm.check_lm_scores(getattr(cfg.data, "lm_scores", "")), exact=exact, packing=packing, batching=batching,
        pooled=batching and not gathering, small_limit=small_limit, top_pairs=top_pairs, top_pairs_min_sep=top_pairs_min_sep,
        target_dir=target_dir, target_min_sep=target_min_sep, ss_nested=(float(nested_theta), int(nested_loop)) if nested_on else None)


def _load_model(cfg: Config, model: Optional[MSATransformer], alphabet, device) -> MSATransformer:
    if model is None:
        model = MSATransformer(alphabet, embed_dim=cfg.model.embed_dim, num_attention_heads=cfg.model.num_attention_heads,
                               num_layers=cfg.model.num_layers, embed_positions_msa=cfg.model.embed_positions_msa,
                               dropout=cfg.model.dropout, attention_dropout=cfg.model.attention_dropout,
                               activation_dropout=cfg.model.activation_dropout, max_tokens_per_msa=cfg.data.max_tokens,
                               max_seqlen=cfg.data.max_seqlen)
        load_checkpoint(model, cfg.data.model_path, device)
    model = model.eval().to(device)
    model.gemm_dtype = cfg.model.gemm_dtype
    return model


def _load_heads(sw: _Switches, model: MSATransformer, alphabet, device, rank: int) -> list:
    """The heads that are on, SS before RSA before the contacts before the LM scores: each reads an alignment's device-resident outputs and makes one record
    of it (rnamsm.ss.SSHead: data.ss_model_path, the maps; rnamsm.rsa.RSAHead: data.rsa_model_dir, the embedding;
    rnamsm.contacts.ContactHead: data.contacts, the maps; rnamsm.lm.LMHead: data.lm_scores, the embedding and the tokens).
    data.ss_prob_text (default on): the `.prob` text is formatted on the device behind the head (rnamsm.ss.prob_text) and the
    writer thread's share of it is one binary write, where np.savetxt formats L^2 numbers under the GIL; the files are the same
    bytes.  data.ss_pairs_device (default on): the pairs are decoded and the bodies of `.ct` / `.bpseq` written on the device too
    (rnamsm.ss.structure), so the writer thread no longer runs secondary_structure and two np.savetxt tables per structure; with
    the formatter on as well no [L, L] float tensor is copied to the host at all.  data.rsa_text_device (default on): the RSA
    head's K + 1 tables are computed and formatted on the device behind the head (rnamsm.rsa.table_text), so the writer thread no
    longer runs K + 1 np.savetxt tables per alignment.  Under gather_to_rank0 all three stay off (the host path): the gathered items
    are the heads' values and the tokens."""
    base_lut = ss.token_base_codes(alphabet, device) if sw.ss_path or sw.rsa_dir else None
    heads: list = []
    if sw.ss_path:
        if rank == 0:
            print(f"SS head arithmetic: {sw.ss_dtype} (data.ss_gemm_dtype; independent of model.gemm_dtype={sw.gemm_dtype})")
        predictor = ss.load_predictor(sw.ss_path, device)
        predictor.gemm_dtype = sw.ss_dtype
        heads.append(ss.SSHead(predictor, alphabet, base_lut, device, text_on=sw.ss_text, pairs_on=sw.ss_pairs, nested=sw.ss_nested))
    if sw.rsa_dir:      # (the reference program's seed; every alignment's draws are taken as its writer job is made, in delivery order)
        heads.append(rsa.RSAHead(rsa.load_ensemble(sw.rsa_dir, device), alphabet, base_lut, random.Random(2022),
                                 text_on=sw.rsa_text, device=device))
    if sw.contacts:     # the trunk's own contact_head.regression.*: no further file to load
        reg = model.contact_head.regression
        heads.append(contacts.ContactHead(reg.weight, reg.bias))
    if sw.lm_mode:      # the trunk's own lm_head.*: "wt" reads every alignment's emb where it lies, "masked" runs L further forwards
        heads.append(lm.LMHead(model, sw.lm_mode))
    return heads


def _route(h, L: int, sw: _Switches, max_seqlen: int):
    """The method that runs head h on an alignment of L body columns, or the reason (a str) it is skipped.  Only an alignment stitched
    from windows (data.long_msa=windows, wider than the model) asks the head (stitched_route): the others stop at L <= 1024, or
    would need per-window semantics."""
    return h.stitched_route(L, sw.long_heads) if sw.windowing and L > max_seqlen - 1 else h.one


def _head_tokens(h, toks: torch.Tensor) -> torch.Tensor:
    """What a head is handed of an alignment's tokens [R, C]: the query behind <cls>; the whole matrix where the head asks
    for it (rnamsm.lm.LMHead: the masked scan runs further forwards on it)."""
    return toks if getattr(h, "whole_tokens", False) else toks[0, 1:]


def _record_event() -> torch.cuda.Event:
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream())
    return ev


class _Reader:
    """Reader + row sub-sampling + crop of one alignment.  All randomness of the CLI lives here, drawn from ONE stream
    in the reference's order -- per item `sample-pretrained`'s weighted draw (dataset.py:88-90), then the crop
    (dataset.py:147) -- seeded 42 like the reference's global numpy state (RNA_MSM_Inference.py:17), so a single
    process reproduces the reference's choices; under sharding every rank draws for its own items."""

    def __init__(self, cfg: Config, sw: _Switches, ids: List[str], files: Dict[str, Path], alphabet, device, put_map, put_stats=None, put_mi=None):
        self.cfg, self.sw, self.ids, self.files, self.alphabet, self.device, self.put_map = cfg, sw, ids, files, alphabet, device, put_map
        self.put_stats, self.put_mi = put_stats, put_mi
        self.rng = np.random.RandomState(42)

    def __call__(self, idx: int) -> np.ndarray:
        torch.cuda.set_device(self.device)
        rna_id = self.ids[idx]
        tokens = load_msa_tokens(self.files[rna_id], self.alphabet, self.cfg.data.max_seqs_per_msa, self.cfg.data.sample_method,
                                 device=self.device, rng=self.rng, filter_seqid=self.sw.filter_seqid,
                                 on_full=(lambda full: self.on_full(rna_id, full)) if self.sw.invcov_on or self.sw.msa_stats_on or self.sw.mi_on else None)
        return tokens if self.sw.windowing else crop_tokens(tokens, self.cfg.data.max_seqlen, self.rng)

    def on_full(self, rna_id: str, full: np.ndarray) -> None:
        if self.sw.invcov_on:
            self.covariance_map(rna_id, full)
        weights = self.alignment_stats(rna_id, full) if self.sw.msa_stats_on else None
        if self.sw.mi_on:
            self.mutual_information(rna_id, full, weights)

    def alignment_stats(self, rna_id: str, full: np.ndarray):
        """data.msa_stats: the weights and the coverage of the alignment as read, left on the device for the sink, and the line with
        Neff; an alignment the kernels refuse gets one line that names the reason, and its other files as usual.  Returns the
        weights on the device (data.mi_weights=seqid counts with them), None for a refused alignment."""
        N, L = full.shape[0], max(full.shape[1] - 1, 1)
        try:
            rec, coverage = msa_stats_device(full, self.alphabet.tok_to_idx["-"], self.sw.seqid_cutoff, self.device)
            neff = float(rec.neff.item())                   # (waits for the reader's stream: the vectors are complete)
        except _lib.RnamsmError as e:
            print(f"{rna_id}: no alignment statistics (data.msa_stats) for this alignment of {N} rows x {L} columns: {e}")
            return None
        self.put_stats(rna_id, (rec.weights, coverage))
        print(f"{rna_id}: {N} rows x {L} columns, Neff {neff:.3f} (Neff/sqrt(L) {neff / math.sqrt(L):.3f}, Neff/L {neff / L:.4f})")
        return rec.weights

    def mutual_information(self, rna_id: str, full: np.ndarray, weights=None) -> None:
        """data.mi: the two maps of the alignment as read (before row sub-sampling and any crop), left on the device for the sink; an
        alignment the kernel refuses gets one line that names the reason, and its other files as usual.  data.mi_weights=seqid: the
        sequence-weighted pair, with `weights` (data.msa_stats' own, where that key made them) or the weights at the same cutoff."""
        try:
            if self.sw.mi_weighted:
                rec = msa_mi_weighted_device(full, self.alphabet.tok_to_idx["-"], self.device, self.sw.mi_gaps, weights, self.sw.seqid_cutoff)
            else:
                rec = msa_mi_device(full, self.alphabet.tok_to_idx["-"], self.device, self.sw.mi_gaps)
            self.put_mi(rna_id, (rec.mi, rec.mip))
            torch.cuda.current_stream().synchronize()       # (the reader's stream: the maps are complete whichever stream copies them)
        except _lib.RnamsmError as e:
            print(f"{rna_id}: no mutual-information maps (data.mi) for this alignment of {full.shape[0]} rows x {full.shape[1] - 1} "
                  f"columns: {e}")

    def covariance_map(self, rna_id: str, full: np.ndarray) -> None:
        """data.invcov: the map of the alignment as read (before row sub-sampling and any crop), left on the device for the sink; an
        alignment the kernel refuses gets one line that names the reason, and its other files as usual."""
        try:
            self.put_map(rna_id, msa_invcov_device(full, self.alphabet.tok_to_idx["-"], self.device))
            torch.cuda.current_stream().synchronize()       # (the reader's stream: the map is complete whichever stream copies it)
        except _lib.RnamsmError as e:
            print(f"{rna_id}: no covariance map (data.invcov) for this alignment of {full.shape[0]} rows x {full.shape[1] - 1} "
                  f"columns: {e}")


def _gather_group(device, rank: int):
    """Transport: RCCL point-to-point where it comes up; otherwise the ranks agree (over the default gloo group) to stage the same
    gather through host memory -- the outputs arrive on rank 0 either way (sharding.negotiate_gather_transport).  A default group
    that is not gloo (a caller's own nccl world) is used as it is, as before."""
    import torch.distributed as dist
    if dist.get_backend() != "gloo":
        return None
    group, label, _ = sharding.negotiate_gather_transport(device, want_backend=os.environ.get("RNAMSM_GATHER_BACKEND", "nccl"))
    if group is False:
        raise RuntimeError(f"gather_to_rank0: no transport to rank 0 ({label}); run without RNAMSM_GATHER_TO_RANK0 "
                           f"(every rank then writes its own files)")
    if label != "primary" and rank == 0:
        print(f"gather to rank 0: {label}")
    return group


class _Sink:
    """The delivery side of the CLI loop: an alignment's outputs and its heads' records become files -- through the
    _AsyncNpyWriter, or on the spot (async_io=False) -- on this rank or, under gather_to_rank0, on rank 0."""

    def __init__(self, ids: List[str], heads: list, save_dir: Path, sw: _Switches, max_seqlen: int, device, rank: int, async_io: bool):
        self.ids, self.heads, self.save_dir, self.sw, self.max_seqlen = ids, heads, save_dir, sw, max_seqlen
        self.written: List[str] = []
        self.invcov_maps: Dict[str, torch.Tensor] = {}      # id -> the map on the device, from the reader until the alignment is delivered
        self.msa_stats: Dict[str, tuple] = {}               # id -> (weights, coverage) on the device, likewise (data.msa_stats)
        self.mi_maps: Dict[str, tuple] = {}                 # id -> (mi, mip) on the device, likewise (data.mi)
        self.device = device
        self.metric_entries: Dict[str, dict] = {}           # id -> what <id>_metrics.json holds (data.target_dir), for the summary
        self.sweep_table = None                             # the sweep's 1001 thresholds on the device, checked and uploaded once
        self.writer = _AsyncNpyWriter(device) if async_io and (not sw.gathering or rank == 0) else None
        # gather_to_rank0: outputs travel to rank 0 one ROUND (one MSA per rank) at a time, round k's RCCL transfers
        # overlapping round k+1's forward, and are handed to the writer as they arrive -- at most one round is resident
        # (an item: emb, atp, every head's flattened record, the covariance map)
        self.gatherer = sharding.RoundGatherer(len(ids), on_item=self.on_item,
                                               tensors_per_item=2 + sum(h.n_tensors for h in heads) + int(sw.invcov_on) + 2 * int(sw.msa_stats_on) + 2 * int(sw.mi_on),
                                               dst=0, device=device, group=_gather_group(device, rank)) if sw.gathering else None

    def put_map(self, rna_id: str, cov: torch.Tensor) -> None:
        self.invcov_maps[rna_id] = cov

    def put_stats(self, rna_id: str, vectors: tuple) -> None:
        self.msa_stats[rna_id] = vectors

    def put_mi(self, rna_id: str, maps: tuple) -> None:
        self.mi_maps[rna_id] = maps

    def top_jobs(self, rna_id: str, maps: list) -> list:
        """data.top_pairs: maps = [(name, the [L, L] map on the device)] -> one writer job per map: the top-k ranked pairs, selected
        and ranked on the device from the map where it lies (ops.top_pairs; k from the spec and THIS map's L), written as
        <id>_<name>_top.txt.  A map with L < 2 or a k beyond the library's limit gets one printed line and no list."""
        jobs = []
        for name, t in maps:
            L = int(t.shape[-1])
            k = contacts.top_pairs_k(self.sw.top_pairs, L)
            if L < 2 or k > _lib.TOP_PAIRS_MAX_K:
                why = f"L={L} is below 2" if L < 2 else f"k={k} exceeds {_lib.TOP_PAIRS_MAX_K}"
                print(f"{rna_id}: no ranked pair list (data.top_pairs={self.sw.top_pairs}) for its {name} map: {why}")
                continue
            rec = ops.top_pairs(t if t.stride(-1) == 1 else t.contiguous(), k, self.sw.top_pairs_min_sep)
            path = os.path.join(self.save_dir, f"{rna_id}_{name}_top.txt")

            def write(pairs, scores, count, path=path) -> None:
                n = int(count)
                with open(path, "w") as f:
                    f.write(contacts.format_top_pairs(pairs[:n], scores[:n], self.sw.top_pairs_min_sep))

            jobs.append((write, (rec.pairs, rec.scores, rec.count)))
        return jobs

    def metrics_job(self, rna_id: str, records, maps: list) -> list:
        """data.target_dir: the accuracy of this alignment's maps against <target_dir>/<id>.bpseq | .ct | .npy, counted on the device
        from the maps where they lie (ops.pair_sweep for the SS probabilities, ops.pair_precision with k = L for every map of
        `maps` = [(name, [L, L] map)]) -> one writer job, <id>_metrics.json, or none.  A missing target, a target of another length
        or L < 10 prints one line that names the reason; that map (or the whole alignment) gets no entry."""
        path = metrics.find_target(self.sw.target_dir, rna_id)
        if path is None:
            print(f"{rna_id}: no metrics (data.target_dir={self.sw.target_dir}): no {rna_id}.bpseq, .ct or .npy there")
            return []
        min_sep, targets = self.sw.target_min_sep, {}

        def target_for(L: int, what: str):
            """(the target on the device, the partner vector on the host) at this length, or None behind one printed line"""
            if L not in targets:
                try:
                    if L < 10:
                        raise ValueError(f"L={L} is below 10")
                    if L > _lib.TOP_PAIRS_MAX_L:
                        raise ValueError(f"L={L} exceeds {_lib.TOP_PAIRS_MAX_L}")
                    t, partner = metrics.read_target(path, L)
                    targets[L] = (torch.from_numpy(t).to(self.device), partner)
                except (ValueError, OSError) as e:
                    targets[L] = str(e)
            if isinstance(targets[L], str):
                print(f"{rna_id}: no metrics (data.target_dir) for its {what}: {targets[L]}")
                return None
            return targets[L]

        tensors, layout, partner_true = [], [], None        # layout: (kind, name, L, how many tensors, host extras)
        for h, r in zip(self.heads, records):
            if r is None or not isinstance(h, ss.SSHead) or r.probs is None:
                continue
            L = int(r.probs.shape[-1])
            got = target_for(L, "SS probability map")
            if got is None:
                continue
            if self.sweep_table is None:
                self.sweep_table = ops.sweep_table(metrics.sweep_thresholds(), self.device)
            probs = r.probs if r.probs.stride(-1) == 1 else r.probs.contiguous()
            tensors.append(ops.pair_sweep(probs, got[0], self.sweep_table, min_sep))
            layout.append(("sweep", "ss", L, 1, None))
            if r.structure is not None:
                tensors.append(r.structure[0])
                layout.append(("structure", "ss", L, 1, got[1]))
            if r.nested is not None:                        # data.ss_nested: the nested structure against the same target
                tensors.append(r.nested[0])
                layout.append(("nested", "ss_nested", L, 1, got[1]))
        for name, t in maps:
            L = int(t.shape[-1])
            got = target_for(L, f"{name} map")
            if got is None:
                continue
            cuts = metrics.precision_cuts(L)
            rec = ops.pair_precision(t if t.stride(-1) == 1 else t.contiguous(), got[0], L, cuts, min_sep)
            tensors += [rec.hits, rec.count]
            layout.append(("precision", name, L, 2, cuts))
        if not layout:
            return []
        out = os.path.join(self.save_dir, f"{rna_id}_metrics.json")

        def write(*host) -> None:
            host, entry = list(host), {"id": rna_id, "target": os.path.basename(path), "min_sep": min_sep}
            for kind, name, L, n, extra in layout:
                got, host = host[:n], host[n:]
                if kind == "sweep":
                    entry.setdefault("ss", {"L": L})["sweep"] = metrics.sweep_entry(got[0])
                elif kind == "structure":
                    entry.setdefault("ss", {"L": L})["structure"] = metrics.structure_scores(got[0], extra)
                elif kind == "nested":
                    entry["ss_nested"] = {"L": L, **metrics.structure_scores(got[0], extra)}
                else:
                    entry.setdefault("precision", {})[name] = metrics.precision_entry(got[0], int(got[1]), extra, L)
            with open(out, "w") as f:
                json.dump(entry, f, indent=1)
                f.write("\n")
            self.metric_entries[rna_id] = entry

        return [(write, tuple(tensors))]

    def write_metrics_summary(self, rank: int, world: int) -> None:
        """data.target_dir, at the end of the list: metrics_summary.json (per rank where several ranks write) -- the summed sweep counts,
        sweep_scores of the sum, and the mean of each precision over the alignments that had one, in list order."""
        if not self.sw.target_dir:
            return
        position = {rna_id: n for n, rna_id in enumerate(self.ids)}
        entries = [self.metric_entries[i] for i in sorted(self.metric_entries, key=position.__getitem__)]
        name = "metrics_summary.json" if world == 1 else f"metrics_summary_rank{rank}.json"
        with open(os.path.join(self.save_dir, name), "w") as f:
            json.dump(metrics.summary(entries), f, indent=1)
            f.write("\n")

    def deliver(self, idx: int, emb: torch.Tensor, atp: torch.Tensor, after: Optional[torch.cuda.Event], records: list) -> None:
        """records: the alignment's record of every head, None for a head skipped on it."""
        if self.gatherer is None:
            self.emit(self.ids[idx], emb, atp, after, records)
            return
        # (a skipped head's share of the item: n_tensors one-element placeholders, dropped again by records_of on rank 0)
        item = (emb, atp) + tuple(t for h, r in zip(self.heads, records) for t in (
            h.flatten(r) if r is not None else [emb.new_zeros(1) for _ in range(h.n_tensors)]))
        if self.sw.invcov_on:           # (the map travels as the item's last tensor; a refused alignment sends a placeholder)
            cov = self.invcov_maps.pop(self.ids[idx], None)
            item += (cov if cov is not None else emb.new_zeros(1),)
        if self.sw.msa_stats_on:        # (the two vectors travel as the item's last tensors, float64; a refused alignment sends fp32 placeholders)
            item += tuple(self.msa_stats.pop(self.ids[idx], None) or (emb.new_zeros(1, dtype=torch.float32),) * 2)
        if self.sw.mi_on:               # (the two maps travel as the item's last tensors; a refused alignment sends placeholders)
            item += tuple(self.mi_maps.pop(self.ids[idx], None) or (emb.new_zeros(1),) * 2)
        self.gatherer.submit(idx, item)

    def on_item(self, i: int, ts) -> None:
        n_mi = 2 * int(self.sw.mi_on)
        mi, ts = (tuple(ts[len(ts) - n_mi:]), ts[:len(ts) - n_mi]) if n_mi else (None, ts)
        n_stats = 2 * int(self.sw.msa_stats_on)
        self.emit(self.ids[i], ts[0], ts[1], records=self.records_of(ts[2:], ts[0].shape[0]),
                  cov=ts[len(ts) - n_stats - 1] if self.sw.invcov_on else None, stats=tuple(ts[len(ts) - n_stats:]) if n_stats else None,
                  mi=mi)

    def records_of(self, flat, L: int) -> list:
        """A gathered item's tensors behind emb and atp -> the heads' records (the inverse of deliver()'s flattening)."""
        flat = iter(flat)
        shares = [(h, [next(flat) for _ in range(h.n_tensors)]) for h in self.heads]
        return [None if isinstance(_route(h, L, self.sw, self.max_seqlen), str) else h.unflatten(ts) for h, ts in shares]

    def emit(self, rna_id: str, emb: torch.Tensor, atp: torch.Tensor, after: Optional[torch.cuda.Event] = None, records=(),
             cov: Optional[torch.Tensor] = None, stats: Optional[tuple] = None, mi: Optional[tuple] = None) -> None:
        """records: this alignment's record of every head that is on, in the order of `heads`; each becomes one writer job (but
        for the heads skipped on a stitched alignment: their entry is None).  cov: a gathered item's covariance map (or
        its one-element placeholder); absent, the one the reader left for this id, if any."""
        extra = [h.writer_job(r, rna_id, self.save_dir) for h, r in zip(self.heads, records) if r is not None]
        cov = self.invcov_maps.pop(rna_id, None) if cov is None else (cov if cov.dim() == 2 else None)
        cov_job = [(self.save_dir / f"{rna_id}_invcov.npy", cov)] if cov is not None else []
        # stats: a gathered item's (weights, coverage) or its placeholders; absent, what the reader left for this id, if anything
        stats = self.msa_stats.pop(rna_id, None) if stats is None else (stats if stats[0].dtype == torch.float64 else None)
        if stats is not None:
            cov_job += [(self.save_dir / f"{rna_id}_weights.npy", stats[0]), (self.save_dir / f"{rna_id}_coverage.npy", stats[1])]
        # mi: a gathered item's (mi, mip) or its placeholders; absent, what the reader left for this id, if anything
        mi = self.mi_maps.pop(rna_id, None) if mi is None else (mi if mi[0].dim() == 2 else None)
        if mi is not None:
            names = ("wmi", "wmip") if self.sw.mi_weighted else ("mi", "mip")
            cov_job += [(self.save_dir / f"{rna_id}_{names[0]}.npy", mi[0]), (self.save_dir / f"{rna_id}_{names[1]}.npy", mi[1])]
        if self.sw.top_pairs or self.sw.target_dir:         # every pair map of this alignment, while it is still on the device
            maps = [("contacts", r.contacts) for h, r in zip(self.heads, records) if r is not None and isinstance(h, contacts.ContactHead)]
            maps += [(Path(path).name[len(rna_id) + 1:-len(".npy")], t) for path, t in cov_job if t.dim() == 2]
            made = self.top_jobs(rna_id, maps) if self.sw.top_pairs else []           # the ranked lists
            if self.sw.target_dir:                          # the accuracy against the known structure
                made += self.metrics_job(rna_id, records, maps)
            extra += made
            if made and after is not None:                  # the copies wait for these kernels too
                after = _record_event()
        if self.writer is not None:
            self.writer.submit([(self.save_dir / f"{rna_id}_atp.npy", atp), (self.save_dir / f"{rna_id}_emb.npy", emb)] + extra + cov_job,
                               lambda r=rna_id: self.written.append(r), after=after)
            return
        for fn, tensors in extra:
            fn(*(t.cpu().numpy() for t in tensors))
        for path, t in cov_job:
            np.save(path, t.cpu().numpy())
        emb_host, atp_host = emb.cpu().numpy(), atp.cpu().numpy()
        np.save(self.save_dir / f"{rna_id}_atp.npy", atp_host)
        np.save(self.save_dir / f"{rna_id}_emb.npy", emb_host)
        self.written.append(rna_id)

    def finish(self) -> None:
        if self.gatherer is not None:
            self.gatherer.finish()

    def close(self) -> None:
        if self.writer is not None:
            self.writer.close()

    def written_in_list_order(self) -> List[str]:
        position = {rna_id: n for n, rna_id in enumerate(self.ids)}
        return sorted(self.written, key=position.__getitem__)              # whatever order the groups ran in


class _Scheduler:
    """The compute side of the CLI loop: which alignments share a launch set, in which order the forwards are enqueued and read back,
    and the heads behind them.  It reaches the device through the model's entry points, the heads' one / one_long / many and the two
    callables it is given -- to_device(host tokens) and record_event() on the current stream -- and nothing else."""

    def __init__(self, model, heads: list, sink, sw: _Switches, ids: List[str], mine: List[int], read, reader, padding_idx: int,
                 to_device, record_event):
        self.model, self.heads, self.sink, self.sw, self.ids, self.mine = model, heads, sink, sw, ids, mine
        self.read, self.reader, self.padding_idx, self.to_device, self.record_event = read, reader, padding_idx, to_device, record_event
        self.group: List = []           # (idx, tokens on the device)
        self.pool: List = []            # (idx, tokens on the host)
        self.inflight = None            # the pipelined forward whose results are still on the device: (the method that finishes it, its arguments...)
        self.pending = None             # the reader's future: the next alignment of the list

    def run(self) -> None:
        self.pending = self.reader.submit(self.read, self.mine[0]) if self.reader and len(self.mine) else None
        try:
            self.read_and_run()
        except Exception:
            # a bad alignment late in the list must not cost the results already computed or read: what waits in the
            # group / pool is run and written (as the one-by-one loop would have done before reaching it), then the
            # error goes up.  KeyboardInterrupt / SystemExit are not caught: they propagate at once.  Under a gatherer the
            # peers are not known to be in the same state (a deliver() could block on them): no salvage there.  A second
            # failure in here is reported and dropped in favour of the first.
            if not self.sw.gathering:
                try:
                    self.drain()
                except Exception as second:                       # noqa: BLE001
                    import warnings
                    warnings.warn(f"while writing the results computed before the error: {type(second).__name__}: {second}")
            raise
        self.drain()
        self.sink.finish()

    def drain(self) -> None:
        self.flush()
        self.run_pool()
        self.settle()

    def read_and_run(self) -> None:
        for n, idx in enumerate(self.mine):
            tokens = self.pending.result() if self.reader else self.read(idx)
            if self.reader and n + 1 < len(self.mine):
                self.pending = self.reader.submit(self.read, self.mine[n + 1])       # parsed while the GPU runs this MSA
            self.step(idx, tokens)

    def step(self, idx: int, tokens: np.ndarray) -> None:
        """One alignment of the list: into the pool or the group where it is small, else by itself."""
        sw, model = self.sw, self.model
        wide = sw.windowing and tokens.shape[1] > model.max_seqlen
        if (sw.batching and not wide and tokens.size <= sw.small_limit and 2 * tokens.shape[1] ** 2 <= FRAME_MAP_ELEMS
                and not (tokens == self.padding_idx).any()):
            if sw.pooled:
                self.pool.append((idx, tokens))
                # (packing: a full group's worth of tokens starts NOW -- the reader goes on under its forward -- instead of
                # waiting for POOL_MSAS alignments or the end of the list)
                if len(self.pool) >= POOL_MSAS or (sw.packing and sum(t.size for _, t in self.pool) >= PACKED_TOKENS):
                    self.run_pool()
                return
            if not (joins_packed if sw.packing else joins_group)([tuple(t.shape) for _, t in self.group], tuple(tokens.shape)):
                self.flush()                                  # the group is full (framed: this one would pad too much)
            self.group.append((idx, self.to_device(tokens)))
            return
        self.flush()
        if wide:
            self.run_wide(idx, tokens)
            return
        has_pad = bool((tokens == self.padding_idx).any())          # on the host: no device round trip before the launches
        t_dev = self.to_device(tokens)
        if sw.gathering:            # (the gather orders its transfers behind the compute stream: one by one there, as before)
            self.settle()
            out = model.checked_forward_one(t_dev, has_pad, need_repr=False, what=self.ids[idx])   # emb + atp are all that is written
            self.deliver(idx, out["emb"], out["atp"], toks=t_dev)
            return
        # PIPELINED (round 6): this forward is enqueued BEFORE the previous one's error word and outputs are read -- the ~3 ms
        # of host work per alignment (weight-table check, ~140 launches, delivery) no longer idle the GPU between forwards
        out = model.forward_one(t_dev, has_pad, need_repr=False)
        ev = self.record_event()
        self.settle()                   # the previous forward is finished first; only then is this one the one in flight
        self.inflight = (self.finish_one, idx, t_dev, has_pad, out, ev)

    def run_wide(self, idx: int, tokens: np.ndarray) -> None:
        """data.long_msa=windows: the lone route, never a group; behind whatever is in flight (its workspace is the model's)."""
        self.settle()
        rna_id, L = self.ids[idx], tokens.shape[1] - 1
        t_dev = self.to_device(tokens)
        out = self.model.forward_windows(t_dev, self.sw.window_stride, what=rna_id)
        for h in self.heads:
            why = _route(h, L, self.sw, self.model.max_seqlen)
            if isinstance(why, str):
                print(f"{rna_id}: L={L} is stitched from windows (data.long_msa=windows); "
                      f"{type(h).__name__}{getattr(h, 'skip_suffix', '')} is skipped for it" + (f" ({why})" if why else ""))
        self.deliver(idx, out["emb"], out["atp"], toks=t_dev)

    def deliver(self, idx: int, emb: torch.Tensor, atp: torch.Tensor, after: Optional[torch.cuda.Event] = None,
                toks: Optional[torch.Tensor] = None, records: Optional[list] = None) -> None:
        """records: this alignment's record of every head, where its group's batched heads (deliver_group) have made them;
        absent, the lone heads run here, on emb and atp where they lie (a packed group's slices included)."""
        if records is None:
            # (a stitched alignment: the heads data.long_heads=stitched lets through run their long route; lm_scores=wt has
            # no length limit and no long route, and keeps its own; a head that names a reason instead is skipped)
            routes = [_route(h, emb.shape[0], self.sw, self.model.max_seqlen) for h in self.heads]
            records = [None if isinstance(run, str) else run(emb, atp, _head_tokens(h, toks)) for h, run in zip(self.heads, routes)]
            if self.heads and after is not None:            # the copies wait for the heads too
                after = self.record_event()
        self.sink.deliver(idx, emb, atp, after, records)

    def deliver_group(self, members_, outs, ev: Optional[torch.cuda.Event] = None) -> None:
        """Every head once over the whole group (one launch set per stage; each member's record is the lone head's bits), then
        the members one by one."""
        embs, atps = [o["emb"].contiguous() for o in outs], [o["atp"].contiguous() for o in outs]
        per_head = [h.many(embs, atps, [_head_tokens(h, t) for _, t in members_]) for h in self.heads]
        if self.heads and ev is not None:                   # the copies wait for the batched heads too
            ev = self.record_event()
        for n, ((i, t), emb, atp) in enumerate(zip(members_, embs, atps)):
            self.deliver(i, emb, atp, ev, t, records=[recs[n] for recs in per_head])

    def finish_packed(self, members_, begun, ev) -> None:
        """Second half of a pipelined packed group: its error word and outputs, read behind the event recorded after its launches."""
        res, mode = begun
        toks_ = [t for _, t in members_]
        try:
            outs = self.model.forward_ragged_finish(toks_, res, mode, after=ev)
            if outs is not res:
                ev = None                                 # a rerun: its outputs are behind everything enqueued so far
            if outs is None:                              # <pad> inside the batch: the framed rerun of forward_ragged
                outs = self.model.forward_ragged(toks_, packed=False)
        except IndexError:                                # name the offending alignment: one by one
            outs, ev = [self.alone(i, t) for i, t in members_], None
        if not all(o["emb"].is_contiguous() and o["atp"].is_contiguous() for o in outs):
            ev = None                                     # .contiguous() below would launch copies on the compute stream
        self.deliver_group(members_, outs, ev)

    def finish_one(self, idx: int, t_dev, has_pad: bool, out, ev) -> None:
        """Second half of a pipelined lone forward (the one-by-one loop of alignments too large to wait for company)."""
        done = self.model.finish_forward_one(t_dev, out, has_pad, need_repr=False, what=self.ids[idx], after=ev)
        self.deliver(idx, done["emb"], done["atp"], ev if done is out else None, t_dev)

    def settle(self) -> None:
        """Read back and deliver what is still in flight, if anything: a packed group or a lone forward."""
        if self.inflight is not None:
            entry, self.inflight = self.inflight, None
            self.finish(entry)

    @staticmethod
    def finish(entry) -> None:
        entry[0](*entry[1:])

    def run_pool(self) -> None:
        sw, pool = self.sw, self.pool
        shapes_ = [tuple(t.shape) for _, t in pool]
        fold_min = ops.get_param("ln_fold_min_tokens") if (sw.exact and self.model.fold_layernorm and ops.get_param("ln_fold") == 1) else 0
        if not sw.packing:
            for members in plan_groups(shapes_):
                self.group.extend((pool[j][0], self.to_device(pool[j][1])) for j in members)
                self.flush()
            pool.clear()
            return
        # Token-packed groups, PIPELINED (round 6): group g+1 is enqueued before group g's error word is read, so g's
        # device-to-host copies and file writes run under g+1's forward instead of after it with the GPU idle (64 small
        # alignments used to be one blocking 117 ms forward followed by 26 ms of deliveries).  A pool that would be ONE group
        # of at least PIPELINE_SPLIT_TOKENS tokens is dealt into two for that.  Same launch sets per group as before: every
        # member's files are byte for byte those of its own forward (exact mode).
        # (one stream carries every forward: what belongs to group g -- its error word, its outputs -- is read behind an EVENT
        # recorded right after g's launches, on side streams, or it would wait for g+1's forward as well)
        # The last group of a pool STAYS in flight when run_pool returns (self.inflight): the reader goes on, the next pool's first group
        # is enqueued behind it, and only then is it read back; settle() ends the pipeline (before a forward outside the pool, at the
        # end of the list).
        waiting, self.inflight = self.inflight, None        # the group in flight (or a lone forward, from before the pool)
        try:
            for members in plan_packed_groups(shapes_, fold_min, split_tokens=PIPELINE_SPLIT_TOKENS):
                members_ = [(pool[j][0], self.to_device(pool[j][1])) for j in members]
                if len(members_) == 1:
                    if waiting is not None:
                        self.finish(waiting)
                        waiting = None
                    self.group.extend(members_)
                    self.flush()
                    continue
                begun = self.model.forward_ragged_begin([t for _, t in members_])
                ev = self.record_event()
                if waiting is not None:
                    self.finish(waiting)
                waiting = (self.finish_packed, members_, begun, ev)
        finally:
            self.inflight = waiting                         # also when a group raised: what is in flight is still delivered (salvage)
        pool.clear()

    def alone(self, i: int, t: torch.Tensor) -> dict:
        """One member of a group by itself, in the arithmetic the GROUP runs in (what a small alignment's
        files hold must not depend on whether it had company).  Exact mode: its own forward IS the packed batch's
        arithmetic, bit for bit.  16-bit modes: a packed batch's attention runs on the exact kernels, a lone forward's on
        the 16-bit ones -- so there a lone small alignment is a packed batch of one."""
        if self.sw.packing and not self.sw.exact:
            try:
                return self.model.forward_ragged([t], packed=True)[0]
            except IndexError:
                raise IndexError(f"{self.ids[i]}: token or position index out of range") from None
        return self.model.checked_forward_one(t, need_repr=False, what=self.ids[i])

    def flush(self) -> None:
        group = self.group
        if len(group) == 1:
            idx0, t0 = group[0]
            self.deliver_group(group, [self.alone(idx0, t0)])
        elif group:
            try:
                outs = self.model.forward_ragged([t for _, t in group], packed=self.sw.packing)
            except IndexError:                                # name the offending alignment: one by one
                outs = [self.alone(i, t) for i, t in group]
            self.deliver_group(group, outs)
        group.clear()


def extract_feat(cfg: Config, model: Optional[MSATransformer] = None, gather_to_rank0: bool = False,
                 async_io: bool = True) -> List[str]:
    """async_io: read/tokenise the next alignment on a helper thread while the GPU runs the current one, and move the
    outputs to disk through `_AsyncNpyWriter`; False = the reference's strictly sequential loop (same files)."""
    import torch.distributed as dist
    rank = dist.get_rank() if dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_initialized() else 1
    refuse_top_pairs_under_gather(getattr(cfg.data, "top_pairs", ""), gather_to_rank0)
    refuse_target_dir_under_gather(getattr(cfg.data, "target_dir", ""), gather_to_rank0)
    sw = read_switches(cfg, gather_to_rank0 and world > 1)
    device = torch.device(cfg.data.device)
    if device.type != "cuda":
        raise RuntimeError("this build runs on the MI355X HIP path only (data.device=cuda); there is no CPU path")
    if device.index is None:          # "cuda": this rank's GPU under a launcher, else the process's current device
        device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", rank)) if world > 1 else torch.cuda.current_device())
    alphabet = RNAAlphabet.from_architecture(cfg.data.architecture)
    if rank == 0:
        print(f"Maximum Number of MSA Seqs:{cfg.data.max_seqs_per_msa}")
        print(f"Inference on: {device}")

    root = Path(cfg.data.root_path)
    with open(root / cfg.data.MSA_list) as f:
        ids = sorted(f.read().splitlines())
    ids = [i for i in ids if i]
    files = find_msa_files(root / cfg.data.MSA_path, ids)
    model = _load_model(cfg, model, alphabet, device)
    save_dir = root / cfg.data.MSA_path
    save_dir.mkdir(parents=True, exist_ok=True)
    heads = _load_heads(sw, model, alphabet, device, rank)
    # the library launches on the calling thread's current device: make it this rank's GPU on the main thread and on
    # the reader thread (whose greedy sub-sampling runs on the device)
    torch.cuda.set_device(device)

    sink = _Sink(ids, heads, save_dir, sw, model.max_seqlen, device, rank, async_io)
    reader = ThreadPoolExecutor(1, thread_name_prefix="rnamsm-msa-reader") if async_io else None
    scheduler = _Scheduler(model, heads, sink, sw, ids, sharding.shard_indices(len(ids), rank, world),
                           _Reader(cfg, sw, ids, files, alphabet, device, sink.put_map, sink.put_stats, sink.put_mi), reader, alphabet.padding_idx,
                           to_device=lambda tokens: torch.from_numpy(tokens).to(device), record_event=_record_event)
    try:
        with torch.no_grad():
            scheduler.run()
    finally:
        if reader is not None:
            reader.shutdown(wait=True)
        sink.close()
    sink.write_metrics_summary(rank, world)
    if rank == 0:
        print(f"Done! Generated files are saved at {save_dir}")
    return sink.written_in_list_order()


