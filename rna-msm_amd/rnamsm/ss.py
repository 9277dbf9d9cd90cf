"""RNA-MSM-SS: secondary structure from the attention maps (the reference's _downstream_tasks/SS).

`SSPredictor` carries the parameters of the reference's `renet_b16()` under the same names and shapes, so its
`rna-msm_attention.pt` state_dict loads with strict=True; its arithmetic is one HIP entry point (rnamsm_ss_head, exact fp32
on the matrix cores) that reads the [120, L, L] maps where they lie on the device.  `write_ss_files` is the reference's
post-processing (code/post_processing/processing_output.py: prob_to_secondary_structure without the VARNA plots): the
same `.ct`, `.bpseq` and `.prob` files, byte for byte.  `prob_text` / `prob_text_many` format the `.prob` text on the device
(rnamsm_ss_prob_text), so that the writer's share of it is one binary write; `structure` / `structure_many` decode the base pairs
and write the bodies of `.ct` / `.bpseq` there too (rnamsm_ss_pairs), so that the probabilities need not leave the device at all.
`SSHead` is the head as the CLI runs it: it makes one `SSResult` per alignment and turns it into the job that writes the three files.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import nn

from . import _lib, ops

NUM_MAPS = 120                  # layers x heads of the MSA transformer
IN_PLANES = 8 + NUM_MAPS        # outer one-hot of the sequence + the maps
CHANNELS = 48
THRESHOLD = 0.516               # pairing threshold of the reference's post-processing
_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _ch in enumerate("ACGU"):     # sklearn OneHotEncoder fitted on A, C, G, U (categories sorted), handle_unknown='ignore'
    _CODE[ord(_ch)] = _i


def base_codes(seq: str) -> np.ndarray:
    """uint8 [L]: 0..3 for A, C, G, U; 255 (the all-zero one-hot vector) for anything else, lowercase and T included."""
    raw = np.frombuffer(seq.encode("latin-1", errors="replace"), dtype=np.uint8)
    return _CODE[raw]


# pixels of one packed call: the workspace of one lone L = 1024 call (403 MB).  The bf16 head keeps both workspace images in fp32
# (rnamsm_ss_head16_packed_workspace_bytes = rnamsm_ss_head_packed_workspace_bytes), so one budget serves both arithmetics.
SS_CHUNK_PIXELS = 1024 * 1024


def plan_ss_chunks(Ls: Sequence[int], max_pixels: int = SS_CHUNK_PIXELS, max_batch: int = _lib.SS_MAX_BATCH) -> List[List[int]]:
    """Indices of `Ls` split into consecutive calls of rnamsm_ss_head_packed, in list order: a chunk takes the next structure
    as long as its sum of L^2 stays within max_pixels and its length within max_batch (greedy, so no two neighbouring chunks
    could have been one).  A structure larger than the budget by itself -- impossible at the default, L <= 1024 -- is a chunk of
    its own."""
    return plan_chunks([int(L) * int(L) for L in Ls], max_pixels, max_batch)


def plan_chunks(weights: Sequence[int], budget: int, max_batch: int) -> List[List[int]]:
    """Indices of `weights` split greedily into consecutive chunks, in list order: a chunk takes the next item as long as its sum
    of weights stays within budget and its length within max_batch; an item heavier than the budget is a chunk of its own."""
    chunks: List[List[int]] = []
    total = 0
    for i, n in enumerate(weights):
        if chunks and total + n <= budget and len(chunks[-1]) < max_batch:
            chunks[-1].append(i)
            total += n
        else:
            chunks.append([i])
            total = n
    return chunks


def long_refusal(L: int, long_on: bool) -> Optional[str]:
    """Why the long entry points do not take a stitched alignment of L body columns; None where they do.  "" with
    data.long_heads=stitched off: the line the CLI prints then names no reason."""
    if not long_on:
        return ""
    if L > _lib.LONG_MAX_L:
        return f"L exceeds the long heads' limit of {_lib.LONG_MAX_L}"
    return None


class _Block(nn.Module):
    """Parameters of the reference's BasicBlock (code/model.py:32-85)."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(CHANNELS, CHANNELS, 3, padding=1, bias=False)
        self.bn1 = nn.LayerNorm(CHANNELS)
        self.conv2 = nn.Conv2d(CHANNELS, CHANNELS, 5, padding=2, bias=False)
        self.bn2 = nn.LayerNorm(CHANNELS)


class SSPredictor(nn.Module):
    """The reference's ResNet(128, BasicBlock, [num_blocks]) (renet_b16: 16 blocks) as parameters; the forward is the HIP head.

    predict(atp, seq) -> [L, L] base-pair probabilities (sigmoid of the head, what predict.py hands to the post-processing);
    logits(atp, seq) -> the pre-sigmoid values.  atp: the [120, L, L] fp32 maps on the HIP device (a view whose planes lie
    further apart is read in place); seq: the query sequence (str) or its base codes (uint8 [L], see base_codes).
    gemm_dtype: "f32" (default: rnamsm_ss_head, exact fp32) or "bf16" (rnamsm_ss_head16: conv operands in bf16, everything else
    fp32); every method that runs the head follows it, and nothing else does -- the formatter and the decoding read whatever
    probabilities the head made."""

    def __init__(self, num_blocks: int = 16, gemm_dtype: str = "f32"):
        super().__init__()
        if not 1 <= num_blocks <= 64:
            raise ValueError(f"num_blocks must be in [1, 64], got {num_blocks}")
        self.num_blocks = num_blocks
        self.gemm_dtype = gemm_dtype
        self.conv1 = nn.Conv2d(IN_PLANES, CHANNELS, 3, padding=1)
        self.bn1 = nn.LayerNorm(CHANNELS)
        self.layer1 = nn.Sequential(*[_Block() for _ in range(num_blocks)])
        self.fc1 = nn.Linear(CHANNELS, 1)
        self._pack_key = None
        self._pack = None
        self._pack16 = None

    @property
    def gemm_dtype(self) -> str:
        return self._gemm_dtype

    @gemm_dtype.setter
    def gemm_dtype(self, value: str) -> None:
        if value not in _lib.SS_GEMM_DTYPES:
            raise ValueError(f"SSPredictor: gemm_dtype must be one of {', '.join(_lib.SS_GEMM_DTYPES)}, got {value!r}")
        self._gemm_dtype = value

    # ------------------------------------------------------------------ weight table of rnamsm_ss_head
    def _packed_weights(self):
        """The weight-pointer table in the kernel layout (conv weights tap-major [kh][kw][out][in]), rebuilt when a parameter was
        replaced or written in place since (its data_ptr or version counter moved) -- the MSATransformer._packed_weights rule.
        In the bf16 mode: the table of rnamsm_ss_head16, whose conv entries are bf16 planes made on the device from those of the
        fp32 table, once per pack key."""
        params = list(self.parameters())
        key = tuple((p.data_ptr(), p._version, p.device) for p in params)
        if key != self._pack_key:
            self._pack = self._fp32_table(key)
            self._pack16 = None
        if self._gemm_dtype != "bf16":
            return self._pack
        if self._pack16 is None:
            ptrs, keep = self._pack
            planes = {i: ops.ss_pack_conv16(t) for i, t in enumerate(keep) if t.dim() == 4}
            self._pack16 = ((ctypes.c_void_p * len(keep))(*[planes.get(i, t).data_ptr() for i, t in enumerate(keep)]), (keep, planes))
        return self._pack16

    def _fp32_table(self, key):
        if self.conv1.weight.device.type != "cuda":
            raise _lib.RnamsmError("SSPredictor must be moved to the HIP device (.to('cuda')): no CPU path exists")
        keep: List[torch.Tensor] = []

        def conv(w: torch.Tensor) -> torch.Tensor:
            t = w.detach().to(torch.float32).permute(2, 3, 0, 1).contiguous()
            keep.append(t)
            return t

        def vec(w: torch.Tensor) -> torch.Tensor:
            t = w.detach().to(torch.float32).reshape(-1).contiguous().clone()
            keep.append(t)
            return t

        table = [conv(self.conv1.weight), vec(self.conv1.bias), vec(self.bn1.weight), vec(self.bn1.bias)]
        for blk in self.layer1:
            table += [conv(blk.conv1.weight), vec(blk.bn1.weight), vec(blk.bn1.bias),
                      conv(blk.conv2.weight), vec(blk.bn2.weight), vec(blk.bn2.bias)]
        table += [vec(self.fc1.weight), vec(self.fc1.bias)]
        assert len(table) == len(_lib.W_SS_STEM) + self.num_blocks * len(_lib.W_SS_BLOCK) + len(_lib.W_SS_HEAD)
        ptrs = (ctypes.c_void_p * len(table))(*[t.data_ptr() for t in table])
        self._pack = (ptrs, keep)
        self._pack_key = key
        return self._pack

    def _apply(self, fn, *args, **kwargs):
        self._pack_key = None
        return super()._apply(fn, *args, **kwargs)

    @staticmethod
    def _codes_of(atp, seq, name: str, seq_name: str, on_device: bool, max_L: int = _lib.SS_MAX_L) -> torch.Tensor:
        """The checks of one (maps, sequence) pair, named as the caller's arguments (`atp` / `atps[3]`) -> its base codes, flat.
        on_device: refuse maps off the HIP device here, before their shape (False: the caller does that for every item afterwards)."""
        if not isinstance(atp, torch.Tensor) or (on_device and not atp.is_cuda):
            raise _lib.RnamsmError(f"SSPredictor: {name} must be a tensor on the HIP device (no CPU path exists)")
        if atp.dim() != 3 or atp.shape[0] != NUM_MAPS or atp.shape[1] != atp.shape[2]:
            raise ValueError(f"SSPredictor: {name} must be [{NUM_MAPS}, L, L], got {tuple(atp.shape)}")
        L = atp.shape[-1]
        if L > max_L:
            raise ValueError(f"SSPredictor: {name}: L = {L} exceeds the head's limit of {max_L}")
        if isinstance(seq, str):
            seq = base_codes(seq)
        codes = torch.as_tensor(seq).reshape(-1)
        if codes.numel() != L:
            raise ValueError(f"SSPredictor: {seq_name} has length {codes.numel()} for attention maps of L = {L}")
        return codes

    def _run(self, atp: torch.Tensor, seq: Union[str, np.ndarray, torch.Tensor], want: str, long: bool = False) -> torch.Tensor:
        """long: the route of a stitched long alignment (rnamsm_ss_head_long, L up to LONG_MAX_L), exact fp32 only."""
        if long and self._gemm_dtype != "f32":
            raise ValueError(f"SSPredictor: the long head runs in exact fp32 only, not in gemm_dtype={self._gemm_dtype!r}")
        max_L = _lib.LONG_MAX_L if long else _lib.SS_MAX_L
        codes = self._codes_of(atp, seq, "atp", "seq", True, max_L).to(device=atp.device, dtype=torch.uint8)
        ptrs, _ = self._packed_weights()
        if long:
            return ops.ss_head_long(atp, codes, ptrs, self.num_blocks, want)
        return ops.ss_head(atp, codes, ptrs, self.num_blocks, want, self._gemm_dtype)

    def predict(self, atp: torch.Tensor, seq) -> torch.Tensor:
        return self._run(atp, seq, "probs")

    def logits(self, atp: torch.Tensor, seq) -> torch.Tensor:
        return self._run(atp, seq, "logits")

    forward = predict

    def predict_long(self, atp: torch.Tensor, seq) -> torch.Tensor:
        """predict() on the stitched maps of a long alignment, L up to LONG_MAX_L = 4096 (rnamsm_ss_head_long: the same kernels, so
        predict()'s bits where both run); exact fp32 only."""
        return self._run(atp, seq, "probs", long=True)

    def logits_long(self, atp: torch.Tensor, seq) -> torch.Tensor:
        return self._run(atp, seq, "logits", long=True)

    def _run_many(self, atps: Sequence[torch.Tensor], seqs: Sequence, want: str) -> List[torch.Tensor]:
        atps, seqs = list(atps), list(seqs)
        if len(atps) != len(seqs):
            raise ValueError(f"SSPredictor: {len(atps)} attention maps for {len(seqs)} sequences")
        # shapes and lengths first: they are wrong on any device
        codes = [self._codes_of(atp, seq, f"atps[{b}]", f"seqs[{b}]", False) for b, (atp, seq) in enumerate(zip(atps, seqs))]
        for b, atp in enumerate(atps):
            if not atp.is_cuda:
                raise _lib.RnamsmError(f"SSPredictor: atps[{b}] must be a tensor on the HIP device (no CPU path exists)")
        codes = [c.to(device=a.device, dtype=torch.uint8) for c, a in zip(codes, atps)]
        ptrs, _ = self._packed_weights()
        out: List[torch.Tensor] = []
        for chunk in plan_ss_chunks([a.shape[-1] for a in atps]):
            out += ops.ss_head_packed([atps[i] for i in chunk], [codes[i] for i in chunk], ptrs, self.num_blocks, want,
                                      self._gemm_dtype)
        return out

    def predict_many(self, atps: Sequence[torch.Tensor], seqs: Sequence) -> List[torch.Tensor]:
        """predict() of every (atps[b], seqs[b]) in as few launch sets as plan_ss_chunks allows (rnamsm_ss_head_packed: all the
        structures of a call share each launch); every result is bit-identical to predict() on that structure alone."""
        return self._run_many(atps, seqs, "probs")

    def logits_many(self, atps: Sequence[torch.Tensor], seqs: Sequence) -> List[torch.Tensor]:
        return self._run_many(atps, seqs, "logits")

    def predict_structure(self, atp: torch.Tensor, seq, letters=None):
        """predict() and structure() of its result -> (probs, partner, counts, ct body, bpseq body), all on the device.  letters:
        the characters the tables print (uint8 [L]); taken from seq when that is a str."""
        probs = self.predict(atp, seq)
        return (probs,) + structure(probs, _letters_for(seq, letters, probs.device))

    def predict_nested(self, atp: torch.Tensor, seq, letters=None, theta: float = _lib.SS_NESTED_THETA,
                       min_loop: int = _lib.SS_NESTED_MIN_LOOP):
        """predict() and nested_structure() of its result -> (probs, partner, counts [5], ct body, bpseq body, dbn), all on the
        device.  letters: as for predict_structure."""
        probs = self.predict(atp, seq)
        return (probs,) + tuple(nested_structure(probs, _letters_for(seq, letters, probs.device), theta, min_loop))

    def predict_structure_many(self, atps: Sequence[torch.Tensor], seqs: Sequence, letters: Optional[Sequence] = None):
        """predict_many() and structure_many() of its results -> a list of predict_structure()'s tuples, each the lone call's."""
        seqs = list(seqs)
        probs = self.predict_many(atps, seqs)
        letters = list(letters) if letters is not None else [None] * len(seqs)
        if len(letters) != len(seqs):
            raise ValueError(f"SSPredictor: {len(letters)} letter rows for {len(seqs)} sequences")
        rows = [_letters_for(s, l, p.device) for s, l, p in zip(seqs, letters, probs)]
        return [(p,) + st for p, st in zip(probs, structure_many(probs, rows))]


def load_predictor(path: Union[str, Path], device, num_blocks: int = 16, gemm_dtype: str = "f32") -> SSPredictor:
    """`rna-msm_attention.pt` (a plain state_dict) -> an SSPredictor on `device`, loaded strictly."""
    state = torch.load(path, map_location="cpu")
    model = SSPredictor(num_blocks, gemm_dtype)
    model.load_state_dict(state, strict=True)
    return model.eval().to(device)


def prob_text(probs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The bytes of `<name>.prob` for the [L, L] probabilities `probs` on the HIP device -> (uint8 [25 L^2], int32 [1]): the text
    np.savetxt would write, and the fallback word -- 1 when an element has no fixed-width form (outside [0, 1]: a NaN-poisoned
    map), in which case the text must not be used (write_ss_files then takes the np.savetxt path)."""
    return ops.ss_prob_text(probs)


def prob_text_many(probs: Sequence[torch.Tensor]) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """prob_text() of every matrix in as few calls as the batch limit allows; each result is the lone call's."""
    probs = list(probs)
    out: List[Tuple[torch.Tensor, torch.Tensor]] = []
    for i in range(0, len(probs), _lib.SS_MAX_BATCH):
        out += ops.ss_prob_text_packed(probs[i:i + _lib.SS_MAX_BATCH])
    return out


def letter_codes(seq: str) -> np.ndarray:
    """uint8 [L]: the bytes the tables print for seq; 0 for a character that is no single ASCII byte (the device then leaves the
    two tables of that structure to the host writer)."""
    return np.fromiter((ord(c) if ord(c) < 128 else 0 for c in seq), dtype=np.uint8, count=len(seq))


def _letters_for(seq, letters, device) -> torch.Tensor:
    if letters is None:
        if not isinstance(seq, str):
            raise ValueError("SSPredictor: letters are needed where the sequence is given as base codes")
        letters = letter_codes(seq)
    return torch.as_tensor(letters).reshape(-1).to(device=device, dtype=torch.uint8)


def structure(probs: torch.Tensor, letters: torch.Tensor):
    """The predicted structure of the [L, L] probabilities `probs` on the HIP device (rnamsm_ss_pairs); letters uint8 [L] on the
    device -> (partner int32 [L]: 0 = unpaired, else the partner's 1-based index; counts int32 [4]: pairs, bytes of the `.ct` body,
    bytes of the `.bpseq` body, fallback; ct body uint8 [32 L]; bpseq body uint8 [12 L]): what secondary_structure and the two
    np.savetxt tables of write_ss_files give on the host, byte for byte.  fallback == 1 (a letter of 0 or >= 128): the bodies are
    not to be used; the partner vector is valid either way."""
    return ops.ss_pairs(probs, letters)


def structure_many(probs: Sequence[torch.Tensor], letters: Sequence[torch.Tensor]):
    """structure() of every (probs[b], letters[b]) in as few calls as the batch limit allows; each result is the lone call's."""
    probs, letters = list(probs), list(letters)
    if len(probs) != len(letters):
        raise ValueError(f"structure_many: {len(probs)} matrices for {len(letters)} letter rows")
    out = []
    for i in range(0, len(probs), _lib.SS_MAX_BATCH):
        out += ops.ss_pairs_packed(probs[i:i + _lib.SS_MAX_BATCH], letters[i:i + _lib.SS_MAX_BATCH])
    return out


def prob_text_long(probs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """prob_text() for L up to LONG_MAX_L (rnamsm_ss_prob_text_long): the same bytes where both run."""
    return ops.ss_prob_text_long(probs)


def structure_long(probs: torch.Tensor, letters: torch.Tensor):
    """structure() for L up to LONG_MAX_L (rnamsm_ss_pairs_long: several bases per thread): the same four results, the host path's
    bytes for every L in range."""
    return ops.ss_pairs_long(probs, letters)


def nested_structure(probs: torch.Tensor, letters: torch.Tensor, theta: float = _lib.SS_NESTED_THETA,
                     min_loop: int = _lib.SS_NESTED_MIN_LOOP):
    """The NESTED structure of the [L, L] probabilities `probs` on the HIP device, L up to LONG_MAX_L (rnamsm_ss_nested): the
    pseudoknot-free matching that maximises the summed pair probability in excess of theta, hairpin loops of at least min_loop
    bases -> (partner int32 [L]; counts int32 [5]: pairs, bytes of the `.ct` body, bytes of the `.bpseq` body, fallback, score;
    ct body uint8 [32 L]; bpseq body uint8 [12 L]; the dot-bracket line uint8 [L]).  Exact integer arithmetic, stated in
    include/rnamsm.h and, in NumPy, by nested_structure_host: the same bytes for the same inputs, always.  Device only."""
    return ops.ss_nested(probs, letters, theta, min_loop)


def nested_structure_many(probs: Sequence[torch.Tensor], letters: Sequence[torch.Tensor], theta: float = _lib.SS_NESTED_THETA,
                          min_loop: int = _lib.SS_NESTED_MIN_LOOP):
    """nested_structure() of every (probs[b], letters[b]) in as few calls as the batch limit allows; each result is the lone call's."""
    probs, letters = list(probs), list(letters)
    if len(probs) != len(letters):
        raise ValueError(f"nested_structure_many: {len(probs)} matrices for {len(letters)} letter rows")
    out = []
    for i in range(0, len(probs), _lib.SS_MAX_BATCH):
        out += ops.ss_nested_packed(probs[i:i + _lib.SS_MAX_BATCH], letters[i:i + _lib.SS_MAX_BATCH], theta, min_loop)
    return out


def nested_structure_host(prob: np.ndarray, theta: float = _lib.SS_NESTED_THETA, min_loop: int = _lib.SS_NESTED_MIN_LOOP):
    """The contract of rnamsm_ss_nested in NumPy, for documentation and tools -> (partner int32 [L], score, dot-bracket str).  Written
    cell by cell for reading, O(L^3) steps of interpreted Python: seconds at L = 100, not usable much beyond L = 200.  Not a fallback
    of nested_structure(), which runs on the device or not at all."""
    p = np.asarray(prob, dtype=np.float32)
    L = p.shape[0]
    if p.shape != (L, L) or not 0.0 <= float(theta) < 1.0 or not 0 <= int(min_loop) <= _lib.SS_NESTED_MAX_LOOP:
        raise ValueError("nested_structure_host: an [L, L] matrix, theta in [0, 1) and min_loop in [0, 32] are needed")
    neg, th = -(1 << 30), np.float32(theta)
    w = np.full((L, L), neg, dtype=np.int64)
    q_theta = int(float(th) * 262144.0)
    for i in range(L):
        for j in range(i + min_loop + 1, L):
            if p[i, j] > th:                                       # float32 compare; NaN and -inf fail it
                w[i, j] = max(1, int(min(float(p[i, j]), 1.0) * 262144.0) - q_theta)
    N = np.zeros((L + 1, L + 1), dtype=np.int64)                   # N[i + 1, j + 1] = N(i, j): row / column 0 hold N(i, i - 1) = 0
    n = lambda i, j: int(N[i + 1, j + 1]) if j >= i else 0         # noqa: E731
    for j in range(L):
        for i in range(j - 1, -1, -1):
            best = n(i, j - 1)
            for k in range(i, j - min_loop):
                if w[k, j] > neg:
                    best = max(best, n(i, k - 1) + int(w[k, j]) + n(k + 1, j - 1))
            N[i + 1, j + 1] = best
    partner, stack = np.zeros(L, dtype=np.int32), [(0, L - 1)]
    while stack:
        i, j = stack.pop()
        if j <= i:
            continue
        if n(i, j) == n(i, j - 1):
            stack.append((i, j - 1))
            continue
        k = next(k for k in range(i, j - min_loop) if w[k, j] > neg and n(i, k - 1) + int(w[k, j]) + n(k + 1, j - 1) == n(i, j))
        partner[k], partner[j] = j + 1, k + 1
        stack += [(i, k - 1), (k + 1, j - 1)]
    return partner, n(0, L - 1), dbn_from_partner(partner)


def dbn_from_partner(partner) -> str:
    """The dot-bracket line of a NESTED partner vector: '(' at the lower base of a pair, ')' at the upper one, '.' elsewhere."""
    return "".join("." if p == 0 else "(" if p > b + 1 else ")" for b, p in enumerate(np.asarray(partner).reshape(-1)))


def write_dbn(name: str, seq: str, dbn, output_dir: Union[str, Path]) -> str:
    """`<output_dir>/SS_result/<name>.dbn`: three lines -- `>name`, the sequence's letters as `.bpseq` prints them, the brackets
    (a str, bytes or a uint8 array of len(seq)).  Returns the path."""
    if not isinstance(dbn, str):
        dbn = bytes(dbn if isinstance(dbn, (bytes, bytearray)) else np.ascontiguousarray(dbn, dtype=np.uint8)).decode("ascii")
    if len(dbn) != len(seq) or set(dbn) - set("()."):
        raise ValueError(f"write_dbn: a dot-bracket line of {len(dbn)} characters ({''.join(sorted(set(dbn)))!r}) for a sequence of length {len(seq)}")
    out = os.path.join(str(output_dir), "SS_result")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, name + ".dbn")
    with open(path, "w", encoding="utf-8", newline="\n") as f:
        f.write(f">{name}\n{seq}\n{dbn}\n")
    return path


def write_nested_files(seq: str, name: str, output_dir: Union[str, Path], partner, counts, ct_body, bpseq_body, dbn) -> str:
    """The files of the nested structure, from nested_structure()'s results on the host: `<output_dir>/SS_result/<name>.dbn`,
    `<name>.nested.ct` and `<name>.nested.bpseq` -- the headers of `.ct` / `.bpseq`, the bodies as the device wrote them; with
    counts[3] set (a letter that is no single ASCII byte) or a name outside ASCII the two tables are formatted on the host from the
    partner vector, as write_ss_files does.  Returns the `.dbn` path."""
    L = len(seq)
    partner, counts = np.asarray(partner).reshape(-1).astype(int), np.asarray(counts).reshape(-1)
    if partner.shape[0] != L or counts.shape[0] != 5:
        raise ValueError(f"write_nested_files: a partner vector of {partner.shape[0]} entries and {counts.shape[0]} counts for a "
                         f"sequence of length {L}")
    path = write_dbn(name, seq, dbn_from_partner(partner) if int(counts[3]) else dbn, output_dir)
    out = os.path.dirname(path)
    if int(counts[3]) or not name.isascii():
        _tables_on_host(out, name, seq, partner, stem=name + ".nested")
        return path
    bodies = []
    for body, n in ((ct_body, int(counts[1])), (bpseq_body, int(counts[2]))):
        body = memoryview(body if isinstance(body, (bytes, bytearray)) else np.ascontiguousarray(body, dtype=np.uint8))
        if not 0 < n <= body.nbytes:
            raise ValueError(f"write_nested_files: a body of {body.nbytes} bytes for a count of {n}")
        bodies.append(body[:n])
    _tables_from_bodies(out, name, L, bodies[0], bodies[1], stem=name + ".nested")
    return path


def pairs_from_partner(partner) -> List[Tuple[int, int]]:
    """The list secondary_structure returns -- pairs (i, j), i < j, 0-based, sorted -- from a partner vector (0 = unpaired, else the
    partner's 1-based index)."""
    if isinstance(partner, torch.Tensor):
        partner = partner.cpu().numpy()
    partner = np.asarray(partner).reshape(-1)
    return [(int(i), int(partner[i]) - 1) for i in np.nonzero(partner)[0] if partner[i] - 1 > i]


# ---------------------------------------------------------------------- post-processing (processing_output.py)
def _multiplet_free(pairs: List[Tuple[int, int]], prob: np.ndarray) -> List[Tuple[int, int]]:
    """multiplets_free_bp: while some base is in two or more pairs, drop -- for every such base, in ascending base order,
    among its pairs in list order -- the first pair of lowest probability, all of one round's choices at once."""
    while True:
        count = {}
        for i, j in pairs:
            count[i] = count.get(i, 0) + 1
            count[j] = count.get(j, 0) + 1
        multi = sorted(b for b, n in count.items() if n > 1)
        if not multi:
            return pairs
        drop = set()
        for b in multi:
            group = [p for p in pairs if b in p]
            vals = [prob[p[0], p[1]] for p in group]
            drop.add(group[vals.index(min(vals))])
        pairs = [p for p in pairs if p not in drop]


def secondary_structure(prob: np.ndarray) -> List[Tuple[int, int]]:
    """Base pairs (i < j, 0-based) of an [L, L] probability matrix: the upper triangle above THRESHOLD in np.triu_indices
    order, then made multiplet-free.  Only i < j is read: the matrix is not symmetric."""
    prob = np.asarray(prob)
    ii, jj = np.triu_indices(prob.shape[0], k=1)
    keep = prob[ii, jj] > THRESHOLD
    pairs = [(int(i), int(j)) for i, j in zip(ii[keep], jj[keep])]
    return _multiplet_free(pairs, prob)


def _tables_on_host(out: str, name: str, seq: str, partner: np.ndarray, stem: Optional[str] = None) -> None:
    """`<out>/<name>.ct` and `.bpseq` as the reference builds them: string tables through np.savetxt.  stem: the files' name where
    it is not the one the headers carry (`<name>.nested`)."""
    stem = name if stem is None else stem
    L = len(seq)
    idx = np.arange(1, L + 1)
    bases = np.array(list(seq))
    fmt_int = lambda a: np.char.mod("%d", a)          # noqa: E731
    ct = np.vstack((fmt_int(idx), bases, fmt_int(idx - 1), fmt_int(np.append(idx[1:], [0])), fmt_int(partner),
                    fmt_int(idx))).T
    np.savetxt(os.path.join(out, stem + ".ct"), ct, delimiter="\t\t", fmt="%s",
               header=f"{L}\t\t{name}\t\tRNAMSM_SS output\n", comments="")
    bp = np.vstack((fmt_int(idx), bases, fmt_int(partner))).T
    np.savetxt(os.path.join(out, stem + ".bpseq"), bp, delimiter=" ", fmt="%s", header="#" + name, comments="")


def _tables_from_bodies(out: str, name: str, L: int, ct_body, bpseq_body, stem: Optional[str] = None) -> None:
    """The same two files from device-made bodies: the header line and one binary write each.  np.savetxt ends the header with a
    newline of its own: the .ct header, which ends in one already, is followed by an empty line."""
    for ext, head, body in ((".ct", f"{L}\t\t{name}\t\tRNAMSM_SS output\n\n", ct_body), (".bpseq", f"#{name}\n", bpseq_body)):
        with open(os.path.join(out, (name if stem is None else stem) + ext), "wb") as f:
            f.write(head.encode("ascii"))
            f.write(body)


def write_ss_files(prob: Optional[np.ndarray], seq: str, name: str, output_dir: Union[str, Path], prob_text=None,
                   fallback: int = 0, *, partner=None, counts=None, ct_body=None, bpseq_body=None) -> List[Tuple[int, int]]:
    """`<output_dir>/SS_result/<name>.{ct,bpseq,prob}` as the reference writes them; returns the pairs.
    prob_text, fallback: the text and the fallback word of prob_text(prob), on the host (bytes or a uint8 array of 25 L^2).  With a
    text and fallback == 0 the `.prob` file is one binary write of it; otherwise np.savetxt formats `prob` as before -- the same
    bytes either way.
    partner, counts, ct_body, bpseq_body: the results of structure(prob, letters), on the host.  With a partner vector the pairs are
    read from it instead of being decoded from `prob`; with the bodies and counts too, and counts[3] == 0, `.ct` and `.bpseq` are a
    header line and one binary write each -- otherwise np.savetxt builds the two tables as before, the same bytes either way.
    `prob` may be None when neither file needs it: a partner vector and a usable `.prob` text are given."""
    L = len(seq)
    if prob is not None:
        prob = np.asarray(prob, dtype=np.float32)
        if prob.shape != (L, L):
            raise ValueError(f"write_ss_files: probabilities of shape {prob.shape} for a sequence of length {L}")
    if prob_text is not None and not int(fallback):
        prob_text = memoryview(prob_text if isinstance(prob_text, (bytes, bytearray)) else np.ascontiguousarray(prob_text, dtype=np.uint8))
        if prob_text.nbytes != _lib.SS_TEXT_RECORD * L * L:
            raise ValueError(f"write_ss_files: a text of {prob_text.nbytes} bytes for a sequence of length {L}")
    else:
        prob_text = None
    if prob is None and (partner is None or prob_text is None):
        raise ValueError("write_ss_files: without probabilities a partner vector and a usable .prob text are needed")
    if partner is not None:
        partner = np.asarray(partner).reshape(-1).astype(int)
        if partner.shape[0] != L:
            raise ValueError(f"write_ss_files: a partner vector of {partner.shape[0]} entries for a sequence of length {L}")
        pairs = pairs_from_partner(partner)
    else:
        pairs = secondary_structure(prob)
        partner = np.zeros(L, dtype=int)
        for i, j in pairs:
            partner[i] = j + 1
            partner[j] = i + 1
    bodies = None
    if ct_body is not None and bpseq_body is not None and counts is not None and name.isascii():
        counts = np.asarray(counts).reshape(-1)
        if counts.shape[0] != 4:
            raise ValueError(f"write_ss_files: {counts.shape[0]} counts, not 4")
        if not int(counts[3]):
            bodies = []
            for body, n in ((ct_body, int(counts[1])), (bpseq_body, int(counts[2]))):
                body = memoryview(body if isinstance(body, (bytes, bytearray)) else np.ascontiguousarray(body, dtype=np.uint8))
                if not 0 < n <= body.nbytes:
                    raise ValueError(f"write_ss_files: a body of {body.nbytes} bytes for a count of {n}")
                bodies.append(body[:n])
    out = os.path.join(str(output_dir), "SS_result")
    os.makedirs(out, exist_ok=True)
    if bodies is not None:
        _tables_from_bodies(out, name, L, bodies[0], bodies[1])
    else:
        _tables_on_host(out, name, seq, partner)
    if prob_text is not None:
        with open(os.path.join(out, name + ".prob"), "wb") as f:
            f.write(prob_text)
    else:
        np.savetxt(os.path.join(out, name + ".prob"), prob, delimiter="\t")
    return pairs


# ---------------------------------------------------------------------- the head in the CLI (rnamsm.inference.extract_feat)
def token_base_codes(alphabet, device) -> torch.Tensor:
    """uint8 [number of tokens] on `device`: a token's base code (0..3 for A, C, G, U, else 255), the look-up table both heads index
    with the query's tokens."""
    lut = torch.full((len(alphabet.all_toks),), 255, dtype=torch.uint8)
    for code, ch in enumerate("ACGU"):
        lut[alphabet.tok_to_idx[ch]] = code
    return lut.to(device)


class SSResult(NamedTuple):
    """One alignment's results of the SS head, on the device (or, on the writer's side, their host copies)."""
    probs: Optional[torch.Tensor]                 # [L, L] base-pair probabilities
    tokens: torch.Tensor                          # [L] the query's tokens
    text: Optional[tuple] = None                  # prob_text(probs): (text, fallback word); None where the formatter is off
    structure: Optional[tuple] = None             # structure(probs, letters): (partner, counts, ct body, bpseq body); None where off
    nested: Optional[tuple] = None                # nested_structure(probs, letters): (partner, counts [5], ct body, bpseq body, dbn)


class SSHead:
    """data.ss_model_path in the CLI: the predictor, the two look-up tables indexed by token (base codes; the letters the tables
    print) and the two switches -- text_on (data.ss_prob_text: the `.prob` text is formatted on the device) and pairs_on
    (data.ss_pairs_device: the pairs are decoded and the bodies of `.ct` / `.bpseq` written there)."""

    def __init__(self, model: Optional[SSPredictor], alphabet, base_lut: Optional[torch.Tensor], device, text_on: bool = True,
                 pairs_on: bool = True, nested: Optional[Tuple[float, int]] = None):
        """nested: (theta, min_loop) of data.ss_nested (the nested structure is decoded on the device behind the head and travels in
        the record's last field), or None.  It never goes through a gather: flatten() / unflatten() do not carry it."""
        self.model, self.base_lut, self.text_on, self.pairs_on = model, base_lut, bool(text_on), bool(pairs_on)
        self.nested = None if nested is None else (float(nested[0]), int(nested[1]))
        self.all_toks = list(alphabet.all_toks)
        # a token that is no single ASCII character is 0: that structure's tables come from the host
        self.letters_lut = torch.tensor([ord(t) if len(t) == 1 and ord(t) < 128 else 0 for t in self.all_toks],
                                        dtype=torch.uint8).to(device) if self.pairs_on or self.nested else None
        self.n_tensors = 2 + 2 * self.text_on + 4 * self.pairs_on

    # ------------------------------------------------------------------ records
    def _one(self, emb: torch.Tensor, atp: torch.Tensor, tokens: torch.Tensor, long: bool) -> SSResult:
        predict, text, pairs = ((self.model.predict_long, prob_text_long, structure_long) if long
                                else (self.model.predict, prob_text, structure))
        probs = predict(atp, self.base_lut[tokens])
        return SSResult(probs, tokens, tuple(text(probs)) if self.text_on else None,
                        tuple(pairs(probs, self.letters_lut[tokens])) if self.pairs_on else None,
                        tuple(nested_structure(probs, self.letters_lut[tokens], *self.nested)) if self.nested else None)

    def one(self, emb: torch.Tensor, atp: torch.Tensor, tokens: torch.Tensor) -> SSResult:
        """A lone alignment through the lone ops; atp is read where it lies (emb is not read: the heads share one signature).  The
        formatter and the decoding run behind the head."""
        return self._one(emb, atp, tokens, False)

    def one_long(self, emb: torch.Tensor, atp: torch.Tensor, tokens: torch.Tensor) -> SSResult:
        """one() on a stitched long alignment (data.long_heads=stitched), L up to LONG_MAX_L: the same record through the long entry
        points; with a switch off, that part is left to the host writer, which has no length limit."""
        return self._one(emb, atp, tokens, True)

    def stitched_route(self, L: int, long_on: bool):
        """On a stitched alignment of L body columns (data.long_msa=windows): the method that runs this head, or the reason (a str)
        it is skipped; long_on: data.long_heads=stitched."""
        why = long_refusal(L, long_on)
        if why is None and self.model.gemm_dtype != "f32":
            why = f"there is no long SS head under data.ss_gemm_dtype={self.model.gemm_dtype}"
        return self.one_long if why is None else why

    def many(self, embs: Sequence[torch.Tensor], atps: Sequence[torch.Tensor], tokens: Sequence[torch.Tensor]) -> List[SSResult]:
        """A group in one launch set per stage (predict_many, prob_text_many, structure_many): every member's record holds the bits
        and bytes of one()."""
        probs = self.model.predict_many(atps, [self.base_lut[t] for t in tokens])
        texts = prob_text_many(probs) if self.text_on else [None] * len(probs)
        structs = structure_many(probs, [self.letters_lut[t] for t in tokens]) if self.pairs_on else [None] * len(probs)
        nests = (nested_structure_many(probs, [self.letters_lut[t] for t in tokens], *self.nested) if self.nested
                 else [None] * len(probs))
        return [SSResult(p, t, None if tx is None else tuple(tx), None if st is None else tuple(st), None if ne is None else tuple(ne))
                for p, t, tx, st, ne in zip(probs, tokens, texts, structs, nests)]

    # ------------------------------------------------------------------ the gather's flat lists
    def flatten(self, rec: SSResult) -> list:
        return [rec.probs, rec.tokens, *(rec.text or ()), *(rec.structure or ())]

    def unflatten(self, tensors: Sequence) -> SSResult:
        """The record of flatten()'s list (n_tensors entries), by this head's switches."""
        if len(tensors) != self.n_tensors:
            raise ValueError(f"SSHead: {len(tensors)} tensors for a record of {self.n_tensors}")
        it = iter(tensors)
        probs, tokens = next(it), next(it)
        text = (next(it), next(it)) if self.text_on else None
        return SSResult(probs, tokens, text, (next(it), next(it), next(it), next(it)) if self.pairs_on else None)

    # ------------------------------------------------------------------ files
    def letters(self, tokens) -> str:
        return "".join(self.all_toks[int(t)] for t in tokens)

    def writer_job(self, rec: SSResult, name: str, output_dir, fetch_probs: Optional[Callable[[], np.ndarray]] = None):
        """-> (write, tensors): write(*host copies of tensors) writes <output_dir>/SS_result/<name>.{ct,bpseq,prob} through
        write_ss_files.  The tensors are the query's tokens, the text and its fallback word, the partner vector, the counts and the two
        bodies, as far as the record has them, then the probabilities -- unless it has both a text and a structure: then they stay where
        they are, and write() fetches them (fetch_probs; default: from rec.probs) only for a map whose text could not be formatted (a
        NaN-poisoned one)."""
        probs, has_text, has_structure, has_nested = rec.probs, rec.text is not None, rec.structure is not None, rec.nested is not None
        lazy = has_text and has_structure
        if fetch_probs is None:         # holds the probabilities alone: the job's other tensors are released once their copies have run
            fetch_probs = lambda: probs.cpu().numpy()      # noqa: E731  (behind the writer's event: the head has run)

        def write(tokens, *made) -> None:
            made, kw = list(made), {}
            if has_text:
                kw.update(prob_text=made.pop(0), fallback=int(made.pop(0)[0]))
            if has_structure:
                kw.update(partner=made.pop(0), counts=made.pop(0), ct_body=made.pop(0), bpseq_body=made.pop(0))
            nested = [made.pop(0) for _ in range(5)] if has_nested else None
            if lazy:
                prob = fetch_probs() if kw["fallback"] else None
            else:
                prob = made.pop(0)
            assert not made
            write_ss_files(prob, self.letters(tokens), name, output_dir, **kw)
            if nested is not None:          # the reference's three files stay as they are: .dbn, .nested.ct, .nested.bpseq beside them
                write_nested_files(self.letters(tokens), name, output_dir, *nested)

        return write, (rec.tokens, *(rec.text or ()), *(rec.structure or ()), *(rec.nested or ()), *(() if lazy else (probs,)))
