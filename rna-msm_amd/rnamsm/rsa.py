"""RNA-MSM RSA: relative solvent accessibility from the embedding (the reference's _downstream_tasks/RSA).

`RSAPredictor` carries the parameters of one of the reference's `FrameModel(Cin, 1, planes=64, depth=1)` networks under the same
names and shapes, so a state_dict taken from an upstream model loads with strict=True; `RSAEnsemble` holds K of them and the
normalisation statistics, and its arithmetic is one HIP entry point (rnamsm_rsa_head: all members in four launches, exact fp32)
that reads the [L, 768] embedding where it lies on the device; `predict_long` does the same up to L = 4096 (rnamsm_rsa_head_long,
for a stitched long alignment); `predict_many` runs a list of alignments through the same four
launches (rnamsm_rsa_head_packed), every result the lone call's bits; `predict_text[_many]` adds the bodies of the result tables,
formatted on the device (rnamsm_rsa_text: `table_text`).  `load_ensemble` reads an upstream model directory -- its `.pt`
files are pickled whole modules and are opened with no upstream code importable -- and `write_rsa_files` is the reference's
host arithmetic and text format (predict.py: doSavePredict_single, per model and for the ensemble), byte for byte -- or, handed the
device-made bodies, a header and one binary write per table, the same bytes.  `RSAHead` is the
ensemble as the CLI runs it: it makes one `RSAResult` per alignment and turns it into the job that writes the texts.
"""
from __future__ import annotations

import ctypes
import glob
import os
import pickle
import re
import types
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import nn

from . import _lib, ops
from .ss import base_codes, letter_codes, long_refusal, plan_chunks

EMBED_DIM = 768
PLANES = 64
HEADS = 8
BN_EPS = 1e-5
ASA_SCALE = {"A": 400, "U": 350, "C": 350, "G": 400}       # predict.py: BASES 'AUCG', asa_std
_BASES = "AUCG"
# positions of one packed call: 32768 x 7 x 64 floats x K of workspace is 176 MB at K = 3 and 470 MB at K = 8, the order of the SS
# head's 403 MB ceiling (a condition, not a measurement)
RSA_CHUNK_POSITIONS = 32768


def plan_rsa_chunks(Ls: Sequence[int], max_positions: int = RSA_CHUNK_POSITIONS, max_batch: int = _lib.RSA_MAX_BATCH) -> List[List[int]]:
    """Indices of `Ls` split into consecutive calls of rnamsm_rsa_head_packed, in list order: a chunk takes the next alignment as
    long as its sum of L stays within max_positions and its length within max_batch (greedy, so no two neighbouring chunks could
    have been one).  An alignment larger than the budget by itself -- impossible at the default, L <= 1024 -- is a chunk of its
    own."""
    return plan_chunks([int(L) for L in Ls], max_positions, max_batch)


class _BasicBlock(nn.Module):
    """Parameters of the reference's squeeze-excite BasicBlock (model/_0713/resnet.py)."""

    def __init__(self, cin: int):
        super().__init__()
        self.conv1 = nn.Conv1d(cin, PLANES, 3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm1d(PLANES)
        self.conv2 = nn.Conv1d(PLANES, PLANES, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm1d(PLANES)
        self.shortcut = nn.Sequential(nn.Conv1d(cin, PLANES, 1, bias=False), nn.BatchNorm1d(PLANES))
        self.fc1 = nn.Conv1d(PLANES, PLANES // 16, 1)
        self.fc2 = nn.Conv1d(PLANES // 16, PLANES, 1)


class _SelfAttention(nn.Module):
    def __init__(self):
        super().__init__()
        self.key = nn.Linear(PLANES, PLANES)
        self.query = nn.Linear(PLANES, PLANES)
        self.value = nn.Linear(PLANES, PLANES)
        self.proj = nn.Linear(PLANES, PLANES)


class _Block(nn.Module):
    """Parameters of the reference's minGPT Block (model/_0713/mingpt.py)."""

    def __init__(self):
        super().__init__()
        self.ln1 = nn.LayerNorm(PLANES)
        self.ln2 = nn.LayerNorm(PLANES)
        self.attn = _SelfAttention()
        self.mlp = nn.Sequential(nn.Linear(PLANES, 4 * PLANES), nn.GELU(), nn.Linear(4 * PLANES, PLANES), nn.Dropout(0.1))


class RSAPredictor(nn.Module):
    """One member: the reference's FrameModel(Cin, 1, planes=64, depth=1, norm_layer_type='BATCHNORM1D') as parameters and
    BatchNorm running statistics (state_dict names `net.0.0.conv1.weight` ... `net.1.0.mlp.2.bias`, `final.*`).
    Cin = 773 (one-hot + embedding + mask) or 769 (embedding + mask).  The arithmetic lives in RSAEnsemble."""

    def __init__(self, cin: int = 4 + EMBED_DIM + 1):
        super().__init__()
        if cin not in (EMBED_DIM + 1, 4 + EMBED_DIM + 1):
            raise ValueError(f"RSAPredictor: {cin} input channels; the network takes {4 + EMBED_DIM + 1} (one-hot + embedding + mask) "
                             f"or {EMBED_DIM + 1} (embedding + mask)")
        self.cin = cin
        self.net = nn.Sequential(nn.Sequential(_BasicBlock(cin)), nn.Sequential(_Block()))
        self.final = nn.Linear(PLANES, 1)

    @property
    def use_onehot(self) -> bool:
        return self.cin == 4 + EMBED_DIM + 1

    @classmethod
    def from_state_dict(cls, state: Dict[str, torch.Tensor]) -> "RSAPredictor":
        """Cin is read off net.0.0.conv1.weight; everything is loaded strictly."""
        w = state.get("net.0.0.conv1.weight")
        if w is None or w.dim() != 3:
            raise _lib.RnamsmError("RSAPredictor: the state has no net.0.0.conv1.weight [64, Cin, 3]")
        model = cls(int(w.shape[1]))
        model.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()}, strict=True)
        return model.eval()

    def packed(self) -> List[torch.Tensor]:
        """The member's 26 table entries in the kernel layout (include/rnamsm.h): BatchNorm folded in float64 into scale / shift,
        matrices transposed to [in][out], the stem's three conv taps and the shortcut as four zero-padded [800][64] slabs."""
        blk, gpt = self.net[0][0], self.net[1][0]
        dev = blk.conv1.weight.device

        def f32(t: torch.Tensor) -> torch.Tensor:
            return t.detach().to(torch.float32).contiguous().clone()

        def bn(m: nn.BatchNorm1d) -> Tuple[torch.Tensor, torch.Tensor]:
            scale = m.weight.detach().double() / torch.sqrt(m.running_var.detach().double() + m.eps)
            shift = m.bias.detach().double() - m.running_mean.detach().double() * scale
            return f32(scale), f32(shift)

        stem = torch.zeros(4, _lib.RSA_CIN_PAD, PLANES, dtype=torch.float32, device=dev)
        stem[:3, :self.cin] = blk.conv1.weight.detach().to(torch.float32).permute(2, 1, 0)
        stem[3, :self.cin] = blk.shortcut[0].weight.detach().to(torch.float32)[:, :, 0].t()
        att = gpt.attn
        qkv_w = torch.stack([f32(m.weight).t() for m in (att.query, att.key, att.value)])
        qkv_b = torch.stack([f32(m.bias) for m in (att.query, att.key, att.value)])
        table = [stem, *bn(blk.bn1), *bn(blk.shortcut[1]), f32(blk.conv2.weight.permute(2, 1, 0)), *bn(blk.bn2),
                 f32(blk.fc1.weight[:, :, 0]), f32(blk.fc1.bias), f32(blk.fc2.weight[:, :, 0]), f32(blk.fc2.bias),
                 f32(gpt.ln1.weight), f32(gpt.ln1.bias), f32(qkv_w), f32(qkv_b), f32(att.proj.weight.t()), f32(att.proj.bias),
                 f32(gpt.ln2.weight), f32(gpt.ln2.bias), f32(gpt.mlp[0].weight.t()), f32(gpt.mlp[0].bias),
                 f32(gpt.mlp[2].weight.t()), f32(gpt.mlp[2].bias), f32(self.final.weight.reshape(-1)), f32(self.final.bias)]
        assert len(table) == len(_lib.W_RSA_MODEL)
        return table


class RSAEnsemble(nn.Module):
    """K RSAPredictors of one kind and their normalisation statistics; the forward is the HIP head.

    predict(emb, seq) -> [K, L] RSA of every member (what predict.py hands to doSavePredict_single); logits(emb, seq) -> the
    pre-sigmoid values.  emb: the [L, 768] fp32 embedding on the HIP device (a view whose rows lie further apart is read in
    place); seq: the sequence (str) or its base codes (uint8 [L], rnamsm.ss.base_codes).
    stats: {"emb": (mu, std)} and, for the one-hot kind, {"oh": (mu, std)}.  The embedding statistics are held in float32 and the
    one-hot statistics in float64, as the reference ships them: numpy's arithmetic on them is what the kernel repeats."""

    def __init__(self, members: Sequence[RSAPredictor], stats: Dict[str, Tuple[np.ndarray, np.ndarray]],
                 names: Optional[Sequence[str]] = None):
        super().__init__()
        members = list(members)
        if not 1 <= len(members) <= _lib.RSA_MAX_MODELS:
            raise ValueError(f"RSAEnsemble: {len(members)} members; the head takes 1 to {_lib.RSA_MAX_MODELS}")
        if len({m.cin for m in members}) != 1:
            raise ValueError("RSAEnsemble: members of both kinds (773 and 769 input channels) in one ensemble")
        self.members = nn.ModuleList(members)
        self.use_onehot = members[0].use_onehot
        self.model_names = list(names) if names is not None else [f"model_{i}" for i in range(len(members))]
        if len(self.model_names) != len(members):
            raise ValueError("RSAEnsemble: one name per member")
        if "emb" not in stats or (self.use_onehot and "oh" not in stats):
            raise _lib.RnamsmError("RSAEnsemble: statistics missing ('emb', and 'oh' for the one-hot kind)")
        mu, std = (np.asarray(a).reshape(-1) for a in stats["emb"])
        if mu.shape != (EMBED_DIM,) or std.shape != (EMBED_DIM,):
            raise ValueError(f"RSAEnsemble: embedding statistics of shapes {mu.shape}, {std.shape}, expected ({EMBED_DIM},)")
        self.register_buffer("mu_emb", torch.from_numpy(mu.astype(np.float32)))
        self.register_buffer("std_emb", torch.from_numpy(std.astype(np.float32)))
        if self.use_onehot:
            mu, std = (np.asarray(a, dtype=np.float64).reshape(-1) for a in stats["oh"])
            if mu.shape != (4,) or std.shape != (4,):
                raise ValueError(f"RSAEnsemble: one-hot statistics of shapes {mu.shape}, {std.shape}, expected (4,)")
            self.register_buffer("mu_oh", torch.from_numpy(mu.copy()))
            self.register_buffer("std_oh", torch.from_numpy(std.copy()))
        self._pack_key = None
        self._pack = None

    def __len__(self) -> int:
        return len(self.members)

    # ------------------------------------------------------------------ weight table of rnamsm_rsa_head
    def _packed_weights(self):
        """The weight-pointer table (statistics, then every member's packed entries), rebuilt when a parameter or buffer was
        replaced or written in place since (its data_ptr or version counter moved) -- the SSPredictor._packed_weights rule."""
        tensors = list(self.parameters()) + list(self.buffers())
        key = tuple((p.data_ptr(), p._version, p.device) for p in tensors)
        if key == self._pack_key:
            return self._pack
        if self.mu_emb.device.type != "cuda":
            raise _lib.RnamsmError("RSAEnsemble must be moved to the HIP device (.to('cuda')): no CPU path exists")
        keep: List[torch.Tensor] = [self.mu_emb.to(torch.float32).contiguous().clone(), self.std_emb.to(torch.float32).contiguous().clone()]
        if self.use_onehot:       # (nn.Module.to(dtype) would have narrowed them with everything else: held in float64 whatever happened)
            keep += [self.mu_oh.to(torch.float64).contiguous().clone(), self.std_oh.to(torch.float64).contiguous().clone()]
            head = [t.data_ptr() for t in keep]
        else:
            head = [t.data_ptr() for t in keep] + [None, None]
        table = []
        for m in self.members:
            table += m.packed()
        keep += table
        assert len(head) == len(_lib.W_RSA_GLOBAL)
        ptrs = (ctypes.c_void_p * (len(head) + len(table)))(*(head + [t.data_ptr() for t in table]))
        self._pack = (ptrs, keep)
        self._pack_key = key
        return self._pack

    def _apply(self, fn, *args, **kwargs):
        self._pack_key = None
        return super()._apply(fn, *args, **kwargs)

    @staticmethod
    def _codes_of(emb, seq, name: str, seq_name: str, on_device: bool, max_L: int = _lib.RSA_MAX_L) -> torch.Tensor:
        """The checks of one (embedding, sequence) pair, named as the caller's arguments (`emb` / `embs[3]`) -> its base codes, flat.
        on_device: refuse an embedding off the HIP device here, before its shape (False: the caller does that for every item
        afterwards)."""
        if not isinstance(emb, torch.Tensor) or (on_device and not emb.is_cuda):
            raise _lib.RnamsmError(f"RSAEnsemble: {name} must be a tensor on the HIP device (no CPU path exists)")
        if emb.dim() != 2 or emb.shape[1] != EMBED_DIM:
            raise ValueError(f"RSAEnsemble: {name} must be [L, {EMBED_DIM}], got {tuple(emb.shape)}")
        L = emb.shape[0]
        if not 1 <= L <= max_L:
            raise ValueError(f"RSAEnsemble: {name}: L = {L} outside the head's range [1, {max_L}]")
        if isinstance(seq, str):
            seq = base_codes(seq)
        codes = torch.as_tensor(seq).reshape(-1)
        if codes.numel() != L:
            raise ValueError(f"RSAEnsemble: {seq_name} has length {codes.numel()} for an embedding of L = {L}")
        return codes

    def _run(self, emb: torch.Tensor, seq: Union[str, np.ndarray, torch.Tensor], want: str, long: bool = False) -> torch.Tensor:
        """long: the route of a stitched long alignment (rnamsm_rsa_head_long, L up to LONG_MAX_L); there the shape and the length
        are checked before the device: they are wrong on any device."""
        codes = self._codes_of(emb, seq, "emb", "seq", not long, _lib.LONG_MAX_L if long else _lib.RSA_MAX_L)
        if not emb.is_cuda:
            raise _lib.RnamsmError("RSAEnsemble: emb must be a tensor on the HIP device (no CPU path exists)")
        ptrs, _ = self._packed_weights()
        head = ops.rsa_head_long if long else ops.rsa_head
        return head(emb, codes.to(device=emb.device, dtype=torch.uint8), ptrs, len(self.members), self.use_onehot, want)

    def predict(self, emb: torch.Tensor, seq) -> torch.Tensor:
        return self._run(emb, seq, "probs")

    def logits(self, emb: torch.Tensor, seq) -> torch.Tensor:
        return self._run(emb, seq, "logits")

    forward = predict

    def predict_long(self, emb: torch.Tensor, seq) -> torch.Tensor:
        """predict() for L up to LONG_MAX_L (rnamsm_rsa_head_long: a stitched long alignment's embedding); the bits of predict()
        for an L both accept."""
        return self._run(emb, seq, "probs", long=True)

    def logits_long(self, emb: torch.Tensor, seq) -> torch.Tensor:
        return self._run(emb, seq, "logits", long=True)

    def predict_text_long(self, emb: torch.Tensor, seq, letters=None):
        """predict_text() for L up to LONG_MAX_L -> ([K, L] RSA, table_text_long of it)."""
        values = self.predict_long(emb, seq)
        return values, table_text_long(values, _letters_for(seq, letters, values.device))

    def _run_many(self, embs: Sequence[torch.Tensor], seqs: Sequence, want: str) -> List[torch.Tensor]:
        embs, seqs = list(embs), list(seqs)
        if len(embs) != len(seqs):
            raise ValueError(f"RSAEnsemble: {len(embs)} embeddings for {len(seqs)} sequences")
        # shapes and lengths first: they are wrong on any device
        codes = [self._codes_of(emb, seq, f"embs[{b}]", f"seqs[{b}]", False) for b, (emb, seq) in enumerate(zip(embs, seqs))]
        for b, emb in enumerate(embs):
            if not emb.is_cuda:
                raise _lib.RnamsmError(f"RSAEnsemble: embs[{b}] must be a tensor on the HIP device (no CPU path exists)")
        codes = [c.to(device=e.device, dtype=torch.uint8) for c, e in zip(codes, embs)]
        if not embs:
            return []
        ptrs, _ = self._packed_weights()
        out: List[torch.Tensor] = []
        for chunk in plan_rsa_chunks([e.shape[0] for e in embs]):
            out += ops.rsa_head_packed([embs[i] for i in chunk], [codes[i] for i in chunk], ptrs, len(self.members), self.use_onehot,
                                       want)
        return out

    def predict_many(self, embs: Sequence[torch.Tensor], seqs: Sequence) -> List[torch.Tensor]:
        """predict() of every (embs[b], seqs[b]) in as few launch sets as plan_rsa_chunks allows (rnamsm_rsa_head_packed: all the
        alignments of a call share each of the four launches); every [K, L_b] result is bit-identical to predict() on that
        alignment alone."""
        return self._run_many(embs, seqs, "probs")

    def logits_many(self, embs: Sequence[torch.Tensor], seqs: Sequence) -> List[torch.Tensor]:
        return self._run_many(embs, seqs, "logits")

    def predict_text(self, emb: torch.Tensor, seq, letters=None):
        """predict(), then the tables' text on the device -> ([K, L] RSA, table_text of it): what write_rsa_files(text=...) takes.
        letters: the characters the tables print (uint8 [L]); by default those of seq, which then has to be a str."""
        values = self.predict(emb, seq)
        return values, table_text(values, _letters_for(seq, letters, values.device))

    def predict_text_many(self, embs: Sequence[torch.Tensor], seqs: Sequence, letters: Optional[Sequence] = None):
        """predict_text() of every alignment: predict_many, then one formatter call per group -> a list of (values, text record),
        each the lone call's bits and bytes."""
        seqs = list(seqs)
        letters = [None] * len(seqs) if letters is None else list(letters)
        if len(letters) != len(seqs):
            raise ValueError(f"RSAEnsemble: {len(letters)} letter rows for {len(seqs)} sequences")
        values = self.predict_many(embs, seqs)
        return list(zip(values, table_text_many(values, [_letters_for(s, l, v.device) for s, l, v in zip(seqs, letters, values)])))


# ---------------------------------------------------------------------- loading an upstream model directory
class _Inert(nn.Module):
    """Stand-in for an upstream module class inside a pickled whole model: it receives the pickled attributes (parameters,
    buffers, submodules) and nothing else; no upstream code runs.  Only state_dict() is ever called on it."""


_STANDINS = {("model._0811.model_entry", "FrameModel"), ("model._0811.model_entry", "WrapLayers"),
             ("model._0713.resnet", "BasicBlock"), ("model._0713.mingpt", "Block"), ("model._0713.mingpt", "SelfAttention")}
_TORCH_PREFIXES = ("torch._utils", "torch.nn.", "torch._tensor", "torch.storage", "torch.serialization")


class _RestrictedUnpickler(pickle.Unpickler):
    """Admits the five upstream classes (as inert stand-ins), torch's own tensor / storage / nn.Module names and
    collections.OrderedDict; any other global is refused before it is looked up."""

    def find_class(self, module: str, name: str):
        if (module, name) in _STANDINS:
            return _Inert
        if (module, name) in (("collections", "OrderedDict"), ("builtins", "set"), ("__builtin__", "set")):
            return super().find_class(module, name)
        if module == "torch" or module.startswith(_TORCH_PREFIXES):
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"refused global {module}.{name}: an RSA checkpoint may name only torch / collections "
                                     f"classes and the reference's five model classes")


def _restricted_load(f, **kwargs):
    return _RestrictedUnpickler(f, **kwargs).load()


_pickle_module = types.ModuleType("rnamsm._rsa_restricted_pickle")
_pickle_module.Unpickler = _RestrictedUnpickler
_pickle_module.load = _restricted_load
_pickle_module.UnpicklingError = pickle.UnpicklingError


def load_state(path: Union[str, Path]) -> Dict[str, torch.Tensor]:
    """One `model_pcc_*.pt`: a plain state_dict, or upstream's pickled whole FrameModel (opened with the restricted unpickler:
    only its state is taken)."""
    try:
        obj = torch.load(str(path), map_location="cpu", pickle_module=_pickle_module, weights_only=False)
    except pickle.UnpicklingError as e:
        raise _lib.RnamsmError(f"{path}: {e}") from None
    if isinstance(obj, nn.Module):
        obj = obj.state_dict()
    if not isinstance(obj, dict) or not all(isinstance(v, torch.Tensor) for v in obj.values()):
        raise _lib.RnamsmError(f"{path}: neither a state_dict nor a pickled model")
    return {k: v.detach() for k, v in obj.items()}


def _load_stats(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """statistic_dict*.pickle: a dict of numpy arrays / scalars; 'mu' and 'std' are taken.  numpy's array reconstruction is all
    the pickle may name."""

    class _NumpyOnly(pickle.Unpickler):
        def find_class(self, module: str, name: str):
            if module.split(".")[0] == "numpy" and name in ("_reconstruct", "ndarray", "dtype", "scalar", "_frombuffer"):
                return super().find_class(module, name)
            raise pickle.UnpicklingError(f"refused global {module}.{name} in {path}")

    with open(path, "rb") as f:
        try:
            d = _NumpyOnly(f).load()
        except pickle.UnpicklingError as e:
            raise _lib.RnamsmError(str(e)) from None
    return np.asarray(d["mu"]), np.asarray(d["std"])


def load_ensemble(model_dir: Union[str, Path], device) -> RSAEnsemble:
    """An upstream model directory (models/OH+RNA-MSM_Emb or models/RNA-MSM_Emb) -> an RSAEnsemble on `device`:
    `model_pcc_*.pt` in SORTED order (the reference takes glob's order, which the file system decides), statistics from
    statistic_dict_oh.pickle + statistic_dict_emb.pickle, or statistic_dict.pickle (embedding only)."""
    model_dir = str(model_dir)
    paths = sorted(glob.glob(os.path.join(glob.escape(model_dir), "model_pcc_*.pt")))
    if not paths:
        raise _lib.RnamsmError(f"{model_dir}: no model_pcc_*.pt")
    members = [RSAPredictor.from_state_dict(load_state(p)) for p in paths]
    stats = {}
    for key, fname in (("oh", "statistic_dict_oh.pickle"), ("emb", "statistic_dict_emb.pickle"), ("emb", "statistic_dict.pickle")):
        p = os.path.join(model_dir, fname)
        if os.path.isfile(p) and key not in stats:
            stats[key] = _load_stats(p)
    ens = RSAEnsemble(members, stats, names=[os.path.basename(p) for p in paths])
    return ens.eval().to(device)


# ---------------------------------------------------------------------- the tables' text on the device (rnamsm_rsa_text)
def _letters_for(seq, letters, device) -> torch.Tensor:
    if letters is None:
        if not isinstance(seq, str):
            raise ValueError("RSAEnsemble: letters are needed where the sequence is given as base codes")
        letters = letter_codes(seq)
    return torch.as_tensor(letters).reshape(-1).to(device=device, dtype=torch.uint8)


def table_text(values: torch.Tensor, letters: torch.Tensor):
    """The bodies of the K member tables and the ensemble table for the [K, L] RSA `values` on the HIP device; letters uint8 [L] on
    the device -> (text uint8 [(K + 1) x 23 L], counts int32 [K + 3], ens float64 [2, L]): body f starts at f x 23 L and has
    counts[f] bytes -- the lines np.savetxt writes in write_rsa_files, byte for byte; counts[K + 1] is the fallback word (1: a value
    outside [0, 1] or a letter outside ACGUT -- the text is not to be used and write_rsa_files takes the host path), counts[K + 2]
    the zero word (1: an ASA of exactly 0, where write_rsa_files raises); ens: the ensemble's (ASA, RSA) write_rsa_files returns."""
    return ops.rsa_text(values, letters)


def table_text_long(values: torch.Tensor, letters: torch.Tensor):
    """table_text() for L up to LONG_MAX_L (rnamsm_rsa_text_long): the same record, the host writer's bytes for every L in range."""
    return ops.rsa_text_long(values, letters)


def table_text_many(values: Sequence[torch.Tensor], letters: Sequence[torch.Tensor]):
    """table_text() of every (values[b], letters[b]) in as few calls as the batch limit allows; each result is the lone call's."""
    values, letters = list(values), list(letters)
    if len(values) != len(letters):
        raise ValueError(f"table_text_many: {len(values)} value tables for {len(letters)} letter rows")
    out = []
    for i in range(0, len(values), _lib.RSA_MAX_BATCH):
        out += ops.rsa_text_packed(values[i:i + _lib.RSA_MAX_BATCH], letters[i:i + _lib.RSA_MAX_BATCH])
    return out


# ---------------------------------------------------------------------- host arithmetic and text files (predict.py)
def _save_single(name: str, seq: str, rsa: Optional[np.ndarray], out_dir: str, des: str, rng, asa: Optional[np.ndarray] = None):
    """doSavePredict_single: ASA = RSA x the per-base scale in float64 (or RSA = ASA / scale when the ASA is given), one text file."""
    os.makedirs(out_dir, exist_ok=True)
    sequence = re.sub(r"[T]", "U", "".join(seq))
    sequence = re.sub(r"[^AGCU]", _BASES[rng.randint(0, 3)], sequence)        # ONE draw per call, whether or not anything matches
    scale = np.array([ASA_SCALE[c] for c in sequence])
    if asa is None:
        asa = np.multiply(rsa, scale).T
    else:
        rsa = asa / scale
    if len(asa[asa == 0]):
        raise _lib.RnamsmError(f"error in predict\t {name},{seq}")
    idx = np.array([i + 1 for i in range(len(seq))])[None, :]
    nts = np.array([c for c in seq])[None, :]
    rows = np.vstack((np.char.mod("%d", idx), nts, np.char.mod("%.2f", asa), np.char.mod("%.3f", rsa))).T
    np.savetxt(os.path.join(out_dir, f"{name}.txt"), rows, delimiter="\t\t", fmt="%s",
               header=f"#{des}\n#index\t\tnt\t\tASA\t\tRSA\n", comments="")
    return asa, rsa


def _table_dirs(out: str, name: str, model_names: Sequence[str]):
    """(directory, description) of every table, the members' and then the ensemble's."""
    return ([(os.path.join(out, f"{name}_{i}"), f"{name} predict by {m}\n") for i, m in enumerate(model_names)]
            + [(os.path.join(out, f"{name}_ensemble"), f"{name} predict by ensemble model\n")])


def _tables_from_bodies(out: str, name: str, model_names: Sequence[str], bodies, rng) -> None:
    """The K + 1 files from device-made bodies: the header np.savetxt writes (it ends the header with a newline of its own) and one
    binary write each.  One draw per table all the same: the host path draws whether or not a letter is replaced, and a later
    alignment's replacements must not move."""
    for (out_dir, des), body in zip(_table_dirs(out, name, model_names), bodies):
        os.makedirs(out_dir, exist_ok=True)
        rng.randint(0, 3)
        with open(os.path.join(out_dir, f"{name}.txt"), "wb") as f:
            f.write(f"#{des}\n#index\t\tnt\t\tASA\t\tRSA\n\n".encode("ascii"))
            f.write(body)


def write_rsa_files(rsa_k: np.ndarray, seq: str, name: str, output_dir: Union[str, Path], model_names: Sequence[str],
                    rng, text=None) -> Tuple[np.ndarray, np.ndarray]:
    """`<output_dir>/RSA_result/<name>_<i>/<name>.txt` for every member and `.../<name>_ensemble/<name>.txt`, as the reference
    writes them (ensemble: mean of the members' ASA, RSA = ASA / scale); returns the ensemble's (ASA, RSA), float64 [L].
    rsa_k: [K, L] float32, the members' RSA.  rng: `random` (the module, seeded 2022 by the reference's program) or a
    random.Random: K + 1 draws are taken from it.  An ASA of exactly 0 raises RnamsmError where the reference exits.
    text: the results of table_text(rsa_k, letters), on the host -- (text, counts, ens).  With its fallback word and its zero word
    both 0 every file is a header and one binary write of its body; otherwise (and for a name np.savetxt would not write as ASCII)
    the host arithmetic and np.savetxt run as before -- the same bytes, the same K + 1 draws and the same error either way."""
    rsa_k = np.asarray(rsa_k, dtype=np.float32)
    seq = str(seq)
    if rsa_k.ndim != 2 or rsa_k.shape[1] != len(seq) or rsa_k.shape[0] != len(model_names):
        raise ValueError(f"write_rsa_files: RSA of shape {rsa_k.shape} for {len(model_names)} models and a sequence of length {len(seq)}")
    out = os.path.join(str(output_dir), "RSA_result")
    if text is not None and name.isascii() and all(str(m).isascii() for m in model_names):
        body, counts, ens = text
        K, L = rsa_k.shape
        counts = np.asarray(counts).reshape(-1)
        if counts.shape[0] != K + 3:
            raise ValueError(f"write_rsa_files: {counts.shape[0]} counts for {K} models, not {K + 3}")
        if not int(counts[K + 1]) and not int(counts[K + 2]):
            body = memoryview(body if isinstance(body, (bytes, bytearray)) else np.ascontiguousarray(body, dtype=np.uint8))
            bound = _lib.RSA_TEXT_LINE_MAX * L
            ens = np.asarray(ens, dtype=np.float64)
            if body.nbytes != (K + 1) * bound or ens.shape != (2, L):
                raise ValueError(f"write_rsa_files: a text of {body.nbytes} bytes and an ensemble of shape {ens.shape} for {K} models "
                                 f"and a sequence of length {L}")
            if any(not 0 < int(n) <= bound for n in counts[:K + 1]):
                raise ValueError(f"write_rsa_files: body counts {counts[:K + 1].tolist()} outside (0, {bound}]")
            os.makedirs(out, exist_ok=True)
            _tables_from_bodies(out, name, model_names, [body[f * bound:f * bound + int(counts[f])] for f in range(K + 1)], rng)
            return ens[0], ens[1]
    os.makedirs(out, exist_ok=True)
    asas = []
    for i, model_name in enumerate(model_names):
        asa, _ = _save_single(name, seq, rsa_k[i], os.path.join(out, f"{name}_{i}"), f"{name} predict by {model_name}\n", rng)
        asas.append(asa)
    mean = np.array(asas).mean(0)
    return _save_single(name, seq, None, os.path.join(out, f"{name}_ensemble"), f"{name} predict by ensemble model\n", rng, asa=mean)


# ---------------------------------------------------------------------- the head in the CLI (rnamsm.inference.extract_feat)
class _Draws:
    """The draws of one alignment's tables, taken ahead of time and handed out again in order (the `rng` of write_rsa_files)."""

    def __init__(self, draws):
        self._draws = list(draws)

    def randint(self, a: int, b: int) -> int:
        return self._draws.pop(0)


class RSAResult(NamedTuple):
    """One alignment's results of the RSA ensemble, on the device (or, on the writer's side, their host copies)."""
    values: torch.Tensor                          # [K, L] the members' RSA
    tokens: torch.Tensor                          # [L] the query's tokens
    text: Optional[tuple] = None                  # table_text(values, letters): (text, counts, ens); None where the formatter is off


class RSAHead:
    """data.rsa_model_dir in the CLI: the ensemble, the two look-up tables indexed by token (base codes; the letters the tables
    print), the members' names, the generator the texts draw from (the reference program's seed, 2022; drawn from as the writer
    jobs are made, in delivery order) and the switch text_on (data.rsa_text_device: the tables' bodies are formatted on the device)."""

    def __init__(self, model: Optional[RSAEnsemble], alphabet, base_lut: Optional[torch.Tensor], rng, model_names: Optional[Sequence[str]] = None,
                 *, text_on: bool = False, device=None):
        self.model, self.base_lut, self.rng, self.text_on = model, base_lut, rng, bool(text_on)
        self.model_names = list(model_names if model_names is not None else model.model_names)
        self.all_toks = list(alphabet.all_toks)
        if device is None:
            device = base_lut.device if base_lut is not None else "cpu"
        # a token that is no single ASCII character is 0: no letter of the domain, so that alignment's tables come from the host
        self.letters_lut = torch.tensor([ord(t) if len(t) == 1 and ord(t) < 128 else 0 for t in self.all_toks],
                                        dtype=torch.uint8).to(device) if self.text_on else None
        self.n_tensors = 2 + 3 * self.text_on

    def _one(self, emb: torch.Tensor, atp: torch.Tensor, tokens: torch.Tensor, long: bool) -> RSAResult:
        predict, text = (self.model.predict_long, table_text_long) if long else (self.model.predict, table_text)
        values = predict(emb, self.base_lut[tokens])
        return RSAResult(values, tokens, tuple(text(values, self.letters_lut[tokens])) if self.text_on else None)

    def one(self, emb: torch.Tensor, atp: torch.Tensor, tokens: torch.Tensor) -> RSAResult:
        """A lone alignment through the lone head; emb is read where it lies (atp is not read: the heads share one signature).  The
        formatter runs behind the head."""
        return self._one(emb, atp, tokens, False)

    def one_long(self, emb: torch.Tensor, atp: torch.Tensor, tokens: torch.Tensor) -> RSAResult:
        """one() on the stitched embedding of a long alignment (data.long_heads=stitched), L up to LONG_MAX_L: the same record through
        the long entry points; with the formatter off the tables are left to the host writer, which has no length limit."""
        return self._one(emb, atp, tokens, True)

    def stitched_route(self, L: int, long_on: bool):
        """On a stitched alignment of L body columns: the method that runs this head, or the reason (a str) it is skipped."""
        why = long_refusal(L, long_on)
        return self.one_long if why is None else why

    def many(self, embs: Sequence[torch.Tensor], atps: Sequence[torch.Tensor], tokens: Sequence[torch.Tensor]) -> List[RSAResult]:
        """A group in one launch set per stage (predict_many, table_text_many): every member's record holds the bits and bytes of
        one()."""
        values = self.model.predict_many(embs, [self.base_lut[t] for t in tokens])
        texts = table_text_many(values, [self.letters_lut[t] for t in tokens]) if self.text_on else [None] * len(values)
        return [RSAResult(v, t, None if tx is None else tuple(tx)) for v, t, tx in zip(values, tokens, texts)]

    def flatten(self, rec: RSAResult) -> list:
        return [rec.values, rec.tokens, *(rec.text or ())]

    def unflatten(self, tensors: Sequence) -> RSAResult:
        """The record of flatten()'s list (n_tensors entries), by this head's switch."""
        if len(tensors) != self.n_tensors:
            raise ValueError(f"RSAHead: {len(tensors)} tensors for a record of {self.n_tensors}")
        return RSAResult(tensors[0], tensors[1], tuple(tensors[2:5]) if self.text_on else None)

    def writer_job(self, rec: RSAResult, name: str, output_dir):
        """-> (write, tensors): write(*host copies of tensors) writes <output_dir>/RSA_result/<name>_*/<name>.txt through
        write_rsa_files.  The tensors are the query's tokens and the values, then the text record where there is one: with its two
        flag words clear the files are its bodies behind their headers, otherwise the host path formats the values as before.
        The alignment's K + 1 draws are taken here, when the job is made -- in delivery order -- and handed to write(): the writer's
        worker threads run the jobs of neighbouring alignments at the same time, and drawing there would let the order of the draws,
        and with it the base a letter outside ACGUT is replaced by, depend on their timing."""
        draws = _Draws(self.rng.randint(0, 3) for _ in range(len(self.model_names) + 1))

        def write(tokens, values, *text) -> None:
            write_rsa_files(values, "".join(self.all_toks[int(t)] for t in tokens), name, output_dir, self.model_names, draws,
                            text=text or None)

        return write, (rec.tokens, rec.values, *(rec.text or ()))
