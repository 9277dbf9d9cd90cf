"""Structured configuration with hydra-style `group.key=value` overrides.

The reference's CLI is a hydra app over dataclasses (RNA_MSM_Inference.py:20-87); hydra / omegaconf are not
available here, so this is a small dotted-override parser over equivalent dataclasses with the same group
names, keys and defaults.
"""
from __future__ import annotations

import dataclasses
import re
from dataclasses import dataclass, field
from fractions import Fraction
from pathlib import Path
from typing import List, Tuple

from ._lib import SS_GEMM_DTYPES        # data.ss_gemm_dtype

LM_SCORES_MODES = ("", "wt", "masked")   # data.lm_scores
LONG_MSA_MODES = ("crop", "windows")     # data.long_msa
LONG_HEADS_MODES = ("skip", "stitched")  # data.long_heads


def check_ss_gemm_dtype(value: str) -> str:
    if value not in SS_GEMM_DTYPES:
        raise ValueError(f"data.ss_gemm_dtype={value!r} is not one of {', '.join(SS_GEMM_DTYPES)}")
    return value


def check_ss_nested(value, threshold, min_loop, ss_model_path: str) -> bool:
    """data.ss_nested / data.ss_nested_threshold / data.ss_nested_min_loop (rnamsm_ss_nested's ranges)."""
    from ._lib import SS_NESTED_MAX_LOOP
    if not isinstance(value, bool):
        raise ValueError(f"data.ss_nested={value!r} is not one of false, true")
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0.0 <= float(threshold) < 1.0:
        raise ValueError(f"data.ss_nested_threshold={threshold!r} is not a number in [0, 1)")
    if isinstance(min_loop, bool) or not isinstance(min_loop, int) or not 0 <= min_loop <= SS_NESTED_MAX_LOOP:
        raise ValueError(f"data.ss_nested_min_loop={min_loop!r} is not an integer in [0, {SS_NESTED_MAX_LOOP}]")
    if value and not ss_model_path:
        raise ValueError("data.ss_nested=true needs data.ss_model_path: the nested structure is decoded from the SS head's probabilities")
    return value


def check_lm_scores(value: str) -> str:
    if value not in LM_SCORES_MODES:
        raise ValueError(f"data.lm_scores={value!r} is not one of {', '.join(repr(m) for m in LM_SCORES_MODES)}")
    return value


def check_long_msa(value: str) -> str:
    if value not in LONG_MSA_MODES:
        raise ValueError(f"data.long_msa={value!r} is not one of {', '.join(repr(m) for m in LONG_MSA_MODES)}")
    return value


def check_long_heads(value: str) -> str:
    if value not in LONG_HEADS_MODES:
        raise ValueError(f"data.long_heads={value!r} is not one of {', '.join(repr(m) for m in LONG_HEADS_MODES)}")
    return value


def check_invcov(value) -> bool:
    if not isinstance(value, bool):
        raise ValueError(f"data.invcov={value!r} is not one of false, true")
    return value


def check_msa_stats(value) -> bool:
    if not isinstance(value, bool):
        raise ValueError(f"data.msa_stats={value!r} is not one of false, true")
    return value


MI_GAPS_MODES = ("pairwise", "state")


def check_mi(value) -> bool:
    if not isinstance(value, bool):
        raise ValueError(f"data.mi={value!r} is not one of false, true")
    return value


def check_mi_gaps(value: str) -> str:
    if value not in MI_GAPS_MODES:
        raise ValueError(f"data.mi_gaps={value!r} is not one of {', '.join(repr(m) for m in MI_GAPS_MODES)}")
    return value


MI_WEIGHTS_MODES = ("none", "seqid")


def check_mi_weights(value: str, mi_on: bool = True) -> str:
    """data.mi_weights; "seqid" reweights data.mi's maps, so it is refused where data.mi is off."""
    if value not in MI_WEIGHTS_MODES:
        raise ValueError(f"data.mi_weights={value!r} is not one of {', '.join(repr(m) for m in MI_WEIGHTS_MODES)}")
    if value != "none" and not mi_on:
        raise ValueError(f"data.mi_weights={value!r} needs data.mi=true: it reweights the maps that key writes")
    return value


def parse_top_pairs_spec(spec):
    """A ranked-pair list's length as a string -> (count, None) for "N", an integer >= 1, or (None, Fraction x) for "<x>L", x > 0 a
    plain decimal read exactly (fractions.Fraction of the string: no float arithmetic)."""
    if not isinstance(spec, str):
        raise ValueError(f"top_pairs spec {spec!r} is not a string")
    text = spec.strip()
    if re.fullmatch(r"[0-9]+", text):
        if int(text) < 1:
            raise ValueError(f"top_pairs spec {spec!r}: the count is below 1")
        return int(text), None
    m = re.fullmatch(r"([0-9]+(?:\.[0-9]*)?|\.[0-9]+)L", text)
    if not m:
        raise ValueError(f"top_pairs spec {spec!r} is neither a positive integer nor a positive decimal multiple of L such as 1.5L")
    x = Fraction(m.group(1))
    if x <= 0:
        raise ValueError(f"top_pairs spec {spec!r}: the multiple of L is not positive")
    return None, x


TOP_PAIRS_MAX_SEP = 32768


def check_top_pairs(value, min_sep=1) -> Tuple[str, int]:
    """data.top_pairs ("" = off, else a spec: "N" or "<x>L") and data.top_pairs_min_sep; the message names the key."""
    if not isinstance(value, str):
        raise ValueError(f"data.top_pairs={value!r} is not a string (\"\" = off, a count such as 100, or a multiple of L such as 1.5L)")
    if value != "":
        try:
            parse_top_pairs_spec(value)
        except ValueError as e:
            raise ValueError(f"data.top_pairs={value!r}: {e}") from None
    if isinstance(min_sep, bool) or not isinstance(min_sep, int):
        raise ValueError(f"data.top_pairs_min_sep={min_sep!r} is not an integer")
    if not 1 <= min_sep <= TOP_PAIRS_MAX_SEP:
        raise ValueError(f"data.top_pairs_min_sep={min_sep} outside [1, {TOP_PAIRS_MAX_SEP}]")
    return value, min_sep


def check_target_dir(value, min_sep=1) -> Tuple[str, int]:
    """data.target_dir ("" = off, else a directory of known structures) and data.target_min_sep; the message names the key.  Whether
    the directory exists is looked at when the run starts, not here."""
    if not isinstance(value, str):
        raise ValueError(f"data.target_dir={value!r} is not a string (\"\" = off, else a directory of <id>.bpseq / .ct / .npy targets)")
    if isinstance(min_sep, bool) or not isinstance(min_sep, int):
        raise ValueError(f"data.target_min_sep={min_sep!r} is not an integer")
    if not 1 <= min_sep <= TOP_PAIRS_MAX_SEP:
        raise ValueError(f"data.target_min_sep={min_sep} outside [1, {TOP_PAIRS_MAX_SEP}]")
    return value, min_sep


def check_filter_seqid(min_seqid, max_seqid, step) -> Tuple[int, int, int]:
    """data.filter_min_seqid / data.filter_max_seqid / data.filter_step (sample_method=seqid-filter); the message names the key."""
    for key, value in (("filter_min_seqid", min_seqid), ("filter_max_seqid", max_seqid), ("filter_step", step)):
        if isinstance(value, bool) or not isinstance(value, int):
            raise ValueError(f"data.{key}={value!r} is not an integer")
    if min_seqid < 1:
        raise ValueError(f"data.filter_min_seqid={min_seqid} is below 1")
    if not 1 <= max_seqid <= 100:
        raise ValueError(f"data.filter_max_seqid={max_seqid} outside [1, 100]")
    if step < 1:
        raise ValueError(f"data.filter_step={step} is below 1")
    return min_seqid, max_seqid, step


@dataclass
class DataConfig:                       # RNA_MSM_Inference.py:20-32
    device: str = "cuda"
    root_path: str = "."
    MSA_path: str = "results"
    MSA_list: str = "rna_id.txt"
    model_path: str = "pretrained/RNA_MSM_pretrained.ckpt"
    num_workers: int = 3
    architecture: str = "rna language"
    max_seqlen: int = 1024
    max_tokens: int = 16384
    max_seqs_per_msa: int = 512
    sample_method: str = "hhfilter"
    # (the name is not checked here: rnamsm.msa.load_msa_tokens refuses an unknown one, and the reference's default, hhfilter, where
    # an alignment is deeper than max_seqs_per_msa -- that external binary is not part of this project.)
    # extra (not in the reference): sample_method=seqid-filter, this project's own identity redundancy filter
    # (rnamsm.msa.seqid_filter; on the device rnamsm_seqid_filter).  It is modelled on what the reference asks of hhfilter
    # (-id 90 -diff max_seqs_per_msa) and is NOT that binary's selection: it counts identity over the whole alignment, hhfilter's
    # -diff per window of 50 columns with a threshold schedule of its own.  Passes at filter_min_seqid, + filter_step, ..., up to
    # filter_max_seqid (per cent) until max_seqs_per_msa rows are kept, then the first max_seqs_per_msa of them.  The keys are read by
    # that method only; min >= 1, 1 <= max <= 100, step >= 1.
    filter_min_seqid: int = 20
    filter_max_seqid: int = 90
    filter_step: int = 5
    # extra (not in the reference): the small alignments (<= 16384 tokens each; 8192 in bf16) of the id list share launch sets
    # (MSATransformer.forward_ragged).  On by default since round 3: a lone forward of a few hundred tokens costs 2.5 ms on a mostly
    # idle chip; data.batch_small_msas=false restores the strictly one-by-one loop of the reference (RNA_MSM_Inference.py:141-148)
    batch_small_msas: bool = True
    # (round 3's framed ragged batches in a 16-bit mode, on request only; the default route below needs no opt-in)
    batch_small_msas_16bit: bool = False
    # round 4: the groups are TOKEN-PACKED -- back to back on the token axis, nothing padded (rnamsm_forward_packed) -- instead of
    # padded into a frame; false = the framed ragged batch of round 3 (A/B, tools/cli_throughput.py).  Round 5: in exact mode an
    # alignment's files are BYTE FOR BYTE those of the one-by-one loop, whatever else is in the list (one arithmetic per alignment:
    # tests/test_gpu_cli.py); in a 16-bit mode (model.gemm_dtype = bf16 | f16x3) the packed batch runs in that mode too (Linear
    # layers on the 16-bit matrix cores, attention on the exact kernels), a lone small alignment as a packed batch of one, so an
    # alignment's files depend on its company at fp32-accumulation rounding at most (which GEMM tile the batch's token count selects)
    pack_small_msas: bool = True
    # extra (not in the reference): "" = off; else the RNA-MSM-SS weights (the reference's model/rna-msm_attention.pt): the
    # secondary-structure head (rnamsm.ss) then runs on every alignment's attention maps where they lie on the device, and
    # SS_result/<id>.{ct,bpseq,prob} are written next to the .npy files (_downstream_tasks/SS/predict.py's files; the sequence
    # is row 0 of the tokens the forward ran on, so a T of the alignment reads as U there)
    ss_model_path: str = ""
    # with the SS head on: SS_result/<id>.prob is formatted on the device (rnamsm_ss_prob_text) and written as one block; false =
    # np.savetxt on the writer thread, as before.  The same bytes either way.
    ss_prob_text: bool = True
    # with the SS head on: the base pairs are decoded and the bodies of SS_result/<id>.ct / .bpseq written on the device
    # (rnamsm_ss_pairs); with ss_prob_text on as well the [L, L] probabilities never reach the host.  false = secondary_structure and
    # np.savetxt on the writer thread, as before.  The same bytes either way.
    ss_pairs_device: bool = True
    # with the SS head on: the arithmetic of its convolutions -- f32 (exact, default) | bf16 (rnamsm_ss_head16: bf16 operands on
    # the matrix cores; accumulation, residual image and LayerNorm stay fp32).  Its own key: it does NOT follow model.gemm_dtype.
    ss_gemm_dtype: str = "f32"
    # with the SS head on: also decode the NESTED (pseudoknot-free) structure of greatest summed pair probability above
    # ss_nested_threshold, hairpin loops of at least ss_nested_min_loop bases, on the device (rnamsm_ss_nested), and write
    # SS_result/<id>.dbn (dot-bracket), <id>.nested.ct and <id>.nested.bpseq beside the reference's files, which stay as they are
    ss_nested: bool = False
    ss_nested_threshold: float = 0.516
    ss_nested_min_loop: int = 3
    # extra (not in the reference): "" = off; else an RSA model directory of the reference (_downstream_tasks/RSA/models/OH+RNA-MSM_Emb:
    # model_pcc_*.pt and the statistic_dict*.pickle files): the solvent-accessibility ensemble (rnamsm.rsa) then runs on every
    # alignment's embedding where it lies on the device, and RSA_result/<id>_<k>/<id>.txt, RSA_result/<id>_ensemble/<id>.txt are
    # written next to the .npy files (_downstream_tasks/RSA/predict.py's files, without the plots)
    rsa_model_dir: str = ""
    # with the RSA head on: the K + 1 tables of RSA_result are computed (float64) and formatted on the device (rnamsm_rsa_text) and
    # written as a header and one block each; false = the host arithmetic and np.savetxt on the writer thread, as before.  The same
    # bytes either way; an alignment with a letter outside ACGUT in its query takes the host path by itself.
    rsa_text_device: bool = True
    # extra (not in the reference): the contact head (contact_head.regression.* of the checkpoint that is loaded anyway: symmetrize
    # + APC + logistic regression on the row attentions, rnamsm.contacts) then runs on every alignment's atp where it lies on the
    # device, and <id>_contacts.npy, (L, L) float32, is written next to <id>_emb.npy / <id>_atp.npy
    contacts: bool = False
    # extra (not in the reference's CLI; its utils/likelihood.py): "" = off; "wt" = the LM head (lm_head.* of the checkpoint that is
    # loaded anyway, rnamsm.lm) on every alignment's emb where it lies, unmasked marginals, no further forward; "masked" = the masked
    # pseudo-likelihood scan (rnamsm.likelihood.scan): one further forward per query position.  <id>_lm_scores.npy, (L, V) float32,
    # log p(token) - log p(wild type) per query position, and <id>_lm_nll.npy, (L,) float32, are written next to <id>_emb.npy;
    # log-probabilities are scores - nll[:, None], the pseudo-perplexity exp(mean(nll))
    lm_scores: str = ""
    # extra (not in the reference): an alignment wider than max_seqlen - 1 columns.  "crop" (default) = the reference's random crop
    # (RandomCropDataset, dataset.py:142-158: <cls> and one random window; the same draws, the same files).  "windows" = nothing is
    # cropped or drawn: the alignment runs as overlapping windows of max_seqlen - 1 columns whose outputs are blended on the device
    # (MSATransformer.forward_windows), and <id>_emb.npy / <id>_atp.npy hold the FULL (L, 768) / (120, L, L).  On such an alignment
    # lm_scores=wt runs on the stitched emb; the SS, RSA and contact heads and lm_scores=masked are skipped with one printed line (data.long_heads below lets the SS, RSA and contact heads through).
    long_msa: str = "crop"
    # with long_msa=windows: the distance between window starts, within [ceil(W / 2), W] for W = max_seqlen - 1; 0 = ceil(W / 2)
    window_stride: int = 0
    # with long_msa=windows: what the downstream heads do on a stitched alignment.  "skip" (default) = as before, one printed line per
    # head.  "stitched" = the contact head and the SS head (exact fp32 only) run on the stitched atp and the RSA head on the stitched
    # emb through the long entry points (rnamsm_contact_head_long, rnamsm_ss_head_long, rnamsm_ss_prob_text_long,
    # rnamsm_ss_pairs_long, rnamsm_rsa_head_long, rnamsm_rsa_text_long) for L up to 4096 and write their usual files at the full L;
    # lm_scores=masked, an SS head under ss_gemm_dtype=bf16 and any longer alignment
    # stay skipped, each with a line that names the reason.  Alignments that are not stitched are untouched by the key.
    long_heads: str = "skip"
    # extra (not in the reference's CLI; its utils/align.py MSA.invcov): the covariance contact map of the alignment AS READ -- every
    # row, before row sub-sampling, and every column, whatever max_seqlen, long_msa and long_heads say -- computed on the device
    # (rnamsm.msa.msa_invcov) and written as <id>_invcov.npy, (L, L) float64, next to <id>_emb.npy.  An alignment the kernel refuses
    # (more than 4096 columns, more than 16 distinct non-gap tokens, fewer than 2 rows) gets one printed line and its other files.
    invcov: bool = False
    # extra (not in the reference's CLI; its utils/align.py MSA.weights, MSA.neff and coverage): the statistics of the alignment AS
    # READ -- every row, before row sub-sampling, and every column -- computed on the device (rnamsm_msa_neff, rnamsm_msa_coverage):
    # <id>_weights.npy, (N,) float64, the sequence weights at a normalised Hamming cutoff of 0.2 (the reference's seqid_cutoff
    # default), and <id>_coverage.npy, (L,) float64, next to <id>_emb.npy, and one printed line with N, L, Neff, Neff / sqrt(L) and
    # Neff / L.  An alignment the kernels refuse (more than 32768 columns, more than 2^20 rows) gets one printed line and its other
    # files.
    msa_stats: bool = False
    # extra (not in the reference's CLI): the mutual-information contacts of the alignment AS READ -- every row, before row
    # sub-sampling, and every column, like data.invcov -- computed on the device (rnamsm.msa.msa_mi) and written as <id>_mi.npy, the
    # mutual information of every pair of columns, and <id>_mip.npy, its average-product correction (the reference's apc,
    # utils/tensor.py:103-113, of the map with a zero diagonal), (L, L) float64 each, next to <id>_emb.npy.  mi_gaps: "pairwise" = rows
    # with a gap in either column are left out of that pair; "state" = the gap is one more state.  An alignment the kernel refuses (as
    # for data.invcov) gets one printed line and its other files.
    mi: bool = False
    mi_gaps: str = "pairwise"
    # mi_weights: "none" = every row counts once (the two files above); "seqid" = row n counts MSA.weights[n] times (1 / the rows
    # within the normalised Hamming cutoff data.msa_stats uses; rnamsm.msa.msa_mi_weighted) and the maps are written as
    # <id>_wmi.npy and <id>_wmip.npy INSTEAD of the unweighted pair.  "seqid" needs data.mi=true; with data.msa_stats on as well the
    # weights are computed once.
    mi_weights: str = "none"
    # extra (not in the reference's CLI; the first step of its utils/metrics.py): "" = off; else the length of a ranked list of the
    # strongest pairs, "N" (a count) or "<x>L" (max(1, ceil(x * L)) for the L of the map at hand, x a decimal: 0.5L, 1.5L, 2L).  For
    # every pair map the run writes for an alignment -- contacts, invcov, mi / mip or wmi / wmip -- <id>_<map>_top.txt appears beside
    # it: a header line, then `i j score` per pair, 1-based, strongest first, equal scores by i then j, pairs with
    # j - i >= top_pairs_min_sep only (1 = every pair off the diagonal, the reference's minsep=0), NaN left out.  The lists are
    # selected and ranked on the device (rnamsm.contacts.top_pairs) from the map where it lies.  A map whose k exceeds 65536 or whose
    # L is below 2 gets one printed line instead; refused under RNAMSM_GATHER_TO_RANK0=1.
    top_pairs: str = ""
    top_pairs_min_sep: int = 1
    # extra (not in the reference's CLI; its utils/metrics.py rna_compute_precisions and compute_precisions): "" = off; else a
    # directory that holds the known structure of an alignment as <id>.bpseq, <id>.ct or <id>.npy (an integer [L, L] array; looked for
    # in that order).  <id>_metrics.json then appears beside the alignment's files: the threshold sweep (tp / fp / tn / fn at the 1001
    # thresholds and F1, PR, PR1, AUC) of the SS probability map, the decoded structure's precision / recall / F1, and P@L, P@L2, P@L5
    # and their AUC (k = L) for contacts and every other pair map the run writes -- counted on the device (rnamsm.ops.pair_sweep,
    # pair_precision) from the maps where they lie, pairs with j - i >= target_min_sep only.  metrics_summary.json at the end of the
    # list carries the summed sweep counts, their scores and the mean of each precision.  A missing target, a length mismatch or
    # L < 10 prints one line and leaves that entry out; refused under RNAMSM_GATHER_TO_RANK0=1.
    target_dir: str = ""
    target_min_sep: int = 1


@dataclass
class MSATransformerModelConfig:        # RNA_MSM_Inference.py:35-43
    embed_dim: int = 768
    num_attention_heads: int = 12
    num_layers: int = 10
    embed_positions_msa: bool = True
    dropout: float = 0.1
    attention_dropout: float = 0.1
    activation_dropout: float = 0.1
    # extra (not in the reference): arithmetic of the Linear GEMMs -- f32 (exact, default) | f16x3 | bf16
    gemm_dtype: str = "f32"


@dataclass
class OptimizerConfig:                  # RNA_MSM_Inference.py:46-54 (unused by inference, kept for key parity)
    name: str = "adam"
    learning_rate: float = 3e-4
    weight_decay: float = 3e-4
    lr_scheduler: str = "warmup_cosine"
    warmup_steps: int = 16000
    adam_betas: Tuple[float, float] = (0.9, 0.999)
    max_steps: int = 500000


@dataclass
class Config:
    data: DataConfig = field(default_factory=DataConfig)
    optimizer: OptimizerConfig = field(default_factory=OptimizerConfig)
    model: MSATransformerModelConfig = field(default_factory=MSATransformerModelConfig)


def _coerce(text: str, current):
    if isinstance(current, bool):
        if text.lower() in ("true", "1", "yes"):
            return True
        if text.lower() in ("false", "0", "no"):
            return False
        raise ValueError(f"expected a boolean, got {text!r}")
    if isinstance(current, int):
        return int(text)
    if isinstance(current, float):
        return float(text)
    if isinstance(current, tuple):
        parts = [p for p in text.strip("()[] ").split(",") if p.strip()]
        return tuple(float(p) for p in parts)
    return text


def parse_overrides(argv: List[str], cfg: Config = None) -> Config:
    """`data.MSA_path=results model.num_layers=10 ...`; unknown groups/keys and malformed tokens raise."""
    cfg = cfg or Config()
    for tok in argv:
        if "=" not in tok:
            raise ValueError(f"override {tok!r} is not of the form group.key=value")
        dotted, value = tok.split("=", 1)
        dotted = dotted.lstrip("+")
        parts = dotted.split(".")
        if len(parts) != 2:
            raise ValueError(f"override key {dotted!r} must be group.key")
        group, key = parts
        if not hasattr(cfg, group):
            raise KeyError(f"unknown config group {group!r} (have: data, model, optimizer)")
        node = getattr(cfg, group)
        names = {f.name for f in dataclasses.fields(node)}
        if key not in names:
            raise KeyError(f"unknown key {key!r} in group {group!r}")
        setattr(node, key, _coerce(value, getattr(node, key)))
    check_ss_gemm_dtype(cfg.data.ss_gemm_dtype)
    check_ss_nested(cfg.data.ss_nested, cfg.data.ss_nested_threshold, cfg.data.ss_nested_min_loop, cfg.data.ss_model_path)
    check_lm_scores(cfg.data.lm_scores)
    check_long_msa(cfg.data.long_msa)
    check_long_heads(cfg.data.long_heads)
    check_invcov(cfg.data.invcov)
    check_msa_stats(cfg.data.msa_stats)
    check_mi(cfg.data.mi)
    check_mi_gaps(cfg.data.mi_gaps)
    check_mi_weights(cfg.data.mi_weights, cfg.data.mi)
    check_filter_seqid(cfg.data.filter_min_seqid, cfg.data.filter_max_seqid, cfg.data.filter_step)
    check_top_pairs(cfg.data.top_pairs, cfg.data.top_pairs_min_sep)
    check_target_dir(cfg.data.target_dir, cfg.data.target_min_sep)
    return cfg
