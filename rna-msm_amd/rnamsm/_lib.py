"""ctypes binding of librnamsm_hip.so (include/rnamsm.h).

The library is the product: there is no CPU or eager-PyTorch fallback.  `load()` raises if the
shared object is missing, and every op wrapper raises if its tensors are not on a HIP device.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (load order: see rnamsm/__init__.py)
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RNAMSM_LIB_PATH") or os.path.join(_HERE, "librnamsm_hip.so")    # override: A/B builds only

RNAMSM_OK = 0
F32, BF16, F16X3 = 0, 1, 3        # (2 was "bf16x3", removed in round 5: include/rnamsm.h)
DTYPES = {"f32": F32, "bf16": BF16, "f16x3": F16X3}
ACT_NONE, ACT_GELU_ERF = 0, 1
OUT_REPR = 1

# index tables of rnamsm_forward's weight-pointer array (include/rnamsm.h)
W_GLOBAL = ("embed_tokens", "embed_positions", "row_pos", "ln_before_g", "ln_before_b", "ln_after_g", "ln_after_b")
W_LAYER = ("row_ln_g", "row_ln_b", "row_wqkv", "row_bqkv", "row_wo", "row_bo",
           "col_ln_g", "col_ln_b", "col_wqkv", "col_bqkv", "col_wo", "col_bo",
           "ffn_ln_g", "ffn_ln_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")

# index tables of rnamsm_ss_head's weight-pointer array (include/rnamsm.h): the reference state_dict's order
W_SS_STEM = ("conv1.weight", "conv1.bias", "bn1.weight", "bn1.bias")
W_SS_BLOCK = ("conv1.weight", "bn1.weight", "bn1.bias", "conv2.weight", "bn2.weight", "bn2.bias")
W_SS_HEAD = ("fc1.weight", "fc1.bias")
SS_GEMM_DTYPES = ("f32", "bf16")   # arithmetics of the SS head's convolutions: rnamsm_ss_head / rnamsm_ss_head16
SS_MAX_L = 1024
SS_MAX_BATCH = 1024
SS_TEXT_RECORD = 25                # bytes of one element of the .prob text: "%.18e" and its separator
SS_CT_LINE_MAX, SS_BPSEQ_LINE_MAX = 32, 12      # rnamsm_ss_struct_text_bytes: bytes of the longest .ct / .bpseq line at L = 1024
# rnamsm_ss_nested / _packed: the longest hairpin loop that may be asked for, and the defaults of the two parameters
SS_NESTED_MAX_LOOP, SS_NESTED_THETA, SS_NESTED_MIN_LOOP = 32, 0.516, 3

# index tables of rnamsm_rsa_head's weight-pointer array (include/rnamsm.h): four statistics, then 26 packed entries per member
W_RSA_GLOBAL = ("mu_emb", "std_emb", "mu_oh", "std_oh")
W_RSA_MODEL = ("stem", "bn1.scale", "bn1.shift", "shortcut.1.scale", "shortcut.1.shift", "conv2.weight", "bn2.scale", "bn2.shift",
               "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "ln1.weight", "ln1.bias", "attn.qkv.weight", "attn.qkv.bias",
               "attn.proj.weight", "attn.proj.bias", "ln2.weight", "ln2.bias", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight",
               "mlp.2.bias", "final.weight", "final.bias")
CONTACT_MAX_L = 1023               # rnamsm_contact_head_atp / _packed: the stripped maps of C <= 1024 columns
CONTACT_MAX_BATCH = 1024
RSA_MAX_L = 1024
RSA_MAX_MODELS = 8
RSA_MAX_BATCH = 1024
RSA_CIN_PAD = 800
RSA_TEXT_LINE_MAX = 23             # rnamsm_rsa_text_bytes: bytes of the longest line of an RSA_result table at L = 1024
# rnamsm_lm_head / _packed (include/rnamsm.h): D a multiple of 64 up to LM_MAX_D, V up to LM_MAX_V, the rows of a call up to LM_MAX_ROWS
LM_MAX_D, LM_MAX_V, LM_MAX_BATCH, LM_MAX_ROWS = 1024, 64, 1024, 1 << 24
W_LM = ("dense.weight", "dense.bias", "layer_norm.weight", "layer_norm.bias", "weight", "bias")     # the weight table's order
LM_OUTPUTS = ("logits", "logp", "scores", "nll")
STITCH_MAX_L, STITCH_MAX_H = 1 << 19, 1 << 16      # rnamsm_stitch_rows / _pairs
LONG_MAX_L = 4096                  # rnamsm_contact_head_long / _ss_head_long / _ss_prob_text_long / _ss_pairs_long / _rsa_head_long /
                                   # _rsa_text_long: a stitched alignment
# rnamsm_msa_invcov: rows, symbols, and the int32 header in front of the optional counts (K, then the symbols)
INVCOV_MAX_N, INVCOV_MAX_K, INVCOV_META = 1 << 20, 16, 32
# rnamsm_msa_mi: gap_mode by the name data.mi_gaps and ops.msa_mi take; rnamsm_apc_f64: the widest map
MI_GAP_MODES = {"pairwise": 0, "state": 1}
APC_MAX_L = 32768
# rnamsm_msa_pdist / _neff / _coverage: columns, rows of the matrix form, rows of the other two
PDIST_MAX_L, PDIST_MAX_N_MATRIX, PDIST_MAX_N = 32768, 16384, 1 << 20
# rnamsm_top_pairs_f64 / _f32: the widest map, the longest list, the largest separation
TOP_PAIRS_MAX_L, TOP_PAIRS_MAX_K, TOP_PAIRS_MAX_SEP = 32768, 65536, 32768
# rnamsm_pair_sweep_* / rnamsm_pair_precision_*: the longest threshold table, the most cuts (L, k and min_sep as top_pairs)
PAIR_SWEEP_MAX_T, PAIR_PRECISION_MAX_CUTS = 4096, 64


class ModelDims(ctypes.Structure):
    _fields_ = [("num_layers", c_int), ("embed_dim", c_int), ("num_heads", c_int), ("ffn_dim", c_int),
                ("vocab", c_int), ("num_positions", c_int), ("pad_idx", c_int), ("ln_eps", c_float),
                ("row_pos_dim", c_int)]          # 0 / 1: scalar per alignment row; embed_dim: the msm/ variant's per-channel rows


class SsItem(ctypes.Structure):
    """rnamsm_ss_item: one structure of an rnamsm_ss_head_packed batch (device pointers as integers)."""
    _fields_ = [("atp", c_void_p), ("atp_plane_stride", c_int64), ("base_codes", c_void_p), ("L", ctypes.c_int32),
                ("logits", c_void_p), ("probs", c_void_p)]


class SsTextItem(ctypes.Structure):
    """rnamsm_ss_text_item: one matrix of an rnamsm_ss_prob_text_packed batch (device pointers as integers)."""
    _fields_ = [("probs", c_void_p), ("L", ctypes.c_int32), ("text", c_void_p), ("fallback", c_void_p)]


class SsPairsItem(ctypes.Structure):
    """rnamsm_ss_pairs_item: one structure of an rnamsm_ss_pairs_packed batch (device pointers as integers)."""
    _fields_ = [("probs", c_void_p), ("letters", c_void_p), ("L", ctypes.c_int32), ("partner", c_void_p), ("counts", c_void_p),
                ("ct", c_void_p), ("bpseq", c_void_p)]


class SsNestedItem(ctypes.Structure):
    """rnamsm_ss_nested_item: one structure of an rnamsm_ss_nested_packed batch (device pointers as integers)."""
    _fields_ = [("probs", c_void_p), ("letters", c_void_p), ("L", ctypes.c_int32), ("partner", c_void_p), ("counts", c_void_p),
                ("ct", c_void_p), ("bpseq", c_void_p), ("dbn", c_void_p)]


class RsaItem(ctypes.Structure):
    """rnamsm_rsa_item: one alignment of an rnamsm_rsa_head_packed batch (device pointers as integers)."""
    _fields_ = [("emb", c_void_p), ("emb_row_stride", c_int64), ("base_codes", c_void_p), ("L", ctypes.c_int32),
                ("probs", c_void_p), ("logits", c_void_p)]


class ContactItem(ctypes.Structure):
    """rnamsm_contact_item: one alignment of an rnamsm_contact_head_packed batch (device pointers as integers)."""
    _fields_ = [("atp", c_void_p), ("plane_stride", c_int64), ("L", ctypes.c_int32), ("contacts", c_void_p)]


class LmItem(ctypes.Structure):
    """rnamsm_lm_item: one member of an rnamsm_lm_head / rnamsm_lm_head_packed call (device pointers as integers)."""
    _fields_ = [("x", c_void_p), ("ld", c_int64), ("rows", c_void_p), ("wt", c_void_p), ("n", ctypes.c_int32),
                ("logits", c_void_p), ("logp", c_void_p), ("scores", c_void_p), ("nll", c_void_p)]


class RsaTextItem(ctypes.Structure):
    """rnamsm_rsa_text_item: one alignment of an rnamsm_rsa_text_packed batch (device pointers as integers)."""
    _fields_ = [("rsa", c_void_p), ("letters", c_void_p), ("L", ctypes.c_int32), ("text", c_void_p), ("counts", c_void_p),
                ("ens", c_void_p)]


_SIGNATURES = {
    "rnamsm_version": (c_int, []),
    "rnamsm_last_error": (c_char_p, []),
    "rnamsm_device_count": (c_int, []),
    "rnamsm_embed_ln": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    "rnamsm_embed_ln_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                     c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    "rnamsm_layernorm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p]),
    "rnamsm_gemm_bias_act_res": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                         c_int64, c_int, c_int, c_int, c_float, c_int, c_void_p, c_int, c_void_p]),
    "rnamsm_gemm_row_scaled": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_float,
                                       c_int, c_void_p, c_int, c_void_p]),
    "rnamsm_split_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "rnamsm_gemm_bf16": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                 c_int64, c_int, c_int, c_int, c_float, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p]),
    "rnamsm_layernorm_split": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_int,
                                       c_void_p]),
    "rnamsm_row_logits_nsplit": (c_int, [c_int, c_int, c_int]),
    "rnamsm_row_logits_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "rnamsm_row_logits": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "rnamsm_softmax_rows": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "rnamsm_softmax_rows_scaled": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_float, c_void_p]),
    "rnamsm_row_chunks": (c_int, [c_int, c_int, c_int]),
    "rnamsm_row_logits_chunked": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                          c_void_p]),
    "rnamsm_softmax_rows_chunked": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p]),
    "rnamsm_row_apply": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int,
                                 c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "rnamsm_col_attn_fused": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int,
                                      c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "rnamsm_row_logits16_nsplit": (c_int, [c_int, c_int, c_int, c_int]),
    "rnamsm_row_logits16_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "rnamsm_row_logits16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int,
                                    c_float, c_int, c_void_p]),
    "rnamsm_softmax_rows_planes": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_int, c_int,
                                           c_void_p, c_int, c_void_p]),
    "rnamsm_row_apply16": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int,
                                   c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_int, c_void_p]),
    "rnamsm_col_attn16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                  c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "rnamsm_col_attn16_prescaled": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                            c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "rnamsm_zero_plane_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int64, c_void_p]),
    "rnamsm_add": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "rnamsm_head_mean": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p]),
    "rnamsm_pad_mask": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "rnamsm_pack_outputs": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "rnamsm_contact_head_workspace_bytes": (c_size_t, [c_int, c_int]),
    "rnamsm_contact_head": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p]),
    "rnamsm_contact_head_atp": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_contact_head_packed_workspace_bytes": (c_size_t, [c_int, POINTER(c_int), c_int]),
    "rnamsm_contact_head_packed": (c_int, [POINTER(ContactItem), c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_lm_head_workspace_bytes": (c_size_t, [c_int, c_int]),
    "rnamsm_lm_head": (c_int, [POINTER(LmItem), c_int, c_int, POINTER(c_void_p), c_float, c_void_p, c_size_t, c_void_p]),
    "rnamsm_lm_head_packed_workspace_bytes": (c_size_t, [c_int, POINTER(c_int), c_int]),
    "rnamsm_lm_head_packed": (c_int, [POINTER(LmItem), c_int, c_int, c_int, POINTER(c_void_p), c_float, c_void_p, c_size_t, c_void_p]),
    "rnamsm_stitch_num_windows": (c_int, [c_int, c_int, c_int]),
    "rnamsm_stitch_rows": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "rnamsm_stitch_pairs": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                    c_void_p]),
    "rnamsm_ss_head_workspace_bytes": (c_size_t, [c_int]),
    "rnamsm_ss_head": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, POINTER(c_void_p), c_void_p, c_void_p, c_void_p, c_size_t,
                               c_void_p]),
    "rnamsm_ss_head_packed_workspace_bytes": (c_size_t, [c_int, POINTER(c_int)]),
    "rnamsm_ss_head_packed": (c_int, [POINTER(SsItem), c_int, c_int, POINTER(c_void_p), c_void_p, c_size_t, c_void_p]),
    "rnamsm_ss_pack_conv16": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "rnamsm_ss_head16_workspace_bytes": (c_size_t, [c_int]),
    "rnamsm_ss_head16": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, POINTER(c_void_p), c_void_p, c_void_p, c_void_p, c_size_t,
                                 c_void_p]),
    "rnamsm_ss_head16_packed_workspace_bytes": (c_size_t, [c_int, POINTER(c_int)]),
    "rnamsm_ss_head16_packed": (c_int, [POINTER(SsItem), c_int, c_int, POINTER(c_void_p), c_void_p, c_size_t, c_void_p]),
    "rnamsm_ss_prob_text_bytes": (c_size_t, [c_int]),
    "rnamsm_ss_prob_text": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "rnamsm_ss_prob_text_packed": (c_int, [POINTER(SsTextItem), c_int, c_void_p]),
    "rnamsm_ss_pairs_workspace_bytes": (c_size_t, [c_int, POINTER(c_int)]),
    "rnamsm_ss_struct_text_bytes": (c_int, [c_int, POINTER(c_size_t), POINTER(c_size_t)]),
    "rnamsm_ss_pairs": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_ss_pairs_packed": (c_int, [POINTER(SsPairsItem), c_int, c_void_p, c_size_t, c_void_p]),
    "rnamsm_contact_head_long_workspace_bytes": (c_size_t, [c_int, c_int]),
    "rnamsm_contact_head_long": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_ss_head_long_workspace_bytes": (c_size_t, [c_int]),
    "rnamsm_ss_head_long": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, POINTER(c_void_p), c_void_p, c_void_p, c_void_p, c_size_t,
                                    c_void_p]),
    "rnamsm_ss_prob_text_long_bytes": (c_size_t, [c_int]),
    "rnamsm_ss_prob_text_long": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "rnamsm_ss_nested_workspace_bytes": (c_size_t, [c_int, POINTER(c_int)]),
    "rnamsm_ss_nested": (c_int, [c_void_p, c_void_p, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_size_t, c_void_p]),
    "rnamsm_ss_nested_packed": (c_int, [POINTER(SsNestedItem), c_int, c_float, c_int, c_void_p, c_size_t, c_void_p]),
    "rnamsm_ss_nested_phases": (c_int, [POINTER(SsNestedItem), c_int, c_float, c_int, c_void_p, c_size_t, c_int, c_void_p]),
    "rnamsm_ss_pairs_long_workspace_bytes": (c_size_t, [c_int]),
    "rnamsm_ss_struct_text_long_bytes": (c_int, [c_int, POINTER(c_size_t), POINTER(c_size_t)]),
    "rnamsm_ss_pairs_long": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_rsa_head_workspace_bytes": (c_size_t, [c_int, c_int]),
    "rnamsm_rsa_head": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_int, POINTER(c_void_p), c_void_p, c_void_p, c_void_p,
                                c_size_t, c_void_p]),
    "rnamsm_rsa_head_packed_workspace_bytes": (c_size_t, [c_int, POINTER(c_int), c_int]),
    "rnamsm_rsa_head_packed": (c_int, [POINTER(RsaItem), c_int, c_int, c_int, POINTER(c_void_p), c_void_p, c_size_t, c_void_p]),
    "rnamsm_rsa_text_bytes": (c_size_t, [c_int, c_int]),
    "rnamsm_rsa_text": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rnamsm_rsa_text_packed": (c_int, [POINTER(RsaTextItem), c_int, c_int, c_void_p]),
    "rnamsm_rsa_head_long_workspace_bytes": (c_size_t, [c_int, c_int]),
    "rnamsm_rsa_head_long": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_int, POINTER(c_void_p), c_void_p, c_void_p, c_void_p,
                                     c_size_t, c_void_p]),
    "rnamsm_rsa_text_long_bytes": (c_size_t, [c_int, c_int]),
    "rnamsm_rsa_text_long": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rnamsm_greedy_select_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "rnamsm_greedy_select": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_msa_weights": (c_int, [c_void_p, c_int, c_int, c_double, c_void_p, c_void_p]),
    "rnamsm_msa_invcov_workspace_bytes": (c_size_t, [c_int, c_int]),
    "rnamsm_msa_invcov": (c_int, [c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_msa_mi_workspace_bytes": (c_size_t, [c_int, c_int]),
    "rnamsm_msa_mi": (c_int, [c_void_p, c_int, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_msa_wmi_workspace_bytes": (c_size_t, [c_int, c_int]),
    "rnamsm_msa_wmi_min_workspace_bytes": (c_size_t, [c_int, c_int]),
    "rnamsm_msa_wmi": (c_int, [c_void_p, c_int, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_size_t, c_void_p]),
    "rnamsm_apc_f64_workspace_bytes": (c_size_t, [c_int]),
    "rnamsm_apc_f64": (c_int, [c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_msa_pdist_workspace_bytes": (c_size_t, [c_int, c_int]),
    "rnamsm_msa_pdist": (c_int, [c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_msa_neff_workspace_bytes": (c_size_t, [c_int, c_int]),
    "rnamsm_msa_neff_min_workspace_bytes": (c_size_t, [c_int, c_int]),
    "rnamsm_msa_neff": (c_int, [c_void_p, c_int, c_int, c_int64, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_msa_coverage": (c_int, [c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p]),
    "rnamsm_seqid_filter_workspace_bytes": (c_size_t, [c_int, c_int]),
    "rnamsm_seqid_filter": (c_int, [c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_top_pairs_workspace_bytes": (c_size_t, [c_int, c_int]),
    "rnamsm_top_pairs_f64": (c_int, [c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_top_pairs_f32": (c_int, [c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_pair_sweep_workspace_bytes": (c_size_t, [c_int]),
    "rnamsm_pair_sweep_f64": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_pair_sweep_f32": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_pair_precision_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "rnamsm_pair_precision_f64": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_pair_precision_f32": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rnamsm_forward_workspace_bytes": (c_size_t, [POINTER(ModelDims), c_int, c_int, c_int, c_int]),
    "rnamsm_forward": (c_int, [POINTER(ModelDims), POINTER(c_void_p), c_void_p, c_int, c_int, c_void_p, c_size_t,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                               POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), c_void_p]),
    "rnamsm_forward_batch_workspace_bytes": (c_size_t, [POINTER(ModelDims), c_int, c_int, c_int]),
    "rnamsm_forward_batch": (c_int, [POINTER(ModelDims), POINTER(c_void_p), c_void_p, c_int, c_int, c_int, c_void_p, c_size_t,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, POINTER(c_void_p), c_int,
                                     POINTER(c_void_p), c_void_p]),
    "rnamsm_forward_packed_workspace_bytes": (c_size_t, [POINTER(ModelDims), c_int, c_void_p]),
    "rnamsm_forward_packed": (c_int, [POINTER(ModelDims), POINTER(c_void_p), c_void_p, c_int, c_void_p, c_void_p, c_size_t,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_void_p), c_int, POINTER(c_void_p),
                                      c_void_p]),
    "rnamsm_ln_fold_weights": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                       c_void_p]),
    "rnamsm_row_partials": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "rnamsm_gemm_residual_stats": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                           c_int64, c_int, c_int, c_void_p, c_int64, c_int, c_void_p]),
    "rnamsm_gemm16_lnfold": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_float, c_int, c_int, c_int, c_void_p]),
    "rnamsm_gemm16_residual_stats": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                             c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p,
                                             c_int64, c_void_p]),
    "rnamsm_row_stats_from_partials": (c_int, [c_void_p, c_int64, c_int64, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "rnamsm_gemm_lnfold": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p,
                                   c_int64, c_int64, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p]),
    "rnamsm_col_attn_fused_prescaled": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int,
                                                c_int, c_int, c_void_p]),
    "rnamsm_col_attn_fused_queries": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int,
                                              c_int, c_int, c_void_p, c_int, c_void_p]),
    "rnamsm_col_attn_probs": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_float,
                                      c_int, c_void_p]),
    "rnamsm_col_attn_probs16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int,
                                        c_void_p, c_int, c_float, c_void_p]),
    "rnamsm_timing_enable": (c_int, [c_int]),
    "rnamsm_timing_collect": (c_int, []),
    "rnamsm_timing_get": (c_int, [c_int, POINTER(c_char_p), POINTER(ctypes.c_longlong), POINTER(ctypes.c_double),
                                  POINTER(ctypes.c_double), POINTER(ctypes.c_double)]),
    "rnamsm_timing_get_bound": (c_int, [c_int, POINTER(ctypes.c_double), POINTER(ctypes.c_double), POINTER(ctypes.c_double)]),
    "rnamsm_timing_get_valu_bound": (c_int, [c_int, POINTER(ctypes.c_double)]),
    "rnamsm_timing_reset": (None, []),
    "rnamsm_set_param": (c_int, [c_char_p, c_int]),
    "rnamsm_get_param": (c_int, [c_char_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


class RnamsmError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load the HIP library; loud failure if it has not been built (python __graft_entry__.py / make -C csrc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RnamsmError(
                f"{LIB_PATH} not found: the HIP extension is the only implementation of this path "
                "(no CPU fallback). Build it with `make -C rna-msm_amd/csrc` or `python -c 'import __graft_entry__ as g; g.build()'`.")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)      # AttributeError if the header and the library disagree
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def check(rc: int) -> None:
    if rc != RNAMSM_OK:
        msg = load().rnamsm_last_error().decode(errors="replace")
        if rc == -2:
            raise NotImplementedError(msg)
        raise RnamsmError(f"librnamsm_hip error {rc}: {msg}")


def kernel_timings() -> dict:
    """Fold completed HIP-event pairs and return {kernel: {launches, ms, flops, bytes, bound_ms, mfma_bound_ms, hbm_bound_ms,
    valu_bound_ms}} (rnamsm_timing_*; bound_ms = per-launch max(matrix, HBM, vector-ALU) roofline times summed over the launches)."""
    lib = load()
    n = lib.rnamsm_timing_collect()
    out = {}
    for c in range(n):
        name, cnt = c_char_p(), ctypes.c_longlong()
        ms, fl, by = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        check(lib.rnamsm_timing_get(c, ctypes.byref(name), ctypes.byref(cnt), ctypes.byref(ms), ctypes.byref(fl),
                                    ctypes.byref(by)))
        bd, mf, hb = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        check(lib.rnamsm_timing_get_bound(c, ctypes.byref(bd), ctypes.byref(mf), ctypes.byref(hb)))
        va = ctypes.c_double()
        check(lib.rnamsm_timing_get_valu_bound(c, ctypes.byref(va)))
        out[name.value.decode()] = {"launches": cnt.value, "ms": ms.value, "flops": fl.value, "bytes": by.value,
                                    "bound_ms": bd.value, "mfma_bound_ms": mf.value, "hbm_bound_ms": hb.value,
                                    "valu_bound_ms": va.value}
    return out
