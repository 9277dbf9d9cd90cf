"""The bf16 SS head without a GPU (rnamsm_ss_head16, rnamsm_ss_head16_packed, rnamsm_ss_pack_conv16, data.ss_gemm_dtype): the
symbols, the workspace sizes, every argument refusal of the C entry points (made before anything is enqueued, on fabricated
aligned addresses that are never dereferenced: the pattern of tests/test_ss_packed_host.py) and the key in the two CLIs."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from rnamsm import _lib, ss
from rnamsm.config import parse_overrides

NUM_BLOCKS = 4
FAKE = 0x10000                             # "device addresses": non-null, 16-byte aligned, never read on the host
LS = [17, 40, 16]
SYMBOLS = ("rnamsm_ss_head16_workspace_bytes", "rnamsm_ss_head16", "rnamsm_ss_head16_packed_workspace_bytes",
           "rnamsm_ss_head16_packed", "rnamsm_ss_pack_conv16")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _size(lib, Ls):
    return lib.rnamsm_ss_head16_packed_workspace_bytes(len(Ls), (ctypes.c_int * max(len(Ls), 1))(*Ls))


def _weights(n_blocks=NUM_BLOCKS):
    n = len(_lib.W_SS_STEM) + n_blocks * len(_lib.W_SS_BLOCK) + len(_lib.W_SS_HEAD)
    return (ctypes.c_void_p * n)(*[FAKE * (i + 1) for i in range(n)])


def _items(Ls):
    items = (_lib.SsItem * len(Ls))()
    for b, L in enumerate(Ls):
        base = FAKE * 1000 * (b + 1)
        items[b] = _lib.SsItem(base, L * L, base + FAKE, L, base + 2 * FAKE, base + 3 * FAKE)
    return items


def _refused(lib, rc, *needles):
    assert rc == -1, rc                                   # RNAMSM_ERR_INVALID
    msg = lib.rnamsm_last_error().decode()
    for n in needles:
        assert n in msg, (n, msg)


def test_the_five_symbols_exist(lib):
    assert set(SYMBOLS) <= set(_lib.EXPORTED_SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert _lib.SS_GEMM_DTYPES == ("f32", "bf16")


def test_workspace_sizes(lib):
    for L in (1, 17, 1024):                                # the two fp32 images of the fp32 head: the residual stream stays fp32
        assert lib.rnamsm_ss_head16_workspace_bytes(L) == lib.rnamsm_ss_head_workspace_bytes(L) == 2 * L * L * 48 * 4
    assert lib.rnamsm_ss_head16_workspace_bytes(0) == 0 and lib.rnamsm_ss_head16_workspace_bytes(1025) == 0
    assert lib.rnamsm_ss_head16_workspace_bytes(-3) == 0
    assert _size(lib, LS) == lib.rnamsm_ss_head_packed_workspace_bytes(3, (ctypes.c_int * 3)(*LS)) > 0
    assert _size(lib, [1024] * 1024) >= 2 * 1024 * 1024 * 1024 * 48 * 4              # the largest batch: no 32-bit overflow
    assert _size(lib, []) == 0 and _size(lib, [8] * 1025) == 0                        # B = 0, B = 1025
    assert _size(lib, [8, 0, 8]) == 0 and _size(lib, [8, 1025]) == 0                  # L = 0, L = 1025
    assert lib.rnamsm_ss_head16_packed_workspace_bytes(2, None) == 0                  # null Ls


def _lone(lib, atp=FAKE, stride=None, codes=2 * FAKE, L=17, num_blocks=NUM_BLOCKS, weights=None, logits=3 * FAKE, probs=4 * FAKE,
          ws=FAKE * 5000, ws_bytes=None):
    stride = L * L if stride is None else stride
    ws_bytes = lib.rnamsm_ss_head16_workspace_bytes(17) if ws_bytes is None else ws_bytes
    return lib.rnamsm_ss_head16(atp, stride, codes, L, num_blocks, _weights() if weights is None else weights, logits, probs, ws,
                                ws_bytes, None)


def test_lone_refusals_on_a_host_without_a_gpu(lib):
    _refused(lib, _lone(lib, L=0, stride=1), "L=0")
    _refused(lib, _lone(lib, L=1025, ws_bytes=1 << 40), "L=1025")
    _refused(lib, _lone(lib, num_blocks=0), "num_blocks=0")
    _refused(lib, _lone(lib, num_blocks=65, weights=_weights(65)), "num_blocks=65")
    for kw in ({"atp": None}, {"codes": None}, {"ws": None}):
        _refused(lib, _lone(lib, **kw), "null")
    assert lib.rnamsm_ss_head16(FAKE, 289, 2 * FAKE, 17, NUM_BLOCKS, None, 3 * FAKE, 4 * FAKE, FAKE * 5000, 1 << 40, None) == -1
    _refused(lib, _lone(lib, logits=None, probs=None), "neither")
    _refused(lib, _lone(lib, stride=288), "stride")
    _refused(lib, _lone(lib, ws_bytes=lib.rnamsm_ss_head16_workspace_bytes(17) - 1), "workspace")
    _refused(lib, _lone(lib, ws=FAKE * 5000 + 8), "alignment")
    bad = _weights()
    bad[7] = None
    _refused(lib, _lone(lib, weights=bad), "weight pointer 7")
    bad = _weights()
    bad[4] = FAKE + 2                                      # a bf16 plane: 16-byte aligned like every entry
    _refused(lib, _lone(lib, weights=bad), "weight pointer 4")


def _packed(lib, items=None, B=None, num_blocks=NUM_BLOCKS, weights=None, ws=FAKE * 5000, ws_bytes=None, Ls=LS):
    items = _items(Ls) if items is None else items
    B = len(Ls) if B is None else B
    ws_bytes = _size(lib, Ls) if ws_bytes is None else ws_bytes
    return lib.rnamsm_ss_head16_packed(items, B, num_blocks, _weights() if weights is None else weights, ws, ws_bytes, None)


def test_packed_refusals_on_a_host_without_a_gpu(lib):
    _refused(lib, _packed(lib, B=0), "B=0")
    _refused(lib, lib.rnamsm_ss_head16_packed(_items([4] * 1025), 1025, NUM_BLOCKS, _weights(), FAKE * 5000, 1 << 40, None), "B=1025")
    _refused(lib, _packed(lib, num_blocks=0), "num_blocks=0")
    _refused(lib, _packed(lib, num_blocks=65, weights=_weights(65)), "num_blocks=65")
    assert lib.rnamsm_ss_head16_packed(None, 3, NUM_BLOCKS, _weights(), FAKE * 5000, 1 << 40, None) == -1
    assert lib.rnamsm_ss_head16_packed(_items(LS), 3, NUM_BLOCKS, None, FAKE * 5000, 1 << 40, None) == -1
    _refused(lib, _packed(lib, ws=None), "null")
    for member in range(len(LS)):
        for field, value, needle in (("L", 0, "L=0"), ("L", 1025, "L=1025"), ("atp", None, "null"), ("base_codes", None, "null"),
                                     ("atp", FAKE + 2, "aligned"), ("logits", FAKE + 1, "aligned"), ("probs", FAKE + 3, "aligned"),
                                     ("atp_plane_stride", LS[member] ** 2 - 1, "stride")):
            items = _items(LS)
            setattr(items[member], field, value)
            _refused(lib, _packed(lib, items=items, ws_bytes=1 << 40), f"member {member}", needle)
        items = _items(LS)
        items[member].logits = None
        items[member].probs = None
        _refused(lib, _packed(lib, items=items), f"member {member}", "neither")
    _refused(lib, _packed(lib, ws_bytes=_size(lib, LS) - 1), "workspace")
    _refused(lib, _packed(lib, ws=FAKE * 5000 + 8), "alignment")
    bad = _weights()
    bad[9] = FAKE + 4
    _refused(lib, _packed(lib, weights=bad), "weight pointer 9")


def test_pack_conv16_refusals(lib):
    _refused(lib, lib.rnamsm_ss_pack_conv16(None, FAKE, 16, None), "null")
    _refused(lib, lib.rnamsm_ss_pack_conv16(FAKE, None, 16, None), "null")
    _refused(lib, lib.rnamsm_ss_pack_conv16(FAKE, 2 * FAKE, 0, None), "n=0")
    _refused(lib, lib.rnamsm_ss_pack_conv16(FAKE + 2, 2 * FAKE, 16, None), "aligned")
    _refused(lib, lib.rnamsm_ss_pack_conv16(FAKE, 2 * FAKE + 8, 16, None), "aligned")


def test_the_predictor_s_property():
    assert ss.SSPredictor(1).gemm_dtype == "f32"
    m = ss.SSPredictor(1, gemm_dtype="bf16")
    assert m.gemm_dtype == "bf16"
    with pytest.raises(ValueError, match="f32, bf16"):
        m.gemm_dtype = "fp8"
    with pytest.raises(ValueError, match="f32, bf16"):
        ss.SSPredictor(1, gemm_dtype="f16x3")
    with pytest.raises(_lib.RnamsmError, match="no CPU path"):           # the refusals of the fp32 predictor, in the bf16 mode too
        m.predict(torch.rand(120, 6, 6), "ACGUAC")


def test_parse_overrides_takes_the_key():
    assert parse_overrides([]).data.ss_gemm_dtype == "f32"
    cfg = parse_overrides(["data.ss_gemm_dtype=bf16", "model.gemm_dtype=f16x3"])
    assert cfg.data.ss_gemm_dtype == "bf16" and cfg.model.gemm_dtype == "f16x3"
    assert parse_overrides(["model.gemm_dtype=bf16"]).data.ss_gemm_dtype == "f32"      # it does not follow the forward's mode


def test_the_clis_refuse_an_unknown_arithmetic():
    with pytest.raises(ValueError, match=r"ss_gemm_dtype='fp8'.*f32, bf16"):
        parse_overrides(["data.ss_gemm_dtype=fp8"])
    sys.path.insert(0, ROOT)
    import RNA_MSM_Inference as cli
    with pytest.raises(ValueError, match="f32, bf16"):
        cli.main(["data.ss_gemm_dtype=fp8"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "SS_predict.py"), "--gemm-dtype", "fp8"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "f32, bf16" in r.stderr, (r.returncode, r.stderr[-500:])
