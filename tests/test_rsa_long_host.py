"""The RSA head on stitched long alignments, without a GPU: the new C-ABI symbols (rnamsm_rsa_head_long, rnamsm_rsa_text_long and
their size functions), the long workspace layout's size, every refusal (made before anything is launched, on fabricated addresses
that are never dereferenced), the range checks of rnamsm.ops and RSAEnsemble, and csrc/rsa_text.h's line writer at the long limit
compiled into a stand-alone program (tests/native/rsa_text_long_check.cpp) with g++, plain and under AddressSanitizer + UBSan.  The
existing entry points keep their limits."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import rsa_truth as T
from conftest import ROOT
from rnamsm import _lib, ops, rsa

NEW = ("rnamsm_rsa_head_long_workspace_bytes", "rnamsm_rsa_head_long", "rnamsm_rsa_text_long_bytes", "rnamsm_rsa_text_long")
FAKE = 0x10000
SRC = os.path.join(ROOT, "tests", "native", "rsa_text_long_check.cpp")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_the_new_symbols_are_declared_bound_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnamsm.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\b(rnamsm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header, flags=re.S))
    for name in NEW:
        assert name in protos and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert len(protos[name].split(",")) == len(_lib._SIGNATURES[name][1]), name
    # the argument lists of the namesakes
    assert _lib._SIGNATURES["rnamsm_rsa_head_long"] == _lib._SIGNATURES["rnamsm_rsa_head"]
    assert _lib._SIGNATURES["rnamsm_rsa_text_long"] == _lib._SIGNATURES["rnamsm_rsa_text"]
    assert re.sub(r"\s+", " ", protos["rnamsm_rsa_head_long"]) == re.sub(r"\s+", " ", protos["rnamsm_rsa_head"])
    assert re.sub(r"\s+", " ", protos["rnamsm_rsa_text_long"]) == re.sub(r"\s+", " ", protos["rnamsm_rsa_text"])
    assert re.search(r"#define RNAMSM_LONG_MAX_L 4096\b", header) and re.search(r"#define RNAMSM_RSA_MAX_L 1024\b", header)
    for fn in ("rsa_head_long", "rsa_text_long"):
        assert callable(getattr(ops, fn))
    for fn in ("predict_long", "logits_long", "predict_text_long"):
        assert callable(getattr(rsa.RSAEnsemble, fn))
    assert callable(rsa.RSAHead.one_long) and callable(rsa.table_text_long)


def test_sizes(lib):
    for K in (1, 3, 8):
        for L in (1, 1025, 4096):
            assert lib.rnamsm_rsa_head_long_workspace_bytes(L, K) > 0
        for L in (1, 31, 1024, 1025, 1057, 4095, 4096):
            assert lib.rnamsm_rsa_head_long_workspace_bytes(L, K) == K * (7 * L * 64 + 128 * 64) * 4
            assert lib.rnamsm_rsa_text_long_bytes(L, K) == (K + 1) * 23 * L
        for L in (0, 4097, -1):
            assert lib.rnamsm_rsa_head_long_workspace_bytes(L, K) == 0 and lib.rnamsm_rsa_text_long_bytes(L, K) == 0
    for K in (0, 9):
        assert lib.rnamsm_rsa_head_long_workspace_bytes(35, K) == 0 and lib.rnamsm_rsa_text_long_bytes(35, K) == 0
    for L in (1, 35, 1024):                               # where both accept the L the text sizes agree; the head's layouts differ
        assert lib.rnamsm_rsa_text_long_bytes(L, 3) == lib.rnamsm_rsa_text_bytes(L, 3)
        assert lib.rnamsm_rsa_head_long_workspace_bytes(L, 3) - lib.rnamsm_rsa_head_workspace_bytes(L, 3) == 3 * 96 * 64 * 4
    # the existing entry points keep their limits and their layout
    assert lib.rnamsm_rsa_head_workspace_bytes(1025, 1) == 0 and lib.rnamsm_rsa_text_bytes(1025, 3) == 0
    assert lib.rnamsm_rsa_head_workspace_bytes(1024, 1) == (7 * 1024 * 64 + 32 * 64) * 4
    assert len("4096\t\tG\t\t400.00\t\t1.000\n") == 23


def _refused(lib, rc, *needles):
    assert rc == -1, rc
    msg = lib.rnamsm_last_error().decode()
    for n in needles:
        assert n in msg, (n, msg)


def _table(K=3):
    n = 4 + 26 * K
    return (ctypes.c_void_p * n)(*[FAKE * (32 + k) for k in range(n)])


def test_refusals_of_the_head(lib):
    def call(emb=FAKE, stride=768, codes=2 * FAKE, L=8, K=3, onehot=1, weights=_table(), probs=3 * FAKE, logits=4 * FAKE,
             workspace=5 * FAKE, nbytes=1 << 30):
        return lib.rnamsm_rsa_head_long(emb, stride, codes, L, K, onehot, weights, probs, logits, workspace, nbytes, None)

    _refused(lib, call(L=0), "rsa_head_long:", "L=0", "[1, 4096]")
    _refused(lib, call(L=4097), "rsa_head_long:", "L=4097", "[1, 4096]")
    _refused(lib, call(L=-5), "L=-5")
    _refused(lib, call(K=0), "n_models=0")
    _refused(lib, call(K=9), "n_models=9")
    for name, shown in (("emb", "emb"), ("codes", "base_codes"), ("weights", "weights"), ("workspace", "workspace")):
        _refused(lib, call(**{name: None}), "rsa_head_long:", "null", f"({shown})")
    _refused(lib, call(probs=None, logits=None), "neither probs nor logits")
    _refused(lib, call(stride=767), "row stride 767")
    for L, K in ((8, 3), (1025, 3), (4096, 8)):
        need = K * (7 * L * 64 + 128 * 64) * 4
        _refused(lib, call(L=L, K=K, weights=_table(K), nbytes=need - 1), f"workspace of {need - 1} bytes", f"{need} needed")
    # the existing layout's size is short for the long call at every L
    _refused(lib, call(L=1024, nbytes=lib.rnamsm_rsa_head_workspace_bytes(1024, 3)), "workspace of", "needed")
    _refused(lib, call(emb=FAKE + 8), "emb", "16-byte")
    _refused(lib, call(workspace=5 * FAKE + 8), "workspace", "16-byte")
    _refused(lib, call(probs=3 * FAKE + 2), "probs", "4-byte")
    _refused(lib, call(logits=4 * FAKE + 2), "logits", "4-byte")
    bad = _table()
    bad[4 + 26 + 5] = None
    _refused(lib, call(weights=bad), "rsa_head_long", "weight pointer 35 is null")
    bad = _table()
    bad[7] = FAKE * 39 + 4
    _refused(lib, call(weights=bad), "rsa_head_long", "weight pointer 7", "16-byte")
    # the existing entry point keeps its limit and its message
    _refused(lib, lib.rnamsm_rsa_head(FAKE, 768, 2 * FAKE, 1025, 3, 1, _table(), 3 * FAKE, 4 * FAKE, 5 * FAKE, 1 << 30, None),
             "rsa_head:", "L=1025", "[1, 1024]")


def test_refusals_of_the_text(lib):
    def call(values=FAKE, letters=2 * FAKE, L=8, K=3, text=3 * FAKE, counts=4 * FAKE, ens=5 * FAKE):
        return lib.rnamsm_rsa_text_long(values, letters, L, K, text, counts, ens, None)

    _refused(lib, call(L=0), "rsa_text_long:", "L=0", "[1, 4096]")
    _refused(lib, call(L=4097), "rsa_text_long:", "L=4097", "[1, 4096]")
    _refused(lib, call(K=0), "n_models=0")
    _refused(lib, call(K=9), "n_models=9")
    for name in ("values", "letters", "text", "counts"):           # ens may be null
        _refused(lib, call(**{name: None}), "rsa_text_long:", "null")
    _refused(lib, call(values=FAKE + 2), "4-byte")
    _refused(lib, call(counts=4 * FAKE + 2), "4-byte")
    _refused(lib, call(text=3 * FAKE + 8), "16-byte")
    _refused(lib, call(ens=5 * FAKE + 4), "8-byte")
    _refused(lib, lib.rnamsm_rsa_text(FAKE, 2 * FAKE, 1025, 3, 3 * FAKE, 4 * FAKE, 5 * FAKE, None), "rsa_text:", "L=1025", "[1, 1024]")


def _ensemble():
    st = T.load_stats("oh")
    member = rsa.RSAPredictor.from_state_dict({k: torch.from_numpy(v) for k, v in T.make_state(5).items()})
    return rsa.RSAEnsemble([member], {"emb": (st["emb_mu"], st["emb_std"]), "oh": (st["oh_mu"], st["oh_std"])})


def test_ops_and_the_ensemble_refuse_a_length_out_of_range_before_anything_else():
    """A length out of range is wrong on any device: ValueError, with the value and the range, before the operand's device is asked
    for.  In range, a host tensor is refused as everywhere (no CPU path)."""
    codes = torch.zeros(4097, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"rsa_head_long: emb: L = 4097 outside \[1, 4096\]"):
        ops.rsa_head_long(torch.zeros(4097, 768), codes, None, 3, True)
    with pytest.raises(ValueError, match=r"L = 0 outside \[1, 4096\]"):
        ops.rsa_head_long(torch.zeros(0, 768), codes[:0], None, 3, True)
    with pytest.raises(ValueError, match=r"rsa_text_long: rsa: L = 4097 outside \[1, 4096\]"):
        ops.rsa_text_long(torch.zeros(3, 4097), codes)
    with pytest.raises(ValueError, match="want must be"):
        ops.rsa_head_long(torch.zeros(8, 768), codes[:8], None, 3, True, want="both")
    with pytest.raises(_lib.RnamsmError, match="no CPU path"):
        ops.rsa_head_long(torch.zeros(1025, 768), codes[:1025], None, 3, True)
    with pytest.raises(_lib.RnamsmError, match="no CPU path"):
        ops.rsa_text_long(torch.zeros(3, 1025), codes[:1025])
    ens = _ensemble()
    for fn in (ens.predict_long, ens.logits_long, ens.predict_text_long):
        with pytest.raises(ValueError, match=r"L = 4097 outside the head's range \[1, 4096\]"):
            fn(torch.zeros(4097, 768), "A" * 4097)
        with pytest.raises(ValueError, match="seq has length 9"):
            fn(torch.zeros(1025, 768), "A" * 9)
        with pytest.raises(ValueError, match=r"must be \[L, 768\]"):
            fn(torch.zeros(1025, 767), "A" * 1025)
        with pytest.raises(_lib.RnamsmError, match="no CPU path"):
            fn(torch.zeros(1025, 768), "A" * 1025)
    # the existing methods keep their range
    with pytest.raises(ValueError, match=r"L = 1025 outside the head's range \[1, 1024\]"):
        ens.predict_many([torch.zeros(1025, 768)], ["A" * 1025])


def test_the_host_writer_has_no_length_limit(tmp_path):
    """write_rsa_files at L = 4096 (the route of data.rsa_text_device=false on a stitched alignment): the last line's index has four
    digits and the longest line is 23 bytes."""
    import random
    L = 4096
    values = np.full((2, L), 1.0, np.float32)
    rsa.write_rsa_files(values, "G" * L, "wide", tmp_path, ["a", "b"], random.Random(2022))
    body = (tmp_path / "RSA_result" / "wide_ensemble" / "wide.txt").read_bytes().split(b"\n")
    assert body[-2] == b"4096\t\tG\t\t400.00\t\t1.000" and max(len(ln) + 1 for ln in body[3:-1]) == _lib.RSA_TEXT_LINE_MAX


# ---------------------------------------------------------------------- rsa_text.h's line writer at the long limit, on the host
def _build(tmp_path_factory, tag, flags):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host check of rsa_text.h"
    exe = str(tmp_path_factory.mktemp("rsa_text_long_" + tag) / "rsa_text_long_check")
    subprocess.run([cxx, "-std=c++17", *flags, SRC, "-o", exe], check=True)
    return exe


def test_line_writer_against_snprintf(tmp_path_factory):
    res = subprocess.run([_build(tmp_path_factory, "plain", ["-O2"])], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert int(res.stdout.split()[1]) > 3 * 6400 + 11 * 60, res.stdout


def test_line_writer_under_sanitizers(tmp_path_factory):
    exe = _build(tmp_path_factory, "asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
