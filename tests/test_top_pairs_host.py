"""The top-k ranked pairs (rnamsm_top_pairs_f64 / _f32, ops.top_pairs, rnamsm.contacts.top_pairs / top_pairs_k / format_top_pairs,
data.top_pairs / data.top_pairs_min_sep) without a GPU: the symbols, the size function, every refusal made before anything is
enqueued (on fabricated aligned addresses that are never dereferenced), the refusal of a device that is no HIP device, the spec, the
text, the two configuration keys, the refusal under a gather, the two statements of the rule (tests/top_pairs_truth.py) against each
other, and the order key's stand-alone host program (tests/native/top_pairs_key_check.cpp)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rnamsm import _lib, contacts, inference, ops
from rnamsm.config import Config, check_top_pairs, parse_overrides
import top_pairs_truth as T

NEW = ("rnamsm_top_pairs_workspace_bytes", "rnamsm_top_pairs_f64", "rnamsm_top_pairs_f32")
FAKE = 0x100000                 # 256-byte aligned, never dereferenced
ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_the_symbols_are_declared_bound_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "rnamsm.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"\b(rnamsm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header, flags=re.S))
    for name in NEW:
        assert name in protos and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert len(protos[name].split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert _lib._SIGNATURES["rnamsm_top_pairs_f64"] == _lib._SIGNATURES["rnamsm_top_pairs_f32"]
    assert "#define RNAMSM_VERSION 600" in text and lib.rnamsm_version() == 600
    doc = re.search(r"/\* The top-k ranked pairs.*?\*/", text, flags=re.S).group(0)
    for phrase in ("ONLY those elements are read", "-0.0 counts as +0.0", "larger v first, then smaller i, then smaller j",
                   "reads nothing back", "every output byte is defined"):
        assert phrase in doc, phrase
    assert callable(ops.top_pairs) and callable(contacts.top_pairs) and callable(contacts.top_pairs_k) and callable(contacts.format_top_pairs)
    assert (_lib.TOP_PAIRS_MAX_L, _lib.TOP_PAIRS_MAX_K, _lib.TOP_PAIRS_MAX_SEP) == (32768, 65536, 32768)


def test_the_size_function_at_and_outside_the_limits(lib):
    size = lib.rnamsm_top_pairs_workspace_bytes
    for L, k in ((1, 8), (0, 8), (-1, 8), (32769, 8), (8, 0), (8, -1), (8, 65537)):
        assert size(L, k) == 0, (L, k)
    for L, k in ((2, 1), (2, 65536), (17, 7), (1024, 1000), (4096, 65536), (32768, 1), (32768, 65536)):
        got = size(L, k)
        blocks = (L - 1) * -(-L // 2048)
        floor = 12 * k + 4 * (blocks + 1) + 2048                 # the selected records, a count per block, the histogram
        assert got % 256 == 0 and floor <= got <= floor + 6 * 256, (L, k, got, floor)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_refusal_is_made_before_anything_is_enqueued(lib, dtype):
    fn, name = getattr(lib, "rnamsm_top_pairs_" + dtype), "top_pairs_" + dtype
    L, k = 9, 5
    need = lib.rnamsm_top_pairs_workspace_bytes(L, k)
    ok = dict(x=FAKE, L=L, ld=L, sep=1, k=k, pairs=FAKE + 4096, scores=FAKE + 8192, count=FAKE + 12288, ws=FAKE + 16384, wsb=need)

    def call(**kw):
        a = dict(ok, **kw)
        rc = fn(a["x"], a["L"], a["ld"], a["sep"], a["k"], a["pairs"], a["scores"], a["count"], a["ws"], a["wsb"], None)
        return rc, lib.rnamsm_last_error().decode()

    for kw, text in (
            (dict(x=None), f"{name}: null pointer"),
            (dict(pairs=None), f"{name}: null pointer"),
            (dict(scores=None), f"{name}: null pointer"),
            (dict(count=None), f"{name}: null pointer"),
            (dict(ws=None), f"{name}: null pointer"),
            (dict(L=1, ld=1), f"{name}: L=1 outside [2, 32768]"),
            (dict(L=32769, ld=32769), f"{name}: L=32769 outside [2, 32768]"),
            (dict(k=0), f"{name}: k=0 outside [1, 65536]"),
            (dict(k=65537), f"{name}: k=65537 outside [1, 65536]"),
            (dict(sep=0), f"{name}: min_sep=0 outside [1, 32768]"),
            (dict(sep=-3), f"{name}: min_sep=-3 outside [1, 32768]"),
            (dict(sep=32769), f"{name}: min_sep=32769 outside [1, 32768]"),
            (dict(ld=8), f"{name}: ld=8 is smaller than L=9"),
            (dict(wsb=need - 1), f"{name}: workspace of {need - 1} bytes is smaller than the {need} that L=9, k=5 need"),
            (dict(wsb=0), f"{name}: workspace of 0 bytes is smaller than the {need} that L=9, k=5 need"),
            (dict(ws=FAKE + 16384 + 128), f"{name}: workspace misaligned (256 bytes)"),
            (dict(x=FAKE + 2), f"{name}: x / pairs / scores / count misaligned"),
            (dict(pairs=FAKE + 4096 + 2), f"{name}: x / pairs / scores / count misaligned"),
            (dict(scores=FAKE + 8192 + 4), f"{name}: x / pairs / scores / count misaligned"),
            (dict(count=FAKE + 12288 + 1), f"{name}: x / pairs / scores / count misaligned")):
        rc, msg = call(**kw)
        assert rc == ERR_INVALID and msg == text, (kw, rc, msg)


def test_no_cpu_path():
    import torch
    with pytest.raises(_lib.RnamsmError, match="no CPU path"):
        ops.top_pairs(torch.zeros(4, 4, dtype=torch.float64), 3)
    for device in (None, "cpu"):
        with pytest.raises(_lib.RnamsmError, match="no CPU path"):
            contacts.top_pairs(np.zeros((4, 4)), 3, device=device)
    with pytest.raises(_lib.RnamsmError, match="no CPU path"):
        contacts.top_pairs(torch.zeros(4, 4), 3)


# ---- the rule, stated twice ------------------------------------------------------------------------------------------------------
def _small_maps():
    rng = np.random.default_rng(11)
    inf, nan, tiny = np.inf, np.nan, 5e-324
    out = {}
    for L in (2, 3, 9, 17):
        out[f"normal{L}"] = rng.standard_normal((L, L))
        out[f"ties{L}"] = rng.integers(0, 4, (L, L)).astype(np.float64)
        out[f"f32_{L}"] = rng.standard_normal((L, L)).astype(np.float32)
    z = np.zeros((9, 9))
    z[::2, 1::2] = -0.0
    out["zeros"] = z
    e = rng.choice(np.array([-inf, -1e308, -1.0, -tiny, -0.0, 0.0, tiny, 1.0, 1.0 + 2 ** -52, 1e308, inf, nan]), (17, 17))
    out["edges"] = e
    out["all_nan"] = np.full((5, 5), nan)
    return out


@pytest.mark.parametrize("name", sorted(_small_maps()))
def test_the_numpy_truth_against_the_loop(name):
    x = _small_maps()[name]
    L = x.shape[0]
    for min_sep in sorted({1, 2, 4, max(L - 1, 1), L}):
        for k in (1, 2, 7, 64, 1000):
            p, s = T.truth(x, k, min_sep)
            lp, ls = T.truth_loop(x, k, min_sep)
            assert p.dtype == np.int64 and s.dtype == np.float64 and p.shape == (len(s), 2)
            assert np.array_equal(p, lp) and s.tobytes() == ls.tobytes(), (name, min_sep, k)
            assert len(s) <= k and np.all(p[:, 1] - p[:, 0] >= min_sep) and not np.isnan(s).any()
            assert not np.any((s == 0) & np.signbit(s))                               # a zero is +0.0
    if name == "all_nan":
        assert len(T.truth(x, 5, 1)[1]) == 0
    pp, ps, n = T.padded(*T.truth(x, 3, 1), 6)
    assert pp.shape == (6, 2) and pp.dtype == np.int32 and n <= 3 and np.all(pp[n:] == -1) and np.isnan(ps[n:]).all()


def test_the_truth_keys_are_monotone():
    v = np.array([-np.inf, -1e308, -1.0, -5e-324, 0.0, 5e-324, 1.0, 1.0 + 2 ** -52, 1e308, np.inf])
    k = T.key_of(v)
    assert k.dtype == np.uint64 and np.all(k[1:] > k[:-1])
    assert T.key_of(np.array([-0.0]))[0] == T.key_of(np.array([0.0]))[0]


# ---- the spec, the text, the keys -------------------------------------------------------------------------------------------------
def test_top_pairs_k():
    k = contacts.top_pairs_k
    assert k("1", 35) == 1 and k("53", 35) == 53 and k("53", 2) == 53
    assert k("1.5L", 35) == 53                      # ceil(52.5)
    assert k("0.1L", 30) == 3                       # exactly 3: float arithmetic gives 3.0000000000000004 and a ceiling of 4
    assert k("0.001L", 30) == 1 and k("0.001L", 4096) == 5
    assert k("2L", 4096) == 8192 and k("0.5L", 35) == 18 and k(".5L", 4) == 2 and k("1L", 7) == 7
    for bad in ("0", "-1", "L", "1.5", "abcL", "", "0L", "0.0L", "1.5l", "1e3L", "-2L", "2 L"):
        with pytest.raises(ValueError, match="top_pairs spec"):
            k(bad, 35)
    for bad in (5, 1.5, None, True):
        with pytest.raises(ValueError, match="is not a string"):
            k(bad, 35)


def test_format_top_pairs_against_literal_text():
    pairs = np.array([[0, 3], [1, 2], [4, 9], [0, 1], [2, 7]])
    scores = np.array([np.inf, 0.1 + 0.2, -0.0, -1.5e-300, -np.inf])
    assert contacts.format_top_pairs(pairs, scores, 3) == (
        "# i j score (1-based, j - i >= 3)\n"
        "1 4 inf\n"
        "2 3 0.30000000000000004\n"
        "5 10 0.0\n"
        "1 2 -1.5e-300\n"
        "3 8 -inf\n")
    assert contacts.format_top_pairs(np.zeros((0, 2), dtype=np.int64), np.zeros(0), 1) == "# i j score (1-based, j - i >= 1)\n"
    assert float("0.30000000000000004") == 0.1 + 0.2              # repr round-trips: the text holds every bit


def test_check_top_pairs_and_the_configuration_keys():
    d = Config().data
    assert d.top_pairs == "" and d.top_pairs_min_sep == 1                              # the default is off
    cfg = parse_overrides(["data.top_pairs=1.5L", "data.top_pairs_min_sep=3"])
    assert cfg.data.top_pairs == "1.5L" and cfg.data.top_pairs_min_sep == 3
    assert parse_overrides(["data.top_pairs=100"]).data.top_pairs == "100"
    assert parse_overrides(["data.top_pairs="]).data.top_pairs == ""
    assert check_top_pairs("", 1) == ("", 1) and check_top_pairs("2L", 6) == ("2L", 6)
    for tok, text in (("data.top_pairs=foo", "data.top_pairs='foo'"), ("data.top_pairs=0", "data.top_pairs='0'"),
                      ("data.top_pairs=-1L", "data.top_pairs='-1L'"), ("data.top_pairs=L", "data.top_pairs='L'"),
                      ("data.top_pairs_min_sep=0", "data.top_pairs_min_sep=0 outside [1, 32768]"),
                      ("data.top_pairs_min_sep=32769", "data.top_pairs_min_sep=32769 outside [1, 32768]")):
        with pytest.raises(ValueError, match=re.escape(text)):
            parse_overrides([tok])
    with pytest.raises(ValueError):
        parse_overrides(["data.top_pairs_min_sep=2.5"])
    with pytest.raises(ValueError, match=re.escape("data.top_pairs=5 is not a string")):
        check_top_pairs(5)
    with pytest.raises(ValueError, match=re.escape("data.top_pairs_min_sep=True is not an integer")):
        check_top_pairs("2L", True)
    cfg = Config()
    cfg.data.top_pairs = "many"                       # set past the parser: refused where the switches are read
    with pytest.raises(ValueError, match=re.escape("data.top_pairs='many'")):
        inference.read_switches(cfg, False)
    sw = inference.read_switches(parse_overrides(["data.top_pairs=2L", "data.top_pairs_min_sep=4"]), False)
    assert sw.top_pairs == "2L" and sw.top_pairs_min_sep == 4
    assert inference.read_switches(Config(), False).top_pairs == ""


def test_the_key_is_refused_under_a_gather():
    cfg = parse_overrides(["data.top_pairs=2L"])
    with pytest.raises(ValueError, match=re.escape("data.top_pairs='2L' is not available with RNAMSM_GATHER_TO_RANK0=1")):
        inference.read_switches(cfg, True)
    with pytest.raises(ValueError, match="RNAMSM_GATHER_TO_RANK0=1"):
        inference.extract_feat(cfg, gather_to_rank0=True)                # at start-up: before a file or the device is looked at
    assert inference.read_switches(Config(), True).top_pairs == ""       # off: the gather is what it was


# ---- the order key's host program --------------------------------------------------------------------------------------------------
def test_the_key_header_in_its_host_program(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host check of top_pairs_key.h"
    exe = str(tmp_path / "top_pairs_key_check")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "native", "top_pairs_key_check.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok "), (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert int(res.stdout.split()[1]) >= 16 * 16 * 4 + 5000 * 8
