"""The identity redundancy filter (rnamsm_seqid_filter; rnamsm.msa.seqid_filter; data.sample_method=seqid-filter) without a GPU: the
host implementation against the plain-loop restatement (tests/seqid_filter_truth.py), indices and kept_at, on random alignments, the
64-row 2DRB_1 excerpt and the full 1176-row alignment (tests/golden/tokens_2DRB_1_full.npz holds all of its rows); the restatement
against the recorded figures on 2DRB_1; the threshold lists; the reader's cut; the keys; every refusal the entry point makes before
anything is enqueued (on fabricated aligned addresses that are never dereferenced); csrc/msa_words.h compiled into a stand-alone
program (tests/native/seqid_words_check.cpp) with g++ and AddressSanitizer + UBSan."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden
from rnamsm import _lib, inference, msa, ops
from rnamsm.alphabet import RNAAlphabet
from rnamsm.config import Config, check_filter_seqid, parse_overrides
import seqid_filter_truth as T

NEW = ("rnamsm_seqid_filter_workspace_bytes", "rnamsm_seqid_filter")
FAKE = 0x100000                 # 256-byte aligned, never dereferenced
GAP = 10


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def full():
    """(the 1176 x 35 alignment, the restatement's pair counts shared by every call on it)"""
    a = golden("tokens_2DRB_1_full.npz")["all_tokens"][:, 1:].astype(np.uint8)
    assert a.shape == (1176, 35)
    return a, {}


def _same(body, num_seqs, *args, order=None, memo=None):
    ti, tat, _ = T.seqid_filter(body, GAP, num_seqs, *args, order=order, memo=memo)
    hi, hat = msa.seqid_filter_host(body, GAP, num_seqs, *args, order=order)
    assert hi.dtype == np.int64 and np.array_equal(hi, ti), (num_seqs, args)
    assert np.array_equal(hat, tat), (num_seqs, args)
    return ti


def test_the_symbols_are_declared_bound_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "rnamsm.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"\b(rnamsm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header, flags=re.S))
    for name in NEW:
        assert name in protos and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert len(protos[name].split(",")) == len(_lib._SIGNATURES[name][1]), name
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    if nm:
        exported = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(rf"\bT {name}$", exported, flags=re.M), name
    assert callable(ops.seqid_filter) and callable(msa.seqid_filter) and callable(msa.seqid_filter_host)
    assert "seqid_filter.hip" in open(os.path.join(ROOT, "rna-msm_amd", "csrc", "Makefile")).read()
    assert "hhfilter-compatible" not in text and "seqid-filter" in msa.SAMPLE_METHODS


def test_the_chunk_parameter(lib):
    assert lib.rnamsm_get_param(b"seqid_filter_chunk") == 256
    try:
        for v in (64, 128, 512, 320):
            assert lib.rnamsm_set_param(b"seqid_filter_chunk", v) == 0 and lib.rnamsm_get_param(b"seqid_filter_chunk") == v
        for v in (0, 32, 100, 576, 1024, -64):
            assert lib.rnamsm_set_param(b"seqid_filter_chunk", v) == -1
            assert f"seqid_filter_chunk={v} is not a multiple of 64 in [64, 512]" in lib.rnamsm_last_error().decode()
            assert lib.rnamsm_get_param(b"seqid_filter_chunk") == 320
    finally:
        assert lib.rnamsm_set_param(b"seqid_filter_chunk", 256) == 0


def test_size_function_at_and_outside_the_limits(lib):
    size = lib.rnamsm_seqid_filter_workspace_bytes
    for N, L in ((0, 8), (-3, 8), ((1 << 20) + 1, 8), (8, 0), (8, -1), (8, 32769)):
        assert size(N, L) == 0, (N, L)
    for N, L in ((1, 1), (64, 64), (65, 65), (1176, 35), (10000, 512), (1 << 20, 1), (1, 32768)):
        rows, words = -(-N // 64) * 64, -(-(-(-L // 8)) // 8) * 8
        assert size(N, L) == rows * words * 8 + 4 * rows * 4 + 256, (N, L)     # the packed rows, four int32 per row, the two counters


def test_every_refusal_made_before_anything_is_enqueued(lib):
    N, L = 12, 9
    need = lib.rnamsm_seqid_filter_workspace_bytes(N, L)
    import ctypes
    n_kept = ctypes.c_int(-7)

    def call(**kw):
        a = dict(msa=FAKE, N=N, L=L, ld=L, gap=GAP, order=FAKE, num_seqs=4, lo=20, hi=90, step=5, idx=FAKE, at=FAKE,
                 nk=ctypes.addressof(n_kept), ws=FAKE, wsb=need)
        a.update(kw)
        rc = lib.rnamsm_seqid_filter(a["msa"], a["N"], a["L"], a["ld"], a["gap"], a["order"], a["num_seqs"], a["lo"], a["hi"], a["step"],
                                     a["idx"], a["at"], a["nk"], a["ws"], a["wsb"], None)
        return rc, lib.rnamsm_last_error().decode()

    for kw, text in (
            (dict(msa=None), "seqid_filter: null pointer"),
            (dict(idx=None), "seqid_filter: null pointer"),
            (dict(nk=None), "seqid_filter: null pointer"),
            (dict(ws=None), "seqid_filter: null pointer"),
            (dict(N=0), "seqid_filter: N=0 outside [1, 1048576]"),
            (dict(N=(1 << 20) + 1), "seqid_filter: N=1048577 outside [1, 1048576]"),
            (dict(L=0), "seqid_filter: L=0 outside [1, 32768]"),
            (dict(L=32769, ld=32769), "seqid_filter: L=32769 outside [1, 32768]"),
            (dict(ld=8), "seqid_filter: ld=8 is smaller than L=9"),
            (dict(gap=-1), "seqid_filter: gap=-1 is not a byte value"),
            (dict(gap=256), "seqid_filter: gap=256 is not a byte value"),
            (dict(num_seqs=-1), "seqid_filter: num_seqs=-1 is negative"),
            (dict(lo=0), "seqid_filter: min_seqid=0 is below 1"),
            (dict(hi=0), "seqid_filter: max_seqid=0 outside [1, 100]"),
            (dict(hi=101), "seqid_filter: max_seqid=101 outside [1, 100]"),
            (dict(step=0), "seqid_filter: step=0 is below 1"),
            (dict(wsb=need - 1), f"seqid_filter: workspace of {need - 1} bytes too small ({need}) or misaligned (256 bytes)"),
            (dict(ws=FAKE + 128), "or misaligned (256 bytes)"),
            (dict(idx=FAKE + 2), "seqid_filter: order / kept_indices / kept_at misaligned"),
            (dict(at=FAKE + 1), "seqid_filter: order / kept_indices / kept_at misaligned"),
            (dict(order=FAKE + 2), "seqid_filter: order / kept_indices / kept_at misaligned")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    assert n_kept.value == -7


def test_a_device_that_is_no_hip_device_is_refused():
    import torch
    with pytest.raises(_lib.RnamsmError, match="no CPU path"):
        ops.seqid_filter(torch.zeros(4, 5, dtype=torch.uint8), GAP, 0)


@pytest.mark.parametrize("num_seqs, want", [(0, [90]), (1, list(range(20, 90, 5)) + [90]), (512, list(range(20, 90, 5)) + [90])])
def test_threshold_lists_at_the_defaults(num_seqs, want):
    assert msa.seqid_thresholds(num_seqs) == want == T.thresholds(num_seqs)


def test_threshold_lists_off_the_defaults():
    for args, want in (((0, 20, 90, 5), [90]), ((0, 95, 40, 5), [40]),             # num_seqs = 0: plain -id
                       ((8, 90, 90, 5), [90]), ((8, 95, 90, 5), [90]), ((8, 100, 1, 1), [1]),     # min >= max
                       ((8, 20, 33, 5), [20, 25, 30, 33]), ((8, 20, 90, 30), [20, 50, 80, 90]), ((8, 89, 90, 5), [89, 90]),   # max off the grid
                       ((8, 1, 100, 1), list(range(1, 101)))):
        assert msa.seqid_thresholds(*args) == want == T.thresholds(*args), args
    for args, text in (((-1, 20, 90, 5), "num_seqs=-1 is negative"), ((4, 0, 90, 5), "min_seqid=0 is below 1"),
                       ((4, 20, 0, 5), "max_seqid=0 outside [1, 100]"), ((4, 20, 101, 5), "max_seqid=101 outside [1, 100]"),
                       ((4, 20, 90, 0), "step=0 is below 1"), ((4, 20.0, 90, 5), "min_seqid=20.0 is not an integer")):
        with pytest.raises(ValueError, match=re.escape(text)):
            msa.seqid_thresholds(*args)
        with pytest.raises(ValueError, match=re.escape(text)):
            msa.seqid_filter_host(np.zeros((2, 3), dtype=np.uint8), GAP, *args)


@pytest.mark.parametrize("N, L, seed", [(1, 1, 0), (2, 7, 1), (3, 8, 2), (17, 9, 3), (64, 33, 4), (130, 40, 5), (300, 25, 6), (257, 40, 7)])
def test_host_equals_the_restatement_on_random_alignments(N, L, seed):
    a = T.alignment(N, L, seed)
    memo = {}
    for num_seqs in (0, 1, max(1, N // 8), N):
        _same(a, num_seqs, memo=memo)
    _same(a, max(1, N // 4), 30, 77, 7, memo=memo)
    _same(a, 0, 20, 100, 5, memo=memo)
    rng = np.random.RandomState(seed)
    _same(a, max(1, N // 8), order=rng.permutation(N), memo=memo)
    b = a.copy()
    b[0] = GAP                                       # an all-gap first row is kept, another all-gap row is not
    if N > 2:
        b[N // 2] = GAP
    kept = _same(b, 0)
    assert kept[0] == 0 and (N <= 2 or N // 2 not in kept)


def test_host_equals_the_restatement_on_the_2drb1_excerpt():
    a = golden("tokens_2DRB_1_first64.npz")["tokens"][:, 1:].astype(np.uint8)
    assert a.shape == (64, 35)
    memo = {}
    for num_seqs in (0, 4, 16, 64):
        _same(a, num_seqs, memo=memo)


@pytest.mark.parametrize("num_seqs", [0, 16, 64, 128, 512])
def test_host_equals_the_restatement_on_the_full_2drb1(full, num_seqs):
    _same(full[0], num_seqs, memo=full[1])


def test_the_restatement_reproduces_the_recorded_figures_on_2drb1(full):
    """All 1176 rows, 35 columns, thresholds 20 / 90 / 5: the rows kept and the kept count after every pass."""
    a, memo = full
    low = [(t, 1) for t in range(20, 70, 5)]
    for num_seqs, kept, passes in ((0, 275, [(90, 275)]),
                                   (16, 35, low + [(70, 3), (75, 8), (80, 35)]),
                                   (64, 93, low + [(70, 3), (75, 8), (80, 35), (85, 93)]),
                                   (128, 308, low + [(70, 3), (75, 8), (80, 35), (85, 93), (90, 308)]),
                                   (512, 308, low + [(70, 3), (75, 8), (80, 35), (85, 93), (90, 308)])):
        idx, at, got = T.seqid_filter(a, GAP, num_seqs, memo=memo)
        assert len(idx) == kept and got == passes, (num_seqs, len(idx), got)
        assert idx[0] == 0 and at[0] == passes[0][0] and (np.diff(idx) > 0).all()
        assert sorted(set(at[at >= 0])) == sorted({t for (t, n), (_, before) in zip(passes, [(0, 0)] + passes) if n > before})


def test_the_reader_cuts_to_the_first_kept_rows(full, full_2drb1_a2m):
    a, memo = full
    alphabet = RNAAlphabet()
    assert alphabet.tok_to_idx["-"] == GAP
    toks = msa.load_msa_tokens(full_2drb1_a2m, alphabet, None)
    assert toks.shape == (1176, 36)
    seen = []
    for cap in (16, 64, 512):              # 35 and 93 kept: cut to the first 16 and 64; 308 kept against 512: all of them
        kept, _, _ = T.seqid_filter(a, GAP, cap, memo=memo)
        got = msa.load_msa_tokens(full_2drb1_a2m, alphabet, cap, "seqid-filter", on_full=lambda t: seen.append(t.shape))
        assert np.array_equal(got, toks[kept[:cap]]) and got.shape[0] == min(cap, len(kept))
        assert np.array_equal(msa.seqid_filter(toks, GAP, cap), kept)
    assert seen == [(1176, 36)] * 3 and got.shape[0] == 308
    kept, _, _ = T.seqid_filter(a, GAP, 64, 50, 95, 15, memo=memo)
    got = msa.load_msa_tokens(full_2drb1_a2m, alphabet, 64, "seqid-filter", filter_seqid=(50, 95, 15))
    assert np.array_equal(got, toks[kept[:64]])
    assert np.array_equal(msa.load_msa_tokens(full_2drb1_a2m, alphabet, 1176, "seqid-filter"), toks)      # nothing to cut: untouched


def test_hhfilter_still_raises_and_an_unknown_name_too():
    path = os.path.join(GOLDEN, "2DRB_1_first64.a2m_msa2")
    a = RNAAlphabet()
    with pytest.raises(NotImplementedError, match="seqid-filter"):
        msa.load_msa_tokens(path, a, 16, "hhfilter")
    with pytest.raises(AssertionError):
        msa.load_msa_tokens(path, a, 16, "seqid_filter")
    assert Config().data.sample_method == "hhfilter"


def test_the_keys_in_the_configuration():
    d = Config().data
    assert (d.filter_min_seqid, d.filter_max_seqid, d.filter_step) == (20, 90, 5)
    cfg = parse_overrides(["data.sample_method=seqid-filter", "data.filter_min_seqid=30", "data.filter_max_seqid=100", "data.filter_step=1"])
    assert (cfg.data.sample_method, cfg.data.filter_min_seqid, cfg.data.filter_max_seqid, cfg.data.filter_step) == ("seqid-filter", 30, 100, 1)
    for tok, text in (("data.filter_min_seqid=0", "data.filter_min_seqid=0 is below 1"),
                      ("data.filter_min_seqid=-5", "data.filter_min_seqid=-5 is below 1"),
                      ("data.filter_max_seqid=0", "data.filter_max_seqid=0 outside [1, 100]"),
                      ("data.filter_max_seqid=101", "data.filter_max_seqid=101 outside [1, 100]"),
                      ("data.filter_step=0", "data.filter_step=0 is below 1")):
        with pytest.raises(ValueError, match=re.escape(text)):
            parse_overrides([tok])
    with pytest.raises(ValueError):
        parse_overrides(["data.filter_step=2.5"])
    assert check_filter_seqid(95, 40, 7) == (95, 40, 7)              # min >= max is no error: one pass at max
    with pytest.raises(ValueError, match="data.filter_step=True is not an integer"):
        check_filter_seqid(20, 90, True)
    cfg = Config()
    cfg.data.filter_max_seqid = 150                                  # set past the parser: refused where the switches are read
    with pytest.raises(ValueError, match=re.escape("data.filter_max_seqid=150 outside [1, 100]")):
        inference.read_switches(cfg, False)
    assert inference.read_switches(Config(), False).filter_seqid == (20, 90, 5)
    assert inference.read_switches(parse_overrides(["data.filter_step=9"]), False).filter_seqid == (20, 90, 9)


@pytest.fixture(scope="module")
def words_program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host check of msa_words.h"
    exe = str(tmp_path_factory.mktemp("seqid_words") / "seqid_words_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "seqid_words_check.cpp"), "-o", exe], check=True)
    return exe


def test_the_word_form_against_a_byte_loop_under_the_sanitizers(words_program):
    res = subprocess.run([words_program], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok "), (res.returncode, res.stdout[-500:], res.stderr[-2000:])
    assert int(res.stdout.split()[1]) >= 256 * 256 + 4 * 11 * 50 + 4 * 200000 * 4 + 4 * 40 * 100 * 2
