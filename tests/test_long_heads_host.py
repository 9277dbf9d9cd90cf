"""The pair heads on stitched long alignments, without a GPU: the new C-ABI symbols, their sizes and their refusals (made before
anything is enqueued, on fabricated addresses that are never dereferenced); csrc/ss_pairs_long.h -- the long decoding's per-thread
round logic and line scan -- compiled into a stand-alone program (tests/native/ss_pairs_long_check.cpp) with g++ and AddressSanitizer
+ UBSan and compared with the host path (ss_pairs_cases.expected); data.long_heads in the configuration."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rnamsm import _lib, ss
from rnamsm.config import Config, parse_overrides
import ss_pairs_cases as C
import ss_pairs_long_cases as LC

NEW = ("rnamsm_contact_head_long_workspace_bytes", "rnamsm_contact_head_long", "rnamsm_ss_head_long_workspace_bytes",
       "rnamsm_ss_head_long", "rnamsm_ss_prob_text_long_bytes", "rnamsm_ss_prob_text_long", "rnamsm_ss_pairs_long_workspace_bytes",
       "rnamsm_ss_struct_text_long_bytes", "rnamsm_ss_pairs_long")
FAKE = 0x10000


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_the_new_symbols_are_declared_bound_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnamsm.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\b(rnamsm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header, flags=re.S))
    for name in NEW:
        assert name in protos and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert len(protos[name].split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert re.search(r"#define RNAMSM_LONG_MAX_L 4096\b", header) and _lib.LONG_MAX_L == 4096
    # the existing limits stand
    assert re.search(r"#define RNAMSM_SS_MAX_L 1024\b", header) and re.search(r"#define RNAMSM_CONTACT_MAX_L 1023\b", header)
    for fn in ("contact_head_long", "ss_head_long", "ss_prob_text_long", "ss_pairs_long"):
        from rnamsm import ops
        assert callable(getattr(ops, fn))
    assert callable(ss.SSPredictor.predict_long)


def test_sizes(lib):
    words = lambda L: (L + 63) // 64                     # noqa: E731
    want = {1: 256, 65: 1280, 1025: 139520, 4096: 2 << 20}
    for L, n in want.items():
        assert lib.rnamsm_ss_pairs_long_workspace_bytes(L) == n == -(-8 * L * words(L) // 256) * 256, L
    assert lib.rnamsm_ss_pairs_long_workspace_bytes(0) == 0 and lib.rnamsm_ss_pairs_long_workspace_bytes(4097) == 0
    for L in (1, 35, 1024):                              # where both accept the L: the existing sizes
        assert lib.rnamsm_ss_pairs_long_workspace_bytes(L) == lib.rnamsm_ss_pairs_workspace_bytes(1, (ctypes.c_int * 1)(L))
        assert lib.rnamsm_ss_prob_text_long_bytes(L) == lib.rnamsm_ss_prob_text_bytes(L)
        assert lib.rnamsm_ss_head_long_workspace_bytes(L) == lib.rnamsm_ss_head_workspace_bytes(L)
        assert lib.rnamsm_contact_head_long_workspace_bytes(min(L, 1023), 120) == lib.rnamsm_contact_head_workspace_bytes(min(L, 1023) + 1, 120)
    assert lib.rnamsm_ss_prob_text_long_bytes(4096) == 25 * 4096 * 4096
    assert lib.rnamsm_ss_prob_text_long_bytes(0) == 0 and lib.rnamsm_ss_prob_text_long_bytes(4097) == 0
    assert lib.rnamsm_ss_prob_text_bytes(1025) == 0                       # the existing entry point keeps its limit
    assert lib.rnamsm_ss_head_long_workspace_bytes(4096) == 2 * 48 * 4 * 4096 * 4096
    assert lib.rnamsm_ss_head_long_workspace_bytes(0) == 0 and lib.rnamsm_ss_head_long_workspace_bytes(4097) == 0
    assert lib.rnamsm_contact_head_long_workspace_bytes(4096, 120) == 4 * (120 * 4096 + 120)
    assert lib.rnamsm_contact_head_long_workspace_bytes(4097, 120) == 0 and lib.rnamsm_contact_head_long_workspace_bytes(0, 120) == 0
    assert lib.rnamsm_contact_head_long_workspace_bytes(5, 0) == 0
    ct, bp = ctypes.c_size_t(), ctypes.c_size_t()
    for L in (1, 1025, 4096):
        assert lib.rnamsm_ss_struct_text_long_bytes(L, ctypes.byref(ct), ctypes.byref(bp)) == 0
        assert (ct.value, bp.value) == (32 * L, 12 * L)
    assert lib.rnamsm_ss_struct_text_long_bytes(0, ctypes.byref(ct), ctypes.byref(bp)) == -1
    assert lib.rnamsm_ss_struct_text_long_bytes(4097, ctypes.byref(ct), ctypes.byref(bp)) == -1
    assert lib.rnamsm_ss_struct_text_long_bytes(5, None, ctypes.byref(bp)) == -1
    # the longest lines at the limit are still 32 and 12 bytes
    assert len("4096\t\tA\t\t4095\t\t1000\t\t1000\t\t4096\n") == 32 and len("4096 A 1000\n") == 12


def _refused(lib, rc, *needles):
    assert rc == -1, rc
    msg = lib.rnamsm_last_error().decode()
    for n in needles:
        assert n in msg, (n, msg)


def test_refusals_of_the_decoding(lib):
    def call(probs=FAKE, letters=2 * FAKE, L=8, partner=3 * FAKE, counts=4 * FAKE, ct=5 * FAKE, bpseq=6 * FAKE, workspace=7 * FAKE,
             nbytes=1 << 22):
        return lib.rnamsm_ss_pairs_long(probs, letters, L, partner, counts, ct, bpseq, workspace, nbytes, None)

    _refused(lib, call(L=0), "ss_pairs_long:", "L=0", "[1, 4096]")
    _refused(lib, call(L=4097), "L=4097")
    for name in ("probs", "letters", "partner", "counts", "ct", "bpseq", "workspace"):
        _refused(lib, call(**{name: None}), "null", f"({name})")
    for name in ("probs", "partner", "counts"):
        _refused(lib, call(**{name: FAKE + 2}), name, "4-byte")
    _refused(lib, call(workspace=7 * FAKE + 8), "workspace", "16-byte")
    _refused(lib, call(nbytes=255), "workspace of 255 bytes", "256 needed")
    _refused(lib, call(L=1025, nbytes=139519), "139520 needed")
    _refused(lib, call(L=4096, nbytes=(2 << 20) - 1), "2097152 needed")


def test_refusals_of_the_text(lib):
    def call(probs=FAKE, L=8, text=2 * FAKE, fallback=3 * FAKE):
        return lib.rnamsm_ss_prob_text_long(probs, L, text, fallback, None)

    _refused(lib, call(L=0), "ss_prob_text_long:", "L=0", "[1, 4096]")
    _refused(lib, call(L=4097), "L=4097")
    for name in ("probs", "text", "fallback"):
        _refused(lib, call(**{name: None}), "ss_prob_text_long:", "null")
    _refused(lib, call(probs=FAKE + 2), "probs", "4-byte")
    _refused(lib, call(fallback=FAKE + 2), "fallback", "4-byte")
    _refused(lib, call(text=2 * FAKE + 8), "text", "16-byte")
    _refused(lib, lib.rnamsm_ss_prob_text(FAKE, 1025, 2 * FAKE, 3 * FAKE, None), "ss_prob_text:", "L=1025", "[1, 1024]")


def test_refusals_of_the_contact_head(lib):
    def call(atp=FAKE, stride=4096 * 4096, L=8, nch=120, weight=2 * FAKE, bias=3 * FAKE, contacts=4 * FAKE, workspace=5 * FAKE,
             nbytes=1 << 22):
        return lib.rnamsm_contact_head_long(atp, stride, L, nch, weight, bias, contacts, workspace, nbytes, None)

    _refused(lib, call(L=0), "contact_head_long:", "L=0", "[1, 4096]")
    _refused(lib, call(L=4097), "L=4097")
    _refused(lib, call(nch=0), "nch=0")
    for name in ("atp", "weight", "bias", "contacts", "workspace"):
        _refused(lib, call(**{name: None}), "null", f"({name})")
    _refused(lib, call(L=100, stride=9999), "plane stride 9999", "10000")
    for name in ("atp", "contacts", "workspace"):
        _refused(lib, call(**{name: FAKE + 2}), name, "4-byte")
    _refused(lib, call(L=4096, nbytes=4 * (120 * 4096 + 120) - 1), "workspace of 1966559 bytes", "1966560 needed")
    _refused(lib, lib.rnamsm_contact_head_atp(FAKE, 1 << 24, 1024, 120, 2 * FAKE, 3 * FAKE, 4 * FAKE, 5 * FAKE, 1 << 22, None),
             "contact_head_atp:", "L=1024", "[1, 1023]")


def test_refusals_of_the_ss_head(lib):
    table = (ctypes.c_void_p * 12)(*[FAKE * (16 + k) for k in range(12)])

    def call(atp=FAKE, stride=4096 * 4096, codes=2 * FAKE, L=8, blocks=1, weights=table, logits=3 * FAKE, probs=4 * FAKE,
             workspace=5 * FAKE, nbytes=1 << 40):
        return lib.rnamsm_ss_head_long(atp, stride, codes, L, blocks, weights, logits, probs, workspace, nbytes, None)

    _refused(lib, call(L=0), "ss_head_long:", "L=0", "[1, 4096]")
    _refused(lib, call(L=4097), "L=4097")
    for name in ("atp", "codes", "weights", "workspace"):
        _refused(lib, call(**{name: None}), "ss_head_long:", "null")
    _refused(lib, call(logits=None, probs=None), "neither logits nor probs")
    _refused(lib, call(blocks=0), "num_blocks=0")
    _refused(lib, call(L=100, stride=9999), "plane stride 9999")
    _refused(lib, call(L=4096, nbytes=2 * 48 * 4 * 4096 * 4096 - 1), "workspace too small")
    _refused(lib, call(workspace=5 * FAKE + 8), "16-byte", "workspace")
    _refused(lib, lib.rnamsm_ss_head(FAKE, 1 << 24, 2 * FAKE, 1025, 1, table, 3 * FAKE, 4 * FAKE, 5 * FAKE, 1 << 40, None),
             "ss_head:", "L=1025", "[1, 1024]")


def test_the_contact_head_on_stripped_maps_refuses_misaligned_pointers(lib):
    """The lone entry holds the long one's alignment refusals, under its own name."""
    def call(atp=FAKE, contacts=4 * FAKE, workspace=5 * FAKE):
        return lib.rnamsm_contact_head_atp(atp, 1 << 20, 8, 120, 2 * FAKE, 3 * FAKE, contacts, workspace, 1 << 22, None)

    for name in ("atp", "contacts", "workspace"):
        _refused(lib, call(**{name: FAKE * 9 + 2}), "contact_head_atp:", name, "4-byte")
        _refused(lib, call(**{name: FAKE * 9 + 1}), "contact_head_atp:", name, "4-byte")


# Each pair of lone entries is one function under two names and limits: the bad arguments of a pair in the order of its checks, as
# (overrides of the good call, words of the refusal).  "over" stands for the entry's own limit + 1.
def _rsa_table(hole=None):
    t = (ctypes.c_void_p * (4 + 26 * 3))(*[FAKE * (32 + k) for k in range(4 + 26 * 3)])
    if hole is not None:
        t[hole] = None
    return t


PAIRS = {
    "contact": dict(
        entries=(("contact_head_atp", 1023), ("contact_head_long", 4096)),
        args=("atp", "stride", "L", "nch", "weight", "bias", "contacts", "workspace", "nbytes"),
        good=dict(atp=FAKE, stride=1 << 24, L=8, nch=120, weight=2 * FAKE, bias=3 * FAKE, contacts=4 * FAKE, workspace=5 * FAKE,
                  nbytes=1 << 22),
        bad=[(dict(atp=None), ("null", "(atp)")), (dict(weight=None), ("null", "(weight)")), (dict(bias=None), ("null", "(bias)")),
             (dict(contacts=None), ("null", "(contacts)")), (dict(workspace=None), ("null", "(workspace)")),
             (dict(L=0), ("L=0",)), (dict(L="over"), ("outside [1,",)), (dict(nch=0), ("nch=0",)),
             (dict(stride=63), ("plane stride 63", "64")), (dict(atp=FAKE + 2), ("atp", "4-byte")),
             (dict(contacts=4 * FAKE + 2), ("contacts", "4-byte")), (dict(workspace=5 * FAKE + 2), ("workspace", "4-byte")),
             (dict(nbytes=4 * (120 * 8 + 120) - 1), ("workspace too small", "workspace of 4319 bytes", "4320 needed"))]),
    "rsa": dict(
        entries=(("rsa_head", 1024), ("rsa_head_long", 4096)),
        args=("emb", "stride", "codes", "L", "K", "onehot", "weights", "probs", "logits", "workspace", "nbytes"),
        good=dict(emb=FAKE, stride=768, codes=2 * FAKE, L=8, K=3, onehot=1, weights=_rsa_table(), probs=3 * FAKE, logits=4 * FAKE,
                  workspace=5 * FAKE, nbytes=1 << 30),
        bad=[(dict(emb=None), ("null", "(emb)")), (dict(codes=None), ("null", "(base_codes)")), (dict(weights=None), ("null", "(weights)")),
             (dict(workspace=None), ("null", "(workspace)")), (dict(probs=None, logits=None), ("neither probs nor logits",)),
             (dict(L=0), ("L=0",)), (dict(L="over"), ("outside [1,",)), (dict(K=9), ("n_models=9",)),
             (dict(stride=767), ("row stride 767",)), (dict(nbytes=1023), ("workspace of 1023 bytes", "needed")),
             (dict(emb=FAKE + 8), ("emb", "16-byte")), (dict(workspace=5 * FAKE + 8), ("workspace", "16-byte")),
             (dict(probs=3 * FAKE + 2), ("probs", "4-byte")), (dict(logits=4 * FAKE + 2), ("logits", "4-byte")),
             (dict(weights=_rsa_table(35)), ("weight pointer 35 is null",))]),
    "ss": dict(
        entries=(("ss_head", 1024), ("ss_head_long", 4096)),
        args=("atp", "stride", "codes", "L", "blocks", "weights", "logits", "probs", "workspace", "nbytes"),
        good=dict(atp=FAKE, stride=1 << 24, codes=2 * FAKE, L=8, blocks=1, weights=(ctypes.c_void_p * 12)(*[FAKE * (16 + k) for k in range(12)]),
                  logits=3 * FAKE, probs=4 * FAKE, workspace=5 * FAKE, nbytes=1 << 40),
        bad=[(dict(atp=None), ("null",)), (dict(logits=None, probs=None), ("neither logits nor probs",)), (dict(L=0), ("L=0",)),
             (dict(L="over"), ("outside [1,",)), (dict(blocks=0), ("num_blocks=0",)), (dict(stride=63), ("plane stride 63",)),
             (dict(nbytes=1023), ("workspace too small",)), (dict(workspace=5 * FAKE + 8), ("16-byte", "workspace"))]),
}


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_both_entries_of_a_pair_refuse_the_same_bad_argument_at_the_same_place(lib, pair):
    """Every bad argument alone, and together with all that a later check would refuse: both entries answer with the earliest check's
    refusal, under their own name and with their own limit."""
    p = PAIRS[pair]
    for name, max_L in p["entries"]:
        fn = getattr(lib, "rnamsm_" + name)
        for i, (bad, words) in enumerate(p["bad"]):
            later = {}
            for more, _ in reversed(p["bad"][i + 1:]):
                later.update(more)
            for overrides in (bad, {**later, **bad}):
                kw = {**p["good"], **overrides}
                if kw["L"] == "over":
                    kw["L"] = max_L + 1
                _refused(lib, fn(*(kw[a] for a in p["args"]), None), name + ":", *words)
                if bad.get("L") == "over":
                    _refused(lib, fn(*(kw[a] for a in p["args"]), None), f"L={max_L + 1}", f"[1, {max_L}]")


# ---------------------------------------------------------------------- ss_pairs_long.h on the host
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host check of ss_pairs_long.h"
    exe = str(tmp_path_factory.mktemp("ss_pairs_long") / "ss_pairs_long_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "ss_pairs_long_check.cpp"), "-o", exe], check=True)
    return exe


def _decode(program, tmp_path, cases):
    """cases: [(prob, seq)] -> [(partner, counts, ct body, bpseq body)] from the program."""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for prob, seq in cases:
            L = len(seq)
            assert prob.shape == (L, L) and prob.dtype == np.float32
            f.write(np.int32(L).tobytes() + bytes(ss.letter_codes(seq)) + np.ascontiguousarray(prob).tobytes())
    res = subprocess.run([program, str(src), str(dst)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    blob, at, out = dst.read_bytes(), 0, []
    for _, seq in cases:
        L = len(seq)
        partner = np.frombuffer(blob, dtype=np.int32, count=L, offset=at)
        counts = np.frombuffer(blob, dtype=np.int32, count=4, offset=at + 4 * L)
        at += 4 * L + 16
        ct, bp = blob[at:at + counts[1]], blob[at + counts[1]:at + counts[1] + counts[2]]
        at += int(counts[1]) + int(counts[2])
        out.append((partner, counts, ct, bp))
    assert at == len(blob)
    return out


def _check(program, tmp_path, named):
    """named: [(key, prob, seq)]: the program's four results against the host function and writer."""
    got = _decode(program, tmp_path, [(p, s) for _, p, s in named])
    for (key, prob, seq), (partner, counts, ct, bp) in zip(named, got):
        pairs, want_partner, want_ct, want_bp, _, _ = C.expected(key, prob, seq)
        assert partner.tolist() == want_partner.tolist(), key
        assert counts.tolist() == [len(pairs), len(want_ct), len(want_bp), 0], key
        assert ct == want_ct and bp == want_bp, key


def test_one_base_per_thread_is_the_existing_decoding(program, tmp_path):
    """L <= 1024: thread t owns base t.  The standard cases (L = 1 among them) and the L = 1024 matrix of the existing kernel's test."""
    named = [(k, p, s) for k, (p, s) in C.standard_cases().items()] + [("helix_1024", C.helix_noise_1024(), C.seq_for(1024, 9))]
    assert any(len(s) == 1 for _, _, s in named)
    _check(program, tmp_path, named)


@pytest.mark.parametrize("L", [1025, 2049, 2304])
def test_several_bases_per_thread(program, tmp_path, L):
    """1025: the first base beyond one per thread (two per thread, the last threads idle); 2049: three for thread 0; 2304: the .ct
    body is longer than a 16-bit offset reaches."""
    named = [LC.case(kind, L) for kind in ("helix", "blocks", "thin")]
    for key, prob, seq in named:
        pairs = C.expected(key, prob, seq)[0]
        assert 0 < len(pairs) < LC.edges_above(prob), key                 # the host function removed at least one pair
    key, prob, seq = named[0]
    pairs, partner, want_ct, _, _, _ = C.expected(key, prob, seq)
    assert (300, 802) in pairs and (300, 800) not in pairs and (300, 801) not in pairs      # the planted multiplet: two rounds
    assert (998, 1024) in pairs or L == 1025                              # 999 as an index and as a partner (line 1025)
    assert (800, 999) in pairs and partner[999] == 801 and partner[800] == 1000             # 1000 as an index and as a partner
    if L == 2304:
        assert len(want_ct) > 65536
    _check(program, tmp_path, named)


def test_a_letter_outside_ascii_sets_the_fallback_word_beyond_one_base_per_thread(program, tmp_path):
    key, prob, seq = LC.case("thin", 1025)
    seq = seq[:1024] + "é"                                                # the one base of the last busy thread's second slot
    (partner, counts, _, _), = _decode(program, tmp_path, [(prob, seq)])
    assert counts[3] == 1 and partner.tolist() == C.expected(key, prob, LC.case("thin", 1025)[2])[1].tolist()


# ---------------------------------------------------------------------- the configuration
def test_config_key_parses_defaults_to_skip_and_refuses_other_words():
    assert Config().data.long_heads == "skip"
    assert parse_overrides(["data.long_heads=stitched"]).data.long_heads == "stitched"
    assert parse_overrides(["data.long_heads=skip"]).data.long_heads == "skip"
    with pytest.raises(ValueError, match="long_heads"):
        parse_overrides(["data.long_heads=windows"])
