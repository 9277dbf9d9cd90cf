"""The device-written RSA_result tables without a GPU: csrc/rsa_text.h compiled into a stand-alone program (tests/native/
rsa_text_check.cpp: "%.2f" / "%.3f" in integers against snprintf, plain and under AddressSanitizer + UBSan), the Python model of
the contract (rsa_text_cases.model) against write_rsa_files byte for byte, the C ABI's symbols, sizes and refusals (made before
anything is enqueued, on fabricated addresses that are never dereferenced), the config key, the head's switch and the writer job
with a hand-made text record."""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import rsa_text_cases as C
from rnamsm import _lib, config, rsa
from rnamsm.alphabet import RNAAlphabet

FAKE = 0x10000
SRC = os.path.join(ROOT, "tests", "native", "rsa_text_check.cpp")
ALPHABET = RNAAlphabet.from_architecture("rna language")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---------------------------------------------------------------------- the formatter header on the host
def _build(tmp_path_factory, tag, flags):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host check of rsa_text.h"
    exe = str(tmp_path_factory.mktemp("rsa_text_" + tag) / "rsa_text_check")
    subprocess.run([cxx, "-std=c++17", *flags, SRC, "-o", exe], check=True)
    return exe


def test_formatter_against_snprintf(tmp_path_factory):
    """Every tie below 512 with both neighbours, the carries, the subnormal end, dense float32 windows and 10^7 seeded products and
    quotients (2 500 000 float32 values x {350, 400} and those / 3)."""
    exe = _build(tmp_path_factory, "plain", ["-O2"])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    n = int(res.stdout.split()[1])
    assert n > 10_000_000 + 3 * (8 + 16) * 512, res.stdout


def test_formatter_under_sanitizers(tmp_path_factory):
    """The same program under AddressSanitizer + UBSan (every field is written into a heap block of exactly its length; a shift
    of 64 or a signed overflow would stop it); the seeded sweep is shorter here, everything else is the same."""
    exe = _build(tmp_path_factory, "asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    res = subprocess.run([exe, "200000"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]


# ---------------------------------------------------------------------- the model of the contract
def _model_matches_host(values, seq, name="x"):
    bodies, counts, ens = C.model(values, seq)
    want, want_ens = C.expected_bodies(values, seq, name)
    K = values.shape[0]
    assert counts[K + 1] == 0 and counts[K + 2] == 0
    assert bodies == want
    assert [int(c) for c in counts[:K + 1]] == [len(b) for b in want]
    assert np.array_equal(ens, want_ens) and ens.dtype == np.float64


def test_model_matches_the_committed_cases():
    """tests/golden/rsa/rsa_text_cases.npz: doSavePredict_single's own bytes.  Cases with a letter outside ACGUT set the fallback
    word (their files depend on the host's generator); the others match byte for byte, headers included."""
    seen = {"exact": 0, "fallback": 0}
    with np.load(os.path.join(GOLDEN, "rsa", "rsa_text_cases.npz")) as z:
        for k in z["order"]:
            values, seq, names = z[f"rsa_{k}"], str(z[f"seq_{k}"]), [str(n) for n in z[f"names_{k}"]]
            bodies, counts, _ = C.model(values, seq)
            K = len(names)
            if any(c not in "ACGUT" for c in seq):
                assert counts[K + 1] == 1 and bodies is None, k
                seen["fallback"] += 1
                continue
            assert counts[K + 1] == 0 and counts[K + 2] == 0
            for f in range(K + 1):
                tag, head = (str(f), C.header(str(k), names[f])) if f < K else ("ensemble", C.header(str(k)))
                assert head + bodies[f] == z[f"text_{k}_{tag}"].tobytes(), (k, tag)
            seen["exact"] += 1
    assert seen["exact"] >= 3 and seen["fallback"] >= 3, seen


@pytest.mark.parametrize("K", C.KS)
def test_model_matches_write_rsa_files_on_random_values(K):
    for L, seed in ((1, 0), (10, 1), (101, 2), (257, 3)):
        _model_matches_host(C.uniform_values(K, L, seed + 10 * K), C.seq_for(L, seed))
    _model_matches_host(C.special_table(K, 300, K), C.seq_for(300, 9))
    _model_matches_host(C.special_table(K, 300, K + 5), "G" * 300)
    _model_matches_host(C.special_table(K, 300, K + 7), "U" * 300)


def test_model_flags():
    good = C.uniform_values(3, 9, 1)
    seq = C.seq_for(9, 1)
    assert C.model(good, seq)[1][4] == 0
    for bad in (np.nan, np.inf, -np.inf, -0.0, -0.25, np.nextafter(np.float32(1), np.float32(2)), 2.0):
        for p in (0, 4, 8):
            v = good.copy()
            v[1, p] = bad
            bodies, counts, ens = C.model(v, seq)
            assert counts[4] == 1 and bodies is None and ens is None, (bad, p)
    for letter in "XNacgu-":
        for p in (0, 4, 8):
            assert C.model(good, seq[:p] + letter + seq[p + 1:])[1][4] == 1, (letter, p)
    v = good.copy()
    v[2, 5] = 0.0
    bodies, counts, _ = C.model(v, seq)
    assert counts[4] == 0 and counts[5] == 1 and bodies is not None
    with pytest.raises(_lib.RnamsmError):                         # the host raises where the zero word is set
        C.expected_files(v, seq)


# ---------------------------------------------------------------------- C ABI
def test_symbols_and_sizes(lib):
    assert {"rnamsm_rsa_text_bytes", "rnamsm_rsa_text", "rnamsm_rsa_text_packed"} <= set(_lib.EXPORTED_SYMBOLS)
    assert ctypes.sizeof(_lib.RsaTextItem) == 48 and _lib.RSA_TEXT_LINE_MAX == C.LINE_MAX == 23
    for L in (1, 35, 1024):
        for K in (1, 3, 8):
            assert lib.rnamsm_rsa_text_bytes(L, K) == (K + 1) * 23 * L
    for L, K in ((0, 3), (1025, 3), (8, 0), (8, 9), (-1, 1)):
        assert lib.rnamsm_rsa_text_bytes(L, K) == 0
    assert lib.rnamsm_version() == 600


def _refused(lib, rc, *needles):
    assert rc == -1, rc
    msg = lib.rnamsm_last_error().decode()
    for n in needles:
        assert n in msg, (n, msg)


def test_refusals_on_a_host_without_a_gpu(lib):
    F = FAKE
    _refused(lib, lib.rnamsm_rsa_text(F, 2 * F, 0, 3, 3 * F, 4 * F, 5 * F, None), "L=0")
    _refused(lib, lib.rnamsm_rsa_text(F, 2 * F, 1025, 3, 3 * F, 4 * F, 5 * F, None), "L=1025")
    _refused(lib, lib.rnamsm_rsa_text(F, 2 * F, 8, 0, 3 * F, 4 * F, 5 * F, None), "n_models=0")
    _refused(lib, lib.rnamsm_rsa_text(F, 2 * F, 8, 9, 3 * F, 4 * F, 5 * F, None), "n_models=9")
    for at in range(4):                                           # rsa, letters, text, counts; ens may be null
        args = [F, 2 * F, 8, 3, 3 * F, 4 * F, 5 * F, None]
        args[at if at < 2 else at + 2] = None
        _refused(lib, lib.rnamsm_rsa_text(*args), "null")
    _refused(lib, lib.rnamsm_rsa_text(F + 2, 2 * F, 8, 3, 3 * F, 4 * F, 5 * F, None), "4-byte")
    _refused(lib, lib.rnamsm_rsa_text(F, 2 * F, 8, 3, 3 * F, 4 * F + 2, 5 * F, None), "4-byte")
    _refused(lib, lib.rnamsm_rsa_text(F, 2 * F, 8, 3, 3 * F + 8, 4 * F, 5 * F, None), "16-byte")
    _refused(lib, lib.rnamsm_rsa_text(F, 2 * F, 8, 3, 3 * F, 4 * F, 5 * F + 4, None), "8-byte")

    def items(n):
        arr = (_lib.RsaTextItem * n)()
        for b in range(n):
            arr[b] = _lib.RsaTextItem(F * (8 * b + 1), F * (8 * b + 2), 8, F * (8 * b + 3), F * (8 * b + 4), F * (8 * b + 5))
        return arr

    _refused(lib, lib.rnamsm_rsa_text_packed(items(1), 0, 3, None), "B=0")
    _refused(lib, lib.rnamsm_rsa_text_packed(items(1025), 1025, 3, None), "B=1025")
    _refused(lib, lib.rnamsm_rsa_text_packed(None, 3, 3, None), "null")
    _refused(lib, lib.rnamsm_rsa_text_packed(items(2), 2, 0, None), "n_models=0")
    _refused(lib, lib.rnamsm_rsa_text_packed(items(2), 2, 9, None), "n_models=9")
    for member in (0, 1, 32, 39):                                 # on either side of the 32-descriptor chunk
        for field, value, needle in (("L", 0, "L=0"), ("L", 1025, "L=1025"), ("rsa", None, "null"), ("letters", None, "null"),
                                     ("text", None, "null"), ("counts", None, "null"), ("text", F + 8, "16-byte"),
                                     ("rsa", F + 1, "4-byte"), ("counts", F + 2, "4-byte"), ("ens", F + 4, "8-byte")):
            arr = items(40)
            setattr(arr[member], field, value)
            _refused(lib, lib.rnamsm_rsa_text_packed(arr, 40, 3, None), f"member {member}:", needle)


def test_ops_refuse_host_tensors_and_bad_shapes():
    from rnamsm import ops
    with pytest.raises(_lib.RnamsmError):
        ops.rsa_text(torch.zeros(3, 8), torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(_lib.RnamsmError):
        ops.rsa_text_packed([torch.zeros(3, 8)], [torch.zeros(8, dtype=torch.uint8)])
    assert ops.rsa_text_packed([], []) == []
    with pytest.raises(ValueError):
        ops.rsa_text_packed([torch.zeros(3, 8)], [])


# ---------------------------------------------------------------------- config, head, writer job
def test_config_key():
    assert config.Config().data.rsa_text_device is True
    assert config.parse_overrides(["data.rsa_text_device=false"]).data.rsa_text_device is False
    assert config.parse_overrides(["data.rsa_text_device=true"]).data.rsa_text_device is True


def _tokens(seq: str) -> torch.Tensor:
    return torch.tensor([ALPHABET.get_idx(c) for c in seq], dtype=torch.int64)


def test_result_and_head_switch():
    v, t = torch.zeros(3, 5), _tokens("ACGUA")
    rec = rsa.RSAResult(v, t)
    assert rec.text is None and tuple(rec) == (v, t, None)
    off = rsa.RSAHead(None, ALPHABET, None, None, model_names=["a", "b", "c"])
    assert off.text_on is False and off.n_tensors == 2 and off.letters_lut is None
    assert off.flatten(rec) == [v, t] and off.unflatten([v, t]) == rec
    on = rsa.RSAHead(None, ALPHABET, None, None, model_names=["a", "b", "c"], text_on=True, device="cpu")
    assert on.n_tensors == 5
    assert bytes(on.letters_lut[t].tolist()) == b"ACGUA"
    assert all(int(on.letters_lut[ALPHABET.get_idx(tok)]) == 0 for tok in ALPHABET.all_toks if len(tok) != 1)
    text = (torch.zeros(4 * 23 * 5, dtype=torch.uint8), torch.zeros(6, dtype=torch.int32), torch.zeros(2, 5, dtype=torch.float64))
    full = rsa.RSAResult(v, t, text)
    flat = on.flatten(full)
    assert len(flat) == 5 and all(isinstance(x, torch.Tensor) for x in flat)
    back = on.unflatten(flat)
    assert all(a is b for a, b in zip(on.flatten(back), flat)) and back.values is v and back.tokens is t
    with pytest.raises(ValueError):
        on.unflatten(flat[:2])
    with pytest.raises(ValueError):
        off.unflatten(flat)


def _run_sequentially(job) -> None:
    fn, tensors = job                                   # extract_feat.emit, async_io=False
    fn(*(t.cpu().numpy() for t in tensors))


def _job_record(values, seq, name, word=0, zero=0, junk=False):
    text, counts, ens = C.text_record_from_host(values, seq, name)
    K = values.shape[0]
    counts[K + 1], counts[K + 2] = word, zero
    if junk:
        text[:] = ord("?")
    return rsa.RSAResult(torch.from_numpy(values), _tokens(seq), (torch.from_numpy(text), torch.from_numpy(counts), torch.from_numpy(ens)))


def test_rsa_jobs_with_a_text_record_write_the_host_path_s_files_and_draw_in_order(tmp_path):
    """The device-route twin of test_cli_heads_host's RSA job test: three alignments in a row, the middle one with its fallback word
    set (its text is junk and must not be used) and an X in its query, which the host path replaces by its draw: the draws of the
    device route before it decide that letter's scale, so they have to have been taken."""
    names = C.NAMES8[:3]
    seqs = {"a": C.seq_for(12, 3, t_every=99), "b": "ACGXUXGCA", "c": C.seq_for(30, 5, t_every=99)}      # (the alphabet has no T)
    values = {i: C.uniform_values(3, len(s), n) for n, (i, s) in enumerate(seqs.items())}
    head = rsa.RSAHead(None, ALPHABET, None, random.Random(2022), model_names=names, text_on=True, device="cpu")
    want_rng = random.Random(2022)
    for i, s in seqs.items():
        v = values[i]
        rec = _job_record(v, "ACGAUAGCA" if i == "b" else s, i, word=1, junk=True)._replace(tokens=_tokens(s)) if i == "b" \
            else _job_record(v, s, i)
        job = head.writer_job(rec, i, tmp_path / "job")
        assert len(job[1]) == head.n_tensors
        _run_sequentially(job)
        rsa.write_rsa_files(v, s, i, tmp_path / "host", names, want_rng)
    got = C.tree(tmp_path / "job")
    assert len(got) == 3 * 4 and got == C.tree(tmp_path / "host")
    assert head.rng.random() == want_rng.random()


def test_write_rsa_files_uses_the_text_as_it_is_and_checks_it(tmp_path):
    v, s = C.uniform_values(2, 7, 4), "ACGUTAC"
    text, counts, ens = C.text_record_from_host(v, s)
    marked = text.copy()
    marked[0] ^= 1                                                # the text is written, not re-derived
    got_ens = rsa.write_rsa_files(v, s, "x", tmp_path / "m", C.NAMES8[:2], random.Random(0), text=(marked, counts, ens))
    data = (tmp_path / "m" / "RSA_result" / "x_0" / "x.txt").read_bytes()
    assert data == C.header("x", C.NAMES8[0]) + bytes(marked[:counts[0]])
    assert np.array_equal(got_ens[0], ens[0]) and np.array_equal(got_ens[1], ens[1])
    with pytest.raises(ValueError):
        rsa.write_rsa_files(v, s, "x", tmp_path / "n", C.NAMES8[:2], random.Random(0), text=(text[:-1], counts, ens))
    with pytest.raises(ValueError):
        rsa.write_rsa_files(v, s, "x", tmp_path / "n", C.NAMES8[:2], random.Random(0), text=(text, counts[:-1], ens))
    zero = counts.copy()
    zero[4] = 1                                                   # zero word: the host path decides (here: nothing is zero, files as usual)
    rsa.write_rsa_files(v, s, "x", tmp_path / "z", C.NAMES8[:2], random.Random(0), text=(np.full_like(text, 63), zero, ens))
    rsa.write_rsa_files(v, s, "x", tmp_path / "h", C.NAMES8[:2], random.Random(0))
    assert C.tree(tmp_path / "z") == C.tree(tmp_path / "h")
    # a name np.savetxt would not write as ASCII goes the host way whatever the words say
    rsa.write_rsa_files(v, s, "é", tmp_path / "u", C.NAMES8[:2], random.Random(0), text=(np.full_like(text, 63), counts, ens))
    rsa.write_rsa_files(v, s, "é", tmp_path / "uh", C.NAMES8[:2], random.Random(0))
    assert C.tree(tmp_path / "u") == C.tree(tmp_path / "uh")


def test_a_zero_raises_from_the_host_path_with_a_text_record(tmp_path):
    v, s = C.uniform_values(2, 7, 4), "ACGUTAC"
    text, counts, ens = C.text_record_from_host(v, s)
    v = v.copy()
    v[1, 3] = 0.0
    counts[4] = 1
    with pytest.raises(_lib.RnamsmError, match="error in predict"):
        rsa.write_rsa_files(v, s, "x", tmp_path, C.NAMES8[:2], random.Random(0), text=(text, counts, ens))
