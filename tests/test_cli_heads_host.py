"""The CLI's head records on the host (rnamsm.ss.SSHead / SSResult, rnamsm.rsa.RSAHead / RSAResult): a record's writer job, run
the way extract_feat's sequential branch runs it, writes the files of write_ss_files / write_rsa_files called the old way, byte
for byte; flatten / unflatten are inverses and count what the gather is told.  No GPU and no library: the "device" is the CPU, the
text and the bodies come from the host path itself."""
import io
import os
import random

import numpy as np
import pytest
import torch

import ss_pairs_cases as C
from rnamsm import rsa, ss
from rnamsm.alphabet import RNAAlphabet

ALPHABET = RNAAlphabet.from_architecture("rna language")
L = 12
PROB, SEQ = C.ties(L, seed=3), C.seq_for(L, 3)
SWITCHES = [(False, False), (True, False), (False, True), (True, True)]


def _tokens(seq: str) -> torch.Tensor:
    return torch.tensor([ALPHABET.get_idx(c) for c in seq], dtype=torch.int64)


def _record(text_on: bool, pairs_on: bool, word: int = 0, table_fallback: int = 0, junk: bool = False) -> ss.SSResult:
    """PROB's record with CPU tensors: the text is np.savetxt's, the bodies are those of write_ss_files called the old way.
    junk: the text and the bodies are filled with '?' instead (they must not be used)."""
    pairs, partner, ct, bp, _, _ = C.expected("cli_heads_ties_12", PROB, SEQ)
    assert pairs and len(pairs) < int((np.triu(PROB, 1) > ss.THRESHOLD).sum())         # a pair is kept, a multiplet is resolved
    buf = io.BytesIO()
    np.savetxt(buf, PROB, delimiter="\t")
    text = np.frombuffer(buf.getvalue(), dtype=np.uint8).copy()
    assert text.shape == (25 * L * L,)
    bodies = [np.full(n * L, ord("?"), dtype=np.uint8) for n in (32, 12)]
    if junk:
        text[:] = ord("?")
    else:
        bodies[0][:len(ct)] = np.frombuffer(ct, dtype=np.uint8)
        bodies[1][:len(bp)] = np.frombuffer(bp, dtype=np.uint8)
    counts = np.array([len(pairs), len(ct), len(bp), table_fallback], dtype=np.int32)
    t = torch.from_numpy
    return ss.SSResult(t(PROB), _tokens(SEQ), (t(text), t(np.array([word], dtype=np.int32))) if text_on else None,
                       (t(partner), t(counts), t(bodies[0]), t(bodies[1])) if pairs_on else None)


def _run_sequentially(job) -> None:
    fn, tensors = job                                   # extract_feat.emit, async_io=False
    fn(*(t.cpu().numpy() for t in tensors))


def _ss_files(root, name="x"):
    return {ext: (root / "SS_result" / f"{name}.{ext}").read_bytes() for ext in ("prob", "ct", "bpseq")}


@pytest.fixture(scope="module")
def host_files(tmp_path_factory):
    root = tmp_path_factory.mktemp("cli_heads_host")
    ss.write_ss_files(PROB, SEQ, "x", root)
    return _ss_files(root)


def _head(text_on, pairs_on):
    return ss.SSHead(None, ALPHABET, None, "cpu", text_on=text_on, pairs_on=pairs_on)


@pytest.mark.parametrize("text_on, pairs_on", SWITCHES)
def test_ss_job_writes_the_host_path_s_files(tmp_path, host_files, text_on, pairs_on):
    head, fetched = _head(text_on, pairs_on), []
    rec = _record(text_on, pairs_on)
    fn, tensors = head.writer_job(rec, "x", tmp_path, fetch_probs=lambda: fetched.append(1) or PROB)
    square = [t for t in tensors if t.dim() == 2 and t.dtype == torch.float32]
    assert len(square) == (0 if text_on and pairs_on else 1)                 # both on: the probabilities are not enqueued
    assert len(tensors) == head.n_tensors - (text_on and pairs_on)
    _run_sequentially((fn, tensors))
    assert _ss_files(tmp_path) == host_files
    assert fetched == []                                                      # fallback word 0: never fetched


@pytest.mark.parametrize("text_on, pairs_on", [(True, False), (True, True)])
def test_ss_job_with_the_prob_fallback_word_set(tmp_path, host_files, text_on, pairs_on):
    """Word 1: the text (junk here) is not used; with both switches on the probabilities are fetched, exactly once."""
    fetched = []
    rec = _record(text_on, pairs_on, word=1, junk=True)._replace(structure=_record(text_on, pairs_on).structure)
    _run_sequentially(_head(text_on, pairs_on).writer_job(rec, "x", tmp_path, fetch_probs=lambda: fetched.append(1) or PROB))
    assert _ss_files(tmp_path) == host_files
    assert len(fetched) == (1 if pairs_on else 0)


def test_ss_job_default_fetch_reads_the_record(tmp_path, host_files):
    rec = _record(True, True, word=1, junk=True)._replace(structure=_record(True, True).structure)
    _run_sequentially(_head(True, True).writer_job(rec, "x", tmp_path))
    assert _ss_files(tmp_path) == host_files


@pytest.mark.parametrize("text_on", [False, True])
def test_ss_job_with_the_tables_fallback_count_set(tmp_path, host_files, text_on):
    """counts[3] == 1: the bodies (junk here) are not used, the host builder writes the tables from the partner vector."""
    rec = _record(text_on, True, table_fallback=1, junk=True)._replace(text=_record(text_on, True).text)
    _run_sequentially(_head(text_on, True).writer_job(rec, "x", tmp_path))
    assert _ss_files(tmp_path) == host_files


def _tree(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def test_rsa_jobs_write_the_host_path_s_files_and_draw_in_order(tmp_path):
    names = [f"model_pcc_{k}.pt" for k in range(3)]
    seqs = {"a": SEQ, "b": C.seq_for(9, 4)}
    values = {i: np.random.RandomState(n).uniform(0.05, 0.95, size=(3, len(s))).astype(np.float32) for n, (i, s) in enumerate(seqs.items())}
    head = rsa.RSAHead(None, ALPHABET, None, random.Random(2022), model_names=names)
    want_rng = random.Random(2022)
    for i, s in seqs.items():
        rec = rsa.RSAResult(torch.from_numpy(values[i]), _tokens(s))
        _run_sequentially(head.writer_job(rec, i, tmp_path / "job"))
        rsa.write_rsa_files(values[i], s, i, tmp_path / "host", names, want_rng)
    got = _tree(tmp_path / "job")
    assert len(got) == 2 * 4 and got == _tree(tmp_path / "host")
    assert head.rng.random() == want_rng.random()


@pytest.mark.parametrize("text_on, pairs_on", SWITCHES)
def test_flatten_and_unflatten_are_inverses(text_on, pairs_on):
    head, rec = _head(text_on, pairs_on), _record(text_on, pairs_on)
    flat = head.flatten(rec)
    assert len(flat) == head.n_tensors == 2 + 2 * text_on + 4 * pairs_on and all(isinstance(t, torch.Tensor) for t in flat)
    back = head.unflatten(flat)
    assert (back.text is None) == (not text_on) and (back.structure is None) == (not pairs_on)
    assert back.probs is rec.probs and back.tokens is rec.tokens
    assert len(head.flatten(back)) == len(flat) and all(a is b for a, b in zip(head.flatten(back), flat))
    r = rsa.RSAHead(None, ALPHABET, None, None, model_names=["m"])
    rr = rsa.RSAResult(torch.zeros(1, L), _tokens(SEQ))
    assert r.unflatten(r.flatten(rr)) is not rr and all(a is b for a, b in zip(r.unflatten(r.flatten(rr)), rr))


def test_n_tensors_with_the_switches_off():
    """What the heads report with the formatter and the decoding off, as they are under gather_to_rank0: two tensors each, so an
    item of emb, atp and the flattened records is 2, 4 or 6 tensors.  (That extract_feat hands this sum to the RoundGatherer is the
    gather_to_rank0 tests' matter, test_gpu_cli.py.)"""
    ss_head, rsa_head = _head(False, False), rsa.RSAHead(None, ALPHABET, None, None, model_names=["m"])
    assert ss_head.n_tensors == 2 and rsa_head.n_tensors == 2
    for heads, n in (([], 2), ([ss_head], 4), ([rsa_head], 4), ([ss_head, rsa_head], 6)):
        assert 2 + sum(h.n_tensors for h in heads) == n
    with pytest.raises(ValueError):
        ss_head.unflatten([torch.zeros(1)] * 3)
