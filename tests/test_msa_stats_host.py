"""Alignment statistics (rnamsm_msa_pdist, rnamsm_msa_neff, rnamsm_msa_coverage; data.msa_stats) without a GPU: the symbols in the
header, the binding and the built library's export list; the size functions at and outside the limits; every refusal the entry points
make before anything is enqueued (on fabricated aligned addresses that are never dereferenced); csrc/msa_words.h -- the word form
and the per-word mismatch count -- compiled into a stand-alone program (tests/native/msa_pdist_words_check.cpp) with g++ and
AddressSanitizer + UBSan; the key in the configuration; and the numpy restatement (tests/msa_stats_truth.py) against the reference's
own MSA class (tests/golden/msa_stats_reference_2drb64.npz, made by tests/golden/make_golden_msa_stats.py) and against scipy."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden
from rnamsm import _lib, inference, msa, ops
from rnamsm.config import Config, check_msa_stats, parse_overrides
import msa_stats_truth as T

NEW = ("rnamsm_msa_pdist_workspace_bytes", "rnamsm_msa_pdist", "rnamsm_msa_neff_workspace_bytes", "rnamsm_msa_neff_min_workspace_bytes",
       "rnamsm_msa_neff", "rnamsm_msa_coverage")
FAKE = 0x100000                 # 256-byte aligned, never dereferenced


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
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    if nm:                      # the export list of the library as built
        exported = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(rf"\bT {name}$", exported, flags=re.M), name
    for fn in (ops.msa_pdist, ops.msa_neff, ops.msa_coverage, msa.msa_pdist, msa.msa_neff, msa.msa_coverage):
        assert callable(fn)
    assert "msa_pdist.hip" in open(os.path.join(ROOT, "rna-msm_amd", "csrc", "Makefile")).read()
    assert lib.rnamsm_version() == 600


def test_size_functions_at_and_outside_the_limits(lib):
    for size, max_n in ((lib.rnamsm_msa_pdist_workspace_bytes, 16384), (lib.rnamsm_msa_neff_workspace_bytes, 1 << 20),
                        (lib.rnamsm_msa_neff_min_workspace_bytes, 1 << 20)):
        for N, L in ((0, 8), (-3, 8), (max_n + 1, 8), (8, 0), (8, -1), (8, 32769)):
            assert size(N, L) == 0, (N, L)
        for N, L in ((1, 1), (max_n, 1), (1, 32768), (1176, 35), (10000, 512)):
            assert size(N, L) > 0, (N, L)
    for N, L in ((1, 1), (64, 64), (65, 65), (200, 513), (10000, 512), (16384, 32768)):
        rows, words = -(-N // 64) * 64, -(-(-(-L // 8)) // 8) * 8
        packed = rows * words * 8                       # the rows as 64-bit words: rows to a multiple of 64, words to one of 8
        assert lib.rnamsm_msa_pdist_workspace_bytes(N, L) == packed
        least, default = lib.rnamsm_msa_neff_min_workspace_bytes(N, L), lib.rnamsm_msa_neff_workspace_bytes(N, L)
        assert least == packed + rows * 4 + rows * 8    # the totals, and one row block's slab of the partial table
        assert least <= default <= packed + rows * 4 + max(rows * 8, 1 << 28)
        assert (default - least) % (rows * 8) == 0 and (default - least) // (rows * 8) < rows // 64
    assert lib.rnamsm_msa_neff_workspace_bytes(1 << 20, 512) < (1 << 20) * 512 + (1 << 20) * 4 + (1 << 28) + 1


def test_every_refusal_made_before_anything_is_enqueued(lib):
    N, L = 12, 9
    p_need, n_least = lib.rnamsm_msa_pdist_workspace_bytes(N, L), lib.rnamsm_msa_neff_min_workspace_bytes(N, L)

    def pdist(**kw):
        a = dict(msa=FAKE, N=N, L=L, ld=L, counts=FAKE, dist=FAKE, ws=FAKE, wsb=p_need)
        a.update(kw)
        rc = lib.rnamsm_msa_pdist(a["msa"], a["N"], a["L"], a["ld"], a["counts"], a["dist"], a["ws"], a["wsb"], None)
        return rc, lib.rnamsm_last_error().decode()

    def neff(**kw):
        a = dict(msa=FAKE, N=N, L=L, ld=L, cutoff=0.2, nn=FAKE, w=FAKE, neff=FAKE, ws=FAKE, wsb=n_least)
        a.update(kw)
        rc = lib.rnamsm_msa_neff(a["msa"], a["N"], a["L"], a["ld"], a["cutoff"], a["nn"], a["w"], a["neff"], a["ws"], a["wsb"], None)
        return rc, lib.rnamsm_last_error().decode()

    def coverage(**kw):
        a = dict(msa=FAKE, N=N, L=L, ld=L, gap=10, out=FAKE)
        a.update(kw)
        return lib.rnamsm_msa_coverage(a["msa"], a["N"], a["L"], a["ld"], a["gap"], a["out"], None), lib.rnamsm_last_error().decode()

    for call, kw, text in (
            (pdist, dict(msa=None), "msa_pdist: null pointer"),
            (pdist, dict(ws=None), "msa_pdist: null pointer"),
            (pdist, dict(N=0), "msa_pdist: N=0 outside [1, 16384]"),
            (pdist, dict(N=16385), "msa_pdist: N=16385 outside [1, 16384]"),
            (pdist, dict(L=0), "msa_pdist: L=0 outside [1, 32768]"),
            (pdist, dict(L=32769, ld=32769), "msa_pdist: L=32769 outside [1, 32768]"),
            (pdist, dict(ld=8), "msa_pdist: ld=8 is smaller than L=9"),
            (pdist, dict(counts=None, dist=None), "msa_pdist: counts and dist are both null: nothing to write"),
            (pdist, dict(wsb=p_need - 1), f"msa_pdist: workspace of {p_need - 1} bytes too small ({p_need}) or misaligned (256 bytes)"),
            (pdist, dict(ws=FAKE + 128), "or misaligned (256 bytes)"),
            (pdist, dict(dist=FAKE + 4), "msa_pdist: counts / dist misaligned"),
            (pdist, dict(counts=FAKE + 2), "msa_pdist: counts / dist misaligned"),
            (neff, dict(msa=None), "msa_neff: null pointer"),
            (neff, dict(N=0), "msa_neff: N=0 outside [1, 1048576]"),
            (neff, dict(N=(1 << 20) + 1), "msa_neff: N=1048577 outside [1, 1048576]"),
            (neff, dict(L=0), "msa_neff: L=0 outside [1, 32768]"),
            (neff, dict(L=32769, ld=32769), "msa_neff: L=32769 outside [1, 32768]"),
            (neff, dict(ld=8), "msa_neff: ld=8 is smaller than L=9"),
            (neff, dict(cutoff=-0.5), "msa_neff: seqid_cutoff=-0.5 outside [0, 1]"),
            (neff, dict(cutoff=1.25), "msa_neff: seqid_cutoff=1.25 outside [0, 1]"),
            (neff, dict(cutoff=math.nan), "outside [0, 1]"),
            (neff, dict(nn=None, w=None, neff=None), "msa_neff: n_neighbors, weights and neff are all null: nothing to write"),
            (neff, dict(wsb=n_least - 1), f"msa_neff: workspace of {n_least - 1} bytes too small ({n_least} at least)"),
            (neff, dict(ws=FAKE + 64), "or misaligned (256 bytes)"),
            (neff, dict(w=FAKE + 4), "msa_neff: n_neighbors / weights / neff misaligned"),
            (coverage, dict(msa=None), "msa_coverage: null pointer"),
            (coverage, dict(out=None), "msa_coverage: null pointer"),
            (coverage, dict(N=0), "msa_coverage: N=0 outside [1, 1048576]"),
            (coverage, dict(N=(1 << 20) + 1), "msa_coverage: N=1048577 outside [1, 1048576]"),
            (coverage, dict(L=32769, ld=32769), "msa_coverage: L=32769 outside [1, 32768]"),
            (coverage, dict(ld=8), "msa_coverage: ld=8 is smaller than L=9"),
            (coverage, dict(gap=-1), "msa_coverage: gap=-1 is not a byte value"),
            (coverage, dict(gap=256), "msa_coverage: gap=256 is not a byte value"),
            (coverage, dict(out=FAKE + 4), "msa_coverage: coverage misaligned")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)


def test_a_device_that_is_no_hip_device_is_refused():
    import torch
    tokens = np.full((3, 5), 4, dtype=np.int64)
    for fn, args in ((msa.msa_pdist, (tokens, "cpu")), (msa.msa_pdist, (tokens, None)), (msa.msa_coverage, (tokens, 10, "cpu")),
                     (msa.msa_neff, (tokens, 0.2, "none", "cpu")), (msa.msa_neff, (tokens,))):
        with pytest.raises(_lib.RnamsmError, match="not a HIP device"):
            fn(*args)
    for fn, args in ((ops.msa_pdist, ()), (ops.msa_neff, (0.2,)), (ops.msa_coverage, (10,))):
        with pytest.raises(_lib.RnamsmError, match="no CPU path"):
            fn(torch.zeros(4, 5, dtype=torch.uint8), *args)
    with pytest.raises(ValueError, match="want="):
        ops.msa_pdist(torch.zeros(4, 5, dtype=torch.uint8), "matrix")


def test_the_key_in_the_configuration():
    assert Config().data.msa_stats is False
    assert parse_overrides(["data.msa_stats=true"]).data.msa_stats is True
    assert parse_overrides(["data.msa_stats=false"]).data.msa_stats is False
    assert parse_overrides(["data.msa_stats=true", "data.invcov=true"]).data.invcov is True
    with pytest.raises(ValueError):
        parse_overrides(["data.msa_stats=maybe"])
    with pytest.raises(ValueError, match="data.msa_stats="):
        check_msa_stats("true")
    assert check_msa_stats(True) is True and check_msa_stats(False) is False
    cfg = Config()
    cfg.data.msa_stats = "yes"                  # set past the parser: refused where the parser's check runs again
    with pytest.raises(ValueError, match="data.msa_stats='yes'"):
        parse_overrides([], cfg)
    with pytest.raises(ValueError, match="data.msa_stats='yes'"):
        inference.read_switches(cfg, False)
    sw = inference.read_switches(Config(), False)
    assert sw.msa_stats_on is False and sw.seqid_cutoff == 0.2
    assert inference.read_switches(parse_overrides(["data.msa_stats=true"]), False).msa_stats_on is True


def test_sink_writes_the_two_vectors_it_was_left(tmp_path):
    """The sequential sink (no device): what the reader left for an id becomes <id>_weights.npy and <id>_coverage.npy beside the usual
    two files; an id without statistics gets the usual two only."""
    import torch
    sw = inference.read_switches(parse_overrides(["data.msa_stats=true"]), False)
    sink = inference._Sink(["a", "b"], [], tmp_path, sw, 64, None, 0, async_io=False)
    w, c = torch.tensor([0.5, 0.25, 1.0], dtype=torch.float64), torch.tensor([1.0, 0.0], dtype=torch.float64)
    sink.put_stats("a", (w, c))
    for i in ("a", "b"):
        sink.emit(i, torch.zeros(2, 4), torch.zeros(1, 2, 2))
    sink.close()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a_atp.npy", "a_coverage.npy", "a_emb.npy", "a_weights.npy", "b_atp.npy", "b_emb.npy"]
    assert np.array_equal(np.load(tmp_path / "a_weights.npy"), w.numpy()) and np.array_equal(np.load(tmp_path / "a_coverage.npy"), c.numpy())
    assert sink.msa_stats == {}


@pytest.fixture(scope="module")
def words_program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host check of msa_words.h"
    exe = str(tmp_path_factory.mktemp("msa_pdist_words") / "msa_pdist_words_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "msa_pdist_words_check.cpp"), "-o", exe], check=True)
    return exe


def test_the_word_form_against_a_byte_loop_under_the_sanitizers(words_program):
    res = subprocess.run([words_program], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok "), (res.returncode, res.stdout[-500:], res.stderr[-2000:])
    assert int(res.stdout.split()[1]) >= 8 * 65536 * 2 + 40 * 200 * 2


def test_the_restatement_equals_the_references_own_values():
    g = golden("msa_stats_reference_2drb64.npz")
    a = golden("tokens_2DRB_1_first64.npz")["tokens"][:, 1:].astype(np.uint8)
    assert a.shape == (64, 35) and float(g["seqid_cutoff"]) == 0.2
    assert np.array_equal(T.dist(a), g["pdist"])
    assert np.array_equal(T.weights(a, 0.2), g["weights"])
    assert np.array_equal(T.coverage(a), g["coverage"])
    assert float(g["neff_none"]) == g["weights"].sum()
    assert float(g["neff_sqrt"]) == g["weights"].sum() / math.sqrt(35) and float(g["neff_seqlen"]) == g["weights"].sum() / 35
    assert 1.0 < float(g["neff_none"]) < 64.0 and (g["pdist"] == g["pdist"].T).all() and not g["pdist"].diagonal().any()


@pytest.mark.parametrize("L", [1, 3, 7, 33, 36, 64, 65, 127, 513, 1000])
def test_the_restatement_equals_scipy(L):
    sp = pytest.importorskip("scipy.spatial.distance")
    a = T.alignment(23, L, 60 + L)
    assert np.array_equal(T.dist(a), sp.squareform(sp.pdist(a, "hamming")))
