"""Covariance contacts (rnamsm_msa_invcov, rnamsm.msa.msa_invcov, data.invcov) without a GPU: the two symbols, the size function at
and outside the limits, every refusal the entry point makes before anything is enqueued (on fabricated aligned addresses that are
never dereferenced: the pattern of tests/test_ss_packed_host.py), the refusal of a device that is no HIP device, the key in the
configuration, and the numpy truth (tests/invcov_truth.py) against itself and against the reference's own MSA.invcov
(tests/golden/invcov_reference_n12_l9.npz, made by tests/golden/make_golden_invcov.py)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden
from rnamsm import _lib, msa, ops
from rnamsm.config import Config, check_invcov, parse_overrides
import invcov_truth as T

NEW = ("rnamsm_msa_invcov_workspace_bytes", "rnamsm_msa_invcov")
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
    assert callable(ops.msa_invcov) and callable(msa.msa_invcov)
    # the header says why token ids give the reference's map, and that the map is mirrored
    doc = re.search(r"/\* Covariance contacts.*?\*/", text, flags=re.S).group(0)
    assert "permutes" in doc and "mirrored" in doc and "exactly symmetric" in doc
    assert "invcov.hip" in open(os.path.join(ROOT, "rna-msm_amd", "csrc", "Makefile")).read()


def test_size_function_at_and_outside_the_limits(lib):
    size = lib.rnamsm_msa_invcov_workspace_bytes
    for N, L in ((1, 8), (0, 8), (-3, 8), ((1 << 20) + 1, 8), (8, 0), (8, -1), (8, _lib.LONG_MAX_L + 1)):
        assert size(N, L) == 0, (N, L)
    for N, L in ((2, 1), (1 << 20, 1), (2, _lib.LONG_MAX_L), (1024, 512), (100000, 1024)):
        assert size(N, L) > 0, (N, L)
    # the planes are laid out for 16 symbols: ceil(N / 64) words rounded up to 16, L * 16 rows rounded up to 64, 8 bytes each; the
    # band of counts holds the whole [L, L, 16, 16] int32 or 256 MB, whichever is less
    for N, L in ((2, 1), (129, 7), (1024, 512), (100000, 1024)):
        words = -(-(-(-N // 64)) // 16) * 16
        rows = -(-L * 16 // 64) * 64
        assert size(N, L) >= words * rows * 8 + min(L * L * 1024, 1 << 28), (N, L)
        assert size(N, L) <= words * rows * 8 + min(L * L * 1024, 1 << 28) + L * 64 + 4096, (N, L)
    assert size(100000, 1024) < 1 << 29


def test_every_refusal_made_before_anything_is_enqueued(lib):
    N, L = 12, 9
    need = lib.rnamsm_msa_invcov_workspace_bytes(N, L)
    ok = dict(tokens=FAKE, N=N, L=L, ld=L, gap=10, out=FAKE, counts=None, ws=FAKE, wsb=need)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.rnamsm_msa_invcov(a["tokens"], a["N"], a["L"], a["ld"], a["gap"], a["out"], a["counts"], a["ws"], a["wsb"], None)
        return rc, lib.rnamsm_last_error().decode()

    for kw, text in (
            (dict(tokens=None), "msa_invcov: null pointer"),
            (dict(out=None), "msa_invcov: null pointer"),
            (dict(ws=None), "msa_invcov: null pointer"),
            (dict(N=1), "msa_invcov: N=1 outside [2, 1048576]"),
            (dict(N=0), "msa_invcov: N=0 outside [2, 1048576]"),
            (dict(N=(1 << 20) + 1), "msa_invcov: N=1048577 outside [2, 1048576]"),
            (dict(L=0), "msa_invcov: L=0 outside [1, 4096]"),
            (dict(L=4097, ld=4097), "msa_invcov: L=4097 outside [1, 4096]"),
            (dict(ld=L - 1), "msa_invcov: ld=8 is smaller than L=9"),
            (dict(gap=-1), "msa_invcov: gap=-1 is not a byte value"),
            (dict(gap=256), "msa_invcov: gap=256 is not a byte value"),
            (dict(wsb=need - 1), "msa_invcov: workspace too small or misaligned (256 bytes)"),
            (dict(wsb=0), "msa_invcov: workspace too small or misaligned (256 bytes)"),
            (dict(ws=FAKE + 128), "msa_invcov: workspace too small or misaligned (256 bytes)"),
            (dict(out=FAKE + 4), "msa_invcov: out / counts misaligned"),
            (dict(counts=FAKE + 2), "msa_invcov: out / counts misaligned")):
        rc, msg = call(**kw)
        assert rc == ERR_INVALID and msg == text, (kw, rc, msg)


def test_no_cpu_path():
    tokens = np.full((4, 6), 4, dtype=np.int64)
    for device in (None, "cpu"):
        with pytest.raises(_lib.RnamsmError, match="no CPU path"):
            msa.msa_invcov(tokens, 10, device)
    import torch
    with pytest.raises(_lib.RnamsmError, match="no CPU path"):
        ops.msa_invcov(torch.zeros(4, 5, dtype=torch.uint8), 10)


def test_the_config_key_is_accepted_and_refused_like_its_neighbours():
    assert Config().data.invcov is False
    assert parse_overrides(["data.invcov=true"]).data.invcov is True
    assert parse_overrides(["data.invcov=false"]).data.invcov is False
    assert parse_overrides(["data.invcov=true", "data.contacts=true"]).data.contacts is True
    with pytest.raises(ValueError):
        parse_overrides(["data.invcov=maybe"])
    with pytest.raises(ValueError, match="data.invcov="):
        check_invcov("true")
    assert check_invcov(True) is True and check_invcov(False) is False
    cfg = Config()
    cfg.data.invcov = "yes"                     # set past the parser: refused where the parser's check runs again
    with pytest.raises(ValueError, match="data.invcov='yes'"):
        parse_overrides([], cfg)


# ---- the numpy truth against itself -------------------------------------------------------------------------------------
def test_truth_equals_the_references_own_invcov():
    """MSA.invcov ran over character bytes (A C G U ascending), the truth over token ids (A4 G5 C6 U7): a permutation of every block's
    rows and columns, which the spectral norm does not see but the order of numpy's additions does -- a few ulps of the largest
    entry (8 eps here; 1.1e-16 measured)."""
    g = golden("invcov_reference_n12_l9.npz")
    want = g["invcov"]
    assert want.shape == (9, 9) and want.dtype == np.float64 and g["tokens"].shape == (12, 9)
    got = T.invcov(g["tokens"])
    dist = float(np.abs(got - want).max())
    print(f"truth vs the reference's MSA.invcov: max abs {dist:.3e} (largest entry {want.max():.4f})")
    assert dist <= 8 * np.finfo(np.float64).eps * want.max()
    assert np.all(want[4] == 0) and np.all(got[4] == 0)           # the fixture's constant column


def test_truth_is_symmetric_and_blind_to_a_symbol_permutation():
    eps = np.finfo(np.float64).eps
    for name in ("N70_L13_K5", "N66_L19_K4_degenerate", "N129_L7_K4"):
        t = T.cases()[name]
        a = T.invcov(t)
        assert a.shape == (t.shape[1], t.shape[1]) and a.dtype == np.float64
        assert np.abs(a - a.T).max() <= 8 * eps * a.max(), name
        perm = np.arange(256, dtype=np.uint8)
        vals = T.symbols(t)
        perm[vals] = vals[::-1] + 100                # reverses the order of the symbols; the gap keeps its value
        b = T.invcov(perm[t])
        assert np.abs(a - b).max() <= 16 * eps * a.max(), name
        assert np.abs(a - T.invcov_eigh(t)).max() <= 64 * eps * a.max(), name


def test_truth_gives_zero_rows_for_a_column_with_one_symbol():
    t = T.cases()["N66_L19_K4_constant"]
    a = T.invcov(t)
    assert np.all(a[11] == 0) and np.all(a[:, 11] == 0) and a.max() > 0.1
    d = T.invcov(T.cases()["N66_L19_K4_degenerate"])
    assert np.all(d[3] == 0) and np.all(d[:, 3] == 0)             # an all-gap column: all zeros in the one-hot


def test_pair_counts_of_the_truth():
    t = T.cases()["N66_L19_K4_degenerate"]
    c = T.pair_counts(t)
    vals = T.symbols(t)
    assert c.shape == (19, 19, 4, 4) and c.dtype == np.int32
    for (i, j, a, b) in ((0, 0, 1, 1), (2, 7, 0, 3), (18, 1, 2, 2), (3, 5, 0, 0)):
        assert c[i, j, a, b] == int(((t[:, i] == vals[a]) & (t[:, j] == vals[b])).sum())
    assert np.array_equal(c, c.transpose(1, 0, 3, 2))
