"""Sequence-weighted mutual information (rnamsm_msa_wmi, ops.msa_wmi, rnamsm.msa.msa_mi_weighted, data.mi_weights) without a GPU: the
symbols, the size functions, every refusal made before anything is enqueued (on fabricated aligned addresses that are never
dereferenced), the refusal of a device that is no HIP device, the configuration key, and the fp64 truth (tests/wmi_truth.py) against
tests/mi_truth.py and against itself.

Measured on the CPU over the mixture and the 64-row excerpt of 2DRB_1 with their 1 / neighbours weights: yardstick mi 1.22e-15
(pairwise) and 1.26e-15 (state), mip 1.67e-15 and 1.79e-15."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from rnamsm import _lib, msa, ops
from rnamsm.config import Config, check_mi_weights, parse_overrides
import invcov_truth as T
import mi_truth as M
import wmi_truth as W

NEW = ("rnamsm_msa_wmi_workspace_bytes", "rnamsm_msa_wmi_min_workspace_bytes", "rnamsm_msa_wmi")
FAKE = 0x100000                 # 256-byte aligned, never dereferenced
ERR_INVALID = -1
EPS = np.finfo(np.float64).eps


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
    assert callable(ops.msa_wmi) and callable(msa.msa_mi_weighted) and callable(msa.msa_mi_weighted_device)
    assert ops.MsaWmi._fields == ("mi", "mip", "wcounts", "wmarg", "symbols")
    doc = re.search(r"/\* Sequence-weighted mutual information.*?\*/", text, flags=re.S).group(0)
    assert "must not be captured into a graph" in doc and "bit for bit" in doc and "the first such row" in doc


def test_size_functions_at_and_outside_the_limits(lib):
    size, least = lib.rnamsm_msa_wmi_workspace_bytes, lib.rnamsm_msa_wmi_min_workspace_bytes
    for N, L in ((1, 8), (0, 8), ((1 << 20) + 1, 8), (8, 0), (8, -1), (8, _lib.LONG_MAX_L + 1)):
        assert size(N, L) == 0 and least(N, L) == 0, (N, L)
    for N, L in ((2, 1), (1 << 20, 1), (2, _lib.LONG_MAX_L), (1024, 512), (100000, 1024), (70, 100)):
        per_col = L * 17 * 17 * 8                                     # one column i of counts at S = 17
        band = min(L * per_col, 1 << 28)
        assert size(N, L) - least(N, L) == band - per_col, (N, L)     # the default holds every column, or 256 MB of them
        assert least(N, L) % 256 == 0 or per_col % 256, (N, L)
        assert least(N, L) > per_col + L * L * 8 + N // 8 * L * 17, (N, L)      # a column, the map, the state planes
    # three bands and more at L = 100 with the least workspace: one column at S = 17 is 18 columns at S = 4 and 11 at S = 5
    assert 100 * 17 * 17 * 8 // (100 * 4 * 4 * 8) == 18 and 100 * 17 * 17 * 8 // (100 * 5 * 5 * 8) == 11


def test_every_refusal_of_msa_wmi_made_before_anything_is_enqueued(lib):
    N, L = 12, 9
    need = lib.rnamsm_msa_wmi_min_workspace_bytes(N, L)
    ok = dict(tokens=FAKE, N=N, L=L, ld=L, gap=10, mode=0, w=FAKE + 1024, mi=FAKE + 2048, mip=FAKE + 4096, wc=None, wm=None, meta=None,
              ws=FAKE, wsb=need)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.rnamsm_msa_wmi(a["tokens"], a["N"], a["L"], a["ld"], a["gap"], a["mode"], a["w"], a["mi"], a["mip"], a["wc"], a["wm"],
                                a["meta"], a["ws"], a["wsb"], None)
        return rc, lib.rnamsm_last_error().decode()

    misaligned = "msa_wmi: weights / mi / mip / wcounts / wmarg / meta misaligned, or one buffer for mi and mip"
    for kw, text in (
            (dict(tokens=None), "msa_wmi: null pointer"),
            (dict(ws=None), "msa_wmi: null pointer"),
            (dict(w=None), "msa_wmi: null pointer"),
            (dict(N=1), "msa_wmi: N=1 outside [2, 1048576]"),
            (dict(N=(1 << 20) + 1), "msa_wmi: N=1048577 outside [2, 1048576]"),
            (dict(L=0), "msa_wmi: L=0 outside [1, 4096]"),
            (dict(L=4097, ld=4097), "msa_wmi: L=4097 outside [1, 4096]"),
            (dict(ld=L - 1), "msa_wmi: ld=8 is smaller than L=9"),
            (dict(gap=256), "msa_wmi: gap=256 is not a byte value"),
            (dict(mode=2), "msa_wmi: gap_mode=2 is not 0 (pairwise) or 1 (state)"),
            (dict(mode=-1), "msa_wmi: gap_mode=-1 is not 0 (pairwise) or 1 (state)"),
            (dict(mi=None, mip=None), "msa_wmi: mi, mip and wcounts are all NULL: nothing to compute"),
            (dict(wsb=need - 1), f"msa_wmi: workspace of {need - 1} bytes is smaller than the {need} that N=12, L=9 need at least"),
            (dict(wsb=0), f"msa_wmi: workspace of 0 bytes is smaller than the {need} that N=12, L=9 need at least"),
            (dict(ws=FAKE + 128), "msa_wmi: workspace misaligned (256 bytes)"),
            (dict(w=FAKE + 4), misaligned),
            (dict(mi=FAKE + 4), misaligned),
            (dict(wc=FAKE + 2), misaligned),
            (dict(wm=FAKE + 1), misaligned),
            (dict(meta=FAKE + 2), misaligned),
            (dict(mip=FAKE + 2048), misaligned)):
        rc, msg = call(**kw)
        assert rc == ERR_INVALID and msg == text, (kw, rc, msg)


def test_no_cpu_path_and_the_python_refusals():
    import torch
    tokens = np.full((4, 6), 4, dtype=np.int64)
    for device in (None, "cpu"):
        with pytest.raises(_lib.RnamsmError, match="no CPU path"):
            msa.msa_mi_weighted(tokens, 10, device)
        with pytest.raises(_lib.RnamsmError, match="no CPU path"):
            msa.msa_mi_weighted(tokens, 10, device, weights=np.ones(4))
    u8 = torch.zeros(4, 5, dtype=torch.uint8)
    with pytest.raises(_lib.RnamsmError, match="no CPU path"):
        ops.msa_wmi(u8, 10, weights=torch.ones(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="gaps='foo'"):
        ops.msa_wmi(u8, 10, gaps="foo", weights=torch.ones(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="weights is required"):
        ops.msa_wmi(u8, 10)


def test_the_config_key_is_accepted_and_refused():
    assert Config().data.mi_weights == "none"                                             # the default is off
    cfg = parse_overrides(["data.mi=true", "data.mi_weights=seqid"])
    assert cfg.data.mi is True and cfg.data.mi_weights == "seqid"
    assert parse_overrides(["data.mi_weights=none"]).data.mi_weights == "none"            # "none" asks for nothing: fine without data.mi
    assert parse_overrides(["data.mi=true", "data.mi_weights=none"]).data.mi_weights == "none"
    with pytest.raises(ValueError, match="data.mi_weights='seqid' needs data.mi=true"):
        parse_overrides(["data.mi_weights=seqid"])                                        # refused at start-up, the key named
    with pytest.raises(ValueError, match="data.mi_weights='seqid' needs data.mi=true"):
        parse_overrides(["data.mi_weights=seqid", "data.mi=false", "data.msa_stats=true"])
    with pytest.raises(ValueError, match="data.mi_weights='neff' is not one of 'none', 'seqid'"):
        parse_overrides(["data.mi=true", "data.mi_weights=neff"])
    assert check_mi_weights("seqid", True) == "seqid" and check_mi_weights("none", False) == "none"
    cfg = Config()
    cfg.data.mi_weights = "seqid"               # set past the parser: refused where the parser's check runs again
    with pytest.raises(ValueError, match="data.mi_weights='seqid' needs data.mi=true"):
        parse_overrides([], cfg)
    from rnamsm.inference import read_switches
    cfg = parse_overrides(["data.mi=true", "data.mi_weights=seqid"])
    assert read_switches(cfg, False).mi_weighted is True and read_switches(Config(), False).mi_weighted is False


# ---- the truth against mi_truth and against itself ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", W.MODES)
def test_unit_weights_give_the_integer_tables_and_their_mi(mode):
    for name in ("N66_L19_K4_degenerate", "N66_L19_K4_constant", "N70_L5_K16", "N3_L7_K4", "N129_L7_K4"):
        t = T.cases()[name]
        ones = np.ones(t.shape[0])
        c = W.tables_fsum(t, ones, mode)
        assert c.dtype == np.float64 and np.array_equal(c, M.tables(t, mode)), name       # exactly the integers
        assert np.array_equal(W.tables_ascending(t, ones, mode), c), name
        assert np.array_equal(W.profile_fsum(t, ones, mode), c[np.arange(t.shape[1]), np.arange(t.shape[1])].diagonal(0, 1, 2)), name
        # the loops of mi_of_tables on integers are mi_ratio_of's sums: every s, r, n is exact, the terms are the same operations
        assert W.mi_of_tables(c).tobytes() == M.mi_ratio(t, mode).tobytes(), name


@pytest.mark.parametrize("mode", W.MODES)
def test_every_row_twice_with_half_weights_leaves_the_tables_bit_identical(mode):
    for name, t in W.alignments().items():
        w = W.real_weights(name)
        if name.startswith("mixture"):
            t, w = t[:600], w[:600]
        c = W.tables_fsum(t, w, mode)
        twice = W.tables_fsum(np.concatenate([t, t]), np.concatenate([w / 2, w / 2]), mode)    # w / 2 is exact, and so is x + x
        assert twice.tobytes() == c.tobytes(), name
        interleaved = W.tables_fsum(np.repeat(t, 2, axis=0), np.repeat(w / 2, 2), mode)
        assert interleaved.tobytes() == c.tobytes(), name


@pytest.mark.parametrize("mode", W.MODES)
def test_the_two_evaluations_agree_within_a_few_ulps(mode):
    y_mi, y_mip = W.yardstick(mode)
    print(f"yardstick({mode}): mi {y_mi:.3e}, mip {y_mip:.3e}")
    assert 1e-17 < y_mi < 64 * EPS and 1e-17 < y_mip < 64 * EPS       # two fp64 evaluations: a few ulps, and not the same sums
    for name, t in W.alignments().items():
        # every ascending sum of N non-negative terms lies within N * 2^-52 relative of the exactly rounded sum
        a, b = W.truth_tables(name, mode), W.tables_ascending(t, W.real_weights(name), mode)
        assert np.all(np.abs(a - b) <= t.shape[0] * 2.0 ** -52 * a), name
        mi, _ = W.truth(name, mode)
        assert mi.min() >= -8 * EPS * mi.max() and np.abs(mi - mi.T).max() <= 8 * EPS * mi.max(), name


def test_the_weights_are_the_references_on_the_shipped_excerpt():
    from conftest import golden
    assert np.array_equal(W.real_weights("2DRB_1_first64"), golden("msa_stats_reference_2drb64.npz")["weights"])
    w = W.real_weights("mixture_N5000_L33")
    assert w.shape == (5000,) and w.min() > 0 and w.max() <= 1.0 and len(np.unique(w)) > 10       # real, unlike weights
