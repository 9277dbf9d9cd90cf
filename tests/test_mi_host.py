"""Mutual-information contacts (rnamsm_msa_mi, rnamsm_apc_f64, rnamsm.msa.msa_mi, data.mi / data.mi_gaps) without a GPU: the symbols, the
size functions, every refusal made before anything is enqueued (on fabricated aligned addresses that are never dereferenced), the
refusal of a device that is no HIP device, the two configuration keys, and the numpy truths (tests/mi_truth.py) against each other and
against the reference's own apc (tests/golden/apc_reference_l9.npz, made by tests/golden/make_golden_apc.py).

Measured on the CPU over invcov_truth.cases() and the mixture: yardstick_mi 8.2e-16 in both modes, yardstick_apc 7.6e-16 (pairwise)
and 7.0e-16 (state); no MI entry below 0."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden
from rnamsm import _lib, msa, ops
from rnamsm.config import Config, check_mi, check_mi_gaps, parse_overrides
import invcov_truth as T
import mi_truth as M

NEW = ("rnamsm_msa_mi_workspace_bytes", "rnamsm_msa_mi", "rnamsm_apc_f64_workspace_bytes", "rnamsm_apc_f64")
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
    assert callable(ops.msa_mi) and callable(ops.apc) and callable(msa.msa_mi) and callable(msa.msa_mi_device)
    doc = re.search(r"/\* Mutual-information contacts.*?\*/", text, flags=re.S).group(0)
    assert "must not be captured into a graph" in doc and "exactly symmetric" in doc and "c[gap][gap] = N - the rest" in doc
    assert "#define RNAMSM_MI_GAPS_PAIRWISE 0" in text and "#define RNAMSM_MI_GAPS_STATE 1" in text
    assert _lib.MI_GAP_MODES == {"pairwise": 0, "state": 1}


def test_size_functions_at_and_outside_the_limits(lib):
    size = lib.rnamsm_msa_mi_workspace_bytes
    for N, L in ((1, 8), (0, 8), ((1 << 20) + 1, 8), (8, 0), (8, -1), (8, _lib.LONG_MAX_L + 1)):
        assert size(N, L) == 0, (N, L)
    for N, L in ((2, 1), (1 << 20, 1), (2, _lib.LONG_MAX_L), (1024, 512), (100000, 1024)):
        # stage 1's bytes, one [L, L] float64 map, the correction's 2 L + 1 sums, each rounded up to 256
        stage1 = lib.rnamsm_msa_invcov_workspace_bytes(N, L)
        assert stage1 + L * L * 8 + (2 * L + 1) * 8 <= size(N, L) <= stage1 + L * L * 8 + (2 * L + 1) * 8 + 3 * 256, (N, L)
    apc = lib.rnamsm_apc_f64_workspace_bytes
    assert apc(0) == 0 and apc(-1) == 0 and apc(_lib.APC_MAX_L + 1) == 0
    for L in (1, 9, 2100, _lib.APC_MAX_L):
        assert (2 * L + 1) * 8 <= apc(L) < (2 * L + 1) * 8 + 256


def test_every_refusal_of_msa_mi_made_before_anything_is_enqueued(lib):
    N, L = 12, 9
    need = lib.rnamsm_msa_mi_workspace_bytes(N, L)
    ok = dict(tokens=FAKE, N=N, L=L, ld=L, gap=10, mode=0, mi=FAKE, mip=FAKE + 4096, ws=FAKE, wsb=need)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.rnamsm_msa_mi(a["tokens"], a["N"], a["L"], a["ld"], a["gap"], a["mode"], a["mi"], a["mip"], a["ws"], a["wsb"], None)
        return rc, lib.rnamsm_last_error().decode()

    for kw, text in (
            (dict(tokens=None), "msa_mi: null pointer"),
            (dict(ws=None), "msa_mi: null pointer"),
            (dict(N=1), "msa_mi: N=1 outside [2, 1048576]"),
            (dict(N=(1 << 20) + 1), "msa_mi: N=1048577 outside [2, 1048576]"),
            (dict(L=0), "msa_mi: L=0 outside [1, 4096]"),
            (dict(L=4097, ld=4097), "msa_mi: L=4097 outside [1, 4096]"),
            (dict(ld=L - 1), "msa_mi: ld=8 is smaller than L=9"),
            (dict(gap=256), "msa_mi: gap=256 is not a byte value"),
            (dict(mode=2), "msa_mi: gap_mode=2 is not 0 (pairwise) or 1 (state)"),
            (dict(mode=-1), "msa_mi: gap_mode=-1 is not 0 (pairwise) or 1 (state)"),
            (dict(mi=None, mip=None), "msa_mi: mi and mip are both NULL: nothing to compute"),
            (dict(wsb=need - 1), f"msa_mi: workspace of {need - 1} bytes is smaller than the {need} that N=12, L=9 need"),
            (dict(ws=FAKE + 128), "msa_mi: workspace misaligned (256 bytes)"),
            (dict(mi=FAKE + 4), "msa_mi: mi / mip misaligned, or one buffer for both"),
            (dict(mip=FAKE), "msa_mi: mi / mip misaligned, or one buffer for both")):
        rc, msg = call(**kw)
        assert rc == ERR_INVALID and msg == text, (kw, rc, msg)


def test_every_refusal_of_apc_f64(lib):
    L = 9
    need = lib.rnamsm_apc_f64_workspace_bytes(L)
    ok = dict(x=FAKE, L=L, ld=L, zd=0, out=FAKE + 4096, ws=FAKE + 8192, wsb=need)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.rnamsm_apc_f64(a["x"], a["L"], a["ld"], a["zd"], a["out"], a["ws"], a["wsb"], None)
        return rc, lib.rnamsm_last_error().decode()

    for kw, text in (
            (dict(x=None), "apc_f64: null pointer"),
            (dict(out=None), "apc_f64: null pointer"),
            (dict(ws=None), "apc_f64: null pointer"),
            (dict(L=0), "apc_f64: L=0 outside [1, 32768]"),
            (dict(L=32769, ld=32769), "apc_f64: L=32769 outside [1, 32768]"),
            (dict(ld=8), "apc_f64: ld=8 is smaller than L=9"),
            (dict(zd=2), "apc_f64: zero_diagonal=2 is not 0 or 1"),
            (dict(wsb=need - 1), f"apc_f64: workspace of {need - 1} bytes is smaller than the {need} that L=9 needs"),
            (dict(x=FAKE + 4), "apc_f64: x / out / workspace misaligned (8 bytes)"),
            (dict(out=FAKE, ld=12), "apc_f64: out == x needs ld == L (ld=12, L=9)")):
        rc, msg = call(**kw)
        assert rc == ERR_INVALID and msg == text, (kw, rc, msg)


def test_no_cpu_path():
    import torch
    tokens = np.full((4, 6), 4, dtype=np.int64)
    for device in (None, "cpu"):
        with pytest.raises(_lib.RnamsmError, match="no CPU path"):
            msa.msa_mi(tokens, 10, device)
    with pytest.raises(_lib.RnamsmError, match="no CPU path"):
        ops.msa_mi(torch.zeros(4, 5, dtype=torch.uint8), 10)
    with pytest.raises(_lib.RnamsmError, match="no CPU path"):
        ops.apc(torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="gaps='foo'"):
        ops.msa_mi(torch.zeros(4, 5, dtype=torch.uint8), 10, gaps="foo")
    with pytest.raises(ValueError, match="want="):
        ops.msa_mi(torch.zeros(4, 5, dtype=torch.uint8), 10, want=())


def test_the_config_keys_are_accepted_and_refused_like_their_neighbours():
    assert Config().data.mi is False and Config().data.mi_gaps == "pairwise"             # the defaults are off
    cfg = parse_overrides(["data.mi=true", "data.mi_gaps=state"])
    assert cfg.data.mi is True and cfg.data.mi_gaps == "state"
    assert parse_overrides(["data.mi=false"]).data.mi is False
    assert parse_overrides(["data.mi=true", "data.invcov=true"]).data.invcov is True
    with pytest.raises(ValueError, match="data.mi_gaps='foo'"):
        parse_overrides(["data.mi_gaps=foo"])                                             # refused at start-up
    with pytest.raises(ValueError):
        parse_overrides(["data.mi=maybe"])
    with pytest.raises(ValueError, match="data.mi="):
        check_mi("true")
    assert check_mi(True) is True and check_mi_gaps("pairwise") == "pairwise"
    cfg = Config()
    cfg.data.mi_gaps = "both"                   # set past the parser: refused where the parser's check runs again
    with pytest.raises(ValueError, match="data.mi_gaps='both'"):
        parse_overrides([], cfg)


# ---- the numpy truths against each other ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", M.MODES)
def test_the_two_mi_restatements_agree(mode):
    y = M.yardstick_mi(mode)
    print(f"yardstick_mi({mode}) = {y:.3e} over {len(M.alignments())} alignments")
    assert 1e-17 < y < 64 * EPS                       # two fp64 evaluations: a few ulps of the largest entry, and not the same code


@pytest.mark.parametrize("mode", M.MODES)
def test_the_two_apc_restatements_agree(mode):
    y = M.yardstick_apc(mode)
    print(f"yardstick_apc({mode}) = {y:.3e}")
    assert 1e-17 < y < 64 * EPS


@pytest.mark.parametrize("mode", M.MODES)
def test_mi_is_not_negative_and_its_diagonal_is_the_entropy(mode):
    lowest = 0.0
    for name, t in M.alignments().items():
        mi = M.truth(name, mode)
        top = mi.max()
        lowest = min(lowest, float(mi.min()))
        assert mi.min() >= -8 * EPS * max(top, 1.0), name                                 # >= 0 up to rounding
        assert np.array_equal(mi, mi.T) or np.abs(mi - mi.T).max() <= 8 * EPS * top, name
        c = M.tables(t, mode)
        L = t.shape[1]
        diag = c[np.arange(L), np.arange(L)].sum(-1)                                      # the column's state counts
        n = diag.sum(-1)
        p = np.divide(diag, n[:, None], out=np.zeros(diag.shape), where=n[:, None] > 0)
        entropy = -(p * np.log(np.where(p > 0, p, 1.0))).sum(-1)
        assert np.abs(np.diag(mi) - entropy).max() <= 8 * EPS * max(top, 1.0), name
    print(f"{mode}: the lowest MI entry {lowest:.3e}")


def test_state_tables_count_every_row_and_pairwise_tables_drop_gapped_rows():
    t = T.cases()["N66_L19_K4_degenerate"]
    vals = list(T.symbols(t)) + [T.GAP]
    state, pairwise = M.tables(t, "state"), M.tables(t, "pairwise")
    assert state.shape == (19, 19, 5, 5) and pairwise.shape == (19, 19, 4, 4)
    assert np.all(state.sum((2, 3)) == 66)
    for (i, j, a, b) in ((0, 1, 4, 4), (3, 7, 4, 2), (7, 3, 2, 4), (2, 2, 4, 4), (5, 9, 1, 4), (18, 0, 0, 0)):
        assert state[i, j, a, b] == int(((t[:, i] == vals[a]) & (t[:, j] == vals[b])).sum()), (i, j, a, b)
    assert np.array_equal(state[:, :, :4, :4], pairwise)
    assert np.all(pairwise[3] == 0) and np.all(state[3, :, :4] == 0)                      # the all-gap column
    # exact zeros: the all-gap column in both modes, the constant column in both modes
    for mode in M.MODES:
        mi = M.mi_ratio(t, mode)
        assert np.all(mi[3] == 0) and np.all(mi[:, 3] == 0), mode
        const = M.mi_ratio(T.cases()["N66_L19_K4_constant"], mode)
        assert np.all(const[11] == 0) and np.all(const[:, 11] == 0) and const.max() > 0.1, mode


def test_apc_numpy_equals_the_references_own_apc():
    """Not bit for bit: the reference's apc is wrapped by coerce_numpy and runs on torch tensors, whose sums over 9 and 81 elements
    are taken in another order than numpy's (measured: the total and some column sums differ in their last bit; 67 of 81 outputs
    differ, by at most 3.7 eps of the largest output).  The bar: a1, a2, a12 are sums of positive numbers, each within 2 eps of the
    exact sum in either order; the product, the division and the subtraction add three roundings: below 8 eps of the largest |x|,
    which bounds a1 * a2 / a12 on a positive map."""
    g = golden("apc_reference_l9.npz")
    for name in ("general", "symmetric"):
        x, want = g["x_" + name], g["apc_" + name]
        assert x.shape == (9, 9) and x.dtype == np.float64 and want.dtype == np.float64 and x.min() >= 0
        for restatement in (M.apc_numpy, M.apc_fsum):
            dist = float(np.abs(restatement(x) - want).max())
            print(f"{name}: {restatement.__name__} vs the reference's apc: max abs {dist / EPS:.2f} eps (largest |x| {x.max():.4f})")
            assert dist <= 8 * EPS * x.max(), name
    assert not np.array_equal(g["x_general"], g["x_general"].T) and np.array_equal(g["x_symmetric"], g["x_symmetric"].T)
    assert np.all(np.diag(g["x_symmetric"]) == 0)
    with np.errstate(all="ignore"):
        assert np.isnan(M.apc_numpy(np.zeros((3, 3)))).all() and np.isnan(M.apc_fsum(np.zeros((1, 1)))).all()
