"""Sequence-weighted mutual information on the GPU (csrc/msa_wmi.hip: rnamsm_msa_wmi on the fp64 matrix pipe; ops.msa_wmi,
rnamsm.msa.msa_mi_weighted), in both gap modes.

Exact facts are compared as bits: with unit weights the counts are ops.msa_invcov's integers and the maps are ops.msa_mi's bits; with
weights from {1, 1/2, 1/4, 1/8} every partial sum is a multiple of 1/8 below 2^50, so any order of summation is exact and the counts
are the host's math.fsum tables.  The shapes cross the kernel's seams: N around the MFMA's 4 rows, the 64-row word and the 256 rows
staged per step; L * S at 1, 64, 65 (one tile and one more row) and 7 * 17 (K = 16 with the gap as a state).

With real weights (1 / neighbours, ops.msa_neff) every count is held to N * 2^-52 relative of the exactly rounded sum: the bound of
N - 1 additions of non-negative terms in any order under either rounding mode (each addition errs by at most 2^-53 of a partial sum
that never exceeds the total, times (1 + 2^-53)^N; the sum has a half-ulp of slack to N * 2^-52).  Derived, not measured.  mi and mip
are held to four times wmi_truth.yardstick, the distance between two fp64 evaluations on the CPU (tables by fsum against tables by
ascending float64 sums; for mip also apc_numpy against apc_fsum).  Measured on the CPU: mi 1.22e-15 (pairwise) / 1.26e-15 (state),
bars 4.9e-15 / 5.0e-15; mip 1.67e-15 / 1.79e-15, bars 6.7e-15 / 7.1e-15.  Measured on an MI355X, the device's distance to the truth:
mi 1.22e-15 (pairwise) / 1.26e-15 (state) on the mixture and 4.2e-16 / 3.7e-16 on 2DRB_1; mip 1.75e-15 / 1.79e-15 and 5.5e-16 /
5.6e-16; the counts within 4.7e-15 relative on the mixture (bound 1.1e-12) and 5.5e-16 on 2DRB_1 (bound 1.4e-14), wmarg 3.9e-15 /
3.9e-16.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import invcov_truth as T
import wmi_truth as W
from rnamsm import _lib, msa, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (2, 3, 5, 63, 64, 65, 130, 255, 256, 257)          # the MFMA's 4 rows, the 64-row word, the 256 staged rows
SHAPES = {"1x1": (1, 1, "pairwise"), "13x5": (13, 5, "pairwise"), "16x4": (16, 4, "pairwise"), "7x17": (7, 16, "state")}   # L, K, mode
DYADIC = np.array([1.0, 0.5, 0.25, 0.125])


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _alignment(shape: str, N: int):
    """tokens of the shape with N rows; K is cut to the cells there are (N = 2 at 7x17: 14 symbols)."""
    L, K, mode = SHAPES[shape]
    rng = np.random.RandomState(1000 * N + L)
    return T.random_alignment(rng, N, L, min(K, N * L), gaps=0.2 if L > 1 else 0.0), mode


def _special_columns():
    """N = 65, L = 13, K = 4: a column of gaps only and a constant column; in state mode L * S = 65."""
    t = T.random_alignment(np.random.RandomState(77), 65, 13, 4, gaps=0.15)
    t[:, 2] = T.GAP
    t[:, 9] = 6
    assert len(T.symbols(t)) == 4
    return t


def _host(rec):
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in rec._asdict().items()}


# ---- exactness, no tolerance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_unit_weights_give_the_integer_counts_and_msa_mi_bits(shape):
    for N in NS:
        t, _ = _alignment(shape, N)
        d, ones = _dev(t), torch.ones(N, dtype=torch.float64, device=DEV)
        _, counts, symbols = ops.msa_invcov(d, T.GAP, want_counts=True)
        for mode in W.MODES:
            got = _host(ops.msa_wmi(d, T.GAP, mode, ones, want_counts=True))
            ref = ops.msa_mi(d, T.GAP, gaps=mode)
            K = len(T.symbols(t))
            assert np.array_equal(got["symbols"], symbols.cpu().numpy()) and got["wcounts"].shape[2] == K + (mode == "state"), (N, mode)
            assert np.array_equal(got["wcounts"][:, :, :K, :K], counts.cpu().numpy().astype(np.float64)), (N, mode)
            assert np.array_equal(got["wcounts"], W.tables_fsum(t, np.ones(N), mode)), (N, mode)
            assert got["mi"].tobytes() == ref.mi.cpu().numpy().tobytes(), (N, mode)
            assert got["mip"].tobytes() == ref.mip.cpu().numpy().tobytes(), (N, mode)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_dyadic_weights_give_the_hosts_exact_sums(shape):
    for N in NS:
        t, mode = _alignment(shape, N)
        w = DYADIC[np.random.RandomState(N).randint(0, 4, size=N)]
        got = _host(ops.msa_wmi(_dev(t), T.GAP, mode, _dev(w), want_counts=True))
        assert got["wcounts"].tobytes() == W.tables_fsum(t, w, mode).tobytes(), N
        assert got["wmarg"].tobytes() == W.profile_fsum(t, w, mode).tobytes(), N
        assert np.isfinite(got["mi"]).all() and got["mi"].tobytes() == np.ascontiguousarray(got["mi"].T).tobytes(), N


@pytest.mark.parametrize("mode", W.MODES)
def test_a_column_of_gaps_and_a_constant_column(mode):
    t = _special_columns()
    w = DYADIC[np.random.RandomState(3).randint(0, 4, size=t.shape[0])]
    d = _dev(t)
    got = _host(ops.msa_wmi(d, T.GAP, mode, _dev(w), want_counts=True))
    assert got["wcounts"].tobytes() == W.tables_fsum(t, w, mode).tobytes()
    assert got["wmarg"].tobytes() == W.profile_fsum(t, w, mode).tobytes()
    if mode == "pairwise":
        assert np.all(got["wcounts"][2] == 0) and np.all(got["wmarg"][2] == 0)
    else:
        assert got["wmarg"][2, 4] == w.sum() and np.all(got["wmarg"][2, :4] == 0)             # all of the weight on the gap state
    assert got["wmarg"][9, 2] == w.sum()                                                      # 6 is the third symbol of 4, 5, 6, 7
    for col in (2, 9):                                                                        # ratio 1.0, log 0: exactly 0
        assert np.all(got["mi"][col] == 0) and np.all(got["mi"][:, col] == 0), col
    assert got["mi"].max() > 0.01
    unit = _host(ops.msa_wmi(d, T.GAP, mode, torch.ones(t.shape[0], dtype=torch.float64, device=DEV)))
    ref = ops.msa_mi(d, T.GAP, gaps=mode)
    assert unit["mi"].tobytes() == ref.mi.cpu().numpy().tobytes() and unit["mip"].tobytes() == ref.mip.cpu().numpy().tobytes()


def test_every_row_twice_with_half_weights_gives_the_same_counts():
    for shape, N in (("13x5", 130), ("7x17", 65), ("16x4", 257)):
        t, mode = _alignment(shape, N)
        w = DYADIC[np.random.RandomState(N + 1).randint(0, 4, size=N)]
        once = _host(ops.msa_wmi(_dev(t), T.GAP, mode, _dev(w), want_counts=True))
        for t2, w2 in ((np.concatenate([t, t]), np.concatenate([w, w]) / 2), (np.repeat(t, 2, axis=0), np.repeat(w, 2) / 2)):
            twice = _host(ops.msa_wmi(_dev(t2), T.GAP, mode, _dev(w2), want_counts=True))
            assert twice["wcounts"].tobytes() == once["wcounts"].tobytes() and twice["wmarg"].tobytes() == once["wmarg"].tobytes(), shape
            assert twice["mi"].tobytes() == once["mi"].tobytes(), shape                       # the same tables, the same formula


# ---- real weights ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real():
    """(name, mode) -> the device's record on the alignment with ops.msa_neff's weights, computed once."""
    out = {}
    for name, t in W.alignments().items():
        d = _dev(t)
        w = ops.msa_neff(d, 0.2).weights
        assert np.array_equal(w.cpu().numpy(), W.real_weights(name)), name                    # the truth's weights, bit for bit
        for mode in W.MODES:
            out[name, mode] = _host(ops.msa_wmi(d, T.GAP, mode, w, want_counts=True))
    return out


@pytest.mark.parametrize("mode", W.MODES)
@pytest.mark.parametrize("name", sorted(W.alignments()))
def test_real_weights_counts_within_the_bound_of_any_order(real, name, mode):
    t = W.alignments()[name]
    bound = t.shape[0] * 2.0 ** -52
    got, want = real[name, mode]["wcounts"], W.truth_tables(name, mode)
    live = want > 0
    worst = float((np.abs(got - want)[live] / want[live]).max())
    prof = W.profile_fsum(t, W.real_weights(name), mode)
    worst_p = float((np.abs(real[name, mode]["wmarg"] - prof)[prof > 0] / prof[prof > 0]).max())
    print(f"{name} {mode}: wcounts within {worst:.3e} relative, wmarg within {worst_p:.3e} (bound {bound:.3e})")
    assert got.shape == want.shape and np.all(got[~live] == 0) and np.all(real[name, mode]["wmarg"][prof == 0] == 0)
    assert np.all(np.abs(got - want) <= bound * want) and np.all(np.abs(real[name, mode]["wmarg"] - prof) <= bound * prof)
    assert got.tobytes() == np.ascontiguousarray(got.transpose(1, 0, 3, 2)).tobytes()         # c(i,a; j,b) == c(j,b; i,a), bit for bit


@pytest.mark.parametrize("mode", W.MODES)
@pytest.mark.parametrize("name", sorted(W.alignments()))
def test_real_weights_mi_and_mip_against_the_fp64_truth(real, name, mode):
    y_mi, y_mip = W.yardstick(mode)
    assert 1e-17 < y_mi < 1e-14 and 1e-17 < y_mip < 1e-14
    mi, mip = W.truth(name, mode)
    got = real[name, mode]
    assert got["mi"].dtype == np.float64 and got["mi"].shape == mi.shape and np.isfinite(got["mi"]).all() and np.isfinite(got["mip"]).all()
    assert got["mi"].tobytes() == np.ascontiguousarray(got["mi"].T).tobytes()                 # exactly symmetric
    d_mi = float(np.abs(got["mi"] - mi).max() / mi.max())
    d_mip = float(np.abs(got["mip"] - mip).max() / np.abs(mip).max())
    print(f"{name} {mode}: mi {d_mi:.3e} of the largest entry (yardstick {y_mi:.3e}, bar {4 * y_mi:.3e}); "
          f"mip {d_mip:.3e} (yardstick {y_mip:.3e}, bar {4 * y_mip:.3e})")
    assert d_mi <= 4 * y_mi and d_mip <= 4 * y_mip
    # the python entry: the same weights from the same cutoff, the same bits; <cls> is dropped
    with_cls = np.concatenate([np.zeros((len(W.alignments()[name]), 1), dtype=np.int64), W.alignments()[name].astype(np.int64)], axis=1)
    a, b = msa.msa_mi_weighted(with_cls, T.GAP, DEV, gaps=mode)
    assert a.tobytes() == got["mi"].tobytes() and b.tobytes() == got["mip"].tobytes()
    c, _ = msa.msa_mi_weighted(with_cls, T.GAP, DEV, gaps=mode, weights=W.real_weights(name))
    assert c.tobytes() == got["mi"].tobytes()
    plain = ops.msa_mi(_dev(W.alignments()[name]), T.GAP, gaps=mode).mi.cpu().numpy()
    assert plain.tobytes() != got["mi"].tobytes()                                             # the weights change the map


# ---- banding, repeatability, strides ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", W.MODES)
def test_bands_runs_and_strides_give_the_same_bits(mode):
    N, L, K = 70, 100, 4
    t = T.random_alignment(np.random.RandomState(100), N, L, K, gaps=0.1)
    w = _dev(1.0 / np.random.RandomState(101).randint(1, 40, size=N))
    lib = _lib.load()
    least, default = lib.rnamsm_msa_wmi_min_workspace_bytes(N, L), lib.rnamsm_msa_wmi_workspace_bytes(N, L)
    S = K + (mode == "state")
    columns = (L * 17 * 17 * 8) // (L * S * S * 8)                    # columns i per band in the least workspace
    print(f"{mode}: least {least} bytes, {columns} columns per band, {-(-L // columns)} bands; default {default} bytes, one band")
    assert least < default and -(-L // columns) >= 3 and L % columns != 0
    d = _dev(t)
    one = _host(ops.msa_wmi(d, T.GAP, mode, w))
    wide = torch.full((N, L + 29), 4, dtype=torch.uint8, device=DEV)
    wide[:, 7:7 + L] = d
    for label, rec in (("least workspace", ops.msa_wmi(d, T.GAP, mode, w, workspace_bytes=least)),
                       ("between", ops.msa_wmi(d, T.GAP, mode, w, workspace_bytes=least + 5 * L * S * S * 8 + 256)),
                       ("second run", ops.msa_wmi(d, T.GAP, mode, w)),
                       ("strided", ops.msa_wmi(wide[:, 7:7 + L], T.GAP, mode, w))):
        other = _host(rec)
        for key in ("mi", "mip", "wmarg"):
            assert other[key].tobytes() == one[key].tobytes(), (label, key)
    counted = _host(ops.msa_wmi(d, T.GAP, mode, w, want_counts=True))      # the counts' own route: one launch, every tile
    assert counted["mi"].tobytes() == one["mi"].tobytes() and counted["wmarg"].tobytes() == one["wmarg"].tobytes()
    assert counted["wcounts"].tobytes() == np.ascontiguousarray(counted["wcounts"].transpose(1, 0, 3, 2)).tobytes()
    assert np.array_equal(counted["wmarg"], counted["wcounts"][np.arange(L), np.arange(L)].diagonal(0, 1, 2))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _raw(lib, t, w, outputs, ws, ws_bytes, mode=0):
    rc = lib.rnamsm_msa_wmi(t.data_ptr(), t.shape[0], t.shape[1], t.stride(0), T.GAP, mode, w.data_ptr(),
                            *(o.data_ptr() if o is not None else None for o in outputs), ws, ws_bytes, None)
    torch.cuda.synchronize()
    return rc, lib.rnamsm_last_error().decode()


def test_bad_weights_and_bad_workspaces_are_refused_and_nothing_is_written():
    lib = _lib.load()
    N, L = 130, 13
    t = _dev(T.random_alignment(np.random.RandomState(5), N, L, 4, gaps=0.1))
    need = lib.rnamsm_msa_wmi_min_workspace_bytes(N, L)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    base = ws.data_ptr() + (-ws.data_ptr()) % 256

    def outputs():
        return [torch.full((n,), -7.0, dtype=torch.float64, device=DEV) for n in (L * L, L * L, L * L * 25, L * 5)] + \
               [torch.full((32,), -7, dtype=torch.int32, device=DEV)]

    good = torch.full((N,), 0.25, dtype=torch.float64, device=DEV)
    for value, rows in ((float("nan"), (64, 129)), (float("inf"), (129,)), (float("-inf"), (3, 4)), (0.0, (0, 77)), (-0.5, (63,)),
                        (-0.0, (128,))):
        w = good.clone()
        w[list(rows)] = value
        outs = outputs()
        rc, msg = _raw(lib, t, w, outs, base, need, mode=1)
        assert rc == -1 and msg == f"msa_wmi: weights[{rows[0]}] is not finite and > 0 (the first such row)", (value, msg)
        assert all(bool((o == -7).all()) for o in outs), value                                # outputs untouched
    outs = outputs()
    for kw, text in ((dict(ws_bytes=need - 1), "is smaller than the"), (dict(ws=base + 128), "workspace misaligned (256 bytes)")):
        rc, msg = _raw(lib, t, good, outs, kw.get("ws", base), kw.get("ws_bytes", need))
        assert rc == -1 and text in msg, msg
    rc, msg = _raw(lib, t, good, [None, None, None, outs[3], outs[4]], base, need)
    assert rc == -1 and msg == "msa_wmi: mi, mip and wcounts are all NULL: nothing to compute"
    assert all(bool((o == -7).all()) for o in outs)
    with pytest.raises(_lib.RnamsmError, match=r"weights\[5\] is not finite and > 0"):
        w = good.clone()
        w[5] = float("inf")
        ops.msa_wmi(t, T.GAP, "pairwise", w)
    with pytest.raises(_lib.RnamsmError, match="is smaller than the"):
        ops.msa_wmi(t, T.GAP, "pairwise", good, workspace_bytes=need - 256)
    # the counts alone, the two maps NULL: accepted
    outs = outputs()
    rc, msg = _raw(lib, t, good, [None, None, outs[2], None, None], base, need, mode=1)
    assert rc == 0, msg
    want = W.tables_fsum(t.cpu().numpy(), np.full(N, 0.25), "state")
    assert outs[2].cpu().numpy().tobytes() == want.reshape(-1).tobytes() and bool((outs[0] == -7).all())
    # a weight of 1 / 0 neighbours: rnamsm_msa_neff at a cutoff of 0 gives inf, which is refused with its row
    with pytest.raises(_lib.RnamsmError, match=r"weights\[0\] is not finite and > 0"):
        ops.msa_wmi(t, T.GAP, "pairwise", ops.msa_neff(t, 0.0).weights)
