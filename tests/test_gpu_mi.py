"""Mutual-information contacts on the GPU (csrc/invcov.hip: rnamsm_msa_mi; csrc/apc.hip: rnamsm_apc_f64; ops.msa_mi, ops.apc,
rnamsm.msa.msa_mi), in both gap modes.

mi is held to the fp64 truth tests/mi_truth.mi_ratio (the definition over numpy's integer tables).  The bar is derived, not chosen:
yardstick_mi = the largest elementwise distance between two fp64 restatements on the CPU (the ratio form and H_i + H_j - H_ij) over
invcov_truth.cases() and the mixture, relative to each map's largest entry; the device, a third evaluation of the same conditioning,
gets 4 x that.  mip is held to apc_numpy of the DEVICE's mi with a zero diagonal (only the correction is under test) within
4 x yardstick_apc (apc_numpy against the math.fsum form) of the largest |entry|.  ops.apc alone has no gap mode: its bar is 4 x the
larger of the two modes' yardstick_apc.  Measured on the CPU: yardstick_mi 8.2e-16 in both modes (bar 3.3e-15), yardstick_apc 7.6e-16
(pairwise) and 7.0e-16 (state) (bars 3.0e-15, 2.8e-15).  The exact facts are compared as bits.  Every test prints its figures before
it asserts."""
import numpy as np
import pytest
import torch

import invcov_truth as T
import mi_truth as M
from conftest import golden
from rnamsm import _lib, msa, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = sorted(M.alignments())


def _dev(t):
    return torch.from_numpy(np.array(t)).to(DEV)


@pytest.fixture(scope="module")
def yards():
    out = {mode: (M.yardstick_mi(mode), M.yardstick_apc(mode)) for mode in M.MODES}
    for mode, (ymi, yapc) in out.items():
        print(f"{mode}: yardstick_mi {ymi:.3e} (bar {4 * ymi:.3e}), yardstick_apc {yapc:.3e} (bar {4 * yapc:.3e})")
        assert 1e-17 < ymi < 1e-14 and 1e-17 < yapc < 1e-14            # two fp64 evaluations: a few ulps, or the yardstick is broken
    return out


@pytest.fixture(scope="module")
def device_results():
    """(name, mode) -> (mi, mip) of every alignment, computed once."""
    out = {}
    for name, t in M.alignments().items():
        for mode in M.MODES:
            rec = ops.msa_mi(_dev(t), T.GAP, gaps=mode)
            out[name, mode] = (rec.mi.cpu().numpy(), rec.mip.cpu().numpy())
    return out


def _check_mi(label, got, want, bar):
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.isfinite(got).all(), label
    assert got.tobytes() == np.ascontiguousarray(got.T).tobytes(), label            # exactly symmetric
    top = float(want.max())
    if top == 0:
        assert np.all(got == 0), label
        return 0.0
    dist = float(np.abs(got - want).max() / top)
    print(f"{label}: {dist:.3e} of the largest entry {top:.4f} (bar {bar:.3e})")
    assert dist <= bar, label
    return dist


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("name", NAMES)
def test_mi_against_the_fp64_truth(device_results, yards, name, mode):
    _check_mi(f"{name} {mode}", device_results[name, mode][0], M.truth(name, mode), 4 * yards[mode][0])


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("name", NAMES)
def test_mip_against_apc_of_the_devices_mi(device_results, yards, name, mode):
    mi, mip = device_results[name, mode]
    want = M.apc_numpy(M.zero_diagonal(mi))
    assert mip.shape == mi.shape and mip.dtype == np.float64
    if M.zero_diagonal(mi).sum() == 0:                                    # L = 1, or every column constant: 0 / 0
        assert np.isnan(want).all() and np.isnan(mip).all(), name
        return
    assert np.isfinite(mip).all(), name
    top = float(np.abs(want).max())
    dist = float(np.abs(mip - want).max() / top)
    print(f"{name} {mode}: mip {dist:.3e} of the largest |entry| {top:.4f} (bar {4 * yards[mode][1]:.3e})")
    assert dist <= 4 * yards[mode][1], name


def test_two_bands_give_the_truth_of_one(yards):
    """L = 2100, N = 66, K = 4: the counts (L * L * 16 * 4 bytes > 256 MB) are made in two bands of columns i, 1984 + 116.  The truth's
    counts come from a float64 matrix product of the one-hot (exact: every count is an integer <= 66).  The whole truth is 180 million
    logarithms (15 s in numpy), so it is made for whole rows i of three slabs -- the first 64 columns, the last 64 of the first band
    with its edge, and all of the second band -- against every column j; the map's exact symmetry carries those rows to their
    columns."""
    rng = np.random.RandomState(17)
    N, L, K = 66, 2100, 4
    t = T.random_alignment(rng, N, L, K, gaps=0.1)
    assert L * L * K * K * 4 > 1 << 28
    flat = (t[:, :, None] == T.symbols(t)[None, None, :]).astype(np.float64).reshape(N, L * K)
    marg = flat.sum(0).reshape(L, K).astype(np.int64)
    rows = np.r_[0:64, 1920:2100]
    counts = (flat.reshape(N, L, K)[:, rows].reshape(N, -1).T @ flat).reshape(len(rows), K, L, K).transpose(0, 2, 1, 3)
    want = {mode: M.mi_ratio_of(M.tables_from_counts(counts, N, mode, marg[rows], marg)) for mode in M.MODES}
    dev_t = _dev(t)
    for mode in M.MODES:
        rec = ops.msa_mi(dev_t, T.GAP, gaps=mode)
        got = rec.mi.cpu().numpy()
        assert got.tobytes() == np.ascontiguousarray(got.T).tobytes() and np.isfinite(got).all() and got.min() > -1e-12
        top = float(want[mode].max())
        dist = float(np.abs(got[rows] - want[mode]).max() / top)
        print(f"two bands {mode}: {dist:.3e} of the largest entry {top:.4f} (bar {4 * yards[mode][0]:.3e})")
        assert dist <= 4 * yards[mode][0]
        ref = M.apc_numpy(M.zero_diagonal(got))
        dist = float(np.abs(rec.mip.cpu().numpy() - ref).max() / np.abs(ref).max())
        print(f"two bands {mode}: mip {dist:.3e} (bar {4 * yards[mode][1]:.3e})")
        assert dist <= 4 * yards[mode][1]


# ---- exact facts, compared as bits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", M.MODES)
def test_constant_and_all_gap_columns_are_exactly_zero(device_results, mode):
    const = device_results["N66_L19_K4_constant", mode][0]
    assert np.all(const[11] == 0) and np.all(const[:, 11] == 0) and const.max() > 0.1
    deg = device_results["N66_L19_K4_degenerate", mode][0]
    assert np.all(deg[3] == 0) and np.all(deg[:, 3] == 0) and deg.max() > 0.1          # the all-gap column


def test_the_diagonal_is_the_entropy_and_the_same_bits_in_both_modes_without_a_gap(device_results, yards):
    seen = 0
    for name, t in M.alignments().items():
        pairwise, state = np.diag(device_results[name, "pairwise"][0]), np.diag(device_results[name, "state"][0])
        no_gap = ~(t == T.GAP).any(0)
        seen += int(no_gap.sum())
        assert pairwise[no_gap].tobytes() == state[no_gap].tobytes(), name
        for mode, diag in (("pairwise", pairwise), ("state", state)):
            c = M.tables(t, mode)
            cols = c[np.arange(len(diag)), np.arange(len(diag))].sum(-1)
            n = cols.sum(-1)
            p = np.divide(cols, n[:, None], out=np.zeros(cols.shape), where=n[:, None] > 0)
            entropy = -(p * np.log(np.where(p > 0, p, 1.0))).sum(-1)
            assert np.abs(diag - entropy).max() <= 4 * yards[mode][0] * max(float(M.truth(name, mode).max()), 1e-300), (name, mode)
    assert seen > 100


@pytest.mark.parametrize("mode", M.MODES)
def test_two_runs_strided_rows_and_recodings(device_results, yards, mode):
    for name in ("N129_L7_K4", "N70_L13_K5", "N70_L65_K1", "mixture_N5000_L33"):
        t = M.alignments()[name]
        mi, mip = device_results[name, mode]
        again = ops.msa_mi(_dev(t), T.GAP, gaps=mode)                                     # two runs: the same bits
        assert again.mi.cpu().numpy().tobytes() == mi.tobytes() and again.mip.cpu().numpy().tobytes() == mip.tobytes(), name
        # one map at a time: the same bits (mip alone is made from a map in the workspace)
        assert ops.msa_mi(_dev(t), T.GAP, gaps=mode, want="mip").mip.cpu().numpy().tobytes() == mip.tobytes(), name
        only = ops.msa_mi(_dev(t), T.GAP, gaps=mode, want=("mi",))
        assert only.mip is None and only.mi.cpu().numpy().tobytes() == mi.tobytes(), name
        N, L = t.shape
        wide = torch.full((N, L + 13), 77, dtype=torch.uint8, device=DEV)                 # 77: a value the view must never show
        wide[:, 5:5 + L] = _dev(t)
        view = wide[:, 5:5 + L]
        assert view.stride(0) == L + 13
        strided = ops.msa_mi(view, T.GAP, gaps=mode)
        assert strided.mi.cpu().numpy().tobytes() == mi.tobytes() and strided.mip.cpu().numpy().tobytes() == mip.tobytes(), name
        vals = T.symbols(t)
        keep = np.arange(256, dtype=np.uint8)
        keep[vals] = vals + 100                                                           # keeps the symbols' order; the gap keeps its value
        assert ops.msa_mi(_dev(keep[t]), T.GAP, gaps=mode).mi.cpu().numpy().tobytes() == mi.tobytes(), name
        flip = np.arange(256, dtype=np.uint8)
        flip[vals] = vals[::-1] + 100                                                     # reverses it: another order of the sum
        _check_mi(f"{name} {mode} recoded", ops.msa_mi(_dev(flip[t]), T.GAP, gaps=mode).mi.cpu().numpy(), M.truth(name, mode),
                  4 * yards[mode][0])


@pytest.mark.parametrize("mode", M.MODES)
def test_mip_is_nan_where_the_total_is_zero(mode):
    one = ops.msa_mi(_dev(T.random_alignment(np.random.RandomState(1), 40, 1, 4, gaps=0.1)), T.GAP, gaps=mode)
    assert one.mi.shape == (1, 1) and float(one.mi[0, 0]) > 0 and bool(torch.isnan(one.mip).all())
    const = np.tile(np.array([4, 5, 6, 7, 4, 4], dtype=np.uint8), (30, 1))                # every column constant: mi is 0 everywhere
    rec = ops.msa_mi(_dev(const), T.GAP, gaps=mode)
    assert bool((rec.mi == 0).all())
    mip = rec.mip.cpu().numpy()
    assert np.isnan(mip).all() and not np.isinf(mip).any()


# ---- ops.apc alone ---------------------------------------------------------------------------------------------------------------------
def _check_apc(label, x, bar, zero_diagonal):
    """x: a float64 [L, L] tensor on the device, possibly a strided view."""
    host = x.cpu().numpy()
    want = M.apc_fsum(M.zero_diagonal(host) if zero_diagonal else host)
    got = ops.apc(x, zero_diagonal=zero_diagonal).cpu().numpy()
    assert got.shape == host.shape and got.dtype == np.float64 and np.isfinite(got).all(), label
    top = float(np.abs(want).max())
    dist = float(np.abs(got - want).max() / top)
    print(f"apc {label} zero_diagonal={zero_diagonal}: {dist:.3e} of the largest |entry| {top:.4f} (bar {bar:.3e})")
    assert dist <= bar, label
    if zero_diagonal:
        assert ops.apc(_dev(M.zero_diagonal(host))).cpu().numpy().tobytes() == got.tobytes(), label
    return got


@pytest.mark.parametrize("zero_diagonal", [False, True])
def test_apc_alone(yards, device_results, zero_diagonal):
    bar = 4 * max(y[1] for y in yards.values())                           # (no gap mode here: the larger of the two yardsticks)
    g = golden("apc_reference_l9.npz")
    rng = np.random.RandomState(29)
    maps = {"fixture general": _dev(g["x_general"]), "fixture symmetric": _dev(g["x_symmetric"]),
            "random 65": _dev(rng.rand(65, 65)), "random 2100": _dev(rng.rand(2100, 2100)),
            "invcov map": ops.msa_invcov(_dev(T.cases()["N70_L33_K4"]), T.GAP)}
    wide = torch.full((65, 80), 1e300, dtype=torch.float64, device=DEV)   # 1e300: a value the view must never show
    wide[:, 7:72] = maps["random 65"]
    for label, x in maps.items():
        got = _check_apc(label, x, bar, zero_diagonal)
        assert ops.apc(x, zero_diagonal=zero_diagonal).cpu().numpy().tobytes() == got.tobytes(), label       # two runs
        if label == "random 65":
            view = wide[:, 7:72]
            assert view.stride(0) == 80
            assert ops.apc(view, zero_diagonal=zero_diagonal).cpu().numpy().tobytes() == got.tobytes()      # ld > L
    if not zero_diagonal:                                                 # the fixture's own outputs: the reference's apc
        for name in ("general", "symmetric"):
            got = ops.apc(maps["fixture " + name]).cpu().numpy()
            assert np.abs(got - g["apc_" + name]).max() <= bar * np.abs(g["apc_" + name]).max(), name


def test_apc_in_place_and_its_refusal():
    lib = _lib.load()
    x = torch.rand(33, 33, dtype=torch.float64, device=DEV)
    want = ops.apc(x).cpu().numpy()
    ws = torch.empty(lib.rnamsm_apc_f64_workspace_bytes(33), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    y = x.clone()
    _lib.check(lib.rnamsm_apc_f64(y.data_ptr(), 33, 33, 0, y.data_ptr(), ws.data_ptr(), ws.numel(), stream))
    assert y.cpu().numpy().tobytes() == want.tobytes()                   # out == x with ld == L: allowed and the same bits
    wide = torch.zeros(33, 40, dtype=torch.float64, device=DEV)
    assert lib.rnamsm_apc_f64(wide.data_ptr(), 33, 40, 0, wide.data_ptr(), ws.data_ptr(), ws.numel(), stream) == -1
    assert lib.rnamsm_last_error().decode() == "apc_f64: out == x needs ld == L (ld=40, L=33)"
    assert bool((wide == 0).all())
    with pytest.raises(ValueError, match="square"):
        ops.apc(torch.zeros(3, 4, dtype=torch.float64, device=DEV))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_value_and_leave_the_outputs_untouched():
    rng = np.random.RandomState(3)
    many = torch.from_numpy(rng.randint(20, 37, size=(40, 6)).astype(np.uint8)).to(DEV)      # 17 distinct values
    many[:17, 0] = torch.arange(20, 37, dtype=torch.uint8, device=DEV)
    gaps = torch.full((5, 4), T.GAP, dtype=torch.uint8, device=DEV)
    for mode in M.MODES:
        with pytest.raises(_lib.RnamsmError, match="msa_mi: 17 distinct non-gap values, more than 16"):
            ops.msa_mi(many, T.GAP, gaps=mode)
        rec = ops.msa_mi(many, 36, gaps=mode)                                  # one of the 17 is the gap: 16 symbols, accepted
        assert np.isfinite(rec.mi.cpu().numpy()).all() and np.isfinite(rec.mip.cpu().numpy()).all()
        with pytest.raises(_lib.RnamsmError, match=r"msa_mi: the alignment holds nothing but the gap value 10 \(K = 0\)"):
            ops.msa_mi(gaps, T.GAP, gaps=mode)
        with pytest.raises(_lib.RnamsmError, match=r"msa_mi: N=1 outside \[2, 1048576\]"):
            ops.msa_mi(gaps[:1], T.GAP, gaps=mode)
        with pytest.raises(_lib.RnamsmError, match=r"msa_mi: L=4097 outside \[1, 4096\]"):
            ops.msa_mi(torch.zeros((2, 4097), dtype=torch.uint8, device=DEV), T.GAP, gaps=mode)
    # through the library itself: a gap mode that does not exist, no output, a workspace one byte short
    lib = _lib.load()
    t = _dev(T.cases()["N70_L17_K4"])
    N, L = t.shape
    need = lib.rnamsm_msa_mi_workspace_bytes(N, L)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    mi = torch.full((L, L), -7.0, dtype=torch.float64, device=DEV)
    mip = torch.full((L, L), -7.0, dtype=torch.float64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for args, text in (
            ((2, mi.data_ptr(), mip.data_ptr(), need), "msa_mi: gap_mode=2 is not 0 (pairwise) or 1 (state)"),
            ((0, None, None, need), "msa_mi: mi and mip are both NULL: nothing to compute"),
            ((1, mi.data_ptr(), mip.data_ptr(), need - 1),
             f"msa_mi: workspace of {need - 1} bytes is smaller than the {need} that N=70, L=17 need")):
        mode, p_mi, p_mip, nbytes = args
        rc = lib.rnamsm_msa_mi(t.data_ptr(), N, L, L, T.GAP, mode, p_mi, p_mip, ws.data_ptr(), nbytes, stream)
        assert rc == -1 and lib.rnamsm_last_error().decode() == text, (args, rc)
    torch.cuda.synchronize()
    assert bool((mi == -7.0).all()) and bool((mip == -7.0).all())
    _lib.check(lib.rnamsm_msa_mi(t.data_ptr(), N, L, L, T.GAP, 1, mi.data_ptr(), mip.data_ptr(), ws.data_ptr(), need, stream))
    assert bool((mi != -7.0).all()) and bool((mip != -7.0).all())              # the exact size is enough


def test_msa_mi_drops_cls(device_results):
    t = T.cases()["N70_L17_K4"]
    with_cls = np.concatenate([np.zeros((70, 1), dtype=np.int64), t.astype(np.int64)], 1)
    for mode in M.MODES:
        mi, mip = msa.msa_mi(with_cls, T.GAP, DEV, gaps=mode)
        assert mi.dtype == np.float64 and mi.tobytes() == device_results["N70_L17_K4", mode][0].tobytes()
        assert mip.tobytes() == device_results["N70_L17_K4", mode][1].tobytes()
    assert msa.msa_mi(with_cls, T.GAP, DEV)[0].tobytes() == device_results["N70_L17_K4", "pairwise"][0].tobytes()
