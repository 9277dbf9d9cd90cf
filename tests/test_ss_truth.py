"""The fp64 restatement of the RNA-MSM-SS head (tests/ss_truth.py) against the reference's own network on 2DRB_1
(ss_head_b2_l35.npz: two blocks, every parameter random), its windowed form (logits_window: the exact fp64 truth of a
block of a large map), the base-code rule, and what the restatement does with a NaN or an inf in one input element (the
truth the GPU tests of tests/test_gpu_ss_nonfinite.py stand on) with the masked comparison that reads it.  CPU only."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import ss_truth
from rnamsm import ss


def _fixture():
    g = np.load(os.path.join(GOLDEN, "ss_head_b2_l35.npz"))
    state = {k[3:]: g[k] for k in g.files if k.startswith("sd/")}
    atp = np.load(os.path.join(GOLDEN, "ss", "2DRB_1_atp.npy"))
    return g, state, ss_truth.features(atp, str(g["seq"]))


def test_features_are_the_reference_input():
    g, _, x = _fixture()
    assert x.shape == (128, 35, 35)
    np.testing.assert_array_equal(x[:8], g["x_onehot"])
    assert abs(x.sum() - float(g["x_sum"])) <= 1e-9 * abs(float(g["x_sum"]))


def test_fp64_restatement_matches_the_reference():
    g, state, x = _fixture()
    assert len(state) == 4 + 6 * 2 + 2
    y = ss_truth.logits(x, state)
    assert np.abs(y - g["logits_f64"]).max() <= 1e-10 * max(1.0, np.abs(g["logits_f64"]).max())
    assert np.abs(y - g["logits"]).max() <= 1e-5


def test_fp32_restatement_drift_is_small():
    _, state, x = _fixture()
    d = np.abs(ss_truth.logits(x, state, torch.float32) - ss_truth.logits(x, state)).max()
    assert d <= 1e-5, d


def test_make_state_covers_every_reference_parameter():
    import json
    names = json.load(open(os.path.join(GOLDEN, "ss_renet_b16_state.json")))
    sd = ss_truth.make_state(16, 0)
    assert [n for n, _ in names] == list(sd)
    assert all(list(sd[n].shape) == s for n, s in names)


def _window_case(L, num_blocks, seed):
    rng = np.random.RandomState(seed)
    atp = rng.exponential(size=(120, L, L))
    atp /= atp.sum(-1, keepdims=True)
    seq = "".join(rng.choice(list("ACGUN"), L))
    return atp, seq, ss_truth.make_state(num_blocks, seed)


@pytest.mark.parametrize("num_blocks, L, windows", [
    (16, 140, [((60, 76), (58, 90)), ((124, 140), (0, 16)), ((0, 16), (50, 82))]),
    (2, 40, [((16, 24), (14, 30)), ((0, 8), (32, 40)), ((20, 28), (34, 40))]),
], ids=["B16", "B2"])
def test_windowed_truth_is_the_full_map(num_blocks, L, windows):
    """logits_window at the receptive margin (1 + 3 B) is the full-map fp64 result bit for bit -- an interior window, a
    corner and a window on one border -- and one pixel less of margin is not (the helper does crop)."""
    atp, seq, state = _window_case(L, num_blocks, seed=num_blocks)
    full = ss_truth.logits(ss_truth.features(atp, seq), state)
    m = ss_truth.receptive_margin(num_blocks)
    dev = torch.from_numpy(atp)                    # a tensor crops like an array
    for rows, cols in windows:
        want = full[rows[0]:rows[1], cols[0]:cols[1]]
        got = ss_truth.logits_window(atp if rows[0] else dev, seq, state, rows, cols)
        assert got.shape == want.shape and np.array_equal(got, want), (rows, cols, np.abs(got - want).max())
        short = ss_truth.logits_window(atp, seq, state, rows, cols, margin=m - 1)
        assert not np.array_equal(short, want), (rows, cols)


def test_square_features_are_the_crop_of_the_whole_image():
    atp, seq, _ = _window_case(23, 1, seed=3)
    x = ss_truth.features(atp, seq)
    np.testing.assert_array_equal(ss_truth.features(atp[:, 5:17, 2:23], seq, (5, 17), (2, 23)), x[:, 5:17, 2:23])
    np.testing.assert_array_equal(ss_truth.features(atp, ss.base_codes(seq)), x)


def test_base_codes_follow_the_one_hot_encoder_rule():
    """Upstream: sklearn OneHotEncoder fitted on the four letters A, C, G, U, handle_unknown='ignore' -- exactly those four
    (upper case) get a one-hot vector, every other character (lowercase, T, N, IUPAC codes, gaps, non-ASCII) all zeros."""
    seq = "ACGUacguTtNnRYKMSWBDHVX-.*\xe9€UGCA"
    want = np.array([[1.0 if ch == b else 0.0 for b in ("A", "C", "G", "U")] for ch in seq])   # [L, 4]
    assert want.sum() == 8 and want[:4].tolist() == np.eye(4).tolist()
    codes = ss.base_codes(seq)
    assert codes.shape == (len(seq),) and codes.dtype == np.uint8
    onehot = np.zeros((len(seq), 4))
    ok = codes < 4
    onehot[np.nonzero(ok)[0], codes[ok]] = 1.0
    np.testing.assert_array_equal(onehot, want)
    assert (codes[~ok] == 255).all()
    L = len(seq)
    x = ss_truth.features(np.zeros((120, L, L)), seq)
    np.testing.assert_array_equal(x[0:4], np.broadcast_to(want.T[:, :, None], (4, L, L)))
    np.testing.assert_array_equal(x[4:8], np.broadcast_to(want.T[:, None, :], (4, L, L)))


# ---- a non-finite input element: the truth's pattern and the masked comparison ----------------------------------------------
NF_L, NF_BLOCKS, NF_STATE_SEED, NF_CASE_SEED = 48, 4, 21, 900
NF_VALUES = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


@pytest.fixture(scope="module")
def nf_clean():
    """The 4-block head at L = 48 on the clean image: state, maps, sequence, fp64 and fp32 logits.  Computed once."""
    state = ss_truth.make_state(NF_BLOCKS, seed=NF_STATE_SEED)
    atp, seq = ss_truth.small_maps_case(NF_L, NF_CASE_SEED)
    x = ss_truth.features(atp, seq)
    t64, t32 = ss_truth.logits(x, state, torch.float64), ss_truth.logits(x, state, torch.float32)
    assert np.isfinite(t64).all() and np.isfinite(t32).all()
    return state, atp, seq, t64, t32


@pytest.mark.parametrize("value", list(NF_VALUES))
def test_one_bad_element_poisons_its_receptive_square_and_nothing_else(nf_clean, value):
    """Plane 3, pixel (20, 22): NaN on the 27 x 27 = 729 pixels within receptive_margin(4) = 13 of it (rows 7..33, columns
    9..35), in fp64 and in fp32, for NaN and both infinities; no inf anywhere; the fp64 logits outside the square are the clean
    image's bit for bit (the tap-wise sum of a pixel depends on its own window alone)."""
    state, atp, seq, clean64, _ = nf_clean
    x = ss_truth.features(ss_truth.poisoned(atp, 3, (20, 22), NF_VALUES[value]), seq)
    square = ss_truth.receptive_square(NF_L, NF_BLOCKS, (20, 22))
    assert ss_truth.receptive_margin(NF_BLOCKS) == 13 and int(square.sum()) == 729
    assert square[7:34, 9:36].all() and not square[6].any() and not square[34].any() and not square[:, 8].any() and not square[:, 36].any()
    for dtype in (torch.float64, torch.float32):
        y = ss_truth.logits(x, state, dtype)
        assert int(np.isnan(y).sum()) == 729 and np.array_equal(np.isnan(y), square), (value, dtype, int(np.isnan(y).sum()))
        assert not np.isinf(y).any(), (value, dtype)
        if dtype == torch.float64:
            assert np.array_equal(y[~square].view(np.uint64), clean64[~square].view(np.uint64)), value


def test_the_square_is_clipped_at_a_corner(nf_clean):
    state, atp, seq, clean64, _ = nf_clean
    y = ss_truth.logits(ss_truth.features(ss_truth.poisoned(atp, 119, (0, 0), float("nan")), seq), state)
    square = ss_truth.receptive_square(NF_L, NF_BLOCKS, (0, 0))
    assert int(square.sum()) == 14 * 14 == 196 and square[:14, :14].all()
    assert np.array_equal(np.isnan(y), square) and not np.isinf(y).any()
    assert np.array_equal(y[~square].view(np.uint64), clean64[~square].view(np.uint64))


def test_masked_comparison_reads_the_pattern_before_the_bars(nf_clean):
    """compare_masked on the truth itself: it passes for a result that is NaN on the truth's square and as close as the fp32
    restatement elsewhere, and fails for each way of being wrong -- a laundered NaN (finite where the truth is NaN: what
    fmaxf(NaN, 0) = 0 gives), a NaN too many, an inf, an error beyond the bars on the finite side, a truth that is not finite
    enough, a truth without the NaN the caller expects."""
    state, atp, seq, clean64, clean32 = nf_clean
    x = ss_truth.features(ss_truth.poisoned(atp, 3, (20, 22), float("nan")), seq)
    t64, t32 = ss_truth.logits(x, state, torch.float64), ss_truth.logits(x, state, torch.float32).astype(np.float64)
    good = t32.astype(np.float32)
    d = ss_truth.compare_masked(good, t64, t32, "restatement", min_finite=0.3)
    assert 0.0 < d < 1e-4
    share = 1.0 - 729 / NF_L ** 2
    assert 0.68 <= share < 0.69
    ss_truth.compare_masked(good, t64, t32, "restatement", min_finite=share)

    def refused(got, a64=t64, a32=t32, **kw):
        with pytest.raises(AssertionError):
            ss_truth.compare_masked(got, a64, a32, "wrong on purpose", **{"min_finite": 0.3, **kw})

    laundered = np.where(np.isnan(good), np.float32(state["fc1.bias"][0]), good)
    refused(laundered)
    refused(clean32.astype(np.float32))                       # the clean image's logits: finite everywhere
    extra = good.copy()
    extra[0, 0] = np.nan
    refused(extra)
    inf = good.copy()
    inf[47, 47] = np.inf
    refused(inf)
    off = good.copy()
    off[40, 3] += np.float32(1e-3)
    refused(off)
    refused(good, min_finite=0.7)
    refused(clean32.astype(np.float32), clean64, clean32.astype(np.float64))        # expect_nan, and the truth has none
    ss_truth.compare_masked(clean32.astype(np.float32), clean64, clean32.astype(np.float64), "clean", min_finite=1.0, expect_nan=False)
    # nothing finite: the pattern alone
    nan = np.full((3, 3), np.nan)
    assert ss_truth.compare_masked(nan.astype(np.float32), nan, nan, "all NaN") == 0.0
    refused(np.zeros((3, 3), dtype=np.float32), nan, nan, min_finite=0.0)
