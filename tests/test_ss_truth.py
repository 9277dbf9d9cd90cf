"""The fp64 restatement of the RNA-MSM-SS head (tests/ss_truth.py) against the reference's own network on 2DRB_1
(ss_head_b2_l35.npz: two blocks, every parameter random), its windowed form (logits_window: the exact fp64 truth of a
block of a large map) and the base-code rule.  CPU only."""
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
