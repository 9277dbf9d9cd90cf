"""The fp64 restatement of the RNA-MSM-SS head (tests/ss_truth.py) against the reference's own network on 2DRB_1
(ss_head_b2_l35.npz: two blocks, every parameter random).  CPU only."""
import os

import numpy as np
import torch

from conftest import GOLDEN
import ss_truth


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
