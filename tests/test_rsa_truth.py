"""The RSA restatement (tests/rsa_truth.py) against the reference's own outputs (tests/golden/rsa/, make_golden_rsa.py), and what it does
with a NaN or an inf in one embedding element (the truth tests/test_gpu_rsa_nonfinite.py stands on)."""
import os

import numpy as np
import pytest
import torch

import rsa_truth as T

G = T.GOLDEN


@pytest.fixture(scope="module")
def ref2drb():
    with np.load(os.path.join(G, "rsa_ref_2DRB_1.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def inputs2drb():
    with open(os.path.join(G, "2DRB_1.fasta")) as f:
        seq = "".join(line.strip() for line in f if not line.startswith(">"))
    return seq, np.load(os.path.join(G, "2DRB_1_emb.npy"))


def test_features_are_the_reference_input(ref2drb, inputs2drb):
    seq, emb = inputs2drb
    x = T.features(emb, seq, T.load_stats("oh"))
    assert x.shape == (773, 35) and x.dtype == np.float32
    assert float(x.astype(np.float64).sum()) == float(ref2drb["x_oh_sum"])
    assert (x[-1] == 1).all()


@pytest.mark.parametrize("k", [0, 1, 2])
def test_real_oh_models(ref2drb, inputs2drb, k):
    seq, emb = inputs2drb
    x = T.features(emb, seq, T.load_stats("oh"))
    sd = T.load_state(f"state_oh_{k}")
    l32, l64 = T.logits(x, sd, torch.float32), T.logits(x, sd, torch.float64)
    assert np.abs(l32 - ref2drb["logits_oh"][k]).max() <= 1e-6
    assert np.abs(l64 - ref2drb["logits_oh_f64"][k]).max() <= 1e-12
    assert np.abs(1 / (1 + np.exp(-l64)) - ref2drb["rsa_oh_f64"][k]).max() <= 1e-12


def test_real_emb_only_model(ref2drb, inputs2drb):
    seq, emb = inputs2drb
    x = T.features(emb, seq, T.load_stats("emb"), use_onehot=False)
    assert x.shape == (769, 35)
    sd = T.load_state("state_emb_0")
    assert np.abs(T.logits(x, sd, torch.float32) - ref2drb["logits_emb"][0]).max() <= 1e-6
    assert np.abs(T.logits(x, sd, torch.float64) - ref2drb["logits_emb_f64"][0]).max() <= 1e-12


@pytest.mark.parametrize("L", [1, 2, 3, 67])
def test_random_model(L):
    sd = T.load_random_state()
    with np.load(os.path.join(G, "rsa_ref_random.npz")) as z:
        x, r32, r64 = z[f"x_{L}"], z[f"logits_{L}"], z[f"logits_f64_{L}"]
    assert np.abs(T.logits(x, sd, torch.float32) - r32).max() <= 1e-6
    assert np.abs(T.logits(x, sd, torch.float64) - r64).max() <= 1e-12


def test_padding_is_zero_in_normalised_space_mask_included():
    """A restatement whose stem sees anything but 0 beyond the ends -- the mask channel reading 1 there, or the normalised image
    of a zero-padded RAW embedding -- must miss the L = 3 fixture (every position of it touches the padding or its neighbour)."""
    sd = T.load_random_state()
    with np.load(os.path.join(G, "rsa_ref_random.npz")) as z:
        x, r64 = z["x_3"], z["logits_f64_3"]
    mask_one = np.zeros(773)
    mask_one[-1] = 1.0
    st = T.load_stats("oh")
    raw = np.concatenate([np.zeros(4), -st["emb_mu"].astype(np.float64) / st["emb_std"], [0.0]])
    for pad in (mask_one, raw):
        assert np.abs(T.logits(x, sd, torch.float64, pad=pad) - r64).max() > 1e-3
    assert np.abs(T.logits(x, sd, torch.float64, pad=np.zeros(773)) - r64).max() <= 1e-12


def test_make_state_has_the_reference_names_and_shapes():
    ref = T.load_state("state_oh_0")
    mine = T.make_state(0)
    assert set(ref) == set(mine)
    assert all(ref[k].shape == mine[k].shape for k in ref)
    assert T.make_state(1, cin=769)["net.0.0.conv1.weight"].shape == (64, 769, 3)


def _poisoned_logits(kind, value, dtype):
    """make_state(11) at L = 70 with embedding element [40, 5] set to value; kind 'oh': the one-hot network (773 channels),
    'emb': the embedding-only one (769)."""
    L = 70
    rng = np.random.RandomState(70)
    st = T.load_stats(kind)
    emb = (st["emb_mu"] + st["emb_std"] * rng.standard_normal((L, 768))).astype(np.float32)
    seq = "".join(rng.choice(list("ACGUN"), L))
    sd = T.make_state(11, cin=773 if kind == "oh" else 769)
    clean = T.logits(T.features(emb, seq, st, use_onehot=kind == "oh"), sd, dtype)
    emb[40, 5] = value
    return clean, T.logits(T.features(emb, seq, st, use_onehot=kind == "oh"), sd, dtype)


@pytest.mark.parametrize("kind", ["oh", "emb"])
@pytest.mark.parametrize("value", ["nan", "inf", "-inf"])
def test_one_bad_embedding_element_makes_every_logit_nan(kind, value):
    """The squeeze mean and the attention spread a NaN over the whole member: all L logits NaN, none inf, in fp64 and fp32."""
    for dtype in (torch.float64, torch.float32):
        clean, y = _poisoned_logits(kind, float(value), dtype)
        assert np.isfinite(clean).all() and clean.shape == y.shape == (70,)
        assert np.isnan(y).all(), (kind, value, dtype, int(np.isnan(y).sum()))


def test_masked_comparison_reads_the_pattern_before_the_bars():
    clean64, nan64 = _poisoned_logits("oh", float("nan"), torch.float64)
    clean32, nan32 = (a.astype(np.float64) for a in _poisoned_logits("oh", float("nan"), torch.float32))
    assert T.compare_masked(nan32.astype(np.float32), nan64, nan32, "all NaN") == 0.0
    for got in (clean32.astype(np.float32), np.full(70, np.inf, dtype=np.float32)):       # laundered; inf in place of NaN
        with pytest.raises(AssertionError):
            T.compare_masked(got, nan64, nan32, "wrong on purpose")
    with pytest.raises(AssertionError):
        T.compare_masked(nan32.astype(np.float32), nan64, nan32, "not finite enough", min_finite=0.5)
    with pytest.raises(AssertionError):
        T.compare_masked(clean32.astype(np.float32), clean64, clean32, "no NaN to expect")
    # a truth that is part NaN: the bars on the rest
    half64, half32 = clean64.copy(), clean32.copy()
    half64[:30] = half32[:30] = np.nan
    got = half32.astype(np.float32)
    assert T.compare_masked(got, half64, half32, "half", min_finite=0.5) < 1e-4
    got[50] += np.float32(1e-3)
    with pytest.raises(AssertionError):
        T.compare_masked(got, half64, half32, "half, one logit off", min_finite=0.5)
