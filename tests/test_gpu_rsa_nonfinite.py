"""The RSA head on the GPU with a NaN or an inf in one embedding element.  In the reference network (tests/rsa_truth.py, pinned on
the CPU by tests/test_rsa_truth.py) the squeeze mean and the attention spread it over the whole member: every logit and every
probability of every ensemble member is NaN, none is inf.  A ReLU written as fmaxf(v, 0) loses the NaN at the poisoned positions
(fmaxf(NaN, 0) = 0), the squeeze mean never sees it and every position comes out finite.

The head works on tiles of 32 positions: the poisoned element lies at the first and the last position, at each side of the tile
seam (31, 32 at L = 65), in the first and in the last embedding channel.  Padding that is NaN and never read, and the neighbours
of a poisoned member in a packed batch, must stay finite and keep their bits."""
import numpy as np
import pytest
import torch

import rsa_truth as T
from test_gpu_rsa_head import _case, _ensemble

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUES = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
POSITIONS = {1: [0], 35: [0, 34], 65: [0, 31, 32, 64]}
CHANNELS = [0, 767]


@pytest.mark.parametrize("which", ["rand3", "emb1"])
@pytest.mark.parametrize("L", sorted(POSITIONS))
def test_one_bad_embedding_element_makes_every_output_nan(which, L):
    ens, states, kind = _ensemble(which)
    emb, seq = _case(L, 40 + L)
    clean = torch.from_numpy(emb).to(DEV)
    assert torch.isfinite(ens.logits(clean, seq)).all()
    for pos in POSITIONS[L]:
        for ch in CHANNELS:
            for name, value in VALUES.items():
                bad = clean.clone()
                bad[pos, ch] = value
                for what, out in (("logits", ens.logits(bad, seq)), ("probs", ens.predict(bad, seq))):
                    label = f"{which} L={L}: {name} at [{pos}, {ch}]: {what}"
                    assert out.shape == (len(ens), L), label
                    finite = int(torch.isfinite(out).sum())
                    assert torch.isnan(out).all(), f"{label}: {finite} of {out.numel()} finite, {int(torch.isinf(out).sum())} inf"
    # once per shape, through the masked comparison against the restatement's own answer to that input
    bad = emb.copy()
    bad[POSITIONS[L][-1], 767] = np.nan
    x = T.features(bad, seq, T.load_stats(kind), use_onehot=kind == "oh")
    t64 = np.stack([T.logits(x, sd, torch.float64) for sd in states])
    t32 = np.stack([T.logits(x, sd, torch.float32) for sd in states]).astype(np.float64)
    assert np.isnan(t64).all()
    T.compare_masked(ens.logits(torch.from_numpy(bad).to(DEV), seq).cpu().numpy(), t64, t32, f"{which} L={L}", min_finite=0.0)


@pytest.mark.parametrize("which", ["rand3", "emb1"])
@pytest.mark.parametrize("L", sorted(POSITIONS))
def test_nan_around_the_embedding_is_never_read(which, L):
    """The [L, 768] view inside a [L, 1000] buffer whose other columns are NaN, and row 0 of a [3, L + 1, 768] representation whose
    other rows are NaN: finite, and the contiguous copy's bits."""
    ens, _, _ = _ensemble(which)
    emb, seq = _case(L, 60 + L)
    e = torch.from_numpy(emb).to(DEV)
    ref_logits, ref_probs = ens.logits(e, seq), ens.predict(e, seq)
    assert torch.isfinite(ref_logits).all() and torch.isfinite(ref_probs).all()
    wide = torch.full((L, 1000), float("nan"), device=DEV)
    wide[:, 8:776] = e
    rep = torch.full((3, L + 1, 768), float("nan"), device=DEV)
    rep[0, 1:] = e
    for name, view in (("columns 8..775 of [L, 1000]", wide[:, 8:776]), ("row 0 of [3, L + 1, 768]", rep[0, 1:])):
        assert view.data_ptr() != e.data_ptr() and torch.equal(view, e), name
        assert torch.equal(ens.logits(view, seq), ref_logits), f"{which} L={L}: logits through {name}"
        assert torch.equal(ens.predict(view, seq), ref_probs), f"{which} L={L}: probs through {name}"
    assert int(torch.isnan(wide).sum()) == L * 232 and int(torch.isnan(rep).sum()) == (2 * (L + 1) + 1) * 768      # inputs untouched


PACKED_LS = [33, 1, 65, 35]
_PACKED = {}


def _packed(which, reverse):
    """rnamsm_rsa_head_packed on Ls = [33, 1, 65, 35] with member 2 alone poisoned (a NaN at the tile seam, position 32, channel 0),
    in list order or reversed -> per member (packed logits, packed probs, lone logits, lone probs) on the host.  Run once."""
    key = (which, reverse)
    if key not in _PACKED:
        ens, _, _ = _ensemble(which)
        cases = [_case(L, 80 + i) for i, L in enumerate(PACKED_LS)]
        embs = [torch.from_numpy(e).to(DEV) for e, _ in cases]
        embs[2][32, 0] = float("nan")
        seqs = [s for _, s in cases]
        order = list(reversed(range(4))) if reverse else list(range(4))
        logits = ens.logits_many([embs[b] for b in order], [seqs[b] for b in order])
        probs = ens.predict_many([embs[b] for b in order], [seqs[b] for b in order])
        out = [None] * 4
        for slot, b in enumerate(order):
            out[b] = (logits[slot].cpu(), probs[slot].cpu(), ens.logits(embs[b], seqs[b]).cpu(), ens.predict(embs[b], seqs[b]).cpu())
        _PACKED[key] = out
    return _PACKED[key]


@pytest.mark.parametrize("which", ["rand3", "emb1"])
@pytest.mark.parametrize("reverse", [False, True], ids=["in-order", "reversed"])
def test_neighbours_of_a_poisoned_member_keep_their_bits(which, reverse):
    out = _packed(which, reverse)
    K = len(_ensemble(which)[0])
    for b in (0, 1, 3):
        logits, probs, lone_logits, lone_probs = out[b]
        assert logits.shape == probs.shape == (K, PACKED_LS[b])
        assert torch.isfinite(logits).all() and torch.isfinite(probs).all(), f"member {b}: the poisoned member leaked"
        assert torch.equal(logits, lone_logits) and torch.equal(probs, lone_probs), f"member {b} differs from its lone run"


@pytest.mark.parametrize("which", ["rand3", "emb1"])
@pytest.mark.parametrize("reverse", [False, True], ids=["in-order", "reversed"])
def test_a_poisoned_member_of_a_batch_is_all_nan(which, reverse):
    logits, probs, lone_logits, lone_probs = _packed(which, reverse)[2]
    K = len(_ensemble(which)[0])
    assert logits.shape == probs.shape == (K, 65)
    for name, t in (("logits", logits), ("probs", probs), ("lone logits", lone_logits), ("lone probs", lone_probs)):
        assert torch.isnan(t).all(), f"member 2: {name}: {int(torch.isfinite(t).sum())} of {t.numel()} finite"
