"""The SS head on the GPU with a NaN or an inf in one input element: the reference network (nn.ReLU, LayerNorm, zero-padded
convolutions; tests/ss_truth.py, pinned on the CPU by tests/test_ss_truth.py) turns it into NaN on the receptive square of the
poisoned pixel -- within receptive_margin(B) = 1 + 3 B pixels, clipped at the border -- and leaves every other logit untouched.
The HIP head must do exactly that: NaN where the truth is NaN, no inf, the truth's bars on the rest (ss_truth.compare_masked), and
the finite logits bit-identical to the same head's on the clean image, since a pixel's arithmetic depends on its own window
alone.  A ReLU written as fmaxf(v, 0) fails here: fmaxf(NaN, 0) = 0, and the head returns a finite map whose poisoned pixels
carry fc1.bias.

L = 48 is 3 x 3 tiles of 16 x 16 pixels: the poisoned pixel lies in the middle of a tile (20, 22), on a seam (15, 16) and at the
corners; the planes are the first and the last of the 120.  Packed, the poisoned member's corner pixels are the ones that lie
next to its neighbours in the shared images."""
import numpy as np
import pytest
import torch

from rnamsm import ss
import ss_truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L4, STATE4_SEED, CASE_SEED = 48, 21, 900
NAN, INF = float("nan"), float("inf")
# every position with NaN, the two infinities at the tile middle and at the seam; both planes meet every kind of position
CASES = [
    ("nan", NAN, 0, (20, 22)), ("nan", NAN, 119, (15, 16)), ("nan", NAN, 119, (0, 0)), ("nan", NAN, 0, (47, 47)),
    ("+inf", INF, 119, (20, 22)), ("-inf", -INF, 0, (20, 22)), ("+inf", INF, 0, (15, 16)), ("-inf", -INF, 119, (15, 16)),
]


def _predictor(state, num_blocks):
    m = ss.SSPredictor(num_blocks)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same(got, want):
    """NaN at the same positions, the same bits everywhere else."""
    g, w = got.detach().cpu(), want.detach().cpu()
    ok = ~torch.isnan(w)
    return g.shape == w.shape and torch.equal(torch.isnan(g), torch.isnan(w)) and np.array_equal(_bits(g[ok]), _bits(w[ok]))


def _truths(atp, seq, state):
    x = ss_truth.features(atp, seq)
    return ss_truth.logits(x, state, torch.float64), ss_truth.logits(x, state, torch.float32).astype(np.float64)


class _Head:
    """A head, one clean image and the head's own logits on it, computed once and left unchanged."""

    def __init__(self, num_blocks, state_seed, L, case_seed):
        self.num_blocks, self.L = num_blocks, L
        self.state = ss_truth.make_state(num_blocks, seed=state_seed)
        self.model = _predictor(self.state, num_blocks)
        self.atp, self.seq = ss_truth.small_maps_case(L, case_seed)
        assert "N" in self.seq and float(self.atp.max()) < 0.1
        self.clean = self.model.logits(torch.from_numpy(self.atp).to(DEV), self.seq).cpu()
        assert torch.isfinite(self.clean).all()

    def check(self, plane, pixel, value, label):
        """One poisoned element: the masked comparison with the truth, the finite logits' bits, the probabilities' pattern."""
        bad = ss_truth.poisoned(self.atp, plane, pixel, value)
        dev = torch.from_numpy(bad).to(DEV)
        logits, probs = self.model.logits(dev, self.seq).cpu(), self.model.predict(dev, self.seq).cpu()
        t64, t32 = _truths(bad, self.seq, self.state)
        square = ss_truth.receptive_square(self.L, self.num_blocks, pixel)
        assert np.array_equal(np.isnan(t64), square), label          # the truth itself: tests/test_ss_truth.py
        ss_truth.compare_masked(logits.numpy(), t64, t32, label, min_finite=0.3)
        fin = torch.from_numpy(~square)
        assert np.array_equal(_bits(logits[fin]), _bits(self.clean[fin])), f"{label}: a finite logit moved with the poisoned pixel"
        assert torch.equal(torch.isnan(probs), torch.isnan(logits)), f"{label}: probs are not NaN exactly where the logits are"
        assert not torch.isinf(probs).any(), label
        return logits


@pytest.fixture(scope="module")
def head4():
    return _Head(4, STATE4_SEED, L4, CASE_SEED)


@pytest.mark.parametrize("name, value, plane, pixel", CASES, ids=[f"{n}-plane{p}-{y}-{x}" for n, _, p, (y, x) in CASES])
def test_one_bad_element_is_nan_on_its_receptive_square_only(head4, name, value, plane, pixel):
    logits = head4.check(plane, pixel, value, f"4 blocks, L=48, {name} at plane {plane}, pixel {pixel}")
    m = ss_truth.receptive_margin(4)
    side = lambda c: min(L4, c + m + 1) - max(0, c - m)          # noqa: E731
    assert int(torch.isnan(logits).sum()) == side(pixel[0]) * side(pixel[1])


def test_sixteen_blocks_at_a_corner():
    """Margin 49: 50 x 50 = 2500 of the 64 x 64 logits are NaN, the other 39 % finite and the clean run's bits."""
    head = _Head(16, 22, 64, 901)
    assert ss_truth.receptive_margin(16) == 49
    logits = head.check(0, (0, 0), NAN, "16 blocks, L=64, nan at plane 0, pixel (0, 0)")
    assert int(torch.isnan(logits).sum()) == 2500
    assert torch.isnan(logits[:50, :50]).all() and torch.isfinite(logits[50:]).all() and torch.isfinite(logits[:, 50:]).all()


def test_nan_between_the_planes_is_never_read(head4):
    """The maps through a plane stride larger than L*L, the gaps filled with NaN: finite everywhere, the contiguous call's bits."""
    n = L4 * L4
    wide = torch.full((120, n + 13), NAN, device=DEV)
    wide[:, :n] = torch.from_numpy(head4.atp).to(DEV).reshape(120, n)
    view = wide[:, :n].view(120, L4, L4)
    assert view.stride() == (n + 13, L4, 1) and torch.isnan(wide[:, n:]).all()
    logits = head4.model.logits(view, head4.seq).cpu()
    assert torch.isfinite(logits).all()
    assert np.array_equal(_bits(logits), _bits(head4.clean))
    probs = head4.model.predict(view, head4.seq).cpu()
    assert torch.isfinite(probs).all()
    assert np.array_equal(_bits(probs), _bits(head4.model.predict(torch.from_numpy(head4.atp).to(DEV), head4.seq).cpu()))


@pytest.mark.parametrize("reverse", [False, True], ids=["in-order", "reversed"])
def test_a_poisoned_member_of_a_batch_stays_alone(head4, reverse):
    """rnamsm_ss_head_packed, Ls = [17, 48, 1, 35]: member 1 carries a NaN in its first and in its last pixel, the two that lie
    next to its neighbours' pixels in the shared images.  Members 0, 2 and 3 are finite and their lone runs' bits; member 1 is its
    lone poisoned run, NaN positions included (what that run must be: the corner cases above)."""
    model = head4.model
    Ls = [17, 48, 1, 35]
    cases = [ss_truth.small_maps_case(L, 910 + i) if L != L4 else (head4.atp, head4.seq) for i, L in enumerate(Ls)]
    bad = ss_truth.poisoned(ss_truth.poisoned(cases[1][0], 0, (0, 0), NAN), 119, (47, 47), NAN)
    atps = [torch.from_numpy(bad if b == 1 else a).to(DEV) for b, (a, _) in enumerate(cases)]
    seqs = [s for _, s in cases]
    lone = [(model.logits(a, s).cpu(), model.predict(a, s).cpu()) for a, s in zip(atps, seqs)]
    order = list(reversed(range(4))) if reverse else list(range(4))
    logits = model.logits_many([atps[b] for b in order], [seqs[b] for b in order])
    probs = model.predict_many([atps[b] for b in order], [seqs[b] for b in order])
    for slot, b in enumerate(order):
        for kind, got, want in (("logits", logits[slot].cpu(), lone[b][0]), ("probs", probs[slot].cpu(), lone[b][1])):
            label = f"{kind} of member {b} (L = {Ls[b]}) in slot {slot}"
            if b != 1:
                assert torch.isfinite(got).all(), f"{label}: the poisoned neighbour leaked"
            assert _same(got, want), f"{label} differ from the lone run's"
    slot1 = order.index(1)
    assert torch.equal(torch.isnan(probs[slot1]), torch.isnan(logits[slot1]))
