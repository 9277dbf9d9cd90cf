"""The SS head on a stitched long alignment (rnamsm_ss_head_long, SSPredictor.predict_long / logits_long): up to L = 1024 the bits
of ops.ss_head; beyond, the bits of ops.ss_head on 1024 x 1024 crops whose origin is a multiple of 16 -- the tiles then coincide,
a pixel's sum has one fixed order in both calls and an out-of-image tap adds +0 -- on every pixel whose receptive square lies
inside the crop or is cut only by the true image border; and ss_truth's fp64 window around the seam pixel (1024, 1024)."""
import numpy as np
import pytest
import torch

from rnamsm import _lib, ss
import ss_truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NB = 4
M = ss_truth.receptive_margin(NB)


@pytest.fixture(scope="module")
def state():
    return ss_truth.make_state(NB, seed=77)


@pytest.fixture(scope="module")
def model(state):
    m = ss.SSPredictor(NB)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV)


def _maps(L: int, seed: int) -> torch.Tensor:
    """Random maps made on the device (120 L^2 floats: 8 GB at the limit), in the range of attention probabilities."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(120, L, L, device=DEV, generator=g).mul_(0.1)


def _codes(L: int, seed: int) -> torch.Tensor:
    return torch.from_numpy(np.random.RandomState(seed).choice(np.array([0, 1, 2, 3, 255], np.uint8), L)).to(DEV)


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def _comparable(L: int, origin: int, n: int = 1024) -> slice:
    """The rows (and columns) of the crop [origin, origin + n) whose receptive interval lies inside it or is cut only by the image."""
    lo = origin if origin == 0 else origin + M
    hi = origin + n if origin + n == L else origin + n - M
    return slice(lo, hi)


def _check_crop(model, atp, codes, long_logits, origin: int) -> int:
    L = atp.shape[-1]
    crop = model.logits(atp[:, origin:origin + 1024, origin:origin + 1024], codes[origin:origin + 1024])
    s = _comparable(L, origin)
    c = slice(s.start - origin, s.stop - origin)
    want, got = _bits(crop[c, c]), _bits(long_logits[s, s])
    assert (got == want).all(), (origin, int((got != want).sum()))
    return want.size


@pytest.mark.parametrize("L", [1, 17, 100])
def test_up_to_1024_logits_and_probabilities_are_the_bits_of_the_existing_head(model, L):
    atp, codes = _maps(L, L), _codes(L, L)
    assert (_bits(model.logits_long(atp, codes)) == _bits(model.logits(atp, codes))).all()
    assert (_bits(model.predict_long(atp, codes)) == _bits(model.predict(atp, codes))).all()


@pytest.fixture(scope="module")
def at_1040(model):
    atp, codes = _maps(1040, 5), _codes(1040, 5)
    return atp, codes, model.logits_long(atp, codes)


def test_65_tiles_a_side_equal_the_existing_head_on_two_crops(model, at_1040):
    atp, codes, logits = at_1040
    assert logits.shape == (1040, 1040) and bool(torch.isfinite(logits).all())
    assert _check_crop(model, atp, codes, logits, 0) == (1024 - M) ** 2
    assert _check_crop(model, atp, codes, logits, 16) == (1024 - M) ** 2
    # together the two crops cover the 65th tile row and column: rows 1024 .. 1039 are compared in the second
    assert _comparable(1040, 16).stop == 1040 and _comparable(1040, 0).start == 0


def test_the_seam_pixel_1024_against_fp64(state, at_1040):
    atp, codes, logits = at_1040
    rows = cols = (1016, 1032)
    seq = codes.cpu().numpy()
    t64 = ss_truth.logits_window(atp, seq, state, rows, cols, torch.float64)
    t32 = ss_truth.logits_window(atp, seq, state, rows, cols, torch.float32)
    ss_truth.compare(logits[1016:1032, 1016:1032].cpu().numpy(), t64, t32, "L=1040 window around (1024, 1024)")


def test_at_the_limit_the_far_corner_equals_the_existing_head(model):
    """L = 4096: pixel offsets beyond 2^31 bytes in the maps (plane 119 starts at 8 GB less 64 MB) and in the workspace images
    (pixel * 48 floats reaches 3.2 GB): the case a 32-bit offset breaks."""
    L = _lib.LONG_MAX_L
    atp, codes = _maps(L, 9), _codes(L, 9)
    logits = model.logits_long(atp, codes)
    assert logits.shape == (L, L)
    assert _check_crop(model, atp, codes, logits, 3072) == (1024 - M) ** 2
    assert bool(torch.isfinite(logits).all())


def test_limits_and_arithmetic_of_the_long_route(model):
    one = torch.zeros(1, device=DEV)                                      # a view of one element: only the shape is looked at
    with pytest.raises(ValueError, match="limit of 4096"):
        model.predict_long(one.expand(120, 4097, 4097), "A" * 4097)
    with pytest.raises(ValueError, match="limit of 1024"):
        model.predict(one.expand(120, 1025, 1025), "A" * 1025)
    m16 = ss.SSPredictor(NB, gemm_dtype="bf16")
    with pytest.raises(ValueError, match="fp32 only"):
        m16.predict_long(torch.zeros(120, 4, 4, device=DEV), "ACGU")
