"""The `.prob` text of a long alignment written on the GPU (rnamsm_ss_prob_text_long, ops.ss_prob_text_long): up to L = 1024 the
bytes of ops.ss_prob_text; beyond, np.savetxt of the same rows.  Every comparison is == on bytes."""
import numpy as np
import pytest
import torch

from rnamsm import _lib, ops
import dec19_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _sigmoid_case(L: int, seed: int) -> torch.Tensor:
    """Sigmoid outputs of logits N(-6, 6) in fp32, made on the device: down to subnormal probabilities, up to 1.0 itself."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.sigmoid(torch.randn(L, L, device=DEV, generator=g).mul_(6.0).sub_(6.0))


def _row_bytes(text: torch.Tensor, L: int, row: int) -> bytes:
    return text[25 * L * row:25 * L * (row + 1)].cpu().numpy().tobytes()


@pytest.mark.parametrize("L", [35, 1024])
def test_up_to_1024_the_bytes_are_those_of_the_existing_kernel(L):
    prob = _sigmoid_case(L, L)
    (text, fb), (want, want_fb) = ops.ss_prob_text_long(prob), ops.ss_prob_text(prob)
    assert text.shape == (25 * L * L,) and int(fb.item()) == int(want_fb.item()) == 0
    assert bool((text == want).all())
    assert _row_bytes(text, L, L - 1) == C.savetxt_bytes(prob[L - 1:].cpu().numpy())


def test_l1030_equals_savetxt_on_the_first_a_middle_and_the_last_row():
    L = 1030
    prob = _sigmoid_case(L, 3)
    text, fb = ops.ss_prob_text_long(prob)
    assert text.dtype == torch.uint8 and text.shape == (25 * L * L,) and fb.shape == (1,) and int(fb.item()) == 0
    host = prob.cpu().numpy()
    for row in (0, 517, 1029):
        assert _row_bytes(text, L, row) == C.savetxt_bytes(host[row:row + 1]), row
    ends = text.view(L, 25 * L)[:, -1]
    assert bool((ends == ord("\n")).all())                                # a '\n' at each row end ...
    seps = text.view(L * L, 25)[:, 24].reshape(L, L)[:, :-1]
    assert bool((seps == ord("\t")).all())                                # ... and a '\t' behind every other record


def test_an_element_above_one_sets_the_fallback_word():
    L = 1030
    prob = _sigmoid_case(L, 4)
    prob[1029, 1029] = 1.5
    assert int(ops.ss_prob_text_long(prob)[1].item()) == 1
    prob[1029, 1029] = float("nan")
    assert int(ops.ss_prob_text_long(prob)[1].item()) == 1
    prob[1029, 1029] = 1.0
    assert int(ops.ss_prob_text_long(prob)[1].item()) == 0


def test_at_the_limit_the_last_block_and_the_tail():
    """L = 4096: 419 MB of text; the last block of 256 elements starts at byte 25 (L^2 - 256), beyond 2^28."""
    L = _lib.LONG_MAX_L
    prob = _sigmoid_case(L, 5)
    text, fb = ops.ss_prob_text_long(prob)
    assert text.shape == (25 * L * L,) and int(fb.item()) == 0
    tail = text[-6400:].cpu().numpy().tobytes()
    want = C.savetxt_bytes(prob[L - 1:, L - 256:].cpu().numpy())
    assert tail == want and tail.endswith(b"\n")
    assert _row_bytes(text, L, 0) == C.savetxt_bytes(prob[:1].cpu().numpy())
    assert _row_bytes(text, L, 2049) == C.savetxt_bytes(prob[2049:2050].cpu().numpy())


def test_the_limits():
    with pytest.raises(ValueError, match=r"\[1, 1024\]"):
        ops.ss_prob_text(torch.zeros(1025, 1025, device=DEV))
    with pytest.raises(ValueError, match=r"\[1, 4096\]"):
        ops.ss_prob_text_long(torch.zeros(1, device=DEV).expand(4097, 4097))
