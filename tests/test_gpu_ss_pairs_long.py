"""The long structure decoding on the GPU (rnamsm_ss_pairs_long, ops.ss_pairs_long): up to L = 1024 its four results are the bytes
of ops.ss_pairs; beyond, those of the host function and writer (ss_pairs_cases.expected), up to the limit of 4096.  Every comparison
is == on integers or bytes."""
import numpy as np
import pytest
import torch

from rnamsm import _lib, ops, ss
import ss_pairs_cases as C
import ss_pairs_long_cases as LC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(prob: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(prob, dtype=np.float32)).to(DEV)


def _letters(seq: str) -> torch.Tensor:
    return torch.from_numpy(ss.letter_codes(seq)).to(DEV)


def _host(out):
    partner, counts, ct, bp = (t.cpu().numpy() for t in out)
    L = partner.shape[0]
    assert partner.dtype == np.int32 and counts.dtype == np.int32 and counts.shape == (4,)
    assert ct.shape == (32 * L,) and bp.shape == (12 * L,) and ct.dtype == np.uint8
    assert 0 < counts[1] <= 32 * L and 0 < counts[2] <= 12 * L
    return partner.tolist(), counts.tolist(), ct[:counts[1]].tobytes(), bp[:counts[2]].tobytes()


def _long(prob: np.ndarray, seq: str):
    return _host(ops.ss_pairs_long(_dev(prob), _letters(seq)))


def _check(key: str, prob: np.ndarray, seq: str, got):
    pairs, partner, ct, bp, _, _ = C.expected(key, prob, seq)
    g_partner, g_counts, g_ct, g_bp = got
    assert g_partner == partner.tolist(), key
    assert g_counts == [len(pairs), len(ct), len(bp), 0], key
    assert g_ct == ct and g_bp == bp, key
    return pairs


def test_up_to_1024_the_bytes_are_those_of_the_existing_kernel():
    """Every standard case (L = 1, 64, 65, 70 ... among them), L = 35 and 64 of the existing test's generator, and L = 1024."""
    cases = dict(C.standard_cases())
    for L in (35, 64):
        cases[f"random_{L}"] = (C.random_sigmoid(L, 100 + L, -4.0), C.seq_for(L, L))
    cases["helix_1024"] = (C.helix_noise_1024(), C.seq_for(1024, 9))
    assert {1, 35, 64, 65, 1024} <= {len(s) for _, s in cases.values()}
    for key, (prob, seq) in cases.items():
        got = _long(prob, seq)
        assert got == _host(ops.ss_pairs(_dev(prob), _letters(seq))), key
        _check(key, prob, seq, got)


@pytest.mark.parametrize("L", [1025, 2049, 2304])
def test_beyond_one_base_per_thread_the_bytes_are_the_host_path_s(L):
    for kind in ("helix", "blocks", "thin"):
        key, prob, seq = LC.case(kind, L)
        pairs = _check(key, prob, seq, _long(prob, seq))
        assert 0 < len(pairs) < LC.edges_above(prob), key                 # the host function removed at least one pair
    key, prob, seq = LC.case("helix", L)
    pairs, _, want_ct, _, _, _ = C.expected(key, prob, seq)
    assert (300, 802) in pairs and (300, 800) not in pairs and (300, 801) not in pairs      # ... over two rounds
    assert L != 2304 or len(want_ct) > 65536


def test_at_the_limit_on_a_sparse_sprinkled_matrix():
    key, prob, seq = LC.case("thin", _lib.LONG_MAX_L)
    assert np.isnan(prob).any() and np.isposinf(prob).any() and np.isneginf(prob).any()
    got = _long(prob, seq)
    pairs, partner, ct, bp = LC.expected_without_prob("thin", _lib.LONG_MAX_L)
    assert got == (partner.tolist(), [len(pairs), len(ct), len(bp), 0], ct, bp)
    assert 0 < len(pairs) < LC.edges_above(prob)
    assert got == _long(prob, seq)                                        # two runs: the same bytes
    assert len(got[2]) > 65536 and max(got[0]) > 4000


def test_nan_is_never_an_edge_and_plus_inf_is_one():
    L = 1500
    prob = np.full((L, L), np.nan, dtype=np.float32)
    prob[3, 1400], prob[1400, 3] = np.inf, np.nan
    prob[7, 1100], prob[8, 1100] = -np.inf, np.nextafter(np.float32(0.516), np.float32(1))
    partner = _long(prob, C.seq_for(L, 1))[0]
    want = [0] * L
    want[3], want[1400], want[8], want[1100] = 1401, 4, 1101, 9
    assert partner == want


def test_a_letter_outside_ascii_sets_the_fallback_word():
    key, prob, seq = LC.case("thin", 1025)
    letters = ss.letter_codes(seq).copy()
    letters[1024] = 200
    out = ops.ss_pairs_long(_dev(prob), torch.from_numpy(letters).to(DEV))
    assert out[1].cpu().tolist()[3] == 1 and out[0].cpu().tolist() == C.expected(key, prob, seq)[1].tolist()


def test_the_existing_entry_point_keeps_its_limit_and_the_long_one_has_its_own():
    with pytest.raises(ValueError, match=r"\[1, 1024\]"):
        ops.ss_pairs(torch.zeros(1025, 1025, device=DEV), torch.zeros(1025, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match=r"\[1, 4096\]"):
        ops.ss_pairs_long(torch.zeros(4097, 4097, device=DEV), torch.zeros(4097, dtype=torch.uint8, device=DEV))
