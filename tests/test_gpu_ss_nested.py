"""rnamsm_ss_nested on the device against the truth of tests/ss_nested_truth.py, byte for byte: the partner vector, the score, the
dot-bracket line and the two bodies; and the property check on every result (a valid, nested matching of allowed pairs whose
weights sum to the score).  Shapes: the edges of the tile schedule (one tile, its edge, two tiles, the first outer phase at 129 and
197, two outer k-tiles at 260), every input family of tests/ss_pairs_cases.py, L = 1024 against the truth once and L = 4096 on a
planted input whose optimum is known by construction; then packed groups, determinism and the parameters' ranges."""
import numpy as np
import pytest
import torch

from rnamsm import _lib, ops, ss
import ss_pairs_cases as C
import ss_nested_truth as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _device_inputs(prob, seq):
    return torch.from_numpy(np.ascontiguousarray(prob)).to(DEV), torch.from_numpy(ss.letter_codes(seq)).to(DEV)


def _host(result):
    """(partner, counts, ct body, bpseq body, dbn) of one device result, cut to the counted bytes."""
    partner, counts, ct, bp, dbn = (t.cpu().numpy() for t in result)
    return partner, counts, ct[:counts[1]].tobytes(), bp[:counts[2]].tobytes(), dbn.tobytes()


def _decode(prob, seq, theta=0.516, min_loop=3):
    return _host(ss.nested_structure(*_device_inputs(prob, seq), theta, min_loop))


def _compare(key, case, got):
    prob, seq, theta, min_loop = case
    partner, counts, ct, bp, dbn = got
    want_partner, want_score, want_ct, want_bp, want_dbn = T.expected(key, prob, seq, theta, min_loop)
    assert counts[4] == want_score, (key, counts.tolist(), want_score)
    assert partner.tolist() == want_partner.tolist(), key
    assert counts[3] == 0 and (ct, bp, dbn) == (want_ct, want_bp, want_dbn), key
    T.check_properties(prob, theta, min_loop, partner, counts, want_score)


@pytest.mark.parametrize("key", list(T.small_cases()))
def test_small_cases_equal_the_truth(key):
    case = T.small_cases()[key]
    _compare(key, case, _decode(*case))


def test_nothing_or_exactly_one_pair_at_the_smallest_lengths():
    for min_loop in (0, 3):
        for L in (1, 2, min_loop + 1, min_loop + 2):
            prob = np.full((L, L), 0.9, dtype=np.float32)
            partner, counts, _, _, dbn = _decode(prob, C.seq_for(L, L), 0.516, min_loop)
            if L <= min_loop + 1:
                assert counts[0] == 0 and counts[4] == 0 and not partner.any() and dbn == b"." * L
            else:                                              # the one pair that can form: (0, L - 1)
                assert counts[0] == 1 and partner.tolist() == [L] + [0] * (L - 2) + [1]
                assert dbn == b"(" + b"." * (L - 2) + b")"
                assert counts[4] == int(T.weights(prob, 0.516, min_loop)[0, L - 1])


def test_the_heavier_of_two_crossing_helices_wins_whole():
    prob, seq, theta, min_loop = T.small_cases()["pseudoknot_40"]
    partner, counts, _, _, _ = _decode(prob, seq, theta, min_loop)
    assert T.pairs_of(partner) == [(2 + n, 25 - n) for n in range(6)] and counts[0] == 6


def test_l1024_against_the_truth():
    prob, seq = C.helix_noise_1024(), C.seq_for(1024, 9)
    _compare("helix_1024", (prob, seq, 0.516, 3), _decode(prob, seq))
    partner = T.expected("helix_1024", prob, seq)[0]
    assert len(T.pairs_of(partner)) > 400


def test_l4096_planted_structure():
    prob, want_partner, want_score = T.planted_4096()
    seq = C.seq_for(4096, 4)
    partner, counts, ct, bp, dbn = _decode(prob, seq)
    assert counts[4] == want_score and counts[0] == len(T.pairs_of(want_partner))
    assert np.array_equal(partner, want_partner)
    assert (ct, bp, dbn) == T.bodies(want_partner, seq)
    T.check_properties(prob, 0.516, 3, partner, counts, want_score)


PACK_LS = (1, 5, 64, 65, 197, 33)


def _pack_members():
    return [(C.random_sigmoid(L, 300 + L, 0.0), C.seq_for(L, 300 + L)) for L in PACK_LS]


def test_packed_members_equal_their_lone_calls_and_a_poisoned_member_harms_nobody():
    members = _pack_members()
    lone = [_decode(p, s) for p, s in members]
    for n, (p, s) in enumerate(members):
        _compare(f"pack_{n}", (p, s, 0.516, 3), lone[n])

    def run(ms):
        probs, letters = zip(*(_device_inputs(p, s) for p, s in ms))
        return [_host(r) for r in ss.nested_structure_many(probs, letters)]

    def same(a, b):
        return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))

    got = run(members)
    assert all(same(g, w) for g, w in zip(got, lone))
    poisoned = list(members)
    poisoned[3] = (np.full((65, 65), np.nan, dtype=np.float32), members[3][1])
    got = run(poisoned)
    for n, (g, w) in enumerate(zip(got, lone)):
        if n == 3:
            assert g[1][0] == 0 and g[1][4] == 0 and g[4] == b"." * 65
        else:
            assert same(g, w), n
    assert got[4][1][0] > 20                                   # the neighbour with an outer phase found its pairs


def test_forty_members_cross_the_descriptor_chunk():
    members = [(C.ties(L, L), C.seq_for(L, L)) for L in [3 + (7 * n) % 70 for n in range(40)]]
    probs, letters = zip(*(_device_inputs(p, s) for p, s in members))
    got = [_host(r) for r in ss.nested_structure_many(probs, letters)]
    for n, ((p, s), g) in enumerate(zip(members, got)):
        _compare(f"forty_{n}", (p, s, 0.516, 3), g)


def test_two_runs_give_the_same_bytes():
    prob, seq = C.ties(260, 11), C.seq_for(260, 11)
    a, b = _decode(prob, seq), _decode(prob, seq)
    assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))
    _compare("ties_260", (prob, seq, 0.516, 3), a)


def test_arguments_out_of_range_are_refused():
    probs, letters = _device_inputs(C.random_sigmoid(8, 1), C.seq_for(8, 1))
    for theta in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="theta"):
            ss.nested_structure(probs, letters, theta)
    for min_loop in (-1, 33):
        with pytest.raises(ValueError, match="min_loop"):
            ss.nested_structure(probs, letters, 0.5, min_loop)
    with pytest.raises(ValueError):
        ops.ss_nested(probs, letters[:-1])
    lib = _lib.load()
    out = torch.zeros(64, dtype=torch.int32, device=DEV)
    rc = lib.rnamsm_ss_nested(probs.data_ptr(), letters.data_ptr(), 8, 0.516, 3, out.data_ptr(), out.data_ptr(), out.data_ptr(),
                              out.data_ptr(), out.data_ptr(), out.data_ptr(), 16, None)
    assert rc == -1 and "32768 needed" in lib.rnamsm_last_error().decode()
    torch.cuda.synchronize()
    assert not out.any()                                       # refused before anything was enqueued
