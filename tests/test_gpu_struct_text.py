"""The three structure decoders end in one tail (csrc/struct_text.h: emit_struct_text).  A planted structure that every decoder
must return unchanged -- mutually nested helices at 0.9 on a zero background, one pair per base, every hairpin with three unpaired
bases (tests/test_struct_text_host.py confirms the claim against the CPU truth) -- goes through each of them: the partner vector,
counts[0..3] and the two bodies are the same bytes from every decoder, and the bytes Python formats.  Lengths: one base, the wave
edges, the digit edge at 1000, the limit of one base per thread, one past it and the long limit; then a packed call whose shorter
members idle under the largest member's block size."""
import numpy as np
import pytest
import torch

from rnamsm import ops
import struct_text_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _inputs(L):
    partner = S.nested_partner(L, L)
    letters = S.letters_for(L, L)
    return partner, letters, torch.from_numpy(S.planted_probs(partner)).to(DEV), torch.from_numpy(letters.copy()).to(DEV)


def _host(result):
    """(partner, counts[0..3], ct body, bpseq body) of one device result, cut to the counted bytes."""
    partner, counts, ct, bp = (t.cpu().numpy() for t in result[:4])
    return partner.tolist(), counts[:4].tolist(), ct[:counts[1]].tobytes(), bp[:counts[2]].tobytes()


def _want(partner, letters):
    ct, bp = S.bodies(partner, letters)
    return partner.tolist(), [S.pairs(partner), len(ct), len(bp), 0], ct, bp


@pytest.mark.parametrize("L", (1, 63, 64, 65, 1000, 1024, 1025, 4096))
def test_every_decoder_returns_the_planted_structure_and_its_text(L):
    partner, letters, prob, codes = _inputs(L)
    want = _want(partner, letters)
    decoders = (ops.ss_pairs_long, ops.ss_nested) + ((ops.ss_pairs,) if L <= 1024 else ())
    for decode in decoders:
        assert _host(decode(prob, codes)) == want, decode.__name__


def test_packed_members_of_unlike_length_equal_the_lone_calls():
    Ls = (65, 1, 1024, 64)
    partners, letters, probs, codes = zip(*(_inputs(L) for L in Ls))
    for packed, lone in ((ops.ss_pairs_packed, ops.ss_pairs), (ops.ss_nested_packed, ops.ss_nested)):
        got = packed(list(probs), list(codes))
        for b, L in enumerate(Ls):
            assert _host(got[b]) == _host(lone(probs[b], codes[b])) == _want(partners[b], letters[b]), (packed.__name__, L)
