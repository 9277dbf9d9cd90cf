"""The summation model the sub-sampling kernels rest on (csrc/greedy_select.hip, f3), on the host.

rnamsm_greedy_select has to repeat numpy's pairwise summation of every candidate's distance history term for term: the
terms m / L are inexact, candidates tie in their mismatch totals, and the order of the additions decides who wins.  This
module writes that order down in plain Python, holds it bit-equal to np.add.reduce for every history length the entry
point accepts (num_seqs <= 2048, so up to 2047 terms), and asserts the structural facts the kernels are built on:
recursion depth <= 5 (greedy_combine<5>, pairwise_sum<5>), <= 32 leaves (the fused kernel's s_off / s_len / s_leaf
slots) of <= 128 terms each.  It also models a recursion cut off after four levels -- the per-thread kernel's order
before it was given five -- which is what tests/test_gpu_subsampling.py chooses its critical num_seqs values with.
"""
import numpy as np
import pytest

MAX_TERMS = 2047                 # num_seqs <= 2048 (include/rnamsm.h, f3): a history of at most 2047 steps


def leaf_sum(a, lo, n):
    """numpy's unrolled leaf (n <= 128): below 8 terms sequential from 0; else eight interleaved accumulators,
    combined as a balanced tree, and the n % 8 trailing terms one after the other."""
    if n < 8:
        res = 0.0
        for i in range(lo, lo + n):
            res += a[i]
        return res
    r = [a[lo + j] for j in range(8)]
    full = n - n % 8
    for i in range(lo + 8, lo + full, 8):
        for j in range(8):
            r[j] += a[i + j]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for i in range(lo + full, lo + n):
        res += a[i]
    return res


def leaves(n, levels=None):
    """(offset, length, depth) of the leaves of numpy's recursion over n terms, left to right.  `levels`: a recursion
    that stops splitting after that many levels, whatever is left (None = numpy's own)."""
    out = []

    def walk(lo, n, depth):
        if n <= 128 or (levels is not None and depth == levels):
            out.append((lo, n, depth))
            return
        n2 = n // 2
        n2 -= n2 % 8
        walk(lo, n2, depth + 1)
        walk(lo + n2, n - n2, depth + 1)

    walk(0, n, 0)
    return out


def pairwise_sum(a, lo=0, n=None, levels=None, depth=0):
    """numpy's DOUBLE_pairwise_sum over a[lo : lo + n] (Python floats are IEEE doubles); `levels` as in leaves()."""
    n = len(a) - lo if n is None else n
    if n <= 128 or (levels is not None and depth == levels):
        return leaf_sum(a, lo, n)
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_sum(a, lo, n2, levels, depth + 1) + pairwise_sum(a, lo + n2, n - n2, levels, depth + 1)


@pytest.mark.parametrize("L", [7, 35])
def test_transcription_equals_numpy_for_every_history_length(L):
    """Bit-equal to np.add.reduce on contiguous float64 for every n in 1..2047, on terms m / L (what cdist 'hamming' gives)."""
    rng = np.random.RandomState(L)
    a = rng.randint(0, L + 1, size=MAX_TERMS).astype(np.float64) / L
    terms = a.tolist()
    for n in range(1, MAX_TERMS + 1):
        want = np.add.reduce(a[:n])
        got = pairwise_sum(terms, 0, n)
        assert got == want and np.float64(got).tobytes() == want.tobytes(), n
    # and along the contiguous axis of a [candidate, step] matrix, as the host path and the reference reduce it
    h = rng.randint(0, L + 1, size=(5, MAX_TERMS)).astype(np.float64) / L
    for n in (7, 8, 128, 129, 1023, 1929, 2047):
        want = h[[0, 2, 4], :n].sum(1)
        assert [pairwise_sum(h[c].tolist(), 0, n) for c in (0, 2, 4)] == want.tolist(), n


def test_order_depends_on_the_grouping_at_all():
    """The check above would be empty if any order gave the same bits: a running sum differs from numpy's on such terms."""
    a = np.random.RandomState(1).randint(0, 36, size=MAX_TERMS).astype(np.float64) / 35
    run, diff = 0.0, 0
    for n, t in enumerate(a.tolist(), 1):
        run += t
        diff += run != np.add.reduce(a[:n])
    assert diff > MAX_TERMS // 10


def test_structure_the_kernels_rest_on():
    """n <= 2047: at most five levels of splitting, at most 32 leaves (17 in fact), every leaf within numpy's unrolled
    loop; the leaves tile [0, n) in order.  2047 -> 1031 -> 519 -> 263 -> 135 -> 64 + 71 is the deepest path."""
    max_depth = max_leaves = 0
    for n in range(1, MAX_TERMS + 1):
        lv = leaves(n)
        pos = 0
        for lo, ln, depth in lv:
            assert lo == pos and 0 < ln <= 128, (n, lo, ln)
            pos += ln
            max_depth = max(max_depth, depth)
        assert pos == n
        max_leaves = max(max_leaves, len(lv))
    assert max_depth == 5
    assert max_leaves == 17 <= 32
    assert [ln for _, ln, _ in leaves(2047)][-2:] == [64, 71]
    assert [(lo, ln) for lo, ln, _ in leaves(135)] == [(0, 64), (64, 71)]


def test_four_levels_are_one_too_few():
    """A recursion cut off after four levels sums a piece of more than 128 terms as ONE leaf where numpy splits it.  That
    happens first at 1929 terms (1929 -> 969 -> 489 -> 249 -> 129) and for 105 of the lengths in [1929, 2047]; five
    levels leave no length up to 2047 with such a piece.  On terms m / 35 the two orders then give different bits for a
    few per cent of random histories."""
    bad4 = [n for n in range(1, MAX_TERMS + 1) if leaves(n, 4) != leaves(n)]
    assert bad4[0] == 1929 and len(bad4) == 105
    assert all(leaves(n, 5) == leaves(n) for n in range(1, MAX_TERMS + 1))
    rng = np.random.RandomState(2)
    trials = 400
    differ = 0
    for _ in range(trials):
        a = (rng.randint(0, 36, size=MAX_TERMS).astype(np.float64) / 35).tolist()
        differ += pairwise_sum(a, 0, MAX_TERMS, levels=4) != pairwise_sum(a, 0, MAX_TERMS)
    assert 0 < differ < trials, differ
