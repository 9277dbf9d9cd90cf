"""Inputs and expected values for the structure decoding (rnamsm_ss_pairs), shared by the host test of csrc/ss_pairs.h
(test_ss_pairs_host.py) and the GPU test of the kernel (test_gpu_ss_pairs.py).  Expected values come from the host code that
tests/test_ss_post.py pins to the reference -- ss.secondary_structure and ss.write_ss_files called the old way -- and from the
reference-made fixtures; never from the code under test.  Every expectation is computed once per process and cached."""
import functools
import os
import tempfile

import numpy as np

from conftest import GOLDEN
from rnamsm import ss

FIXTURE_CASES = ("multiplets", "threshold", "dense", "helix")


def seq_for(L: int, seed: int = 0) -> str:
    return "".join(np.random.RandomState(1000 + seed).choice(list("ACGUN-"), L, p=[0.22, 0.22, 0.22, 0.22, 0.08, 0.04]))


def fixture(case: str):
    g = np.load(os.path.join(GOLDEN, "ss_post_cases.npz"))
    return g["prob_" + case], str(g["seq_" + case]), g["ct_" + case].tobytes(), g["bpseq_" + case].tobytes()


def shipped_2drb1():
    from rnamsm.msa import read_fasta_records
    (name, seq), = read_fasta_records(os.path.join(GOLDEN, "ss", "2DRB_1.fasta"))
    prob = np.loadtxt(os.path.join(GOLDEN, "ss", "SS_result", "2DRB_1.prob"), delimiter="\t").astype(np.float32)
    return prob, seq


def dense(L: int, value: float = 0.9) -> np.ndarray:
    """Every pair an edge of one value: L - 2 rounds, one surviving pair."""
    return np.full((L, L), value, dtype=np.float32)


def ties(L: int, seed: int = 0) -> np.ndarray:
    """Values drawn from {0.1, 0.6, 0.7, 0.9}: most minima are ties, decided by the partner index."""
    return np.random.RandomState(seed).choice(np.array([0.1, 0.6, 0.7, 0.9], dtype=np.float32), size=(L, L))


def random_sigmoid(L: int, seed: int = 0, shift: float = -1.0) -> np.ndarray:
    z = np.random.RandomState(seed).normal(shift, 3.0, size=(L, L))
    return (1.0 / (1.0 + np.exp(-z))).astype(np.float32)


def sprinkled(L: int, seed: int = 0) -> np.ndarray:
    """NaN, +inf and -inf in a twelfth of the entries each, on both sides of the diagonal; the rest straddles the threshold, the two
    floats next to float32(0.516) included."""
    rng = np.random.RandomState(seed)
    p = random_sigmoid(L, seed + 50, 0.0)
    t = np.float32(0.516)
    near = np.array([t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0))], dtype=np.float32)
    pick = rng.randint(0, 12, size=(L, L))
    p[pick == 0] = np.nan
    p[pick == 1] = np.inf
    p[pick == 2] = -np.inf
    p[pick == 3] = near[rng.randint(0, 3, size=int((pick == 3).sum()))]
    return p


def with_garbage_below(p: np.ndarray, kind: str) -> np.ndarray:
    """The same upper triangle over a lower triangle (and diagonal) the decoding must never read."""
    L = p.shape[0]
    low = {"nan": np.full((L, L), np.nan, dtype=np.float32), "one": np.ones((L, L), dtype=np.float32),
           "transposed": (1.0 - p.T).astype(np.float32)}[kind]
    return np.where(np.triu(np.ones((L, L), dtype=bool), k=1), p, low).astype(np.float32)


def iterative_6x6() -> np.ndarray:
    """The case of tests/test_ss_post.py::test_multiplets_are_resolved_iteratively."""
    p = np.zeros((6, 6), dtype=np.float32)
    p[0, 3], p[0, 4], p[1, 4], p[2, 4] = 0.9, 0.8, 0.7, 0.95
    return p


def helix_noise_1024(seed: int = 7) -> np.ndarray:
    """L = 1024: stacked helices (i, j = c - i) of high probability, sparse noise above the threshold (which crosses helices:
    multiplets), and one planted multiplet that needs two rounds.  Four pairs of probability 1 put partner indices on every
    digit-count boundary (9/10, 99/100, 999/1000, 1024)."""
    L = 1024
    rng = np.random.RandomState(seed)
    p = (0.3 * rng.rand(L, L)).astype(np.float32)
    for lo, hi in ((0, 120), (130, 400), (410, 980)):
        for k in range((hi - lo) // 2 - 3):
            p[lo + k, hi - k] = 0.8 + 0.19 * rng.rand()
    noise = rng.rand(L, L) < 2e-4
    p[noise] = 0.55 + 0.4 * rng.rand(int(noise.sum())).astype(np.float32)
    # planted multiplet: base 300 alone with three partners of unlike value loses one edge per round: two rounds
    for b in (300, 800, 801, 802):
        p[b, :] = 0.1
        p[:, b] = 0.1
    p[300, 800], p[300, 801], p[300, 802] = 0.6, 0.7, 0.8
    p[8, 1023] = 1.0             # partner 1024 on line 9, partner 9 on the last line
    p[9, 999] = 1.0              # partners 1000 and 10
    p[98, 998] = 1.0             # partners 999 and 99
    p[99, 1000] = 1.0            # partners 1001 and 100
    return p


def partner_of_pairs(pairs, L: int) -> np.ndarray:
    partner = np.zeros(L, dtype=np.int32)
    for i, j in pairs:
        partner[i] = j + 1
        partner[j] = i + 1
    return partner


_CACHE = {}


def expected(key: str, prob: np.ndarray, seq: str, name: str = "x"):
    """(pairs, partner, ct body, bpseq body, ct file, bpseq file) of the host path called the old way, once per key."""
    if key not in _CACHE:
        with tempfile.TemporaryDirectory() as tmp:
            pairs = ss.write_ss_files(prob, seq, name, tmp)
            ct = open(os.path.join(tmp, "SS_result", name + ".ct"), "rb").read()
            bp = open(os.path.join(tmp, "SS_result", name + ".bpseq"), "rb").read()
        L = len(seq)
        ct_head, bp_head = f"{L}\t\t{name}\t\tRNAMSM_SS output\n\n".encode(), f"#{name}\n".encode()
        assert ct.startswith(ct_head) and bp.startswith(bp_head)
        assert pairs == ss.secondary_structure(prob)
        _CACHE[key] = (pairs, partner_of_pairs(pairs, L), ct[len(ct_head):], bp[len(bp_head):], ct, bp)
    return _CACHE[key]


@functools.lru_cache(maxsize=None)
def standard_cases():
    """name -> (prob, seq): the matrices both tests decode."""
    cases = {}
    for c in FIXTURE_CASES:
        prob, seq, _, _ = fixture(c)
        cases["fixture_" + c] = (prob, seq)
    cases["2DRB_1"] = shipped_2drb1()
    for L in (2, 3, 65):
        cases[f"dense_{L}"] = (dense(L), seq_for(L, L))
    for L, seed in ((7, 1), (39, 2), (65, 3)):
        cases[f"ties_{L}"] = (ties(L, seed), seq_for(L, seed))
    for L, seed in ((1, 4), (17, 5), (64, 6), (70, 7)):
        cases[f"sprinkled_{L}"] = (sprinkled(L, seed), seq_for(L, seed))
    cases["iterative_6x6"] = (iterative_6x6(), "ACGUAC")
    cases["iterative_6x6_T"] = (iterative_6x6().T.copy(), "ACGUAC")
    return cases
