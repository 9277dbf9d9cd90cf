"""Inputs for the long structure decoding (rnamsm_ss_pairs_long, L up to 4096), shared by the host test of csrc/ss_pairs_long.h
(test_long_heads_host.py) and the GPU test of the kernel (test_gpu_ss_pairs_long.py).  Expected values come from ss_pairs_cases.expected
-- the host function and writer -- never from the code under test.  The host function is quadratic in the number of edges per round,
so beyond L = 1024 the matrices are sparse: ss_pairs_cases' dense / ties / sprinkled generators fill BLOCKS that straddle the thread
boundaries of the long kernel (one base per thread ends at 1024; thread t owns bases [t * per, (t + 1) * per)), or are thinned to
about one edge per base."""
import functools

import numpy as np

import ss_pairs_cases as C

THRESHOLD = np.float32(0.516)


def edges_above(p: np.ndarray) -> int:
    return int((p[np.triu_indices(p.shape[0], k=1)] > THRESHOLD).sum())


def helix_noise(L: int, seed: int = 7) -> np.ndarray:
    """ss_pairs_cases.helix_noise_1024 at any L >= 1025: stacked helices, sparse noise above the threshold that crosses them, one
    planted multiplet that needs two rounds, and pairs of probability 1 that put 999 / 1000 into the partner column and onto lines
    999 / 1000, and L itself into the partner column."""
    rng = np.random.RandomState(seed)
    p = (0.3 * rng.rand(L, L)).astype(np.float32)
    for lo, hi in ((0, 120), (130, 400), (410, 980), (1030, L - 2)):
        for k in range((hi - lo) // 2 - 3):
            p[lo + k, hi - k] = 0.8 + 0.19 * rng.rand()
    noise = rng.rand(L, L) < 0.2 / L
    p[noise] = 0.55 + 0.4 * rng.rand(int(noise.sum())).astype(np.float32)
    for b in (300, 800, 801, 802, 8, 998, 999, 1024, L - 1):
        p[b, :] = 0.1
        p[:, b] = 0.1
    p[300, 800], p[300, 801], p[300, 802] = 0.6, 0.7, 0.8          # two rounds
    p[8, L - 1] = 1.0                # partner L on line 9
    p[998, 1024] = 1.0               # line 999 with partner 1025; partner 999 on line 1025 (the first base beyond one per thread)
    p[800, 999] = 0.9                # line 1000 / partner 1000 (800 keeps it once 300 has let go of it)
    return p


def blocks(L: int, seed: int = 0) -> np.ndarray:
    """Zeros with a `dense` block on the last 24 bases (22 rounds, across the last threads' runs), a `ties` block of 48 bases from
    1000 on where L allows (across base 1024) and a `sprinkled` block (NaN, +-inf, the floats next to the threshold) on the first 40."""
    p = np.zeros((L, L), dtype=np.float32)
    n = min(L, 40)
    p[:n, :n] = C.sprinkled(n, seed + 3)
    if L >= 1100:
        p[1000:1048, 1000:1048] = C.ties(48, seed + 1)
    if L >= 64:
        p[L - 24:, L - 24:] = C.dense(24)
    return p


def thin_sprinkled(L: int, seed: int = 0) -> np.ndarray:
    """ss_pairs_cases.sprinkled thinned to about two candidate entries per row (the rest NaN, -inf or 0.1 by turns: never an edge),
    generated row block by row block so that L = 4096 stays cheap."""
    rng = np.random.RandomState(seed)
    t = THRESHOLD
    near = np.array([t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0)), np.inf, 0.9, 0.7, 0.6], dtype=np.float32)
    p = np.array([np.nan, -np.inf, 0.1], dtype=np.float32)[rng.randint(0, 3, size=(L, L))]
    n = 2 * L
    p[rng.randint(0, L, n), rng.randint(0, L, n)] = near[rng.randint(0, len(near), n)]
    return p


@functools.lru_cache(maxsize=None)
def expected_without_prob(kind: str, L: int):
    """ss_pairs_cases.expected's (pairs, partner, ct body, bpseq body) for case(kind, L) from the same host function and the same
    table writer, without the `.prob` text write_ss_files formats beside them (16.7 M numbers at L = 4096)."""
    import os
    import tempfile
    from rnamsm import ss
    _, prob, seq = case(kind, L)
    pairs = ss.secondary_structure(prob)
    partner = C.partner_of_pairs(pairs, L)
    with tempfile.TemporaryDirectory() as tmp:
        ss._tables_on_host(tmp, "x", seq, partner.astype(int))
        ct, bp = (open(os.path.join(tmp, "x" + ext), "rb").read() for ext in (".ct", ".bpseq"))
    ct_head, bp_head = f"{L}\t\tx\t\tRNAMSM_SS output\n\n".encode(), b"#x\n"
    assert ct.startswith(ct_head) and bp.startswith(bp_head)
    return pairs, partner, ct[len(ct_head):], bp[len(bp_head):]


@functools.lru_cache(maxsize=None)
def case(kind: str, L: int):
    """-> (key, prob, seq); the key names the ss_pairs_cases.expected cache entry."""
    prob = {"helix": helix_noise, "blocks": blocks, "thin": thin_sprinkled}[kind](L)
    return f"long_{kind}_{L}", prob, C.seq_for(L, L % 97)
