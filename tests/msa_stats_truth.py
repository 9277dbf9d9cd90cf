"""The numpy restatement of the reference's alignment statistics (utils/align.py: MSA.pdist :121-126, MSA.weights :250-253, MSA.neff
:259-269, coverage :242-247) that the device kernels of csrc/msa_pdist.hip are held to, and the alignments the tests run on.  Every
quantity is exact: integer counts and one IEEE division each, so the tests compare bits.  tests/test_msa_stats_host.py ties the
restatement to the reference's own MSA class (tests/golden/msa_stats_reference_2drb64.npz) and to scipy."""
import numpy as np

GAP = 10                        # the tokenizer's id of '-'
TOKENS = (4, 5, 6, 7, GAP)      # A G C U -


def counts(a: np.ndarray) -> np.ndarray:
    """m(i, j): the columns in which rows i and j differ, int32 [N, N]."""
    a = np.asarray(a)
    out = np.empty((a.shape[0], a.shape[0]), dtype=np.int32)
    step = max(1, (1 << 24) // max(1, a.shape[0] * a.shape[1]))
    for i0 in range(0, a.shape[0], step):
        out[i0:i0 + step] = (a[i0:i0 + step, None] != a[None]).sum(-1)
    return out


def dist(a: np.ndarray) -> np.ndarray:
    return counts(a) / np.float64(a.shape[1])


def n_neighbors(a: np.ndarray, cutoff: float) -> np.ndarray:
    return (dist(a) < cutoff).sum(1).astype(np.int32)


def weights(a: np.ndarray, cutoff: float) -> np.ndarray:
    with np.errstate(divide="ignore"):
        return 1 / (dist(a) < cutoff).sum(1)


def coverage(a: np.ndarray, gap: int = GAP) -> np.ndarray:
    return (np.asarray(a) != gap).mean(0)


def alignment(N: int, L: int, seed: int) -> np.ndarray:
    """uint8 [N, L] over the five tokens, drawn around three founders with a per-row mutation rate between 0 and 0.6: near and far
    pairs both occur, so every cutoff in (0, 1) splits the pairs; every ninth row repeats an earlier one."""
    rng = np.random.RandomState(seed)
    founders = rng.choice(TOKENS, size=(3, L))
    a = founders[rng.randint(0, 3, size=N)]
    rate = rng.rand(N, 1) * 0.6
    flip = rng.rand(N, L) < rate
    a[flip] = rng.choice(TOKENS, size=int(flip.sum()))
    for i in range(9, N, 9):
        a[i] = a[i // 2]
    return np.ascontiguousarray(a.astype(np.uint8))


# every N of {1, 2, 63, 64, 65, 129, 200} (a lone row, tile seams, a ragged last tile, more than one tile each way) and every L of
# {1, 7, 8, 9, 63, 64, 65, 513} (word seams, the masked tail, more than one staged step) at least twice
SHAPES = [(1, 1), (1, 64), (2, 7), (2, 513), (63, 8), (63, 65), (64, 9), (64, 63), (65, 1), (65, 64), (129, 7), (129, 513), (200, 8),
          (200, 9), (200, 63), (200, 65), (65, 7), (65, 63), (65, 65)]
