"""Truths for the covariance contact map (rnamsm_msa_invcov; MSA.invcov, utils/align.py:183-193), in numpy on the CPU.

invcov()       the reference's three lines without scikit-learn: the one-hot over the distinct non-gap values (ascending, a gap all
               zeros), np.cov in float64, the spectral norm of every K x K block by numpy's SVD.
invcov_eigh()  the same covariance, the norm as sqrt(eigvalsh(B^T B).max()): a second fp64 restatement.  Its elementwise distance to
               invcov() is the yardstick the device's Jacobi (a third algorithm of the same conditioning) is held to, times four.
pair_counts()  n_ab(i, j) as integers, from an integer matrix product: the truth of stage 1.
cases()        the shapes the GPU tests run, made once.
"""
import functools

import numpy as np

GAP = 10            # the tokenizer's id of '-'
TILE = 64           # rows (column, symbol) of a tile of the count kernel: 64 / K alignment columns


def symbols(tokens: np.ndarray, gap: int = GAP) -> np.ndarray:
    vals = np.unique(tokens)
    return vals[vals != gap]


def one_hot(tokens: np.ndarray, gap: int = GAP) -> np.ndarray:
    """[N, L, K] float64; K symbols ascending; a gap is all zeros."""
    return (tokens[:, :, None] == symbols(tokens, gap)[None, None, :]).astype(np.float64)


def covariance(tokens: np.ndarray, gap: int = GAP) -> np.ndarray:
    Y = one_hot(tokens, gap)
    N, L, K = Y.shape
    return np.cov(Y.reshape(N, L * K).T, dtype=np.float64).reshape(L, K, L, K)


def invcov(tokens: np.ndarray, gap: int = GAP) -> np.ndarray:
    return np.linalg.norm(covariance(tokens, gap), ord=2, axis=(1, 3))


def invcov_eigh(tokens: np.ndarray, gap: int = GAP) -> np.ndarray:
    B = covariance(tokens, gap).transpose(0, 2, 1, 3)                       # [L, L, K, K]
    G = np.einsum("ijka,ijkb->ijab", B, B)
    return np.sqrt(np.maximum(np.linalg.eigvalsh(G)[..., -1], 0.0))


def pair_counts(tokens: np.ndarray, gap: int = GAP) -> np.ndarray:
    """int32 [L, L, K, K]: rows with symbol a in column i and symbol b in column j."""
    Y = (tokens[:, :, None] == symbols(tokens, gap)[None, None, :]).astype(np.int64)
    N, L, K = Y.shape
    flat = Y.reshape(N, L * K)
    return (flat.T @ flat).reshape(L, K, L, K).transpose(0, 2, 1, 3).astype(np.int32)


def random_alignment(rng, N: int, L: int, K: int, gaps: float = 0.0, alphabet=None) -> np.ndarray:
    """uint8 [N, L] over K symbols (every one of them present), a share `gaps` of the cells the gap."""
    alphabet = np.asarray(alphabet if alphabet is not None else [4, 5, 6, 7, 8, 9] + list(range(20, 30)), dtype=np.uint8)[:K]
    assert len(alphabet) == K and N * L >= K
    t = alphabet[rng.randint(0, K, size=(N, L))]
    if gaps:
        t[rng.rand(N, L) < gaps] = GAP
    t.reshape(-1)[rng.choice(N * L, K, replace=False)] = alphabet
    return t


def mixture_alignment(seed: int = 5, N: int = 5000, L: int = 33) -> np.ndarray:
    """A seeded two-state mixture: every row follows one of two founder sequences (probability 1/2 each) with 10 % of its cells
    redrawn and 5 % gaps, so columns where the founders differ co-vary."""
    rng = np.random.RandomState(seed)
    bases = np.array([4, 5, 6, 7], dtype=np.uint8)
    founders = bases[rng.randint(0, 4, size=(2, L))]
    t = founders[rng.randint(0, 2, size=N)]
    noise = rng.rand(N, L) < 0.10
    t[noise] = bases[rng.randint(0, 4, size=int(noise.sum()))]
    t[rng.rand(N, L) < 0.05] = GAP
    return t


@functools.lru_cache(maxsize=None)
def cases():
    """name -> uint8 [N, L] tokens.  N at the edges of the 64-row words; L at the edges of the count kernel's tile of 64 / K columns
    (and the flat (column, symbol) count L * K at 63, 64, 65 and beyond one tile); K in {1, 2, 4, 5, 16}; with and without gaps; an
    all-gap column, an all-gap row, a constant column."""
    rng = np.random.RandomState(20240)
    out = {}
    for N in (2, 3, 63, 64, 65, 128, 129):
        out[f"N{N}_L7_K4"] = random_alignment(rng, N, 7, min(4, N * 7), gaps=0.2 if N > 3 else 0.0)
    for K in (1, 2, 4, 5, 16):
        tile = TILE // K                                                       # K = 5: 12 columns and 4 rows of a 13th
        for L in sorted({1, 2, tile - 1, tile, tile + 1, 2 * tile + 1} - {0}):
            if 70 * L >= K:
                out[f"N70_L{L}_K{K}"] = random_alignment(rng, 70, L, K, gaps=0.0 if L % 2 else 0.15)
    t = random_alignment(rng, 66, 19, 4, gaps=0.1)
    t[:, 3] = GAP                   # an all-gap column
    t[5, :] = GAP                   # an all-gap row
    out["N66_L19_K4_degenerate"] = t
    t = random_alignment(rng, 66, 19, 4, gaps=0.1)
    t[:, 11] = 6                    # a constant column: every block with it has rank 0
    out["N66_L19_K4_constant"] = t
    for v in out.values():
        v.setflags(write=False)
    return out


def yardstick(names=None) -> float:
    """The largest elementwise distance between the two fp64 restatements over the cases, relative to each map's largest entry."""
    worst = 0.0
    for name, t in cases().items():
        if names is None or name in names:
            a, b = invcov(t), invcov_eigh(t)
            worst = max(worst, float(np.abs(a - b).max() / a.max()) if a.max() > 0 else 0.0)
    return worst
