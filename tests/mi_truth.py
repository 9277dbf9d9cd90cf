"""Truths for the mutual-information contacts (rnamsm_msa_mi, rnamsm_apc_f64), in numpy fp64 on the CPU, built on tests/invcov_truth.py.

tables()         the integer table c[a][b] of every pair of columns, [L, L, S, S]: mode "pairwise" over the K symbols (rows with a gap
                 in either column left out), mode "state" with the gap as state K (S = K + 1), from the integer pair counts.
mi_ratio()       the definition: sum over c > 0 of (c / n) * log((c * n) / (r_a * s_b)), a-major then b.
mi_entropy()     H_i + H_j - H_ij from the same tables: a second fp64 restatement.
apc_numpy()      the reference's apc (utils/tensor.py:103-113), line by line.
apc_fsum()       the same with the row, column and total sums by math.fsum (correctly rounded sums).
yardstick_mi()   the largest elementwise distance between the two MI restatements over the cases and the mixture, relative to each
                 map's largest entry; yardstick_apc() the same between apc_numpy and apc_fsum on mi0 (mi_ratio with a zero diagonal).
The device is a third evaluation of the same conditioning and is held to four times the yardstick, against the truth.
"""
import functools
import math

import numpy as np

import invcov_truth as T

MODES = ("pairwise", "state")


def tables_from_counts(counts: np.ndarray, N: int, mode: str, marg_i=None, marg_j=None) -> np.ndarray:
    """int64 [Li, Lj, S, S] from n_ab(i, j) as [Li, Lj, K, K] (any integer or exact float dtype).  marg_i [Li, K], marg_j [Lj, K]: the
    marginals n_a of the columns i and j; absent, the counts are every pair of the alignment's columns and n_a(i) = n_aa(i, i)."""
    c = np.asarray(counts).astype(np.int64)
    if mode == "pairwise":
        return c
    assert mode == "state", mode
    Li, Lj, K, _ = c.shape
    if marg_i is None:
        marg_i = marg_j = c[np.arange(Li), np.arange(Li)][:, np.arange(K), np.arange(K)]
    out = np.zeros((Li, Lj, K + 1, K + 1), dtype=np.int64)
    out[:, :, :K, :K] = c
    out[:, :, :K, K] = np.asarray(marg_i, dtype=np.int64)[:, None, :] - c.sum(3)
    out[:, :, K, :K] = np.asarray(marg_j, dtype=np.int64)[None, :, :] - c.sum(2)
    out[:, :, K, K] = N - out.sum((2, 3))
    assert out.min() >= 0
    return out


def tables(tokens: np.ndarray, mode: str, gap: int = T.GAP) -> np.ndarray:
    return tables_from_counts(T.pair_counts(tokens, gap), tokens.shape[0], mode)


def mi_ratio_of(c: np.ndarray) -> np.ndarray:
    n = c.sum((2, 3))
    r, s = c.sum(3), c.sum(2)
    num = c * n[:, :, None, None]                                                   # exact integers below 2^40
    den = r[:, :, :, None] * s[:, :, None, :]
    live = c > 0
    ratio = np.divide(num.astype(np.float64), den.astype(np.float64), out=np.ones(c.shape), where=live)
    weight = np.divide(c.astype(np.float64), n[:, :, None, None].astype(np.float64), out=np.zeros(c.shape), where=live)
    terms = weight * np.log(ratio)
    out = np.zeros(n.shape)
    for a in range(c.shape[2]):                                                     # a-major then b, ascending; a term of c = 0 is +0.0
        for b in range(c.shape[3]):
            out = out + terms[:, :, a, b]
    return out


def mi_ratio(tokens: np.ndarray, mode: str, gap: int = T.GAP) -> np.ndarray:
    return mi_ratio_of(tables(tokens, mode, gap))


def _entropy(counts: np.ndarray, n: np.ndarray) -> np.ndarray:
    """-sum p log p over the last axis, p = counts / n; 0 where n = 0."""
    p = np.divide(counts.astype(np.float64), n[..., None].astype(np.float64), out=np.zeros(counts.shape), where=n[..., None] > 0)
    return -(p * np.log(np.where(p > 0, p, 1.0))).sum(-1)


def mi_entropy_of(c: np.ndarray) -> np.ndarray:
    L = c.shape[0]
    n = c.sum((2, 3))
    return _entropy(c.sum(3), n) + _entropy(c.sum(2), n) - _entropy(c.reshape(L, L, -1), n)


def mi_entropy(tokens: np.ndarray, mode: str, gap: int = T.GAP) -> np.ndarray:
    return mi_entropy_of(tables(tokens, mode, gap))


def zero_diagonal(x: np.ndarray) -> np.ndarray:
    out = np.array(x, dtype=np.float64)
    np.fill_diagonal(out, 0.0)
    return out


def apc_numpy(x: np.ndarray) -> np.ndarray:
    a1 = x.sum(-1, keepdims=True)
    a2 = x.sum(-2, keepdims=True)
    a12 = x.sum((-1, -2), keepdims=True)
    avg = a1 * a2
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = avg / a12
    return x - avg


def apc_fsum(x: np.ndarray) -> np.ndarray:
    a1 = np.array([math.fsum(row) for row in x])[:, None]
    a2 = np.array([math.fsum(col) for col in x.T])[None, :]
    a12 = math.fsum(x.reshape(-1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return x - (a1 * a2) / np.float64(a12)


def alignments():
    """name -> tokens: invcov_truth's cases and its mixture, the alignments the yardsticks run over."""
    out = dict(T.cases())
    out["mixture_N5000_L33"] = T.mixture_alignment()
    return out


def _relative(a: np.ndarray, b: np.ndarray) -> float:
    top = float(np.abs(a).max())
    return float(np.abs(a - b).max() / top) if top > 0 and np.isfinite(top) else 0.0


@functools.lru_cache(maxsize=None)
def truth(name: str, mode: str) -> np.ndarray:
    """mi_ratio of a named alignment, made once."""
    out = mi_ratio(alignments()[name], mode)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def yardstick_mi(mode: str) -> float:
    return max(_relative(truth(name, mode), mi_entropy(t, mode)) for name, t in alignments().items())


@functools.lru_cache(maxsize=None)
def yardstick_apc(mode: str) -> float:
    worst = 0.0
    for name in alignments():
        mi0 = zero_diagonal(truth(name, mode))
        if mi0.sum() > 0:                                                           # (a total of 0: NaN both ways)
            worst = max(worst, _relative(apc_numpy(mi0), apc_fsum(mi0)))
    return worst
