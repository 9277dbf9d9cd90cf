"""Truths for the sequence-weighted mutual information (rnamsm_msa_wmi), in fp64 on the CPU, built on tests/mi_truth.py and
tests/invcov_truth.py.

states()            [N, L] index of every cell's state: the symbol's rank, and for a gap K ("state") or -1 ("pairwise": in no entry).
tables_fsum()       c[i, j, a, b] = math.fsum of the weights of the rows with state a in column i and b in column j: the exactly
                    rounded sum, float64 [L, L, S, S].
tables_ascending()  the same sums taken one row after the other, ascending, in float64 (np.bincount's loop): a second legitimate
                    fp64 evaluation.
mi_of_tables()      the device's formula in numpy: s_b, r_a, n by ascending loops, then the sum over a then b ascending, the entries
                    with c > 0 only, of (c / n) * log((c * n) / (r_a * s_b)).
weights_cpu()       MSA.weights in numpy: 1 / rows within the normalised Hamming cutoff (the strict comparison of the reference).
yardstick()         the largest elementwise distance, relative to each map's largest |entry|, between the two evaluations over the
                    weighted alignments(): for mi the formula on tables_fsum against the formula on tables_ascending; for mip,
                    apc_numpy of the first against apc_fsum of the second (mi with a zero diagonal), so the correction's order of
                    summation varies too.  The device is a third evaluation (another order again) and is held to four times that,
                    against the tables_fsum truth -- the rule and the margin of tests/test_gpu_mi.py.
"""
import functools
import math

import numpy as np

import invcov_truth as T
import mi_truth as M
from conftest import golden

MODES = M.MODES


def states(tokens: np.ndarray, mode: str, gap: int = T.GAP) -> np.ndarray:
    sym = T.symbols(tokens, gap)
    idx = np.full(tokens.shape, len(sym) if mode == "state" else -1, dtype=np.int64)
    for a, v in enumerate(sym):
        idx[tokens == v] = a
    assert mode in MODES
    return idx


def n_states(tokens: np.ndarray, mode: str, gap: int = T.GAP) -> int:
    return len(T.symbols(tokens, gap)) + (mode == "state")


def _tables(tokens, weights, mode, gap, entry_sums) -> np.ndarray:
    """entry_sums(codes [n], w [n], S * S) -> float64 [S * S]: the sum of w per code."""
    idx, S = states(tokens, mode, gap), n_states(tokens, mode, gap)
    w = np.asarray(weights, dtype=np.float64)
    N, L = tokens.shape
    assert w.shape == (N,)
    out = np.zeros((L, L, S, S))
    for i in range(L):
        for j in range(i, L):
            live = (idx[:, i] >= 0) & (idx[:, j] >= 0)
            block = entry_sums(idx[live, i] * S + idx[live, j], w[live], S * S).reshape(S, S)
            out[i, j] = block
            out[j, i] = block.T
    return out


def _fsum_per_code(codes, w, n):
    order = np.argsort(codes, kind="stable")
    codes, w = codes[order], w[order]
    edges = np.searchsorted(codes, np.arange(n + 1))
    return np.array([math.fsum(w[edges[c]:edges[c + 1]]) for c in range(n)])


def tables_fsum(tokens: np.ndarray, weights: np.ndarray, mode: str, gap: int = T.GAP) -> np.ndarray:
    return _tables(tokens, weights, mode, gap, _fsum_per_code)


def tables_ascending(tokens: np.ndarray, weights: np.ndarray, mode: str, gap: int = T.GAP) -> np.ndarray:
    return _tables(tokens, weights, mode, gap, lambda codes, w, n: np.bincount(codes, weights=w, minlength=n))


def profile_fsum(tokens: np.ndarray, weights: np.ndarray, mode: str, gap: int = T.GAP) -> np.ndarray:
    """float64 [L, S]: the exactly rounded weight of every state of every column (wmarg)."""
    idx, S = states(tokens, mode, gap), n_states(tokens, mode, gap)
    w = np.asarray(weights, dtype=np.float64)
    return np.array([[math.fsum(w[idx[:, i] == a]) for a in range(S)] for i in range(tokens.shape[1])]).reshape(tokens.shape[1], S)


def mi_of_tables(c: np.ndarray) -> np.ndarray:
    c = np.asarray(c, dtype=np.float64)
    L, _, S, _ = c.shape
    s = np.zeros((L, L, S))
    r = np.zeros((L, L, S))
    n = np.zeros((L, L))
    for a in range(S):
        s = s + c[:, :, a, :]                                                      # s_b: a ascending
    for b in range(S):
        r = r + c[:, :, :, b]                                                      # r_a: b ascending
        n = n + s[:, :, b]
    out = np.zeros((L, L))
    with np.errstate(all="ignore"):
        for a in range(S):
            for b in range(S):
                cab = c[:, :, a, b]
                live = (cab > 0) & (n > 0)
                ratio = np.divide(cab * n, r[:, :, a] * s[:, :, b], out=np.ones((L, L)), where=live)
                weight = np.divide(cab, n, out=np.zeros((L, L)), where=live)
                out = out + np.where(live, weight * np.log(ratio), 0.0)
    return out


def mip_of(mi: np.ndarray, apc=M.apc_numpy) -> np.ndarray:
    return apc(M.zero_diagonal(mi))


def weights_cpu(tokens: np.ndarray, seqid_cutoff: float = 0.2) -> np.ndarray:
    N, L = tokens.shape
    counts = np.zeros(N, dtype=np.int64)
    step = max(1, (1 << 24) // (N * L))
    for i0 in range(0, N, step):
        mismatches = (tokens[i0:i0 + step, None, :] != tokens[None, :, :]).sum(-1)
        counts[i0:i0 + step] = (mismatches.astype(np.float64) / np.float64(L) < seqid_cutoff).sum(1)
    return 1.0 / counts


def alignments():
    """name -> tokens uint8 [N, L]: invcov_truth's mixture and the shipped 64-row excerpt of 2DRB_1 (no <cls>)."""
    return {"mixture_N5000_L33": T.mixture_alignment(),
            "2DRB_1_first64": np.ascontiguousarray(golden("tokens_2DRB_1_first64.npz")["tokens"][:, 1:].astype(np.uint8))}


@functools.lru_cache(maxsize=None)
def real_weights(name: str) -> np.ndarray:
    w = weights_cpu(alignments()[name], 0.2)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def truth_tables(name: str, mode: str) -> np.ndarray:
    out = tables_fsum(alignments()[name], real_weights(name), mode)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def truth(name: str, mode: str):
    """(mi, mip) from the exactly rounded tables, made once."""
    mi = mi_of_tables(truth_tables(name, mode))
    mip = mip_of(mi)
    mi.setflags(write=False)
    mip.setflags(write=False)
    return mi, mip


def _relative(a: np.ndarray, b: np.ndarray) -> float:
    top = float(np.abs(a).max())
    return float(np.abs(a - b).max() / top) if top > 0 and np.isfinite(top) else 0.0


@functools.lru_cache(maxsize=None)
def yardstick(mode: str):
    """(yardstick_mi, yardstick_mip) over alignments() with their real weights."""
    y_mi = y_mip = 0.0
    for name, t in alignments().items():
        mi, mip = truth(name, mode)
        other = mi_of_tables(tables_ascending(t, real_weights(name), mode))
        y_mi = max(y_mi, _relative(mi, other))
        y_mip = max(y_mip, _relative(mip, mip_of(other, M.apc_fsum)))
    return y_mi, y_mip
