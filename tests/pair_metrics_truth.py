"""The two rules of rnamsm_pair_sweep_* and rnamsm_pair_precision_* (include/rnamsm.h) on the CPU, each stated twice.
tests/test_pair_metrics_host.py holds the two forms of each against each other and against the reference's recorded results
(tests/golden/pair_metrics_reference.npz); the GPU tests compare the device's integers with them.

sweep      candidates: i < j, j - i >= min_sep, neither i nor j skipped; positive iff target != 0; tp[t] / fp[t] = the positives /
           negatives with value >= thresholds[t] (NaN reaches none); fn = P - tp, tn = N - fp.  int64 [4, T]: tp, fp, tn, fn.
  sweep_broadcast  the reference's statement: np.greater_equal(values[n, 1], T[1, T]) and four sums over n (small maps only)
  sweep_hist       np.searchsorted + np.bincount + one suffix sum: any size
precision  candidates: i < j, j - i >= min_sep, j - i < max_sep when max_sep > 0, target >= 0, value not NaN; ranked as top_pairs ranks;
           n = min(k, candidates); hits[c] = the pairs with target > 0 among the first min(cuts[c], n).
  precision_ranked  on top_pairs_truth's order (NaN written at the excluded pairs)
  precision_loop    a Python loop and Python's sort (L <= 17)"""
import numpy as np

import top_pairs_truth as TP


def _candidates(x, target, min_sep, skip):
    L = x.shape[0]
    i, j = np.triu_indices(L, k=int(min_sep))
    if skip is not None:
        s = np.asarray(skip).astype(bool)
        keep = ~s[i] & ~s[j]
        i, j = i[keep], j[keep]
    return x[i, j].astype(np.float64), target[i, j] != 0


def sweep_broadcast(x, target, thresholds, min_sep=1, skip=None):
    v, pos = _candidates(x[:, :x.shape[0]], target[:, :x.shape[0]], min_sep, skip)
    T = np.asarray(thresholds, dtype=np.float64)[None, :]
    with np.errstate(invalid="ignore"):
        out = np.greater_equal(v[:, None], T)
    t = pos[:, None]
    tp = np.sum(np.logical_and(out, t), axis=0)
    tn = np.sum(np.logical_and(np.logical_not(out), np.logical_not(t)), axis=0)
    fp = np.sum(np.logical_and(out, np.logical_not(t)), axis=0)
    fn = np.sum(np.logical_and(np.logical_not(out), t), axis=0)
    return np.stack([tp, fp, tn, fn]).astype(np.int64)


def sweep_hist(x, target, thresholds, min_sep=1, skip=None):
    L = x.shape[0]
    v, pos = _candidates(x[:, :L], target[:, :L], min_sep, skip)
    th = np.asarray(thresholds, dtype=np.float64)
    T = len(th)
    bins = np.searchsorted(th, v, side="right")            # the thresholds <= v; NaN sorts past the end:
    bins[np.isnan(v)] = 0                                   # it reaches none
    out = []
    for sel in (pos, ~pos):
        h = np.bincount(bins[sel], minlength=T + 1).astype(np.int64)
        out.append(h.sum() - np.cumsum(h)[:T])             # the candidates whose bin is above t
    tp, fp = out
    return np.stack([tp, fp, (~pos).sum() - fp, pos.sum() - tp]).astype(np.int64)


def _masked(x, target, min_sep, max_sep):
    L = x.shape[0]
    m = np.array(x[:, :L], dtype=x.dtype, copy=True)
    sep = np.arange(L)[None, :] - np.arange(L)[:, None]
    bad = target[:, :L] < 0
    if max_sep > 0:
        bad = bad | (sep >= max_sep)
    m[bad] = np.nan
    return m


def precision_ranked(x, target, k, cuts, min_sep, max_sep=0):
    """-> (hits int32 [ncuts], n, pairs int64 [n, 2], scores float64 [n])"""
    pairs, scores = TP.truth(_masked(x, target, min_sep, max_sep), k, min_sep)
    n = len(scores)
    hit = target[pairs[:, 0], pairs[:, 1]] > 0
    run = np.concatenate([[0], np.cumsum(hit)])
    hits = np.array([run[min(int(c), n)] for c in cuts], dtype=np.int32)
    return hits, n, pairs, scores


def precision_loop(x, target, k, cuts, min_sep, max_sep=0):
    L = x.shape[0]
    assert L <= 17
    cands = []
    for i in range(L):
        for j in range(i + 1, L):
            v = float(x[i, j])
            if j - i >= min_sep and (max_sep <= 0 or j - i < max_sep) and target[i, j] >= 0 and v == v:
                cands.append((-v, i, j))
    cands.sort()
    cands = cands[:k]
    n = len(cands)
    hits = np.array([sum(1 for _, i, j in cands[:min(int(c), n)] if target[i, j] > 0) for c in cuts], dtype=np.int32)
    pairs = np.array([(i, j) for _, i, j in cands], dtype=np.int64).reshape(-1, 2)
    scores = np.array([0.0 if nv == 0 else -nv for nv, _, _ in cands], dtype=np.float64)
    return hits, n, pairs, scores
