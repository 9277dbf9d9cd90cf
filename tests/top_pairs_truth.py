"""The rule of rnamsm_top_pairs_f64 / _f32 (include/rnamsm.h) stated twice on the CPU: in numpy -- mask, canonicalise the zero, one
np.lexsort on the integer key, so that +-inf and ties are exact -- and as a plain Python loop with a float sort key for small maps.
tests/test_top_pairs_host.py holds the two against each other; the GPU tests compare the device's bytes with the first.

Candidates: (i, j), 0 <= i < j < L, j - i >= min_sep, x[i, j] not NaN.  Value v = float64(x[i, j]); -0.0 counts as +0.0.  Order: larger
v first, then smaller i, then smaller j.  A zero is reported as +0.0."""
import numpy as np

SIGN = np.uint64(1) << np.uint64(63)


def key_of(v: np.ndarray) -> np.ndarray:
    """float64 values (no NaN) -> uint64 keys, strictly monotone in the value, both zeros on one key."""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64).copy()
    b[(b << np.uint64(1)) == 0] = 0
    return np.where((b & SIGN) != 0, ~b, b | SIGN)


def ranked(x: np.ndarray, min_sep: int):
    """Every candidate of x ([L, ld >= L], float32 or float64) in the rule's order -> (pairs int64 [M, 2], scores float64 [M])."""
    L = x.shape[0]
    i, j = np.triu_indices(L, k=int(min_sep))                 # j - i >= min_sep; nothing at all for min_sep >= L
    v = x[i, j].astype(np.float64)
    keep = ~np.isnan(v)
    i, j, v = i[keep], j[keep], v[keep]
    order = np.lexsort((j, i, ~key_of(v)))                    # the last key is the primary one: descending key, then i, then j
    return np.stack([i[order], j[order]], axis=1).astype(np.int64), v[order] + 0.0        # (-0.0 + 0.0 is +0.0)


def truth(x: np.ndarray, k: int, min_sep: int):
    pairs, scores = ranked(x, min_sep)
    return pairs[:k], scores[:k]


def padded(pairs: np.ndarray, scores: np.ndarray, k: int):
    """A ranked list (at least min(k, M) rows of it) as the device writes it: (pairs int32 [k, 2], scores float64 [k], count), the rows
    from count on -1, -1 and NaN."""
    n = min(k, len(scores))
    out_p = np.full((k, 2), -1, dtype=np.int32)
    out_s = np.full(k, np.nan, dtype=np.float64)
    out_p[:n], out_s[:n] = pairs[:n], scores[:n]
    return out_p, out_s, n


def truth_loop(x: np.ndarray, k: int, min_sep: int):
    """The same rule as a loop and Python's sort on floats (-0.0 == 0.0 and the infinities compare as the rule says); L <= 17."""
    L = x.shape[0]
    assert L <= 17
    cands = []
    for i in range(L):
        for j in range(i + 1, L):
            v = float(x[i, j])
            if j - i >= min_sep and v == v:
                cands.append((-v, i, j))
    cands.sort()
    cands = cands[:k]
    pairs = np.array([(i, j) for _, i, j in cands], dtype=np.int64).reshape(-1, 2)
    scores = np.array([0.0 if nv == 0 else -nv for nv, _, _ in cands], dtype=np.float64)
    return pairs, scores
