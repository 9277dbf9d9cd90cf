"""The identity redundancy filter (rnamsm_seqid_filter, rnamsm.msa.seqid_filter) restated in plain loops over bytes: no words, no
vectorised masks, nothing shared with rnamsm.  The rule, all in integers:

  both(i, j) = the columns where neither row has the gap; same(i, j) = those of them where the bytes are equal; nres(i) = both(i, i).
  Row k is redundant to row j at threshold t iff both > 0 and 100 * same >= t * both.
  Order: row 0, then the others by descending nres, ties by ascending index (or the order given).
  Thresholds: num_seqs > 0: min_seqid, min_seqid + step, ... while below max_seqid, then max_seqid; num_seqs == 0 or
  min_seqid >= max_seqid: max_seqid alone.
  A pass at t walks the rows not kept yet, in order; a row is kept iff it is redundant at t to no kept row (of an earlier pass or
  earlier in this one); a row with nres == 0 is never kept unless it is the first of the order, which always is.
  The walk stops after the first pass that leaves num_seqs rows kept (num_seqs > 0), and after the last threshold.

`memo` (a dict) keeps the pair counts of one alignment between calls: they depend on neither the thresholds nor num_seqs."""
import numpy as np


def thresholds(num_seqs, min_seqid=20, max_seqid=90, step=5):
    out = []
    if num_seqs > 0:
        t = min_seqid
        while t < max_seqid:
            out.append(t)
            t += step
    out.append(max_seqid)
    return out


def pair(a, b, gap):
    """(both, same) of two rows given as bytes."""
    both = same = 0
    for x, y in zip(a, b):
        if x != gap and y != gap:
            both += 1
            if x == y:
                same += 1
    return both, same


def default_order(rows, gap):
    nres = [sum(1 for x in r if x != gap) for r in rows]
    return [0] + sorted(range(1, len(rows)), key=lambda i: (-nres[i], i))


def seqid_filter(msa, gap, num_seqs, min_seqid=20, max_seqid=90, step=5, order=None, memo=None):
    """msa: uint8 [N, L] -> (kept indices ascending, kept_at per row, [(threshold, rows kept after that pass)])."""
    rows = [bytes(np.asarray(r, dtype=np.uint8).tobytes()) for r in msa]
    N = len(rows)
    memo = {} if memo is None else memo
    order = default_order(rows, gap) if order is None else [int(i) for i in order]
    nres = [sum(1 for x in r if x != gap) for r in rows]
    kept_at = [-1] * N
    kept = []
    passes = []
    for t in thresholds(num_seqs, min_seqid, max_seqid, step):
        for pos, r in enumerate(order):
            if kept_at[r] >= 0 or (nres[r] == 0 and pos != 0):
                continue
            redundant = False
            for j in kept:
                key = (r, j) if r < j else (j, r)
                c = memo.get(key)
                if c is None:
                    c = memo[key] = pair(rows[r], rows[j], gap)
                if c[0] > 0 and 100 * c[1] >= t * c[0]:
                    redundant = True
                    break
            if not redundant:
                kept.append(r)
                kept_at[r] = t
        passes.append((t, len(kept)))
        if num_seqs > 0 and len(kept) >= num_seqs:
            break
    return np.array(sorted(kept), dtype=np.int64), np.array(kept_at, dtype=np.int32), passes


def alignment(N, L, seed, gap=10, symbols=(4, 5, 6, 7), p_gap=0.15, families=None, p_mut=0.12):
    """A synthetic alignment with planted near copies: `families` founders of random symbols and gaps, every other row a founder
    with each column redrawn with probability p_mut (rates drawn per row between 0 and 2 * p_mut, so that identities spread over
    the thresholds).  uint8 [N, L]."""
    rng = np.random.RandomState(seed)
    families = max(1, N // 6) if families is None else families
    alphabet = np.array(list(symbols) + [gap], dtype=np.uint8)
    p = np.array([(1 - p_gap) / len(symbols)] * len(symbols) + [p_gap])
    founders = alphabet[rng.choice(len(alphabet), size=(families, L), p=p)]
    out = np.empty((N, L), dtype=np.uint8)
    for i in range(N):
        f = founders[rng.randint(families)]
        rate = rng.uniform(0, 2 * p_mut)
        redraw = rng.rand(L) < rate
        out[i] = np.where(redraw, alphabet[rng.choice(len(alphabet), size=L, p=p)], f)
    return out
