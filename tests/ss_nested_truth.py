"""Truth for the nested structure decoding (rnamsm_ss_nested), written from the contract in include/rnamsm.h and independent of
csrc/ss_nested.h -- never the code under test.  NumPy int64 throughout.
  weights            the allowed pairs and their integer weights
  decode             the recurrence, one column at a time (vectorised over k and i), and the canonical traceback
  score_second       a differently shaped recurrence (bifurcations over two sub-intervals) whose optimum must equal decode's
  brute_force_score  every matching of at most ten bases enumerated; the crossing ones thrown away
  check_properties   what every device result must satisfy
  bodies             the .ct / .bpseq bodies and the dot-bracket line of a partner vector
Inputs shared by the host test and the GPU test are built here too (from tests/ss_pairs_cases.py), each expectation once per process."""
import functools

import numpy as np

import ss_pairs_cases as C

NEG = -(1 << 30)
SCALE = 1 << 18


def weights(prob: np.ndarray, theta: float, min_loop: int) -> np.ndarray:
    """int64 [L, L]: w(i, j) on the allowed pairs of the strict upper triangle, NEG everywhere else."""
    p = np.asarray(prob, dtype=np.float32)
    L = p.shape[0]
    th = np.float32(theta)
    with np.errstate(invalid="ignore"):
        above = p > th                                         # NaN and -inf: False
    i, j = np.indices((L, L))
    allowed = above & (j - i > min_loop)
    clipped = np.where(allowed, np.minimum(p.astype(np.float64), 1.0), 0.0)      # a float32 times 2^18 is exact in float64 too
    q = np.floor(clipped * SCALE).astype(np.int64)
    q_theta = int(np.floor(float(th) * SCALE))
    return np.where(allowed, np.maximum(1, q - q_theta), NEG).astype(np.int64)


def _tables(W: np.ndarray, min_loop: int):
    """A [L, L + 1] with A[i, k] = N(i, k - 1) (NEG for k < i, 0 at k = i) and M [L, L]; column j of N needs only earlier columns."""
    L = W.shape[0]
    A = np.full((L, L + 1), NEG, dtype=np.int64)
    A[np.arange(L), np.arange(L)] = 0
    M = np.full((L, L), NEG, dtype=np.int64)
    for j in range(L):
        # N(k + 1, j - 1) = A[k + 1, j] for k + 1 <= j - 1, else 0
        if j >= 1:
            inner = np.zeros(j, dtype=np.int64)
            if j >= 2:
                inner[:j - 1] = A[1:j, j]                      # rows k + 1 = 1 .. j - 1; k = j - 1 encloses nothing
            ok = W[:j, j] > NEG
            M[:j, j] = np.where(ok, W[:j, j] + inner, NEG)
        col = A[:j + 1, j].copy()                              # N(i, j - 1), i <= j (0 at i = j)
        hi = j - min_loop                                      # k < hi
        if hi > 0:
            cand = A[:hi, :hi] + M[:hi, j][None, :]            # [i, k]; k < i holds NEG + something: never the maximum
            col[:hi] = np.maximum(col[:hi], cand.max(axis=1))
        A[:j + 1, j + 1] = col
    return A, M


def decode(prob: np.ndarray, theta: float = 0.516, min_loop: int = 3):
    """-> (partner int32 [L], score): the canonical structure of the contract."""
    W = weights(prob, theta, min_loop)
    L = W.shape[0]
    A, M = _tables(W, min_loop)
    partner = np.zeros(L, dtype=np.int32)
    stack = [(0, L - 1)]
    while stack:
        i, j = stack.pop()
        while j > i:
            if A[i, j + 1] == A[i, j]:                         # N(i, j) == N(i, j - 1): j stays unpaired
                j -= 1
                continue
            ks = np.arange(i, j - min_loop)
            hit = np.nonzero(A[i, ks] + M[ks, j] == A[i, j + 1])[0]
            k = int(ks[hit[0]])                                # the smallest
            partner[k], partner[j] = j + 1, k + 1
            stack.append((k + 1, j - 1))
            j = k - 1
    return partner, int(A[0, L])


def score_second(prob: np.ndarray, theta: float, min_loop: int) -> int:
    """N(i, j) = max(N(i+1, j), N(i, j-1), N(i+1, j-1) + w(i, j) if allowed, max_k N(i, k) + N(k+1, j))."""
    W = weights(prob, theta, min_loop)
    L = W.shape[0]
    N = np.zeros((L + 1, L + 1), dtype=np.int64)               # N[i, j] = 0 for j <= i; row L and the lower triangle stay 0
    for d in range(1, L):
        for i in range(L - d):
            j = i + d
            best = max(N[i + 1, j], N[i, j - 1])
            if W[i, j] > NEG:
                best = max(best, N[i + 1, j - 1] + W[i, j])
            if d >= 2:
                best = max(best, int((N[i, i:j] + N[i + 1:j + 1, j]).max()))
            N[i, j] = best
    return int(N[0, L - 1])


def brute_force_score(prob: np.ndarray, theta: float, min_loop: int) -> int:
    W = weights(prob, theta, min_loop)
    L = W.shape[0]
    assert L <= 10
    best = 0

    def crossing(pairs):
        return any(a < c < b < d or c < a < d < b for n, (a, b) in enumerate(pairs) for c, d in pairs[n + 1:])

    def walk(pos, used, pairs, total):
        nonlocal best
        if pos == L:
            if total > best and not crossing(pairs):
                best = total
            return
        walk(pos + 1, used, pairs, total)
        if pos in used:
            return
        for j in range(pos + 1, L):
            if j not in used and W[pos, j] > NEG:
                walk(pos + 1, used | {pos, j}, pairs + [(pos, j)], total + int(W[pos, j]))

    walk(0, frozenset(), [], 0)
    return best


def pairs_of(partner) -> list:
    return [(b, int(p) - 1) for b, p in enumerate(partner) if p > b + 1]


def check_properties(prob, theta, min_loop, partner, counts, want_score=None):
    """A valid matching, nested, of allowed pairs, whose weights sum to counts[4] (and to the truth's score)."""
    W = weights(prob, theta, min_loop)
    L = W.shape[0]
    partner = np.asarray(partner)
    assert partner.shape == (L,) and partner.min() >= 0 and partner.max() <= L
    for b, p in enumerate(partner):
        assert p == 0 or (p - 1 != b and partner[p - 1] == b + 1), (b, p)
    pairs = pairs_of(partner)
    assert 2 * len(pairs) == int((partner > 0).sum()) and counts[0] == len(pairs)
    open_at = []                                               # nested <=> the brackets close in stack order
    for b, p in enumerate(partner):
        if p > b + 1:
            open_at.append(b)
        elif p:
            assert open_at and open_at.pop() == p - 1, ("crossing pairs", b, p)
    assert not open_at
    assert all(W[i, j] > NEG for i, j in pairs)
    total = sum(int(W[i, j]) for i, j in pairs)
    assert total == int(counts[4]), (total, int(counts[4]))
    if want_score is not None:
        assert total == want_score, (total, want_score)


def bodies(partner, seq: str):
    """(.ct body, .bpseq body, dot-bracket line) of a partner vector, as bytes."""
    L = len(seq)
    ct = "".join("%d\t\t%s\t\t%d\t\t%d\t\t%d\t\t%d\n" % (i, seq[i - 1], i - 1, 0 if i == L else i + 1, partner[i - 1], i)
                 for i in range(1, L + 1))
    bp = "".join("%d %s %d\n" % (i, seq[i - 1], partner[i - 1]) for i in range(1, L + 1))
    dbn = "".join("." if p == 0 else "(" if p > b + 1 else ")" for b, p in enumerate(partner))
    return ct.encode(), bp.encode(), dbn.encode()


def partner_from_dbn(dbn: str) -> np.ndarray:
    partner, open_at = np.zeros(len(dbn), dtype=np.int32), []
    for b, ch in enumerate(dbn):
        if ch == "(":
            open_at.append(b)
        elif ch == ")":
            a = open_at.pop()
            partner[a], partner[b] = b + 1, a + 1
        else:
            assert ch == "."
    assert not open_at
    return partner


_CACHE = {}


def expected(key: str, prob: np.ndarray, seq: str, theta: float = 0.516, min_loop: int = 3):
    """(partner, score, ct body, bpseq body, dbn) of the truth, once per key."""
    if key not in _CACHE:
        partner, score = decode(prob, theta, min_loop)
        _CACHE[key] = (partner, score, *bodies(partner, seq))
    return _CACHE[key]


# ---------------------------------------------------------------------- inputs
def pseudoknot(L: int = 40) -> np.ndarray:
    """Two crossing helices on a quiet background: six pairs at 0.9 (bases 2..7 with 25..20) and five at 0.95 (bases 12..16 with
    36..32).  Each pair of the second crosses each pair of the first; the first is heavier as a whole (6 x 0.384 > 5 x 0.434), so it
    must win whole, although every single pair of the second is heavier."""
    p = np.full((L, L), 0.05, dtype=np.float32)
    for n in range(6):
        p[2 + n, 25 - n] = 0.9
    for n in range(5):
        p[12 + n, 36 - n] = 0.95
    return p


def planted_4096():
    """L = 4096 with a known optimum: nested helices at p = 0.9 -- disjoint ones side by side, and stacks of one inside another --
    noise strictly below theta everywhere else, and one crossing helix at 0.8, lighter than what it crosses.
    -> (prob, partner, score)"""
    L = 4096
    rng = np.random.RandomState(4096)
    p = (0.5 * rng.rand(L, L)).astype(np.float32)              # < 0.516
    partner = np.zeros(L, dtype=np.int32)
    n_pairs = 0
    for lo in range(0, L, 256):                                # sixteen domains of 256 bases, side by side
        for a, b, n in ((lo + 2, lo + 250, 40), (lo + 45, lo + 120, 30), (lo + 125, lo + 205, 35), (lo + 162, lo + 168, 1)):
            for s in range(n):                                 # a helix of n stacked pairs (a + s, b - s)
                p[a + s, b - s] = 0.9
                partner[a + s], partner[b - s] = b - s + 1, a + s + 1
                n_pairs += 1
    # spanning pairs across tile and domain borders, nested around everything: bases 0 / 1 of the first domain with the last two
    p[0, L - 1] = p[1, L - 3] = 0.9
    partner[0], partner[L - 1], partner[1], partner[L - 3] = L, 1, L - 2, 2
    n_pairs += 2
    for s in range(20):                                        # the crossing helix: opens inside the 30-pair helix of domain 3,
        p[3 * 256 + 80 + s, 9 * 256 + 100 - s] = 0.8           # closes inside a loop of domain 9: it crosses 40 + 30 pairs at least
    w = int(np.floor(float(np.float32(0.9)) * SCALE)) - int(np.floor(float(np.float32(0.516)) * SCALE))
    return p, partner, n_pairs * w


@functools.lru_cache(maxsize=None)
def small_cases():
    """name -> (prob, seq, theta, min_loop): the maps the host test and the GPU test both decode."""
    cases = {}
    for L in (1, 2, 4, 5, 63, 64, 65, 129, 197, 200, 260):
        cases[f"random_{L}"] = (C.random_sigmoid(L, 100 + L), C.seq_for(L, L), 0.516, 3)
    for L, seed in ((7, 1), (39, 2), (65, 3), (130, 4)):
        cases[f"ties_{L}"] = (C.ties(L, seed), C.seq_for(L, seed), 0.516, 3)
    for L in (3, 5, 66):
        cases[f"dense_{L}"] = (C.dense(L), C.seq_for(L, L), 0.516, 3)
    for L, seed in ((17, 5), (64, 6), (70, 7), (131, 8)):
        cases[f"sprinkled_{L}"] = (C.sprinkled(L, seed), C.seq_for(L, seed), 0.516, 3)
    for kind in ("nan", "one", "transposed"):
        cases[f"garbage_{kind}_67"] = (C.with_garbage_below(C.random_sigmoid(67, 21), kind), C.seq_for(67, 21), 0.516, 3)
    cases["pseudoknot_40"] = (pseudoknot(), C.seq_for(40, 40), 0.516, 3)
    cases["theta0_66"] = (C.random_sigmoid(66, 31), C.seq_for(66, 31), 0.0, 3)
    cases["theta099_70"] = (C.random_sigmoid(70, 32, 2.0), C.seq_for(70, 32), 0.99, 3)
    cases["loop0_69"] = (C.random_sigmoid(69, 33), C.seq_for(69, 33), 0.516, 0)
    cases["loop32_100"] = (C.random_sigmoid(100, 34, 0.0), C.seq_for(100, 34), 0.516, 32)
    cases["sprinkled_theta0_33"] = (C.sprinkled(33, 9), C.seq_for(33, 9), 0.0, 0)
    return cases
