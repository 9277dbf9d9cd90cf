"""Partner vectors and their `.ct` / `.bpseq` bodies for the tests of csrc/struct_text.h (tests/test_struct_text_host.py on the CPU,
tests/test_gpu_struct_text.py on the device).  The bodies come from Python's own formatting, never from the header."""
import numpy as np

CT_LINE = "%d\t\t%c\t\t%d\t\t%d\t\t%d\t\t%d\n"
BPSEQ_LINE = "%d %c %d\n"
MIN_LOOP = 3


def letters_for(L: int, seed: int) -> np.ndarray:
    """uint8 [L]: the characters of a seeded sequence over ACGU."""
    return np.frombuffer(b"ACGU", dtype=np.uint8)[np.random.default_rng(1000 + seed).integers(0, 4, L)]


def nested_partner(L: int, seed: int) -> np.ndarray:
    """int32 [L], 0 or the partner's 1-based index: a seeded set of mutually nested helices.  No base is in two pairs, every pair
    (i, j) has j - i > MIN_LOOP (so every hairpin keeps at least MIN_LOOP unpaired bases), and for L > 4 the pair (1, L) is in it."""
    rng = np.random.default_rng(seed)
    partner = np.zeros(L, dtype=np.int32)
    stack = [(0, L - 1, True)]
    while stack:
        lo, hi, forced = stack.pop()
        if hi - lo <= MIN_LOOP:
            continue
        r = rng.random()
        if forced or r < 0.6:                                  # a pair, and most often the next one of its helix inside it
            partner[lo], partner[hi] = hi + 1, lo + 1
            stack.append((lo + 1, hi - 1, False))
        elif r < 0.8:
            stack.append((lo + 1, hi, False))
        else:                                                  # two structures side by side
            mid = int(rng.integers(lo, hi))
            stack += [(lo, mid, False), (mid + 1, hi, False)]
    return partner


def widest_partner(L: int) -> np.ndarray:
    """int32 [L]: every base with the partner of the most digits that is not itself (a column of numbers for the formatter, not a
    structure)."""
    partner = np.full(L, L, dtype=np.int32)
    partner[L - 1] = L - 1
    return partner


def pairs(partner) -> int:
    return int(sum(p > b + 1 for b, p in enumerate(partner)))


def bodies(partner, letters):
    """(.ct body, .bpseq body) as bytes."""
    L = len(partner)
    rows = [(b + 1, int(c), int(p)) for b, (c, p) in enumerate(zip(letters, partner))]
    ct = "".join(CT_LINE % (i, c, i - 1, 0 if i == L else i + 1, p, i) for i, c, p in rows)
    bp = "".join(BPSEQ_LINE % (i, c, p) for i, c, p in rows)
    return ct.encode("latin-1"), bp.encode("latin-1")


def planted_probs(partner) -> np.ndarray:
    """float32 [L, L]: zero but for 0.9 at the upper-triangle entry of every pair."""
    L = len(partner)
    prob = np.zeros((L, L), dtype=np.float32)
    lower = [b for b in range(L) if partner[b] > b + 1]
    prob[lower, [partner[b] - 1 for b in lower]] = 0.9
    return prob
