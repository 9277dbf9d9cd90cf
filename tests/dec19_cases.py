"""Bit patterns of float32 values in [0, 1] on which a "%.18e" formatter can go wrong, shared by the host test of csrc/dec19.h
(test_dec19_host.py) and the GPU test of the kernel around it (test_gpu_ss_text.py).  Everything is derived with exact integer or
rational arithmetic; nothing here comes from the code under test."""
import io
from fractions import Fraction

import numpy as np

ONE = 0x3F800000                      # bits of 1.0f: the domain is [0, ONE]
SMALLEST_NORMAL = 0x00800000


def bits_of(frac: Fraction) -> int:
    """Bits of the float32 that equals `frac` exactly (asserted)."""
    v = np.float32(float(frac))
    assert Fraction(float(v)) == frac, frac
    return int(v.view(np.uint32))


def powers_of_two():
    """2^-k, 3 2^-k and 5 2^-k for k = 0 .. 149, where they lie in [0, 1] (all are exact float32 values)."""
    out = []
    for k in range(150):
        for m in (1, 3, 5):
            if m <= 2 ** k:                    # m 2^-149 is a subnormal float32 for every m < 2^23
                out.append(bits_of(Fraction(m, 2 ** k)))
    return out


def around(center: int, n: int = 64):
    return [b for b in range(center - n, center + n + 1) if 0 <= b <= ONE]


def decade_neighbours():
    """The two float32 values that enclose 10^-d, d = 1 .. 45: the exponent estimate has to tell them apart."""
    out = []
    for d in range(1, 46):
        exact = Fraction(1, 10 ** d)
        b = int(np.float32(float(exact)).view(np.uint32))
        f = Fraction(float(np.uint32(b).view(np.float32)))
        lo, hi = (b - 1, b) if f >= exact else (b, b + 1)
        assert Fraction(float(np.uint32(lo).view(np.float32))) <= exact <= Fraction(float(np.uint32(hi).view(np.float32)))
        out += [lo, hi]
    return out


def ties():
    """Every m 2^-k (m odd, m < 2^12, k <= 60) in [0, 1] whose exact decimal expansion has exactly 20 significant digits: the
    20th is a 5 with nothing behind it, so the 19 printed digits are a round-half-even tie.  m 2^-k = m 5^k / 10^k and m 5^k is
    odd, so its digits are the expansion's significant digits."""
    out = []
    for k in range(1, 61):
        p5 = 5 ** k
        for m in range(1, 1 << 12, 2):
            if m <= 2 ** k and len(str(m * p5)) == 20:
                out.append(bits_of(Fraction(m, 2 ** k)))
    return out


def special_values():
    """The whole special-value set, without duplicates, in a fixed order."""
    vals = powers_of_two() + [0, ONE] + list(range(ONE - 64, ONE)) + around(SMALLEST_NORMAL - 1) + around(SMALLEST_NORMAL)
    vals += decade_neighbours() + ties()
    return list(dict.fromkeys(vals))


def random_patterns(n: int = 1 << 16, seed: int = 19):
    return [int(b) for b in np.random.RandomState(seed).randint(0, ONE + 1, size=n, dtype=np.int64)]


def floats_of(bits) -> np.ndarray:
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def savetxt_bytes(prob: np.ndarray) -> bytes:
    """What the parent's write_ss_files puts into `<name>.prob`."""
    buf = io.BytesIO()
    np.savetxt(buf, prob, delimiter="\t")
    return buf.getvalue()
