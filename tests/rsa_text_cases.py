"""The contract of the RSA_result tables' device text (include/rnamsm.h: rnamsm_rsa_text) as a Python model, and the cases the host
and GPU tests share.  The model uses no `%` formatting of floats: the digits come from the double's exact ratio, rounded half to
even in integers, so that its agreement with write_rsa_files (np.char.mod + np.savetxt) is a finding and not a tautology.
expected_files() is the yardstick everywhere: write_rsa_files itself, run into a temporary directory."""
import os
import random
import tempfile

import numpy as np

from rnamsm import rsa

LINE_MAX = 23
NAMES8 = [f"model_pcc_{k}_{10 + k}=0.5{k}.pt" for k in range(8)]
LENGTHS = (1, 2, 9, 10, 99, 100, 101, 255, 256, 257, 999, 1000, 1023, 1024)      # index digits change; the 256-line scan passes
KS = (1, 3, 8)
CHUNK = 256                                                                      # positions of one pass of rsa_text_kernel


def header(name: str, model_name=None) -> bytes:
    """What np.savetxt writes in front of a table's rows (it ends the header with a newline of its own)."""
    des = f"{name} predict by {model_name}\n" if model_name is not None else f"{name} predict by ensemble model\n"
    return f"#{des}\n#index\t\tnt\t\tASA\t\tRSA\n\n".encode("ascii")


def seq_for(L: int, seed: int, t_every: int = 7) -> str:
    """ACGU with a T at every t_every-th place."""
    r = np.random.RandomState(seed)
    s = r.choice(list("ACGU"), size=L)
    s[t_every - 1::t_every] = "T"
    return "".join(s)


def uniform_values(K: int, L: int, seed: int) -> np.ndarray:
    return np.random.RandomState(seed).uniform(0.0005, 1.0, size=(K, L)).astype(np.float32)


def _f32_neighbours(x: float):
    c = np.float32(x)
    return [np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(2))]


def special_values() -> np.ndarray:
    """float32 RSA values whose tables sit on the formatter's edges: ASA on a "%.2f" tie (m / 128 x 400 = 25 m / 8, m / 16 x 350 =
    175 m / 8, m odd), RSA on a "%.3f" tie (j / 16, j odd), the carries (ASA 399.995 -> 400.00, 349.995, 9.995, 99.995; RSA 0.9995 -> 1.000)
    with both float32 neighbours, 1.0, and the smallest normal and subnormal (0.00, yet no zero)."""
    vals = [m / 128 for m in range(1, 128, 2)] + [j / 16 for j in range(1, 16, 2)]
    for x in (399.995 / 400, 349.995 / 350, 0.9995, 9.995 / 400, 9.995 / 350, 99.995 / 400, 99.995 / 350, 0.0005, 0.005 / 400, 0.995 / 350,
              0.125 / 400, 0.5, 0.0625, 0.1875):
        vals += _f32_neighbours(x)
    vals += [1.0, np.nextafter(np.float32(1), np.float32(0)), np.float32(2.0 ** -126), np.float32(2.0 ** -149), np.float32(2.0 ** -140)]
    return np.array(vals, dtype=np.float32)


def seam_positions(L: int):
    """First, last, and both sides of every seam between two passes of the kernel."""
    pos = {0, L - 1}
    for s in range(CHUNK, L, CHUNK):
        pos |= {s - 1, s}
    return sorted(p for p in pos if 0 <= p < L)


def special_table(K: int, L: int, seed: int) -> np.ndarray:
    """Uniform values with the special set at the first and last position and around every seam (a different special value per
    member and place, all of them used over the lengths and members), and one stretch of them in a row where L allows."""
    v = uniform_values(K, L, seed)
    sp = special_values()
    n = 0
    for p in seam_positions(L):
        for k in range(K):
            v[k, p] = sp[(seed + n) % len(sp)]
            n += 1
    if L > len(sp) + 2:
        v[seed % K, 1:1 + len(sp)] = sp
    return v


# ---------------------------------------------------------------------- the model
def _round_half_even(v: float, d: int) -> int:
    num, den = float(v).as_integer_ratio()            # den: a power of two
    num *= 10 ** d
    q, r = divmod(num, den)
    return q + (1 if 2 * r > den or (2 * r == den and q & 1) else 0)


def _fixed(v: float, d: int) -> str:
    q = _round_half_even(v, d)
    return f"{q // 10 ** d}.{q % 10 ** d:0{d}d}"


SCALE = {"A": 400, "G": 400, "C": 350, "U": 350, "T": 350}


def model(values: np.ndarray, seq: str):
    """-> (bodies: K + 1 byte strings or None with the fallback word set, counts int32 [K + 3], ens float64 [2, L] or None)."""
    values = np.asarray(values, dtype=np.float32)
    K, L = values.shape
    counts = np.zeros(K + 3, dtype=np.int32)
    bits = values.view(np.uint32)
    if (bits > 0x3f800000).any() or any(c not in SCALE for c in seq):
        counts[K + 1] = 1
        return None, counts, None
    scale = [SCALE[c] for c in seq]
    asa = [[float(values[k, p]) * scale[p] for p in range(L)] for k in range(K)]           # Python floats: IEEE doubles, nothing fused
    asa_e, rsa_e = [], []
    for p in range(L):
        s = asa[0][p]
        for k in range(1, K):
            s = s + asa[k][p]
        asa_e.append(s / K)
        rsa_e.append(asa_e[-1] / scale[p])
    counts[K + 2] = int(any(a == 0 for row in asa for a in row) or any(a == 0 for a in asa_e))
    tables = [(asa[k], [float(values[k, p]) for p in range(L)]) for k in range(K)] + [(asa_e, rsa_e)]
    bodies = []
    for f, (a, r) in enumerate(tables):
        body = "".join(f"{p + 1}\t\t{seq[p]}\t\t{_fixed(a[p], 2)}\t\t{_fixed(r[p], 3)}\n" for p in range(L)).encode("ascii")
        assert len(body) <= LINE_MAX * L
        counts[f] = len(body)
        bodies.append(body)
    return bodies, counts, np.array([asa_e, rsa_e], dtype=np.float64)


# ---------------------------------------------------------------------- the yardstick
def tree(root) -> dict:
    root = str(root)
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def expected_files(values: np.ndarray, seq: str, name: str = "x", names=None, rng=None):
    """write_rsa_files on the host -> (files {relative path: bytes}, (asa_e, rsa_e))."""
    names = NAMES8[:values.shape[0]] if names is None else names
    with tempfile.TemporaryDirectory(prefix="rsa_text_cases_") as d:
        ens = rsa.write_rsa_files(values, seq, name, d, names, rng or random.Random(2022))
        return tree(d), ens


def expected_bodies(values: np.ndarray, seq: str, name: str = "x"):
    """The K + 1 bodies of write_rsa_files' tables (the files without their headers) and the ensemble it returns."""
    K = values.shape[0]
    files, ens = expected_files(values, seq, name)
    bodies = []
    for f in range(K + 1):
        sub, head = (f"{name}_{f}", header(name, NAMES8[f])) if f < K else (f"{name}_ensemble", header(name))
        data = files[os.path.join("RSA_result", sub, f"{name}.txt")]
        assert data.startswith(head), data[:80]
        bodies.append(data[len(head):])
    return bodies, np.array(ens, dtype=np.float64)


def split_text(text: np.ndarray, counts: np.ndarray, K: int, L: int):
    """The K + 1 bodies of a device text buffer, by its counts."""
    text, counts = np.asarray(text, dtype=np.uint8).reshape(-1), np.asarray(counts).reshape(-1)
    assert text.shape[0] == (K + 1) * LINE_MAX * L and counts.shape[0] == K + 3
    return [bytes(text[f * LINE_MAX * L:f * LINE_MAX * L + int(counts[f])]) for f in range(K + 1)]


def text_record_from_host(values: np.ndarray, seq: str, name: str = "x", fill: int = 0xFF):
    """A text record as the device would hand it over, built from the host path's own files: (text uint8, counts int32, ens)."""
    K, L = values.shape
    bodies, ens = expected_bodies(values, seq, name)
    text = np.full((K + 1) * LINE_MAX * L, fill, dtype=np.uint8)
    counts = np.zeros(K + 3, dtype=np.int32)
    for f, b in enumerate(bodies):
        text[f * LINE_MAX * L:f * LINE_MAX * L + len(b)] = np.frombuffer(b, dtype=np.uint8)
        counts[f] = len(b)
    return text, counts, ens
