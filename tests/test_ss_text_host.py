"""The device-written `.prob` text without a GPU: the C ABI's symbols, sizes and refusals (made before anything is enqueued, on
fabricated addresses that are never dereferenced) and write_ss_files' two paths on 2DRB_1-sized inputs."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from rnamsm import _lib, ss
import dec19_cases as C

FAKE = 0x10000


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_and_sizes(lib):
    assert {"rnamsm_ss_prob_text_bytes", "rnamsm_ss_prob_text", "rnamsm_ss_prob_text_packed"} <= set(_lib.EXPORTED_SYMBOLS)
    assert ctypes.sizeof(_lib.SsTextItem) == 32 and _lib.SS_TEXT_RECORD == 25
    for L in (1, 35, 128, 512, 1024):
        assert lib.rnamsm_ss_prob_text_bytes(L) == 25 * L * L
    assert lib.rnamsm_ss_prob_text_bytes(0) == 0 and lib.rnamsm_ss_prob_text_bytes(1025) == 0


def _refused(lib, rc, *needles):
    assert rc == -1, rc
    msg = lib.rnamsm_last_error().decode()
    for n in needles:
        assert n in msg, (n, msg)


def test_refusals_on_a_host_without_a_gpu(lib):
    _refused(lib, lib.rnamsm_ss_prob_text(FAKE, 0, 2 * FAKE, 3 * FAKE, None), "L=0")
    _refused(lib, lib.rnamsm_ss_prob_text(FAKE, 1025, 2 * FAKE, 3 * FAKE, None), "L=1025")
    _refused(lib, lib.rnamsm_ss_prob_text(None, 8, 2 * FAKE, 3 * FAKE, None), "null")
    _refused(lib, lib.rnamsm_ss_prob_text(FAKE, 8, 2 * FAKE + 4, 3 * FAKE, None), "16-byte")
    _refused(lib, lib.rnamsm_ss_prob_text(FAKE + 2, 8, 2 * FAKE, 3 * FAKE, None), "4-byte")

    def items(n):
        arr = (_lib.SsTextItem * n)()
        for b in range(n):
            arr[b] = _lib.SsTextItem(FAKE * (4 * b + 1), 8, FAKE * (4 * b + 2), FAKE * (4 * b + 3))
        return arr

    _refused(lib, lib.rnamsm_ss_prob_text_packed(items(1), 0, None), "B=0")
    _refused(lib, lib.rnamsm_ss_prob_text_packed(items(1025), 1025, None), "B=1025")
    _refused(lib, lib.rnamsm_ss_prob_text_packed(None, 3, None), "null")
    for member in (0, 1, 32, 39):                        # on either side of the 32-descriptor chunk
        for field, value, needle in (("L", 0, "L=0"), ("L", 1025, "L=1025"), ("probs", None, "null"), ("text", None, "null"),
                                     ("fallback", None, "null"), ("text", FAKE + 8, "16-byte"), ("fallback", FAKE + 1, "4-byte")):
            arr = items(40)
            setattr(arr[member], field, value)
            _refused(lib, lib.rnamsm_ss_prob_text_packed(arr, 40, None), f"member {member}:", needle)


def test_write_ss_files_text_and_fallback(tmp_path):
    """A [35, 35] matrix (the size of tests/golden/ss/2DRB_1_atp.npy's maps): a given text is written as it is when the word is 0,
    and ignored when it is 1; .ct and .bpseq never depend on it."""
    L = np.load(os.path.join(GOLDEN, "ss", "2DRB_1_atp.npy"), mmap_mode="r").shape[-1]
    assert L == 35
    rng = np.random.RandomState(3)
    prob = (1.0 / (1.0 + np.exp(-rng.normal(-2.0, 4.0, size=(L, L))))).astype(np.float32)
    seq = "".join(rng.choice(list("ACGU"), L))
    text = C.savetxt_bytes(prob)
    assert len(text) == 25 * L * L

    def files(root):
        return {ext: (root / "SS_result" / f"x.{ext}").read_bytes() for ext in ("ct", "bpseq", "prob")}

    p0 = ss.write_ss_files(prob, seq, "x", tmp_path / "host")
    p1 = ss.write_ss_files(prob, seq, "x", tmp_path / "bytes", prob_text=text)
    p2 = ss.write_ss_files(prob, seq, "x", tmp_path / "array", prob_text=np.frombuffer(text, dtype=np.uint8), fallback=0)
    p3 = ss.write_ss_files(prob, seq, "x", tmp_path / "ignored", prob_text=b"?" * len(text), fallback=1)
    want = files(tmp_path / "host")
    assert want["prob"] == text
    for name in ("bytes", "array", "ignored"):
        assert files(tmp_path / name) == want, name
    assert p0 == p1 == p2 == p3
    marked = bytes([text[0] ^ 1]) + text[1:]              # the text is written, not re-derived
    ss.write_ss_files(prob, seq, "x", tmp_path / "marked", prob_text=marked)
    assert files(tmp_path / "marked")["prob"] == marked
    with pytest.raises(ValueError):
        ss.write_ss_files(prob, seq, "x", tmp_path / "short", prob_text=text[:-25])
