"""The structure decoding without a GPU.  csrc/ss_pairs.h -- the kernel's round logic and its line formatter -- is compiled into a
stand-alone program (tests/native/ss_pairs_check.cpp) with g++ and AddressSanitizer + UBSan, which runs the rounds serially over the
"threads" on heap buffers of exactly the documented sizes; its partner vectors and bodies are compared with the host path called the
old way (ss.secondary_structure, ss.write_ss_files: pinned to the reference by tests/test_ss_post.py) and with the reference-made
fixtures.  Then the C ABI's symbols, sizes and refusals (made before anything is enqueued, on fabricated addresses that are never
dereferenced) and write_ss_files' new arguments."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rnamsm import _lib, ss
import ss_pairs_cases as C

SRC = os.path.join(ROOT, "tests", "native", "ss_pairs_check.cpp")
FAKE = 0x10000


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host check of ss_pairs.h"
    exe = str(tmp_path_factory.mktemp("ss_pairs") / "ss_pairs_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    SRC, "-o", exe], check=True)
    return exe


def _decode(program, tmp_path, cases):
    """cases: [(prob, seq)] -> [(partner, counts, ct body, bpseq body)] from the program."""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for prob, seq in cases:
            L = len(seq)
            assert prob.shape == (L, L) and prob.dtype == np.float32
            f.write(np.int32(L).tobytes() + bytes(ss.letter_codes(seq)) + np.ascontiguousarray(prob).tobytes())
    res = subprocess.run([program, str(src), str(dst)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    blob, at, out = dst.read_bytes(), 0, []
    for _, seq in cases:
        L = len(seq)
        partner = np.frombuffer(blob, dtype=np.int32, count=L, offset=at)
        counts = np.frombuffer(blob, dtype=np.int32, count=4, offset=at + 4 * L)
        at += 4 * L + 16
        ct, bp = blob[at:at + counts[1]], blob[at + counts[1]:at + counts[1] + counts[2]]
        at += int(counts[1]) + int(counts[2])
        out.append((partner, counts, ct, bp))
    assert at == len(blob)
    return out


def test_standard_cases_match_the_host_path(program, tmp_path):
    cases = C.standard_cases()
    got = _decode(program, tmp_path, list(cases.values()))
    for (key, (prob, seq)), (partner, counts, ct, bp) in zip(cases.items(), got):
        pairs, want_partner, want_ct, want_bp, _, _ = C.expected(key, prob, seq)
        assert partner.tolist() == want_partner.tolist(), key
        assert ss.pairs_from_partner(partner) == pairs, key
        assert counts[0] == len(pairs) and counts[3] == 0, key
        assert ct == want_ct, key
        assert bp == want_bp, key
    assert len(C.expected("dense_65", *cases["dense_65"])[0]) == 1          # L - 2 rounds leave one pair
    assert C.expected("iterative_6x6", *cases["iterative_6x6"])[0] == [(0, 3), (2, 4)]


def test_fixture_cases_equal_their_stored_tables(program, tmp_path):
    cases = [C.fixture(c) for c in C.FIXTURE_CASES]
    got = _decode(program, tmp_path, [(p, s) for p, s, _, _ in cases])
    for c, (_, seq, ct_file, bp_file), (_, _, ct, bp) in zip(C.FIXTURE_CASES, cases, got):
        assert f"{len(seq)}\t\t{c}\t\tRNAMSM_SS output\n\n".encode() + ct == ct_file, c
        assert f"#{c}\n".encode() + bp == bp_file, c


def test_l1024_with_planted_multiplets_and_every_digit_boundary(program, tmp_path):
    prob, seq = C.helix_noise_1024(), C.seq_for(1024, 9)
    pairs, want_partner, want_ct, want_bp, _, _ = C.expected("helix_1024", prob, seq)
    above = int((prob[np.triu_indices(1024, k=1)] > np.float32(0.516)).sum())
    assert len(pairs) < above                                             # the host function removed at least one pair
    assert (300, 802) in pairs and (300, 800) not in pairs and (300, 801) not in pairs      # ... over two rounds
    assert {9, 10, 99, 100, 999, 1000, 1024} <= set(want_partner.tolist())
    (partner, counts, ct, bp), = _decode(program, tmp_path, [(prob, seq)])
    assert partner.tolist() == want_partner.tolist()
    assert ct == want_ct and bp == want_bp and counts[0] == len(pairs)


def test_line_formatter_at_every_digit_boundary(program):
    rows = []
    for L in (1, 9, 10, 11, 99, 100, 101, 999, 1000, 1001, 1024):
        for i in sorted({1, 2, 9, 10, 11, 99, 100, 101, 999, 1000, 1001, 1023, 1024, L - 1, L} & set(range(1, L + 1))):
            for partner in sorted({0, 1, 9, 10, 99, 100, 999, 1000, 1024} & set(range(0, L + 1))):
                rows.append((i, L, partner, ord("ACGU~ "[(i + partner) % 6])))
    res = subprocess.run([program, "--lines"], input="".join("%d %d %d %d\n" % r for r in rows).encode(), capture_output=True)
    assert res.returncode == 0, res.stderr[-2000:]
    want = b"".join(("%d\t\t%c\t\t%d\t\t%d\t\t%d\t\t%d\n" % (i, c, i - 1, 0 if i == L else i + 1, p, i)
                     + "%d %c %d\n" % (i, c, p)).encode() for i, L, p, c in rows)
    assert res.stdout == want
    assert any(r[0] == r[1] for r in rows) and len(rows) > 500              # last lines (the 0) are among them
    longest = max(len("%d\t\t%c\t\t%d\t\t%d\t\t%d\t\t%d\n" % (i, c, i - 1, 0 if i == L else i + 1, p, i)) for i, L, p, c in rows)
    assert longest == _lib.SS_CT_LINE_MAX == 32 and _lib.SS_BPSEQ_LINE_MAX == len("1024 A 1000\n") == 12


def test_a_letter_outside_ascii_sets_the_fallback_word(program, tmp_path):
    prob = C.ties(7, 1)
    (partner, counts, _, _), = _decode(program, tmp_path, [(prob, "ACGéACG")])
    assert counts[3] == 1 and partner.tolist() == C.partner_of_pairs(ss.secondary_structure(prob), 7).tolist()


# ---------------------------------------------------------------------- the library, without a GPU
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_sizes_and_bounds(lib):
    assert {"rnamsm_ss_pairs_workspace_bytes", "rnamsm_ss_struct_text_bytes", "rnamsm_ss_pairs",
            "rnamsm_ss_pairs_packed"} <= set(_lib.EXPORTED_SYMBOLS)
    assert ctypes.sizeof(_lib.SsPairsItem) == 56
    ct, bp = ctypes.c_size_t(), ctypes.c_size_t()
    for L in (1, 35, 64, 65, 1024):
        assert lib.rnamsm_ss_struct_text_bytes(L, ctypes.byref(ct), ctypes.byref(bp)) == 0
        assert (ct.value, bp.value) == (32 * L, 12 * L)
        one = lib.rnamsm_ss_pairs_workspace_bytes(1, (ctypes.c_int * 1)(L))
        assert one >= 8 * L * ((L + 63) // 64) and one % 256 == 0
    assert lib.rnamsm_ss_pairs_workspace_bytes(1, (ctypes.c_int * 1)(1024)) == 128 * 1024
    Ls = (ctypes.c_int * 3)(1, 65, 1024)
    assert lib.rnamsm_ss_pairs_workspace_bytes(3, Ls) == sum(lib.rnamsm_ss_pairs_workspace_bytes(1, (ctypes.c_int * 1)(L)) for L in Ls)
    assert lib.rnamsm_ss_pairs_workspace_bytes(0, Ls) == 0 and lib.rnamsm_ss_pairs_workspace_bytes(1025, Ls) == 0
    assert lib.rnamsm_ss_pairs_workspace_bytes(3, None) == 0
    assert lib.rnamsm_ss_pairs_workspace_bytes(2, (ctypes.c_int * 2)(5, 0)) == 0
    assert lib.rnamsm_ss_pairs_workspace_bytes(2, (ctypes.c_int * 2)(1025, 5)) == 0
    assert lib.rnamsm_ss_struct_text_bytes(0, ctypes.byref(ct), ctypes.byref(bp)) == -1
    assert lib.rnamsm_ss_struct_text_bytes(1025, ctypes.byref(ct), ctypes.byref(bp)) == -1
    assert lib.rnamsm_ss_struct_text_bytes(5, None, ctypes.byref(bp)) == -1


def _refused(lib, rc, *needles):
    assert rc == -1, rc
    msg = lib.rnamsm_last_error().decode()
    for n in needles:
        assert n in msg, (n, msg)


def test_refusals_on_a_host_without_a_gpu(lib):
    ws = 1 << 20

    def lone(probs=FAKE, letters=2 * FAKE, L=8, partner=3 * FAKE, counts=4 * FAKE, ct=5 * FAKE, bpseq=6 * FAKE, work=7 * FAKE, nbytes=ws):
        return lib.rnamsm_ss_pairs(probs, letters, L, partner, counts, ct, bpseq, work, nbytes, None)

    _refused(lib, lone(L=0), "ss_pairs:", "L=0")
    _refused(lib, lone(L=1025), "L=1025")
    for name in ("probs", "letters", "partner", "counts", "ct", "bpseq", "work"):
        _refused(lib, lone(**{name: None}), "null")
    for name in ("probs", "partner", "counts"):
        _refused(lib, lone(**{name: FAKE + 2}), "4-byte")
    _refused(lib, lone(work=7 * FAKE + 8), "16-byte")
    _refused(lib, lone(nbytes=255), "workspace of 255 bytes", "256 needed")
    _refused(lib, lone(L=1024, nbytes=128 * 1024 - 1), "131072 needed")

    def items(n):
        arr = (_lib.SsPairsItem * n)()
        for b in range(n):
            arr[b] = _lib.SsPairsItem(*[FAKE * (8 * b + k) for k in (1, 2)], 8, *[FAKE * (8 * b + k) for k in (3, 4, 5, 6)])
        return arr

    _refused(lib, lib.rnamsm_ss_pairs_packed(items(1), 0, FAKE, ws, None), "ss_pairs_packed:", "B=0")
    _refused(lib, lib.rnamsm_ss_pairs_packed(items(1025), 1025, FAKE, ws, None), "B=1025")
    _refused(lib, lib.rnamsm_ss_pairs_packed(None, 3, FAKE, ws, None), "null")
    _refused(lib, lib.rnamsm_ss_pairs_packed(items(3), 3, None, ws, None), "null")
    _refused(lib, lib.rnamsm_ss_pairs_packed(items(3), 3, FAKE + 4, ws, None), "16-byte")
    _refused(lib, lib.rnamsm_ss_pairs_packed(items(40), 40, FAKE, 40 * 256 - 1, None), "workspace of 10239 bytes", "10240 needed")
    for member in (0, 1, 32, 39):                        # on either side of the 32-descriptor chunk
        for field, value, needle in (("L", 0, "L=0"), ("L", 1025, "L=1025"), ("probs", None, "null"), ("letters", None, "null"),
                                     ("partner", None, "null"), ("counts", None, "null"), ("ct", None, "null"),
                                     ("bpseq", None, "null"), ("probs", FAKE + 1, "4-byte"), ("partner", FAKE + 2, "4-byte"),
                                     ("counts", FAKE + 3, "4-byte")):
            arr = items(40)
            setattr(arr[member], field, value)
            _refused(lib, lib.rnamsm_ss_pairs_packed(arr, 40, FAKE, ws, None), f"member {member}:", needle)


# ---------------------------------------------------------------------- write_ss_files' new arguments
def _files(root, name="x"):
    return {ext: (root / "SS_result" / f"{name}.{ext}").read_bytes() for ext in ("ct", "bpseq", "prob")}


def test_write_ss_files_with_device_results(tmp_path):
    """The partner vector and the bodies as the device hands them over (here: cut from the host path's own files, padded to the
    buffer bounds): one binary write per table when the fallback word is 0, the host tables when it is 1; no probabilities needed
    when a usable .prob text comes along."""
    import dec19_cases as D
    prob, seq = C.random_sigmoid(35, 11), C.seq_for(35, 11)
    pairs, partner, ct_body, bp_body, _, _ = C.expected("write_35", prob, seq)
    assert len(pairs) >= 3
    text = D.savetxt_bytes(prob)
    counts = np.array([len(pairs), len(ct_body), len(bp_body), 0], dtype=np.int32)
    ct_buf = np.frombuffer(ct_body + b"\xff" * (32 * 35 - len(ct_body)), dtype=np.uint8)
    bp_buf = np.frombuffer(bp_body + b"\xff" * (12 * 35 - len(bp_body)), dtype=np.uint8)
    ss.write_ss_files(prob, seq, "x", tmp_path / "host")
    want = _files(tmp_path / "host")
    kw = dict(partner=partner, counts=counts, ct_body=ct_buf, bpseq_body=bp_buf)
    assert ss.write_ss_files(prob, seq, "x", tmp_path / "a", **kw) == pairs
    assert ss.write_ss_files(None, seq, "x", tmp_path / "b", prob_text=text, fallback=0, **kw) == pairs
    assert ss.write_ss_files(prob, seq, "x", tmp_path / "c", partner=partner) == pairs
    bad = counts.copy()
    bad[3] = 1
    junk = np.full(32 * 35, ord("?"), dtype=np.uint8)
    assert ss.write_ss_files(None, seq, "x", tmp_path / "d", prob_text=text, partner=partner, counts=bad, ct_body=junk,
                             bpseq_body=junk[:12 * 35]) == pairs
    for d in "abcd":
        assert _files(tmp_path / d) == want, d
    marked = ct_buf.copy()
    marked[0] ^= 1                                        # the bodies are written, not re-derived
    ss.write_ss_files(prob, seq, "x", tmp_path / "m", partner=partner, counts=counts, ct_body=marked, bpseq_body=bp_buf)
    got = _files(tmp_path / "m")
    assert got["ct"] != want["ct"] and got["ct"][-len(ct_body) + 1:] == ct_body[1:] and got["bpseq"] == want["bpseq"]
    with pytest.raises(ValueError):
        ss.write_ss_files(None, seq, "x", tmp_path / "e", partner=partner)              # no way to write .prob
    with pytest.raises(ValueError):
        ss.write_ss_files(None, seq, "x", tmp_path / "e", prob_text=text, fallback=1, **kw)
    with pytest.raises(ValueError):
        ss.write_ss_files(None, seq, "x", tmp_path / "e", prob_text=text)              # no way to find the pairs
    with pytest.raises(ValueError):
        ss.write_ss_files(prob, seq, "x", tmp_path / "e", partner=partner[:-1])


def test_pairs_from_partner():
    assert ss.pairs_from_partner(np.array([4, 0, 5, 1, 3, 0])) == [(0, 3), (2, 4)]
    assert ss.pairs_from_partner(np.zeros(3, dtype=np.int32)) == []
    for key in ("ties_39", "sprinkled_70"):
        prob, seq = C.standard_cases()[key]
        pairs = ss.secondary_structure(prob)
        assert ss.pairs_from_partner(C.partner_of_pairs(pairs, len(seq))) == pairs


def test_config_key_defaults_to_on():
    from rnamsm.config import Config
    assert Config().data.ss_pairs_device is True
