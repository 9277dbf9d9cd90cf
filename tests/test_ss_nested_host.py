"""The nested structure decoding without a GPU.  csrc/ss_nested.h -- the kernels' tile working set, cell logic and traceback steps --
is compiled into a stand-alone program (tests/native/ss_nested_check.cpp) with g++ and AddressSanitizer + UBSan, which runs the tile
schedule serially on heap buffers of exactly the documented sizes; its partner vectors, scores, dot-bracket lines and bodies are
compared with the truth of tests/ss_nested_truth.py (written from the contract, checked here against a second recurrence and a
brute-force enumeration).  Then the C ABI's symbols, sizes and refusals (made before anything is enqueued, on fabricated addresses
that are never dereferenced), the config keys, write_dbn and write_nested_files."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rnamsm import _lib, ss
import ss_pairs_cases as C
import ss_nested_truth as T

SRC = os.path.join(ROOT, "tests", "native", "ss_nested_check.cpp")
FAKE = 0x10000


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host check of ss_nested.h"
    exe = str(tmp_path_factory.mktemp("ss_nested") / "ss_nested_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe],
                   check=True)
    return exe


def _decode(program, tmp_path, cases):
    """cases: [(prob, seq, theta, min_loop)] -> [(partner, counts, ct body, bpseq body, dbn)] from the program."""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for prob, seq, theta, min_loop in cases:
            L = len(seq)
            assert prob.shape == (L, L) and prob.dtype == np.float32
            f.write(np.int32(L).tobytes() + np.float32(theta).tobytes() + np.int32(min_loop).tobytes() + bytes(ss.letter_codes(seq))
                    + np.ascontiguousarray(prob).tobytes())
    res = subprocess.run([program, str(src), str(dst)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    blob, at, out = dst.read_bytes(), 0, []
    for _, seq, _, _ in cases:
        L = len(seq)
        partner = np.frombuffer(blob, dtype=np.int32, count=L, offset=at)
        counts = np.frombuffer(blob, dtype=np.int32, count=5, offset=at + 4 * L)
        at += 4 * L + 20
        ct, bp = blob[at:at + counts[1]], blob[at + counts[1]:at + counts[1] + counts[2]]
        at += int(counts[1]) + int(counts[2])
        out.append((partner, counts, ct, bp, blob[at:at + L]))
        at += L
    assert at == len(blob)
    return out


def _compare(key, case, got):
    prob, seq, theta, min_loop = case
    partner, counts, ct, bp, dbn = got
    want_partner, want_score, want_ct, want_bp, want_dbn = T.expected(key, prob, seq, theta, min_loop)
    assert partner.tolist() == want_partner.tolist(), key
    assert counts[4] == want_score and counts[3] == 0, key
    assert (ct, bp, dbn) == (want_ct, want_bp, want_dbn), key
    T.check_properties(prob, theta, min_loop, partner, counts, want_score)


def _tiny_cases():
    cases = {}
    for L in range(1, 11):
        for theta in (0.0, 0.516, 0.7):
            for min_loop in (0, 3):
                cases[f"tiny_{L}_{theta}_{min_loop}"] = (C.random_sigmoid(L, 7 * L + min_loop, 0.5), C.seq_for(L, L), theta, min_loop)
        cases[f"tiny_ties_{L}"] = (C.ties(L, L), C.seq_for(L, L), 0.516, 0)
    return cases


def test_the_truth_agrees_with_brute_force_and_with_the_second_recurrence():
    some = 0
    for key, (prob, seq, theta, min_loop) in _tiny_cases().items():
        _, score, _, _, _ = T.expected(key, prob, seq, theta, min_loop)
        assert score == T.brute_force_score(prob, theta, min_loop) == T.score_second(prob, theta, min_loop), key
        some += score > 0
    assert some > 40
    for key in ("random_63", "ties_65", "sprinkled_70", "pseudoknot_40", "theta0_66", "loop0_69"):
        prob, seq, theta, min_loop = T.small_cases()[key]
        assert T.expected(key, prob, seq, theta, min_loop)[1] == T.score_second(prob, theta, min_loop), key


def test_brute_force_cases_match_the_truth(program, tmp_path):
    cases = _tiny_cases()
    for (key, case), got in zip(cases.items(), _decode(program, tmp_path, list(cases.values()))):
        _compare(key, case, got)


def test_small_cases_match_the_truth(program, tmp_path):
    cases = T.small_cases()
    assert {len(c[1]) for c in cases.values()} >= {1, 2, 4, 5, 63, 64, 65, 129, 200}
    for (key, case), got in zip(cases.items(), _decode(program, tmp_path, list(cases.values()))):
        _compare(key, case, got)


def test_the_heavier_of_two_crossing_helices_wins_whole(program, tmp_path):
    case = T.small_cases()["pseudoknot_40"]
    (partner, counts, _, _, dbn), = _decode(program, tmp_path, [case])
    assert T.pairs_of(partner) == [(2 + n, 25 - n) for n in range(6)] and counts[0] == 6
    assert dbn == b"..((((((............))))))" + b"." * 14
    both = ss.secondary_structure(case[0])                           # the reference's decoding keeps the pseudoknot
    assert len(both) == 11


def test_a_letter_outside_ascii_sets_the_fallback_word(program, tmp_path):
    prob = C.random_sigmoid(9, 3, 0.5)
    (partner, counts, _, _, _), = _decode(program, tmp_path, [(prob, "ACGéACGUA", 0.516, 3)])
    assert counts[3] == 1 and partner.tolist() == T.decode(prob)[0].tolist()


def test_nested_structure_host_states_the_same_contract():
    for key in ("random_63", "ties_39", "sprinkled_17", "pseudoknot_40", "loop0_69", "sprinkled_theta0_33"):
        prob, seq, theta, min_loop = T.small_cases()[key]
        partner, score, dbn = ss.nested_structure_host(prob, theta, min_loop)
        want = T.expected(key, prob, seq, theta, min_loop)
        assert partner.tolist() == want[0].tolist() and score == want[1] and dbn.encode() == want[4], key
    with pytest.raises(ValueError):
        ss.nested_structure_host(np.zeros((3, 3), dtype=np.float32), theta=1.0)


# ---------------------------------------------------------------------- the library, without a GPU
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_and_sizes(lib):
    assert {"rnamsm_ss_nested_workspace_bytes", "rnamsm_ss_nested", "rnamsm_ss_nested_packed"} <= set(_lib.EXPORTED_SYMBOLS)
    assert ctypes.sizeof(_lib.SsNestedItem) == 64 and _lib.SS_NESTED_MAX_LOOP == 32
    for L, Lp in ((1, 64), (64, 64), (65, 128), (1024, 1024), (4095, 4096), (4096, 4096)):
        assert lib.rnamsm_ss_nested_workspace_bytes(1, (ctypes.c_int * 1)(L)) == 8 * Lp * Lp
    Ls = (ctypes.c_int * 3)(1, 65, 4096)
    assert lib.rnamsm_ss_nested_workspace_bytes(3, Ls) == 8 * (64 * 64 + 128 * 128 + 4096 * 4096)
    assert lib.rnamsm_ss_nested_workspace_bytes(0, Ls) == 0 and lib.rnamsm_ss_nested_workspace_bytes(1025, Ls) == 0
    assert lib.rnamsm_ss_nested_workspace_bytes(3, None) == 0
    assert lib.rnamsm_ss_nested_workspace_bytes(2, (ctypes.c_int * 2)(5, 0)) == 0
    assert lib.rnamsm_ss_nested_workspace_bytes(2, (ctypes.c_int * 2)(4097, 5)) == 0


def _refused(lib, rc, *needles):
    assert rc == -1, rc
    msg = lib.rnamsm_last_error().decode()
    for n in needles:
        assert n in msg, (n, msg)


def test_refusals_on_a_host_without_a_gpu(lib):
    ws = 1 << 30

    def lone(probs=FAKE, letters=2 * FAKE, L=8, theta=0.516, min_loop=3, partner=3 * FAKE, counts=4 * FAKE, ct=5 * FAKE,
             bpseq=6 * FAKE, dbn=7 * FAKE, work=8 * FAKE, nbytes=ws):
        return lib.rnamsm_ss_nested(probs, letters, L, theta, min_loop, partner, counts, ct, bpseq, dbn, work, nbytes, None)

    _refused(lib, lone(L=0), "ss_nested:", "L=0")
    _refused(lib, lone(L=4097), "L=4097")
    for theta in (-0.01, 1.0, 1.5, float("nan"), float("inf")):
        _refused(lib, lone(theta=theta), "theta")
    for min_loop in (-1, 33):
        _refused(lib, lone(min_loop=min_loop), f"min_loop={min_loop}")
    for name in ("probs", "letters", "partner", "counts", "ct", "bpseq", "dbn", "work"):
        _refused(lib, lone(**{name: None}), "null")
    for name in ("probs", "partner", "counts"):
        _refused(lib, lone(**{name: FAKE + 2}), "4-byte")
    _refused(lib, lone(work=8 * FAKE + 8), "16-byte")
    _refused(lib, lone(nbytes=32767), "workspace of 32767 bytes", "32768 needed")
    _refused(lib, lone(L=4096, nbytes=8 * 4096 * 4096 - 1), "134217728 needed")

    def items(n):
        arr = (_lib.SsNestedItem * n)()
        for b in range(n):
            arr[b] = _lib.SsNestedItem(*[FAKE * (8 * b + k) for k in (1, 2)], 8, *[FAKE * (8 * b + k) for k in (3, 4, 5, 6, 7)])
        return arr

    def packed(arr, B, theta=0.516, min_loop=3, work=FAKE, nbytes=ws):
        return lib.rnamsm_ss_nested_packed(arr, B, theta, min_loop, work, nbytes, None)

    _refused(lib, packed(items(1), 0), "ss_nested_packed:", "B=0")
    _refused(lib, packed(items(1025), 1025), "B=1025")
    _refused(lib, packed(None, 3), "null")
    _refused(lib, packed(items(3), 3, work=None), "null")
    _refused(lib, packed(items(3), 3, work=FAKE + 4), "16-byte")
    _refused(lib, packed(items(3), 3, theta=float("nan")), "theta")
    _refused(lib, packed(items(3), 3, min_loop=40), "min_loop=40")
    _refused(lib, packed(items(40), 40, nbytes=40 * 32768 - 1), "workspace of 1310719 bytes", "1310720 needed")
    for member in (0, 1, 32, 39):                        # on either side of the 32-descriptor chunk
        for field, value, needle in (("L", 0, "L=0"), ("L", 4097, "L=4097"), ("probs", None, "null"), ("letters", None, "null"),
                                     ("partner", None, "null"), ("counts", None, "null"), ("ct", None, "null"),
                                     ("bpseq", None, "null"), ("dbn", None, "null"), ("probs", FAKE + 1, "4-byte"),
                                     ("partner", FAKE + 2, "4-byte"), ("counts", FAKE + 3, "4-byte")):
            arr = items(40)
            setattr(arr[member], field, value)
            _refused(lib, packed(arr, 40), f"member {member}:", needle)


def test_phases_entry_point_refuses_as_the_packed_call_does(lib):
    assert "rnamsm_ss_nested_phases" in _lib.EXPORTED_SYMBOLS
    arr = (_lib.SsNestedItem * 2)()
    for b in range(2):
        arr[b] = _lib.SsNestedItem(*[FAKE * (8 * b + k) for k in (1, 2)], 8, *[FAKE * (8 * b + k) for k in (3, 4, 5, 6, 7)])
    for phases in (0, 4, -1):
        _refused(lib, lib.rnamsm_ss_nested_phases(arr, 2, 0.516, 3, FAKE, 1 << 20, phases, None), f"phases={phases}")
    _refused(lib, lib.rnamsm_ss_nested_phases(arr, 2, 0.516, 3, FAKE, 65535, 1, None), "65536 needed")
    _refused(lib, lib.rnamsm_ss_nested_phases(None, 2, 0.516, 3, FAKE, 1 << 20, 3, None), "null")
    _refused(lib, lib.rnamsm_ss_nested_phases(arr, 2, 2.0, 3, FAKE, 1 << 20, 3, None), "theta")


# ---------------------------------------------------------------------- config keys, write_dbn, write_nested_files
def test_config_keys():
    from rnamsm.config import Config, parse_overrides
    d = Config().data
    assert (d.ss_nested, d.ss_nested_threshold, d.ss_nested_min_loop) == (False, 0.516, 3)
    cfg = parse_overrides(["data.ss_model_path=w.pt", "data.ss_nested=true", "data.ss_nested_threshold=0.4", "data.ss_nested_min_loop=0"])
    assert (cfg.data.ss_nested, cfg.data.ss_nested_threshold, cfg.data.ss_nested_min_loop) == (True, 0.4, 0)
    for argv, key in ((["data.ss_nested=true"], "data.ss_model_path"),
                      (["data.ss_nested_threshold=1.0"], "data.ss_nested_threshold"),
                      (["data.ss_nested_threshold=-0.1"], "data.ss_nested_threshold"),
                      (["data.ss_nested_threshold=nan"], "data.ss_nested_threshold"),
                      (["data.ss_nested_min_loop=33"], "data.ss_nested_min_loop"),
                      (["data.ss_nested_min_loop=-1"], "data.ss_nested_min_loop")):
        with pytest.raises(ValueError, match=key):
            parse_overrides(argv)
    with pytest.raises(ValueError):
        parse_overrides(["data.ss_nested=maybe"])


def test_ss_nested_is_refused_under_a_gather_and_read_into_the_switches():
    from rnamsm.config import parse_overrides
    from rnamsm import inference
    with pytest.raises(ValueError, match="data.ss_nested"):
        inference.refuse_ss_nested_under_gather(True, True)
    inference.refuse_ss_nested_under_gather(True, False)
    inference.refuse_ss_nested_under_gather(False, True)
    on = parse_overrides(["data.ss_model_path=w.pt", "data.ss_nested=true", "data.ss_nested_threshold=0.25", "data.ss_nested_min_loop=5"])
    assert inference.read_switches(on, False).ss_nested == (0.25, 5)
    assert inference.read_switches(parse_overrides(["data.ss_model_path=w.pt"]), False).ss_nested is None
    with pytest.raises(ValueError, match="RNAMSM_GATHER_TO_RANK0"):
        inference.read_switches(on, True)


def test_write_nested_files_from_device_bodies_and_on_the_host(program, tmp_path):
    prob, seq = C.random_sigmoid(35, 11, 0.5), C.seq_for(35, 11)
    (partner, counts, ct, bp, dbn), = _decode(program, tmp_path, [(prob, seq, 0.516, 3)])
    assert counts[0] >= 3
    pad = lambda b, n: np.frombuffer(b + b"\xff" * (n - len(b)), dtype=np.uint8)      # noqa: E731
    path = ss.write_nested_files(seq, "x", tmp_path / "a", partner, counts, pad(ct, 32 * 35), pad(bp, 12 * 35), np.frombuffer(dbn, dtype=np.uint8))
    out = tmp_path / "a" / "SS_result"
    assert path == str(out / "x.dbn") and sorted(f.name for f in out.iterdir()) == ["x.dbn", "x.nested.bpseq", "x.nested.ct"]
    want = {"x.dbn": f">x\n{seq}\n".encode() + dbn + b"\n", "x.nested.ct": f"35\t\tx\t\tRNAMSM_SS output\n\n".encode() + ct,
            "x.nested.bpseq": b"#x\n" + bp}
    assert {f.name: f.read_bytes() for f in out.iterdir()} == want
    bad = counts.copy()
    bad[3] = 1                                                     # the fallback word: the tables and the brackets come from the partner vector
    junk = np.full(32 * 35, ord("?"), dtype=np.uint8)
    ss.write_nested_files(seq, "x", tmp_path / "b", partner, bad, junk, junk[:12 * 35], junk[:35])
    assert {f.name: f.read_bytes() for f in (tmp_path / "b" / "SS_result").iterdir()} == want
    with pytest.raises(ValueError):
        ss.write_nested_files(seq, "x", tmp_path / "c", partner[:-1], counts, ct, bp, dbn)
    with pytest.raises(ValueError):
        ss.write_nested_files(seq, "x", tmp_path / "c", partner, counts[:4], ct, bp, dbn)


def test_the_record_carries_the_nested_results_in_a_trailing_field():
    rec = ss.SSResult(None, None)
    assert rec.nested is None and ss.SSResult._fields[-1] == "nested" and ss.SSResult._fields[:4] == ("probs", "tokens", "text", "structure")


# ---------------------------------------------------------------------- write_dbn
def test_write_dbn_bytes(tmp_path):
    path = ss.write_dbn("x1", "ACGUNACGU", "((.....))", tmp_path)
    assert path == str(tmp_path / "SS_result" / "x1.dbn")
    assert open(path, "rb").read() == b">x1\nACGUNACGU\n((.....))\n"
    ss.write_dbn("x2", "ACG-U", np.frombuffer(b"(...)", dtype=np.uint8), tmp_path)
    assert (tmp_path / "SS_result" / "x2.dbn").read_bytes() == b">x2\nACG-U\n(...)\n"
    ss.write_dbn("x3", "AC", b"..", tmp_path)
    assert (tmp_path / "SS_result" / "x3.dbn").read_bytes() == b">x3\nAC\n..\n"
    for bad in ("(..", "(.[.]", "(...)x"):
        with pytest.raises(ValueError):
            ss.write_dbn("x4", "ACGUA", bad, tmp_path)
    assert ss.dbn_from_partner([9, 8, 0, 0, 0, 0, 0, 2, 1]) == "((.....))"
    assert T.partner_from_dbn("((.....))").tolist() == [9, 8, 0, 0, 0, 0, 0, 2, 1]
