"""The tail of the structure decoders without a GPU.  csrc/struct_text.h -- who owns which bases, measure_lines, the packed sums,
put_lines -- is compiled into a stand-alone program (tests/native/struct_text_check.cpp) with g++ and AddressSanitizer + UBSan.  For
every block size in use it runs the tail serially over the "threads", on heap buffers of exactly the announced sizes, and compares
with a single pass over all bases; the single pass's bytes are compared here with Python's own formatting.  The lengths are the
digit edges and the ownership edges; the partner vectors are: nobody paired, a seeded nested structure with the pair (1, L), and
every base with a partner of the most digits."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rnamsm import ss
import ss_nested_truth as T
import struct_text_cases as S

SRC = os.path.join(ROOT, "tests", "native", "struct_text_check.cpp")
LENGTHS = (1, 2, 9, 10, 11, 99, 100, 101, 999, 1000, 1001, 1023, 1024, 1025, 4095, 4096)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host check of struct_text.h"
    exe = str(tmp_path_factory.mktemp("struct_text") / "struct_text_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    SRC, "-o", exe], check=True)
    return exe


def _cases():
    out = []
    for L in LENGTHS:
        letters = S.letters_for(L, L)
        marked = letters.copy()
        marked[L // 2] = 0xC3                                   # a letter for the host writer: the fallback word
        nested = S.nested_partner(L, L)
        assert (L <= 4) == (nested[0] == 0) and (L <= 4 or nested[0] == L)
        out += [(np.zeros(L, dtype=np.int32), letters), (nested, letters), (S.widest_partner(L), marked)]
    return out


def test_threads_and_single_pass_write_the_bytes_python_formats(program, tmp_path):
    cases = _cases()
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for partner, letters in cases:
            f.write(np.int32(len(partner)).tobytes() + letters.tobytes() + partner.astype(np.int32).tobytes())
    res = subprocess.run([program, str(src), str(dst)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    blob, at = dst.read_bytes(), 0
    for partner, letters in cases:
        L = len(partner)
        want_ct, want_bp = S.bodies(partner, letters)
        counts = np.frombuffer(blob, dtype=np.int32, count=4, offset=at).tolist()
        assert counts == [S.pairs(partner), len(want_ct), len(want_bp), int((letters >= 128).any())], L
        at += 16
        assert blob[at:at + counts[1]] == want_ct and blob[at + counts[1]:at + counts[1] + counts[2]] == want_bp, L
        at += counts[1] + counts[2]
    assert at == len(blob)
    # the longest lines there can be are among them
    ct, bp = S.bodies(S.widest_partner(4096), S.letters_for(4096, 4096))
    assert max(map(len, ct.split(b"\n"))) + 1 == 32 and max(map(len, bp.split(b"\n"))) + 1 == 12


@pytest.mark.parametrize("L", (1, 63, 64, 65, 1000))
def test_a_planted_structure_is_what_both_decodings_return(L):
    """The precondition of tests/test_gpu_struct_text.py, at the sizes where the truth is cheap: one pair per base, so the
    multiplet removal takes nothing away; every weight positive and every pair compatible, so the nested optimum is the planted set."""
    partner = S.nested_partner(L, L)
    prob = S.planted_probs(partner)
    assert ss.pairs_from_partner(partner) == ss.secondary_structure(prob)
    assert T.decode(prob)[0].tolist() == partner.tolist()
