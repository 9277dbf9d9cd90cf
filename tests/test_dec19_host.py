"""csrc/dec19.h on the host: the 24 characters of "%.18e" for float32 values in [0, 1], computed in integers, against Python's own
`%` operator (the one np.savetxt formats with).  The header is compiled into a stand-alone program (tests/native/dec19_check.cpp)
with g++ and AddressSanitizer + UBSan, so an out-of-range table index or shift would stop it.  The program's `--all` mode (every
pattern of [0, 1] against snprintf) is not run here: DESIGN 3.8 records its result."""
import os
import shutil
import struct
import subprocess

import pytest

from conftest import ROOT
import dec19_cases as C

SRC = os.path.join(ROOT, "tests", "native", "dec19_check.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host check of dec19.h"
    exe = str(tmp_path_factory.mktemp("dec19") / "dec19_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    SRC, "-o", exe], check=True)
    return exe


def _expected(bits: int) -> str:
    return "%.18e" % struct.unpack("<f", struct.pack("<I", bits))[0]


def _run(program, patterns):
    res = subprocess.run([program], input="".join(f"{b:08x}\n" for b in patterns), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(patterns)
    return lines


def test_the_tie_set_is_what_the_issue_describes():
    t = C.ties()
    assert len(t) >= 20, len(t)
    assert C.bits_of(C.Fraction(1, 2 ** 28)) in t
    assert _expected(C.bits_of(C.Fraction(1, 2 ** 28))) == "3.725290298461914062e-09"       # half to even: ...0625 -> ...062


def test_special_values(program):
    vals = C.special_values()
    assert len(vals) > 1000
    got = _run(program, vals)
    bad = [(f"{b:08x}", g, _expected(b)) for b, g in zip(vals, got) if g != _expected(b)]
    assert not bad, (len(bad), bad[:5])
    assert got[vals.index(0)] == "0.000000000000000000e+00" and got[vals.index(C.ONE)] == "1.000000000000000000e+00"
    assert got[vals.index(C.bits_of(C.Fraction(1, 2 ** 28)))] == "3.725290298461914062e-09"


def test_random_patterns(program):
    vals = C.random_patterns()
    assert len(vals) == 1 << 16 and min(vals) >= 0 and max(vals) <= C.ONE
    got = _run(program, vals)
    bad = [(f"{b:08x}", g, _expected(b)) for b, g in zip(vals, got) if g != _expected(b)]
    assert not bad, (len(bad), bad[:5])


def test_a_pattern_outside_the_domain_is_refused_by_the_program(program):
    res = subprocess.run([program], input="3f800001\n", capture_output=True, text=True)
    assert res.returncode == 2
