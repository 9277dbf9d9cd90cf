"""Long alignments on the host: the window plan (rnamsm/windows.py), the blend weights, the numpy fp32 restatement of the stitch
(tests/windows_truth.py) on hand-made cases, data.long_msa in the configuration -- with the key off, crop_tokens and the random
stream behind it are what they were -- the new C-ABI symbols, and stitch_plan.h (the header the device stitcher computes its plan
with) against the same plans in a stand-alone program built with AddressSanitizer + UBSan."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import windows_truth as T
from rnamsm import _lib, windows
from rnamsm.config import Config, parse_overrides

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rnamsm_stitch_num_windows", "rnamsm_stitch_rows", "rnamsm_stitch_pairs")


def _cases():
    for W in range(1, 71):
        for stride in range((W + 1) // 2, W + 1):
            for L in range(W + 1, 3 * W + 6):
                yield L, W, stride


def test_plan_covers_every_column_with_windows_of_w_and_a_right_aligned_last_one():
    count = 0
    for L, W, stride in _cases():
        plan = windows.plan_windows(L, W, stride)
        st = np.array([s for s, _, _ in plan])
        n = -(-(L - W) // stride) + 1
        assert len(plan) == n >= 2, (L, W, stride)
        assert st[0] == 0 and st[-1] == L - W and (st[:-1] == stride * np.arange(n - 1)).all(), (L, W, stride)
        assert (np.diff(st) >= 1).all() and (np.diff(st) <= W).all(), (L, W, stride)      # ascending, no gap: every column is covered
        assert st[-1] + W == L and (st >= 0).all()                                        # all W wide, inside [0, L)
        assert [f for _, f, _ in plan] == [True] + [False] * (n - 1) and [l for _, _, l in plan] == [False] * (n - 1) + [True]
        assert list(st) == T.starts(L, W, stride)
        count += 1
    assert count > 100000


def test_coverage_is_counted_column_by_column_on_the_issue_example():
    plan = windows.plan_windows(70, 32, 16)
    assert [s for s, _, _ in plan] == [0, 16, 32, 38]
    cover = np.zeros(70, int)
    for s, _, _ in plan:
        cover[s:s + 32] += 1
    assert cover.min() == 1 and cover.max() == 3 and (cover[38:48] == 3).all()


@pytest.mark.parametrize("W", [1, 2, 5, 32, 33])
def test_inadmissible_strides_are_refused_with_the_bounds_in_the_message(W):
    lo = (W + 1) // 2
    for stride in (lo - 1, W + 1, 0, -3):
        with pytest.raises(ValueError, match=re.escape(f"[{lo}, {W}]")):
            windows.plan_windows(2 * W + 3, W, stride)
    with pytest.raises(ValueError):
        windows.plan_windows(W, W, W)                     # L must exceed W


def test_weights():
    for W in range(1, 71):
        for stride in range((W + 1) // 2, W + 1):
            ramp = W - stride
            first, mid, last = (windows.blend_weights(W, stride, f, l) for f, l in ((True, False), (False, False), (False, True)))
            for u, (f, l) in ((first, (True, False)), (mid, (False, False)), (last, (False, True))):
                assert u.dtype == np.float32 and u.tobytes() == T.weights(W, stride, f, l).tobytes()
                assert (u > 0).all() and (u <= 1).all()
            if ramp == 0:
                assert (first == 1).all() and (mid == 1).all() and (last == 1).all()
                continue
            assert (first[:stride] == 1).all()                              # the first window has no left ramp
            assert (last[W - stride:] == 1).all()                           # the last window has no right ramp
            assert mid[0] == np.float32(1) / np.float32(ramp) and mid[-1] == mid[0]
            assert (mid[ramp - 1:W - ramp + 1] == 1).all()                  # beyond both ramps
    # singly covered columns have u == 1, whatever the plan
    for L, W, stride in ((70, 32, 16), (41, 20, 13), (13, 5, 3), (11, 5, 5), (200, 33, 17)):
        st = T.starts(L, W, stride)
        cover = np.zeros(L, int)
        for s in st:
            cover[s:s + W] += 1
        for k, s in enumerate(st):
            u = windows.blend_weights(W, stride, k == 0, k == len(st) - 1)
            assert (u[cover[s:s + W] == 1] == 1).all(), (L, W, stride, k)


def test_the_vectorised_weights_of_the_truth_are_its_loop_byte_for_byte():
    """windows_truth.weights works on whole arrays so that the GPU tests can afford windows of 2^18 columns; weights_loop is the
    definition it restates.  Every (W, stride) of this file's plans, every position of the window in the plan, and the shipped
    width."""
    count = 0
    for W, stride in ([(W, s) for W in range(1, 71) for s in range((W + 1) // 2, W + 1)]
                      + [(1023, 512), (1023, 700), (1023, 1022), (1023, 1023), (4097, 2049)]):
        for first, last in ((True, False), (False, False), (False, True), (True, True)):
            u = T.weights(W, stride, first, last)
            assert u.dtype == np.float32 and u.shape == (W,)
            assert u.tobytes() == T.weights_loop(W, stride, first, last).tobytes(), (W, stride, first, last)
            count += 1
    assert count > 5000


def test_numpy_stitch_on_hand_computed_cases():
    # W = 2, stride = 1, L = 3: windows at 0 and 1, ramp 1 -> every weight is 1; column 1 is the plain mean of both windows
    xs = [np.array([[1.0], [3.0]], np.float32), np.array([[5.0], [7.0]], np.float32)]
    assert T.stitch_rows(xs, 3, 2, 1).tolist() == [[1.0], [4.0], [7.0]]
    maps = [np.array([[[1.0, 2.0], [3.0, 4.0]]], np.float32), np.array([[[10.0, 20.0], [30.0, 40.0]]], np.float32)]
    out = T.stitch_pairs(maps, 3, 2, 1)
    assert out.tolist() == [[[1.0, 2.0, 0.0], [3.0, 7.0, 20.0], [0.0, 30.0, 40.0]]]
    assert not np.signbit(out).any()
    # W = 4, stride = 2, L = 6: ramp 2; window 0 ends 1, 1/2 -- window 1 begins 1/2, 1: column 2 = (1 * a + 1/2 * b) / (3/2)
    xs = [np.full((4, 1), 3.0, np.float32), np.full((4, 1), 9.0, np.float32)]
    got = T.stitch_rows(xs, 6, 4, 2)[:, 0]
    assert got[0] == got[1] == 3 and got[4] == got[5] == 9
    assert got[2] == np.float32(np.float32(3 + 4.5) / np.float32(1.5)) and got[3] == np.float32(np.float32(1.5 + 9) / np.float32(1.5))
    # stride = W: nothing overlaps but at the right-aligned last window
    xs = [np.full((3, 2), float(k + 1), np.float32) for k in range(3)]
    assert T.stitch_rows(xs, 7, 3, 3)[:, 0].tolist() == [1, 1, 1, 2, 2.5, 2.5, 3]
    assert T.covered_pairs(7, 3, 3).sum() == 9 + 9 + 9 - 4                     # three 3 x 3 blocks, 4 pairs shared by the last two
    # a NaN in one window reaches the outputs that window covers and no others; -0.0 of a lone window keeps its sign
    xs = [np.zeros((4, 1), np.float32), np.zeros((4, 1), np.float32)]
    xs[0][3, 0], xs[0][0, 0] = np.nan, -0.0
    got = T.stitch_rows(xs, 6, 4, 2)[:, 0]
    assert np.isnan(got).tolist() == [False, False, False, True, False, False] and np.signbit(got[0])


def test_config_default_is_the_crop_and_other_values_are_refused():
    cfg = Config()
    assert cfg.data.long_msa == "crop" and cfg.data.window_stride == 0
    assert parse_overrides(["data.long_msa=windows", "data.window_stride=700"]).data.window_stride == 700
    assert parse_overrides(["data.long_msa=crop"]).data.long_msa == "crop"
    with pytest.raises(ValueError, match="long_msa"):
        parse_overrides(["data.long_msa=nonsense"])


def test_with_the_key_off_the_crop_and_its_random_stream_are_unchanged():
    from rnamsm.inference import crop_tokens
    tokens = np.arange(3 * 2000, dtype=np.int64).reshape(3, 2000)
    rng, ref = np.random.RandomState(42), np.random.RandomState(42)
    got = crop_tokens(tokens, 1024, rng)
    start = ref.randint(1, 2000 - 1024)                                      # RandomCropDataset (dataset.py:147)
    assert got.shape == (3, 1024) and (got[:, 0] == tokens[:, 0]).all() and (got[:, 1:] == tokens[:, start:start + 1023]).all()
    assert crop_tokens(tokens[:, :1024], 1024, rng) is not None and rng.randint(1 << 30) == ref.randint(1 << 30)   # narrow: no draw
    # the whole state, not one draw: a fresh pair of streams after the same calls
    a, b = np.random.RandomState(42), np.random.RandomState(42)
    crop_tokens(tokens, 1024, a)
    b.randint(1, 2000 - 1024)
    sa, sb = a.get_state(), b.get_state()
    assert sa[0] == sb[0] and (sa[1] == sb[1]).all() and sa[2:] == sb[2:]


def test_the_new_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnamsm.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\b(rnamsm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header, flags=re.S))
    lib = _lib.load()
    for name in NEW:
        assert name in protos and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert len(protos[name].split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert re.search(rf"#define RNAMSM_STITCH_MAX_L \(1 << 19\)", header) and _lib.STITCH_MAX_L == 1 << 19
    assert re.search(rf"#define RNAMSM_STITCH_MAX_H \(1 << 16\)", header) and _lib.STITCH_MAX_H == 1 << 16
    assert "#define RNAMSM_VERSION 600" in header and lib.rnamsm_version() == 600
    # the plan as the library counts it (host code: no device needed)
    assert lib.rnamsm_stitch_num_windows(70, 32, 16) == 4 and lib.rnamsm_stitch_num_windows(1500, 1023, 512) == 2
    assert lib.rnamsm_stitch_num_windows(32, 32, 16) == 0 and lib.rnamsm_stitch_num_windows(70, 32, 15) == 0
    assert lib.rnamsm_stitch_num_windows(70, 32, 33) == 0 and lib.rnamsm_stitch_num_windows((1 << 19) + 1, 32, 16) == 0


def test_stitch_plan_header_under_sanitizers(tmp_path):
    """stitch_plan.h on the host: every plan of W <= 24, the shipped width up to L = 4096 and the plans at the length limit 2^19
    against a brute-force restatement inside the program, and a few hand-computed plans and weights given on the command line."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host check of stitch_plan.h"
    exe = str(tmp_path / "stitch_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "stitch_plan_check.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
    assert "plans ok" in res.stdout
    # the weights the program prints for (L, W, stride) are the numpy model's bits
    for L, W, stride in ((70, 32, 16), (13, 5, 3), (200, 33, 17), (2100, 1023, 512), (1535, 1023, 700),
                         (1 << 19, (1 << 18) + 1, (1 << 17) + 1), ((1 << 19) - 3, 300001, 150001)):
        res = subprocess.run([exe, str(L), str(W), str(stride)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        lines = res.stdout.split()
        st = T.starts(L, W, stride)
        want = [f"{s}" for s in st] + [f"{b:08x}" for k in range(len(st))
                                        for b in T.weights(W, stride, k == 0, k == len(st) - 1).view(np.uint32)]
        assert lines == want, (L, W, stride)
