"""The device stitcher (rnamsm_stitch_rows / rnamsm_stitch_pairs) against the numpy fp32 model of tests/windows_truth.py, BIT FOR
BIT: every operation of the stitch is one correctly rounded fp32 multiply, add or divide in a fixed order, so equality is the
derived bar and no tolerance applies.  Windows are applied one call each (a one-by-one run) and all in one call (a batched forward),
read through strides wider than their extent; outputs are prefilled with NaN and must come back fully defined, uncovered pairs as
+0.0; a NaN and an inf planted in one window reach exactly what that window covers; refusals enqueue nothing."""
import ctypes

import numpy as np
import pytest
import torch

import windows_truth as T
from rnamsm import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _plans():
    seen = []
    for W in (1, 2, 5, 32, 33, 64, 65):
        for stride in ((W + 1) // 2, W - 1, W):
            if not (W + 1) // 2 <= stride <= W:
                continue
            for L in (W + 1, W + stride, 2 * W + 3):
                if (L, W, stride) not in seen:
                    seen.append((L, W, stride))
    seen.append((70, 32, 16))            # three-fold coverage near the right end
    return seen


PLANS = _plans()


def _values(shape, seed):
    rng = np.random.RandomState(seed)
    x = (rng.standard_normal(shape) * np.exp(rng.uniform(-3, 3, shape))).astype(np.float32)
    x.reshape(-1)[::17] = -0.0                                    # signed zeros travel too
    return x


def _same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    return got.tobytes() == want.tobytes()


def _garbage(shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def _rows_both_routes(xs_host, L, W, stride, strided):
    """The stitched rows after one call per window and after one call for all -> two host arrays."""
    n, D = len(xs_host), xs_host[0].shape[1]
    if strided:                                                   # rows inside a wider buffer, windows further apart
        buf = torch.full((n, W + 2, D + 5), float("nan"), device=DEV)
        x = buf[:, 1:W + 1, 2:2 + D]
    else:
        x = torch.empty(n, W, D, device=DEV)
    x.copy_(torch.from_numpy(np.stack(xs_host)))
    one = _garbage((L, D))
    for k in range(n):
        ops.stitch_rows(x[k:k + 1], one, stride, k)
    many = ops.stitch_rows(x, _garbage((L, D)), stride, 0)
    return one.cpu().numpy(), many.cpu().numpy()


def _pairs_both_routes(maps_host, L, W, stride, with_cls):
    n, H = len(maps_host), maps_host[0].shape[0]
    if with_cls:                  # the offset / row-stride / plane-stride form: maps that still carry a <cls> row and column
        buf = torch.full((n, H, W + 1, W + 3), float("nan"), device=DEV)
        a, off = buf[:, :, :, :W + 1], 1
        a[:, :, 1:, 1:] = torch.from_numpy(np.stack(maps_host)).to(DEV)
    else:
        a, off = torch.from_numpy(np.stack(maps_host)).to(DEV), 0
    one = _garbage((H, L, L))
    for k in range(n):
        ops.stitch_pairs(a[k:k + 1], one, stride, k, off)
    many = ops.stitch_pairs(a, _garbage((H, L, L)), stride, 0, off)
    return one.cpu().numpy(), many.cpu().numpy()


@pytest.mark.parametrize("L,W,stride", PLANS)
def test_rows_are_the_fp32_model_bit_for_bit(L, W, stride):
    n = len(T.starts(L, W, stride))
    assert _lib.load().rnamsm_stitch_num_windows(L, W, stride) == n
    for D in (3, 64, 768):
        xs = [_values((W, D), 100 * k + D) for k in range(n)]
        want = T.stitch_rows(xs, L, W, stride)
        for strided in (False, True):
            one, many = _rows_both_routes(xs, L, W, stride, strided)
            assert not np.isnan(one).any() and not np.isnan(many).any()           # fully defined
            assert _same_bits(one, want) and _same_bits(many, want), (D, strided)


@pytest.mark.parametrize("L,W,stride", PLANS)
def test_pairs_are_the_fp32_model_bit_for_bit(L, W, stride):
    n = len(T.starts(L, W, stride))
    covered = T.covered_pairs(L, W, stride)
    for H in (1, 3):
        maps = [_values((H, W, W), 1000 * k + H) for k in range(n)]
        want = T.stitch_pairs(maps, L, W, stride)
        for with_cls in (False, True):
            one, many = _pairs_both_routes(maps, L, W, stride, with_cls)
            assert not np.isnan(one).any() and not np.isnan(many).any()
            assert _same_bits(one, want) and _same_bits(many, want), (H, with_cls)
            assert (one.view(np.uint32)[:, ~covered] == 0).all()                   # +0.0: every bit, the sign included


def test_pairs_of_120_planes():
    L, W, stride, H = 13, 5, 3, 120
    maps = [_values((H, W, W), k) for k in range(len(T.starts(L, W, stride)))]
    want = T.stitch_pairs(maps, L, W, stride)
    for with_cls in (False, True):
        one, many = _pairs_both_routes(maps, L, W, stride, with_cls)
        assert _same_bits(one, want) and _same_bits(many, want)


def test_a_nan_and_an_inf_reach_exactly_what_their_window_covers():
    L, W, stride, H, D = 70, 32, 16, 3, 64
    st = T.starts(L, W, stride)
    n = len(st)
    xs = [_values((W, D), k) for k in range(n)]
    maps = [_values((H, W, W), 50 + k) for k in range(n)]
    clean_rows, clean_pairs = T.stitch_rows(xs, L, W, stride), T.stitch_pairs(maps, L, W, stride)
    k, s = 1, st[1]
    xs[k][3, 7], xs[k][20, 9] = np.nan, np.inf
    maps[k][2, 3, 30], maps[k][0, 25, 4] = np.nan, np.inf
    want_rows, want_pairs = T.stitch_rows(xs, L, W, stride), T.stitch_pairs(maps, L, W, stride)
    # what the model must say first: one output element each, the one the planted element is blended into
    bad_rows = np.zeros((L, D), bool)
    bad_rows[s + 3, 7] = bad_rows[s + 20, 9] = True
    bad_pairs = np.zeros((H, L, L), bool)
    bad_pairs[2, s + 3, s + 30] = bad_pairs[0, s + 25, s + 4] = True
    assert (~np.isfinite(want_rows) == bad_rows).all() and (~np.isfinite(want_pairs) == bad_pairs).all()
    assert np.isnan(want_rows[s + 3, 7]) and want_rows[s + 20, 9] == np.inf
    assert np.isnan(want_pairs[2, s + 3, s + 30]) and want_pairs[0, s + 25, s + 4] == np.inf
    for got, want, clean, bad in (
            [(g, want_rows, clean_rows, bad_rows) for g in _rows_both_routes(xs, L, W, stride, True)]
            + [(g, want_pairs, clean_pairs, bad_pairs) for g in _pairs_both_routes(maps, L, W, stride, True)]):
        assert (np.isnan(got) == np.isnan(want)).all() and (np.isinf(got) == np.isinf(want)).all()
        assert (got[np.isinf(want)] == np.inf).all()
        assert (got.view(np.uint32)[~bad] == clean.view(np.uint32)[~bad]).all()     # every other element: the bits it has without them


def test_refusals_return_invalid_and_enqueue_nothing():
    lib = _lib.load()
    L, W, stride, D, H = 70, 32, 16, 8, 2
    x = torch.ones(4, W, D, device=DEV)
    a = torch.ones(4, H, W, W, device=DEV)
    out_r, out_p = torch.full((L, D), 5.0, device=DEV), torch.full((H, L, L), 5.0, device=DEV)
    s = torch.cuda.current_stream().cuda_stream

    def rows(xp=x.data_ptr(), op=out_r.data_ptr(), L=L, W=W, stride=stride, k0=0, nb=4, D=D, ld=D, ws=W * D):
        return lib.rnamsm_stitch_rows(xp, ws, ld, L, W, stride, k0, nb, D, op, s)

    def pairs(ap=a.data_ptr(), op=out_p.data_ptr(), L=L, W=W, stride=stride, k0=0, nb=4, H=H, ld=W, ps=W * W, ws=H * W * W, off=0):
        return lib.rnamsm_stitch_pairs(ap, ws, ps, ld, off, L, W, stride, k0, nb, H, op, s)

    bad = [rows(xp=None), rows(op=None), rows(L=W), rows(L=W - 1), rows(stride=15), rows(stride=33), rows(stride=0), rows(k0=1, nb=4),
           rows(nb=0), rows(k0=-1), rows(D=0), rows(ld=D - 1), rows(ws=W * D - 1), rows(xp=x.data_ptr() + 2), rows(L=(1 << 19) + 1),
           pairs(ap=None), pairs(op=None), pairs(L=W), pairs(stride=15), pairs(stride=33), pairs(k0=4, nb=1), pairs(H=0),
           pairs(ld=W - 1), pairs(ps=W * W - 1), pairs(ws=H * W * W - 1), pairs(off=-1), pairs(off=1), pairs(op=out_p.data_ptr() + 1)]
    assert bad == [-1] * len(bad)
    assert pairs(stride=15) == -1 and "[16, 32]" in lib.rnamsm_last_error().decode()      # the message names the bounds
    torch.cuda.synchronize()
    assert (out_r == 5.0).all() and (out_p == 5.0).all()                                  # nothing was enqueued
    with pytest.raises(_lib.RnamsmError, match=r"\[16, 32\]"):
        ops.stitch_rows(x, out_r, 15)
    assert rows() == 0 and pairs() == 0                                                   # and the same calls, valid, run
    torch.cuda.synchronize()
    assert torch.isfinite(out_r).all() and torch.isfinite(out_p).all()
