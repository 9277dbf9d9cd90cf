"""The device stitcher (rnamsm_stitch_rows / rnamsm_stitch_pairs) against the numpy fp32 model of tests/windows_truth.py, BIT FOR
BIT: every operation of the stitch is one correctly rounded fp32 multiply, add or divide in a fixed order, so equality is the
derived bar and no tolerance applies.  Windows are applied one call each (a one-by-one run) and all in one call (a batched forward),
read through strides wider than their extent; outputs are prefilled with NaN and must come back fully defined, uncovered pairs as
+0.0; a NaN and an inf planted in one window reach exactly what that window covers; refusals enqueue nothing.

Past one 256-column tile of stitch_pairs_kernel (the second half of this file): plans of two to four q tiles with a ragged last one,
the shipped width W = 1023 up to L = 4096, rows at D beside and beyond 256 and at the length limit L = 2^19, every way to cut a
plan's windows into consecutive calls -- the truth does not depend on the cut, and between calls the elements of later windows
still hold their prefill -- and plane counts at which a block walks one plane and another two."""
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


# ---- past one 256-column tile ---------------------------------------------------------------------------------------------------
Q_TILE = 256                              # stitch.hip: a block of stitch_pairs_kernel is one row and 256 consecutive columns
# L on both sides of 256 and of 512, three and four tiles with a ragged last one; all three-fold covered at the right end
TILE_PLANS = [(256, 160, 80), (257, 160, 80), (300, 160, 80), (511, 256, 128), (513, 256, 128), (769, 300, 150)]
# (L, W, stride, H): the shipped window, its default stride, and once stride = W (ramp 0: no division); L = W + 1, five windows'
# worth of tiles, and the long heads' limit (one plane there: the output alone is 67 MB)
SHIPPED = [(1024, 1023, 512, 2), (2100, 1023, 512, 2), (4096, 1023, 512, 1), (2100, 1023, 1023, 2)]
PERIOD = 1000003                          # a prime: no tile, window or plane size divides it


def _many_values(shape, seed):
    """_values; above PERIOD elements, PERIOD drawn values repeated (the draw, not the kernel, is what takes time there)."""
    size = int(np.prod(shape))
    return _values(shape, seed) if size <= PERIOD else np.resize(_values((PERIOD,), seed), shape)


def _fold(L, W, stride):
    """How many windows contain each column."""
    cover = np.zeros(L, int)
    for s in T.starts(L, W, stride):
        cover[s:s + W] += 1
    return cover


def _first_window(L, W, stride):
    """int [L]: the first window of the plan that contains each column."""
    first = np.full(L, -1)
    for k, s in reversed(list(enumerate(T.starts(L, W, stride)))):
        first[s:s + W] = k
    assert (first >= 0).all()
    return first


def _cuts(n):
    """Every way to cut the windows 0 .. n - 1 into consecutive calls, as lists of call sizes: 2^(n-1) of them."""
    out = []
    for bits in range(1 << (n - 1)):
        sizes = [1]
        for k in range(n - 1):
            if bits >> k & 1:
                sizes.append(1)
            else:
                sizes[-1] += 1
        out.append(sizes)
    assert len(out) == 1 << (n - 1) and all(sum(c) == n for c in out) and [n] in out and [1] * n in out
    return out


def _rows_source(xs_host, strided):
    n, (W, D) = len(xs_host), xs_host[0].shape
    if strided:                                                   # rows inside a wider buffer, windows further apart
        x = torch.full((n, W + 2, D + 5), float("nan"), device=DEV)[:, 1:W + 1, 2:2 + D]
    else:
        x = torch.empty(n, W, D, device=DEV)
    x.copy_(torch.from_numpy(np.stack(xs_host)))
    return x


def _pairs_source(maps_host, with_cls, spare=0):
    """The windows' maps on the device -> (a, off); with_cls: the offset form with padded rows and planes; spare: that many more
    planes in the buffer than the stack uses, so that windows lie further apart than H planes."""
    n, (H, W, _) = len(maps_host), maps_host[0].shape
    m = torch.from_numpy(np.stack(maps_host)).to(DEV)
    if with_cls:
        a = torch.full((n, H + spare, W + 1, W + 3), float("nan"), device=DEV)[:, :H, :, :W + 1]
        a[:, :, 1:, 1:] = m
        return a, 1
    if spare:
        a = torch.full((n, H + spare, W, W), float("nan"), device=DEV)[:, :H]
        a.copy_(m)
        return a, 0
    return m, 0


def _in_calls(fn, src, out, stride, sizes, between=None, **kw):
    """The windows src[0 .. n) applied to `out` in consecutive calls of the given sizes, ascending; between(k) runs after every call
    but the last, k = the last window applied so far."""
    k0 = 0
    for nb in sizes:
        fn(src[k0:k0 + nb], out, stride, k0, **kw)
        k0 += nb
        if between is not None and k0 < src.shape[0]:
            between(k0 - 1)
    assert k0 == src.shape[0]
    return out


def _both_routes(fn, src, shape, stride, **kw):
    """One call per window and one call for all -> two host arrays."""
    n = src.shape[0]
    return tuple(_in_calls(fn, src, _garbage(shape), stride, sizes, **kw).cpu().numpy() for sizes in ([1] * n, [n]))


def _check_pairs(maps, want, covered, stride, with_cls, spare=0):
    a, off = _pairs_source(maps, with_cls, spare)
    for got in _both_routes(ops.stitch_pairs, a, want.shape, stride, off=off):
        assert not np.isnan(got).any()                                             # fully defined
        assert _same_bits(got, want), (with_cls, spare)
        assert (got.view(np.uint32)[:, ~covered] == 0).all()                       # +0.0: every bit, the sign included


@pytest.mark.parametrize("L,W,stride", TILE_PLANS)
def test_pairs_across_q_tiles(L, W, stride):
    assert [-(-p[0] // Q_TILE) for p in TILE_PLANS] == [1, 2, 2, 2, 3, 4]          # q tiles: the last one ragged wherever there are two
    assert -(-L // Q_TILE) >= 2 or (L, W, stride) == TILE_PLANS[0]
    assert _fold(L, W, stride).max() == 3 and _fold(L, W, stride)[T.starts(L, W, stride)[-1]] == 3
    n = len(T.starts(L, W, stride))
    covered = T.covered_pairs(L, W, stride)
    assert not covered.all()
    for H in (1, 3):
        maps = [_values((H, W, W), 1000 * k + H) for k in range(n)]
        want = T.stitch_pairs(maps, L, W, stride)
        for with_cls in (False, True):
            _check_pairs(maps, want, covered, stride, with_cls)


@pytest.mark.parametrize("L,W,stride,H", SHIPPED)
def test_pairs_at_the_shipped_width(L, W, stride, H):
    st = T.starts(L, W, stride)
    n = len(st)
    covered = T.covered_pairs(L, W, stride)
    if L == 1024:
        # L = W + 1: two windows one column apart; every pair is covered but the two corners (0, L - 1) and (L - 1, 0)
        assert st == [0, 1] and (~covered).sum() == 2 and not covered[0, L - 1] and not covered[L - 1, 0]
    if L == 4096:
        assert n == 8 and _fold(L, W, stride).max() == 3 and 0.65 < 1 - covered.mean() < 0.67
    base = _many_values((n, H, W, W), L + stride)
    maps = [base[k] for k in range(n)]
    want = T.stitch_pairs(maps, L, W, stride)
    for with_cls in (False, True):
        _check_pairs(maps, want, covered, stride, with_cls)


@pytest.mark.parametrize("L,W,stride", TILE_PLANS + sorted({p[:3] for p in SHIPPED}))
def test_rows_at_the_same_plans(L, W, stride):
    """D = 1, across the 256 threads of a block (257, 300), the shipped 768, and 1000: three passes and a ragged fourth."""
    n = len(T.starts(L, W, stride))
    assert _lib.load().rnamsm_stitch_num_windows(L, W, stride) == n
    base = _many_values((n, W, 1000), L + W)
    for D in (1, 257, 300, 768, 1000):
        xs = [base[k, :, :D] for k in range(n)]
        want = T.stitch_rows(xs, L, W, stride)
        for strided in (False, True):
            for got in _both_routes(ops.stitch_rows, _rows_source(xs, strided), (L, D), stride):
                assert not np.isnan(got).any()
                assert _same_bits(got, want), (D, strided)


CUT_PLANS = [(p, None) for p in TILE_PLANS + [(70, 32, 16), (13, 5, 3)]] + [((2100, 1023, 512), [[2, 2], [1, 2, 1], [3, 1]])]


@pytest.mark.parametrize("plan,cuts", CUT_PLANS, ids=["-".join(map(str, p[0])) for p in CUT_PLANS])
def test_every_grouping_of_the_windows_into_calls_gives_the_same_bits(plan, cuts):
    """A call applies the windows k0 .. k0 + nb - 1: any ascending cut of 0 .. n - 1 into calls gives the truth's bytes (compared on
    the device, as 32-bit integers), and after a call the elements whose windows all lie in later calls -- an uncovered pair's:
    the windows of its row -- still hold the NaN the output was prefilled with, while every other element is a number."""
    L, W, stride = plan
    D, H = 300, 3
    n = len(T.starts(L, W, stride))
    assert n <= 5
    cuts = cuts or _cuts(n)
    base_x, base_a = _many_values((n, W, D), 7 * L), _many_values((n, H, W, W), 11 * L)
    xs, maps = [base_x[k] for k in range(n)], [base_a[k] for k in range(n)]
    want_rows = torch.from_numpy(T.stitch_rows(xs, L, W, stride)).to(DEV).view(torch.int32)
    want_pairs = torch.from_numpy(T.stitch_pairs(maps, L, W, stride)).to(DEV).view(torch.int32)
    first = _first_window(L, W, stride)
    pair_first = np.where(T.covered_pairs(L, W, stride), np.maximum(first[:, None], first[None, :]), first[:, None])
    first_dev, pair_first_dev = torch.from_numpy(first).to(DEV), torch.from_numpy(pair_first).to(DEV)
    x = _rows_source(xs, True)
    sources = [_pairs_source(maps, with_cls) for with_cls in (False, True)]
    for sizes in cuts:
        out = _garbage((L, D))

        def rows_between(k):
            assert torch.equal(torch.isnan(out), (first_dev > k)[:, None].expand(L, D)), (sizes, k)
        _in_calls(ops.stitch_rows, x, out, stride, sizes, rows_between)
        assert torch.equal(out.view(torch.int32), want_rows), sizes
        for a, off in sources:
            out = _garbage((H, L, L))

            def pairs_between(k):
                assert torch.equal(torch.isnan(out), (pair_first_dev > k)[None].expand(H, L, L)), (sizes, off, k)
            _in_calls(ops.stitch_pairs, a, out, stride, sizes, pairs_between, off=off)
            assert torch.equal(out.view(torch.int32), want_pairs), (sizes, off)


@pytest.mark.parametrize("H", [8, 9, 12, 15, 16, 17])
def test_plane_walks_of_one_and_of_two_planes(H):
    """A block walks every 8th plane: at 8 < H < 16 some blocks of a launch walk two planes and the others one."""
    L, W, stride = 300, 160, 80
    n = len(T.starts(L, W, stride))
    covered = T.covered_pairs(L, W, stride)
    maps = [_values((H, W, W), 31 * k + H) for k in range(n)]
    want = T.stitch_pairs(maps, L, W, stride)
    for with_cls in (False, True):
        _check_pairs(maps, want, covered, stride, with_cls, spare=3)           # windows further apart than H planes


def test_a_nan_and_an_inf_at_two_tiles_reach_exactly_what_their_window_covers():
    L, W, stride, H, D = 513, 256, 128, 3, 64
    st = T.starts(L, W, stride)
    n = len(st)
    xs = [_values((W, D), k) for k in range(n)]
    maps = [_values((H, W, W), 50 + k) for k in range(n)]
    clean_rows, clean_pairs = T.stitch_rows(xs, L, W, stride), T.stitch_pairs(maps, L, W, stride)
    k, s = 1, st[1]
    assert s == 128
    xs[k][3, 7], xs[k][200, 9] = np.nan, np.inf
    maps[k][2, 3, 200], maps[k][0, 130, 4] = np.nan, np.inf                       # the NaN at q = 328, the inf at p = 258, q = 132
    assert s + 200 >= Q_TILE and s + 130 >= Q_TILE and s + 4 < Q_TILE
    want_rows, want_pairs = T.stitch_rows(xs, L, W, stride), T.stitch_pairs(maps, L, W, stride)
    # what the model must say first: one output element each, the one the planted element is blended into
    bad_rows = np.zeros((L, D), bool)
    bad_rows[s + 3, 7] = bad_rows[s + 200, 9] = True
    bad_pairs = np.zeros((H, L, L), bool)
    bad_pairs[2, s + 3, s + 200] = bad_pairs[0, s + 130, s + 4] = True
    assert (~np.isfinite(want_rows) == bad_rows).all() and (~np.isfinite(want_pairs) == bad_pairs).all()
    assert np.isnan(want_rows[s + 3, 7]) and want_rows[s + 200, 9] == np.inf
    assert np.isnan(want_pairs[2, s + 3, s + 200]) and want_pairs[0, s + 130, s + 4] == np.inf
    for got, want, clean, bad in (
            [(g, want_rows, clean_rows, bad_rows) for g in _rows_both_routes(xs, L, W, stride, True)]
            + [(g, want_pairs, clean_pairs, bad_pairs) for g in _pairs_both_routes(maps, L, W, stride, True)]):
        assert (np.isnan(got) == np.isnan(want)).all() and (np.isinf(got) == np.isinf(want)).all()
        assert (got[np.isinf(want)] == np.inf).all()
        assert (got.view(np.uint32)[~bad] == clean.view(np.uint32)[~bad]).all()     # every other element: the bits it has without them


@pytest.mark.parametrize("L,W,stride,D", [(1 << 19, (1 << 18) + 1, (1 << 17) + 1, 1), ((1 << 19) - 3, 300001, 150001, 2)])
def test_rows_at_the_length_limit(L, W, stride, D):
    assert L <= _lib.STITCH_MAX_L and (L == _lib.STITCH_MAX_L or D == 2)
    n = len(T.starts(L, W, stride))
    assert n == 3 and _lib.load().rnamsm_stitch_num_windows(L, W, stride) == n and _fold(L, W, stride).max() == 3
    xs = [_values((W, D), L % 1000 + k) for k in range(n)]
    want = T.stitch_rows(xs, L, W, stride)
    for strided in (False, True):
        for got in _both_routes(ops.stitch_rows, _rows_source(xs, strided), (L, D), stride):
            assert not np.isnan(got).any()
            assert _same_bits(got, want), strided
