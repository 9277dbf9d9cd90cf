"""The windowed forward's plan, weights and stitch restated in numpy fp32, independent of the product (rnamsm/windows.py, stitch.hip):
the oracle of tests/test_windows_host.py and of the GPU tests of the stitcher.

Every operation below is one numpy float32 ufunc -- a correctly rounded IEEE multiply, add or divide, never fused -- applied in the
order the issue states: per output element, over the windows that contain it in ascending order, starting from the first term; the
normalising sum in the same order; one division at the end.  A pair no window contains is +0.0."""
import numpy as np

F = np.float32


def starts(L, W, stride):
    n = -(-(L - W) // stride) + 1
    return [k * stride for k in range(n - 1)] + [L - W]


def weights_loop(W, stride, first, last):
    """u(i), i in [0, W), float32: the definition, one column at a time."""
    ramp = W - stride
    if ramp == 0:
        return np.ones(W, dtype=F)
    u = np.empty(W, dtype=F)
    for i in range(W):
        left = ramp if first else i + 1
        right = ramp if last else W - i
        u[i] = F(min(left, right, ramp)) / F(ramp)
    return u


def weights(W, stride, first, last):
    """u(i), i in [0, W), float32: weights_loop on whole arrays (a window of 2^18 columns takes the loop seconds) -- the same
    integers, converted to float32 exactly (ramp <= W < 2^24) and divided once; tests/test_windows_host.py holds the two equal."""
    ramp = W - stride
    if ramp == 0:
        return np.ones(W, dtype=F)
    i = np.arange(W, dtype=np.int64)
    m = np.full(W, ramp, dtype=np.int64)
    if not first:
        m = np.minimum(m, i + 1)
    if not last:
        m = np.minimum(m, W - i)
    return m.astype(F) / F(ramp)


def _accumulate(num, den, seen, term, w):
    """num / den [region] += term / w where the region was seen before, = where it was not."""
    num[...] = np.where(seen, num + term, term)
    den[...] = np.where(seen, den + w, w)
    seen[...] = True


def stitch_rows(xs, L, W, stride):
    """xs: the windows' [W, D] float32 arrays in plan order -> [L, D] float32."""
    st = starts(L, W, stride)
    assert len(xs) == len(st)
    D = xs[0].shape[1]
    num, den, seen = np.zeros((L, D), F), np.zeros((L, 1), F), np.zeros((L, 1), bool)
    with np.errstate(all="ignore"):
        for k, (s, x) in enumerate(zip(st, xs)):
            u = weights(W, stride, k == 0, k == len(st) - 1)[:, None]
            sl = slice(s, s + W)
            _accumulate(num[sl], den[sl], seen[sl], u * x.astype(F), u)
        assert seen.all()
        return num / den


def stitch_pairs(maps, L, W, stride):
    """maps: the windows' [H, W, W] float32 arrays in plan order -> [H, L, L] float32, +0.0 where no window holds the pair."""
    st = starts(L, W, stride)
    assert len(maps) == len(st)
    H = maps[0].shape[0]
    num, den, seen = np.zeros((H, L, L), F), np.zeros((1, L, L), F), np.zeros((1, L, L), bool)
    with np.errstate(all="ignore"):
        for k, (s, a) in enumerate(zip(st, maps)):
            u = weights(W, stride, k == 0, k == len(st) - 1)
            w = (u[:, None] * u[None, :])[None]
            sl = (slice(None), slice(s, s + W), slice(s, s + W))
            _accumulate(num[sl], den[sl], seen[sl], w * a.astype(F), w)
        out = np.zeros((H, L, L), F)
        np.divide(num, den, out=out, where=np.broadcast_to(seen, num.shape))
    return out


def covered_pairs(L, W, stride):
    """bool [L, L]: the pairs some window contains."""
    c = np.zeros((L, L), bool)
    for s in starts(L, W, stride):
        c[s:s + W, s:s + W] = True
    return c
