"""Long alignments: the window plan.

An alignment of L > W body columns (W = max_seqlen - 1: the learned positional table ends there) runs as overlapping windows of
exactly W columns, and the windows' outputs are blended on the device (rnamsm_stitch_rows / rnamsm_stitch_pairs, ops.stitch_*).
This module is the host's side of it: where the windows start, and -- for documentation and host-side checks only, the product
blends on the device -- the blend weight of a window at a local column.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np


def default_stride(W: int) -> int:
    """ceil(W / 2): every column but the ends lies in two windows."""
    return (int(W) + 1) // 2


def check_stride(W: int, stride: int) -> int:
    lo = default_stride(W)
    if not lo <= stride <= W:
        raise ValueError(f"window stride {stride} outside [ceil(W / 2), W] = [{lo}, {W}] for windows of W = {W} columns")
    return int(stride)


def plan_windows(L: int, W: int, stride: int) -> List[Tuple[int, bool, bool]]:
    """(start, is_first, is_last) of the n = ceil((L - W) / stride) + 1 windows of an alignment of L > W body columns: window k
    starts at k * stride, the last one at L - W, so every window is W wide and the last one is right-aligned."""
    L, W, stride = int(L), int(W), int(stride)
    if W < 1 or L <= W:
        raise ValueError(f"plan_windows: L = {L} must exceed W = {W} >= 1 (a shorter alignment is one forward)")
    check_stride(W, stride)
    n = -(-(L - W) // stride) + 1
    starts = [k * stride for k in range(n - 1)] + [L - W]
    return [(s, k == 0, k == n - 1) for k, s in enumerate(starts)]


def blend_weights(W: int, stride: int, is_first: bool, is_last: bool) -> np.ndarray:
    """u(i), i in [0, W), float32: 1 where ramp = W - stride is 0, else min(left, right, ramp) / ramp in fp32, left = ramp in the
    first window, else i + 1, right = ramp in the last window, else W - i."""
    check_stride(W, stride)
    ramp = W - stride
    if ramp == 0:
        return np.ones(W, dtype=np.float32)
    i = np.arange(W, dtype=np.int64)
    left = np.full(W, ramp, dtype=np.int64) if is_first else i + 1
    right = np.full(W, ramp, dtype=np.int64) if is_last else W - i
    m = np.minimum(np.minimum(left, right), ramp)
    return m.astype(np.float32) / np.float32(ramp)
