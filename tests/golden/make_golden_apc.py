#!/usr/bin/env python3
"""Generates tests/golden/apc_reference_l9.npz with the reference's own apc (utils/tensor.py:103-113; needs the reference tree, see
_refimport -- at generation time only; nothing under tests/ imports it at test time).

  x_general     a 9 x 9 float64 map, not symmetric, positive
  apc_general   utils.tensor.apc(x_general), float64 [9, 9]
  x_symmetric   a symmetric 9 x 9 float64 map with a zero diagonal (the shape of a mutual-information map)
  apc_symmetric utils.tensor.apc(x_symmetric)

Run:  python tests/golden/make_golden_apc.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def main():
    from _refimport import install
    install()
    from utils.tensor import apc
    rng = np.random.RandomState(103)
    x_general = rng.rand(9, 9) + 0.05
    half = rng.rand(9, 9) ** 2
    x_symmetric = half + half.T
    np.fill_diagonal(x_symmetric, 0.0)
    out = os.path.join(HERE, "apc_reference_l9.npz")
    got = {}
    for name, x in (("general", x_general), ("symmetric", x_symmetric)):
        y = np.asarray(apc(x))
        assert y.dtype == np.float64 and y.shape == (9, 9), (y.dtype, y.shape)
        got["x_" + name], got["apc_" + name] = x, y
    np.savez(out, **got)
    print(f"wrote {out}: " + ", ".join(f"{k} {v.shape}" for k, v in got.items()))


if __name__ == "__main__":
    main()
