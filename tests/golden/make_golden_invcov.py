#!/usr/bin/env python3
"""Generates tests/golden/invcov_reference_n12_l9.npz with the reference's own MSA.invcov (utils/align.py:183-193; needs the
reference tree, see _refimport, and scikit-learn -- at generation time only; nothing under tests/ imports them at test time).

  sequences  the 12 aligned sequences of 9 columns over A C G U and '-', as text
  tokens     the same as uint8 token ids [12, 9] (A4 G5 C6 U7 -10)
  invcov     MSA.from_sequences(sequences).invcov(), float64 [9, 9]

Run:  python tests/golden/make_golden_invcov.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "..", "rna-msm_amd"))


def main():
    from _refimport import reference_modules
    from rnamsm.alphabet import RNAAlphabet
    MSA = reference_modules()[4]
    rng = np.random.RandomState(183)
    founders = rng.randint(0, 4, size=(2, 9))
    body = founders[rng.randint(0, 2, size=12)]
    flip = rng.rand(12, 9) < 0.2
    body[flip] = rng.randint(0, 4, size=int(flip.sum()))
    chars = np.array(list("ACGU-"))[np.where(rng.rand(12, 9) < 0.1, 4, body)]
    chars[:, 4] = chars[0, 4] if chars[0, 4] != "-" else "A"           # a constant column: its blocks are zero
    sequences = ["".join(row) for row in chars]
    ref = MSA.from_sequences(sequences).invcov()
    tokens = RNAAlphabet().encode(sequences)[:, 1:].astype(np.uint8)
    out = os.path.join(HERE, "invcov_reference_n12_l9.npz")
    np.savez(out, sequences=np.array(sequences), tokens=tokens, invcov=np.asarray(ref, dtype=np.float64))
    print(f"wrote {out}: map {ref.shape}, max {ref.max():.6f}")


if __name__ == "__main__":
    main()
