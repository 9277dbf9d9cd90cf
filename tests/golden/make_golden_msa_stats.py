#!/usr/bin/env python3
"""Generates tests/golden/msa_stats_reference_2drb64.npz with the reference's own MSA class (utils/align.py; needs the reference tree,
see _refimport -- at generation time only; nothing under tests/ imports it at test time) on the shipped 64-row excerpt
tests/golden/2DRB_1_first64.a2m_msa2, read by MSA.from_fasta as the reference's dataset reads it.

  pdist        MSA.pdist(), float64 [64, 64] (:121-126)
  weights      MSA.weights at the default seqid_cutoff = 0.2, float64 [64] (:250-253)
  neff_none / neff_sqrt / neff_seqlen    MSA.neff("none" | "sqrt" | "seqlen"), float64 scalars (:259-269)
  coverage     MSA.coverage, float64 [L] (:242-247)
  seqid_cutoff the cutoff the weights were made at

Run:  python tests/golden/make_golden_msa_stats.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def main():
    from _refimport import reference_modules
    MSA = reference_modules()[4]
    msa = MSA.from_fasta(os.path.join(HERE, "2DRB_1_first64.a2m_msa2"))
    out = os.path.join(HERE, "msa_stats_reference_2drb64.npz")
    np.savez(out, pdist=np.asarray(msa.pdist(), dtype=np.float64), weights=np.asarray(msa.weights, dtype=np.float64),
             neff_none=np.float64(msa.neff("none")), neff_sqrt=np.float64(msa.neff("sqrt")), neff_seqlen=np.float64(msa.neff("seqlen")),
             coverage=np.asarray(msa.coverage, dtype=np.float64), seqid_cutoff=np.float64(msa.seqid_cutoff))
    print(f"wrote {out}: {msa.depth} rows x {msa.seqlen} columns, Neff {msa.neff():.6f}")


if __name__ == "__main__":
    main()
