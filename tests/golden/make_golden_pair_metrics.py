#!/usr/bin/env python3
"""Generates tests/golden/pair_metrics_reference.npz with the reference's own rna_compute_precisions and compute_precisions
(utils/metrics.py; needs the reference tree and scikit-learn, see _refimport -- at generation time only; nothing under tests/ imports
it at test time).

  sweep<n>_x / _tgt / _missing / _minsep      one map of rna_compute_precisions: float32 [L, L] in [0, 1), a 0 / 1 target with a few
                                              helices, the missing_nt_index (empty = None) and the reference's minsep; L in {10, 37, 64},
                                              minsep in {0, 3}, with and without missing positions
  sweep<n>_F1 / _PR / _PR1 / _AUC / _Recall / _PREC   what the reference returns for that map alone (PR1 is float32 there: it wraps
                                              sklearn's Python float in torch.tensor); _PR1_f64: sklearn's auc on the returned float64
                                              Recall and PREC, the same call before that rounding
  set_items, set_F1 ...                       a two-item list (the dataset sum) and what the reference returns for it
  prec<n>_x / _tgt / _minsep / _maxsep        one map of compute_precisions: float32 [L, L] with DISTINCT values, targets in {-1, 0, 1}
                                              that leave at least L valid candidates (maxsep 0 = None) -- asserted here: with those the
                                              reference's unstable argsort and its -inf tail cannot differ from the rule
  prec<n>_AUC / _P@L / _P@L2 / _P@L5          what the reference returns, float32
  cuts_L0, cuts                               the ten list lengths (gather indices + 1) for every L in [10, 4096]: int32 [4087, 10]

Run:  python tests/golden/make_golden_pair_metrics.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def helices(rng, L):
    """A symmetric 0 / 1 target with a few stacked pairs."""
    t = np.zeros((L, L), dtype=np.float32)
    used = np.zeros(L, dtype=bool)
    for _ in range(max(1, L // 12)):
        i, j, n = int(rng.randint(0, L // 2)), int(rng.randint(L // 2, L)), int(rng.randint(2, 5))
        for s in range(n):
            a, b = i + s, j - s
            if 0 <= a < b < L and b - a >= 2 and not used[a] and not used[b]:
                t[a, b] = t[b, a] = 1
                used[a] = used[b] = True
    return t


def main():
    import torch
    from _refimport import install
    install()
    from sklearn.metrics import auc
    from utils.metrics import compute_precisions, rna_compute_precisions
    rng = np.random.RandomState(322)
    got = {}

    def record(prefix, res):
        for name in ("F1", "PR", "PR1", "AUC", "Recall", "PREC"):
            got[f"{prefix}_{name}"] = np.asarray(res[name].cpu().numpy() if hasattr(res[name], "cpu") else res[name])
        # the reference wraps sklearn's Python float in torch.tensor, which rounds PR1 to float32; the same call on the float64
        # Recall and PREC it returns gives the number before that rounding
        assert got[f"{prefix}_PR1"].dtype == np.float32 and got[f"{prefix}_PR"].dtype == np.float64
        with np.errstate(invalid="ignore"):
            got[f"{prefix}_PR1_f64"] = np.float64(auc(got[f"{prefix}_Recall"], got[f"{prefix}_PREC"]))

    def batch(x, tgt, missing):
        return {"predictions": torch.from_numpy(x), "tgt": torch.from_numpy(tgt), "missing_nt_index": list(missing) if len(missing) else None}

    n = 0
    for L in (10, 37, 64):
        for minsep in (0, 3):
            for with_missing in (False, True):
                x = rng.rand(L, L).astype(np.float32)
                x[rng.rand(L, L) < 0.5] *= np.float32(0.01)                          # most of a probability map is near 0
                tgt = helices(rng, L)
                missing = np.sort(rng.choice(L, size=max(1, L // 9), replace=False)).astype(np.int64) if with_missing else np.zeros(0, np.int64)
                got[f"sweep{n}_x"], got[f"sweep{n}_tgt"], got[f"sweep{n}_missing"], got[f"sweep{n}_minsep"] = x, tgt.astype(np.int8), missing, np.int64(minsep)
                record(f"sweep{n}", rna_compute_precisions([batch(x, tgt, missing)], minsep=minsep))
                n += 1
    got["n_sweep"] = np.int64(n)
    items = np.array([7, 10], dtype=np.int64)                                       # L = 37 and L = 64, both minsep = 3, one with missing
    assert int(got["sweep7_minsep"]) == 3 and int(got["sweep10_minsep"]) == 3 and len(got["sweep7_missing"]) and not len(got["sweep10_missing"])
    got["set_items"] = items
    record("set", rna_compute_precisions(
        [batch(got[f"sweep{i}_x"], got[f"sweep{i}_tgt"].astype(np.float32), got[f"sweep{i}_missing"]) for i in items], minsep=3))

    m = 0
    for L, minsep, maxsep in ((10, 1, 0), (37, 6, 0), (64, 6, 0), (64, 1, 24), (37, 3, 0)):
        vals = rng.permutation(L * L).astype(np.float32) / np.float32(L * L)          # distinct: L * L < 2^24 integers, one division each
        x = vals.reshape(L, L)
        tgt = helices(rng, L).astype(np.int64)
        x[(tgt == 1) & (rng.rand(L, L) < 0.7)] += np.float32(1)                       # most true pairs score high
        assert len(np.unique(x)) == L * L
        tgt[rng.rand(L, L) < 0.1] = -1
        sep = np.arange(L)[None, :] - np.arange(L)[:, None]
        valid = (sep >= minsep) & (tgt >= 0) & ((sep < maxsep) if maxsep else True)
        assert int(valid.sum()) >= L, (L, minsep, maxsep, int(valid.sum()))
        res = compute_precisions(torch.from_numpy(x), torch.from_numpy(tgt), minsep=minsep, maxsep=maxsep or None)
        got[f"prec{m}_x"], got[f"prec{m}_tgt"], got[f"prec{m}_minsep"], got[f"prec{m}_maxsep"] = x, tgt.astype(np.int8), np.int64(minsep), np.int64(maxsep)
        for name in ("AUC", "P@L", "P@L2", "P@L5"):
            v = res[name].numpy()
            assert v.dtype == np.float32 and v.shape == (1,)
            got[f"prec{m}_{name}"] = v[0]
        m += 1
    got["n_prec"] = np.int64(m)

    frac = torch.arange(0.1, 1.1, 0.1).unsqueeze(0)
    assert frac.shape == (1, 10) and frac.dtype == torch.float32
    lengths = torch.arange(10, 4097, dtype=torch.long).unsqueeze(1)
    got["cuts_L0"] = np.int64(10)
    got["cuts"] = ((frac * lengths).type(torch.long) - 1 + 1).numpy().astype(np.int32)
    assert got["cuts"].shape == (4087, 10)

    out = os.path.join(HERE, "pair_metrics_reference.npz")
    np.savez_compressed(out, **got)
    print(f"wrote {out}: {n} sweep maps, {m} precision maps, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
