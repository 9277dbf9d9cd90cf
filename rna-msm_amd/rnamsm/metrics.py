"""Accuracy of a pair map against a target structure, from the integer counts the device makes (ops.pair_sweep, ops.pair_precision;
include/rnamsm.h states both rules).  Everything here runs on the host, in numpy, on a few thousand numbers:

  sweep_thresholds / sweep_scores   the reference's rna_compute_precisions (utils/metrics.py:9-70): F1, PR, PR1, AUC, Recall, PREC from
                                    the tp / fp / tn / fn of the 1001 thresholds.  The counts add over a dataset, so a dataset's scores
                                    are sweep_scores(the sum of its counts) -- what the reference accumulates.
  precision_cuts / precisions       the reference's compute_precisions (utils/metrics.py:180-252): P@L, P@L2, P@L5 and their AUC from
                                    the hits among the first 0.1 L, 0.2 L, ..., L ranked pairs.
  read_target / structure_scores    a known structure from a .bpseq, .ct or .npy file, and a decoded structure against it.

The reference's `minsep` differs between its two functions: the sweep masks with triu(minsep + 1), compute_precisions with
sep >= minsep.  The device calls take min_sep = the least j - i; sweep_min_sep and precision_min_sep translate."""
from __future__ import annotations

import os
from typing import Dict, Tuple

import numpy as np

TARGET_SUFFIXES = (".bpseq", ".ct", ".npy")


def sweep_min_sep(minsep: int) -> int:
    """rna_compute_precisions' minsep -> the device's min_sep."""
    return int(minsep) + 1


def precision_min_sep(minsep: int) -> int:
    """compute_precisions' minsep -> the device's min_sep (the same number; 0 also means 1: the diagonal is no pair)."""
    return max(int(minsep), 1)


def sweep_thresholds(step: float = 0.001) -> np.ndarray:
    """The reference's threshold table: np.arange(0, 1 + step, step), 1001 float64 values at the default step."""
    return np.arange(0, 1 + step, step)


def _trapezoid(y: np.ndarray, x: np.ndarray) -> float:
    """np.trapz as numpy forms it: (diff(x) * (y[1:] + y[:-1]) / 2.0).sum()."""
    return float((np.diff(x) * (y[1:] + y[:-1]) / 2.0).sum())


def sweep_scores(counts) -> Dict[str, object]:
    """counts: integers [4, T], the rows tp, fp, tn, fn (one map's, or the sum over a dataset) -> the reference's dictionary: F1 (the
    largest over the thresholds, NaN left out), PR = trapz(y=recall, x=prec), PR1 = the area under (recall, prec) with the sign
    sklearn's auc gives it (-1 for an x that never ascends and descends somewhere, else +1), AUC = trapz(y=sens, x=spec), Recall and
    PREC [T].  float64 throughout, with the reference's expressions: 0 / 0 is NaN, and prec's NaN become 0."""
    c = np.asarray(counts)
    if c.ndim != 2 or c.shape[0] != 4 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"sweep_scores: expected integer counts [4, T], got {c.shape} of {c.dtype}")
    tp, fp, tn, fn = (c[r].astype(np.int64) for r in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = tp / (tp + fp).astype(float)
        recall = tp / (tp + fn).astype(float)
        sens = tp / (tp + fn).astype(float)
        spec = tn / (tn + fp).astype(float)
        prec[np.isnan(prec)] = 0
        f1 = 2 * ((prec * sens) / (prec + sens))
        best = float(np.nanmax(f1)) if not np.isnan(f1).all() else float("nan")
        dx = np.diff(recall)
        direction = -1.0 if (np.any(dx < 0) and np.all(dx <= 0)) else 1.0
        if np.any(dx < 0) and not np.all(dx <= 0):
            raise ValueError("sweep_scores: the recall neither ascends nor descends over the thresholds: these are no sweep counts")
        pr1 = direction * _trapezoid(prec, recall)
        pr = _trapezoid(recall, prec)
        auc = _trapezoid(sens, spec)
    return {"F1": best, "PR1": pr1, "AUC": auc, "PR": pr, "Recall": recall, "PREC": prec}


def precision_cuts(L: int) -> np.ndarray:
    """The ten list lengths of compute_precisions for a map of L positions: its gather indices + 1, i.e. the ten float32 values
    0.1, 0.2, ..., 1.0 (each formed in float64 as 0.1 + 0.1 i and rounded once) times L in float32, truncated.  int32 [10], ascending,
    the last one L.  L < 10 is refused: the reference's first index is -1 there."""
    L = int(L)
    if L < 10:
        raise ValueError(f"precision_cuts: L={L} is below 10 (the reference's first list would be empty)")
    frac = (0.1 + 0.1 * np.arange(10, dtype=np.float64)).astype(np.float32)
    return (frac * np.float32(L)).astype(np.int64).astype(np.int32)


def precisions(hits, cuts) -> Dict[str, np.float32]:
    """hits [10] at precision_cuts' ten cuts -> P@L, P@L2, P@L5 and AUC (their mean over the ten cuts) in float32, as the reference
    forms them: a float32 count divided by a float32 length."""
    h = np.asarray(hits).astype(np.float32)
    c = np.asarray(cuts).astype(np.float32)
    if h.shape != (10,) or c.shape != (10,):
        raise ValueError(f"precisions: expected ten hits and ten cuts, got {h.shape} and {c.shape}")
    binned = h / c
    return {"AUC": _mean10(binned), "P@L": binned[9], "P@L2": binned[4], "P@L5": binned[1]}


def _mean10(v: np.ndarray) -> np.float32:
    """The mean of ten float32 values as torch.mean forms it on the CPU (the bits tests/golden/pair_metrics_reference.npz records):
    float32 throughout, one vector of eight lanes and a tail of two -- the tail's sum first, then the eight lanes added in index
    order -- and one division by 10.  That order belongs to the torch build the fixture was recorded with (its vectorised inner
    reduction); another build may sum in another order and differ in the last bit.  It was checked against that build on 3000 random
    vectors of this shape and is held to the fixture's five maps by tests/test_pair_metrics_host.py."""
    s = np.float32(0)
    for e in list(v[8:]) + list(v[:8]):
        s = np.float32(s + e)
    return np.float32(s / np.float32(10))


def _partner_from_text(path: str) -> np.ndarray:
    """.bpseq (`i base j`) or .ct (a header line, then `i base i-1 i+1 j i`) -> the partner column in file order, checked."""
    ct = path.endswith(".ct")
    rows = []
    with open(path) as f:
        lines = [ln.split() for ln in f if ln.strip() and not ln.lstrip().startswith("#")]
    if ct:
        lines = lines[1:]                                  # the header: length and name
    for n, fields in enumerate(lines, 1):
        want = 6 if ct else 3
        if len(fields) < want:
            raise ValueError(f"{path}: row {n} has {len(fields)} fields, expected {want}")
        idx, partner = int(fields[0]), int(fields[4 if ct else 2])
        if idx != n:
            raise ValueError(f"{path}: row {n} is numbered {idx}")
        rows.append(partner)
    return np.asarray(rows, dtype=np.int64)


def read_target(path: str, L: int) -> Tuple[np.ndarray, np.ndarray]:
    """A known structure of L positions -> (target int8 [L, L], partner int32 [L]: 0 = unpaired, else the partner's 1-based index).
    .bpseq / .ct: the partner column; target[i, j] = target[j, i] = 1 for every pair.  .npy: an integer [L, L] array taken as the target
    as it is (negative = invalid, as in compute_precisions); its partner vector names, per position, the first j with a positive
    entry in row or column.  A length other than L raises an error that names both lengths."""
    L = int(L)
    if path.endswith(".npy"):
        a = np.load(path)
        if a.ndim != 2 or a.shape[0] != a.shape[1] or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{path}: expected a square integer array, got {a.shape} of {a.dtype}")
        if a.shape[0] != L:
            raise ValueError(f"{path}: a target of length {a.shape[0]} for an alignment of length {L}")
        if a.size and (a.min() < -128 or a.max() > 127):
            raise ValueError(f"{path}: entries outside int8")
        target = np.ascontiguousarray(a.astype(np.int8))
        pos = (target > 0) | (target > 0).T
        partner = np.where(pos.any(1), pos.argmax(1) + 1, 0).astype(np.int32)
        return target, partner
    if not path.endswith((".bpseq", ".ct")):
        raise ValueError(f"{path}: a target is a .bpseq, .ct or .npy file")
    col = _partner_from_text(path)
    if col.shape[0] != L:
        raise ValueError(f"{path}: a target of length {col.shape[0]} for an alignment of length {L}")
    if col.size and (col.min() < 0 or col.max() > L):
        raise ValueError(f"{path}: a partner outside [0, {L}]")
    target = np.zeros((L, L), dtype=np.int8)
    i = np.flatnonzero(col)
    target[i, col[i] - 1] = 1
    target[col[i] - 1, i] = 1
    return target, col.astype(np.int32)


def find_target(target_dir: str, rna_id: str):
    """<target_dir>/<id>.bpseq, then .ct, then .npy -> the first that exists, or None."""
    for suffix in TARGET_SUFFIXES:
        path = os.path.join(target_dir, rna_id + suffix)
        if os.path.isfile(path):
            return path
    return None


def structure_scores(partner_pred, partner_true) -> Dict[str, float]:
    """A decoded structure against the known one, both as partner vectors of one length (0 = unpaired, else the partner's 1-based
    index): the pairs (i, j), i < j, as sets -> tp, fp, fn, precision = tp / (tp + fp), recall = tp / (tp + fn) and
    F1 = 2 tp / (2 tp + fp + fn); a ratio of 0 / 0 is NaN."""
    a, b = (np.asarray(p).reshape(-1).astype(np.int64) for p in (partner_pred, partner_true))
    if a.shape != b.shape:
        raise ValueError(f"structure_scores: partner vectors of {a.shape[0]} and {b.shape[0]} entries")

    def pairs(p):
        return {(int(i), int(p[i]) - 1) for i in np.flatnonzero(p) if p[i] - 1 > i}

    pa, pb = pairs(a), pairs(b)
    tp, fp, fn = len(pa & pb), len(pa - pb), len(pb - pa)

    def ratio(n, d):
        return n / d if d else float("nan")

    return {"tp": tp, "fp": fp, "fn": fn, "precision": ratio(tp, tp + fp), "recall": ratio(tp, tp + fn),
            "F1": ratio(2 * tp, 2 * tp + fp + fn)}


# ---- what the CLI writes (data.target_dir): <id>_metrics.json and metrics_summary.json -----------------------------------------------
SWEEP_SCALARS = ("F1", "PR", "PR1", "AUC")
PRECISION_NAMES = ("P@L", "P@L2", "P@L5", "AUC")


def sweep_entry(counts) -> Dict[str, object]:
    """int64 [4, T] counts -> {"counts": {"tp", "fp", "tn", "fn": lists}, "F1", "PR", "PR1", "AUC": floats}"""
    c = np.asarray(counts).astype(np.int64)
    s = sweep_scores(c)
    return {"counts": {n: [int(v) for v in c[r]] for r, n in enumerate(("tp", "fp", "tn", "fn"))}, **{n: float(s[n]) for n in SWEEP_SCALARS}}


def precision_entry(hits, count: int, cuts, L: int) -> Dict[str, object]:
    """hits at precision_cuts(L), the length of the ranked list -> {"L", "count", "cuts", "hits", "P@L", "P@L2", "P@L5", "AUC"}"""
    p = precisions(hits, cuts)
    return {"L": int(L), "count": int(count), "cuts": [int(c) for c in cuts], "hits": [int(h) for h in np.asarray(hits)],
            **{n: float(p[n]) for n in PRECISION_NAMES}}


def summary(entries) -> Dict[str, object]:
    """The entries of the <id>_metrics.json files, in list order -> the dataset's record: the summed sweep counts with sweep_scores of
    the sum (what the reference accumulates over a list), and per map the float64 mean of each precision over the alignments that
    have one."""
    out: Dict[str, object] = {"alignments": len(entries)}
    sweeps = [e["ss"]["sweep"]["counts"] for e in entries if "sweep" in e.get("ss", {})]
    if sweeps:
        total = sum(np.array([c[n] for n in ("tp", "fp", "tn", "fn")], dtype=np.int64) for c in sweeps)
        out["sweep"] = {"alignments": len(sweeps), **sweep_entry(total)}
    per_map: Dict[str, list] = {}
    for e in entries:
        for name, rec in e.get("precision", {}).items():
            per_map.setdefault(name, []).append(rec)
    out["precision"] = {name: {"alignments": len(recs), **{n: float(np.mean(np.array([r[n] for r in recs], dtype=np.float64))) for n in PRECISION_NAMES}}
                        for name, recs in per_map.items()}
    nested = [e["ss_nested"] for e in entries if "ss_nested" in e]       # data.ss_nested: absent, the summary is what it was
    if nested:
        def mean(name):          # over the alignments where the ratio exists (0 / 0 is NaN there); NaN where it exists nowhere
            vals = np.array([r[name] for r in nested], dtype=np.float64)
            vals = vals[~np.isnan(vals)]
            return float(vals.mean()) if vals.size else float("nan")

        out["ss_nested"] = {"alignments": len(nested), **{n: mean(n) for n in ("precision", "recall", "F1")}}
    return out
