"""Pair-map accuracy against a target (rnamsm_pair_sweep_* / rnamsm_pair_precision_*, ops.pair_sweep / pair_precision, rnamsm.metrics)
without a GPU: the two statements of each rule (tests/pair_metrics_truth.py) against each other,
the truth's counts through rnamsm.metrics against what the reference returned (tests/golden/pair_metrics_reference.npz, written by
tests/golden/make_golden_pair_metrics.py), the cut-offs for every L, the target readers, the two configuration keys and the gather refusal, the symbols, and every
argument refusal of the four entry points on fabricated aligned addresses that are never dereferenced."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from rnamsm import _lib, inference, metrics, ops
from rnamsm.config import Config, check_target_dir, parse_overrides
import pair_metrics_truth as T

GOLD = os.path.join(ROOT, "tests", "golden", "pair_metrics_reference.npz")
SS_DIR = os.path.join(ROOT, "tests", "golden", "ss", "SS_result")
NEW = ("rnamsm_pair_sweep_workspace_bytes", "rnamsm_pair_sweep_f64", "rnamsm_pair_sweep_f32",
       "rnamsm_pair_precision_workspace_bytes", "rnamsm_pair_precision_f64", "rnamsm_pair_precision_f32")
FAKE = 0x100000                 # 256-byte aligned, never dereferenced
ERR_INVALID = -1
TH = metrics.sweep_thresholds()


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def same_bits(a, b) -> bool:
    """float64 bits, NaN matching NaN of either sign or payload"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    both_nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(both_nan | (a.view(np.int64) == b.view(np.int64))))


def sweep_case(gold, n):
    x, t, missing, minsep = gold[f"sweep{n}_x"], gold[f"sweep{n}_tgt"], gold[f"sweep{n}_missing"], int(gold[f"sweep{n}_minsep"])
    skip = np.zeros(x.shape[0], dtype=np.uint8)
    skip[missing] = 1
    return x, t, skip if len(missing) else None, metrics.sweep_min_sep(minsep)


# ---- the rules, each stated twice ------------------------------------------------------------------------------------------------
def test_the_two_statements_of_the_sweep():
    rng = np.random.default_rng(5)
    assert len(TH) == 1001 and TH[0] == 0 and TH.dtype == np.float64
    for L in (2, 3, 9, 17):
        for dt in (np.float32, np.float64):
            vals = rng.choice(np.concatenate([TH.astype(dt), rng.random(50).astype(dt), np.array([np.nan, np.inf, -np.inf, -0.0, -1, 2], dtype=dt)]), (L, L))
            tgt = rng.choice(np.array([0, 0, 0, 1, 2, -1], dtype=np.int8), (L, L))
            for min_sep in sorted({1, 2, 4, max(L - 1, 1), L}):
                for skip in (None, rng.random(L) < 0.3):
                    a, b = T.sweep_broadcast(vals, tgt, TH, min_sep, skip), T.sweep_hist(vals, tgt, TH, min_sep, skip)
                    assert a.dtype == b.dtype == np.int64 and a.shape == (4, 1001) and np.array_equal(a, b), (L, dt, min_sep)
                    assert np.all(a.sum(0) == a.sum(0)[0])                     # tp + fp + tn + fn = the candidates, at every threshold


def test_the_two_statements_of_the_precision_rule():
    rng = np.random.default_rng(6)
    for L in (2, 3, 9, 17):
        for vals in (rng.standard_normal((L, L)), rng.integers(0, 3, (L, L)).astype(np.float32), np.zeros((L, L))):
            vals = vals.copy()
            vals[rng.random((L, L)) < 0.1] = np.nan
            tgt = rng.choice(np.array([0, 0, 1, -1], dtype=np.int8), (L, L))
            for min_sep in sorted({1, 2, max(L - 1, 1), L}):
                for max_sep in (0, 1, 3, L):
                    for k, cuts in ((1, [1]), (7, [1, 3, 7]), (200, [1, 2, 50, 200])):
                        a, b = T.precision_ranked(vals, tgt, k, cuts, min_sep, max_sep), T.precision_loop(vals, tgt, k, cuts, min_sep, max_sep)
                        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3].tobytes() == b[3].tobytes()
                        assert a[0].dtype == np.int32 and np.all(np.diff(a[0]) >= 0) and a[0][-1] <= a[1] <= k


# ---- against the reference's recorded results ---------------------------------------------------------------------------------------
def check_scores(got, gold, prefix):
    for name in ("Recall", "PREC", "F1", "PR", "AUC"):
        assert same_bits(got[name], gold[f"{prefix}_{name}"]), (prefix, name)
    # PR1: sklearn's auc may order and sign the trapezoid's terms differently: any summation order of the 1000 terms stays within
    # 1001 * 2^-52 of the sum of their magnitudes
    want = float(gold[f"{prefix}_PR1_f64"])
    if np.isnan(want):
        assert np.isnan(got["PR1"]), prefix
        return
    terms = np.abs(np.diff(got["Recall"]) * (got["PREC"][1:] + got["PREC"][:-1]) / 2.0)
    assert abs(got["PR1"] - want) <= 1001 * 2.0 ** -52 * terms.sum(), (prefix, got["PR1"], want)
    # what the reference hands out is that number rounded to float32 (torch.tensor of a Python float)
    ref32 = gold[f"{prefix}_PR1"]
    assert ref32.dtype == np.float32 and abs(np.float32(got["PR1"]) - ref32) <= np.spacing(np.abs(ref32)), prefix


def test_sweep_scores_equal_the_reference(gold):
    counts = {}
    shapes = set()
    for n in range(int(gold["n_sweep"])):
        x, t, skip, min_sep = sweep_case(gold, n)
        counts[n] = T.sweep_hist(x, t, TH, min_sep, skip)
        shapes.add((x.shape[0], min_sep, skip is not None))
        check_scores(metrics.sweep_scores(counts[n]), gold, f"sweep{n}")
    assert shapes == {(L, m, s) for L in (10, 37, 64) for m in (1, 4) for s in (False, True)}
    items = [int(i) for i in gold["set_items"]]
    assert len(items) == 2
    check_scores(metrics.sweep_scores(sum(counts[i] for i in items)), gold, "set")        # a dataset: the scores of the summed counts
    with pytest.raises(ValueError, match=r"integer counts \[4, T\]"):
        metrics.sweep_scores(np.zeros((4, 5)))


def test_precision_cuts_for_every_length(gold):
    L0 = int(gold["cuts_L0"])
    assert L0 == 10 and gold["cuts"].shape == (4087, 10)
    for L in range(L0, 4097):
        c = metrics.precision_cuts(L)
        assert c.dtype == np.int32 and np.array_equal(c, gold["cuts"][L - L0]), L
        assert c[-1] == L and c[0] >= 1 and np.all(np.diff(c) >= 0)
    for L in (9, 1, 0):
        with pytest.raises(ValueError, match=f"L={L} is below 10"):
            metrics.precision_cuts(L)


def test_precisions_equal_the_reference(gold):
    for m in range(int(gold["n_prec"])):
        x, t = gold[f"prec{m}_x"], gold[f"prec{m}_tgt"]
        L = x.shape[0]
        cuts = metrics.precision_cuts(L)
        hits, n, _, _ = T.precision_ranked(x, t, L, cuts, metrics.precision_min_sep(int(gold[f"prec{m}_minsep"])), int(gold[f"prec{m}_maxsep"]))
        assert n == L and len(np.unique(x)) == L * L and (t < 0).any()
        got = metrics.precisions(hits, cuts)
        for name in ("AUC", "P@L", "P@L2", "P@L5"):
            assert got[name].dtype == np.float32 and got[name].tobytes() == np.float32(gold[f"prec{m}_{name}"]).tobytes(), (m, name)
    assert any(float(gold[f"prec{m}_P@L"]) > 0 for m in range(int(gold["n_prec"])))
    with pytest.raises(ValueError, match="ten hits and ten cuts"):
        metrics.precisions([1, 2], [1, 2])


# ---- targets -------------------------------------------------------------------------------------------------------------------------
def test_read_target_and_structure_scores(tmp_path):
    tb, pb = metrics.read_target(os.path.join(SS_DIR, "2DRB_1.bpseq"), 35)
    tc, pc = metrics.read_target(os.path.join(SS_DIR, "2DRB_1.ct"), 35)
    assert tb.dtype == np.int8 and tb.shape == (35, 35) and pb.dtype == np.int32 and pb.shape == (35,)
    assert np.array_equal(pb, pc) and np.array_equal(tb, tc) and np.array_equal(tb, tb.T)
    assert pb[0] == 31 and pb[30] == 1 and tb[0, 30] == 1 and tb.sum() == 2 * np.count_nonzero(pb) // 2 and np.count_nonzero(pb) > 0
    with pytest.raises(ValueError, match="a target of length 35 for an alignment of length 36"):
        metrics.read_target(os.path.join(SS_DIR, "2DRB_1.ct"), 36)
    a = np.zeros((12, 12), dtype=np.int64)
    a[1, 9] = a[9, 1] = 1
    a[2, 3] = -1
    np.save(tmp_path / "x.npy", a)
    tn, pn = metrics.read_target(str(tmp_path / "x.npy"), 12)
    assert tn.dtype == np.int8 and np.array_equal(tn, a) and pn[1] == 10 and pn[9] == 2 and np.count_nonzero(pn) == 2
    with pytest.raises(ValueError, match="a target of length 12 for an alignment of length 11"):
        metrics.read_target(str(tmp_path / "x.npy"), 11)
    np.save(tmp_path / "f.npy", np.zeros((12, 12)))
    with pytest.raises(ValueError, match="square integer array"):
        metrics.read_target(str(tmp_path / "f.npy"), 12)
    assert metrics.find_target(SS_DIR, "2DRB_1").endswith("2DRB_1.bpseq") and metrics.find_target(str(tmp_path), "x").endswith("x.npy")
    assert metrics.find_target(str(tmp_path), "nothing") is None
    s = metrics.structure_scores(pb, pb)
    assert s["precision"] == 1.0 and s["recall"] == 1.0 and s["F1"] == 1.0 and s["fp"] == s["fn"] == 0 and s["tp"] == np.count_nonzero(pb) // 2
    other = pb.copy()
    other[[0, 30]] = 0                                     # one pair fewer
    other[[33, 34]] = [35, 34]                             # and one that is not in the target
    s = metrics.structure_scores(other, pb)
    assert (s["tp"], s["fp"], s["fn"]) == (np.count_nonzero(pb) // 2 - 1, 1, 1) and s["precision"] == s["recall"]
    empty = metrics.structure_scores(np.zeros(35, int), np.zeros(35, int))
    assert np.isnan(empty["precision"]) and np.isnan(empty["recall"]) and np.isnan(empty["F1"])


# ---- the keys ------------------------------------------------------------------------------------------------------------------------
def test_the_configuration_keys_and_the_gather_refusal():
    d = Config().data
    assert d.target_dir == "" and d.target_min_sep == 1
    cfg = parse_overrides(["data.target_dir=/some/where", "data.target_min_sep=4"])
    assert cfg.data.target_dir == "/some/where" and cfg.data.target_min_sep == 4
    assert check_target_dir("", 1) == ("", 1) and check_target_dir("t", 6) == ("t", 6)
    for tok, text in (("data.target_min_sep=0", "data.target_min_sep=0 outside [1, 32768]"),
                      ("data.target_min_sep=32769", "data.target_min_sep=32769 outside [1, 32768]")):
        with pytest.raises(ValueError, match=re.escape(text)):
            parse_overrides([tok])
    with pytest.raises(ValueError, match=re.escape("data.target_dir=5 is not a string")):
        check_target_dir(5)
    with pytest.raises(ValueError, match=re.escape("data.target_min_sep=True is not an integer")):
        check_target_dir("t", True)
    sw = inference.read_switches(cfg, False)
    assert sw.target_dir == "/some/where" and sw.target_min_sep == 4 and inference.read_switches(Config(), False).target_dir == ""
    with pytest.raises(ValueError, match=re.escape("data.target_dir='/some/where' is not available with RNAMSM_GATHER_TO_RANK0=1")):
        inference.read_switches(cfg, True)
    with pytest.raises(ValueError, match="RNAMSM_GATHER_TO_RANK0=1"):
        inference.extract_feat(cfg, gather_to_rank0=True)                # at start-up: before a file or the device is looked at
    assert inference.read_switches(Config(), True).target_dir == ""      # off: the gather is what it was


def test_the_json_entries_and_the_summary():
    rng = np.random.default_rng(3)
    entries, total = [], np.zeros((4, 1001), dtype=np.int64)
    for n in range(3):
        x, t = rng.random((12, 12)), (rng.random((12, 12)) < 0.3).astype(np.int8)
        c = T.sweep_hist(x, t, TH, 1)
        total += c
        cuts = metrics.precision_cuts(12)
        hits = T.precision_ranked(x, t, 12, cuts, 1)[0]
        e = {"id": str(n), "ss": {"L": 12, "sweep": metrics.sweep_entry(c)}, "precision": {"contacts": metrics.precision_entry(hits, 12, cuts, 12)}}
        assert e["ss"]["sweep"]["counts"]["tp"] == c[0].tolist() and e["precision"]["contacts"]["P@L"] == float(metrics.precisions(hits, cuts)["P@L"])
        entries.append(e)
    entries.append({"id": "bare"})
    s = metrics.summary(entries)
    want = metrics.sweep_scores(total)
    assert s["alignments"] == 4 and s["sweep"]["alignments"] == 3 and s["sweep"]["counts"]["fn"] == total[3].tolist()
    assert all(same_bits(s["sweep"][k], want[k]) for k in ("F1", "PR", "PR1", "AUC"))
    assert s["precision"]["contacts"]["alignments"] == 3
    assert s["precision"]["contacts"]["AUC"] == float(np.mean([e["precision"]["contacts"]["AUC"] for e in entries[:3]]))


# ---- the library -----------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_bound_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "rnamsm.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"\b(rnamsm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header, flags=re.S))
    for name in NEW:
        assert name in protos and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert len(protos[name].split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert _lib._SIGNATURES["rnamsm_pair_sweep_f64"] == _lib._SIGNATURES["rnamsm_pair_sweep_f32"]
    assert _lib._SIGNATURES["rnamsm_pair_precision_f64"] == _lib._SIGNATURES["rnamsm_pair_precision_f32"]
    doc = re.search(r"/\* A pair map against a target structure.*?\*/", text, flags=re.S).group(0)
    for phrase in ("ONLY candidate elements of x and target are read", "the sweep's `minsep` is min_sep - 1", "NaN gives 0",
                   "target[i, j] != 0", "target[i, j] >= 0", "larger v first, then smaller i, then smaller j", "read nothing back",
                   "no output bit depends on the order", "the rest count as misses"):
        assert phrase in doc, phrase
    assert callable(ops.pair_sweep) and callable(ops.pair_precision)
    assert (_lib.PAIR_SWEEP_MAX_T, _lib.PAIR_PRECISION_MAX_CUTS) == (4096, 64)
    src = open(os.path.join(ROOT, "rna-msm_amd", "csrc", "Makefile")).read()
    assert " top_pairs.hip pair_metrics.hip " in src


def test_the_size_functions(lib):
    sweep, prec = lib.rnamsm_pair_sweep_workspace_bytes, lib.rnamsm_pair_precision_workspace_bytes
    for T_ in (0, -1, 4097):
        assert sweep(T_) == 0
    for T_ in (1, 1001, 4096):
        assert sweep(T_) % 256 == 0 and 16 * (T_ + 1) <= sweep(T_) < 16 * (T_ + 1) + 256
    for L, k, e in ((1, 8, 8), (32769, 8, 8), (8, 0, 8), (8, 65537, 4), (8, 8, 2), (8, 8, 0)):
        assert prec(L, k, e) == 0, (L, k, e)
    for L, k, e in ((2, 1, 4), (17, 7, 8), (1024, 1024, 4), (4096, 4096, 8)):
        floor = L * L * e + 16 * k + lib.rnamsm_top_pairs_workspace_bytes(L, k)
        assert prec(L, k, e) % 256 == 0 and floor <= prec(L, k, e) <= floor + 4 * 256, (L, k, e)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_refusal_of_the_sweep(lib, dtype):
    fn, name = getattr(lib, "rnamsm_pair_sweep_" + dtype), "pair_sweep_" + dtype
    need = lib.rnamsm_pair_sweep_workspace_bytes(1001)
    ok = dict(x=FAKE, L=9, ld=9, t=FAKE + 4096, ldt=9, skip=None, sep=1, th=FAKE + 8192, T=1001, counts=FAKE + 65536, ws=FAKE + 131072, wsb=need)

    def call(**kw):
        a = dict(ok, **kw)
        rc = fn(a["x"], a["L"], a["ld"], a["t"], a["ldt"], a["skip"], a["sep"], a["th"], a["T"], a["counts"], a["ws"], a["wsb"], None)
        return rc, lib.rnamsm_last_error().decode()

    for kw, text in (
            (dict(x=None), f"{name}: null pointer"), (dict(t=None), f"{name}: null pointer"), (dict(th=None), f"{name}: null pointer"),
            (dict(counts=None), f"{name}: null pointer"), (dict(ws=None), f"{name}: null pointer"),
            (dict(L=1, ld=1, ldt=1), f"{name}: L=1 outside [2, 32768]"), (dict(L=32769, ld=32769, ldt=32769), f"{name}: L=32769 outside [2, 32768]"),
            (dict(T=0), f"{name}: T=0 outside [1, 4096]"), (dict(T=4097), f"{name}: T=4097 outside [1, 4096]"),
            (dict(sep=0), f"{name}: min_sep=0 outside [1, 32768]"), (dict(sep=32769), f"{name}: min_sep=32769 outside [1, 32768]"),
            (dict(ld=8), f"{name}: ld=8 is smaller than L=9"), (dict(ldt=8), f"{name}: ld_t=8 is smaller than L=9"),
            (dict(wsb=need - 1), f"{name}: workspace of {need - 1} bytes is smaller than the {need} that T=1001 needs"),
            (dict(ws=FAKE + 131072 + 128), f"{name}: workspace misaligned (256 bytes)"),
            (dict(x=FAKE + 2), f"{name}: x / thresholds / counts misaligned"), (dict(th=FAKE + 8192 + 4), f"{name}: x / thresholds / counts misaligned"),
            (dict(counts=FAKE + 65536 + 4), f"{name}: x / thresholds / counts misaligned")):
        rc, msg = call(**kw)
        assert rc == ERR_INVALID and msg == text, (kw, rc, msg)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_refusal_of_the_precision_call(lib, dtype):
    fn, name = getattr(lib, "rnamsm_pair_precision_" + dtype), "pair_precision_" + dtype
    L, k, e = 9, 5, 8 if dtype == "f64" else 4
    need = lib.rnamsm_pair_precision_workspace_bytes(L, k, e)
    ok = dict(x=FAKE, L=L, ld=L, t=FAKE + 4096, ldt=L, sep=1, maxsep=0, k=k, cuts=FAKE + 8192, nc=3, hits=FAKE + 12288, count=FAKE + 16384,
              pairs=FAKE + 20480, scores=FAKE + 24576, ws=FAKE + 65536, wsb=need)

    def call(**kw):
        a = dict(ok, **kw)
        rc = fn(a["x"], a["L"], a["ld"], a["t"], a["ldt"], a["sep"], a["maxsep"], a["k"], a["cuts"], a["nc"], a["hits"], a["count"], a["pairs"],
                a["scores"], a["ws"], a["wsb"], None)
        return rc, lib.rnamsm_last_error().decode()

    mis = f"{name}: x / cuts / hits / count / pairs / scores misaligned"
    for kw, text in (
            (dict(x=None), f"{name}: null pointer"), (dict(t=None), f"{name}: null pointer"), (dict(cuts=None), f"{name}: null pointer"),
            (dict(hits=None), f"{name}: null pointer"), (dict(count=None), f"{name}: null pointer"), (dict(ws=None), f"{name}: null pointer"),
            (dict(L=1, ld=1, ldt=1), f"{name}: L=1 outside [2, 32768]"), (dict(L=32769, ld=32769, ldt=32769), f"{name}: L=32769 outside [2, 32768]"),
            (dict(k=0), f"{name}: k=0 outside [1, 65536]"), (dict(k=65537), f"{name}: k=65537 outside [1, 65536]"),
            (dict(nc=0), f"{name}: ncuts=0 outside [1, 64]"), (dict(nc=65), f"{name}: ncuts=65 outside [1, 64]"),
            (dict(sep=0), f"{name}: min_sep=0 outside [1, 32768]"), (dict(sep=32769), f"{name}: min_sep=32769 outside [1, 32768]"),
            (dict(maxsep=-1), f"{name}: max_sep=-1 is negative (0 = no upper limit)"),
            (dict(ld=8), f"{name}: ld=8 is smaller than L=9"), (dict(ldt=8), f"{name}: ld_t=8 is smaller than L=9"),
            (dict(wsb=need - 1), f"{name}: workspace of {need - 1} bytes is smaller than the {need} that L=9, k=5 need"),
            (dict(ws=FAKE + 65536 + 128), f"{name}: workspace misaligned (256 bytes)"),
            (dict(x=FAKE + 2), mis), (dict(cuts=FAKE + 8192 + 2), mis), (dict(hits=FAKE + 12288 + 1), mis), (dict(count=FAKE + 16384 + 2), mis),
            (dict(pairs=FAKE + 20480 + 2), mis), (dict(scores=FAKE + 24576 + 4), mis)):
        rc, msg = call(**kw)
        assert rc == ERR_INVALID and msg == text, (kw, rc, msg)


def test_no_cpu_path():
    import torch
    x, t = torch.zeros(12, 12), torch.zeros(12, 12, dtype=torch.int8)
    with pytest.raises(_lib.RnamsmError, match="no CPU path"):
        ops.pair_sweep(x, t, TH)
    with pytest.raises(_lib.RnamsmError, match="no CPU path"):
        ops.pair_precision(x, t, 12, metrics.precision_cuts(12), 1)
