"""data.target_dir / data.target_min_sep in the CLI loop (rnamsm.inference.extract_feat) on a small list with synthetic weights and a
synthetic SS head.  The targets are the run's own SS_result/<id>.bpseq of a first pass (two alignments), one hand-made .npy, one that
is missing, one of the wrong length and one alignment shorter than 10.  Every number of <id>_metrics.json equals the numpy truth
(tests/pair_metrics_truth.py) applied to np.load of the map the run wrote, and to the `.prob` file for the SS map; the summary equals
sweep_scores of the summed counts; the skip lines are printed; with the key absent the directory is what it was, byte for byte."""
import contextlib
import io
import json
import shutil

import numpy as np
import pytest
import torch

from rnamsm import metrics, ss, synthetic
import pair_metrics_truth as T
import ss_truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"rnaA": (6, 20), "rnaB": (5, 32), "rnaC": (4, 24), "rnaMiss": (4, 15), "rnaTiny": (3, 8), "rnaWrong": (4, 18)}
NB, MIN_SEP = 4, 2
BASE = ["data.contacts=true", "data.invcov=true", "data.mi=true"]
TH = metrics.sweep_thresholds()
MAPS = ("contacts", "invcov", "mi", "mip")


@pytest.fixture(scope="module")
def model():
    from rnamsm.model import MSATransformer
    state = synthetic.make_state_dict(seed=0)
    m = MSATransformer(num_layers=10)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV)


def _run(model, root, overrides):
    from rnamsm.config import Config, parse_overrides
    from rnamsm.inference import extract_feat
    rng = np.random.RandomState(11)
    (root / "results").mkdir(parents=True)
    for i, (depth, length) in SHAPES.items():
        first = "".join(rng.choice(list("ACGU"), length))
        rows = [first] + ["".join(c if rng.rand() < 0.8 else rng.choice(list("ACGU")) for c in first) for _ in range(depth - 1)]
        (root / "results" / f"{i}.a2m_msa2").write_text("".join(f">s{r}\n{row}\n" for r, row in enumerate(rows)))
    (root / "rna_id.txt").write_text("\n".join(SHAPES) + "\n")
    ss_pt = root / "rna-msm_attention.pt"
    torch.save({k: torch.from_numpy(v) for k, v in ss_truth.make_state(NB, seed=5).items()}, ss_pt)
    cfg = Config()
    cfg.data.root_path, cfg.data.MSA_path, cfg.data.MSA_list = str(root), "results", "rna_id.txt"
    cfg.data.sample_method, cfg.data.max_seqs_per_msa = "first", 64
    cfg = parse_overrides(BASE + [f"data.ss_model_path={ss_pt}"] + list(overrides), cfg)
    real_load = ss.load_predictor
    printed = io.StringIO()
    with pytest.MonkeyPatch.context() as mp, contextlib.redirect_stdout(printed):
        mp.setattr(ss, "load_predictor", lambda path, device, num_blocks=NB: real_load(path, device, num_blocks))
        assert extract_feat(cfg, model=model) == sorted(SHAPES)
    files = {str(f.relative_to(root / "results")): f.read_bytes() for f in sorted((root / "results").rglob("*"))
             if f.is_file() and f.suffix != ".a2m_msa2"}
    return files, printed.getvalue().replace(str(root), "<root>")


@pytest.fixture(scope="module")
def runs(model, tmp_path_factory):
    root = tmp_path_factory.mktemp("pair_metrics_cli")
    first = _run(model, root / "first", [])
    tdir = root / "targets"
    tdir.mkdir()
    for i in ("rnaA", "rnaB", "rnaTiny"):
        shutil.copy(root / "first" / "results" / "SS_result" / f"{i}.bpseq", tdir / f"{i}.bpseq")
    shutil.copy(root / "first" / "results" / "SS_result" / "rnaA.bpseq", tdir / "rnaWrong.bpseq")        # 20 positions for 18
    rng = np.random.default_rng(24)
    hand = rng.choice(np.array([0, 0, 0, 1, -1], dtype=np.int64), (24, 24))
    np.save(tdir / "rnaC.npy", hand)
    on = _run(model, root / "on", [f"data.target_dir={tdir}", f"data.target_min_sep={MIN_SEP}"])
    empty = _run(model, root / "empty", ["data.target_dir=", f"data.target_min_sep={MIN_SEP}"])
    return root, tdir, {"first": first, "on": on, "empty": empty}


def _entry(runs, i):
    return json.loads(runs[2]["on"][0][f"{i}_metrics.json"])


@pytest.mark.parametrize("i", ["rnaA", "rnaB", "rnaC"])
def test_every_number_equals_the_truth_on_the_written_files(runs, i):
    root, tdir, _ = runs
    res = root / "on" / "results"
    L = SHAPES[i][1]
    path = metrics.find_target(str(tdir), i)
    target, partner = metrics.read_target(path, L)
    e = _entry(runs, i)
    assert e["id"] == i and e["min_sep"] == MIN_SEP and e["target"] == i + (".npy" if i == "rnaC" else ".bpseq")
    probs = np.loadtxt(res / "SS_result" / f"{i}.prob")
    assert probs.shape == (L, L)
    counts = T.sweep_hist(probs, target, TH, MIN_SEP)
    assert np.array_equal(counts, T.sweep_broadcast(probs, target, TH, MIN_SEP))
    sweep = e["ss"]["sweep"]
    assert e["ss"]["L"] == L and [sweep["counts"][n] for n in ("tp", "fp", "tn", "fn")] == counts.tolist()
    want = metrics.sweep_scores(counts)
    for name in ("F1", "PR", "PR1", "AUC"):
        assert sweep[name] == float(want[name]) or (np.isnan(sweep[name]) and np.isnan(want[name])), name
    # the decoded structure against the target's partner vector
    _, mine = metrics.read_target(str(res / "SS_result" / f"{i}.bpseq"), L)
    assert json.dumps(e["ss"]["structure"], sort_keys=True) == json.dumps(metrics.structure_scores(mine, partner), sort_keys=True)
    if i != "rnaC":                                       # the run's own structure is its target: nothing missed, nothing extra
        st, pairs = e["ss"]["structure"], int(np.count_nonzero(mine)) // 2
        assert (st["tp"], st["fp"], st["fn"]) == (pairs, 0, 0)
        assert (st["precision"] == st["recall"] == st["F1"] == 1.0) if pairs else np.isnan(st["precision"])
    assert sorted(e["precision"]) == sorted(MAPS)
    for kind in MAPS:
        x = np.load(res / f"{i}_{kind}.npy")
        assert x.shape == (L, L)
        cuts = metrics.precision_cuts(L)
        hits, n, _, _ = T.precision_ranked(x, target, L, cuts, MIN_SEP)
        p, rec = metrics.precisions(hits, cuts), e["precision"][kind]
        assert (rec["L"], rec["count"], rec["cuts"], rec["hits"]) == (L, n, cuts.tolist(), hits.tolist()), kind
        for name in ("P@L", "P@L2", "P@L5", "AUC"):
            assert rec[name] == float(p[name]), (kind, name)


def test_structure_scores_of_a_structure_against_itself():
    partner = np.array([0, 8, 7, 0, 0, 0, 3, 2, 0, 0])
    s = metrics.structure_scores(partner, partner)
    assert (s["tp"], s["fp"], s["fn"], s["precision"], s["recall"], s["F1"]) == (2, 0, 0, 1.0, 1.0, 1.0)


def test_the_summary_equals_the_scores_of_the_summed_counts(runs):
    files = runs[2]["on"][0]
    s = json.loads(files["metrics_summary.json"])
    entries = [_entry(runs, i) for i in ("rnaA", "rnaB", "rnaC")]
    total = sum(np.array([e["ss"]["sweep"]["counts"][n] for n in ("tp", "fp", "tn", "fn")], dtype=np.int64) for e in entries)
    want = metrics.sweep_scores(total)
    assert s["alignments"] == 3 and s["sweep"]["alignments"] == 3
    assert [s["sweep"]["counts"][n] for n in ("tp", "fp", "tn", "fn")] == total.tolist()
    for name in ("F1", "PR", "PR1", "AUC"):
        assert s["sweep"][name] == float(want[name]) or (np.isnan(s["sweep"][name]) and np.isnan(want[name])), name
    for kind in MAPS:
        for name in ("P@L", "P@L2", "P@L5", "AUC"):
            assert s["precision"][kind]["alignments"] == 3
            assert s["precision"][kind][name] == float(np.mean(np.array([e["precision"][kind][name] for e in entries], dtype=np.float64)))
    assert json.dumps(s, sort_keys=True) == json.dumps(metrics.summary(entries), sort_keys=True)


def test_the_skip_lines(runs):
    files, printed = runs[2]["on"]
    assert sorted(f for f in files if "metrics" in f) == ["metrics_summary.json", "rnaA_metrics.json", "rnaB_metrics.json", "rnaC_metrics.json"]
    lines = [ln for ln in printed.splitlines() if "no metrics" in ln]
    miss = [ln for ln in lines if ln.startswith("rnaMiss:")]
    assert len(miss) == 1 and "no rnaMiss.bpseq, .ct or .npy there" in miss[0]
    wrong = [ln for ln in lines if ln.startswith("rnaWrong:")]
    assert len(wrong) == 5 and all("a target of length 20 for an alignment of length 18" in ln for ln in wrong)      # the SS map and four maps
    tiny = [ln for ln in lines if ln.startswith("rnaTiny:")]
    assert len(tiny) == 5 and all("L=8 is below 10" in ln for ln in tiny)
    assert len(lines) == 11


def test_the_key_changes_no_other_file_and_absent_is_what_it_was(runs):
    first, on, empty = (runs[2][k] for k in ("first", "on", "empty"))
    assert {f: d for f, d in on[0].items() if "metrics" not in f} == first[0]
    assert first == empty                                                  # the file set, every byte, and stdout
    assert not any("metrics" in f for f in first[0]) and "metrics" not in first[1]
    assert [ln for ln in on[1].splitlines() if "no metrics" not in ln] == first[1].splitlines()
