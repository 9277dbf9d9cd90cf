"""data.ss_nested / data.ss_nested_threshold / data.ss_nested_min_loop in the CLI loop (rnamsm.inference.extract_feat) on the shipped
64-row excerpt of 2DRB_1 and a small synthetic list (which shares packed groups), with synthetic weights and a synthetic 16-block SS
head.  With the key on SS_result/<id>.dbn, <id>.nested.ct and <id>.nested.bpseq appear, the `.dbn` parses back to the partner vector
of `.nested.bpseq`, and both equal the truth (tests/ss_nested_truth.py) on the `.prob` file the same run wrote; `.ct`, `.bpseq`,
`.prob` and the `.npy` files are the bytes of a run with the key off, which writes no new file.  With data.target_dir the metrics JSON
gains `ss_nested`, equal to structure_scores of the truth's partner vector.  The bf16 head goes the same way.  SS_predict.py --nested
writes the CLI's `.dbn`."""
import contextlib
import io
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from rnamsm import metrics, ss, synthetic
import ss_nested_truth as T
import ss_truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"rnaA": (6, 20), "rnaB": (5, 32), "rnaC": (4, 70), "rnaTiny": (3, 8)}
IDS = ["2DRB_1"] + list(SHAPES)
THETA, MIN_LOOP = 0.3, 2
NEW = (".dbn", ".nested.ct", ".nested.bpseq")


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
    rng = np.random.RandomState(23)
    (root / "results").mkdir(parents=True)
    shutil.copy(os.path.join(GOLDEN, "2DRB_1_first64.a2m_msa2"), root / "results" / "2DRB_1.a2m_msa2")
    for i, (depth, length) in SHAPES.items():
        first = "".join(rng.choice(list("ACGU"), length))
        rows = [first] + ["".join(c if rng.rand() < 0.8 else rng.choice(list("ACGU")) for c in first) for _ in range(depth - 1)]
        (root / "results" / f"{i}.a2m_msa2").write_text("".join(f">s{r}\n{row}\n" for r, row in enumerate(rows)))
    (root / "rna_id.txt").write_text("\n".join(IDS) + "\n")
    (root / "model").mkdir()
    ss_pt = root / "model" / "rna-msm_attention.pt"
    torch.save({k: torch.from_numpy(v) for k, v in ss_truth.make_state(16, seed=5).items()}, ss_pt)
    cfg = Config()
    cfg.data.root_path, cfg.data.MSA_path, cfg.data.MSA_list = str(root), "results", "rna_id.txt"
    cfg.data.sample_method, cfg.data.max_seqs_per_msa = "first", 64
    cfg = parse_overrides([f"data.ss_model_path={ss_pt}"] + list(overrides), cfg)
    with contextlib.redirect_stdout(io.StringIO()):
        assert extract_feat(cfg, model=model) == sorted(IDS)
    return {str(f.relative_to(root / "results")): f.read_bytes() for f in sorted((root / "results").rglob("*"))
            if f.is_file() and f.suffix != ".a2m_msa2"}


ON = ["data.ss_nested=true", f"data.ss_nested_threshold={THETA}", f"data.ss_nested_min_loop={MIN_LOOP}"]


@pytest.fixture(scope="module")
def runs(model, tmp_path_factory):
    root = tmp_path_factory.mktemp("ss_nested_cli")
    off = _run(model, root / "off", [])
    tdir = root / "targets"
    tdir.mkdir()
    for i in ("2DRB_1", "rnaB", "rnaC"):
        shutil.copy(root / "off" / "results" / "SS_result" / f"{i}.bpseq", tdir / f"{i}.bpseq")
    on = _run(model, root / "on", ON + [f"data.target_dir={tdir}"])
    off_target = _run(model, root / "off_target", [f"data.target_dir={tdir}"])
    bf16 = _run(model, root / "bf16", ON + ["data.ss_gemm_dtype=bf16"])
    return root, tdir, {"off": off, "on": on, "off_target": off_target, "bf16": bf16}


def _bpseq(data: bytes):
    rows = [ln.split() for ln in data.decode().splitlines()[1:]]
    return "".join(r[1] for r in rows), np.array([int(r[2]) for r in rows], dtype=np.int32)


def _check_against_the_truth(files, i):
    prob = np.loadtxt(io.BytesIO(files[f"SS_result/{i}.prob"]), delimiter="\t", ndmin=2).astype(np.float32)
    L = prob.shape[0]
    want_partner, _ = T.decode(prob, THETA, MIN_LOOP)
    head, seq, brackets = files[f"SS_result/{i}.dbn"].decode().split("\n")[:3]
    letters, partner = _bpseq(files[f"SS_result/{i}.nested.bpseq"])
    assert head == ">" + i and seq == letters and len(brackets) == L and files[f"SS_result/{i}.dbn"].count(b"\n") == 3
    assert T.partner_from_dbn(brackets).tolist() == partner.tolist() == want_partner.tolist(), i
    want_ct, want_bp, want_dbn = T.bodies(want_partner, seq)
    assert files[f"SS_result/{i}.nested.ct"] == f"{L}\t\t{i}\t\tRNAMSM_SS output\n\n".encode() + want_ct
    assert files[f"SS_result/{i}.nested.bpseq"] == f"#{i}\n".encode() + want_bp and brackets.encode() == want_dbn
    assert _bpseq(files[f"SS_result/{i}.bpseq"])[0] == seq                         # the letters .bpseq prints
    return want_partner


@pytest.mark.parametrize("run", ["on", "bf16"])
def test_the_three_files_equal_the_truth_on_the_prob_file_of_the_same_run(runs, run):
    files = runs[2][run]
    for i in IDS:
        _check_against_the_truth(files, i)
    assert sorted(f for f in files if f.endswith(NEW)) == sorted(f"SS_result/{i}{ext}" for i in IDS for ext in NEW)


def test_the_other_files_are_what_they_were_and_the_key_off_writes_nothing_new(runs):
    off, on, off_target = (runs[2][k] for k in ("off", "on", "off_target"))
    assert not [f for f in list(off) + list(off_target) if f.endswith(NEW) or "nested" in f]
    kept = {f: b for f, b in on.items() if not f.endswith(NEW) and "metrics" not in f}
    assert kept == off and any(f.endswith(".prob") for f in kept) and any(f.endswith(".ct") for f in kept)
    for f in (f for f in off_target if "metrics" in f):                      # with the key off the metrics files hold no such entry
        assert b"ss_nested" not in off_target[f]


def test_the_metrics_gain_an_entry_equal_to_structure_scores_of_the_truth(runs):
    _, tdir, all_runs = runs
    on, off_target = all_runs["on"], all_runs["off_target"]
    got = []
    for i in ("2DRB_1", "rnaB", "rnaC"):
        e = json.loads(on[f"{i}_metrics.json"])
        L = len(_bpseq(on[f"SS_result/{i}.bpseq"])[0])
        _, target = metrics.read_target(str(tdir / f"{i}.bpseq"), L)
        want = metrics.structure_scores(_check_against_the_truth(on, i), target)
        assert json.dumps(e["ss_nested"], sort_keys=True) == json.dumps({"L": L, **want}, sort_keys=True), i
        rest = {k: v for k, v in e.items() if k != "ss_nested"}
        assert json.dumps(rest, sort_keys=True) == json.dumps(json.loads(off_target[f"{i}_metrics.json"]), sort_keys=True)
        got.append(e["ss_nested"])
    s = json.loads(on["metrics_summary.json"])
    assert s["ss_nested"]["alignments"] == 3
    for n in ("precision", "recall", "F1"):
        vals = np.array([g[n] for g in got], dtype=np.float64)
        want = float(vals[~np.isnan(vals)].mean()) if not np.isnan(vals).all() else float("nan")
        assert s["ss_nested"][n] == want or (np.isnan(s["ss_nested"][n]) and np.isnan(want)), n
    rest = {k: v for k, v in s.items() if k != "ss_nested"}
    assert json.dumps(rest, sort_keys=True) == json.dumps(json.loads(off_target["metrics_summary.json"]), sort_keys=True)


def test_ss_predict_nested_writes_the_same_dbn(runs, tmp_path):
    root, _, all_runs = runs
    on = all_runs["on"]
    feat = tmp_path / "feat"
    feat.mkdir()
    seq, _ = _bpseq(on["SS_result/2DRB_1.bpseq"])
    (feat / "2DRB_1.fasta").write_text(f">2DRB_1\n{seq}\n")
    (feat / "2DRB_1_atp.npy").write_bytes(on["2DRB_1_atp.npy"])
    sys.path.insert(0, ROOT)
    try:
        import SS_predict
    finally:
        sys.path.remove(ROOT)
    with contextlib.redirect_stdout(io.StringIO()):
        SS_predict.main(["--rootdir", str(root / "on"), "--featdir", str(feat), "--rnaid", "2DRB_1", "--nested",
                         "--nested-threshold", str(THETA), "--nested-min-loop", str(MIN_LOOP)])
    for ext in NEW:
        assert (feat / "SS_result" / f"2DRB_1{ext}").read_bytes() == on[f"SS_result/2DRB_1{ext}"], ext
    with contextlib.redirect_stdout(io.StringIO()):
        SS_predict.main(["--rootdir", str(root / "on"), "--featdir", str(feat), "--rnaid", "2DRB_1"])        # without the flag: nothing new
    with pytest.raises(SystemExit, match="--nested-threshold"):
        SS_predict.main(["--rootdir", str(root / "on"), "--featdir", str(feat), "--rnaid", "2DRB_1", "--nested", "--nested-threshold", "1.5"])
