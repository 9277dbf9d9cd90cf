"""data.sample_method=seqid-filter through the CLI on the GPU: on the shipped 64-row excerpt (tests/golden/2DRB_1_first64.a2m_msa2)
with data.max_seqs_per_msa below its depth, <id>_emb.npy and <id>_atp.npy are byte for byte those of a run with sample_method=first
over a pre-filtered copy of the alignment that holds the rows the plain-loop restatement (tests/seqid_filter_truth.py) keeps; the
statistics of the alignment as read (data.msa_stats) still see every row; and a list run with sample_method=first writes the same
bytes with and without the new keys at their defaults."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden
from rnamsm import msa, synthetic
import seqid_filter_truth as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP = 10
CAP = 16


@pytest.fixture(scope="module")
def model():
    from rnamsm.model import MSATransformer
    state = synthetic.make_state_dict(seed=0)
    m = MSATransformer(num_layers=10)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV)


@pytest.fixture(scope="module")
def records():
    return msa.read_fasta_records(os.path.join(GOLDEN, "2DRB_1_first64.a2m_msa2"))


def _run(model, root, alignments, overrides):
    """alignments: id -> the records of its file.  -> (files, printed with the run's own directory taken out)"""
    from rnamsm.config import Config, parse_overrides
    from rnamsm.inference import extract_feat
    (root / "results").mkdir(parents=True)
    for rna_id, recs in alignments.items():
        (root / "results" / f"{rna_id}.a2m_msa2").write_text("".join(f">{h}\n{s}\n" for h, s in recs))
    (root / "rna_id.txt").write_text("\n".join(alignments) + "\n")
    cfg = Config()
    cfg.data.root_path, cfg.data.MSA_path, cfg.data.MSA_list = str(root), "results", "rna_id.txt"
    cfg.data.max_seqs_per_msa = CAP
    cfg = parse_overrides(list(overrides), cfg)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        assert extract_feat(cfg, model=model) == sorted(alignments)
    files = {str(f.relative_to(root / "results")): f.read_bytes() for f in sorted((root / "results").rglob("*"))
             if f.is_file() and f.suffix != ".a2m_msa2"}
    return files, printed.getvalue().replace(str(root), "<root>")


@pytest.mark.parametrize("keys, schedule", [([], (20, 90, 5)), (["data.filter_min_seqid=50", "data.filter_max_seqid=85", "data.filter_step=35"], (50, 85, 35))])      # 30 kept, cut to 16; 13 kept, all of them
def test_the_filtered_run_equals_a_run_over_the_pre_filtered_alignment(model, records, tmp_path, keys, schedule):
    body = golden("tokens_2DRB_1_first64.npz")["tokens"][:, 1:].astype(np.uint8)
    kept, _, passes = T.seqid_filter(body, GAP, CAP, *schedule)
    rows = kept[:CAP]
    assert 1 < len(rows) <= CAP and list(rows) != list(range(len(rows))), (rows, passes)       # not what `first` would take
    got, printed = _run(model, tmp_path / "filtered", {"2DRB_1": records},
                        ["data.sample_method=seqid-filter", "data.msa_stats=true"] + keys)
    want, _ = _run(model, tmp_path / "pre", {"2DRB_1": [records[i] for i in rows]}, ["data.sample_method=first"])
    assert sorted(want) == ["2DRB_1_atp.npy", "2DRB_1_emb.npy"]
    for name in want:
        assert got[name] == want[name], name
    assert np.load(tmp_path / "filtered" / "results" / "2DRB_1_atp.npy").shape[-1] == 35
    # the alignment as read: every row, whatever the sub-sampling keeps
    w = np.load(tmp_path / "filtered" / "results" / "2DRB_1_weights.npy")
    assert w.shape == (64,) and np.array_equal(w, golden("msa_stats_reference_2drb64.npz")["weights"])
    assert "2DRB_1: 64 rows x 35 columns, Neff " in printed


def test_a_list_run_with_first_is_untouched_by_the_new_keys(model, records, tmp_path):
    tiny = [("q", "ACGU-ACG"), ("r", "ACGUUAC-"), ("s", "AC-UUACG")]
    alignments = {"2DRB_1": records, "rnaTiny": tiny, "rnaDeep": records[:40]}
    plain = _run(model, tmp_path / "plain", alignments, ["data.sample_method=first"])
    keyed = _run(model, tmp_path / "keyed", alignments, ["data.sample_method=first", "data.filter_min_seqid=20",
                                                         "data.filter_max_seqid=90", "data.filter_step=5"])
    assert plain == keyed and len(plain[0]) == 6
