"""data.mi_weights in the CLI loop (rnamsm.inference.extract_feat), on tests/golden/2DRB_1_first64.a2m_msa2 (64 rows x 35 columns) and
an alignment of one row, with synthetic weights: with data.mi=true data.mi_weights=seqid the two files <id>_wmi.npy / <id>_wmip.npy are
rnamsm.msa.msa_mi_weighted of the file's tokens bit for bit -- every row, before the sub-sampling to 4, and the full width, before the
crop to 32 columns -- and take the place of the unweighted pair; with data.msa_stats on as well the weights are made once; the
alignment of one row is refused with one line and keeps its other files; with the key absent or "none" the directory is what
data.mi=true gives, file for file and byte for byte."""
import contextlib
import io
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from rnamsm import msa, ops, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP = 10
MAX_SEQLEN = 33
IDS = ["2DRB_1", "rnaOne"]


@pytest.fixture(scope="module")
def model():
    from rnamsm.model import MSATransformer
    state = synthetic.make_state_dict(seed=0, max_seqlen=MAX_SEQLEN)
    m = MSATransformer(num_layers=10, max_seqlen=MAX_SEQLEN)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV)


def _run(model, root, overrides):
    """-> (files, printed with the run's own directory taken out, calls of ops.msa_neff)"""
    from rnamsm.config import Config, parse_overrides
    from rnamsm.inference import extract_feat
    (root / "results").mkdir(parents=True)
    shutil.copy(os.path.join(GOLDEN, "2DRB_1_first64.a2m_msa2"), root / "results" / "2DRB_1.a2m_msa2")
    (root / "results" / "rnaOne.a2m_msa2").write_text(">s0\nGGCCAUUGCACC\n")
    (root / "rna_id.txt").write_text("\n".join(IDS) + "\n")
    cfg = Config()
    cfg.data.root_path, cfg.data.MSA_path, cfg.data.MSA_list = str(root), "results", "rna_id.txt"
    cfg.data.sample_method, cfg.data.max_seqs_per_msa = "first", 4            # 2DRB_1 loses 60 of its 64 rows to the sub-sampling
    cfg = parse_overrides([f"data.max_seqlen={MAX_SEQLEN}"] + list(overrides), cfg)
    printed = io.StringIO()
    calls, real_neff = [], ops.msa_neff

    def counting(*args, **kwargs):
        calls.append(1)
        return real_neff(*args, **kwargs)

    ops.msa_neff = counting
    try:
        with contextlib.redirect_stdout(printed):
            assert extract_feat(cfg, model=model) == sorted(IDS)
    finally:
        ops.msa_neff = real_neff
    files = {str(f.relative_to(root / "results")): f.read_bytes() for f in sorted((root / "results").rglob("*"))
             if f.is_file() and f.suffix != ".a2m_msa2"}
    return files, printed.getvalue().replace(str(root), "<root>"), len(calls)


@pytest.fixture(scope="module")
def runs(model, tmp_path_factory):
    root = tmp_path_factory.mktemp("wmi_cli")
    return root, {name: _run(model, root / name, keys) for name, keys in (
        ("seqid", ["data.mi=true", "data.mi_weights=seqid"]),
        ("seqid_state_stats", ["data.mi=true", "data.mi_weights=seqid", "data.mi_gaps=state", "data.msa_stats=true"]),
        ("stats", ["data.mi=true", "data.msa_stats=true"]),
        ("plain", ["data.mi=true"]), ("none", ["data.mi=true", "data.mi_weights=none"]))}


def _tokens_of(path):
    from rnamsm.alphabet import RNAAlphabet
    from rnamsm.msa import load_msa_tokens
    return load_msa_tokens(path, RNAAlphabet(), None, "first")


@pytest.mark.parametrize("name,mode", [("seqid", "pairwise"), ("seqid_state_stats", "state")])
def test_cli_writes_the_weighted_maps_of_the_alignment_as_read(runs, name, mode):
    root, by = runs
    files, printed, _ = by[name]
    tokens = _tokens_of(root / name / "results" / "2DRB_1.a2m_msa2")
    assert tokens.shape == (64, 36)                                                  # every row, the full width and <cls>
    want = dict(zip(("wmi", "wmip"), msa.msa_mi_weighted(tokens, GAP, DEV, gaps=mode)))
    for kind in ("wmi", "wmip"):
        got = np.load(root / name / "results" / f"2DRB_1_{kind}.npy")
        assert got.shape == (35, 35) and got.dtype == np.float64, kind               # the full width, whatever max_seqlen says
        assert got.tobytes() == want[kind].tobytes(), kind
    assert "2DRB_1_mi.npy" not in files and "2DRB_1_mip.npy" not in files            # instead of the unweighted pair
    assert want["wmi"].tobytes() != msa.msa_mi(tokens, GAP, DEV, gaps=mode)[0].tobytes()
    assert np.load(root / name / "results" / "2DRB_1_emb.npy").shape[0] == MAX_SEQLEN - 1       # the forward was cropped
    # the alignment of one row is refused with one line that names the reason; its other files are written
    assert not any(f.startswith("rnaOne_wmi") or f.startswith("rnaOne_mi") for f in files) and "rnaOne_emb.npy" in files
    lines = [ln for ln in printed.splitlines() if "rnaOne" in ln and "data.mi" in ln]
    assert len(lines) == 1 and "msa_wmi: N=1 outside [2, 1048576]" in lines[0], printed


def test_with_msa_stats_the_weights_are_made_once(runs):
    _, by = runs
    assert by["seqid"][2] == len(IDS) and by["stats"][2] == len(IDS) and by["plain"][2] == 0
    assert by["seqid_state_stats"][2] == len(IDS)                                    # not twice per alignment
    both, stats = by["seqid_state_stats"][0], by["stats"][0]
    assert both["2DRB_1_weights.npy"] == stats["2DRB_1_weights.npy"] and both["2DRB_1_coverage.npy"] == stats["2DRB_1_coverage.npy"]
    drop = ("_mi.npy", "_mip.npy", "_wmi.npy", "_wmip.npy")
    assert {f: d for f, d in both.items() if not f.endswith(drop)} == {f: d for f, d in stats.items() if not f.endswith(drop)}


def test_cli_with_the_key_absent_or_none_is_what_it_was(runs):
    _, by = runs
    assert by["plain"][:2] == by["none"][:2]                                         # the file set, every byte, and stdout
    files, printed, _ = by["plain"]
    assert not any("_wmi" in f for f in files) and "2DRB_1_mi.npy" in files and "2DRB_1_mip.npy" in files
    on = by["seqid"][0]
    assert {f: d for f, d in on.items() if "_wmi" not in f} == {f: d for f, d in files.items() if "_mi" not in f}
    assert sorted(set(on) - set(files)) == ["2DRB_1_wmi.npy", "2DRB_1_wmip.npy"]
