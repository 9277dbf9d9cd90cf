"""data.mi / data.mi_gaps in the CLI loop (rnamsm.inference.extract_feat), on tests/golden/2DRB_1_first64.a2m_msa2 (64 rows x 35
columns) and an alignment of one row, with synthetic weights: the two files of an alignment are rnamsm.msa.msa_mi of the file's tokens
bit for bit -- every row, before the sub-sampling to 4, and the full width, before the crop to 32 columns; data.mi_gaps=state gives
the other map; the alignment of one row is refused with one line and keeps its other files; off, nothing differs."""
import contextlib
import io
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from rnamsm import msa, synthetic

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
    """-> (files, printed with the run's own directory taken out)"""
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
    with contextlib.redirect_stdout(printed):
        assert extract_feat(cfg, model=model) == sorted(IDS)
    files = {str(f.relative_to(root / "results")): f.read_bytes() for f in sorted((root / "results").rglob("*"))
             if f.is_file() and f.suffix != ".a2m_msa2"}
    return files, printed.getvalue().replace(str(root), "<root>")


@pytest.fixture(scope="module")
def runs(model, tmp_path_factory):
    root = tmp_path_factory.mktemp("mi_cli")
    return root, {name: _run(model, root / name, keys) for name, keys in (
        ("pairwise", ["data.mi=true"]), ("state", ["data.mi=true", "data.mi_gaps=state"]), ("absent", []), ("false", ["data.mi=false"]))}


def _tokens_of(path):
    from rnamsm.alphabet import RNAAlphabet
    from rnamsm.msa import load_msa_tokens
    return load_msa_tokens(path, RNAAlphabet(), None, "first")


@pytest.mark.parametrize("mode", ["pairwise", "state"])
def test_cli_writes_the_maps_of_the_alignment_as_read(runs, mode):
    root, by = runs
    files, printed = by[mode]
    tokens = _tokens_of(root / mode / "results" / "2DRB_1.a2m_msa2")
    assert tokens.shape == (64, 36)                                                  # every row, the full width and <cls>
    want = dict(zip(("mi", "mip"), msa.msa_mi(tokens, GAP, DEV, gaps=mode)))
    for kind in ("mi", "mip"):
        got = np.load(root / mode / "results" / f"2DRB_1_{kind}.npy")
        assert got.shape == (35, 35) and got.dtype == np.float64, kind               # the full width, whatever max_seqlen says
        assert got.tobytes() == want[kind].tobytes(), kind
    assert np.load(root / mode / "results" / "2DRB_1_emb.npy").shape[0] == MAX_SEQLEN - 1       # the forward was cropped
    # the maps come from every row: the first 4 rows alone give another map
    few = msa.msa_mi(tokens[:4], GAP, DEV, gaps=mode)[0]
    assert few.tobytes() != want["mi"].tobytes()
    # the alignment of one row is refused with one line that names the reason; its other files are written
    assert "rnaOne_mi.npy" not in files and "rnaOne_mip.npy" not in files and "rnaOne_emb.npy" in files and "rnaOne_atp.npy" in files
    lines = [ln for ln in printed.splitlines() if "rnaOne" in ln and "data.mi" in ln]
    assert len(lines) == 1 and "msa_mi: N=1 outside [2, 1048576]" in lines[0], printed


def test_mi_gaps_state_gives_the_other_map(runs):
    _, by = runs
    pairwise, state = by["pairwise"][0], by["state"][0]
    assert pairwise["2DRB_1_mi.npy"] != state["2DRB_1_mi.npy"] and pairwise["2DRB_1_mip.npy"] != state["2DRB_1_mip.npy"]
    assert {f: d for f, d in pairwise.items() if "_mi" not in f} == {f: d for f, d in state.items() if "_mi" not in f}


def test_cli_with_the_key_off_is_what_it_was(runs):
    _, by = runs
    assert by["absent"] == by["false"]                                               # the file set, every byte, and stdout
    files, printed = by["absent"]
    assert not any("_mi" in f for f in files) and "data.mi" not in printed and "mutual" not in printed
    on = by["pairwise"][0]
    assert {f: d for f, d in on.items() if "_mi" not in f} == files                  # the key adds files and changes none
    assert sorted(set(on) - set(files)) == ["2DRB_1_mi.npy", "2DRB_1_mip.npy"]
