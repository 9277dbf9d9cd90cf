"""The CLI key data.msa_stats on the GPU: the shipped 64-row excerpt (tests/golden/2DRB_1_first64.a2m_msa2) with the key on writes
<id>_weights.npy and <id>_coverage.npy with the values of the reference's own MSA class (tests/golden/msa_stats_reference_2drb64.npz),
bit for bit, for the alignment as read -- every row, although the forward runs on 16 of them -- and prints the line with Neff; with the
key off or absent the printed lines and the files are what they were, and the key on adds to them and changes none."""
import contextlib
import io
import math
import os
import re
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden
from rnamsm import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = ["2DRB_1", "rnaTiny"]


@pytest.fixture(scope="module")
def model():
    from rnamsm.model import MSATransformer
    state = synthetic.make_state_dict(seed=0)
    m = MSATransformer(num_layers=10)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV)


def _run(model, root, overrides):
    """-> (files, printed with the run's own directory taken out)"""
    from rnamsm.config import Config, parse_overrides
    from rnamsm.inference import extract_feat
    (root / "results").mkdir(parents=True)
    shutil.copy(os.path.join(GOLDEN, "2DRB_1_first64.a2m_msa2"), root / "results" / "2DRB_1.a2m_msa2")
    (root / "results" / "rnaTiny.a2m_msa2").write_text(">q\nACGU-ACG\n>r\nACGUUAC-\n>s\nAC-UUACG\n")
    (root / "rna_id.txt").write_text("\n".join(IDS) + "\n")
    cfg = Config()
    cfg.data.root_path, cfg.data.MSA_path, cfg.data.MSA_list = str(root), "results", "rna_id.txt"
    cfg.data.sample_method, cfg.data.max_seqs_per_msa = "first", 16           # the forward sees 16 of the 64 rows
    cfg = parse_overrides(list(overrides), cfg)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        assert extract_feat(cfg, model=model) == sorted(IDS)
    files = {str(f.relative_to(root / "results")): f.read_bytes() for f in sorted((root / "results").rglob("*"))
             if f.is_file() and f.suffix != ".a2m_msa2"}
    return files, printed.getvalue().replace(str(root), "<root>")


@pytest.fixture(scope="module")
def runs(model, tmp_path_factory):
    root = tmp_path_factory.mktemp("msa_stats_cli")
    return root, {name: _run(model, root / name, keys) for name, keys in (
        ("on", ["data.msa_stats=true"]), ("absent", []), ("false", ["data.msa_stats=false"]))}


def test_cli_writes_the_references_values_and_prints_the_line(runs):
    root, by = runs
    files, printed = by["on"]
    g = golden("msa_stats_reference_2drb64.npz")
    w, c = np.load(root / "on" / "results" / "2DRB_1_weights.npy"), np.load(root / "on" / "results" / "2DRB_1_coverage.npy")
    assert w.dtype == np.float64 and c.dtype == np.float64 and w.shape == (64,) and c.shape == (35,)
    assert np.array_equal(w, g["weights"]) and np.array_equal(c, g["coverage"])
    lines = [ln for ln in printed.splitlines() if ln.startswith("2DRB_1: ")]
    assert len(lines) == 1, printed
    m = re.fullmatch(r"2DRB_1: 64 rows x 35 columns, Neff ([0-9.]+) \(Neff/sqrt\(L\) ([0-9.]+), Neff/L ([0-9.]+)\)", lines[0])
    assert m, lines[0]
    neff = float(g["neff_none"])
    assert m.group(1) == f"{neff:.3f}" and m.group(2) == f"{neff / math.sqrt(35):.3f}" and m.group(3) == f"{neff / 35:.4f}"
    # the second alignment: three rows of eight columns, one gap each in three columns
    assert np.array_equal(np.load(root / "on" / "results" / "rnaTiny_coverage.npy"), np.array([1, 1, 2 / 3, 1, 2 / 3, 1, 1, 2 / 3]))
    assert len([ln for ln in printed.splitlines() if ln.startswith("rnaTiny: 3 rows x 8 columns, Neff ")]) == 1


def test_cli_with_the_key_off_is_what_it_was(runs):
    _, by = runs
    assert by["absent"] == by["false"]                                               # the file set, every byte, and stdout
    files, printed = by["absent"]
    assert not any("weights" in f or "coverage" in f for f in files) and "Neff" not in printed
    on, on_printed = by["on"]
    assert {f: d for f, d in on.items() if f in files} == files                      # the key adds files and changes none
    assert sorted(set(on) - set(files)) == ["2DRB_1_coverage.npy", "2DRB_1_weights.npy", "rnaTiny_coverage.npy", "rnaTiny_weights.npy"]
    assert [ln for ln in on_printed.splitlines() if "Neff" not in ln] == printed.splitlines()      # ... and lines, and changes none
