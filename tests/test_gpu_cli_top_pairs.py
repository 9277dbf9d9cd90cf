"""data.top_pairs / data.top_pairs_min_sep in the CLI loop (rnamsm.inference.extract_feat), on tests/golden/2DRB_1_first64.a2m_msa2
(64 rows x 35 columns) and an alignment of one row, with synthetic weights and max_seqlen 33: beside every pair map an alignment gets,
<id>_<map>_top.txt is byte for byte format_top_pairs of the numpy truth (tests/top_pairs_truth.py) on the .npy file the run wrote, with
k resolved by THAT map's L; data.mi_weights=seqid moves the MI lists to the wmi / wmip names; a map that is refused leaves no list;
with the key absent or empty the files and the output are those of a run without it."""
import contextlib
import io
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from rnamsm import contacts, synthetic
import top_pairs_truth as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_SEQLEN = 33
IDS = ["2DRB_1", "rnaOne"]
BASE = ["data.mi=true", "data.invcov=true", "data.contacts=true"]
SPEC, MIN_SEP = "1.5L", 3


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
    cfg.data.sample_method, cfg.data.max_seqs_per_msa = "first", 4
    cfg = parse_overrides([f"data.max_seqlen={MAX_SEQLEN}"] + list(overrides), cfg)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        assert extract_feat(cfg, model=model) == sorted(IDS)
    files = {str(f.relative_to(root / "results")): f.read_bytes() for f in sorted((root / "results").rglob("*"))
             if f.is_file() and f.suffix != ".a2m_msa2"}
    return files, printed.getvalue().replace(str(root), "<root>")


@pytest.fixture(scope="module")
def runs(model, tmp_path_factory):
    root = tmp_path_factory.mktemp("top_pairs_cli")
    on = [f"data.top_pairs={SPEC}", f"data.top_pairs_min_sep={MIN_SEP}"]
    return root, {name: _run(model, root / name, keys) for name, keys in (
        ("on", BASE + on), ("weighted", BASE + on + ["data.mi_weights=seqid"]), ("absent", BASE),
        ("empty", BASE + ["data.top_pairs=", f"data.top_pairs_min_sep={MIN_SEP}"]))}


def _expected(root, run, rna_id, kind):
    x = np.load(root / run / "results" / f"{rna_id}_{kind}.npy")
    assert x.ndim == 2 and x.shape[0] == x.shape[1]
    k = contacts.top_pairs_k(SPEC, x.shape[0])
    pairs, scores = T.truth(x, k, MIN_SEP)
    return contacts.format_top_pairs(pairs, scores, MIN_SEP).encode(), x, k


@pytest.mark.parametrize("run,kinds", [("on", ("contacts", "invcov", "mi", "mip")), ("weighted", ("contacts", "invcov", "wmi", "wmip"))])
def test_a_list_beside_every_pair_map(runs, run, kinds):
    root, by = runs
    files, printed = by[run]
    for kind in kinds:
        want, x, k = _expected(root, run, "2DRB_1", kind)
        # k from the map's own L: the alignment's 35 columns for the maps of the alignment as read, the cropped 32 for the contacts
        assert (x.shape[0], k) == ((32, 48) if kind == "contacts" else (35, 53)), kind
        assert x.dtype == (np.float32 if kind == "contacts" else np.float64)
        got = files[f"2DRB_1_{kind}_top.txt"]
        assert got == want, (kind, got[:200], want[:200])
        lines = got.decode().splitlines()
        assert lines[0] == f"# i j score (1-based, j - i >= {MIN_SEP})" and 1 < len(lines) <= k + 1
    tops = sorted(f for f in files if f.endswith("_top.txt"))
    # the alignment of one row: data.mi and data.invcov refuse it (one line each, no map, so no list); its contacts list is there
    assert tops == sorted([f"2DRB_1_{kind}_top.txt" for kind in kinds] + ["rnaOne_contacts_top.txt"]), tops
    assert files["rnaOne_contacts_top.txt"] == _expected(root, run, "rnaOne", "contacts")[0]
    assert "rnaOne_emb.npy" in files and "rnaOne_atp.npy" in files and "rnaOne_contacts.npy" in files
    lines = [ln for ln in printed.splitlines() if "rnaOne" in ln and "data.mi" in ln]
    assert len(lines) == 1 and "N=1 outside [2, 1048576]" in lines[0], printed
    other = {"mi", "mip", "wmi", "wmip"} - set(kinds)
    assert not any(f"_{kind}_top.txt" in f or f"_{kind}.npy" in f for f in files for kind in other)


def test_the_lists_change_no_other_file(runs):
    _, by = runs
    on, absent = by["on"][0], by["absent"][0]
    assert {f: d for f, d in on.items() if not f.endswith("_top.txt")} == absent
    assert by["on"][1] == by["absent"][1]                                             # nothing more is printed either


def test_cli_with_the_key_absent_or_empty_is_what_it_was(runs):
    _, by = runs
    assert by["absent"] == by["empty"]                                               # the file set, every byte, and stdout
    files, printed = by["absent"]
    assert not any(f.endswith("_top.txt") for f in files) and "top_pairs" not in printed


def test_a_map_that_cannot_have_a_list_is_skipped_with_one_line(model, tmp_path):
    files, printed = _run(model, tmp_path / "big", BASE + ["data.top_pairs=65537"])
    assert not any(f.endswith("_top.txt") for f in files)
    lines = [ln for ln in printed.splitlines() if "data.top_pairs" in ln]
    assert len(lines) == 5 and all("k=65537 exceeds 65536" in ln for ln in lines), printed      # four maps of 2DRB_1, one of rnaOne
    assert {f: d for f, d in files.items()} == {f: d for f, d in _run(model, tmp_path / "plain", BASE)[0].items()}
