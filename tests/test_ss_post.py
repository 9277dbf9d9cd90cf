"""RNA-MSM-SS host side (rnamsm.ss), CPU only: the post-processing writes the reference's files byte for byte, and
SSPredictor carries the reference's parameter names and shapes."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from rnamsm import ss
from rnamsm.msa import read_fasta_records

SS_DIR = os.path.join(GOLDEN, "ss")


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_shipped_2drb1_files_are_reproduced(tmp_path):
    (name, seq), = read_fasta_records(os.path.join(SS_DIR, "2DRB_1.fasta"))
    prob = np.loadtxt(os.path.join(SS_DIR, "SS_result", "2DRB_1.prob"), delimiter="\t").astype(np.float32)
    ss.write_ss_files(prob, seq, name, tmp_path)
    for ext in ("bpseq", "prob"):
        assert _read(tmp_path / "SS_result" / f"2DRB_1.{ext}") == _read(os.path.join(SS_DIR, "SS_result", f"2DRB_1.{ext}")), ext
    got = _read(tmp_path / "SS_result" / "2DRB_1.ct").split(b"\n")
    want = _read(os.path.join(SS_DIR, "SS_result", "2DRB_1.ct")).split(b"\n")
    # the shipped file predates the current header wording; the code writes "RNAMSM_SS output"
    assert got[0] == b"35\t\t2DRB_1\t\tRNAMSM_SS output" and want[0] == b"35\t\t2DRB_1\t\tSPOT-RNA output"
    assert got[1:] == want[1:]


@pytest.mark.parametrize("case", ["multiplets", "threshold", "dense", "helix"])
def test_synthetic_cases_match_the_reference(tmp_path, case):
    g = np.load(os.path.join(GOLDEN, "ss_post_cases.npz"))
    ss.write_ss_files(g["prob_" + case], str(g["seq_" + case]), case, tmp_path)
    for ext, key in (("ct", "ct_"), ("bpseq", "bpseq_"), ("prob", "probtxt_")):
        assert _read(tmp_path / "SS_result" / f"{case}.{ext}") == g[key + case].tobytes(), ext


def test_multiplets_are_resolved_iteratively():
    p = np.zeros((6, 6), dtype=np.float32)
    p[0, 3], p[0, 4], p[1, 4], p[2, 4] = 0.9, 0.8, 0.7, 0.95
    # round 1: base 0 drops (0,4), base 4 drops (1,4) -> (0,3), (2,4) remain
    assert ss.secondary_structure(p) == [(0, 3), (2, 4)]
    assert ss.secondary_structure(p.T) == []             # the lower triangle is never read


def test_base_codes():
    assert ss.base_codes("ACGUacgtTNX-").tolist() == [0, 1, 2, 3] + [255] * 8


def test_predictor_loads_the_reference_state_dict_strictly():
    names = json.load(open(os.path.join(GOLDEN, "ss_renet_b16_state.json")))
    state = {n: torch.randn(s) for n, s in names}
    model = ss.SSPredictor()
    model.load_state_dict(state, strict=True)
    assert [(n, list(t.shape)) for n, t in model.state_dict().items()] == [(n, s) for n, s in names]
    bad = dict(state)
    bad["layer1.3.conv2.weight"] = torch.randn(48, 48, 3, 3)
    with pytest.raises(RuntimeError, match="size mismatch"):
        ss.SSPredictor().load_state_dict(bad, strict=True)
    missing = dict(state)
    del missing["fc1.bias"]
    with pytest.raises(RuntimeError, match="Missing"):
        ss.SSPredictor().load_state_dict(missing, strict=True)
    with pytest.raises(RuntimeError, match="Unexpected"):
        ss.SSPredictor(num_blocks=15).load_state_dict(state, strict=True)


def test_predictor_refuses_host_tensors():
    from rnamsm import _lib
    model = ss.SSPredictor(num_blocks=1)
    with pytest.raises(_lib.RnamsmError, match="HIP device"):
        model.predict(torch.zeros(120, 4, 4), "ACGU")


def test_ss_predict_refuses_plots_and_cpu(tmp_path):
    import subprocess
    import sys
    script = os.path.join(os.path.dirname(os.path.dirname(GOLDEN)), "SS_predict.py")
    for extra, msg in ((["--plots", "True"], "VARNA"), (["--device", "cpu"], "cuda")):
        r = subprocess.run([sys.executable, script, "--featdir", SS_DIR, "--rootdir", str(tmp_path)] + extra,
                           capture_output=True, text=True)
        assert r.returncode != 0 and msg in r.stderr, (r.returncode, r.stderr[-500:])
