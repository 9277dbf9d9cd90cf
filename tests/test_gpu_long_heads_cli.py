"""data.long_heads in the CLI, on the fixture of test_gpu_long_cli.py: one 70-column alignment and two short ones through
extract_feat with data.max_seqlen=33, data.long_msa=windows, an SS head of 4 blocks and data.contacts=true.  With
data.long_heads=stitched the wide alignment gets its contacts and its three SS files at the full L, made from the stitched atp by
the long entry points; everything else keeps its bytes."""
import contextlib
import io

import numpy as np
import pytest
import torch

import ss_truth
from rnamsm import ops, ss, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_SEQLEN = 33
SHAPES = {"rnaLong": (5, 70), "rnaA": (3, 20), "rnaB": (6, 32)}
KEYS = [f"data.max_seqlen={MAX_SEQLEN}", "data.lm_scores=wt", "data.long_msa=windows", "data.contacts=true"]
NB = 4


@pytest.fixture(scope="module")
def model():
    from rnamsm.model import MSATransformer
    state = synthetic.make_state_dict(seed=0, max_seqlen=MAX_SEQLEN)
    m = MSATransformer(num_layers=10, max_seqlen=MAX_SEQLEN)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV)


@pytest.fixture(scope="module")
def ss_state():
    return ss_truth.make_state(NB, seed=5)


def _tree(root):
    return {str(f.relative_to(root)): f.read_bytes() for f in sorted(root.rglob("*")) if f.is_file() and f.suffix != ".a2m_msa2"}


def _run(model, ss_state, root, overrides):
    """-> (files, printed)"""
    from rnamsm.config import Config, parse_overrides
    from rnamsm.inference import extract_feat
    rng = np.random.RandomState(11)
    (root / "results").mkdir(parents=True)
    for i, (depth, length) in SHAPES.items():
        text = "".join(f">s{r}\n{''.join(rng.choice(list('ACGU'), length))}\n" for r in range(depth))
        (root / "results" / f"{i}.a2m_msa2").write_text(text)
    (root / "rna_id.txt").write_text("\n".join(SHAPES) + "\n")
    ss_pt = root / "rna-msm_attention.pt"
    torch.save({k: torch.from_numpy(v) for k, v in ss_state.items()}, ss_pt)
    cfg = Config()
    cfg.data.root_path, cfg.data.MSA_path, cfg.data.MSA_list = str(root), "results", "rna_id.txt"
    cfg.data.sample_method, cfg.data.max_seqs_per_msa = "first", 64
    cfg = parse_overrides(KEYS + [f"data.ss_model_path={ss_pt}"] + list(overrides), cfg)
    real_load = ss.load_predictor
    printed = io.StringIO()
    with pytest.MonkeyPatch.context() as mp, contextlib.redirect_stdout(printed):
        mp.setattr(ss, "load_predictor", lambda path, device, num_blocks=NB: real_load(path, device, num_blocks))
        assert extract_feat(cfg, model=model) == sorted(SHAPES)
    return _tree(root / "results"), printed.getvalue()


@pytest.fixture(scope="module")
def runs(model, ss_state, tmp_path_factory):
    """The run with the key, and the run without it, once."""
    root = tmp_path_factory.mktemp("long_heads_cli")

    return (root, _run(model, ss_state, root / "on", ["data.long_heads=stitched"])[0],
            _run(model, ss_state, root / "off", [])[0])


def _skipped(printed: str, head: str):
    return [ln for ln in printed.splitlines() if "rnaLong" in ln and head in ln and "skipped" in ln]


def _ss_files(files, i):
    return {f.rsplit(".", 1)[1]: d for f, d in files.items() if f.startswith("SS_result/") and f"/{i}." in f}


def _host_files(probs: np.ndarray, seq: str, name: str, tmp) -> dict:
    ss.write_ss_files(probs, seq, name, tmp)
    return {ext: (tmp / "SS_result" / f"{name}.{ext}").read_bytes() for ext in ("ct", "bpseq", "prob")}


def _query(root) -> str:
    return (root / "results" / "rnaLong.a2m_msa2").read_text().splitlines()[1]


def test_contacts_of_the_wide_alignment_are_the_long_head_on_the_written_atp(model, runs):
    root, on, _ = runs
    atp = np.load(root / "on" / "results" / "rnaLong_atp.npy")
    got = np.load(root / "on" / "results" / "rnaLong_contacts.npy")
    assert atp.shape == (120, 70, 70) and got.shape == (70, 70) and got.dtype == np.float32
    reg = model.contact_head.regression
    want = ops.contact_head_long(torch.from_numpy(atp).to(DEV), reg.weight.detach(), reg.bias.detach())
    assert got.tobytes() == want.cpu().numpy().tobytes()


def test_ss_files_of_the_wide_alignment_are_the_host_path_on_the_head_s_probabilities(runs, ss_state, tmp_path):
    root, on, _ = runs
    files = _ss_files(on, "rnaLong")
    assert sorted(files) == ["bpseq", "ct", "prob"]
    seq = _query(root / "on")
    assert len(seq) == 70
    predictor = ss.SSPredictor(NB)
    predictor.load_state_dict({k: torch.from_numpy(v) for k, v in ss_state.items()}, strict=True)
    atp = torch.from_numpy(np.load(root / "on" / "results" / "rnaLong_atp.npy")).to(DEV)
    probs = predictor.eval().to(DEV).predict_long(atp, seq).cpu().numpy()
    assert files == _host_files(probs, seq, "rnaLong", tmp_path)
    assert len(files["prob"]) == 25 * 70 * 70


def test_everything_else_keeps_its_bytes(runs):
    _, on, off = runs
    new = {"rnaLong_contacts.npy", "SS_result/rnaLong.ct", "SS_result/rnaLong.bpseq", "SS_result/rnaLong.prob"}
    assert set(on) - set(off) == new and set(off) <= set(on)
    assert {f: d for f, d in on.items() if f not in new} == off           # the trunk files and the short alignments' files
    assert sum("rnaA" in f or "rnaB" in f for f in off) == 2 * (4 + 1 + 3)


def test_no_line_says_the_two_heads_were_skipped(model, ss_state, tmp_path):
    files, printed = _run(model, ss_state, tmp_path, ["data.long_heads=stitched"])
    assert not _skipped(printed, "SSHead") and not _skipped(printed, "ContactHead")
    assert "rnaLong_contacts.npy" in files


def test_under_bf16_the_ss_head_s_skip_line_is_back_and_the_contacts_are_still_written(model, ss_state, runs, tmp_path):
    files, printed = _run(model, ss_state, tmp_path, ["data.long_heads=stitched", "data.ss_gemm_dtype=bf16"])
    lines = _skipped(printed, "SSHead")
    assert len(lines) == 1 and "L=70" in lines[0] and "bf16" in lines[0], printed
    assert not _skipped(printed, "ContactHead")
    assert _ss_files(files, "rnaLong") == {} and len(_ss_files(files, "rnaA")) == 3
    assert files["rnaLong_contacts.npy"] == runs[1]["rnaLong_contacts.npy"]


def test_with_the_decoding_and_the_formatter_on_the_host_the_same_bytes_come_out(model, ss_state, runs, tmp_path):
    files, _ = _run(model, ss_state, tmp_path, ["data.long_heads=stitched", "data.ss_pairs_device=false", "data.ss_prob_text=false"])
    assert files == runs[1]
