"""data.long_msa in the CLI: a list of one 70-column alignment and two short ones through extract_feat with data.max_seqlen=33.
With data.long_msa=windows the wide alignment's files hold the full L and are MSATransformer.forward_windows on its tokens, bit for
bit; with the key off they are the reference's crop; the short alignments' files are the same bytes either way.  lm_scores=wt runs
on the stitched emb; the SS and contact heads are skipped for the wide alignment with one printed line each and still run on the
others."""
import io

import numpy as np
import pytest
import torch

import ss_truth
from rnamsm import lm, ss, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_SEQLEN = 33
SHAPES = {"rnaLong": (5, 70), "rnaA": (3, 20), "rnaB": (6, 32)}          # rnaB: exactly max_seqlen columns with <cls> -- not wide
KEYS = [f"data.max_seqlen={MAX_SEQLEN}", "data.lm_scores=wt"]


@pytest.fixture(scope="module")
def model():
    from rnamsm.model import MSATransformer
    state = synthetic.make_state_dict(seed=0, max_seqlen=MAX_SEQLEN)
    m = MSATransformer(num_layers=10, max_seqlen=MAX_SEQLEN)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV)


def _tree(root):
    return {str(f.relative_to(root)): f.read_bytes() for f in sorted(root.rglob("*")) if f.is_file() and f.suffix != ".a2m_msa2"}


def _run(model, root, overrides):
    from rnamsm.config import Config, parse_overrides
    from rnamsm.inference import extract_feat
    rng = np.random.RandomState(11)
    (root / "results").mkdir(parents=True)
    for i, (depth, length) in SHAPES.items():
        text = "".join(f">s{r}\n{''.join(rng.choice(list('ACGU'), length))}\n" for r in range(depth))
        (root / "results" / f"{i}.a2m_msa2").write_text(text)
    (root / "rna_id.txt").write_text("\n".join(SHAPES) + "\n")
    cfg = Config()
    cfg.data.root_path, cfg.data.MSA_path, cfg.data.MSA_list = str(root), "results", "rna_id.txt"
    cfg.data.sample_method, cfg.data.max_seqs_per_msa = "first", 64
    cfg = parse_overrides(list(overrides), cfg)
    assert extract_feat(cfg, model=model) == sorted(SHAPES)
    return _tree(root / "results")


def _tokens(root, name):
    from rnamsm.alphabet import RNAAlphabet
    from rnamsm.config import Config
    from rnamsm.msa import load_msa_tokens
    alphabet = RNAAlphabet.from_architecture(Config().data.architecture)
    return torch.from_numpy(load_msa_tokens(root / "results" / f"{name}.a2m_msa2", alphabet, 64, "first")).to(DEV)


@pytest.fixture(scope="module")
def runs(model, tmp_path_factory):
    root = tmp_path_factory.mktemp("long_cli")
    return root, _run(model, root / "on", KEYS + ["data.long_msa=windows"]), _run(model, root / "off", KEYS)


def _short(files):
    return {f: data for f, data in files.items() if "rnaLong" not in f}


def test_windows_write_the_full_length_and_are_forward_windows(model, runs):
    root, on, _ = runs
    D, NLH = model.embed_dim, model.num_layers * model.num_attention_heads
    emb, atp = np.load(root / "on" / "results" / "rnaLong_emb.npy"), np.load(root / "on" / "results" / "rnaLong_atp.npy")
    assert emb.shape == (70, D) and atp.shape == (NLH, 70, 70) and emb.dtype == atp.dtype == np.float32
    toks = _tokens(root / "on", "rnaLong")
    assert tuple(toks.shape) == (5, 71)
    want = model.forward_windows(toks)
    assert emb.tobytes() == want["emb"].cpu().numpy().tobytes() and atp.tobytes() == want["atp"].cpu().numpy().tobytes()
    assert np.isfinite(emb).all() and np.isfinite(atp).all()
    # lm_scores=wt ran on the stitched emb: 70 rows, the lone head on the written file
    scores, nll = np.load(root / "on" / "results" / "rnaLong_lm_scores.npy"), np.load(root / "on" / "results" / "rnaLong_lm_nll.npy")
    assert scores.shape == (70, len(model.vocab)) and nll.shape == (70,)
    head = lm.kernel_of(model).rows(torch.from_numpy(emb).to(DEV), None, toks[0, 1:], want=("scores", "nll"))
    assert scores.tobytes() == head["scores"].cpu().numpy().tobytes() and nll.tobytes() == head["nll"].cpu().numpy().tobytes()


def test_with_the_key_off_the_wide_alignment_is_cropped_as_before(model, runs):
    root, _, off = runs
    D, NLH = model.embed_dim, model.num_layers * model.num_attention_heads
    emb, atp = np.load(root / "off" / "results" / "rnaLong_emb.npy"), np.load(root / "off" / "results" / "rnaLong_atp.npy")
    assert emb.shape == (MAX_SEQLEN - 1, D) and atp.shape == (NLH, MAX_SEQLEN - 1, MAX_SEQLEN - 1)
    assert np.load(root / "off" / "results" / "rnaLong_lm_scores.npy").shape == (MAX_SEQLEN - 1, len(model.vocab))
    # the reference's draw: the first and only crop of the RandomState(42) stream ("first" sub-sampling draws nothing)
    from rnamsm.inference import crop_tokens
    toks = _tokens(root / "off", "rnaLong")
    cropped = torch.from_numpy(crop_tokens(toks.cpu().numpy(), MAX_SEQLEN, np.random.RandomState(42))).to(DEV)
    want = model.checked_forward_one(cropped, need_repr=False)
    assert emb.tobytes() == want["emb"].cpu().numpy().tobytes() and atp.tobytes() == want["atp"].cpu().numpy().tobytes()


def test_the_short_alignments_have_the_same_bytes_either_way(runs):
    _, on, off = runs
    kinds = ("atp", "emb", "lm_nll", "lm_scores")
    assert sorted(on) == sorted(off) == sorted(f"{i}_{k}.npy" for i in SHAPES for k in kinds)
    assert _short(on) == _short(off) and len(_short(on)) == 8
    assert np.load(io.BytesIO(on["rnaB_emb.npy"])).shape[0] == 32


def test_a_window_stride_of_the_users_choice(model, tmp_path):
    files = _run(model, tmp_path, KEYS + ["data.long_msa=windows", "data.window_stride=32"])
    want = model.forward_windows(_tokens(tmp_path, "rnaLong"), stride=32)
    assert np.load(io.BytesIO(files["rnaLong_emb.npy"])).shape[0] == 70
    assert np.load(tmp_path / "results" / "rnaLong_emb.npy").tobytes() == want["emb"].cpu().numpy().tobytes()
    assert np.load(tmp_path / "results" / "rnaLong_atp.npy").tobytes() == want["atp"].cpu().numpy().tobytes()
    with pytest.raises(ValueError, match=r"\[16, 32\]"):
        _run(model, tmp_path / "bad", KEYS + ["data.long_msa=windows", "data.window_stride=5"])


def test_heads_with_a_length_limit_are_skipped_for_the_wide_alignment_only(model, runs, tmp_path, monkeypatch, capsys):
    root, on, _ = runs
    ss_pt = tmp_path / "rna-msm_attention.pt"
    torch.save({k: torch.from_numpy(v) for k, v in ss_truth.make_state(4, seed=5).items()}, ss_pt)
    real_load = ss.load_predictor
    monkeypatch.setattr(ss, "load_predictor", lambda path, device, num_blocks=4: real_load(path, device, num_blocks))
    heads = [f"data.ss_model_path={ss_pt}", "data.contacts=true"]
    capsys.readouterr()
    win = _run(model, tmp_path / "on", KEYS + heads + ["data.long_msa=windows"])
    printed = capsys.readouterr().out
    crop = _run(model, tmp_path / "off", KEYS + heads)
    for head in ("SSHead", "ContactHead"):
        lines = [ln for ln in printed.splitlines() if "rnaLong" in ln and "L=70" in ln and head in ln and "skipped" in ln]
        assert len(lines) == 1, printed
    assert "LMHead" not in printed
    ss_files = lambda files, i: sorted(f for f in files if f.startswith("SS_result/") and f"/{i}." in f)      # noqa: E731
    assert ss_files(win, "rnaLong") == [] and "rnaLong_contacts.npy" not in win
    assert len(ss_files(crop, "rnaLong")) == 3 and "rnaLong_contacts.npy" in crop
    for i in ("rnaA", "rnaB"):
        assert len(ss_files(win, i)) == 3 and f"{i}_contacts.npy" in win
    assert _short(win) == _short(crop)
    # and the trunk's files do not depend on which heads are on
    assert {f: d for f, d in win.items() if f in on} == on
