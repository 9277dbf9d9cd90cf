"""data.lm_scores in the CLI: one lone (above the packing threshold) and three packed small alignments through extract_feat.  "wt":
every <id>_lm_scores.npy / <id>_lm_nll.npy is, bit for bit, the lone head on that alignment's written <id>_emb.npy, and the other
files are those of a run with the key off; "masked": the files are likelihood.scan on the alignment's tokens; with data.contacts as
well both heads' files are written."""
import numpy as np
import pytest
import torch

from rnamsm import likelihood, lm, ops, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"rnaA": (3, 20), "rnaB": (6, 35), "rnaC": (2, 12), "rnaBig": (64, 256)}     # rnaBig: 64 x 257 tokens > 16384, a lone forward


@pytest.fixture(scope="module")
def model():
    from rnamsm.model import MSATransformer
    state = synthetic.make_state_dict(seed=0)
    m = MSATransformer(num_layers=10)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV)


def _tree(root):
    return {str(f.relative_to(root)): f.read_bytes() for f in sorted(root.rglob("*")) if f.is_file() and f.suffix == ".npy"}


def _run(model, root, shapes, overrides=()):
    from rnamsm.config import Config, parse_overrides
    from rnamsm.inference import extract_feat
    rng = np.random.RandomState(7)
    (root / "results").mkdir(parents=True)
    for i, (depth, length) in shapes.items():
        text = "".join(f">s{r}\n{''.join(rng.choice(list('ACGU'), length))}\n" for r in range(depth))
        (root / "results" / f"{i}.a2m_msa2").write_text(text)
    (root / "rna_id.txt").write_text("\n".join(shapes) + "\n")
    cfg = Config()
    cfg.data.root_path, cfg.data.MSA_path, cfg.data.MSA_list = str(root), "results", "rna_id.txt"
    cfg.data.sample_method, cfg.data.max_seqs_per_msa = "first", 64
    cfg = parse_overrides(list(overrides), cfg)
    assert extract_feat(cfg, model=model) == sorted(shapes)
    return _tree(root / "results")


def _tokens(root, name):
    from rnamsm.alphabet import RNAAlphabet
    from rnamsm.config import Config
    from rnamsm.msa import load_msa_tokens
    alphabet = RNAAlphabet.from_architecture(Config().data.architecture)
    return torch.from_numpy(load_msa_tokens(root / "results" / f"{name}.a2m_msa2", alphabet, 64, "first")).to(DEV)


def _check_wt_files(model, root, shapes):
    head = lm.kernel_of(model)
    for i, (_, length) in shapes.items():
        scores, nll = np.load(root / "results" / f"{i}_lm_scores.npy"), np.load(root / "results" / f"{i}_lm_nll.npy")
        assert scores.shape == (length, len(model.vocab)) and nll.shape == (length,)
        assert scores.dtype == nll.dtype == np.float32 and scores.flags["C_CONTIGUOUS"]
        emb = torch.from_numpy(np.load(root / "results" / f"{i}_emb.npy")).to(DEV)
        toks = _tokens(root, i)
        want = head.rows(emb, None, toks[0, 1:], want=("scores", "nll"))
        assert scores.tobytes() == want["scores"].cpu().numpy().tobytes(), i
        assert nll.tobytes() == want["nll"].cpu().numpy().tobytes(), i
        assert np.isfinite(scores).all() and (scores[np.arange(length), toks[0, 1:].cpu().numpy()] == 0.0).all() and (nll > 0).all()


def test_wt_scores_are_the_lone_head_on_the_written_emb_and_change_no_other_file(model, tmp_path):
    on = _run(model, tmp_path / "on", SHAPES, ["data.lm_scores=wt"])
    off = _run(model, tmp_path / "off", SHAPES)
    assert sorted(on) == sorted(f"{i}_{kind}.npy" for i in SHAPES for kind in ("atp", "emb", "lm_nll", "lm_scores"))
    assert off == {f: data for f, data in on.items() if "_lm_" not in f}           # emb and atp: byte-identical, no LM file when off
    _check_wt_files(model, tmp_path / "on", SHAPES)


def test_masked_scores_are_the_scan_and_say_what_they_cost(model, tmp_path, capsys):
    shapes = {"rnaM": (8, 16)}                                                         # 8 x 17 tokens
    files = _run(model, tmp_path, shapes, ["data.lm_scores=masked"])
    printed = capsys.readouterr().out
    assert "lm_scores=masked" in printed and "16 further forwards" in printed
    assert sorted(files) == ["rnaM_atp.npy", "rnaM_emb.npy", "rnaM_lm_nll.npy", "rnaM_lm_scores.npy"]
    s = likelihood.scan(model, _tokens(tmp_path, "rnaM"))
    assert np.load(tmp_path / "results" / "rnaM_lm_scores.npy").tobytes() == s.scores.cpu().numpy().tobytes()
    assert np.load(tmp_path / "results" / "rnaM_lm_nll.npy").tobytes() == s.nll.cpu().numpy().tobytes()
    assert s.scores.shape == (16, len(model.vocab)) and torch.isfinite(s.scores).all()


def test_with_the_contact_head_on_as_well_both_heads_write_their_own(model, tmp_path):
    shapes = {k: SHAPES[k] for k in ("rnaA", "rnaB", "rnaC")}
    files = _run(model, tmp_path, shapes, ["data.lm_scores=wt", "data.contacts=true"])
    assert sorted(files) == sorted(f"{i}_{kind}.npy" for i in shapes for kind in ("atp", "contacts", "emb", "lm_nll", "lm_scores"))
    _check_wt_files(model, tmp_path, shapes)
    for i, (_, length) in shapes.items():
        atp = torch.from_numpy(np.load(tmp_path / "results" / f"{i}_atp.npy")).to(DEV)
        reg = model.contact_head.regression
        want = ops.contact_head_atp(atp, reg.weight.detach(), reg.bias.detach()).cpu().numpy()
        assert np.load(tmp_path / "results" / f"{i}_contacts.npy").tobytes() == want.tobytes(), i
