"""data.contacts in the CLI: three tiny alignments of unlike (depth, length) through extract_feat.  Every <id>_contacts.npy is, byte
for byte, model.predict_contacts on that alignment's own tokens; the tree does not depend on data.batch_small_msas; and with the key
absent there is no such file and the other files are those of a run with the key."""
import numpy as np
import pytest
import torch

from rnamsm import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"rnaA": (3, 20), "rnaB": (6, 35), "rnaC": (2, 12)}


@pytest.fixture(scope="module")
def model():
    from rnamsm.model import MSATransformer
    state = synthetic.make_state_dict(seed=0)
    m = MSATransformer(num_layers=10)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV)


def _tree(root):
    return {str(f.relative_to(root)): f.read_bytes() for f in sorted(root.rglob("*")) if f.is_file() and f.suffix == ".npy"}


def _run(model, root, contacts, batching=True):
    from rnamsm.config import Config, parse_overrides
    from rnamsm.inference import extract_feat
    rng = np.random.RandomState(7)
    (root / "results").mkdir(parents=True)
    for i, (depth, length) in SHAPES.items():
        text = "".join(f">s{r}\n{''.join(rng.choice(list('ACGU'), length))}\n" for r in range(depth))
        (root / "results" / f"{i}.a2m_msa2").write_text(text)
    (root / "rna_id.txt").write_text("\n".join(SHAPES) + "\n")
    cfg = Config()
    cfg.data.root_path, cfg.data.MSA_path, cfg.data.MSA_list = str(root), "results", "rna_id.txt"
    cfg.data.sample_method, cfg.data.max_seqs_per_msa, cfg.data.batch_small_msas = "first", 64, batching
    if contacts is not None:
        cfg = parse_overrides([f"data.contacts={contacts}"], cfg)
    assert extract_feat(cfg, model=model) == sorted(SHAPES)
    return _tree(root / "results")


def test_contacts_files_are_the_model_s_own_contacts_whatever_the_batching(model, tmp_path):
    from rnamsm.alphabet import RNAAlphabet
    from rnamsm.config import Config
    from rnamsm.msa import load_msa_tokens
    batched = _run(model, tmp_path / "batched", "true", True)
    plain = _run(model, tmp_path / "plain", "true", False)
    assert batched == plain                                       # the whole tree, byte for byte
    assert sorted(batched) == sorted(f"{i}_{kind}.npy" for i in SHAPES for kind in ("atp", "contacts", "emb"))
    alphabet = RNAAlphabet.from_architecture(Config().data.architecture)
    for i, (_, length) in SHAPES.items():
        got = np.load(tmp_path / "batched" / "results" / f"{i}_contacts.npy")
        assert got.shape == (length, length) and got.dtype == np.float32 and got.flags["C_CONTIGUOUS"]
        toks = torch.from_numpy(load_msa_tokens(tmp_path / "batched" / "results" / f"{i}.a2m_msa2", alphabet, 64, "first")).to(DEV)
        with torch.no_grad():
            want = model.predict_contacts(toks[None])[0].cpu().numpy()
        assert got.tobytes() == want.tobytes(), i
        assert np.isfinite(got).all() and 0.0 < got.min() and got.max() < 1.0
    # the key absent, and the key set to false: no contacts file, the other files unchanged
    for name, value in (("absent", None), ("off", "false")):
        off = _run(model, tmp_path / name, value)
        assert not [f for f in off if f.endswith("_contacts.npy")]
        assert off == {f: data for f, data in batched.items() if not f.endswith("_contacts.npy")}
