"""data.rsa_model_dir beside data.long_msa=windows data.long_heads=stitched in the CLI, on the fixture of test_gpu_long_heads_cli.py:
one 70-column alignment and two short ones through extract_feat with data.max_seqlen=33 (windows of 32), and RSA_predict.py on an
embedding of more than 1024 rows.  With data.long_heads=stitched the wide alignment gets its RSA_result tables at the full L, made from the stitched emb by the long entry
points; with data.long_heads=skip the skip line and the files are what they were; the narrow alignments keep their bytes."""
import contextlib
import io
import pickle
import random

import numpy as np
import pytest
import torch

import rsa_text_cases as C
import rsa_truth as T
from rnamsm import rsa, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_SEQLEN = 33
SHAPES = {"rnaLong": (5, 70), "rnaA": (3, 20), "rnaB": (6, 32)}
KEYS = [f"data.max_seqlen={MAX_SEQLEN}", "data.long_msa=windows"]


@pytest.fixture(scope="module")
def model():
    from rnamsm.model import MSATransformer
    state = synthetic.make_state_dict(seed=0, max_seqlen=MAX_SEQLEN)
    m = MSATransformer(num_layers=10, max_seqlen=MAX_SEQLEN)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV)


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("rsa_models") / "OH+RNA-MSM_Emb"
    d.mkdir()
    for k in range(3):
        torch.save({n: torch.from_numpy(v) for n, v in T.load_state(f"state_oh_{k}").items()}, d / f"model_pcc_{k}_1{k}=0.5.pt")
    st = T.load_stats("oh")
    with open(d / "statistic_dict_oh.pickle", "wb") as f:
        pickle.dump({"mu": st["oh_mu"], "std": st["oh_std"]}, f)
    with open(d / "statistic_dict_emb.pickle", "wb") as f:
        pickle.dump({"mu": st["emb_mu"], "std": st["emb_std"]}, f)
    return d


def _run(model, model_dir, root, overrides):
    """-> (files under results/, printed)"""
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
    cfg = parse_overrides(KEYS + [f"data.rsa_model_dir={model_dir}"] + list(overrides), cfg)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        assert extract_feat(cfg, model=model) == sorted(SHAPES)
    files = {str(f.relative_to(root / "results")): f.read_bytes() for f in sorted((root / "results").rglob("*"))
             if f.is_file() and f.suffix != ".a2m_msa2"}
    return files, printed.getvalue()


@pytest.fixture(scope="module")
def runs(model, model_dir, tmp_path_factory):
    """The run with the key, the same with the tables formatted on the host, and the run without the key, once each."""
    root = tmp_path_factory.mktemp("rsa_long_cli")
    return (root, _run(model, model_dir, root / "on", ["data.long_heads=stitched"]),
            _run(model, model_dir, root / "host", ["data.long_heads=stitched", "data.rsa_text_device=false"]),
            _run(model, model_dir, root / "off", []))


def _tables(i):
    return {f"RSA_result/{i}_{tag}/{i}.txt" for tag in ("0", "1", "2", "ensemble")}


def _skipped(printed: str):
    return [ln for ln in printed.splitlines() if "rnaLong" in ln and "RSAHead" in ln and "skipped" in ln]


def test_the_wide_alignment_s_tables_are_the_host_path_on_the_written_emb(runs, model_dir, tmp_path):
    root, (on, printed), _, _ = runs
    assert _tables("rnaLong") <= set(on) and not _skipped(printed)
    emb = np.load(root / "on" / "results" / "rnaLong_emb.npy")
    seq = (root / "on" / "results" / "rnaLong.a2m_msa2").read_text().splitlines()[1]
    assert emb.shape == (70, 768) and len(seq) == 70
    ens = rsa.load_ensemble(model_dir, DEV)
    values = ens.predict(torch.from_numpy(emb).to(DEV), seq).cpu().numpy()
    # the generator behind the two short alignments' draws (a draw only decides what replaces a letter outside ACGU: none here)
    rng = random.Random(2022)
    [rng.randint(0, 3) for _ in range(2 * (len(ens) + 1))]
    rsa.write_rsa_files(values, seq, "rnaLong", tmp_path, ens.model_names, rng)
    want = {k.replace("\\", "/"): v for k, v in C.tree(tmp_path).items()}
    assert set(want) == _tables("rnaLong")
    assert {f: on[f] for f in want} == want
    last = on["RSA_result/rnaLong_ensemble/rnaLong.txt"].splitlines()[-1]
    assert last.startswith(b"70\t\t")


def test_the_host_formatter_writes_the_same_bytes(runs):
    _, (on, _), (host, printed), _ = runs
    assert host == on and not _skipped(printed)


def test_with_the_key_off_the_skip_line_and_the_files_are_as_before(runs):
    _, (on, _), _, (off, printed) = runs
    lines = _skipped(printed)
    assert len(lines) == 1 and "L=70" in lines[0] and "(" not in lines[0].split("skipped for it")[1], printed
    assert not any("RSA_result/rnaLong" in f for f in off)
    # the narrow alignments and the trunk's files keep their bytes; the wide alignment's four tables are all that the key adds
    assert set(on) - set(off) == _tables("rnaLong") and set(off) <= set(on)
    assert {f: d for f, d in on.items() if f not in _tables("rnaLong")} == off
    assert _tables("rnaA") | _tables("rnaB") <= set(off)


def test_rsa_predict_takes_the_long_route_for_an_embedding_of_more_than_1024_rows(model_dir, tmp_path):
    """RSA_predict.py (in this process) on a [1057, 768] <name>_emb.npy, as a stitched run leaves it: the files are the host path on
    predict_long, with the device formatter and without; the parent's program refuses that length."""
    import sys
    from conftest import ROOT
    import rsa_stages as S
    sys.path.insert(0, ROOT)
    import RSA_predict
    L = 1057
    emb, _ = S.case(L, 17)
    seq = C.seq_for(L, 17)
    root, feat = model_dir.parent.parent, tmp_path / "feat"
    if not (root / "models").exists():
        (root / "models").symlink_to(model_dir.parent, target_is_directory=True)
    feat.mkdir()
    (feat / "wide.fasta").write_text(f">wide\n{seq}\n")
    np.save(feat / "wide_emb.npy", emb)
    ens = rsa.load_ensemble(model_dir, DEV)
    values = ens.predict_long(torch.from_numpy(emb).to(DEV), seq).cpu().numpy()
    rsa.write_rsa_files(values, seq, "wide", tmp_path / "want", ens.model_names, random.Random(2022))
    want = C.tree(tmp_path / "want")
    assert len(want) == 4
    for flag in ("--text-device", "--no-text-device"):
        with contextlib.redirect_stdout(io.StringIO()):
            RSA_predict.main(["--rootdir", str(root), "--featdir", str(feat), "--rnaid", "wide", "--device", "cuda", flag])
        got = {k: v for k, v in C.tree(feat).items() if k.startswith("RSA_result")}
        assert got == want, flag
        for f in got:
            (feat / f).unlink()
