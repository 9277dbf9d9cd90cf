"""The RSA head behind the front ends: the CLI key data.rsa_model_dir of RNA_MSM_Inference.py and the drop-in RSA_predict.py."""
import os
import pickle
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, golden
from rnamsm import rsa, synthetic
import rsa_truth as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAGS = ("0", "1", "2", "ensemble")


def _model_dir(root):
    """<root>/models/OH+RNA-MSM_Emb built from the fixtures: plain state_dicts and the two statistics pickles."""
    d = root / "models" / "OH+RNA-MSM_Emb"
    d.mkdir(parents=True)
    for k in range(3):
        torch.save({n: torch.from_numpy(v) for n, v in T.load_state(f"state_oh_{k}").items()}, d / f"model_pcc_{k}_1{k}=0.5.pt")
    st = T.load_stats("oh")
    with open(d / "statistic_dict_oh.pickle", "wb") as f:
        pickle.dump({"mu": st["oh_mu"], "std": st["oh_std"]}, f)
    with open(d / "statistic_dict_emb.pickle", "wb") as f:
        pickle.dump({"mu": st["emb_mu"], "std": st["emb_std"]}, f)
    return d


def _texts(base, name):
    return {t: (base / "RSA_result" / f"{name}_{t}" / f"{name}.txt").read_bytes() for t in TAGS}


@pytest.mark.parametrize("batching", [True, False])
def test_cli_key_writes_the_four_texts_per_alignment(tmp_path, batching):
    sys.path.insert(0, ROOT)
    import RNA_MSM_Inference as cli
    state = synthetic.make_state_dict(seed=0)
    ckpt = tmp_path / "model.ckpt"
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in state.items()}}, ckpt)
    model_dir = _model_dir(tmp_path)
    ids = ["2DRB_1", "2DRB_1b"]
    outs = {}
    for key in (False, True):
        res = tmp_path / ("with" if key else "without")
        res.mkdir()
        for i in ids:
            shutil.copy(os.path.join(GOLDEN, "2DRB_1_first64.a2m_msa2"), res / f"{i}.a2m_msa2")
        (tmp_path / "rna_id.txt").write_text("\n".join(ids) + "\n")
        cli.main([f"data.root_path={tmp_path}", f"data.MSA_path={res.name}", f"data.model_path={ckpt}", "data.MSA_list=rna_id.txt",
                  "data.max_seqs_per_msa=32", "data.sample_method=first", f"data.batch_small_msas={batching}"]
                 + ([f"data.rsa_model_dir={model_dir}"] if key else []))
        outs[key] = res
    assert not (outs[False] / "RSA_result").exists() and not (outs[True] / "SS_result").exists()
    for i in ids:                                      # the .npy files do not change with the key
        for kind in ("atp", "emb"):
            assert (outs[False] / f"{i}_{kind}.npy").read_bytes() == (outs[True] / f"{i}_{kind}.npy").read_bytes()
    toks = golden("tokens_2DRB_1_first64.npz")["tokens"]
    letters = {4: "A", 5: "G", 6: "C", 7: "U", 8: "X", 10: "-"}
    seq = "".join(letters[int(t)] for t in toks[0, 1:])
    ens = rsa.load_ensemble(model_dir, DEV)
    rng = random.Random(2022)
    again = tmp_path / "again"
    for i in ids:
        emb = np.load(outs[True] / f"{i}_emb.npy")
        values = ens.predict(torch.from_numpy(emb).to(DEV), seq).cpu().numpy()
        rsa.write_rsa_files(values, seq, i, again, ens.model_names, rng)
        assert _texts(outs[True], i) == _texts(again, i), i
        rows = _texts(again, i)["ensemble"].decode().split("\n")
        assert rows[0] == f"#{i} predict by ensemble model" and len([r for r in rows if r and not r.startswith("#")]) == len(seq)


def test_rsa_predict_gives_the_same_files(tmp_path):
    model_dir = _model_dir(tmp_path)
    feat = tmp_path / "feat"
    feat.mkdir()
    shutil.copy(os.path.join(T.GOLDEN, "2DRB_1.fasta"), feat / "2DRB_1.fasta")
    shutil.copy(os.path.join(T.GOLDEN, "2DRB_1_emb.npy"), feat / "2DRB_1_emb.npy")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "RSA_predict.py"), "--rootdir", str(tmp_path), "--featdir", str(feat),
                        "--rnaid", "2DRB_1", "--device", "cuda"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    ens = rsa.load_ensemble(model_dir, DEV)
    seq = "".join(ln.strip() for ln in (feat / "2DRB_1.fasta").read_text().split("\n") if not ln.startswith(">"))
    values = ens.predict(torch.from_numpy(np.load(feat / "2DRB_1_emb.npy")).to(DEV), seq).cpu().numpy()
    rsa.write_rsa_files(values, seq, "2DRB_1", tmp_path / "again", ens.model_names, random.Random(2022))
    assert _texts(feat, "2DRB_1") == _texts(tmp_path / "again", "2DRB_1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "RSA_predict.py"), "--device", "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "HIP device only" in r.stderr
