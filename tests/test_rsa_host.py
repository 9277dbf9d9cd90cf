"""Host side of the RSA head (rnamsm.rsa): the text files, the loaders, the ABI and the CLI key.  No GPU."""
import glob
import os
import pickle
import random
import sys
import types

import numpy as np
import pytest
import torch
from torch import nn

import rsa_truth as T
from rnamsm import _lib, config, rsa

G = T.GOLDEN
REFERENCE_MODELS = "/root/reference/_downstream_tasks/RSA/models"


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _written(tmp, name, K):
    tags = [str(i) for i in range(K)] + ["ensemble"]
    return {t: _read(os.path.join(tmp, "RSA_result", f"{name}_{t}", f"{name}.txt")) for t in tags}


def test_text_cases_byte_for_byte(tmp_path):
    """Several calls in a row from one stream seeded 2022: the once-per-call draw is part of what is pinned."""
    rng = random.Random(2022)
    with np.load(os.path.join(G, "rsa_text_cases.npz")) as z:
        for k in z["order"]:
            rsa_k, seq, names = z[f"rsa_{k}"], str(z[f"seq_{k}"]), [str(n) for n in z[f"names_{k}"]]
            asa, r = rsa.write_rsa_files(rsa_k, seq, str(k), tmp_path, names, rng)
            assert asa.dtype == np.float64 and r.dtype == np.float64 and asa.shape == (len(seq),)
            got = _written(tmp_path, k, len(names))
            for tag, text in got.items():
                assert text == z[f"text_{k}_{tag}"].tobytes(), (k, tag)


def test_2drb_texts_byte_for_byte(tmp_path):
    with np.load(os.path.join(G, "rsa_ref_2DRB_1.npz")) as z:
        with open(os.path.join(G, "2DRB_1.fasta")) as f:
            seq = "".join(line.strip() for line in f if not line.startswith(">"))
        rsa.write_rsa_files(z["rsa_oh"], seq, "2DRB_1", tmp_path, [str(n) for n in z["names"]], random.Random(2022))
        for tag, text in _written(tmp_path, "2DRB_1", 3).items():
            assert text == z[f"text_{tag}"].tobytes(), tag


def test_module_level_random_is_accepted(tmp_path):
    random.seed(2022)
    rsa.write_rsa_files(np.full((1, 3), 0.5, np.float32), "ANG", "m", tmp_path, ["a.pt"], random)
    first = _written(tmp_path, "m", 1)
    rsa.write_rsa_files(np.full((1, 3), 0.5, np.float32), "ANG", "m", tmp_path, ["a.pt"], random.Random(2022))
    assert first == _written(tmp_path, "m", 1)


@pytest.mark.parametrize("tag", ["0", "1", "2", "ensemble"])
def test_shipped_examples_have_the_same_structure(tmp_path, tag):
    """The shipped outputs_example files pin the format only (they cannot be reproduced from the shipped embedding): a '#'
    description line, then one row per nucleotide of index, letter, %.2f ASA, %.3f RSA separated by two tabs."""
    text = _read(os.path.join(G, f"example_2DRB_1_{tag}.txt")).decode()
    rsa.write_rsa_files(np.full((3, 35), 0.4321, np.float32), "G" * 35, "x", tmp_path, ["a", "b", "c"], random.Random(0))
    mine = _written(tmp_path, "x", 3)[tag].decode()

    def rows(t):
        lines = t.split("\n")
        assert lines[0].startswith("#") and " predict by " in lines[0] and t.endswith("\n")
        return [ln.split("\t\t") for ln in lines if ln and not ln.startswith("#")]

    theirs, ours = rows(text), rows(mine)
    assert len(theirs) == len(ours) == 35
    for a, b in zip(theirs, ours):
        assert len(a) == len(b) == 4 and a[0] == b[0]
        for x, y in zip(a[2:], b[2:]):
            assert len(x.split(".")[1]) == len(y.split(".")[1])


def test_zero_asa_raises(tmp_path):
    with pytest.raises(_lib.RnamsmError):
        rsa.write_rsa_files(np.array([[0.5, 0.0, 0.5]], np.float32), "ACG", "z", tmp_path, ["a.pt"], random.Random(1))
    with pytest.raises(ValueError):
        rsa.write_rsa_files(np.zeros((2, 3), np.float32), "ACG", "z", tmp_path, ["a.pt"], random.Random(1))


@pytest.mark.parametrize("name, cin", [("state_oh_0", 773), ("state_oh_1", 773), ("state_oh_2", 773), ("state_emb_0", 769)])
def test_predictor_loads_fixture_states_strictly(name, cin):
    sd = {k: torch.from_numpy(v) for k, v in T.load_state(name).items()}
    m = rsa.RSAPredictor.from_state_dict(sd)
    assert m.cin == cin and m.use_onehot == (cin == 773)
    mine = m.state_dict()
    assert list(mine) and set(mine) == set(sd)
    assert all(mine[k].shape == sd[k].shape and torch.equal(mine[k], sd[k]) for k in sd)
    assert len(mine) == 40 and sum(v.numel() for v in mine.values()) == (261576 if cin == 773 else 260552)
    with pytest.raises(RuntimeError):
        bad = dict(sd)
        bad.pop("net.0.0.bn1.running_var")
        rsa.RSAPredictor.from_state_dict(bad)


def _model_dir(tmp_path, kind="oh", whole=False):
    d = tmp_path / ("whole" if whole else "plain")
    d.mkdir()
    st = T.load_stats(kind)
    names = ["state_oh_0", "state_oh_1", "state_oh_2"] if kind == "oh" else ["state_emb_0"]
    files = []
    for i, n in enumerate(reversed(names)):           # written in reverse: the loader sorts
        j = len(names) - 1 - i
        sd = {k: torch.from_numpy(v) for k, v in T.load_state(n).items()}
        path = d / f"model_pcc_{j}_{10 + j}=0.5.pt"
        obj = _upstream_like_module(sd) if whole else sd
        torch.save(obj, path)
        files.append(path.name)
    if kind == "oh":
        pickle.dump({"mu": st["oh_mu"], "std": st["oh_std"], "count": 3}, open(d / "statistic_dict_oh.pickle", "wb"))
        pickle.dump({"mu": st["emb_mu"], "std": st["emb_std"], "count": 3}, open(d / "statistic_dict_emb.pickle", "wb"))
    else:
        pickle.dump({"mu": st["emb_mu"], "std": st["emb_std"]}, open(d / "statistic_dict.pickle", "wb"))
    return d, sorted(files)


_UPSTREAM = {"model._0811.model_entry": ("FrameModel", "WrapLayers"), "model._0713.resnet": ("BasicBlock",),
             "model._0713.mingpt": ("Block", "SelfAttention")}


def _upstream_like_module(sd):
    """A module tree pickled under upstream's class names (registered in sys.modules by the caller): the predictor's own tree
    with the classes swapped for stand-ins of those names."""
    cls = {}
    for mod, names in _UPSTREAM.items():
        for n in names:
            cls[n] = getattr(sys.modules[mod], n)
    src = rsa.RSAPredictor.from_state_dict(sd)

    def clone(m, c):
        out = c.__new__(c)
        nn.Module.__init__(out)
        out.__dict__.update({k: v for k, v in m.__dict__.items() if k not in ("_modules",)})
        return out

    top = clone(src, cls["FrameModel"])
    block = clone(src.net[0][0], cls["BasicBlock"])
    for k, v in src.net[0][0]._modules.items():
        block._modules[k] = v
    gpt = clone(src.net[1][0], cls["Block"])
    for k, v in src.net[1][0]._modules.items():
        gpt._modules[k] = v
    att = clone(src.net[1][0].attn, cls["SelfAttention"])
    for k, v in src.net[1][0].attn._modules.items():
        att._modules[k] = v
    gpt._modules["attn"] = att
    w0, w1, net = (c.__new__(c) for c in (cls["WrapLayers"],) * 3)
    for w in (w0, w1, net):
        nn.Module.__init__(w)
    w0._modules["0"], w1._modules["0"] = block, gpt
    net._modules["0"], net._modules["1"] = w0, w1
    top._modules["net"], top._modules["final"] = net, src.final
    return top


@pytest.fixture
def upstream_names():
    """Stand-in classes under upstream's module names, for the duration of a torch.save; gone again before anything is loaded."""
    created = []
    for mod, names in _UPSTREAM.items():
        parts = mod.split(".")
        for i in range(1, len(parts) + 1):
            name = ".".join(parts[:i])
            if name not in sys.modules:
                sys.modules[name] = types.ModuleType(name)
                created.append(name)
        for n in names:
            c = type(n, (nn.Module,), {"__module__": mod})
            setattr(sys.modules[mod], n, c)
    yield
    for name in created:
        sys.modules.pop(name, None)


def _same_members(ens, names):
    assert len(ens) == len(names)
    for m, n in zip(ens.members, names):
        ref = T.load_state(n)
        got = m.state_dict()
        assert set(got) == set(ref) and all(np.array_equal(got[k].numpy(), ref[k]) for k in ref)


def test_load_ensemble_plain_state_dicts(tmp_path):
    d, files = _model_dir(tmp_path, "oh")
    ens = rsa.load_ensemble(d, "cpu")
    assert ens.model_names == files and ens.use_onehot
    _same_members(ens, ["state_oh_0", "state_oh_1", "state_oh_2"])
    st = T.load_stats("oh")
    assert ens.mu_emb.dtype == torch.float32 and np.array_equal(ens.mu_emb.numpy(), st["emb_mu"])
    assert ens.std_oh.dtype == torch.float64 and np.array_equal(ens.std_oh.numpy(), st["oh_std"])
    (tmp_path / "e").mkdir()
    d2, _ = _model_dir(tmp_path / "e", "emb")
    ens2 = rsa.load_ensemble(d2, "cpu")
    assert not ens2.use_onehot and len(ens2) == 1
    with pytest.raises(_lib.RnamsmError):        # no CPU path
        ens.predict(torch.zeros(3, 768), "ACG")


def test_load_ensemble_whole_module_pickles_without_upstream_code(tmp_path, upstream_names):
    d, files = _model_dir(tmp_path, "oh", whole=True)
    for mod in list(_UPSTREAM) + ["model._0811", "model._0713", "model"]:      # nothing of upstream importable from here on
        sys.modules.pop(mod, None)
    with pytest.raises(Exception):
        torch.load(d / files[0], map_location="cpu", weights_only=False)        # the plain loader needs the classes
    ens = rsa.load_ensemble(d, "cpu")
    assert ens.model_names == files
    _same_members(ens, ["state_oh_0", "state_oh_1", "state_oh_2"])


class _Evil:
    def __reduce__(self):
        return (os.getcwd, ())


def test_foreign_global_is_refused(tmp_path):
    d = tmp_path / "evil"
    d.mkdir()
    torch.save({"net.0.0.conv1.weight": torch.zeros(64, 773, 3), "x": _Evil()}, d / "model_pcc_0.pt")
    with pytest.raises(_lib.RnamsmError, match="refused global"):
        rsa.load_ensemble(d, "cpu")
    pickle.dump({"mu": _Evil(), "std": 1}, open(d / "statistic_dict.pickle", "wb"))
    with pytest.raises(_lib.RnamsmError, match="refused global"):
        rsa._load_stats(str(d / "statistic_dict.pickle"))


@pytest.mark.skipif(not os.path.isdir(REFERENCE_MODELS), reason="the upstream tree is not on this machine")
@pytest.mark.parametrize("kind, cin", [("OH+RNA-MSM_Emb", 773), ("RNA-MSM_Emb", 769)])
def test_real_checkpoints_load(kind, cin):
    assert not any(m == "model" or m.startswith("model.") for m in sys.modules)
    ens = rsa.load_ensemble(os.path.join(REFERENCE_MODELS, kind), "cpu")
    assert len(ens) == 3 and all(m.cin == cin for m in ens.members)
    assert ens.model_names == sorted(os.path.basename(p) for p in glob.glob(os.path.join(REFERENCE_MODELS, kind, "model_pcc_*.pt")))
    if cin == 773:
        _same_members(ens, ["state_oh_0", "state_oh_1", "state_oh_2"])


def test_abi_symbols_and_limits():
    assert {"rnamsm_rsa_head", "rnamsm_rsa_head_workspace_bytes"} <= set(_lib.EXPORTED_SYMBOLS)
    lib = _lib.load()
    assert lib.rnamsm_rsa_head_workspace_bytes(0, 1) == 0 and lib.rnamsm_rsa_head_workspace_bytes(1025, 1) == 0
    assert lib.rnamsm_rsa_head_workspace_bytes(35, 0) == 0 and lib.rnamsm_rsa_head_workspace_bytes(35, 9) == 0
    one, three = lib.rnamsm_rsa_head_workspace_bytes(35, 1), lib.rnamsm_rsa_head_workspace_bytes(35, 3)
    assert one > 0 and three == 3 * one and one % 16 == 0
    header = open(os.path.join(os.path.dirname(T.GOLDEN), "..", "..", "include", "rnamsm.h")).read()
    assert "RNAMSM_RSA_MAX_L 1024" in header and "RNAMSM_RSA_MAX_MODELS 8" in header
    assert f"RNAMSM_RSA_WEIGHTS_PER_MODEL {len(_lib.W_RSA_MODEL)}" in header


def test_packed_table_layout():
    m = rsa.RSAPredictor.from_state_dict({k: torch.from_numpy(v) for k, v in T.make_state(5).items()})
    t = m.packed()
    assert len(t) == 26 and all(x.dtype == torch.float32 and x.is_contiguous() for x in t)
    assert t[0].shape == (4, 800, 64) and float(t[0][:, 773:].abs().max()) == 0.0
    sd = m.state_dict()
    assert torch.equal(t[0][1, 5], sd["net.0.0.conv1.weight"][:, 5, 1]) and torch.equal(t[0][3, 7], sd["net.0.0.shortcut.0.weight"][:, 7, 0])
    scale = sd["net.0.0.bn1.weight"].double() / torch.sqrt(sd["net.0.0.bn1.running_var"].double() + 1e-5)
    assert torch.equal(t[1], scale.float())
    assert torch.equal(t[14][1], sd["net.1.0.attn.key.weight"].t()) and torch.equal(t[20], sd["net.1.0.mlp.0.weight"].t())


def test_config_accepts_the_key():
    cfg = config.Config()
    assert cfg.data.rsa_model_dir == ""
    cfg = config.parse_overrides(["data.rsa_model_dir=/some/dir"])
    assert cfg.data.rsa_model_dir == "/some/dir" and cfg.data.ss_model_path == ""
