"""RNA-MSM RSA head on the GPU (rnamsm.rsa -> rnamsm_rsa_head) against the fp64 restatement (tests/rsa_truth.py).

Every kernel of the head works on tiles of 32 positions (RSA_TILE, csrc/rsa_head.hip) and the attention streams its keys in
chunks of 64, so the lengths cover each side of the edges 32, 64, 96 and 128 (31 .. 129), the shortest sequences (1, 2, 3:
every position touches the padding), the shipped example's 35 and the limit (1023, 1024).  Bars: rsa_truth.compare -- rel-L2 to
fp64 within 2 x the fp32 CPU restatement's on the same input (4 x at L <= 3, where one to nine logits make the ratio a matter of
single roundings: measured 2.5 for one make_state member at L = 2, rsa_truth.L2_MULT_SHORT), element-wise within 2 x its max-abs
+ 4 fp32 ulps of the largest |logit|.
Stage by stage (h1 .. v, the tile sums and the logits, each on the head's own input image): tests/test_gpu_rsa_head_stages.py."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import rsa_truth as T
from rnamsm import _lib, rsa

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EDGES = [31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129]
LENGTHS = [1, 2, 3, 35] + EDGES + [1023, 1024]


def _members(states):
    return [rsa.RSAPredictor.from_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}) for sd in states]


def _stats(kind):
    st = T.load_stats(kind)
    out = {"emb": (st["emb_mu"], st["emb_std"])}
    if kind == "oh":
        out["oh"] = (st["oh_mu"], st["oh_std"])
    return out


_CACHE = {}


def _ensemble(which: str):
    """'real3' / 'real1': the shipped one-hot models; 'emb1': the shipped embedding-only model; 'rand3' / 'rand1' / 'randemb1':
    make_state weights.  Built once, shared and left unchanged."""
    if which not in _CACHE:
        if which.startswith("real"):
            states = [T.load_state(f"state_oh_{k}") for k in range(int(which[-1]))]
        elif which == "emb1":
            states = [T.load_state("state_emb_0")]
        elif which == "randemb1":
            states = [T.make_state(21, cin=769)]
        else:
            states = [T.make_state(11 + k) for k in range(int(which[-1]))]
        kind = "emb" if "emb" in which else "oh"
        _CACHE[which] = (rsa.RSAEnsemble(_members(states), _stats(kind)).eval().to(DEV), states, kind)
    return _CACHE[which]


def _case(L, seed):
    """An embedding with the shipped statistics' spread and a sequence with characters outside A, C, G, U."""
    rng = np.random.RandomState(seed)
    st = T.load_stats("oh")
    emb = (st["emb_mu"] + st["emb_std"] * rng.standard_normal((L, 768))).astype(np.float32)
    seq = "".join(rng.choice(list("ACGU"), L))
    if L > 3:
        seq = seq[:1] + "N" + seq[2:-1] + "t"
    return emb, seq


_TRUTH = {}


def _truth(which, L, seed):
    key = (which, L, seed)
    if key not in _TRUTH:
        _, states, kind = _ensemble(which)
        emb, seq = _case(L, seed)
        x = T.features(emb, seq, T.load_stats(kind), use_onehot=kind == "oh")
        _TRUTH[key] = (np.stack([T.logits(x, sd, torch.float64) for sd in states]),
                       np.stack([T.logits(x, sd, torch.float32) for sd in states]).astype(np.float64))
    return _TRUTH[key]


def _check(which, L, seed=0):
    ens, _, _ = _ensemble(which)
    emb, seq = _case(L, seed)
    got = ens.logits(torch.from_numpy(emb).to(DEV), seq).cpu().numpy()
    assert got.shape == (len(ens), L) and got.dtype == np.float32
    t64, t32 = _truth(which, L, seed)
    T.compare(got, t64, t32, f"{which} L={L}", l2_mult=T.L2_MULT_SHORT if L <= 3 else T.L2_MULT)
    return got


@pytest.mark.parametrize("L", LENGTHS)
def test_random_weights_three_members(L):
    _check("rand3", L, seed=L)


@pytest.mark.parametrize("L", [1, 3, 35, 64, 65, 1024])
def test_real_weights_three_members(L):
    _check("real3", L, seed=L)


@pytest.mark.parametrize("which", ["rand1", "real1", "emb1", "randemb1"])
@pytest.mark.parametrize("L", [2, 35, 97])
def test_single_member_and_embedding_only(which, L):
    _check(which, L, seed=100 + L)


def test_probabilities_are_the_sigmoid_of_the_logits():
    ens, _, _ = _ensemble("real3")
    emb, seq = _case(131, 7)
    e = torch.from_numpy(emb).to(DEV)
    p, z = ens.predict(e, seq).cpu().double(), ens.logits(e, seq).cpu().double()
    assert float((p - torch.sigmoid(z)).abs().max()) <= 1e-6


@pytest.mark.parametrize("L", [35, 1024])
def test_two_runs_give_identical_bits(L):
    ens, _, _ = _ensemble("rand3")
    emb, seq = _case(L, 3)
    e = torch.from_numpy(emb).to(DEV)
    a, b = ens.logits(e, seq), ens.logits(e, seq)
    assert torch.equal(a, b) and torch.equal(ens.predict(e, seq), ens.predict(e, seq))


def test_strided_view_of_the_representation_is_read_in_place():
    """Row 0, columns 1..L of a [R, C, 768] representation: the same bits as its contiguous copy."""
    ens, _, _ = _ensemble("real3")
    L = 70
    emb, seq = _case(L, 5)
    rep = torch.randn(3, L + 1, 768, device=DEV)
    rep[0, 1:] = torch.from_numpy(emb).to(DEV)
    view = rep[0, 1:]
    wide = torch.randn(L, 1000, device=DEV)
    wide[:, 8:776] = view
    assert not wide[:, 8:776].is_contiguous()
    ref = ens.logits(view.contiguous(), seq)
    assert torch.equal(ens.logits(view, seq), ref)
    assert torch.equal(ens.logits(wide[:, 8:776], seq), ref)


def test_member_of_an_ensemble_equals_its_lone_run():
    ens3, states, _ = _ensemble("rand3")
    emb, seq = _case(99, 9)
    e = torch.from_numpy(emb).to(DEV)
    all3 = ens3.logits(e, seq)
    for k in range(3):
        lone = rsa.RSAEnsemble(_members([states[k]]), _stats("oh")).eval().to(DEV)
        assert torch.equal(lone.logits(e, seq)[0], all3[k]), k


def test_2drb_1_with_the_shipped_ensemble(tmp_path):
    ens, _, _ = _ensemble("real3")
    with np.load(os.path.join(T.GOLDEN, "rsa_ref_2DRB_1.npz")) as z:
        ref = {k: z[k] for k in z.files}
    with open(os.path.join(T.GOLDEN, "2DRB_1.fasta")) as f:
        seq = "".join(line.strip() for line in f if not line.startswith(">"))
    emb = np.load(os.path.join(T.GOLDEN, "2DRB_1_emb.npy"))
    got = ens.predict(torch.from_numpy(emb).to(DEV), seq).cpu().numpy()
    print(f"2DRB_1: max-abs vs the reference's fp32 rsa {np.abs(got - ref['rsa_oh']).max():.2e}, vs its fp64 "
          f"{np.abs(got - ref['rsa_oh_f64']).max():.2e}")
    assert np.abs(got.astype(np.float64) - ref["rsa_oh"]).max() <= 1e-6
    rsa.write_rsa_files(got, seq, "2DRB_1", tmp_path, [str(n) for n in ref["names"]], random.Random(2022))
    for tag in ("0", "1", "2", "ensemble"):
        with open(os.path.join(tmp_path, "RSA_result", f"2DRB_1_{tag}", "2DRB_1.txt")) as f:
            mine = f.read().split("\n")
        theirs = ref[f"text_{tag}"].tobytes().decode().split("\n")
        assert len(mine) == len(theirs)
        for a, b in zip(mine, theirs):
            if a.startswith("#") or not a:
                assert a == b
                continue
            fa, fb = a.split("\t\t"), b.split("\t\t")
            assert fa[:2] == fb[:2] and len(fa) == len(fb) == 4
            assert abs(float(fa[2]) - float(fb[2])) <= 0.01 + 1e-9 and abs(float(fa[3]) - float(fb[3])) <= 0.001 + 1e-9


def test_out_of_range_arguments_are_refused_before_any_launch():
    ens, _, _ = _ensemble("real3")
    lib = _lib.load()
    ptrs, _ = ens._packed_weights()
    L = 40
    emb = torch.zeros(L, 768, device=DEV)
    codes = torch.zeros(L, dtype=torch.uint8, device=DEV)
    out = torch.full((8, 1024), -7.0, device=DEV)
    ws = torch.empty(lib.rnamsm_rsa_head_workspace_bytes(1024, 8), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(L_=L, K=3, stride=768, ws_bytes=None, e=emb.data_ptr(), w=ptrs, o=out.data_ptr(), wsp=None):
        return lib.rnamsm_rsa_head(e, stride, codes.data_ptr(), L_, K, 1, w, o, None, ws.data_ptr() if wsp is None else wsp,
                                   ws.numel() if ws_bytes is None else ws_bytes, stream)

    for kwargs in ({"L_": 0}, {"L_": 1025}, {"K": 0}, {"K": 9}, {"stride": 767},
                   {"ws_bytes": lib.rnamsm_rsa_head_workspace_bytes(L, 3) - 1}, {"e": None}, {"o": None},
                   {"wsp": ws.data_ptr() + 4}, {"e": emb.data_ptr() + 4}):
        assert call(**kwargs) == -1, kwargs
        assert b"rsa_head" in lib.rnamsm_last_error()
    bad = (ctypes.c_void_p * len(ptrs))(*list(ptrs))
    bad[10] = None
    assert call(w=bad) == -1
    torch.cuda.synchronize()
    assert float(out.min()) == -7.0 and float(out.max()) == -7.0          # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert float(out.view(-1)[:3 * L].max()) < 1.0 + 1e-6 and float(out.view(-1)[:3 * L].min()) >= 0.0


def test_cpu_tensors_and_bad_shapes_raise():
    ens, _, _ = _ensemble("real3")
    with pytest.raises(_lib.RnamsmError):
        ens.predict(torch.zeros(5, 768), "ACGUA")
    with pytest.raises(ValueError):
        ens.predict(torch.zeros(5, 767, device=DEV), "ACGUA")
    with pytest.raises(ValueError):
        ens.predict(torch.zeros(5, 768, device=DEV), "ACGU")
    with pytest.raises(ValueError):
        ens.predict(torch.zeros(1025, 768, device=DEV), "A" * 1025)


def test_packed_table_follows_parameter_writes():
    states = [T.make_state(31)]
    ens = rsa.RSAEnsemble(_members(states), _stats("oh")).eval().to(DEV)
    emb, seq = _case(20, 1)
    e = torch.from_numpy(emb).to(DEV)
    a = ens.logits(e, seq)
    with torch.no_grad():
        ens.members[0].final.bias.add_(1.0)
    b = ens.logits(e, seq)
    assert float((b - a - 1.0).abs().max()) <= 1e-5
