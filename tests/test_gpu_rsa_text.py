"""The RSA_result tables written on the GPU (rnamsm_rsa_text / _packed, rnamsm.rsa.table_text, RSAEnsemble.predict_text,
write_rsa_files(text=...), the CLI key data.rsa_text_device).  The expected bytes are always those of write_rsa_files' host path on
the same values, run into a temporary directory (rsa_text_cases.expected_bodies); every comparison is byte for byte, and the
ensemble's (ASA, RSA) bit for bit."""
import os
import pickle
import random
import shutil
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import rsa_text_cases as C
import rsa_truth as T
from rnamsm import _lib, ops, rsa, synthetic
from rnamsm.ss import letter_codes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(values: np.ndarray, seq: str):
    return torch.from_numpy(np.ascontiguousarray(values)).to(DEV), torch.from_numpy(letter_codes(seq)).to(DEV)


def _host(rec):
    return tuple(t.cpu().numpy() for t in rec)


def _same_record(a, b, K, L) -> bool:
    """Two text records (device or host), byte for byte where a body was written (behind its count a buffer holds whatever was there)."""
    a, b = (tuple(t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in r) for r in (a, b))
    return (np.array_equal(a[1], b[1]) and C.split_text(a[0], a[1], K, L) == C.split_text(b[0], b[1], K, L)
            and np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)))


def _lone(values: np.ndarray, seq: str):
    return _host(ops.rsa_text(*_dev(values, seq)))


_expected = {}


def _want(kind: str, K: int, L: int):
    """(values, seq, bodies, ens) of one case, the host path run once per session."""
    key = (kind, K, L)
    if key not in _expected:
        seed = 1000 * K + L
        values = C.uniform_values(K, L, seed) if kind == "uniform" else C.special_table(K, L, seed)
        seq = C.seq_for(L, seed)
        _expected[key] = (values, seq, *C.expected_bodies(values, seq))
    return _expected[key]


def _check(rec, K, L, bodies, ens):
    text, counts, got_ens = rec
    assert counts.dtype == np.int32 and counts.shape == (K + 3,) and got_ens.dtype == np.float64 and got_ens.shape == (2, L)
    assert counts[K + 1] == 0 and counts[K + 2] == 0, counts
    assert [int(c) for c in counts[:K + 1]] == [len(b) for b in bodies]
    got = C.split_text(text, counts, K, L)
    for f in range(K + 1):
        assert got[f] == bodies[f], (f, got[f][:60], bodies[f][:60])
    assert np.array_equal(got_ens.view(np.uint64), ens.view(np.uint64))


@pytest.mark.parametrize("K", C.KS)
@pytest.mark.parametrize("kind", ["uniform", "special"])
def test_bytes_counts_and_ensemble_match_the_host_path(kind, K):
    """Every length at which the index gains a digit and at the edges of the kernel's 256-position passes; sequences over ACGU with
    some T; the special tables carry the tie and carry values at the first and last position and on both sides of every seam."""
    for L in C.LENGTHS:
        values, seq, bodies, ens = _want(kind, K, L)
        assert "T" in seq or L < 7
        _check(_lone(values, seq), K, L, bodies, ens)


def test_all_one_letter_sequences_and_the_model():
    """All-G and all-U (both scales at every special value), and the Python model of the contract on the device's bytes too."""
    for seq_letter in "GUT":
        values = C.special_table(3, 300, ord(seq_letter))
        seq = seq_letter * 300
        bodies, ens = C.expected_bodies(values, seq)
        rec = _lone(values, seq)
        _check(rec, 3, 300, bodies, ens)
        m_bodies, m_counts, m_ens = C.model(values, seq)
        assert m_bodies == bodies and np.array_equal(m_counts, rec[1]) and np.array_equal(m_ens, rec[2])


BAD_VALUES = [np.nan, np.inf, -0.0, np.float32(1.0000001)]


@pytest.mark.parametrize("L", [1, 300])
def test_flag_words(L):
    K = 3
    values, seq = C.uniform_values(K, L, 5), C.seq_for(L, 5)
    places = sorted({0, L // 2, L - 1})
    assert np.float32(1.0000001) > 1
    for p in places:
        for bad in BAD_VALUES:
            for k in (0, K - 1):
                v = values.copy()
                v[k, p] = bad
                counts = _lone(v, seq)[1]
                assert counts[K + 1] == 1, (bad, k, p, counts)
                assert all(0 <= int(c) <= C.LINE_MAX * L for c in counts[:K + 1])
        for letter in "XNa":
            counts = _lone(values, seq[:p] + letter + seq[p + 1:])[1]
            assert counts[K + 1] == 1 and counts[K + 2] == 0, (letter, p, counts)
        v = values.copy()
        v[1, p] = 0.0
        counts = _lone(v, seq)[1]
        assert counts[K + 1] == 0 and counts[K + 2] == 1, (p, counts)
    counts = _lone(values, seq)[1]
    assert counts[K + 1] == 0 and counts[K + 2] == 0


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)])
def test_a_flagged_member_leaves_its_neighbours_alone(order):
    K = 3
    Ls = (35, 257, 10)
    vals = [C.uniform_values(K, L, 40 + i) for i, L in enumerate(Ls)]
    seqs = [C.seq_for(L, 40 + i) for i, L in enumerate(Ls)]
    vals[1][2, 100] = np.nan
    seqs[2] = "N" + seqs[2][1:]
    vals[2][0, 3] = 0.0
    lone = [_lone(v, s) for v, s in zip(vals, seqs)]
    assert [int(r[1][K + 1]) for r in lone] == [0, 1, 1] and [int(r[1][K + 2]) for r in lone] == [0, 0, 1]
    dev = [_dev(vals[i], seqs[i]) for i in order]
    packed = [_host(r) for r in ops.rsa_text_packed([d[0] for d in dev], [d[1] for d in dev])]
    for slot, i in enumerate(order):
        assert np.array_equal(packed[slot][1][K + 1:], lone[i][1][K + 1:])
    clean = order.index(0)
    assert C.split_text(packed[clean][0], packed[clean][1], K, Ls[0]) == C.split_text(lone[0][0], lone[0][1], K, Ls[0])
    assert np.array_equal(packed[clean][1], lone[0][1]) and np.array_equal(packed[clean][2], lone[0][2])
    _check(packed[clean], K, Ls[0], *C.expected_bodies(vals[0], seqs[0]))


def _raw_packed(members, K, fill=0xFF):
    """rnamsm_rsa_text_packed through ctypes on pre-filled buffers -> per member (text, counts, ens) on the host."""
    lib = _lib.load()
    B = len(members)
    items = (_lib.RsaTextItem * B)()
    keep = []
    for b, (values, seq) in enumerate(members):
        L = values.shape[1]
        v, l = _dev(values, seq)
        text = torch.full(((K + 1) * C.LINE_MAX * L,), fill, dtype=torch.uint8, device=DEV)
        counts = torch.full((K + 3,), -1, dtype=torch.int32, device=DEV)
        ens = torch.full((2, L), -1.0, dtype=torch.float64, device=DEV)
        keep.append((v, l, text, counts, ens))
        items[b] = _lib.RsaTextItem(v.data_ptr(), l.data_ptr(), L, text.data_ptr(), counts.data_ptr(), ens.data_ptr())
    with torch.cuda.device(DEV):
        _lib.check(lib.rnamsm_rsa_text_packed(items, B, K, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return [(k[2].cpu().numpy(), k[3].cpu().numpy(), k[4].cpu().numpy()) for k in keep]


def test_packed_members_are_the_lone_calls_and_nothing_else_is_written():
    """Members of unlike L, 33 of them (one past the 32 descriptors of a launch): every output is the lone call's, bytes behind a
    body's count keep the 0xFF they were filled with, and a second run gives the same bytes."""
    K = 3
    Ls = [1, 10, 257, 35] + [3 + 7 * i for i in range(29)]
    assert len(Ls) == 33
    members = [(C.special_table(K, L, 70 + i) if L > 100 else C.uniform_values(K, L, 70 + i), C.seq_for(L, 70 + i)) for i, L in enumerate(Ls)]
    first, second = _raw_packed(members, K), _raw_packed(members, K)
    for b, ((values, seq), got, again) in enumerate(zip(members, first, second)):
        L = Ls[b]
        lone = _lone(values, seq)
        bound = C.LINE_MAX * L
        for f in range(K + 1):
            n = int(got[1][f])
            assert 0 < n <= bound
            assert np.array_equal(got[0][f * bound:f * bound + n], lone[0][f * bound:f * bound + n]), (b, f)
            assert (got[0][f * bound + n:(f + 1) * bound] == 0xFF).all(), (b, f)
        assert np.array_equal(got[1], lone[1]) and np.array_equal(got[2].view(np.uint64), lone[2].view(np.uint64)), b
        for a, c in zip(got, again):
            assert np.array_equal(a, c), b
    for b in (0, 2, 32):
        _check(first[b], K, Ls[b], *C.expected_bodies(*members[b]))
    # the op's carved buffers give the same records
    via_op = ops.rsa_text_packed(*zip(*[_dev(v, s) for v, s in members]))
    for b, rec in enumerate(via_op):
        lone = _lone(*members[b])
        host = _host(rec)
        assert rec[0].data_ptr() % 16 == 0
        assert C.split_text(host[0], host[1], K, Ls[b]) == C.split_text(lone[0], lone[1], K, Ls[b]) and np.array_equal(host[1], lone[1])
        assert np.array_equal(host[2], lone[2])


def test_a_null_ens_is_skipped():
    lib = _lib.load()
    values, seq = C.uniform_values(2, 40, 3), C.seq_for(40, 3)
    v, l = _dev(values, seq)
    text = torch.empty(3 * C.LINE_MAX * 40, dtype=torch.uint8, device=DEV)
    counts = torch.empty(5, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(lib.rnamsm_rsa_text(v.data_ptr(), l.data_ptr(), 40, 2, text.data_ptr(), counts.data_ptr(), None,
                                       torch.cuda.current_stream().cuda_stream))
    lone = _lone(values, seq)
    assert np.array_equal(counts.cpu().numpy(), lone[1])
    assert C.split_text(text.cpu().numpy(), lone[1], 2, 40) == C.split_text(lone[0], lone[1], 2, 40)


# ---------------------------------------------------------------------- the whole route
def _ensemble():
    members = [rsa.RSAPredictor.from_state_dict({n: torch.from_numpy(v) for n, v in T.load_state(f"state_oh_{k}").items()}) for k in range(3)]
    st = T.load_stats("oh")
    return rsa.RSAEnsemble(members, {"oh": (st["oh_mu"], st["oh_std"]), "emb": (st["emb_mu"], st["emb_std"])},
                           names=C.NAMES8[:3]).eval().to(DEV)


def _fasta_seq():
    with open(os.path.join(T.GOLDEN, "2DRB_1.fasta")) as f:
        return "".join(line.strip() for line in f if not line.startswith(">"))


def test_predict_text_and_the_writer_job_give_the_host_path_s_files(tmp_path):
    from rnamsm.alphabet import RNAAlphabet
    from rnamsm.ss import token_base_codes
    ens, seq = _ensemble(), _fasta_seq()
    emb = torch.from_numpy(np.load(os.path.join(T.GOLDEN, "2DRB_1_emb.npy"))).to(DEV)
    values, text = ens.predict_text(emb, seq)
    assert torch.equal(values, ens.predict(emb, seq))
    want_ens = rsa.write_rsa_files(values.cpu().numpy(), seq, "2DRB_1", tmp_path / "host", ens.model_names, random.Random(2022))
    got_ens = rsa.write_rsa_files(values.cpu().numpy(), seq, "2DRB_1", tmp_path / "text", ens.model_names, random.Random(2022),
                                  text=_host(text))
    assert C.tree(tmp_path / "text") == C.tree(tmp_path / "host") and len(C.tree(tmp_path / "host")) == 4
    assert np.array_equal(got_ens[0], want_ens[0]) and np.array_equal(got_ens[1], want_ens[1])
    assert int(text[1][4]) == 0 and int(text[1][5]) == 0
    many = ens.predict_text_many([emb, emb[:20]], [seq, seq[:20]])
    assert torch.equal(many[0][0], values) and _same_record(many[0][1], text, 3, len(seq))
    assert torch.equal(many[1][0], ens.predict(emb[:20], seq[:20])) and many[1][1][0].numel() == 4 * C.LINE_MAX * 20
    # the head as the CLI runs it, lone and grouped, and its writer job
    alphabet = RNAAlphabet.from_architecture("rna language")
    head = rsa.RSAHead(ens, alphabet, token_base_codes(alphabet, DEV), random.Random(2022), text_on=True, device=DEV)
    tokens = torch.tensor([alphabet.get_idx(c) for c in seq], dtype=torch.int64, device=DEV)
    one = head.one(emb, None, tokens)
    group = head.many([emb, emb], [None, None], [tokens, tokens])
    for rec in (one, group[1]):
        assert _same_record(rec.text, text, 3, len(seq)) and torch.equal(rec.values, values)
    fn, tensors = head.writer_job(one, "2DRB_1", tmp_path / "job")
    fn(*(t.cpu().numpy() for t in tensors))
    assert C.tree(tmp_path / "job") == C.tree(tmp_path / "host")
    want = random.Random(2022)
    [want.randint(0, 3) for _ in range(4)]
    assert head.rng.random() == want.random()


def _model_dir(root):
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


def test_cli_key_on_and_off_write_identical_trees(tmp_path):
    """Three alignments, the middle one with an X in its query: its tables come from the host path mid-list (the X is replaced by
    the generator's draw), and the draws of the device-made tables around it keep the generator in step."""
    sys.path.insert(0, ROOT)
    import RNA_MSM_Inference as cli
    state = synthetic.make_state_dict(seed=0)
    ckpt = tmp_path / "model.ckpt"
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in state.items()}}, ckpt)
    model_dir = _model_dir(tmp_path)
    ids = ["a_first", "b_with_x", "c_last"]
    src = open(os.path.join(GOLDEN, "2DRB_1_first64.a2m_msa2")).read().split("\n")
    assert src[0].startswith(">") and set(src[1]) <= set("ACGU")
    with_x = "\n".join([src[0], src[1][:4] + "X" + src[1][5:]] + src[2:])
    trees = {}
    for key in ("true", "false"):
        res = tmp_path / f"text_{key}"
        res.mkdir()
        for i in ids:
            if i == "b_with_x":
                (res / f"{i}.a2m_msa2").write_text(with_x)
            else:
                shutil.copy(os.path.join(GOLDEN, "2DRB_1_first64.a2m_msa2"), res / f"{i}.a2m_msa2")
        (tmp_path / "rna_id.txt").write_text("\n".join(ids) + "\n")
        cli.main([f"data.root_path={tmp_path}", f"data.MSA_path={res.name}", f"data.model_path={ckpt}", "data.MSA_list=rna_id.txt",
                  "data.max_seqs_per_msa=32", "data.sample_method=first", f"data.rsa_model_dir={model_dir}",
                  f"data.rsa_text_device={key}"])
        trees[key] = C.tree(res / "RSA_result")
    assert len(trees["true"]) == 12 and trees["true"] == trees["false"]
    x_table = trees["true"][os.path.join("b_with_x_ensemble", "b_with_x.txt")].decode().split("\n")
    assert [r.split("\t\t")[1] for r in x_table if r.startswith("5\t\t")] == ["X"]
