"""The batched RSA ensemble on the GPU (rnamsm_rsa_head_packed, RSAEnsemble.predict_many / logits_many): every member's bits
are those of the lone head on that member -- on both sides of the 32-position tile and the 64-key chunk, in either order, beside
neighbours whose data differ wildly, read in place from a wider buffer -- plus one comparison with the fp64 truth, run-to-run
bits, the chunked path and the CLI's group deliveries."""
import ctypes
import pickle
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from rnamsm import _lib, ops, rsa, ss, synthetic
import rsa_truth as T
import ss_truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EDGE_LS = [1, 2, 3, 31, 32, 33, 35, 63, 64, 65, 97, 128, 129]      # both sides of the 32-position tile and the 64-key chunk


def _members(states):
    return [rsa.RSAPredictor.from_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}) for sd in states]


def _stats(kind):
    st = T.load_stats(kind)
    out = {"emb": (st["emb_mu"], st["emb_std"])}
    if kind == "oh":
        out["oh"] = (st["oh_mu"], st["oh_std"])
    return out


_CACHE = {}


def _ensemble(which):
    """'rand3': make_state weights; 'real3': the shipped one-hot models (K = 3, 773 channels each); 'emb1': the shipped
    embedding-only model (K = 1, 769 channels).  Built once, shared and left unchanged; the states come along for the truth."""
    if which not in _CACHE:
        if which == "rand3":
            states, kind = [T.make_state(11 + k) for k in range(3)], "oh"
        elif which == "real3":
            states, kind = [T.load_state(f"state_oh_{k}") for k in range(3)], "oh"
        else:
            assert which == "emb1"
            states, kind = [T.load_state("state_emb_0")], "emb"
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


def _cases(Ls, seed0):
    cases = [_case(L, seed0 + i) for i, L in enumerate(Ls)]
    return [torch.from_numpy(e).to(DEV) for e, _ in cases], [s for _, s in cases]


def _same_bits(got, want, label):
    assert tuple(got.shape) == tuple(want.shape), label
    assert got.detach().cpu().numpy().tobytes() == want.detach().cpu().numpy().tobytes(), label


_EDGE = {}


def _edge_batch(which):
    """The tile-edge batch of an ensemble and its lone results, computed once."""
    if which not in _EDGE:
        ens = _ensemble(which)[0]
        embs, seqs = _cases(EDGE_LS, 300)
        _EDGE[which] = (embs, seqs, [ens.logits(e, s) for e, s in zip(embs, seqs)], [ens.predict(e, s) for e, s in zip(embs, seqs)])
    return _EDGE[which]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("which", ["rand3", "real3", "emb1"])
def test_every_member_has_the_lone_head_s_bits(which, reverse):
    ens = _ensemble(which)[0]
    embs, seqs, lone_logits, lone_probs = (list(reversed(v)) if reverse else v for v in _edge_batch(which))
    logits = ens.logits_many(embs, seqs)
    probs = ens.predict_many(embs, seqs)
    assert len(logits) == len(probs) == len(embs)
    for b, L in enumerate(e.shape[0] for e in embs):
        assert tuple(logits[b].shape) == (len(ens), L)
        _same_bits(logits[b], lone_logits[b], f"{which}: logits of member {b} (L = {L})")
        _same_bits(probs[b], lone_probs[b], f"{which}: probs of member {b} (L = {L})")


def test_tile_and_chunk_counts_at_the_limit():
    """32 tiles and 16 key chunks beside one-tile neighbours: the only long case."""
    ens = _ensemble("rand3")[0]
    embs, seqs = _cases([1024, 1, 33], 350)
    logits, probs = ens.logits_many(embs, seqs), ens.predict_many(embs, seqs)
    for b, (e, s) in enumerate(zip(embs, seqs)):
        _same_bits(logits[b], ens.logits(e, s), f"logits of member {b}")
        _same_bits(probs[b], ens.predict(e, s), f"probs of member {b}")


def test_more_members_than_one_descriptor_launch():
    """33 alignments: the descriptor table goes up in two launches (32 + 1), so a member on either side of that seam must find
    its own entry.  L drawn from 1..70 (one to three tiles, one or two key chunks)."""
    ens = _ensemble("rand3")[0]
    Ls = [int(v) for v in np.random.RandomState(33).randint(1, 71, size=33)]
    embs, seqs = _cases(Ls, 900)
    logits, probs = ens.logits_many(embs, seqs), ens.predict_many(embs, seqs)
    assert len(logits) == len(probs) == 33
    for b, (e, s) in enumerate(zip(embs, seqs)):
        _same_bits(logits[b], ens.logits(e, s), f"logits of member {b} (L = {Ls[b]})")
        _same_bits(probs[b], ens.predict(e, s), f"probs of member {b} (L = {Ls[b]})")


SENTINEL = -7.0


def _codes(seq):
    return torch.from_numpy(ss.base_codes(seq)).to(DEV)


def _call_c(ens, embs, strides, codes, wants):
    """rnamsm_rsa_head_packed itself, on a workspace filled with NaN.  wants[b]: a subset of {"logits", "probs"}.  Every member
    has a logits and a probs slot in one arena filled with SENTINEL; only the wanted ones are handed to the call.
    Returns per member {"logits": [K, L], "probs": [K, L]} -- views of the arena, wanted or not."""
    lib = _lib.load()
    B, K = len(embs), len(ens)
    Ls = [int(c.numel()) for c in codes]
    nbytes = lib.rnamsm_rsa_head_packed_workspace_bytes(B, (ctypes.c_int * B)(*Ls), K)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)        # 0xFFFFFFFF: a NaN in every float
    arena = torch.full((2 * K * sum(Ls),), SENTINEL, device=DEV)
    items = (_lib.RsaItem * B)()
    outs, off = [], 0
    for b, L in enumerate(Ls):
        o = {}
        for kind in ("logits", "probs"):
            o[kind] = arena[off:off + K * L].view(K, L)
            off += K * L
        outs.append(o)
        items[b] = _lib.RsaItem(embs[b].data_ptr(), strides[b], codes[b].data_ptr(), L,
                                o["probs"].data_ptr() if "probs" in wants[b] else None,
                                o["logits"].data_ptr() if "logits" in wants[b] else None)
    ptrs, _ = ens._packed_weights()
    _lib.check(lib.rnamsm_rsa_head_packed(items, B, K, 1 if ens.use_onehot else 0, ptrs, ws.data_ptr(), ws.numel(),
                                          torch.cuda.current_stream().cuda_stream))
    del items                                             # the host array may go when the call returns
    torch.cuda.synchronize()
    return outs


def test_neighbours_do_not_leak_into_a_member():
    """The members' slabs are neighbours in the workspace, and the stem's and conv2's halo rows of member 1 lie one row before
    and after its own.  Its neighbours' embeddings grow by six orders of magnitude between the two calls: member 1 must not
    move by a bit, equal the lone head, and nothing may be NaN although the workspace started as NaN."""
    ens = _ensemble("rand3")[0]
    Ls = [33, 40, 31]
    embs, seqs = _cases(Ls, 500)
    codes = [_codes(s) for s in seqs]
    both = [("logits", "probs")] * 3
    first = _call_c(ens, embs, [768] * 3, codes, both)
    loud = [embs[0] * 1e6, embs[1], embs[2] * 1e6]
    second = _call_c(ens, loud, [768] * 3, codes, both)
    for run in (first, second):
        for o in run:
            assert not torch.isnan(o["logits"]).any() and not torch.isnan(o["probs"]).any()
    for kind, lone in (("logits", ens.logits(embs[1], seqs[1])), ("probs", ens.predict(embs[1], seqs[1]))):
        _same_bits(second[1][kind], first[1][kind], f"member 1's {kind} moved with its neighbours' data")
        _same_bits(first[1][kind], lone, f"member 1's {kind} differ from the lone head's")
    for b in (0, 2):
        assert second[b]["logits"].cpu().numpy().tobytes() != first[b]["logits"].cpu().numpy().tobytes()   # the neighbours did change
        _same_bits(first[b]["logits"], ens.logits(embs[b], seqs[b]), f"member {b}")


def test_members_read_in_place_and_mixed_requests(monkeypatch):
    ens = _ensemble("real3")[0]
    Ls = [12, 35, 20, 64]
    embs, seqs = _cases(Ls, 600)
    codes = [_codes(s) for s in seqs]
    want = {"logits": [ens.logits(e, s) for e, s in zip(embs, seqs)], "probs": [ens.predict(e, s) for e, s in zip(embs, seqs)]}
    # row slices of one [sum L, 768 + 64] buffer, NaN in the 64 columns between the rows
    wide = torch.full((sum(Ls), 768 + 64), float("nan"), device=DEV)
    views, off = [], 0
    for e, L in zip(embs, Ls):
        wide[off:off + L, :768] = e
        views.append(wide[off:off + L, :768])
        off += L
    for v in views:
        assert v.stride() == (832, 1) and v.data_ptr() % 16 == 0 and not (v.shape[0] > 1 and v.is_contiguous())
    seen = []
    real = ops.rsa_head_packed
    with monkeypatch.context() as m:
        m.setattr(ops, "rsa_head_packed", lambda e, *rest, **kw: seen.extend((t.data_ptr(), t.stride(0)) for t in e) or real(e, *rest, **kw))
        got = {"logits": ens.logits_many(views, seqs), "probs": ens.predict_many(views, seqs)}
    assert seen == [(v.data_ptr(), 832) for v in views] * 2          # handed on as they lie, no copy made of them
    for kind in ("logits", "probs"):
        for b in range(len(Ls)):
            _same_bits(got[kind][b], want[kind][b], f"{kind} of member {b} read in place")
    # logits only / probs only / both / probs only, per member; the slots that were not handed over keep the sentinel
    wants = [("logits",), ("probs",), ("logits", "probs"), ("probs",)]
    outs = _call_c(ens, views, [832] * len(Ls), codes, wants)
    for b, w in enumerate(wants):
        for kind in ("logits", "probs"):
            if kind in w:
                _same_bits(outs[b][kind], want[kind][b], f"member {b}: {kind}")
            else:
                assert bool((outs[b][kind] == SENTINEL).all()), f"member {b}: {kind} was written without being asked for"


def test_a_batch_against_the_fp64_truth():
    """The lone head's bars (rsa_truth.compare, L2_MULT), once: independent of the lone kernels, a guard should a later change
    move lone and packed together."""
    ens, states, kind = _ensemble("rand3")
    Ls = [35, 64, 97]
    cases = [_case(L, 700 + L) for L in Ls]
    got = ens.logits_many([torch.from_numpy(e).to(DEV) for e, _ in cases], [s for _, s in cases])
    for (emb, seq), g in zip(cases, got):
        x = T.features(emb, seq, T.load_stats(kind), use_onehot=True)
        t64 = np.stack([T.logits(x, sd, torch.float64) for sd in states])
        t32 = np.stack([T.logits(x, sd, torch.float32) for sd in states]).astype(np.float64)
        T.compare(g.cpu().numpy(), t64, t32, f"packed, L={len(seq)}", l2_mult=T.L2_MULT)


def test_two_runs_give_the_same_bits_and_a_batch_of_one_is_the_lone_call():
    ens = _ensemble("rand3")[0]
    embs, seqs, lone_logits, lone_probs = _edge_batch("rand3")
    r1 = [p.clone() for p in ens.predict_many(embs, seqs)]
    r2 = ens.predict_many(embs, seqs)
    for b in range(len(embs)):
        _same_bits(r2[b], r1[b], f"member {b}")
    for b in (0, 5, 12):                                  # L = 1, 33, 129
        one_l, one_p = ens.logits_many([embs[b]], [seqs[b]]), ens.predict_many([embs[b]], [seqs[b]])
        assert len(one_l) == len(one_p) == 1
        _same_bits(one_l[0], lone_logits[b], f"B = 1, logits, L = {EDGE_LS[b]}")
        _same_bits(one_p[0], lone_probs[b], f"B = 1, probs, L = {EDGE_LS[b]}")
    assert ens.predict_many([], []) == []


def test_chunked_calls_give_the_unchunked_bits(monkeypatch):
    ens = _ensemble("rand3")[0]
    Ls = [40, 40, 40, 20, 64]
    embs, seqs = _cases(Ls, 800)
    whole = [p.clone() for p in ens.predict_many(embs, seqs)]
    calls = []
    real = ops.rsa_head_packed
    monkeypatch.setattr(ops, "rsa_head_packed", lambda e, *rest, **kw: calls.append(len(e)) or real(e, *rest, **kw))
    ens.predict_many(embs, seqs)
    assert calls == [5]                                   # 204 positions: one call at the default budget
    del calls[:]
    monkeypatch.setattr(rsa.plan_rsa_chunks, "__defaults__", (80, rsa.plan_rsa_chunks.__defaults__[1]))
    assert rsa.plan_rsa_chunks(Ls) == [[0, 1], [2, 3], [4]]
    parts = ens.predict_many(embs, seqs)
    assert calls == [2, 2, 1]
    for b in range(len(Ls)):
        _same_bits(parts[b], whole[b], f"member {b}")


# ---------------------------------------------------------------------------------------------------------------------- the CLI
TAGS = ("0", "1", "2", "ensemble")
SHAPES = [(4, 12), (8, 40), (5, 17), (6, 33), (7, 16), (4, 25)]          # depth 4..8, length 12..40
IDS = [f"rna{k}" for k in range(len(SHAPES))]


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


def _cli_runs(tmp_path, monkeypatch, extra_keys):
    """The six alignments through the CLI twice -- batching on (with the lone RSA head booby-trapped and the batched one
    counted), then off.  Returns (grouped directory, one-by-one directory, sizes of the predict_many calls)."""
    sys.path.insert(0, ROOT)
    import RNA_MSM_Inference as cli
    state = synthetic.make_state_dict(seed=0, num_layers=10)
    ckpt = tmp_path / "model.ckpt"
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in state.items()}}, ckpt)
    model_dir = _model_dir(tmp_path)
    rng = np.random.RandomState(92)
    texts = {i: "".join(f">s{r}\n{''.join(rng.choice(list('ACGU'), L))}\n" for r in range(R)) for i, (R, L) in zip(IDS, SHAPES)}
    (tmp_path / "rna_id.txt").write_text("\n".join(IDS) + "\n")

    def run(name, batching):
        res = tmp_path / name
        res.mkdir()
        for i in IDS:
            (res / f"{i}.a2m_msa2").write_text(texts[i])
        cli.main([f"data.root_path={tmp_path}", f"data.MSA_path={name}", f"data.model_path={ckpt}", "data.MSA_list=rna_id.txt",
                  "data.max_seqs_per_msa=32", "data.sample_method=first", f"data.batch_small_msas={batching}",
                  f"data.rsa_model_dir={model_dir}"] + extra_keys)
        return res

    sizes = []
    real_many = rsa.RSAEnsemble.predict_many

    def counted(self, embs, seqs):
        sizes.append(len(embs))
        return real_many(self, embs, seqs)

    def boom(*a, **k):
        raise AssertionError("the lone RSA head ran for a member of a group")

    with monkeypatch.context() as m:
        m.setattr(rsa.RSAEnsemble, "predict", boom)
        m.setattr(ops, "rsa_head", boom)
        m.setattr(rsa.RSAEnsemble, "predict_many", counted)
        grouped = run("grouped", True)
    return grouped, run("single", False), sizes


def _rsa_texts(base, name):
    return {t: (base / "RSA_result" / f"{name}_{t}" / f"{name}.txt").read_bytes() for t in TAGS}


def _check_rsa_files(grouped, single):
    for i, (_, L) in zip(IDS, SHAPES):
        a, b = _rsa_texts(grouped, i), _rsa_texts(single, i)
        assert all(a.values()) and a == b, i
        rows = a["ensemble"].decode().split("\n")
        assert rows[0] == f"#{i} predict by ensemble model" and len([r for r in rows if r and not r.startswith("#")]) == L
        for kind in ("atp", "emb"):
            assert (grouped / f"{i}_{kind}.npy").read_bytes() == (single / f"{i}_{kind}.npy").read_bytes(), (i, kind)


def test_cli_groups_go_through_the_batched_ensemble(tmp_path, monkeypatch):
    """Six small alignments with the RSA key on: the lone head must never run (it raises here), at least one predict_many call
    covers two or more members, and every RSA_result text equals the one-by-one run's (lone head, no batching) byte for byte
    -- which also needs the writer thread to have drawn from rsa_rng in the same order."""
    grouped, single, sizes = _cli_runs(tmp_path, monkeypatch, extra_keys=[])
    assert sum(sizes) == len(IDS) and max(sizes) >= 2, sizes
    assert not (grouped / "SS_result").exists()
    _check_rsa_files(grouped, single)


def test_cli_groups_with_both_heads(tmp_path, monkeypatch):
    """The same with the SS key set as well: both heads' files match the one-by-one run's."""
    ss_pt = tmp_path / "model" / "rna-msm_attention.pt"
    ss_pt.parent.mkdir(parents=True)
    torch.save({k: torch.from_numpy(v) for k, v in ss_truth.make_state(4, seed=5).items()}, ss_pt)
    # rnamsm.ss.load_predictor builds the 16-block network by default: the CLI loads a 4-block file through it here
    real_load = ss.load_predictor
    monkeypatch.setattr(ss, "load_predictor", lambda path, device, num_blocks=4: real_load(path, device, num_blocks))
    grouped, single, sizes = _cli_runs(tmp_path, monkeypatch, extra_keys=[f"data.ss_model_path={ss_pt}"])
    assert sum(sizes) == len(IDS) and max(sizes) >= 2, sizes
    _check_rsa_files(grouped, single)
    for i in IDS:
        for ext in ("ct", "bpseq", "prob"):
            a, b = (grouped / "SS_result" / f"{i}.{ext}").read_bytes(), (single / "SS_result" / f"{i}.{ext}").read_bytes()
            assert a and a == b, (i, ext)
