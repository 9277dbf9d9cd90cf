"""The batched SS head on the GPU (rnamsm_ss_head_packed, SSPredictor.predict_many / logits_many): every member's bits are
those of the lone head on that member -- at the tile edges, in either order, beside neighbours whose data differ wildly, read
in place from a shared or a wider buffer -- plus one comparison with the fp64 truth, run-to-run bits, the chunked path and
the CLI's group deliveries."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from rnamsm import _lib, ops, ss, synthetic
import ss_truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EDGE_LS = [1, 2, 15, 16, 17, 33, 35, 35, 48, 100]      # below / at / above a multiple of the 16-pixel tile; two equal L


def _predictor(state, num_blocks):
    m = ss.SSPredictor(num_blocks)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV)


def _case(L, seed):
    """Attention-like maps (rows on the simplex) and a sequence with one character outside A, C, G, U."""
    rng = np.random.RandomState(seed)
    atp = rng.exponential(size=(120, L, L)).astype(np.float32)
    atp /= atp.sum(-1, keepdims=True)
    seq = "".join(rng.choice(list("ACGU"), L))
    if L > 3:
        seq = seq[:2] + "N" + seq[3:]
    return atp, seq


def _cases(Ls, seed0):
    cases = [_case(L, seed0 + i) for i, L in enumerate(Ls)]
    return [torch.from_numpy(a).to(DEV) for a, _ in cases], [s for _, s in cases]


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same_bits(got, want, label):
    assert got.shape == want.shape, label
    assert np.array_equal(_bits(got), _bits(want)), label


@pytest.fixture(scope="module")
def head4():
    return _predictor(ss_truth.make_state(4, seed=21), 4)


@pytest.fixture(scope="module")
def edge_batch(head4):
    """The tile-edge batch and its lone results, computed once."""
    atps, seqs = _cases(EDGE_LS, 300)
    assert not torch.equal(atps[6], atps[7])             # the two L = 35 members carry different data
    lone_logits = [head4.logits(a, s) for a, s in zip(atps, seqs)]
    lone_probs = [head4.predict(a, s) for a, s in zip(atps, seqs)]
    return atps, seqs, lone_logits, lone_probs


@pytest.mark.parametrize("reverse", [False, True])
def test_every_member_has_the_lone_head_s_bits(head4, edge_batch, reverse):
    atps, seqs, lone_logits, lone_probs = (list(reversed(v)) if reverse else v for v in edge_batch)
    logits = head4.logits_many(atps, seqs)
    probs = head4.predict_many(atps, seqs)
    assert len(logits) == len(probs) == len(atps)
    for b, L in enumerate(a.shape[-1] for a in atps):
        _same_bits(logits[b], lone_logits[b], f"logits of member {b} (L = {L})")
        _same_bits(probs[b], lone_probs[b], f"probs of member {b} (L = {L})")


def test_sixteen_blocks_have_the_lone_head_s_bits():
    head = _predictor(ss_truth.make_state(16, seed=22), 16)
    atps, seqs = _cases([17, 35, 64], 400)
    logits, probs = head.logits_many(atps, seqs), head.predict_many(atps, seqs)
    for b, (a, s) in enumerate(zip(atps, seqs)):
        _same_bits(logits[b], head.logits(a, s), f"logits of member {b}")
        _same_bits(probs[b], head.predict(a, s), f"probs of member {b}")


def test_more_members_than_one_descriptor_launch():
    """33 structures: the descriptor table goes up in two launches (32 + 1), so a member on either side of that seam must find
    its own entry.  One block, L drawn from 1..20 (one or two tiles a side): a few milliseconds."""
    head = _predictor(ss_truth.make_state(1, seed=23), 1)
    Ls = [int(v) for v in np.random.RandomState(33).randint(1, 21, size=33)]
    atps, seqs = _cases(Ls, 700)
    logits, probs = head.logits_many(atps, seqs), head.predict_many(atps, seqs)
    assert len(logits) == len(probs) == 33
    for b, (a, s) in enumerate(zip(atps, seqs)):
        _same_bits(logits[b], head.logits(a, s), f"logits of member {b} (L = {Ls[b]})")
        _same_bits(probs[b], head.predict(a, s), f"probs of member {b} (L = {Ls[b]})")


def _call_c(model, atps, strides, codes, wants, poison=True):
    """rnamsm_ss_head_packed itself.  wants[b]: a subset of {"logits", "probs"}.  The workspace is filled with NaN first.
    Returns per member {"logits": tensor or None, "probs": tensor or None}."""
    lib = _lib.load()
    B = len(atps)
    Ls = [int(c.numel()) for c in codes]
    nbytes = lib.rnamsm_ss_head_packed_workspace_bytes(B, (ctypes.c_int * B)(*Ls))
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF if poison else 0, dtype=torch.uint8, device=DEV)        # 0xFFFFFFFF: a NaN in every float
    items = (_lib.SsItem * B)()
    outs = []
    for b, L in enumerate(Ls):
        o = {k: (torch.full((L, L), float("nan"), device=DEV) if k in wants[b] else None) for k in ("logits", "probs")}
        outs.append(o)
        items[b] = _lib.SsItem(atps[b].data_ptr(), strides[b], codes[b].data_ptr(), L,
                               o["logits"].data_ptr() if o["logits"] is not None else None,
                               o["probs"].data_ptr() if o["probs"] is not None else None)
    ptrs, _ = model._packed_weights()
    _lib.check(lib.rnamsm_ss_head_packed(items, B, model.num_blocks, ptrs, ws.data_ptr(), ws.numel(),
                                         torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return outs


def _codes(seq):
    return torch.from_numpy(ss.base_codes(seq)).to(DEV)


def test_neighbours_do_not_leak_into_a_member():
    """Images are neighbours in the workspace: member 1's halo rows lie in member 0's last and member 2's first pixels.  With
    large LayerNorm betas relu(LN(anything)) is far from the zero padding, and the neighbours' values are changed by six
    orders of magnitude between the two calls: member 1 must not move by a bit, and equal the lone head."""
    head = _predictor(ss_truth.make_state(4, seed=7, beta_scale=5.0), 4)
    Ls = [17, 40, 16]
    atps, seqs = _cases(Ls, 500)
    codes = [_codes(s) for s in seqs]
    strides = [L * L for L in Ls]
    both = [("logits", "probs")] * 3
    first = _call_c(head, atps, strides, codes, both)
    loud = [torch.full_like(atps[0], 1e3), atps[1], torch.full_like(atps[2], 1e3)]
    second = _call_c(head, loud, strides, codes, both)
    for kind, lone in (("logits", head.logits(atps[1], seqs[1])), ("probs", head.predict(atps[1], seqs[1]))):
        assert torch.isfinite(first[1][kind]).all()
        _same_bits(second[1][kind], first[1][kind], f"member 1's {kind} moved with its neighbours' data")
        _same_bits(first[1][kind], lone, f"member 1's {kind} differ from the lone head's")
    assert not np.array_equal(_bits(second[0]["logits"]), _bits(first[0]["logits"]))      # the neighbours themselves did change
    for b in (0, 2):
        _same_bits(first[b]["logits"], head.logits(atps[b], seqs[b]), f"member {b}")


def test_members_read_in_place_and_mixed_requests(head4):
    Ls = [12, 35, 20]
    atps, seqs = _cases(Ls, 600)
    codes = [_codes(s) for s in seqs]
    want = [head4.logits_many(atps, seqs), head4.predict_many(atps, seqs)]
    # the layout of rnamsm_forward_packed's atp: every member's [120, L, L] back to back in one buffer
    flat = torch.cat([a.reshape(-1) for a in atps])
    views, off = [], 0
    for L in Ls:
        views.append(flat[off:off + 120 * L * L].view(120, L, L))
        off += 120 * L * L
    # ... and member 1 in a wider buffer instead: plane stride L*L + 13, NaN in the gaps
    L1 = Ls[1]
    wide = torch.full((120, L1 * L1 + 13), float("nan"), device=DEV)
    wide[:, :L1 * L1] = atps[1].reshape(120, -1)
    views[1] = wide[:, :L1 * L1].view(120, L1, L1)
    assert views[1].stride() == (L1 * L1 + 13, L1, 1) and views[0].data_ptr() == flat.data_ptr()
    for kind, got in (("logits", head4.logits_many(views, seqs)), ("probs", head4.predict_many(views, seqs))):
        for b in range(3):
            _same_bits(got[b], want[kind == "probs"][b], f"{kind} of member {b} read in place")
    # logits only / probs only / both, per member
    outs = _call_c(head4, views, [v.stride(0) for v in views], codes, [("logits",), ("probs",), ("logits", "probs")])
    assert outs[0]["probs"] is None and outs[1]["logits"] is None
    _same_bits(outs[0]["logits"], want[0][0], "member 0: logits only")
    _same_bits(outs[1]["probs"], want[1][1], "member 1: probs only")
    _same_bits(outs[2]["logits"], want[0][2], "member 2: logits")
    _same_bits(outs[2]["probs"], want[1][2], "member 2: probs")


def test_a_batch_against_the_fp64_truth():
    """The lone head's bars (ss_truth.compare with seams), once: a guard should a later change move lone and packed together."""
    state = ss_truth.make_state(4, seed=31)
    head = _predictor(state, 4)
    Ls = [5, 35, 129]
    cases = [_case(L, 700 + L) for L in Ls]
    got = head.logits_many([torch.from_numpy(a).to(DEV) for a, _ in cases], [s for _, s in cases])
    for (atp, seq), g in zip(cases, got):
        x = ss_truth.features(atp, seq)
        t64 = ss_truth.logits(x, state, torch.float64)
        t32 = ss_truth.logits(x, state, torch.float32).astype(np.float64)
        ss_truth.compare(g.cpu().numpy().astype(np.float64), t64, t32, f"packed, L={len(seq)}", seams=True)


def test_two_runs_give_the_same_bits(head4, edge_batch):
    atps, seqs = edge_batch[0], edge_batch[1]
    r1 = [p.clone() for p in head4.predict_many(atps, seqs)]
    r2 = head4.predict_many(atps, seqs)
    for b in range(len(atps)):
        _same_bits(r2[b], r1[b], f"member {b}")


def test_chunked_calls_give_the_unchunked_bits(head4, monkeypatch):
    Ls = [40, 40, 40, 20, 64]
    atps, seqs = _cases(Ls, 800)
    whole = [p.clone() for p in head4.predict_many(atps, seqs)]
    calls = []
    real = ops.ss_head_packed
    monkeypatch.setattr(ops, "ss_head_packed", lambda a, *rest, **kw: calls.append(len(a)) or real(a, *rest, **kw))
    head4.predict_many(atps, seqs)
    assert calls == [5]                                   # 11 296 pixels: one call at the default budget
    del calls[:]
    monkeypatch.setattr(ss.plan_ss_chunks, "__defaults__", (64 * 64, ss.plan_ss_chunks.__defaults__[1]))
    assert ss.plan_ss_chunks(Ls) == [[0, 1], [2, 3], [4]]
    parts = head4.predict_many(atps, seqs)
    assert calls == [2, 2, 1]
    for b in range(len(Ls)):
        _same_bits(parts[b], whole[b], f"member {b}")


def test_cli_groups_go_through_the_batched_head(tmp_path, monkeypatch):
    """Six small alignments with the SS key on: the lone head must never run (it raises here), at least one call of the batched
    head covers two or more members, and every SS_result file equals the one-by-one run's (lone head, no batching) byte for
    byte."""
    sys.path.insert(0, ROOT)
    import RNA_MSM_Inference as cli
    state = synthetic.make_state_dict(seed=0, num_layers=10)
    ckpt = tmp_path / "model.ckpt"
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in state.items()}}, ckpt)
    ss_pt = tmp_path / "model" / "rna-msm_attention.pt"
    ss_pt.parent.mkdir(parents=True)
    torch.save({k: torch.from_numpy(v) for k, v in ss_truth.make_state(4, seed=5).items()}, ss_pt)
    # rnamsm.ss.load_predictor builds the 16-block network by default: the CLI loads a 4-block file through it here
    real_load = ss.load_predictor
    monkeypatch.setattr(ss, "load_predictor", lambda path, device, num_blocks=4: real_load(path, device, num_blocks))
    rng = np.random.RandomState(91)
    shapes = [(4, 12), (8, 40), (5, 17), (6, 33), (7, 16), (4, 25)]          # depth 4..8, length 12..40
    ids = [f"rna{k}" for k in range(len(shapes))]
    texts = {i: "".join(f">s{r}\n{''.join(rng.choice(list('ACGU'), L))}\n" for r in range(R)) for i, (R, L) in zip(ids, shapes)}
    (tmp_path / "rna_id.txt").write_text("\n".join(ids) + "\n")

    def run(name, batching):
        res = tmp_path / name
        res.mkdir()
        for i in ids:
            (res / f"{i}.a2m_msa2").write_text(texts[i])
        cli.main([f"data.root_path={tmp_path}", f"data.MSA_path={name}", f"data.model_path={ckpt}", "data.MSA_list=rna_id.txt",
                  "data.max_seqs_per_msa=32", "data.sample_method=first", f"data.batch_small_msas={batching}",
                  f"data.ss_model_path={ss_pt}"])
        return res

    sizes = []
    real_packed = ops.ss_head_packed

    def boom(*a, **k):
        raise AssertionError("the lone SS head ran for a member of a group")

    with monkeypatch.context() as m:
        m.setattr(ops, "ss_head", boom)
        m.setattr(ops, "ss_head_packed", lambda a, *rest, **kw: sizes.append(len(a)) or real_packed(a, *rest, **kw))
        grouped = run("grouped", True)
    assert sum(sizes) == len(ids) and max(sizes) >= 2, sizes
    del sizes[:]
    single = run("single", False)
    for i, (_, L) in zip(ids, shapes):
        for ext in ("ct", "bpseq", "prob"):
            a, b = (grouped / "SS_result" / f"{i}.{ext}").read_bytes(), (single / "SS_result" / f"{i}.{ext}").read_bytes()
            assert a and a == b, (i, ext)
        assert np.loadtxt(grouped / "SS_result" / f"{i}.prob", delimiter="\t", ndmin=2).shape == (L, L)
        for kind in ("atp", "emb"):
            assert (grouped / f"{i}_{kind}.npy").read_bytes() == (single / f"{i}_{kind}.npy").read_bytes(), (i, kind)
