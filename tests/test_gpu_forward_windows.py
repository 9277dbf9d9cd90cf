"""MSATransformer.forward_windows on synthetic weights, exact mode: an alignment wider than max_seqlen comes out as the numpy fp32
stitch (tests/windows_truth.py) of the lone forwards of its windows, bit for bit; a singly covered region carries that window's
own bits; the batched and the one-by-one route agree bit for bit; an alignment that fits is the lone forward itself.  A padded
alignment is the stitch of its windows' forwards under the one mask decision forward_windows takes for all of them, on both routes;
in a 16-bit mode the one-by-one route is the fp32 stitch of that mode's own lone forwards."""
import numpy as np
import pytest
import torch

import windows_truth as T
from rnamsm import synthetic, windows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (embed_dim, heads, layers, max_seqlen, R, L)
SMALL = (128, 2, 4, 33, 5, 70)            # (8 maps: a batch member stays 16-byte aligned at C = 33) W = 32, default stride 16: starts 0, 16, 32, 38 -- three-fold coverage at the right end
FULL = (768, 12, 10, 17, 3, 40)           # the shipped width and depth: W = 16, stride 8: starts 0, 8, 16, 24
WIDE = (128, 2, 4, 129, 3, 300)           # W = 128, default stride 64: starts 0, 64, 128, 172 -- the stitched atp is two 256-column tiles wide, three-fold coverage at the right end


def _model(D, H, NL, max_seqlen):
    from rnamsm.model import MSATransformer
    state = synthetic.make_state_dict(seed=3, embed_dim=D, num_layers=NL, num_heads=H, max_seqlen=max_seqlen)
    m = MSATransformer(embed_dim=D, num_attention_heads=H, num_layers=NL, max_seqlen=max_seqlen)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV)


def _tokens(R, L, seed):
    rng = np.random.RandomState(seed)
    body = rng.choice(synthetic.RESIDUE_TOKENS, size=(R, L))
    return torch.from_numpy(np.concatenate([np.full((R, 1), synthetic.CLS_IDX), body], 1).astype(np.int64)).to(DEV)


@pytest.fixture(scope="module", params=[SMALL, FULL, WIDE], ids=["d128", "d768", "wide"])
def case(request):
    """The model, the tokens, the lone forwards of the windows (computed once, never changed) and their numpy stitch."""
    D, H, NL, max_seqlen, R, L = request.param
    model = _model(D, H, NL, max_seqlen)
    toks = _tokens(R, L, seed=L)
    W = max_seqlen - 1
    stride = (W + 1) // 2
    lone = []
    for s in T.starts(L, W, stride):
        out = model.checked_forward_one(torch.cat([toks[:, :1], toks[:, 1 + s:1 + s + W]], 1), need_repr=False)
        lone.append((out["emb"].cpu().numpy(), out["atp"].cpu().numpy()))
    want = {"emb": T.stitch_rows([e for e, _ in lone], L, W, stride), "atp": T.stitch_pairs([a for _, a in lone], L, W, stride)}
    for v in want.values():
        v.setflags(write=False)
    return model, toks, W, stride, lone, want


def _host(out):
    return out["emb"].cpu().numpy(), out["atp"].cpu().numpy()


def test_forward_windows_is_the_numpy_stitch_of_the_lone_forwards(case):
    model, toks, W, stride, lone, want = case
    L = toks.shape[1] - 1
    assert model.gemm_dtype == "f32"
    emb, atp = _host(model.forward_windows(toks))
    assert emb.shape == (L, model.embed_dim) and atp.shape == (model.num_layers * model.num_attention_heads, L, L)
    assert np.isfinite(emb).all() and np.isfinite(atp).all()
    assert emb.tobytes() == want["emb"].tobytes() and atp.tobytes() == want["atp"].tobytes()
    # the default stride is ceil(W / 2); naming it changes nothing, another stride does
    e2, a2 = _host(model.forward_windows(toks, stride=stride))
    assert e2.tobytes() == emb.tobytes() and a2.tobytes() == atp.tobytes()
    e3, _ = _host(model.forward_windows(toks, stride=W))
    assert e3.shape == emb.shape and e3.tobytes() != emb.tobytes()
    with pytest.raises(ValueError, match="stride"):
        model.forward_windows(toks, stride=stride - 1)


def test_singly_covered_regions_carry_their_window_s_own_bits(case):
    model, toks, W, stride, lone, want = case
    L = toks.shape[1] - 1
    emb, atp = _host(model.forward_windows(toks))
    st = T.starts(L, W, stride)
    cover = np.zeros(L, int)
    for s in st:
        cover[s:s + W] += 1
    assert cover[0] == 1 and cover[L - 1] == 1
    for k in (0, len(st) - 1):
        s = st[k]
        own = np.flatnonzero(cover[s:s + W] == 1)
        assert len(own) >= 1
        assert emb[s + own].tobytes() == lone[k][0][own].tobytes()
        assert atp[:, s + own][:, :, s + own].tobytes() == lone[k][1][:, own][:, :, own].tobytes()
    uncovered = ~T.covered_pairs(L, W, stride)
    assert uncovered.any() and (atp.view(np.uint32)[:, uncovered] == 0).all()


def test_the_batched_and_the_one_by_one_route_give_the_same_bits(case, monkeypatch):
    model, toks, W, stride, lone, want = case
    calls = {"batch": 0, "one": 0}
    batch, one = model.checked_forward_batch, model.checked_forward_one
    monkeypatch.setattr(model, "checked_forward_batch", lambda *a, **k: (calls.__setitem__("batch", calls["batch"] + 1), batch(*a, **k))[1])
    monkeypatch.setattr(model, "checked_forward_one", lambda *a, **k: (calls.__setitem__("one", calls["one"] + 1), one(*a, **k))[1])
    n = len(lone)
    assert n * toks.shape[0] * model.max_seqlen <= model.batch_token_budget
    batched = _host(model.forward_windows(toks))
    assert calls == {"batch": 1, "one": 0}
    single = _host(model.forward_windows(toks, batched=False))
    assert calls == {"batch": 1, "one": n}
    monkeypatch.setattr(model, "batch_token_budget", n * toks.shape[0] * model.max_seqlen - 1)      # one token short: one by one
    short = _host(model.forward_windows(toks))
    assert calls == {"batch": 1, "one": 2 * n}
    for got in (batched, single, short):
        assert got[0].tobytes() == want["emb"].tobytes() and got[1].tobytes() == want["atp"].tobytes()


def test_an_alignment_that_fits_is_the_lone_forward(case):
    model, toks, W, stride, lone, want = case
    fits = toks[:, :model.max_seqlen].contiguous()
    ref = model.checked_forward_one(fits, need_repr=False)
    got = model.forward_windows(fits)
    assert sorted(got) == ["atp", "emb"]
    assert got["emb"].cpu().numpy().tobytes() == ref["emb"].cpu().numpy().tobytes()
    assert got["atp"].cpu().numpy().tobytes() == ref["atp"].cpu().numpy().tobytes()
    assert windows.default_stride(W) == stride


def _stitch_of_lone_forwards(model, toks, W, stride, has_padding=None):
    """The numpy stitch of checked_forward_one(window, has_padding, need_repr=False) over the plan's windows -> (emb, atp) on the host."""
    L = toks.shape[1] - 1
    lone = []
    for s in T.starts(L, W, stride):
        out = model.checked_forward_one(torch.cat([toks[:, :1], toks[:, 1 + s:1 + s + W]], 1), has_padding, need_repr=False)
        lone.append((out["emb"].cpu().numpy(), out["atp"].cpu().numpy()))
    return T.stitch_rows([e for e, _ in lone], L, W, stride), T.stitch_pairs([a for _, a in lone], L, W, stride)


# (the case, then the body column at which a <pad> tail starts in row 1 and in row 2)
@pytest.mark.parametrize("params,tail1,tail2", [(SMALL, 34, 38), (WIDE, 150, 172)], ids=["d128", "wide"])
def test_a_padded_alignment_is_the_stitch_of_its_windows_under_one_mask_decision(params, tail1, tail2, monkeypatch):
    """Two rows end in <pad>: one tail starts inside the overlap of windows 1 and 2, so that window 0 holds no <pad> at all and
    still runs with the masks on; the other starts where the last window starts and fills that row of it."""
    D, H, NL, max_seqlen, R, L = params
    model = _model(D, H, NL, max_seqlen)
    W = max_seqlen - 1
    stride = windows.default_stride(W)
    st = T.starts(L, W, stride)
    assert st[2] <= tail1 < st[1] + W and tail1 < st[3] and tail2 == st[-1]
    toks = _tokens(R, L, seed=L + 1)
    pad = model.vocab.pad_idx
    assert pad == synthetic.PAD_IDX
    toks[1, 1 + tail1:] = pad
    toks[2, 1 + tail2:] = pad
    assert not (toks[:, :1 + st[0] + W] == pad).any() and (toks[2, 1 + st[-1]:] == pad).all()
    want_emb, want_atp = _stitch_of_lone_forwards(model, toks, W, stride, has_padding=True)
    assert np.isfinite(want_emb).all() and np.isfinite(want_atp).all()
    calls = {"batch": 0}
    batch = model.checked_forward_batch
    monkeypatch.setattr(model, "checked_forward_batch", lambda *a, **k: (calls.__setitem__("batch", calls["batch"] + 1), batch(*a, **k))[1])
    batched = _host(model.forward_windows(toks))
    assert calls == {"batch": 1}                                               # the padded alignment did take the batched route
    single = _host(model.forward_windows(toks, batched=False))
    assert calls == {"batch": 1}
    for emb, atp in (batched, single):
        assert emb.tobytes() == want_emb.tobytes() and atp.tobytes() == want_atp.tobytes()


@pytest.mark.parametrize("mode", ["f16x3", "bf16"])
def test_the_one_by_one_route_in_a_16bit_mode_is_the_fp32_stitch_of_that_mode_s_lone_forwards(mode):
    """The stitch is fp32 whatever produced the windows.  (The batched route is not held to it in these modes: equal bits of the two
    routes are promised for exact mode only.)"""
    D, H, NL, max_seqlen, R, L = SMALL
    model = _model(D, H, NL, max_seqlen)
    W = max_seqlen - 1
    stride = windows.default_stride(W)
    toks = _tokens(R, L, seed=L)
    exact = _host(model.forward_windows(toks, batched=False))
    try:
        model.gemm_dtype = mode
        assert model.layers[3].column_self_attention.layer.gemm_dtype == mode
        want_emb, want_atp = _stitch_of_lone_forwards(model, toks, W, stride)
        emb, atp = _host(model.forward_windows(toks, batched=False))
    finally:
        model.gemm_dtype = "f32"
    assert np.isfinite(emb).all() and np.isfinite(atp).all()
    assert emb.tobytes() == want_emb.tobytes() and atp.tobytes() == want_atp.tobytes()
    assert emb.tobytes() != exact[0].tobytes()                                 # the mode did run: these are not the exact path's bits
