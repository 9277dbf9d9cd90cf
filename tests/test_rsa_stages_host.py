"""The staged RSA restatement and its stage checks (tests/rsa_stages.py) without a GPU: that the recomposed logits_torch kept its
bits, that the exciting inputs excite what they are for, and that the checks have teeth.

Every breach below is an fp32 variant of ONE stage with ONE fault, fed the honest fp32 image of that stage's input; the check of
tests/test_gpu_rsa_head_stages.py must refuse it, and pass the variant with the fault switched off (for the attention that is
the kernel's own order: two sweeps, 64-key chunks, two-level sums) as well as the fp32 restatement itself."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rsa_stages as S
import rsa_truth as T
from rsa_stages import B0, G0, KEYS, TILE
from rsa_truth import HEADS, PLANES

F32, F64 = torch.float32, torch.float64
STATS = T.load_stats("oh")
PEAKED_LS = [33, 64, 65, 97, 129, 1024]


# ------------------------------------------------------------------------------------------------- logits_torch kept its bits
def _logits_torch_as_it_was(x, sd, pad=None):
    """rsa_truth.logits_torch before it became the composition of the four stages, verbatim."""
    x = x[None]
    b = "net.0.0."

    def bn(h, name):
        return F.batch_norm(h, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"],
                            training=False, eps=1e-5)

    if pad is None:
        c1 = F.conv1d(x, sd[b + "conv1.weight"], padding=1)
    else:
        col = pad[None, :, None]
        c1 = F.conv1d(torch.cat([col, x, col], dim=2), sd[b + "conv1.weight"])
    h = torch.relu(bn(c1, b + "bn1"))
    h = torch.relu(bn(F.conv1d(h, sd[b + "conv2.weight"], padding=1), b + "bn2"))
    w = h.mean(dim=2, keepdim=True)
    w = torch.relu(F.conv1d(w, sd[b + "fc1.weight"], sd[b + "fc1.bias"]))
    w = torch.sigmoid(F.conv1d(w, sd[b + "fc2.weight"], sd[b + "fc2.bias"]))
    y = torch.relu(h * w + bn(F.conv1d(x, sd[b + "shortcut.0.weight"]), b + "shortcut.1"))
    y = y[0].t()                                                             # [L, 64]
    g = "net.1.0."
    L = y.shape[0]
    t = F.layer_norm(y, (PLANES,), sd[g + "ln1.weight"], sd[g + "ln1.bias"], eps=1e-5)

    def heads(name):
        return F.linear(t, sd[g + f"attn.{name}.weight"], sd[g + f"attn.{name}.bias"]).view(L, HEADS, PLANES // HEADS).transpose(0, 1)

    q, k, v = heads("query"), heads("key"), heads("value")
    att = torch.softmax((q @ k.transpose(-2, -1)) * (1.0 / math.sqrt(PLANES // HEADS)), dim=-1)
    ctx = (att @ v).transpose(0, 1).contiguous().view(L, PLANES)
    y = y + F.linear(ctx, sd[g + "attn.proj.weight"], sd[g + "attn.proj.bias"])
    t = F.layer_norm(y, (PLANES,), sd[g + "ln2.weight"], sd[g + "ln2.bias"], eps=1e-5)
    t = F.linear(F.gelu(F.linear(t, sd[g + "mlp.0.weight"], sd[g + "mlp.0.bias"])), sd[g + "mlp.2.weight"], sd[g + "mlp.2.bias"])
    y = y + t
    return F.linear(y, sd["final.weight"], sd["final.bias"])[:, 0]


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("which", ["make_state(11)", "state_oh_0"])
def test_recomposed_logits_torch_has_the_bits_of_the_single_function(which, dtype):
    state = T.make_state(11) if which.startswith("make") else T.load_state("state_oh_0")
    sd = S.tensors(state, dtype)
    raw = torch.as_tensor(np.concatenate([np.zeros(4), -STATS["emb_mu"].astype(np.float64) / STATS["emb_std"], [0.0]])).to(dtype)
    for L in (1, 2, 35, 97):
        emb, seq = S.case(L, 40 + L)
        x = torch.as_tensor(T.features(emb, seq, STATS)).to(dtype)
        assert torch.equal(T.logits_torch(x, sd), _logits_torch_as_it_was(x, sd)), (which, dtype, L)
        assert torch.equal(T.logits_torch(x, sd, raw), _logits_torch_as_it_was(x, sd, raw)), (which, dtype, L, "pad")
        assert np.array_equal(T.logits(x.numpy(), state, dtype), _logits_torch_as_it_was(x, sd).numpy())


def test_the_chain_with_32_position_tiles_is_the_same_network():
    """Tile sums added in tile order give the mean to rounding: the staged chain and logits_torch agree far inside the bars."""
    state = T.make_state(11)
    emb, seq = S.case(97, 5)
    x = T.features(emb, seq, STATS)
    c = S.chain(x, state, F64)
    assert c["sums"].shape == (4, PLANES) and all(c[n].shape == (97, PLANES) for n in S.IMAGES)
    assert np.abs(c["logits"].numpy() - T.logits(x, state, F64)).max() <= 1e-13
    assert torch.equal(c["sums"][3], c["h2"][96])                         # the ragged tile: one position


# ------------------------------------------------------------------------------------------------------------- honest images
@functools.lru_cache(maxsize=None)
def _images(which, L, halo=False):
    """(state, features, fp64 chain, fp32 chain) of a named state at L, computed once and left unchanged."""
    state = {"rand": lambda: T.make_state(11), "peaked": S.peaked_state, "gated": S.gated_state,
             "sunk": lambda: S.peaked_state(sink=S.PEAKED_SINK)}[which]()
    emb, seq = S.stage_case(L, halo)
    x = T.features(emb, seq, STATS)
    return state, x, S.chain(x, state, F64), S.chain(x, state, F32)


def _refused(got, t64, t32, label):
    with pytest.raises(AssertionError):
        S.check_stage(got, t64, t32, label + " (breach)")


# -------------------------------------------------------------------------------------------------- the inputs excite (part 2)
@pytest.mark.parametrize("L", PEAKED_LS)
def test_peaked_state_needs_the_right_row_maximum(L):
    _, _, c64, c32 = _images("peaked", L)
    s = S.attn_scores(c64["q"], c64["k"])
    top = torch.softmax(s, dim=-1).max(dim=-1).values
    arg = s.argmax(dim=-1)
    last = (L - 1) // KEYS * KEYS
    print(f"peaked L={L}: largest |scaled logit| {float(s.abs().max()):.1f}, median largest weight {float(top.median()):.4f}, "
          f"rows with the maximum at j >= 64: {int((arg >= KEYS).sum())}, in the last chunk [{last}, {L}): {int((arg >= last).sum())}")
    assert float(s.abs().max()) >= 120.0
    assert float(top.median()) >= 0.9
    if L in (97, 129):
        assert int((arg >= KEYS).sum()) > 0 and int((arg >= last).sum()) > 0 and L % KEYS != 0
        # and far enough above the first chunk's maximum for exp() to overflow if that were the one subtracted
        gap = s[..., KEYS:].max(dim=-1).values - s[..., :KEYS].max(dim=-1).values
        print(f"peaked L={L}: rows more than 89 above the maximum of their first 64 keys: {int((gap > 89.0).sum())}")
        assert int((gap > 89.0).sum()) > 0
    for c in (c64, c32):
        assert all(bool(torch.isfinite(c[n]).all()) for n in S.IMAGES + ("sums", "logits"))


@pytest.mark.parametrize("L", [33, 97])
def test_sunk_head_has_every_real_logit_below_minus_100(L):
    _, _, c64, c32 = _images("sunk", L)
    s = S.attn_scores(c64["q"], c64["k"])
    assert float(s[0].max()) < -100.0 and float(s[1:].max()) > 0.0
    assert bool(torch.isfinite(c64["logits"]).all()) and bool(torch.isfinite(c32["logits"]).all())


@pytest.mark.parametrize("L", [33, 1024])
def test_gated_state_has_a_live_gate_that_follows_the_last_tile(L):
    state, x, c64, c32 = _images("gated", L)
    sd = S.tensors(state, F64)
    _, hid, z = S.se_gate(c64["sums"], L, sd)
    z = z.view(-1)
    assert int((hid > 0).sum()) >= 2
    assert int((z > 0).sum()) > 0 and int((z < 0).sum()) > 0 and int((z.abs() < 2).sum()) >= PLANES // 2
    moved = c64["sums"].clone()
    moved[-1] *= 1.01
    z64 = c64["logits"]
    rel = float((S.attn(*S.mix(c64["shortcut"], c64["h2"], moved, sd), sd) - z64).norm() / z64.norm())
    bar = T.L2_MULT * max(float((c32["logits"].to(F64) - z64).norm() / z64.norm()), T.L2_FLOOR)
    print(f"gated L={L}: live hidden units {int((hid > 0).sum())}, z > 0 on {int((z > 0).sum())} channels, |z| < 2 on "
          f"{int((z.abs() < 2).sum())}; last tile sum + 1 %: logits move by rel-L2 {rel:.2e}, end-to-end bar {bar:.2e}")
    assert rel > bar


def test_halo_case_scales_the_seam_and_end_positions():
    emb, _ = S.halo_case(97, 3)
    plain, _ = S.case(97, 3)
    scaled = sorted({p % 97 for p in S.HALO_POSITIONS})
    assert scaled == [0, 31, 32, 63, 64, 96]
    for p in range(97):
        assert np.array_equal(emb[p], plain[p] * np.float32(8.0 if p in scaled else 1.0))


# --------------------------------------------------------------------------------------------------------------------- stem
RAW_PAD = np.concatenate([np.zeros(4), -STATS["emb_mu"].astype(np.float64) / STATS["emb_std"], [0.0]])
MASK_ONE = np.concatenate([np.zeros(772), [1.0]])


@pytest.mark.parametrize("L", [65, 97])
def test_stem_check_refuses_every_breach(L):
    state, x, _, c32 = _images("rand", L, halo=True)
    t64, t32 = S.stem(x, state, F64), S.stem(x, state, F32)
    assert torch.equal(t32[0], c32["h1"]) and torch.equal(t32[1], c32["shortcut"])
    zero_pad = S.stem(x, state, F32, pad=np.zeros(773))                   # the honest stem by another route
    for i, name in enumerate(("h1", "shortcut")):
        S.check_stage(t32[i], t64[i], t32[i], f"stem {name} L={L}: the restatement")
        S.check_stage(zero_pad[i], t64[i], t32[i], f"stem {name} L={L}: explicit zero columns")
    _refused(S.stem(x, state, F32, pad=RAW_PAD)[0], t64[0], t32[0], f"stem h1 L={L}: raw input padded")
    _refused(S.stem(x, state, F32, pad=MASK_ONE)[0], t64[0], t32[0], f"stem h1 L={L}: mask padded with ones")
    short = x.copy()
    short[768:773] = 0.0
    for i, name in enumerate(("h1", "shortcut")):
        _refused(S.stem(short, state, F32)[i], t64[i], t32[i], f"stem {name} L={L}: channels 768 .. 772 dropped")
    flipped = dict(state)
    flipped[B0 + "conv1.weight"] = state[B0 + "conv1.weight"][:, :, ::-1].copy()
    _refused(S.stem(x, flipped, F32)[0], t64[0], t32[0], f"stem h1 L={L}: taps reversed")


# -------------------------------------------------------------------------------------------------------------------- conv2
def _conv2_by_tiles(h1, sd, left=True, right=True, relu_first=False):
    """conv2 as the kernel stages it: per 32-position tile, one halo position on either side where the sequence goes on."""
    L = h1.shape[0]
    rows = h1.t()[None].contiguous()
    out = []
    for p0 in range(0, L, TILE):
        n = min(TILE, L - p0)
        xin = torch.zeros(1, PLANES, n + 2, dtype=h1.dtype)
        xin[:, :, 1:n + 1] = rows[:, :, p0:p0 + n]
        if p0 > 0 and left:
            xin[:, :, 0] = rows[:, :, p0 - 1]
        if p0 + n < L and right:
            xin[:, :, n + 1] = rows[:, :, p0 + n]
        c = F.conv1d(xin, sd[B0 + "conv2.weight"])
        out.append(S._bn(torch.relu(c), sd, B0 + "bn2") if relu_first else torch.relu(S._bn(c, sd, B0 + "bn2")))
    return torch.cat(out, dim=2)[0].t()


@pytest.mark.parametrize("L", [33, 65, 97])
def test_conv2_check_refuses_every_breach(L):
    state, _, _, c32 = _images("rand", L, halo=True)
    h1, sd = c32["h1"], S.tensors(state, F32)
    t64, t32 = S.conv2(h1, state, F64)[0], S.conv2(h1, state, F32)[0]
    assert torch.equal(t32, c32["h2"])
    S.check_stage(t32, t64, t32, f"conv2 L={L}: the restatement")
    S.check_stage(_conv2_by_tiles(h1, sd), t64, t32, f"conv2 L={L}: tile by tile with both halos")
    _refused(_conv2_by_tiles(h1, sd, left=False), t64, t32, f"conv2 L={L}: halo p0 - 1 read as zero")
    _refused(_conv2_by_tiles(h1, sd, right=False), t64, t32, f"conv2 L={L}: halo p0 + 32 read as zero")
    _refused(_conv2_by_tiles(h1, sd, relu_first=True), t64, t32, f"conv2 L={L}: ReLU before BatchNorm")


@pytest.mark.parametrize("L", [33, 97, 1024])
def test_tile_sum_check_refuses_every_breach(L):
    _, _, _, c32 = _images("gated" if L == 1024 else "rand", L, halo=L != 1024)
    h2 = c32["h2"]
    tiles = (L + TILE - 1) // TILE
    assert S.check_tile_sums(S.tile_sums(h2), h2, f"L={L}: torch's fp32 sums") <= 1.0
    one_by_one = torch.stack([functools.reduce(torch.add, list(h2[a:min(a + TILE, L)])) for a in range(0, L, TILE)])
    S.check_tile_sums(one_by_one, h2, f"L={L}: fp32 sums position by position")
    if L % TILE:                                                          # rows L .. of the buffer hold an older, longer image
        stale = torch.cat([h2, torch.full((tiles * TILE - L, PLANES), 0.25)])
        with pytest.raises(AssertionError):
            S.check_tile_sums(S.tile_sums(stale), h2, f"L={L}: ragged tile summed over 32 stale positions (breach)")
    for gone in {0, tiles - 1}:
        dropped = S.tile_sums(h2)
        dropped[gone] = 0.0
        with pytest.raises(AssertionError):
            S.check_tile_sums(dropped, h2, f"L={L}: tile {gone} dropped (breach)")


# ---------------------------------------------------------------------------------------------------------------------- mix
def _mix_variant(shortcut, h2, sums, sd, divisor=None, gate_shortcut=False, eps=1e-5, swap=False):
    L = h2.shape[0]
    w = torch.sigmoid(S.se_gate(sums, divisor or L, sd)[2])
    sh = S._rows(shortcut)
    y = torch.relu(S._rows(h2) * w + (sh * w if gate_shortcut else sh))[0].t()
    t = F.layer_norm(y, (PLANES,), sd[G0 + "ln1.weight"], sd[G0 + "ln1.bias"], eps=eps)
    q, k, v = (F.linear(t, sd[G0 + f"attn.{n}.weight"], sd[G0 + f"attn.{n}.bias"]) for n in ("query", "key", "value"))
    return (y, k, q, v) if swap else (y, q, k, v)


@pytest.mark.parametrize("L", [33, 97])
def test_mix_check_refuses_every_breach(L):
    state, _, _, c32 = _images("gated", L)
    sd = S.tensors(state, F32)
    args = (c32["shortcut"], c32["h2"], c32["sums"])
    t64, t32 = S.mix(*args, state, F64), S.mix(*args, state, F32)
    names = ("y", "q", "k", "v")
    assert all(torch.equal(t32[i], c32[n]) for i, n in enumerate(names))

    def run(label, expect, **kw):
        got = _mix_variant(*args, sd, **kw)
        for i, n in enumerate(names):
            if n in expect:
                _refused(got[i], t64[i], t32[i], f"mix {n} L={L}: {label}")
            elif expect != "all":
                S.check_stage(got[i], t64[i], t32[i], f"mix {n} L={L}: {label} (untouched image)")

    run("no fault", ())
    tiles = (L + TILE - 1) // TILE
    run("mean over 32 x tiles", ("y", "q", "k", "v"), divisor=TILE * tiles)
    run("gate on the shortcut too", ("y", "q", "k", "v"), gate_shortcut=True)
    run("LN1 with eps 1e-6", ("q", "k", "v"), eps=1e-6)
    run("q and k swapped", ("q", "k"), swap=True)


# --------------------------------------------------------------------------------------------------------------------- attn
def _context_in_kernel_order(q, k, v, row_max="real", scale=S.SCALE, zero_keys=False, head_xor=0, subtract=True):
    """The kernel's attention in torch fp32: sweep 1 the row maximum, sweep 2 the exponentials, sums inside a 64-key chunk and
    then over the chunks.  row_max: 'real' (keys [0, L)), 'first' (the first chunk only), 'padded' (the zero-filled slots j >= L
    of the last chunk included); zero_keys: those slots also enter the sums, with zero K and V."""
    L = q.shape[0]
    Lp = (L + KEYS - 1) // KEYS * KEYS
    Q, K, V = S.heads(q), S.heads(k), S.heads(v)
    if head_xor:
        K = K[[h ^ head_xor for h in range(HEADS)]]
    K, V = (F.pad(t, (0, 0, 0, Lp - L)) for t in (K, V))
    s = (Q @ K.transpose(-2, -1)) * scale                                 # [8][L][Lp], 0 at the padded slots
    mx = {"real": s[..., :L], "first": s[..., :min(KEYS, L)], "padded": s}[row_max].max(dim=-1, keepdim=True).values
    e = torch.exp(s - mx if subtract else s)
    n = Lp if zero_keys else L
    den, o = torch.zeros(HEADS, L, 1), torch.zeros(HEADS, L, PLANES // HEADS)
    for j0 in range(0, n, KEYS):
        j1 = min(j0 + KEYS, n)
        den = den + e[..., j0:j1].sum(dim=-1, keepdim=True)
        o = o + e[..., j0:j1] @ V[:, j0:j1]
    return (o / den).transpose(0, 1).contiguous().view(L, PLANES)


def _tail_variant(y, ctx, sd, gelu="none", bias=True):
    y = y + F.linear(ctx, sd[G0 + "attn.proj.weight"], sd[G0 + "attn.proj.bias"])
    t = F.layer_norm(y, (PLANES,), sd[G0 + "ln2.weight"], sd[G0 + "ln2.bias"], eps=1e-5)
    t = F.linear(F.gelu(F.linear(t, sd[G0 + "mlp.0.weight"], sd[G0 + "mlp.0.bias"]), approximate=gelu),
                 sd[G0 + "mlp.2.weight"], sd[G0 + "mlp.2.bias"])
    return F.linear(y + t, sd["final.weight"], sd["final.bias"] if bias else None)[:, 0]


def _attn_stage(which, L):
    state, _, _, c32 = _images(which, L)
    imgs = tuple(c32[n] for n in ("y", "q", "k", "v"))
    t64, t32 = S.attn(*imgs, state, F64), S.attn(*imgs, state, F32)
    assert torch.equal(t32, c32["logits"])
    return S.tensors(state, F32), imgs, t64, t32


@pytest.mark.parametrize("which,L", [("peaked", 97), ("peaked", 129), ("sunk", 97), ("rand", 97), ("rand", 33)])
def test_attn_check_passes_the_kernel_s_order(which, L):
    sd, (y, q, k, v), t64, t32 = _attn_stage(which, L)
    S.check_stage(t32, t64, t32, f"attn {which} L={L}: the restatement")
    S.check_stage(S.attn_tail(y, _context_in_kernel_order(q, k, v), sd), t64, t32, f"attn {which} L={L}: two sweeps, 64-key chunks")
    S.check_stage(_tail_variant(y, S.attn_context(q, k, v), sd), t64, t32, f"attn {which} L={L}: the tail restated")


@pytest.mark.parametrize("L", [97, 129])
def test_attn_check_refuses_a_wrong_row_maximum(L):
    sd, (y, q, k, v), t64, t32 = _attn_stage("peaked", L)
    for label, kw in (("row maximum over the first 64 keys", {"row_max": "first"}), ("no maximum subtracted", {"subtract": False})):
        got = S.attn_tail(y, _context_in_kernel_order(q, k, v, **kw), sd)
        assert not bool(torch.isfinite(got).all()), label                  # fp32 overflow: what makes the fault visible at all
        _refused(got, t64, t32, f"attn peaked L={L}: {label}")


def test_attn_check_refuses_a_maximum_that_includes_the_zero_filled_slots():
    """Head 0 of the sunk member: every real logit is below -100, so with the 31 zero-filled slots of the last chunk in the
    maximum every exponential of the row underflows to 0."""
    sd, (y, q, k, v), t64, t32 = _attn_stage("sunk", 97)
    got = S.attn_tail(y, _context_in_kernel_order(q, k, v, row_max="padded"), sd)
    _refused(got, t64, t32, "attn sunk L=97: row maximum over 64-padded keys")
    # on the peaked member every row maximum is positive and the same fault changes nothing: the sunk head is what shows it
    sd, (y, q, k, v), t64, t32 = _attn_stage("peaked", 97)
    S.check_stage(S.attn_tail(y, _context_in_kernel_order(q, k, v, row_max="padded"), sd), t64, t32, "attn peaked L=97: the same")


@pytest.mark.parametrize("which,L", [("rand", 97), ("rand", 33), ("sunk", 97)])
def test_attn_check_refuses_the_other_breaches(which, L):
    sd, (y, q, k, v), t64, t32 = _attn_stage(which, L)
    for label, kw in (("scale 1 / sqrt 64", {"scale": 1.0 / math.sqrt(PLANES)}),
                      ("keys j >= L of the last chunk included", {"zero_keys": True}),
                      ("head h reads the key channels of head h ^ 1", {"head_xor": 1})):
        _refused(S.attn_tail(y, _context_in_kernel_order(q, k, v, **kw), sd), t64, t32, f"attn {which} L={L}: {label}")
    ctx = S.attn_context(q, k, v)
    _refused(_tail_variant(y, ctx, sd, gelu="tanh"), t64, t32, f"attn {which} L={L}: tanh-GELU")
    _refused(_tail_variant(y, ctx, sd, bias=False), t64, t32, f"attn {which} L={L}: final bias dropped")
