"""Every launch of the RSA head (csrc/rsa_head.hip: stem, conv2, mix, attn) held to fp64 on its OWN input image.

One call of rnamsm_rsa_head on a NaN-filled workspace leaves per model h1, shortcut, h2, y, q, k, v ([L][64]) and the tile sums
([32][64], the first ceil(L / 32) rows written) in that order -- rsa_stages.model_floats(L) floats, the layout this file pins.
Each stage is then compared with the fp64 restatement of that stage (tests/rsa_stages.py) applied to the images the DEVICE
produced for its input, with the fp32 CPU restatement on the same images as the yardstick (rsa_stages.check_stage: the bars and
constants of rsa_truth.compare), so nothing cascades and a failure names its stage; the tile sums are held to the fp64 sums of the
device's h2 at 32 x 2^-24 per entry (rsa_stages.check_tile_sums).  tests/test_rsa_stages_host.py shows on the CPU which faults
these checks refuse, and that the peaked, sunk, gated and halo inputs excite what random weights leave asleep: a row maximum
that must be right (logits of several hundred, maxima in later and partial key chunks, a head whose logits are all below -100),
a squeeze-excite gate on the slope of its sigmoid, and positions of 8 x the size on both sides of every tile seam.
Measured ratios: tests/analysis/README.md."""
import ctypes

import numpy as np
import pytest
import torch

import rsa_stages as S
import rsa_truth as T
from rnamsm import _lib, rsa, ss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
PLANES, TILE = S.PLANES, S.TILE
GUARD = 4096                       # bytes behind the workspace the call is told about: they must stay as they were
STAGES = ("stem", "conv2", "mix", "attn")
# The one stage and input that needs the rule's provision (at most 4 x, named and recorded: tests/analysis/README.md):
# h1 of the stem on the halo embedding.  The stem adds its 800 x 3 products in chains of 200 (one accumulator per tap and quarter
# of every 32-channel step, then summed in fixed order), F.conv1d in the CPU library's blocked order.  Measured rel-L2 to fp64 at
# L >= 31: the head 1.9e-7 .. 2.6e-7 on plain embeddings and 1.9e-7 .. 3.0e-7 on the halo ones, the fp32 restatement
# 1.4e-7 .. 1.9e-7 and 1.2e-7 .. 2.1e-7 -- a few positions of 8 x the size carry the norm there, and the blocked order loses
# less on them.  Ratio at most 1.47 on every plain input; halo L = 65: 1.83, 2.07 and 1.64 (the three members), L = 97: 1.44 .. 1.53.
# Element-wise the same images are at 0.59 of their bar or less.
STEM_HALO_L2_MULT = 4.0


def _states(which):
    if which == "rand3":
        return [T.make_state(11 + k) for k in range(3)], "oh"
    if which == "randemb1":
        return [T.make_state(21, cin=769)], "emb"
    if which == "real3":
        return [T.load_state(f"state_oh_{k}") for k in range(3)], "oh"
    if which == "peaked":          # the peaked member and the same with head 0 sunk below -100
        return [S.peaked_state(), S.peaked_state(sink=S.PEAKED_SINK)], "oh"
    assert which == "gated"
    return [S.gated_state()], "oh"


_ENS = {}


def _ensemble(which):
    """(ensemble on the device, the members' states, kind), built once and left unchanged."""
    if which not in _ENS:
        states, kind = _states(which)
        st = T.load_stats(kind)
        stats = {"emb": (st["emb_mu"], st["emb_std"])}
        if kind == "oh":
            stats["oh"] = (st["oh_mu"], st["oh_std"])
        members = [rsa.RSAPredictor.from_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}) for sd in states]
        _ENS[which] = (rsa.RSAEnsemble(members, stats).eval().to(DEV), states, kind)
    return _ENS[which]


def _slabs(floats, L, K):
    """Views of K consecutive model slabs in a host float tensor: per model a dict over rsa_stages.IMAGES and 'sums' (the rows
    the head writes).  Every float of those is finite; the rows of the tile-sum slot beyond ceil(L / 32) were never written."""
    mf, tiles = S.model_floats(L), (L + TILE - 1) // TILE
    out = []
    for m in range(K):
        slab = floats[m * mf:(m + 1) * mf]
        imgs = slab[:7 * L * PLANES].view(7, L, PLANES)
        sums = slab[7 * L * PLANES:].view(S.MAX_TILES, PLANES)
        assert bool(torch.isfinite(imgs).all()), f"model {m}: {int((~torch.isfinite(imgs)).sum())} floats of the images are not finite"
        assert bool(torch.isfinite(sums[:tiles]).all()) and bool(torch.isnan(sums[tiles:]).all()), f"model {m}: tile sums"
        d = {n: imgs[i] for i, n in enumerate(S.IMAGES)}
        d["sums"] = sums[:tiles]
        out.append(d)
    return out


def _lone(ens, emb, seq):
    """One rnamsm_rsa_head call on a NaN-filled workspace of exactly rnamsm_rsa_head_workspace_bytes(L, K) -> (slabs, logits)."""
    lib = _lib.load()
    K, L = len(ens), len(seq)
    nbytes = lib.rnamsm_rsa_head_workspace_bytes(L, K)
    assert nbytes == 4 * K * S.model_floats(L)
    ws = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)          # 0xFFFFFFFF: a NaN in every float
    logits = torch.full((K, L), float("nan"), device=DEV)
    e = torch.from_numpy(emb).to(DEV)
    codes = torch.from_numpy(ss.base_codes(seq)).to(DEV)
    ptrs, _ = ens._packed_weights()
    _lib.check(lib.rnamsm_rsa_head(e.data_ptr(), 768, codes.data_ptr(), L, K, 1 if ens.use_onehot else 0, ptrs, None,
                                   logits.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    host = ws.cpu()
    assert bool((host[nbytes:] == 0xFF).all()), "bytes behind the workspace were written"
    logits = logits.cpu()
    assert bool(torch.isfinite(logits).all())
    return _slabs(host[:nbytes].view(F32), L, K), logits


_RUNS = {}


def _run(which, L, halo=False):
    """The device's images of one case and what the restatements need, computed once, shared by the four stage tests and left
    unchanged: (states, features, slabs, logits)."""
    key = (which, L, halo)
    if key not in _RUNS:
        ens, states, kind = _ensemble(which)
        emb, seq = S.stage_case(L, halo)
        x = T.features(emb, seq, T.load_stats(kind), use_onehot=kind == "oh")
        _RUNS[key] = (states, x) + _lone(ens, emb, seq)
    return _RUNS[key]


def _check(stage, which, L, halo=False):
    states, x, slabs, logits = _run(which, L, halo)
    for m, (state, dev) in enumerate(zip(states, slabs)):
        tag = f"{which}{' halo' if halo else ''} L={L} model {m}"
        if stage == "stem":
            t64, t32 = S.stem(x, state, F64), S.stem(x, state, F32)
            S.check_stage(dev["h1"], t64[0], t32[0], f"{tag} stem h1", l2_mult=STEM_HALO_L2_MULT if halo else T.L2_MULT)
            S.check_stage(dev["shortcut"], t64[1], t32[1], f"{tag} stem shortcut")
        elif stage == "conv2":
            S.check_stage(dev["h2"], S.conv2(dev["h1"], state, F64)[0], S.conv2(dev["h1"], state, F32)[0], f"{tag} conv2 h2")
            S.check_tile_sums(dev["sums"], dev["h2"], f"{tag} conv2")
        elif stage == "mix":
            args = (dev["shortcut"], dev["h2"], dev["sums"])
            t64, t32 = S.mix(*args, state, F64), S.mix(*args, state, F32)
            for i, n in enumerate(("y", "q", "k", "v")):
                S.check_stage(dev[n], t64[i], t32[i], f"{tag} mix {n}")
        else:
            args = (dev["y"], dev["q"], dev["k"], dev["v"])
            # one to three logits: the ratio of single roundings, rsa_truth.L2_MULT_SHORT as for the whole head at L <= 3
            S.check_stage(logits[m], S.attn(*args, state, F64), S.attn(*args, state, F32), f"{tag} attn logits",
                          l2_mult=T.L2_MULT_SHORT if L <= 3 else T.L2_MULT)


@pytest.mark.parametrize("L", [1, 2, 31, 32, 33, 63, 64, 65, 97, 129, 1024])
@pytest.mark.parametrize("stage", STAGES)
def test_random_weights_three_members(stage, L):
    _check(stage, "rand3", L)


@pytest.mark.parametrize("L", [35, 65])
@pytest.mark.parametrize("which", ["randemb1", "real3"])
@pytest.mark.parametrize("stage", STAGES)
def test_embedding_only_and_shipped_weights(stage, which, L):
    _check(stage, which, L)


@pytest.mark.parametrize("L", [33, 64, 65, 97, 129, 1024])
@pytest.mark.parametrize("stage", STAGES)
def test_peaked_attention(stage, L):
    """Scaled logits of several hundred, row maxima in every chunk (the lone key of the last one at L = 65 and 129), and as
    second member the same with every logit of head 0 below -100."""
    _check(stage, "peaked", L)


@pytest.mark.parametrize("L", [33, 64, 65, 97, 129, 1024])
def test_peaked_attention_end_to_end(L):
    states, x, _, logits = _run("peaked", L)
    t64 = np.stack([T.logits(x, sd, F64) for sd in states])
    t32 = np.stack([T.logits(x, sd, F32) for sd in states]).astype(np.float64)
    T.compare(logits.numpy(), t64, t32, f"peaked L={L}, whole head")


@pytest.mark.parametrize("L", [33, 1024])
@pytest.mark.parametrize("stage", STAGES)
def test_live_squeeze_excite_gate(stage, L):
    _check(stage, "gated", L)


@pytest.mark.parametrize("L", [65, 97])
@pytest.mark.parametrize("stage", STAGES)
def test_halo_positions_of_eight_times_the_size(stage, L):
    _check(stage, "rand3", L, halo=True)


def test_packed_members_hold_the_bits_of_their_lone_runs_slab_by_slab():
    """One packed call over (97, 1, 64, 33): behind the descriptor table of rsa_stages.members_bytes(B) bytes the members'
    slabs follow in member order, K models each, with the bits of that member's lone run in all seven images and the tile sums;
    nothing behind the last slab is touched."""
    ens, _, _ = _ensemble("peaked")
    lib = _lib.load()
    Ls = [97, 1, 64, 33]
    B, K = len(Ls), len(ens)
    cases = [S.stage_case(L) for L in Ls]
    nbytes = lib.rnamsm_rsa_head_packed_workspace_bytes(B, (ctypes.c_int * B)(*Ls), K)
    floats = [K * S.model_floats(L) for L in Ls]
    assert nbytes == S.members_bytes(B) + 4 * sum(floats)
    ws = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    embs = [torch.from_numpy(e).to(DEV) for e, _ in cases]
    codes = [torch.from_numpy(ss.base_codes(s)).to(DEV) for _, s in cases]
    outs = [torch.full((K, L), float("nan"), device=DEV) for L in Ls]
    items = (_lib.RsaItem * B)()
    for b, L in enumerate(Ls):
        items[b] = _lib.RsaItem(embs[b].data_ptr(), 768, codes[b].data_ptr(), L, None, outs[b].data_ptr())
    ptrs, _ = ens._packed_weights()
    _lib.check(lib.rnamsm_rsa_head_packed(items, B, K, 1, ptrs, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    host = ws.cpu()
    assert bool((host[nbytes:] == 0xFF).all()), "bytes behind the workspace were written"
    body = host[S.members_bytes(B):nbytes].view(F32)
    assert body.numel() == sum(floats)
    off = 0
    for b, L in enumerate(Ls):
        _, _, lone, lone_logits = _run("peaked", L)
        packed = _slabs(body[off:off + floats[b]], L, K)
        off += floats[b]
        for m in range(K):
            for n in S.IMAGES + ("sums",):
                assert torch.equal(packed[m][n], lone[m][n]), f"member {b} (L = {L}), model {m}: {n}"
        assert torch.equal(outs[b].cpu(), lone_logits), f"member {b} (L = {L}): logits"
