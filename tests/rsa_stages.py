"""The RSA restatement (tests/rsa_truth.py) cut at the head's own four launches (csrc/rsa_head.hip: stem, conv2, mix, attn), the
check that holds one stage's image to it, and inputs that excite what random weights do not.  Test infrastructure only.

The head leaves every stage's output in its workspace -- per model h1, shortcut, h2, y, q, k, v ([L][64] each) and the tile sums
[32][64], model_floats(L) floats, no slot overwritten by a later stage -- so each stage can be held to the fp64 restatement of that
stage applied to the head's OWN input image (tests/test_gpu_rsa_head_stages.py): nothing cascades, and a failure names its stage.
The stage functions work on [L][64] images under the reference's parameter names and never see the packed weight table.
rsa_truth.logits_torch is their composition, bit for bit what it was as one function (tests/test_rsa_stages_host.py)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import rsa_truth as T
from rsa_truth import HEADS, PLANES

TILE, KEYS, MAX_TILES = 32, 64, 32       # positions per block, keys per streamed chunk, rows of the tile-sum slot
IMAGES = ("h1", "shortcut", "h2", "y", "q", "k", "v")
B0, G0 = "net.0.0.", "net.1.0."


def model_floats(L: int) -> int:
    """Floats of one model's slab of the workspace: the seven images, then the tile sums."""
    return 7 * L * PLANES + MAX_TILES * PLANES


def members_bytes(B: int) -> int:
    """Bytes of the descriptor table in front of a packed call's slabs (64 bytes per member, rounded up to 256)."""
    return (B * 64 + 255) & ~255


def tensors(state: dict, dtype) -> dict:
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in state.items() if not k.endswith("num_batches_tracked")}


def _args(sd, dtype, *images):
    """dtype None: tensors that already share a dtype (logits_torch); else arrays or tensors of any dtype, converted."""
    if dtype is None:
        return (sd,) + images
    return (tensors(sd, dtype),) + tuple(torch.as_tensor(np.asarray(a)).to(dtype) for a in images)


def _bn(h, sd, name):
    return F.batch_norm(h, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"],
                        training=False, eps=1e-5)


def _rows(img):
    """[L][64] image -> the network's [1, 64, L]."""
    return img.t()[None].contiguous()


# ------------------------------------------------------------------------------------------------------------------ the stages
def stem(x, sd, dtype=None, pad=None):
    """(h1, shortcut) [L][64] from the normalised features x [Cin, L] (rsa_truth.features).  pad: rsa_truth.logits."""
    sd, x = _args(sd, dtype, x)
    x = x[None]
    if pad is None:
        c1 = F.conv1d(x, sd[B0 + "conv1.weight"], padding=1)
    else:
        col = torch.as_tensor(np.asarray(pad)).to(x.dtype)[None, :, None] if not torch.is_tensor(pad) else pad[None, :, None]
        c1 = F.conv1d(torch.cat([col, x, col], dim=2), sd[B0 + "conv1.weight"])
    h1 = torch.relu(_bn(c1, sd, B0 + "bn1"))
    sh = _bn(F.conv1d(x, sd[B0 + "shortcut.0.weight"]), sd, B0 + "shortcut.1")
    return h1[0].t(), sh[0].t()


def tile_sums(h2, tile=TILE):
    """[tiles][64]: row i is the sum of the image h2 [L][64] over positions tile * i .. min(tile * (i + 1), L)."""
    rows = h2.t()
    L = rows.shape[1]
    tile = tile or L
    return torch.stack([rows[:, a:min(a + tile, L)].sum(dim=1) for a in range(0, L, tile)])


def conv2(h1, sd, dtype=None, tile=TILE):
    """(h2 [L][64], tile sums [tiles][64]).  tile None: one tile over the whole sequence (logits_torch: torch's own reduction)."""
    sd, h1 = _args(sd, dtype, h1)
    h = torch.relu(_bn(F.conv1d(_rows(h1), sd[B0 + "conv2.weight"], padding=1), sd, B0 + "bn2"))
    return h[0].t(), tile_sums(h[0].t(), tile)


def se_gate(sums, L, sd):
    """(channel mean [64], hidden units [4] after the ReLU, pre-sigmoid gate [64]) from the tile sums, added in tile order."""
    tot = sums[0]
    for i in range(1, sums.shape[0]):
        tot = tot + sums[i]
    mean = tot / L
    hid = torch.relu(F.conv1d(mean.view(1, PLANES, 1), sd[B0 + "fc1.weight"], sd[B0 + "fc1.bias"]))
    z = F.conv1d(hid, sd[B0 + "fc2.weight"], sd[B0 + "fc2.bias"])
    return mean, hid.view(-1), z


def mix(shortcut, h2, sums, sd, dtype=None):
    """(y, q, k, v) [L][64]: the squeeze mean as the tile sums over L, excite, gate, + shortcut, ReLU; LN1; the three projections."""
    sd, shortcut, h2, sums = _args(sd, dtype, shortcut, h2, sums)
    L = h2.shape[0]
    w = torch.sigmoid(se_gate(sums, L, sd)[2])
    y = torch.relu(_rows(h2) * w + _rows(shortcut))[0].t()
    t = F.layer_norm(y, (PLANES,), sd[G0 + "ln1.weight"], sd[G0 + "ln1.bias"], eps=1e-5)
    q, k, v = (F.linear(t, sd[G0 + f"attn.{n}.weight"], sd[G0 + f"attn.{n}.bias"]) for n in ("query", "key", "value"))
    return y, q, k, v


def heads(img):
    """[L][64] -> [8 heads][L][8]."""
    return img.view(img.shape[0], HEADS, PLANES // HEADS).transpose(0, 1)


SCALE = 1.0 / math.sqrt(PLANES // HEADS)


def attn_scores(q, k):
    """[8][L][L] scaled attention logits."""
    return (heads(q) @ heads(k).transpose(-2, -1)) * SCALE


def attn_context(q, k, v):
    att = torch.softmax(attn_scores(q, k), dim=-1)
    return (att @ heads(v)).transpose(0, 1).contiguous().view(q.shape[0], PLANES)


def attn_tail(y, ctx, sd):
    y = y + F.linear(ctx, sd[G0 + "attn.proj.weight"], sd[G0 + "attn.proj.bias"])
    t = F.layer_norm(y, (PLANES,), sd[G0 + "ln2.weight"], sd[G0 + "ln2.bias"], eps=1e-5)
    t = F.linear(F.gelu(F.linear(t, sd[G0 + "mlp.0.weight"], sd[G0 + "mlp.0.bias"])), sd[G0 + "mlp.2.weight"], sd[G0 + "mlp.2.bias"])
    y = y + t
    return F.linear(y, sd["final.weight"], sd["final.bias"])[:, 0]


def attn(y, q, k, v, sd, dtype=None):
    """logits [L]: softmax attention (8 heads of 8, 1 / sqrt 8 on the logit), proj + residual, LN2, erf-GELU MLP + residual, final."""
    sd, y, q, k, v = _args(sd, dtype, y, q, k, v)
    return attn_tail(y, attn_context(q, k, v), sd)


def chain(x, state, dtype, tile=TILE):
    """Every image of the restatement on the features x, each stage fed the one before: a dict over IMAGES, 'sums', 'logits'."""
    sd = tensors(state, dtype)
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    out = {}
    out["h1"], out["shortcut"] = stem(x, sd)
    out["h2"], out["sums"] = conv2(out["h1"], sd, tile=tile)
    out["y"], out["q"], out["k"], out["v"] = mix(out["shortcut"], out["h2"], out["sums"], sd)
    out["logits"] = attn(out["y"], out["q"], out["k"], out["v"], sd)
    return out


# ------------------------------------------------------------------------------------------------------------------ the checks
def check_stage(got, t64, t32, label: str, l2_mult: float = T.L2_MULT, ew_mult: float = T.EW_MULT) -> dict:
    """The project's rule for heads (rsa_truth.compare and its constants) on one image of one stage: t64 and t32 are the fp64 and
    the fp32 restatement of THAT stage on the same input image.  Prints what it measured; returns the two ratios to the bars'
    yardsticks (rel-L2 over max(the restatement's, the floor); max-abs over the restatement's)."""
    got, t64, t32 = (np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64) for a in (got, t64, t32))
    assert got.shape == t64.shape == t32.shape, f"{label}: shapes {got.shape} {t64.shape} {t32.shape}"
    assert np.isfinite(t64).all() and np.isfinite(t32).all(), f"{label}: the restatement is not finite"
    assert np.isfinite(got).all(), f"{label}: {int((~np.isfinite(got)).sum())} of {got.size} values are not finite"
    norm = max(float(np.linalg.norm(t64)), 1e-30)
    err, drift = float(np.linalg.norm(got - t64)) / norm, float(np.linalg.norm(t32 - t64)) / norm
    d, d32 = float(np.abs(got - t64).max()), float(np.abs(t32 - t64).max())
    ulp = float(np.spacing(np.float32(np.abs(t64).max())))
    ew_bar = ew_mult * d32 + T.EW_ULPS * ulp
    r = {"l2": err / max(drift, T.L2_FLOOR), "ew": d / max(d32, 1e-30), "ew_bar": d / max(ew_bar, 1e-30), "err": err, "drift": drift}
    msg = (f"{label}: rel-L2 {err:.2e} (fp32 restatement {drift:.2e}, ratio to max(it, floor) {r['l2']:.2f}, bar {l2_mult:g}), max-abs "
           f"{d:.2e} (restatement {d32:.2e}, ratio {r['ew']:.2f}; bar {ew_bar:.2e}, share {r['ew_bar']:.2f})")
    print(msg)
    assert err <= l2_mult * max(drift, T.L2_FLOOR), msg
    assert d <= ew_bar, msg
    return r


SUM_BAR = TILE * 2.0 ** -24


def check_tile_sums(got, h2, label: str) -> float:
    """The tile sums [tiles][64] against the fp64 sums of the image h2 they were taken from.  h2 is not negative (a ReLU's output),
    so an fp32 sum of n <= 32 of its values in any order is within (n - 1) 2^-24 of the true one, relatively: the bar is 32 x 2^-24
    per entry, derived, not measured.  Returns the largest share of the bar."""
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64)
    want = tile_sums(torch.as_tensor(np.asarray(h2)).to(torch.float64)).numpy()
    assert got.shape == want.shape, f"{label}: {got.shape[0]} tile sums for {want.shape[0]} tiles"
    assert np.isfinite(got).all() and (want >= 0).all(), label
    dev, bar = np.abs(got - want), SUM_BAR * want
    share = float((dev / np.maximum(bar, 1e-300)).max()) if (want > 0).any() else 0.0
    i = np.unravel_index(np.argmax(dev - bar), dev.shape)
    msg = f"{label}: tile sums, largest share of the 32 x 2^-24 bar {share:.3f}; worst entry {i}: {got[i]!r} for {want[i]!r}"
    print(msg)
    assert (dev <= bar).all(), msg
    return share


# ------------------------------------------------------------------------------------------------------------------ the inputs
def case(L: int, seed: int):
    """An embedding with the shipped statistics' spread and a sequence with characters outside A, C, G, U (the _case of the
    head's other tests)."""
    rng = np.random.RandomState(seed)
    st = T.load_stats("oh")
    emb = (st["emb_mu"] + st["emb_std"] * rng.standard_normal((L, 768))).astype(np.float32)
    seq = "".join(rng.choice(list("ACGU"), L))
    if L > 3:
        seq = seq[:1] + "N" + seq[2:-1] + "t"
    return emb, seq


HALO_POSITIONS, HALO_GAIN = (0, 31, 32, 63, 64, -1), 8.0


def halo_case(L: int, seed: int):
    """case() with the positions on both sides of the 32-position seams and at both ends multiplied by 8: a wrong or missing
    one-position halo there moves the neighbouring outputs by a multiple of their size."""
    emb, seq = case(L, seed)
    for p in HALO_POSITIONS:
        if p < L:
            emb[p] *= np.float32(HALO_GAIN)
    return emb, seq


def stage_case(L: int, halo: bool = False):
    """The one input per length of the stage tests, on the CPU and on the GPU: the conditions asserted on the CPU
    (tests/test_rsa_stages_host.py) are conditions of these inputs."""
    return (halo_case if halo else case)(L, 900 + L)


# peaked_state: gain and seed are chosen on the CPU so that the conditions of tests/test_rsa_stages_host.py hold on the fp64
# restatement of stage_case(L) at every L >= 33 of the GPU cases.  The scaled logits grow with the square of the gain.  Gain 5
# already gives a largest |logit| of 182 .. 261 and a median largest softmax weight of 0.989 .. 0.9998, but a row's maximum over
# its first 64 keys is then never more than 52 below its true maximum at L = 97 and 129: a maximum taken over the first chunk only
# would still not overflow (e^88), and the breach stays invisible.  At gain 8 the gap exceeds 89 on 12 rows at L = 97, 3 at
# L = 129 and 1 at L = 65 (gain 7: 2, 1, 0).  Seeds 11 .. 22 all meet the first two conditions; at L = 129 seeds 14, 15 and 22
# have no row whose maximum is the lone key of the last chunk, seed 11 has 17 (and 19 at L = 65).
PEAKED_SEED, PEAKED_GAIN = 11, 8.0
# sink: +sink on the query bias and -sink on the key bias of channel 0 of head 0 (after the gain), so that every logit of head 0
# is near -sink^2 / sqrt 8 and its row maxima lie far below -100 -- where a maximum that includes zero-filled slots is 0 instead.
PEAKED_SINK = 64.0


def peaked_state(seed: int = PEAKED_SEED, gain: float = PEAKED_GAIN, sink: float = 0.0) -> dict:
    """A make_state member whose attn.query and attn.key weights and biases are multiplied by gain."""
    sd = T.make_state(seed)
    for n in ("query", "key"):
        for p in ("weight", "bias"):
            sd[G0 + f"attn.{n}.{p}"] = (sd[G0 + f"attn.{n}.{p}"] * np.float32(gain)).astype(np.float32)
    if sink:
        sd[G0 + "attn.query.bias"][0] += np.float32(sink)
        sd[G0 + "attn.key.bias"][0] -= np.float32(sink)
    return sd


# gated_state: make_state(11) as it stands has 3 live hidden units and every |z| < 1 (a gate near 1/2 everywhere); fc1 x 4 and
# fc2 x 2 spread z to both sides of 0 with 44 .. 46 of 64 channels inside |z| < 2 and 2 .. 3 hidden units alive at L = 33 and 1024.
GATED_SEED, GATED_FC1, GATED_FC2 = 11, 4.0, 2.0


def gated_state(seed: int = GATED_SEED, fc1: float = GATED_FC1, fc2: float = GATED_FC2) -> dict:
    """A make_state member whose squeeze-excite weights are scaled (fc1.weight by fc1, fc2.weight by fc2) so that the gate sits on
    the slope of the sigmoid and follows the channel means (conditions: tests/test_rsa_stages_host.py)."""
    sd = T.make_state(seed)
    sd[B0 + "fc1.weight"] = (sd[B0 + "fc1.weight"] * np.float32(fc1)).astype(np.float32)
    sd[B0 + "fc2.weight"] = (sd[B0 + "fc2.weight"] * np.float32(fc2)).astype(np.float32)
    return sd
