"""fp64 truth for the RNA-MSM-SS head (rnamsm.ss): the reference's network (_downstream_tasks/SS/code/model.py) restated in
torch functional form, at any dtype.  Test infrastructure only: tests/test_ss_truth.py ties it to the reference's own output
(ss_head_b2_l35.npz); the GPU tests then check the HIP head against it at every size."""
import numpy as np
import torch
import torch.nn.functional as F

from rnamsm import ss


def features(atp: np.ndarray, seq, rows=None, cols=None) -> np.ndarray:
    """[128, R, C]: outer one-hot of the sequence (channels 0-3: base i, 4-7: base j) and the 120 maps, on the crop
    rows [r0, r1) x cols [c0, c1) of the [L, L] image (default: the whole image); atp is that crop, [120, R, C].
    seq: the whole query (str) or its base codes (uint8 [L], ss.base_codes)."""
    codes = ss.base_codes(seq) if isinstance(seq, str) else np.asarray(seq, dtype=np.uint8).reshape(-1)
    r0, r1 = rows if rows is not None else (0, atp.shape[-2])
    c0, c1 = cols if cols is not None else (0, atp.shape[-1])
    assert atp.shape[-2:] == (r1 - r0, c1 - c0), (atp.shape, rows, cols)

    def onehot(c):
        oh = np.zeros((len(c), 4))
        ok = c < 4
        oh[np.nonzero(ok)[0], c[ok]] = 1.0
        return oh

    x = np.zeros((128, r1 - r0, c1 - c0))
    x[0:4] = onehot(codes[r0:r1]).T[:, :, None]
    x[4:8] = onehot(codes[c0:c1]).T[:, None, :]
    x[8:] = atp
    return x


def receptive_margin(num_blocks: int) -> int:
    """An output pixel depends on inputs within this many pixels: 1 for the stem's 3x3, then 1 + 2 per block."""
    return 1 + 3 * num_blocks


def logits_window(atp, seq, state: dict, rows, cols, dtype=torch.float64, device="cpu", margin=None) -> np.ndarray:
    """The block rows [r0, r1) x cols [c0, c1) of logits(features(atp, seq), state), computed on a crop that reaches
    `margin` pixels beyond the block (default: the receptive margin, which gives the full map's result exactly), clipped
    at the image border, where the crop's zero padding is the image's own.  atp: [120, L, L], a host array or a device
    tensor; only the crop is copied."""
    nb = sum(1 for k in state if k.endswith(".conv2.weight"))
    m = receptive_margin(nb) if margin is None else margin
    L = atp.shape[-1]
    (r0, r1), (c0, c1) = rows, cols
    assert 0 <= r0 < r1 <= L and 0 <= c0 < c1 <= L, (rows, cols, L)
    R0, R1, C0, C1 = max(0, r0 - m), min(L, r1 + m), max(0, c0 - m), min(L, c1 + m)
    crop = atp[:, R0:R1, C0:C1]
    if isinstance(crop, torch.Tensor):
        crop = crop.detach().to("cpu", torch.float64).numpy()
    y = logits(features(crop, seq, (R0, R1), (C0, C1)), state, dtype, device)
    return y[r0 - R0:r1 - R0, c0 - C0:c1 - C0]


def make_state(num_blocks: int, seed: int, beta_scale: float = 0.3) -> dict:
    """Random parameters of every kind (LayerNorm affines and both biases included), float32 numpy, reference names."""
    rng = np.random.RandomState(seed)
    sd = {}

    def conv(name, cout, cin, k):
        sd[name] = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)

    def ln(name):
        sd[name + ".weight"] = (1.0 + 0.3 * rng.standard_normal(48)).astype(np.float32)
        sd[name + ".bias"] = (beta_scale * rng.standard_normal(48)).astype(np.float32)

    conv("conv1.weight", 48, 128, 3)
    sd["conv1.bias"] = (0.3 * rng.standard_normal(48)).astype(np.float32)
    ln("bn1")
    for k in range(num_blocks):
        conv(f"layer1.{k}.conv1.weight", 48, 48, 3)
        ln(f"layer1.{k}.bn1")
        conv(f"layer1.{k}.conv2.weight", 48, 48, 5)
        ln(f"layer1.{k}.bn2")
    sd["fc1.weight"] = (rng.standard_normal((1, 48)) / np.sqrt(48)).astype(np.float32)
    sd["fc1.bias"] = (0.3 * rng.standard_normal(1)).astype(np.float32)
    return sd


def _ln_relu(x, sd, name):
    y = F.layer_norm(x.permute(1, 2, 0), (48,), sd[name + ".weight"], sd[name + ".bias"], eps=1e-5)
    return torch.relu(y.permute(2, 0, 1))


def _conv(x, w, b=None):
    """nn.Conv2d(padding=k // 2) on [C, H, W], as a sum over the k x k taps of [O, C] x [C, H, W] products.
    Every output element is then summed in an order that does not depend on H or W (F.conv2d's single GEMM over C k k
    is split by the CPU BLAS differently for different image sizes), which makes logits_window exact."""
    k = w.shape[-1]
    p = k // 2
    H, W = x.shape[-2:]
    xp = F.pad(x, (p, p, p, p))
    out = torch.zeros(w.shape[0], H, W, dtype=x.dtype, device=x.device)
    for dy in range(k):
        for dx in range(k):
            out += torch.einsum("oc,chw->ohw", w[:, :, dy, dx], xp[:, dy:dy + H, dx:dx + W])
    return out if b is None else out + b[:, None, None]


def logits(x: np.ndarray, state: dict, dtype=torch.float64, device="cpu") -> np.ndarray:
    """[L, L] pre-sigmoid output of the head on features x [128, L, L]."""
    sd = {k: (v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))).to(device=device, dtype=dtype)
          for k, v in state.items()}
    nb = sum(1 for k in sd if k.endswith(".conv2.weight"))
    # fp64: the tap-wise sum (exact windows); any other dtype: F.conv2d, the reference network's own arithmetic (nn.Conv2d) --
    # the fp32 restatement is the yardstick of the GPU tests' bars and stays what those bars were measured against
    conv = _conv if dtype == torch.float64 else (lambda v, w, b=None: F.conv2d(v[None], w, b, padding=w.shape[-1] // 2)[0])
    h = torch.as_tensor(x).to(device=device, dtype=dtype)
    h = conv(h, sd["conv1.weight"], sd["conv1.bias"])
    for k in range(nb):
        p = f"layer1.{k}"
        t = conv(_ln_relu(h, sd, p + ".bn1"), sd[p + ".conv1.weight"])
        h = conv(_ln_relu(t, sd, p + ".bn2"), sd[p + ".conv2.weight"]) + h
    y = _ln_relu(h, sd, "bn1").permute(1, 2, 0) @ sd["fc1.weight"][0] + sd["fc1.bias"][0]
    return y.cpu().numpy()


# element-wise bar of the GPU tests: max-abs vs fp64 within EW_MULT x the fp32 restatement's max-abs on the same pixels
# (floor: EW_FLOOR x the largest |logit|); the rel-L2 bar is _check's, 2 x the restatement's (tests/analysis/README.md)
EW_MULT, EW_FLOOR = 4.0, 1e-7
L2_MULT, L2_FLOOR = 2.0, 1e-7


def compare(got, t64, t32, label: str = "", seams: bool = False, floor: float = None, l2_mult: float = L2_MULT) -> float:
    """Assert that the HIP logits `got` are as close to the fp64 truth `t64` as the fp32 restatement `t32` is, on the same
    pixels: by rel-L2 and element-wise.  seams=True (`got` a whole [L, L] map): also report the worst error on the border
    pixels (rows / columns 0, 1, L - 2, L - 1) and on the tile-seam pixels (index mod 16 in {0, 15}).  floor: one relative
    floor for both bars in place of L2_FLOOR / EW_FLOOR (a single pixel, where the restatement's error is one rounding sample
    and can be any fraction of an ulp).  l2_mult: the rel-L2 multiple, where the tolerance table records a finding.
    Returns the max-abs."""
    got, t64, t32 = (np.asarray(a, dtype=np.float64) for a in (got, t64, t32))
    assert got.shape == t64.shape == t32.shape and np.isfinite(got).all(), label
    d, d32 = np.abs(got - t64), np.abs(t32 - t64)
    err, drift = float(np.linalg.norm(got - t64)), float(np.linalg.norm(t32 - t64))
    norm = max(float(np.linalg.norm(t64)), 1e-30)
    err, drift = err / norm, drift / norm
    l2_floor, ew_floor = (L2_FLOOR, EW_FLOOR) if floor is None else (floor, floor)
    ew_bar = EW_MULT * max(float(d32.max()), ew_floor * float(np.abs(t64).max()))
    msg = (f"{label}: rel-L2 {err:.2e} (fp32 restatement {drift:.2e}), max-abs {d.max():.2e} (restatement {d32.max():.2e}, "
           f"bar {ew_bar:.2e}, ratio {d.max() / ew_bar:.2f})")
    if seams:
        L = got.shape[0]
        idx = np.arange(L)
        edge = np.isin(idx, [0, 1, L - 2, L - 1])
        seam = np.isin(idx % 16, [0, 15])
        worst = lambda m: float(d[m].max()) if m.any() else 0.0        # noqa: E731
        msg += (f"; worst border {worst(edge[:, None] | edge[None, :]):.2e}, "
                f"worst seam {worst(seam[:, None] | seam[None, :]):.2e}")
    print(msg)
    assert err <= l2_mult * max(drift, l2_floor), msg
    assert d.max() <= ew_bar, msg
    return float(d.max())


def check_nan_pattern(got, t64, t32, label: str, min_finite: float, expect_nan: bool) -> np.ndarray:
    """The non-finite side of a masked comparison, shared with rsa_truth.compare_masked: `got` is NaN exactly where the fp64
    truth is and holds no inf the truth does not hold; at least the share min_finite of the truth is finite, and at least one
    element is NaN where the caller expects one (so neither side of the comparison passes on an empty set).  The fp32
    restatement must be finite wherever the fp64 truth is: it is the yardstick of the bars there.  Returns the mask of the finite
    elements of t64."""
    assert got.shape == t64.shape == t32.shape, label
    nan64, fin64 = np.isnan(t64), np.isfinite(t64)
    share = float(fin64.mean())
    assert share >= min_finite, f"{label}: only {share:.3f} of the truth is finite, {min_finite} asked for"
    assert nan64.any() or not expect_nan, f"{label}: a NaN was expected in the truth and there is none"
    wrong = np.isnan(got) != nan64
    assert not wrong.any(), (f"{label}: NaN pattern differs from the truth's at {int(wrong.sum())} of {got.size} elements "
                             f"(truth {int(nan64.sum())} NaN, got {int(np.isnan(got).sum())}); first at "
                             f"{tuple(int(v) for v in np.argwhere(wrong)[0])}")
    extra_inf = np.isinf(got) & ~np.isinf(t64)
    assert not extra_inf.any(), f"{label}: {int(extra_inf.sum())} inf where the truth has none"
    assert np.isfinite(t32[fin64]).all(), f"{label}: the fp32 restatement is not finite where the fp64 truth is"
    return fin64


def compare_masked(got, t64, t32, label: str = "", min_finite: float = 0.0, expect_nan: bool = True, **bars) -> float:
    """compare() for truths that hold NaN (a non-finite input: the reference's ReLU, LayerNorm and convolutions carry it over the
    receptive square): the NaN pattern first (check_nan_pattern), then compare() itself -- the same bars, multiples and floors
    -- on the elements where the fp64 truth is finite.  bars: compare's floor / l2_mult.  Returns the max-abs on the finite
    elements (0 where there is none)."""
    got, t64, t32 = (np.asarray(a, dtype=np.float64) for a in (got, t64, t32))
    fin = check_nan_pattern(got, t64, t32, label, min_finite, expect_nan)
    if not fin.any():
        return 0.0
    return compare(got[fin], t64[fin], t32[fin], f"{label} [{int(fin.sum())} of {fin.size} finite]", **bars)


def small_maps_case(L: int, seed: int):
    """The inputs of the non-finite tests (CPU and GPU): maps uniform in [0, 0.1), float32 [120, L, L], and a sequence with one
    character outside A, C, G, U."""
    rng = np.random.RandomState(seed)
    atp = (0.1 * rng.rand(120, L, L)).astype(np.float32)
    seq = "".join(rng.choice(list("ACGU"), L))
    if L > 3:
        seq = seq[:2] + "N" + seq[3:]
    return atp, seq


def poisoned(atp: np.ndarray, plane: int, pixel, value: float) -> np.ndarray:
    """A copy of atp with the one element [plane, pixel] set to value (NaN, +inf, -inf)."""
    out = np.array(atp, copy=True)
    out[plane, pixel[0], pixel[1]] = value
    return out


def receptive_square(L: int, num_blocks: int, pixel) -> np.ndarray:
    """bool [L, L]: the output pixels whose window holds the input pixel -- within receptive_margin of it, clipped at the border."""
    m = receptive_margin(num_blocks)
    idx = np.arange(L)
    return (np.abs(idx - pixel[0]) <= m)[:, None] & (np.abs(idx - pixel[1]) <= m)[None, :]
