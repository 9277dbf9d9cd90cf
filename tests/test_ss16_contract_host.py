"""The per-stage contract checker of the bf16 SS head (tests/ss16_contract.py) without a GPU: that it has teeth.

The honest stand-in for the head is the yardstick's arithmetic with another summation order (ss_truth._conv, tap by tap in fp32,
where the yardstick has F.conv2d): it passes every stage at every case of tests/test_gpu_ss_head16_stages.py, and both conditions
of a usable case hold there (printed with every stage).  The mutants are torch fp32 restatements of ONE stage with ONE breach of
the contract, fed the stand-in's own images: each puts at least half of the stage's elements over the element-wise bar and exceeds
the rel-L2 bar -- but for the two whose breach cannot reach half of the elements, which assert what they reach and say why."""
import functools

import pytest
import torch

import ss16_contract as C
import ss_truth
from ss16_contract import F32, F64

NB = C.CASE_BLOCKS


@functools.lru_cache(maxsize=None)
def _cases():
    return C.small_cases()


@functools.lru_cache(maxsize=None)
def _standin(label):
    L, state, atp, seq = _cases()[label]
    feat = C.features32(atp, seq)
    images, logits = C.standin_chain(feat, state, NB)
    return state, feat, images, logits


# ---------------------------------------------------------------------- the rounding
def test_bf16_grid_is_torch_s_cast_on_fp32_values():
    g = torch.Generator().manual_seed(0)
    x = torch.rand(200_000, generator=g) * torch.exp2(torch.randint(-20, 6, (200_000,), generator=g).float())
    hi = x.to(torch.bfloat16).float()
    step = torch.exp2(torch.floor(torch.log2(hi.clamp(min=1e-30))) - 7)
    mid = hi + step / 2                                     # exact ties: fp32 has the bits
    tiny = torch.tensor([0.0, 2.0 ** -126, 2.0 ** -127, 2.0 ** -133, 3 * 2.0 ** -134, 1.0, 255 / 256, 1 - 2.0 ** -9, 3.0e38])
    v = torch.cat([x, mid, tiny])
    r, ulp, dist = C.bf16_grid(v.to(F64))
    assert torch.equal(r, C.rne(v))
    assert bool((dist <= ulp / 2).all()) and bool((dist[len(x):len(x) + len(mid)] == 0).all())
    assert bool(((r - v.to(F64)).abs() <= ulp / 2).all())
    # one rounding straight from fp64: 1 + 2^-8 + 2^-40 lies above the tie and goes up; through fp32 first it would land on the tie
    a = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -40], dtype=F64)
    assert C.bf16_grid(a)[0].item() == 1 + 2.0 ** -7 and a.float().to(torch.bfloat16).item() == 1.0
    t = C.truncate_bf16(v)
    assert bool((t <= v).all()) and bool((t.to(torch.bfloat16).float() == t).all()) and not torch.equal(t.to(F64), r)


# ---------------------------------------------------------------------- the stand-in passes, the conditions hold
@pytest.mark.parametrize("label", list(C.small_cases()))
def test_the_honest_stand_in_passes_every_stage(label):
    state, feat, images, logits = _standin(label)
    reps = C.check_chain(images, feat, state, NB, label, logits=logits)
    assert len(reps) == 2 + 2 * NB
    for r in reps:
        assert r.passed and r.ambiguous <= C.MAX_AMBIGUOUS and r.zero_share >= C.MIN_ZERO_ALLOWANCE, r.line()


def test_a_window_with_its_halo_is_the_whole_image_s_check():
    """The L = 1024 test checks windows of crops: the contract of a window computed on the crop that region() cuts -- the window and
    two pixels around it, clipped at the border -- has the bits of the whole image's, and the stand-in passes on it."""
    L = 40
    state = C.limit_state()
    atp, seq = C.case(L, 140)
    feat = C.features32(atp, seq)
    images, _ = C.standin_chain(feat, state, 1)
    (bn1, c1), (bn2, c2) = C.block_names(0)
    whole = {"X0": C.stem64(feat, state), "T1": C.trunk64(images["X0"], state, bn1, c1)[0],
             "X1": C.trunk64(images["T1"], state, bn2, c2, images["X0"])[0]}
    for rows, cols in (((0, 16), (0, 16)), ((24, 40), (0, 16)), ((32, 40), (32, 40)), ((8, 24), (8, 24)), ((39, 40), (3, 9))):
        (R0, R1), (C0, C1), inner = C.region(L, rows, cols)
        crop = {k: v[:, R0:R1, C0:C1] for k, v in images.items()}
        f = C.features32(atp[:, R0:R1, C0:C1], seq, (R0, R1), (C0, C1))
        assert torch.equal(f, feat[:, R0:R1, C0:C1])
        part = {"X0": C.stem64(f, state), "T1": C.trunk64(crop["X0"], state, bn1, c1)[0],
                "X1": C.trunk64(crop["T1"], state, bn2, c2, crop["X0"])[0]}
        for k in whole:
            assert torch.equal(part[k][:, inner[0], inner[1]], whole[k][:, rows[0]:rows[1], cols[0]:cols[1]]), (k, rows, cols)
        for r in C.check_chain(crop, f, state, 1, f"window {rows} x {cols}", inner):
            assert r.passed


# ---------------------------------------------------------------------- the mutants
def _trunk_mutant(X, state, bn, conv, residual=None, *, pre=None, ln_bf16=False, round_act=None, round_w=None, w_edit=None,
                  residual_mult=1.0, round_residual=False, pad_relu_beta=False):
    """trunk32 with the stand-in's tap-wise sums and the named breach."""
    sd = C.tensors(state, F32)
    X = C._img(X, F32)
    if pre is not None:
        X = pre(X)
    if ln_bf16:                                            # statistics and affine in bf16
        a = ss_truth._ln_relu(X.to(torch.bfloat16), C.tensors(state, torch.bfloat16), bn).float()
    else:
        a = ss_truth._ln_relu(X, sd, bn)
    a = (round_act or (lambda v: C.rne(v, F32)))(a)
    w = (round_w or (lambda v: C.rne(v, F32)))(sd[conv])
    if w_edit is not None:
        w = w_edit(w.clone())
    if pad_relu_beta:                                      # the window's out-of-image pixels hold relu(LN(0)) = relu(beta)
        p = w.shape[-1] // 2
        H, W = a.shape[-2:]
        fill = C.rne(torch.relu(sd[bn + ".bias"]), F32)[:, None, None].expand(48, H + 2 * p, W + 2 * p).clone()
        fill[:, p:p + H, p:p + W] = a
        out = torch.zeros(48, H, W)
        for dy in range(w.shape[-2]):
            for dx in range(w.shape[-1]):
                out += torch.einsum("oc,chw->ohw", w[:, :, dy, dx], fill[:, dy:dy + H, dx:dx + W])
    else:
        out = ss_truth._conv(a, w)
    if residual is not None:
        r = C._img(residual, F32)
        out = out + residual_mult * (C.rne(r, F32) if round_residual else r)
    return out


def _drop_half_step(w):
    w[:, 32:48, -1, -1] = 0.0                              # the last MFMA step's two live chunks: channels 32..47 of the last tap
    return w


TRUNK_MUTANTS = {
    "activations truncated": dict(round_act=C.truncate_bf16),
    "weights truncated": dict(round_w=C.truncate_bf16),
    "input image in bf16": dict(pre=lambda X: C.rne(X, F32)),
    "LayerNorm in bf16": dict(ln_bf16=True),
    "last half step dropped": dict(w_edit=_drop_half_step),
}
RESIDUAL_MUTANTS = {
    "residual image in bf16": dict(round_residual=True),
    "residual added twice": dict(residual_mult=2.0),
    "residual not added": dict(residual_mult=0.0),
}
MUTANT_CASE = "L=35"


def _fails(rep, share=0.5):
    assert rep.usable, rep.line()
    assert rep.over >= share and rep.ew_ratio > 1.0, f"the element-wise bar lets the mutant through: {rep.line()}"
    assert rep.l2_ratio > 1.0, f"the rel-L2 bar lets the mutant through: {rep.line()}"


@pytest.mark.parametrize("block", [0, 1])
@pytest.mark.parametrize("ks", [3, 5])
@pytest.mark.parametrize("name", list(TRUNK_MUTANTS))
def test_a_trunk_mutant_fails(name, ks, block):
    state, feat, im, _ = _standin(MUTANT_CASE)
    (bn, conv) = C.block_names(block)[0 if ks == 3 else 1]
    X, res = (im[f"X{block}"], None) if ks == 3 else (im[f"T{block + 1}"], im[f"X{block}"])
    got = _trunk_mutant(X, state, bn, conv, res, **TRUNK_MUTANTS[name])
    _fails(C.check_trunk(got, X, state, bn, conv, res, f"MUTANT {name}, block {block} {ks}x{ks}", assert_=False))


@pytest.mark.parametrize("block", [0, 1])
@pytest.mark.parametrize("name", list(RESIDUAL_MUTANTS))
def test_a_residual_mutant_fails(name, block):
    state, feat, im, _ = _standin(MUTANT_CASE)
    bn, conv = C.block_names(block)[1]
    X, res = im[f"T{block + 1}"], im[f"X{block}"]
    got = _trunk_mutant(X, state, bn, conv, res, **RESIDUAL_MUTANTS[name])
    _fails(C.check_trunk(got, X, state, bn, conv, res, f"MUTANT {name}, block {block}", assert_=False))


@pytest.mark.parametrize("ks", [3, 5])
def test_padding_with_relu_beta_fails_on_the_border(ks):
    """The large-beta state of test_zero_padding_of_the_normalised_input at L = 17.  The breach moves only the output pixels whose
    window leaves the image -- the outer ring, 1 pixel wide for the 3x3 (64 of 289 pixels, 22 %) and 2 for the 5x5 (120 of 289,
    42 %) -- so it cannot reach half of the stage's elements: it must put every element of the ring over the bar (relu(beta) is
    up to 10 and every output channel has weights on it) and no other, and exceed the rel-L2 bar."""
    state, feat, im, _ = _standin("large betas")
    bn, conv = C.block_names(0)[0 if ks == 3 else 1]
    X, res = (im["X0"], None) if ks == 3 else (im["T1"], im["X0"])
    got = _trunk_mutant(X, state, bn, conv, res, pad_relu_beta=True)
    c64, a64, z64 = C.trunk64(X, state, bn, conv, res)
    y32, a32 = C.trunk32(X, state, bn, conv, res)
    allow, delta, amb = C.flip_allowance(a64, z64, a32, state[conv])
    rep = C.measure(got, c64, y32, allow, f"MUTANT padding with relu(beta), {ks}x{ks}", delta, amb)
    L, p = 17, ks // 2
    ring = torch.ones(L, L, dtype=torch.bool)
    ring[p:L - p, p:L - p] = False
    share = float(ring.double().mean())
    assert abs(rep.over - share) < 1e-12, (rep.over, share)
    zero = allow == 0
    yard = float((y32.to(F64) - c64)[zero].abs().max())
    over = (got.to(F64) - c64).abs() > C.EW_MULT * max(yard, C.EW_FLOOR * float(c64.abs().max())) + allow
    assert bool(over[:, ring].all()) and not bool(over[:, ~ring].any())
    assert rep.usable and rep.l2_ratio > 1.0, rep.line()


def _stem_mutant(feat, state, *, round_w=None, round_bias=False, onehot_rows=False):
    sd = C.tensors(state, F32)
    if onehot_rows:
        feat = feat.clone()
        feat[4:8] = feat[0:4]                              # channels 4-7 from the row's code: the pixel (i, j) holds base i twice
    w = (round_w or (lambda v: C.rne(v, F32)))(sd["conv1.weight"])
    b = C.rne(sd["conv1.bias"], F32) if round_bias else sd["conv1.bias"]
    return ss_truth._conv(C.rne(feat, F32), w, b)


@pytest.mark.parametrize("name,knobs", [("weights truncated", dict(round_w=C.truncate_bf16)),
                                        ("bias in bf16", dict(round_bias=True)),
                                        ("one-hot channels 4-7 from the row's code", dict(onehot_rows=True))])
def test_a_stem_mutant_fails(name, knobs):
    state, feat, im, _ = _standin(MUTANT_CASE)
    _fails(C.check_stem(_stem_mutant(feat, state, **knobs), feat, state, f"MUTANT stem, {name}", assert_=False))


def test_the_stem_s_inputs_truncated_fail():
    state, feat, im, _ = _standin(MUTANT_CASE)
    sd = C.tensors(state, F32)
    got = ss_truth._conv(C.truncate_bf16(feat), C.rne(sd["conv1.weight"], F32), sd["conv1.bias"])
    _fails(C.check_stem(got, feat, state, "MUTANT stem, inputs truncated", assert_=False))


def test_the_output_pass_with_bf16_activations_fails():
    state, feat, im, _ = _standin(MUTANT_CASE)
    sd = C.tensors(state, F32)
    X = im[f"X{NB}"]
    a = C.rne(ss_truth._ln_relu(X, sd, "bn1"), F32)
    got = a.permute(1, 2, 0) @ sd["fc1.weight"][0] + sd["fc1.bias"][0]
    _fails(C.check_out(got, X, state, "MUTANT output pass, activations in bf16", assert_=False))


def test_the_output_pass_reads_the_residual_image():
    """What the GPU test's reading of the workspace rests on: out64 of the residual image reproduces the logits, out64 of the middle
    image does not."""
    state, feat, im, logits = _standin(MUTANT_CASE)
    assert C.check_out(logits, im[f"X{NB}"], state, "logits of X").passed
    assert not C.check_out(logits, im[f"T{NB}"], state, "logits of X against the middle image", assert_=False).passed
