"""The bf16 mode of the RNA-MSM-SS head (rnamsm_ss_head16, SSPredictor.gemm_dtype = "bf16") on the GPU.

The accuracy bar is the reference's own bf16 arithmetic: tb = the reference network under .bfloat16() on the CPU (weights,
activations, LayerNorm and sums all in bf16), t64 = ss_truth.logits in fp64; the bf16 head, which keeps fp32 accumulation, an fp32
residual image and fp32 LayerNorm, must be no further from t64 than tb is (ratio of the rel-L2 distances <= 1.0).  Element-wise it is
held to ss_truth.compare's own bars with tb's error in the place of the fp32 restatement's (rel-L2 multiple 1.0, max-abs within
ss_truth.EW_MULT x tb's on the same pixels).

tb is `logits_bf16` below and not ss_truth.logits(x, state, torch.bfloat16): that call runs the network in bf16 -- torch's CPU
conv2d and layer_norm take bfloat16 -- and then fails in its last line, `.numpy()` of a bfloat16 tensor.  logits_bf16 is the same
sequence of calls (F.conv2d, ss_truth._ln_relu, the fc1 product) on the same .bfloat16() tensors, widened to float before it leaves
torch; nothing is rounded that the network under .bfloat16() does not round."""
import functools
import os
import shutil
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT
from rnamsm import ops, ss, synthetic
import ss_truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")


def logits_bf16(x: np.ndarray, state: dict) -> np.ndarray:
    dt = torch.bfloat16
    sd = {k: torch.as_tensor(np.asarray(v)).to(dt) for k, v in state.items()}
    nb = sum(1 for k in sd if k.endswith(".conv2.weight"))
    conv = lambda v, w, b=None: F.conv2d(v[None], w, b, padding=w.shape[-1] // 2)[0]      # noqa: E731
    h = conv(torch.as_tensor(x).to(dt), sd["conv1.weight"], sd["conv1.bias"])
    for k in range(nb):
        p = f"layer1.{k}"
        t = conv(ss_truth._ln_relu(h, sd, p + ".bn1"), sd[p + ".conv1.weight"])
        h = conv(ss_truth._ln_relu(t, sd, p + ".bn2"), sd[p + ".conv2.weight"]) + h
    y = ss_truth._ln_relu(h, sd, "bn1").permute(1, 2, 0) @ sd["fc1.weight"][0] + sd["fc1.bias"][0]
    return y.float().numpy().astype(np.float64)


def _predictor(state, num_blocks, gemm_dtype="bf16"):
    m = ss.SSPredictor(num_blocks, gemm_dtype=gemm_dtype)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV)


def _case(L, seed):
    """Attention-like maps (rows on the simplex) and a sequence with one character outside A, C, G, U (test_gpu_ss_head.py)."""
    rng = np.random.RandomState(seed)
    atp = rng.exponential(size=(120, L, L)).astype(np.float32)
    atp /= atp.sum(-1, keepdims=True)
    seq = "".join(rng.choice(list("ACGU"), L))
    if L > 3:
        seq = seq[:2] + "N" + seq[3:]
    return atp, seq


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(float(np.linalg.norm(b)), 1e-30))


def _bar1(got, atp, seq, state, label, seams=False):
    """Bar 1 (rel-L2 ratio <= 1.0 against the reference's bf16 arithmetic) and the element-wise bars -> the ratio."""
    x = ss_truth.features(atp, seq)
    t64 = ss_truth.logits(x, state, torch.float64)
    tb = logits_bf16(x, state)
    assert np.isfinite(tb).all(), label
    got = np.asarray(got, dtype=np.float64)
    ratio = _rel(got, t64) / _rel(tb, t64)
    print(f"{label}: bf16 head rel-L2 {_rel(got, t64):.2e}, reference in bf16 {_rel(tb, t64):.2e}, ratio {ratio:.3f}")
    assert ratio <= 1.0, label
    ss_truth.compare(got, t64, tb, label, seams=seams, l2_mult=1.0)
    return ratio


def _logits(model, atp, seq):
    return model.logits(torch.from_numpy(atp).to(DEV), seq).cpu().numpy()


def _bits(a):
    return (a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).view(np.uint32)


# ---------------------------------------------------------------------- 1. the accuracy bar
@pytest.mark.parametrize("num_blocks", [1, 2, 4])
@pytest.mark.parametrize("L", [1, 2, 15, 16, 17, 33, 35])
def test_no_further_from_fp64_than_the_reference_in_bf16(L, num_blocks):
    state = ss_truth.make_state(num_blocks, seed=L)
    atp, seq = _case(L, 100 + L)
    _bar1(_logits(_predictor(state, num_blocks), atp, seq), atp, seq, state, f"L={L} blocks={num_blocks}")


@pytest.mark.parametrize("L,num_blocks", [(35, 16), (129, 2)])
def test_sixteen_blocks_and_several_tiles_per_side(L, num_blocks):
    """L = 129: 9 x 9 tiles with a one-pixel ragged edge in both directions."""
    state = ss_truth.make_state(num_blocks, seed=L)
    atp, seq = _case(L, 100 + L)
    _bar1(_logits(_predictor(state, num_blocks), atp, seq), atp, seq, state, f"L={L} blocks={num_blocks}")


# ---------------------------------------------------------------------- 2. the K tail
def _masked_state(state, keep):
    """Every conv weight ([out][in][kh][kw]) zeroed but for `keep`: "channels" = input channels 32..47, "tap" = the last tap,
    "none" = all zero."""
    out = dict(state)
    for k, w in state.items():
        if w.ndim == 4:
            m = np.zeros_like(w)
            if keep == "channels":
                m[:, 32:48] = w[:, 32:48]
            elif keep == "tap":
                m[:, :, -1, -1] = w[:, :, -1, -1]
            out[k] = m
    return out


@pytest.mark.parametrize("keep", ["channels", "tap"])
def test_the_half_step_tail_and_the_last_tap_are_summed(keep):
    """K is flat over (tap, channel): the last MFMA step of a trunk conv holds two chunks of 8 channels and two zero chunks, and
    they are channels 32..47 of the last tap.  With every other weight zero a dropped half step or a dropped tap gives the
    all-zero-weight logits."""
    L, nb = 17, 2
    state = ss_truth.make_state(nb, seed=17)
    atp, seq = _case(L, 117)
    st = _masked_state(state, keep)
    got = _logits(_predictor(st, nb), atp, seq)
    _bar1(got, atp, seq, st, f"K tail, {keep}")
    zero = _logits(_predictor(_masked_state(state, "none"), nb), atp, seq)
    assert np.isfinite(zero).all() and not np.array_equal(got, zero)
    assert _rel(got.astype(np.float64), zero.astype(np.float64)) > 1e-2, "the kept weights do not reach the logits"


# ---------------------------------------------------------------------- 3. element-wise at the seams
@pytest.mark.parametrize("L", [33, 35])
def test_element_wise_at_tile_seams(L):
    state = ss_truth.make_state(4, seed=40 + L)
    atp, seq = _case(L, 140 + L)
    _bar1(_logits(_predictor(state, 4), atp, seq), atp, seq, state, f"seams L={L}", seams=True)


# ---------------------------------------------------------------------- 4. zero padding of relu(LN(x))
def test_zero_padding_of_the_normalised_input():
    """Large LayerNorm betas: relu(LN(0)) = relu(beta) is far from 0, so padding the RAW input would move every border pixel."""
    state = ss_truth.make_state(4, seed=7, beta_scale=5.0)
    atp, seq = _case(17, 9)
    _bar1(_logits(_predictor(state, 4), atp, seq), atp, seq, state, "large betas L=17", seams=True)


# ---------------------------------------------------------------------- 5. non-finite inputs
@functools.lru_cache(maxsize=None)
def _nf():
    L, nb = 35, 2
    state = ss_truth.make_state(nb, seed=35)
    atp, seq = ss_truth.small_maps_case(L, 935)
    return L, nb, state, atp, seq, _predictor(state, nb)


@pytest.mark.parametrize("value", [NAN, INF, -INF], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("plane", [0, 119])
@pytest.mark.parametrize("pixel", [(8, 8), (15, 16), (0, 0), (34, 34)], ids=["centre", "seam", "corner00", "cornerLL"])
def test_a_non_finite_input_is_nan_where_the_truth_is(pixel, plane, value):
    L, nb, state, atp, seq, model = _nf()
    bad = ss_truth.poisoned(atp, plane, pixel, value)
    x = ss_truth.features(bad, seq)
    t64 = ss_truth.logits(x, state, torch.float64)
    tb = logits_bf16(x, state)
    a = torch.from_numpy(bad).to(DEV)
    logits, probs = model.logits(a, seq).cpu().numpy(), model.predict(a, seq).cpu().numpy()
    label = f"{value} at plane {plane}, pixel {pixel}"
    fin = ss_truth.check_nan_pattern(logits.astype(np.float64), t64, tb, label, min_finite=0.1, expect_nan=True)
    assert np.array_equal(np.isnan(probs), np.isnan(logits)), f"{label}: probs and logits are NaN at different pixels"
    assert not np.isinf(logits).any() and not np.isinf(probs).any(), f"{label}: an inf in the output"
    g, t, b = logits.astype(np.float64)[fin], t64[fin], tb[fin]
    assert _rel(g, t) <= _rel(b, t), label
    ss_truth.compare(g, t, b, label, l2_mult=1.0)


# ---------------------------------------------------------------------- 6. bits
PACK_LS = (1, 17, 35, 16)


@pytest.fixture(scope="module")
def head4():
    return _predictor(ss_truth.make_state(4, seed=21), 4)


@pytest.fixture(scope="module")
def pack_cases():
    cases = [_case(L, 300 + i) for i, L in enumerate(PACK_LS)]
    return [(torch.from_numpy(a).to(DEV), s) for a, s in cases]


def test_two_runs_give_the_same_bits(head4, pack_cases):
    a, seq = pack_cases[2]
    assert np.array_equal(_bits(head4.predict(a, seq)), _bits(head4.predict(a, seq)))
    assert np.array_equal(_bits(head4.logits(a, seq)), _bits(head4.logits(a, seq)))


@pytest.mark.parametrize("reverse", [False, True])
def test_every_member_of_a_packed_call_has_the_lone_call_s_bits(head4, pack_cases, reverse):
    cases = pack_cases[::-1] if reverse else pack_cases
    for many, lone in ((head4.logits_many, head4.logits), (head4.predict_many, head4.predict)):
        got = many([a for a, _ in cases], [s for _, s in cases])
        for (a, s), g in zip(cases, got):
            want = lone(a, s)
            assert torch.isfinite(want).all()
            assert np.array_equal(_bits(g), _bits(want)), f"L={a.shape[-1]} reverse={reverse}"


def test_a_strided_view_gives_the_contiguous_bits(head4, pack_cases):
    a, seq = pack_cases[2]
    L = a.shape[-1]
    wide = torch.full((120, L * L + 13), NAN, device=DEV)
    wide[:, :L * L] = a.reshape(120, -1)
    view = wide[:, :L * L].view(120, L, L)
    assert view.stride() == (L * L + 13, L, 1)
    assert np.array_equal(_bits(head4.predict(view, seq)), _bits(head4.predict(a, seq)))


def test_the_planes_are_built_once_per_pack_key(head4, pack_cases):
    a, seq = pack_cases[1]
    head4.predict(a, seq)
    first = head4._pack16
    head4.predict(a, seq)
    assert head4._pack16 is first
    planes = first[1][1]
    w = head4.layer1[0].conv2.weight.detach().permute(2, 3, 0, 1).contiguous()
    idx = 4 + 3                                            # block 0's conv2 in the table
    assert planes[idx].dtype == torch.bfloat16 and torch.equal(planes[idx], w.to(torch.bfloat16))      # round to nearest even


# ---------------------------------------------------------------------- 7. the default is untouched
def test_the_default_predictor_is_the_fp32_head(pack_cases):
    state = ss_truth.make_state(4, seed=21)
    model = _predictor(state, 4, gemm_dtype="f32")
    assert ss.SSPredictor(4).gemm_dtype == "f32"
    a, seq = pack_cases[2]
    codes = torch.from_numpy(ss.base_codes(seq)).to(DEV)
    ptrs, _ = model._packed_weights()
    for want, call in (("probs", model.predict), ("logits", model.logits)):
        direct = ops.ss_head(a, codes, ptrs, 4, want)
        assert np.array_equal(_bits(call(a, seq)), _bits(direct)), want
    # switching the property there and back returns to the same bits, and the two arithmetics do differ
    f32 = model.predict(a, seq)
    model.gemm_dtype = "bf16"
    b16 = model.predict(a, seq)
    model.gemm_dtype = "f32"
    assert np.array_equal(_bits(model.predict(a, seq)), _bits(f32)) and not np.array_equal(_bits(b16), _bits(f32))


# ---------------------------------------------------------------------- 8. the pipeline
SS_SEED, SS_BIAS_SHIFT = 162, -0.103                        # chosen on the CPU: see the test's docstring


def _pipeline_state():
    state = ss_truth.make_state(2, SS_SEED)
    state["fc1.bias"] = (state["fc1.bias"] + np.float32(SS_BIAS_SHIFT)).astype(np.float32)
    return state


def test_cli_in_bf16_writes_the_bf16_head_s_files(tmp_path, capsys, monkeypatch):
    """RNA_MSM_Inference with data.ss_model_path and data.ss_gemm_dtype=bf16 on two small alignments and a seeded 2-block state.
    (a) the three files are byte for byte write_ss_files on the host applied to the bf16 head's own probabilities;
    (b) `.ct` equals the f32 run's on every base whose row and column (upper triangle: the pixels the decoding reads) hold no
        pixel whose f32 probability lies within that structure's error bound of the 0.516 threshold.  The bound is the element-wise
        bar of test 3 -- ss_truth.EW_MULT x the max-abs distance of the reference in bf16 from fp64, in logits, on the maps the CLI
        wrote -- carried to probabilities by the sigmoid's slope (<= 1/4).  Under 1 % of the pixels may be excluded.
    The head's state was chosen on the CPU, on the oracle's maps of this alignment, so that the fp64 truth alone satisfies (b) with
    a structure in it.  A random state's logits have a spread of ~0.25 and the bound is ~0.07 in logits, so with the threshold inside
    the bulk hundreds of pixels lie within the bound, and with every pixel above it the multiplet-free step decides the pairs by
    comparing probabilities WITH EACH OTHER, which a margin to the threshold does not cover (seed 29 has no pixel near 0.516, 595
    above it, and the bf16 run pairs base 16 where the f32 run does not).  So the seeded state's fc1.bias is shifted to put the
    threshold in the upper tail: make_state(2, 162) with fc1.bias - 0.103 has 4 pixels above 0.516, the nearest 0.034 from it (bound
    0.019), 3 pairs, the same pairs from the reference in bf16 and from the bf16 contract restated in torch, and the same pairs in
    1000 draws of the logits perturbed by up to the whole bound on every pixel (seeds 0..199 searched)."""
    sys.path.insert(0, ROOT)
    import RNA_MSM_Inference as cli
    # rnamsm.ss.load_predictor builds the 16-block network by default: the CLI loads the 2-block file through it here
    real_load = ss.load_predictor
    monkeypatch.setattr(ss, "load_predictor", lambda path, device, num_blocks=2: real_load(path, device, num_blocks))
    mstate = synthetic.make_state_dict(seed=0)
    ckpt = tmp_path / "model.ckpt"
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in mstate.items()}}, ckpt)
    state = _pipeline_state()
    ss_pt = tmp_path / "rna-msm_attention.pt"
    torch.save({k: torch.from_numpy(v) for k, v in state.items()}, ss_pt)
    ids = ["2DRB_1", "2DRB_1b"]
    (tmp_path / "rna_id.txt").write_text("\n".join(ids) + "\n")
    outs = {}
    for mode in ("bf16", "f32"):
        res = tmp_path / mode
        res.mkdir()
        for n, i in enumerate(ids):
            shutil.copy(os.path.join(GOLDEN, "2DRB_1_first64.a2m_msa2"), res / f"{i}.a2m_msa2")
        cli.main([f"data.root_path={tmp_path}", f"data.MSA_path={mode}", f"data.model_path={ckpt}", "data.MSA_list=rna_id.txt",
                  "data.max_seqs_per_msa=32", "data.sample_method=first", f"data.ss_model_path={ss_pt}",
                  f"data.ss_gemm_dtype={mode}"])
        outs[mode] = res
        assert f"SS head arithmetic: {mode}" in capsys.readouterr().out
    import conftest
    toks = conftest.golden("tokens_2DRB_1_first64.npz")["tokens"]
    letters = {4: "A", 5: "G", 6: "C", 7: "U", 8: "X", 10: "-"}
    seq = "".join(letters[int(t)] for t in toks[0, 1:])
    model = _predictor(state, 2)
    f32_model = _predictor(state, 2, gemm_dtype="f32")
    for i in ids:
        atp = np.load(outs["bf16"] / f"{i}_atp.npy")
        assert np.array_equal(atp, np.load(outs["f32"] / f"{i}_atp.npy"))
        a = torch.from_numpy(atp).to(DEV)
        # (a)
        host = tmp_path / f"host_{i}"
        ss.write_ss_files(model.predict(a, seq).cpu().numpy(), seq, i, host)
        for ext in ("prob", "ct", "bpseq"):
            assert (host / "SS_result" / f"{i}.{ext}").read_bytes() == (outs["bf16"] / "SS_result" / f"{i}.{ext}").read_bytes(), ext
        # (b)
        x = ss_truth.features(atp, seq)
        bound = ss_truth.EW_MULT * float(np.abs(logits_bf16(x, state) - ss_truth.logits(x, state, torch.float64)).max()) / 4
        p32 = f32_model.predict(a, seq).cpu().numpy().astype(np.float64)
        L = len(seq)
        near = np.triu(np.abs(p32 - ss.THRESHOLD) <= bound, k=1)
        share = near.sum() / (L * (L - 1) / 2)
        print(f"{i}: bound {bound:.2e} in probability, {int(near.sum())} pixels within it of the threshold ({share:.2%})")
        assert share < 0.01
        ct = {m: (outs[m] / "SS_result" / f"{i}.ct").read_text().split("\n") for m in ("bf16", "f32")}
        assert ct["bf16"][:2] == ct["f32"][:2] and len(ct["bf16"]) == len(ct["f32"])
        touched = near.any(0) | near.any(1)                 # a base with such a pixel, and whoever it pairs with in either run
        for lines in ct.values():
            for b in np.nonzero(near.any(0) | near.any(1))[0]:
                partner = int(lines[2 + b].split("\t\t")[4])
                if partner:
                    touched[partner - 1] = True
        for b in range(L):
            if not touched[b]:
                assert ct["bf16"][2 + b] == ct["f32"][2 + b], (i, b)
        paired = [b for b in range(L) if not touched[b] and int(ct["f32"][2 + b].split("\t\t")[4])]
        assert len(paired) >= 4, f"{i}: the comparison needs a structure: {len(paired)} paired bases compared"
