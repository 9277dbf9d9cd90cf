"""Every writer of 16-bit planes held to the per-element contract of tests/planes_contract.py, and every 16-bit consumer run
on operands in the fp16-subnormal range.

The 16-bit modes hand every activation from kernel to kernel as planes hi = round16(x) (+ lo = round16(x - hi) in f16x3).  The
rest of the suite sees those conversions through aggregates (rel-L2 of hi + lo) and takes rnamsm_split_bf16's output as the
truth of the operand tests; here each conversion site is checked element by element against an independent conversion (torch
on the CPU).  "Both formats" = the two shipped modes: bf16 hi only (split 1, fmt 0) and the fp16 pair (split 3, fmt 1).

    writer                         check              against                           inputs
    rnamsm_split_bf16              check_exact        its own input                     720 896-pattern bit sweep + edge values, near-tie
                                                                                        data at 1 / 2^-12 / 2^-18 (bf16: 2^-120), tails of
                                                                                        n = 1..4099 inside guard-filled buffers
    rnamsm_gemm16_residual_stats   check_exact        the fp32 x it writes itself       M 2048 / 2300; GEMM outputs, and a zero update that
                                                                                        leaves near-tie x (1 and 2^-12) to be split
    rnamsm_softmax_rows_planes     check_exact        probs * 4096 (exact on the host)  C 1..1024, H 1 / 12, key mask, 60-nat spread
    rnamsm_layernorm_split         check_near + shape rnamsm_layernorm                  D 128..1024, T 1..4097, offset row, tiny gamma
    rnamsm_gemm_bf16 (O planes)    check_near + shape the same call with Cout           gemm16_dma 0 / 1 / 3 / 4, M 300 / 2047 / 2049,
                                                                                        16x16x32 kernel (N 1280), none / GELU / column scale,
                                                                                        one-hot W (near-tie outputs)
    rnamsm_row_apply               check_near + shape its fp32 ctx                      R 1 / 7 / 65, C 40 (row_narrow 0 / 1) / 130,
                                                                                        softmax P and one-hot P (near-tie outputs)
    rnamsm_col_attn_fused          check_near + shape its fp32 ctx (R = 1: check_exact  col_small 0 / 1 at R 3 / 16, col_dma 0 / 1 at
                                                      against v)                        R 40 / 300, random and one-hot attention
    rnamsm_row_apply16             check_near + shape its fp32 ctx                      C 130 / 300 / 400, both formats
    rnamsm_col_attn16              check_near + shape its fp32 ctx                      the shapes of test_gpu_attn16's plane test
    rnamsm_gemm16_lnfold           check_pair_shape   -- (no fp32 twin exists)          + the rel-L2 bars of its existing test

rnamsm_gemm_bf16 refuses plane output with an fp32 A (the plane epilogue exists for plane input only), so the "fp32 A staged"
family has no plane writer: the refusal itself is asserted.

Wall time of the whole module on an MI355X host: 16 s (135 cases; 2026-10-16), against 21.2 s (103 cases) for
tests/test_gpu_attn16.py in the same session: no shape list was trimmed.
Its first run found two writers whose fp32 "twin" was another arithmetic, not another compilation (8 failing cases, no
conversion at fault); both are twins by construction since: rnamsm_layernorm and rnamsm_layernorm_split share one row routine,
and the one-wave column kernel writes planes itself (tests/analysis/README.md, Findings).
"""
import numpy as np
import pytest
import torch

import planes_contract as pc
from conftest import rel_l2
from oracle import msm_oracle as O
from rnamsm import synthetic

pytestmark = pytest.mark.gpu

FORMATS = [(1, 0), (3, 1)]          # (split, fmt) of the two shipped modes
# (split, fmt, bar vs the fp64 product of the plane values): tests/test_gpu_attn16.py MODES, tests/test_gpu_kernels.py
CONSUMER_MODES = [(1, 0, 2e-6), (3, 1, 3e-6)]
SMALL = [2.0 ** -12, 2.0 ** -18]
HT = pc.DTYPE


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rnamsm import _lib
    _lib.load()
    return torch.device("cuda:0")


def _ok(rep, what=""):
    assert rep.count == 0, f"{what}\n{rep}"


def _rand(name, shape, scale=1.0):
    return torch.from_numpy((scale * synthetic.normal(name, 31, shape)).astype(np.float32))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _eff(pl, fmt):
    """fp64 values a (hi, lo | None) pair of int16 planes holds, on the host."""
    v = pl[0].cpu().view(HT[fmt]).double()
    return v if pl[1] is None else v + pl[1].cpu().view(HT[fmt]).double()


def _host_planes(x, split, fmt, dev):
    """Planes made by the host reference (NOT by rnamsm_split_bf16): (device int16 pair, fp64 values they hold)."""
    hi, lo = pc.split_reference(x.contiguous(), fmt)
    pl = (hi.view(torch.int16).to(dev), lo.view(torch.int16).to(dev) if split == 3 else None)
    return pl, hi.double() + (lo.double() if split == 3 else 0)


def _views(pl, a, b):
    return (pl[0][:, a:b], None if pl[1] is None else pl[1][:, a:b])


def _near_and_shape(pl, x32, fmt, what):
    _ok(pc.check_near(pl[0], pl[1], x32, fmt), what)
    if pl[1] is not None:
        _ok(pc.check_pair_shape(pl[0], pl[1], fmt), what)


# ======================================================================================== rnamsm_split_bf16
@pytest.mark.parametrize("want_lo", [False, True])
@pytest.mark.parametrize("fmt", [0, 1])
def test_split_equals_the_independent_conversion_on_every_bit_pattern(dev, fmt, want_lo):
    """The producer of every operand the 16-bit kernel tests use, against torch's CPU conversion, bit for bit: all exponents,
    both tie positions, subnormal results, the fp16 overflow edge, signed zeros, inf and NaN.  (A bf16 lo plane is still
    written on request, though no shipped mode reads one.)"""
    from rnamsm import ops
    x = torch.cat([pc.bit_sweep(), pc.edge_values()])
    hi, lo = ops.split_bf16(x.to(dev), want_lo=want_lo, fmt=fmt)
    _ok(pc.check_exact(hi, lo, x, fmt), "bit sweep")
    scales = (1.0, 2.0 ** -12, 2.0 ** -18) + ((2.0 ** -120,) if fmt == 0 else ())
    for s in scales:
        x = pc.near_tie(f"split.{fmt}", (300001,), fmt, s)
        hi, lo = ops.split_bf16(x.to(dev), want_lo=want_lo, fmt=fmt)
        _ok(pc.check_exact(hi, lo, x, fmt), f"near-tie data at scale {s}")


@pytest.mark.parametrize("want_lo", [False, True])
@pytest.mark.parametrize("fmt", [0, 1])
def test_split_writes_exactly_n_elements(dev, fmt, want_lo):
    """n around the 8-element and 256-thread edges, on slices in the middle of guard-filled buffers: elements [0, n) are the
    conversion, everything before and after keeps the guard, in both planes."""
    from rnamsm import _lib
    lib = _lib.load()
    GUARD, OFF, PAD = 0x5A5A, 37, 301
    for n in (1, 3, 7, 8, 9, 255, 257, 4099):
        x = pc.near_tie(f"tail.{n}", (n + 2 * OFF,), fmt)
        xd = x.to(dev)
        hi = torch.full((n + OFF + PAD,), GUARD, dtype=torch.int16, device=dev)
        lo = torch.full((n + OFF + PAD,), GUARD, dtype=torch.int16, device=dev)
        _lib.check(lib.rnamsm_split_bf16(xd.data_ptr() + 4 * OFF, hi.data_ptr() + 2 * OFF,
                                         lo.data_ptr() + 2 * OFF if want_lo else None, n, fmt, _stream()))
        torch.cuda.synchronize()
        _ok(pc.check_exact(hi[OFF:OFF + n], lo[OFF:OFF + n] if want_lo else None, x[OFF:OFF + n], fmt), f"n = {n}")
        for plane, written in ((hi, True), (lo, want_lo)):
            p = plane.cpu()
            assert bool((p[:OFF] == GUARD).all()) and bool((p[OFF + n:] == GUARD).all()), (n, "guard overwritten")
            assert written or bool((p == GUARD).all())


# ======================================================================================== rnamsm_gemm16_residual_stats
@pytest.mark.parametrize("split,fmt", FORMATS)
@pytest.mark.parametrize("M", [2048, 2300])
def test_residual_gemm_planes_are_the_split_of_the_x_it_stores(dev, M, split, fmt):
    """x += A W^T + b writes the new fp32 x AND its planes in one launch: the planes must be the exact split of the stored x.
    M = 2300 ends in a ragged 256-row panel.  Second and third pass: A = 0, so x stays the near-tie data it was (at 1 and at
    2^-12, where the fp16 lo plane is subnormal) and every eighth element is a rounding decision."""
    from rnamsm import ops
    N, K = 768, 128
    lo = split == 3
    w = ops.split_bf16(_rand("rs.w", (N, K), 0.05).to(dev), want_lo=lo, fmt=fmt)
    b = _rand("rs.b", (N,), 0.1).to(dev)
    a = ops.split_bf16(pc.near_tie("rs.a", (M, K), fmt).to(dev), want_lo=lo, fmt=fmt)
    x = pc.near_tie("rs.x", (M, N), fmt).to(dev)
    xpl, _ = ops.linear_planes_residual_stats(a, w, b, x, fmt=fmt)
    _ok(pc.check_exact(xpl[0], xpl[1], x, fmt), "GEMM outputs")
    zero = (torch.zeros(M, K, dtype=torch.int16, device=dev), torch.zeros(M, K, dtype=torch.int16, device=dev) if lo else None)
    for s in (1.0, 2.0 ** -12):
        x0 = pc.near_tie("rs.x0", (M, N), fmt, s)
        x = x0.to(dev)
        xpl, _ = ops.linear_planes_residual_stats(zero, w, None, x, fmt=fmt)
        assert torch.equal(x.cpu(), x0)                                           # x + 0 stored back unchanged
        _ok(pc.check_exact(xpl[0], xpl[1], x0, fmt), f"near-tie x at scale {s}")


# ======================================================================================== rnamsm_softmax_rows_planes
@pytest.mark.parametrize("split,fmt", FORMATS)
@pytest.mark.parametrize("H", [1, 12])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 257, 1024])
def test_softmax_planes_are_the_split_of_the_probabilities_it_stores(dev, C, H, split, fmt):
    """probs and the planes of probs * plane_scale come out of one launch; plane_scale = 4096 is a power of two, so
    x = probs * 4096 is exact on the host.  With and without a key mask (masked keys: probability exactly 0, planes +0), the
    columns [C, ldp) all zero, and logits spread over ~60 nats, where most of P * 4096 lies in fp16 subnormals."""
    from rnamsm import ops
    PS = 4096.0
    ldp = (C + 63) // 64 * 64
    nsplit = 1 if C == 1024 else 2
    mask = (torch.arange(C) % 3 == 1).to(torch.uint8)
    for spread, use_mask in ((2.0, False), (2.0, True), (15.0, False)):      # sigma 15: +-2 sigma of the summed logits span 60 nats
        partial = _rand(f"sm.{C}.{H}.{spread}", (nsplit, H, C, C), spread / np.sqrt(nsplit)).to(dev)
        probs, pp = ops.softmax_rows_planes(partial, split=split, fmt=fmt, key_mask=mask.to(dev) if use_mask else None, plane_scale=PS)
        p = probs.cpu()
        assert bool(torch.isfinite(p).all())
        x = p * PS
        hi = pp[0].view(H, C, ldp)
        lo = None if pp[1] is None else pp[1].view(H, C, ldp)
        _ok(pc.check_exact(hi[:, :, :C], None if lo is None else lo[:, :, :C], x, fmt), f"spread {spread}, mask {use_mask}")
        assert int(hi[:, :, C:].abs().max() if ldp > C else 0) == 0 and (lo is None or int(lo[:, :, C:].abs().max() if ldp > C else 0) == 0)
        if use_mask and C > 1:
            m = mask.bool()
            assert float(p[:, :, m].abs().max()) == 0.0 and not bool(torch.signbit(p[:, :, m]).any())
            assert int(hi[:, :, :C][:, :, m.to(dev)].abs().max()) == 0 and (lo is None or int(lo[:, :, :C][:, :, m.to(dev)].abs().max()) == 0)
            want = torch.softmax(partial.sum(0).double().cpu().masked_fill(m[None, None, :], -10000.0), -1)
            assert float((p.double() - want).abs().max()) < 2e-6
        if spread > 10 and fmt == 1 and C >= 63:
            assert float(((x > 0) & (x < 2.0 ** -14)).float().mean()) > 0.5       # the regime the case is there for


# ======================================================================================== rnamsm_layernorm_split
@pytest.mark.parametrize("split,fmt", FORMATS)
@pytest.mark.parametrize("T", [1, 33, 4097])
@pytest.mark.parametrize("D", [128, 768, 1024])
def test_layernorm_planes_against_the_fp32_layernorm(dev, D, T, split, fmt):
    """rnamsm_layernorm_split against its fp32 twin rnamsm_layernorm (the same arithmetic in another kernel): near-tie rows,
    one row riding on a large common offset, and gamma / beta so small that the fp16 planes are subnormal.
    beta = 0.1 * normal cancels part of the product where |y| is small, so a last-bit difference in rstd between the two
    kernels would show as several fp32 ulps of the result: the first run of this test found exactly that (the two kernels'
    variance sums were contracted differently: 24-647 fp16-pair elements per case beyond the pair bar, up to 3.7 x); both now
    call ln_row_stats / ln_value of csrc/common.h."""
    from rnamsm import ops
    x = pc.near_tie(f"ln.{D}.{T}", (T, D), fmt)
    x[T // 2] += 1000.0
    xd = x.to(dev)
    for gs in (1.0,) + tuple(SMALL):
        g = ((1 + 0.1 * _rand("ln.g", (D,))) * gs).to(dev)
        b = (0.1 * gs * _rand("ln.b", (D,))).to(dev)
        y = ops.layernorm(xd, g, b)
        pl = ops.layernorm_split(xd, g, b, split=split, fmt=fmt)
        _near_and_shape(pl, y, fmt, f"gamma scale {gs}")


# ======================================================================================== rnamsm_gemm_bf16, plane epilogue
def _one_hot_w(N, K):
    w = torch.zeros(N, K)
    w[torch.arange(N), (torch.arange(N) * 7 + 3) % K] = 1.0
    return w


# (gemm16_dma, M, N): 0 = register-staged 128x128, 1 = LDS-DMA 128x128, 3 / 4 below 2048 rows = the same, from 2048 rows the
# 256x256 software-pipelined kernel (4: 32-deep K tiles for bf16 too); plain bf16 with N > 1024 = the 16x16x32-MFMA kernel
GEMM_CASES = [(0, 300, 256), (1, 300, 256), (3, 2047, 256), (3, 2049, 256), (3, 2300, 1280), (4, 2049, 256)]


@pytest.mark.parametrize("split,fmt", FORMATS)
@pytest.mark.parametrize("dma,M,N", GEMM_CASES)
def test_gemm_plane_epilogue_against_its_fp32_output(dev, dma, M, N, split, fmt):
    """O_hi / O_lo of rnamsm_gemm_bf16 against the same call writing fp32 Cout, in every kernel family that has a plane
    epilogue, with each epilogue: none, GELU, and a column scale whose edge (96) cuts a 64-column store slab.  A one-hot W with
    zero bias copies A's values (hi + lo, sums of two halves: near the 16-bit grid's ties) to the output."""
    from rnamsm import ops, _lib
    from rnamsm._lib import ACT_GELU_ERF
    lib = _lib.load()
    K = 192
    lo = split == 3
    default = lib.rnamsm_get_param(b"gemm16_dma")
    try:
        _lib.check(lib.rnamsm_set_param(b"gemm16_dma", dma))
        a = ops.split_bf16(pc.near_tie(f"g.a.{M}", (M, K), fmt).to(dev), want_lo=lo, fmt=fmt)
        w = ops.split_bf16((0.05 * pc.near_tie(f"g.w.{N}", (N, K), fmt)).to(dev), want_lo=lo, fmt=fmt)
        b = _rand("g.b", (N,), 0.1).to(dev)
        for what, kw in (("none", {}), ("colscale", dict(scale=0.125, scale_cols=96))):
            y = ops.linear_planes(a, w, b, fmt=fmt, **kw)
            pl = ops.linear_planes(a, w, b, out_planes=True, fmt=fmt, **kw)
            _near_and_shape(pl, y, fmt, f"{what}, dma {dma}")
        # GELU has no fp32 twin instance (include/rnamsm.h: plane input with fp32 output supports act none only).  Its planes
        # get the x-free check, and check_near's two bars against the fp64 erf-GELU of the fp32 pre-activation z with the twin's
        # slack widened by what GELU in fp32 may cost -- derived: 1 + erf carries a few ulps of 1 (2^-21 absolute), times
        # |z| / 2, plus two product roundings of 2^-24 |z| each: 2^-21 |z| in all; and z itself is the twin's, one fp32 ulp off
        # at most, which GELU passes on with |gelu'| <= 1.13.
        z = ops.linear_planes(a, w, b, fmt=fmt).cpu().reshape(-1)
        pl = ops.linear_planes(a, w, b, act=ACT_GELU_ERF, out_planes=True, fmt=fmt)
        if pl[1] is not None:
            _ok(pc.check_pair_shape(pl[0], pl[1], fmt), "gelu")
        want = O.gelu_erf(z.double())
        slack = 2.0 ** -21 * z.double().abs() + 1.13 * pc.ulp32(z)
        hv = pc.values(pl[0], fmt)
        assert bool(torch.isfinite(hv).all())
        worst = ((hv - want).abs() / (pc.ulp16(hv, fmt) / 2 + slack)).max()
        assert float(worst) <= 1.0, ("gelu hi", float(worst))
        if lo:
            err = (hv + pc.values(pl[1], fmt) - want).abs()
            worst = (err / (torch.clamp(want.abs() * 2.0 ** -22, min=2.0 ** -25) + slack)).max()
            assert float(worst) <= 1.0, ("gelu pair", float(worst))
        # near-tie OUTPUTS: one-hot W, no bias -> output = A's value, exactly
        w1 = _one_hot_w(N, K)
        wp = ops.split_bf16(w1.to(dev), want_lo=lo, fmt=fmt)
        y = ops.linear_planes(a, wp, None, fmt=fmt)
        assert torch.equal(y.cpu().double(), _eff(a, fmt) @ w1.double().t())
        pl = ops.linear_planes(a, wp, None, out_planes=True, fmt=fmt)
        _ok(pc.check_exact(pl[0], pl[1], y, fmt), f"one-hot W, dma {dma}")          # y IS the value that was split
    finally:
        _lib.check(lib.rnamsm_set_param(b"gemm16_dma", default))


def test_gemm_refuses_plane_output_from_an_fp32_a(dev):
    """The fp32-A-staged kernels have no plane epilogue: asking for one is an error, never another path taken silently."""
    from rnamsm import ops, _lib
    lib = _lib.load()
    M, N, K = 300, 128, 64
    a = _rand("rf.a", (M, K)).to(dev)
    w = ops.split_bf16(_rand("rf.w", (N, K)).to(dev), fmt=1)
    oh = torch.empty(M, N, dtype=torch.int16, device=dev)
    ol = torch.empty(M, N, dtype=torch.int16, device=dev)
    with pytest.raises(_lib.RnamsmError):
        _lib.check(lib.rnamsm_gemm_bf16(a.data_ptr(), K, w[0].data_ptr(), w[1].data_ptr(), None, None, 0, None, N, M, N, K, 0, 1.0,
                                        0, 3, 1, None, None, oh.data_ptr(), ol.data_ptr(), _stream()))


# ======================================================================================== rnamsm_row_apply (exact kernel)
def _row_apply(probs, v, R, C, H, fmt=None, want_lo=False):
    """rnamsm_row_apply: fp32 ctx (fmt None) or (hi, lo | None) planes."""
    from rnamsm import _lib
    D = 64 * H
    ctx = hi = lo = None
    if fmt is None:
        ctx = torch.empty(R * C, D, device=v.device, dtype=torch.float32)
    else:
        hi = torch.empty(R * C, D, device=v.device, dtype=torch.int16)
        lo = torch.empty(R * C, D, device=v.device, dtype=torch.int16) if want_lo else None
    p = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.load().rnamsm_row_apply(probs.data_ptr(), v.data_ptr(), v.stride(0), p(ctx), D, R, C, H, 64, p(hi), p(lo),
                                            fmt or 0, 0, _stream()))
    return ctx if fmt is None else (hi, lo)


def _one_hot_probs(H, C):
    p = torch.zeros(H, C, C)
    for h in range(H):
        p[h, torch.arange(C), (torch.arange(C) * 7 + 3 + h) % C] = 1.0
    return p


@pytest.mark.parametrize("split,fmt", FORMATS)
@pytest.mark.parametrize("C,narrow", [(40, 1), (40, 0), (130, 1)])
@pytest.mark.parametrize("R", [1, 7, 65])
def test_row_apply_planes_against_its_fp32_context(dev, R, C, narrow, split, fmt):
    """ctx_hi / ctx_lo of the exact row-attention update against its fp32 ctx.  The planes always come from the tile kernel;
    at C <= 64 the fp32 twin is the narrow kernel ("row_narrow" 1, bit-identical by its own test) or the tile kernel (0).
    One-hot probabilities copy near-tie v rows to the output: there the fp32 ctx is v itself and the check is exact."""
    from rnamsm import _lib
    lib = _lib.load()
    H = 2
    D = 64 * H
    v = pc.near_tie(f"ra.v.{R}.{C}", (R * C, D), fmt).to(dev)
    try:
        _lib.check(lib.rnamsm_set_param(b"row_narrow", narrow))
        probs = torch.softmax(_rand(f"ra.p.{C}", (H, C, C), 2.0), -1).contiguous().to(dev)
        ctx = _row_apply(probs, v, R, C, H)
        pl = _row_apply(probs, v, R, C, H, fmt=fmt, want_lo=split == 3)
        _near_and_shape(pl, ctx, fmt, "softmax P")
        p1 = _one_hot_probs(H, C)
        ctx = _row_apply(p1.to(dev), v, R, C, H)
        want = torch.einsum("hij,rjhd->rihd", p1.double(), v.cpu().double().view(R, C, H, 64)).reshape(R * C, D)
        assert torch.equal(ctx.cpu().double(), want)
        pl = _row_apply(p1.to(dev), v, R, C, H, fmt=fmt, want_lo=split == 3)
        _ok(pc.check_exact(pl[0], pl[1], ctx, fmt), "one-hot P")
    finally:
        _lib.check(lib.rnamsm_set_param(b"row_narrow", 1))


# ======================================================================================== rnamsm_col_attn_fused (exact kernel)
def _col_attn(q, k, v, R, C, H, fmt=None, want_lo=False):
    from rnamsm import _lib
    D = 64 * H
    ctx = hi = lo = None
    if fmt is None:
        ctx = torch.empty(R * C, D, device=v.device, dtype=torch.float32)
    else:
        hi = torch.empty(R * C, D, device=v.device, dtype=torch.int16)
        lo = torch.empty(R * C, D, device=v.device, dtype=torch.int16) if want_lo else None
    p = lambda t: None if t is None else t.data_ptr()
    assert q.stride(0) == k.stride(0) == v.stride(0)
    _lib.check(_lib.load().rnamsm_col_attn_fused(q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), p(ctx), D, R, C, H, 64, None,
                                                 p(hi), p(lo), fmt or 0, 0, _stream()))
    return ctx if fmt is None else (hi, lo)


def _one_hot_qk(R, C, H):
    """q, k [R, C, H, 64] under which query i < 128 attends exactly one key, perm[i]: q_i = +-e_(i % 64), the key carries +-80 on
    that axis (every other score is 0 or -80: below 2^-100 of the sum); queries from 128 on are zero (uniform attention)."""
    q = torch.zeros(R, C, H, 64)
    k = torch.zeros(R, C, H, 64)
    perm = (np.arange(R) * 37 + 11) % R if R % 37 else (np.arange(R) + 1) % R
    for i in range(min(R, 128)):
        s = 1.0 if i < 64 else -1.0
        q[i, :, :, i % 64] = s
        k[int(perm[i]), :, :, i % 64] += 80.0 * s
    return q, k, perm


@pytest.mark.parametrize("split,fmt", FORMATS)
@pytest.mark.parametrize("R,knob,value", [(3, "col_small", 0), (3, "col_small", 1), (16, "col_small", 0), (16, "col_small", 1),
                                          (40, "col_dma", 0), (40, "col_dma", 1), (300, "col_dma", 0), (300, "col_dma", 1)])
def test_col_attention_planes_against_its_fp32_context(dev, R, knob, value, split, fmt):
    """ctx_hi / ctx_lo of the exact column attention against its fp32 ctx, under both staging variants and -- for shallow
    alignments -- on both kernels: with "col_small" = 1 planes and fp32 ctx both come from the one-wave 16x16x4-MFMA kernel, with
    0 both from the 128-query-block kernel.  (The first run of this test found the planes of R <= 16 always written by the
    block kernel while the fp32 ctx came from the one-wave kernel, which sums in another order: up to 14.8 x the pair bar.)
    One-hot attention copies near-tie v rows to the output, where every kernel must agree exactly."""
    from rnamsm import _lib
    lib = _lib.load()
    C, H = 5, 2
    D = 64 * H
    default = lib.rnamsm_get_param(knob.encode())
    qkv = pc.near_tie(f"ca.{R}", (R * C, 3 * D), fmt)
    qkv[:, :D] *= 0.125
    try:
        _lib.check(lib.rnamsm_set_param(knob.encode(), value))
        t = qkv.to(dev)
        args = (t[:, :D], t[:, D:2 * D], t[:, 2 * D:], R, C, H)
        ctx = _col_attn(*args)
        pl = _col_attn(*args, fmt=fmt, want_lo=split == 3)
        random_near = pc.check_near(pl[0], pl[1], ctx, fmt)
        q1, k1, perm = _one_hot_qk(R, C, H)
        t = torch.cat([q1.view(R * C, D), k1.view(R * C, D), qkv[:, 2 * D:]], 1).contiguous().to(dev)
        args = (t[:, :D], t[:, D:2 * D], t[:, 2 * D:], R, C, H)
        ctx = _col_attn(*args)
        n1 = min(R, 128)
        v = qkv[:, 2 * D:].view(R, C, D)
        assert torch.equal(ctx.cpu().view(R, C, D)[:n1], v[torch.from_numpy(perm[:n1].astype(np.int64))])
        pl = _col_attn(*args, fmt=fmt, want_lo=split == 3)
        _near_and_shape(pl, ctx, fmt, "one-hot attention")
        first = lambda p: None if p is None else p.view(R, C, D)[:n1]
        _ok(pc.check_exact(first(pl[0]), first(pl[1]), ctx.view(R, C, D)[:n1], fmt), "one-hot attention, copied rows")
        _ok(random_near, "random attention")
        if pl[1] is not None:
            _ok(pc.check_pair_shape(pl[0], pl[1], fmt), "random attention")
    finally:
        _lib.check(lib.rnamsm_set_param(knob.encode(), default))


@pytest.mark.parametrize("split,fmt", FORMATS)
def test_col_attention_planes_of_a_single_row_are_the_split_of_v(dev, split, fmt):
    """R = 1: softmax over one key is 1 and ctx = v (modules.py:882-894), a pure conversion of v: exact, in every regime."""
    C, H = 70, 2
    D = 64 * H
    for s in (1.0,) + tuple(SMALL):
        qkv = pc.near_tie(f"ca1.{s}", (C, 3 * D), fmt)
        qkv[:, 2 * D:] *= s
        t = qkv.to(dev)
        args = (t[:, :D], t[:, D:2 * D], t[:, 2 * D:], 1, C, H)
        assert torch.equal(_col_attn(*args).cpu(), qkv[:, 2 * D:])
        pl = _col_attn(*args, fmt=fmt, want_lo=split == 3)
        _ok(pc.check_exact(pl[0], pl[1], qkv[:, 2 * D:], fmt), f"v at scale {s}")


# ======================================================================================== rnamsm_row_apply16
def _row_apply16(p, v, R, C, H, fmt, out_scale, planes):
    from rnamsm import _lib
    D = 64 * H
    ctx = hi = lo = None
    if planes:
        hi = torch.empty(R * C, D, device=v[0].device, dtype=torch.int16)
        lo = torch.empty(R * C, D, device=v[0].device, dtype=torch.int16) if p[1] is not None else None
    else:
        ctx = torch.empty(R * C, D, device=v[0].device, dtype=torch.float32)
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.load().rnamsm_row_apply16(ptr(p[0]), ptr(p[1]), p[0].stride(0), ptr(v[0]), ptr(v[1]), v[0].stride(0), ptr(ctx), D,
                                              R, C, H, 64, out_scale, ptr(hi), ptr(lo), fmt, _stream()))
    return (hi, lo) if planes else ctx


@pytest.mark.parametrize("split,fmt", FORMATS)
@pytest.mark.parametrize("R,C", [(5, 130), (5, 300), (3, 400), (5, 400)])
def test_row_apply16_planes_against_its_fp32_context(dev, R, C, split, fmt):
    """ctx planes of the 16-bit row-attention update against its fp32 ctx: the 128x128-tile kernel (C < 256, or R < 4) and the
    256x256-tile kernel, C on both sides of 384; P planes hold P * 4096 and out_scale undoes it, as in the forward."""
    from rnamsm import ops
    H = 2
    D = 64 * H
    PS = 4096.0
    ldp = (C + 63) // 64 * 64
    P = torch.zeros(H * C, ldp)
    P[:, :C] = torch.softmax(_rand(f"r16.p.{C}", (H, C, C), 2.0), -1).view(H * C, C) * PS
    pp = ops.split_bf16(P.to(dev), want_lo=split == 3, fmt=fmt)
    v = ops.split_bf16(pc.near_tie(f"r16.v.{R}.{C}", (R * C, D), fmt).to(dev), want_lo=split == 3, fmt=fmt)
    ctx = _row_apply16(pp, v, R, C, H, fmt, 1.0 / PS, planes=False)
    pl = _row_apply16(pp, v, R, C, H, fmt, 1.0 / PS, planes=True)
    _near_and_shape(pl, ctx, fmt, "softmax P")
    # one-hot P (times 4096, exact in both formats): the output is v's plane value, a near-tie number in the pair mode
    P1 = torch.zeros(H * C, ldp)
    P1[:, :C] = _one_hot_probs(H, C).view(H * C, C) * PS
    pp = ops.split_bf16(P1.to(dev), want_lo=split == 3, fmt=fmt)
    ctx = _row_apply16(pp, v, R, C, H, fmt, 1.0 / PS, planes=False)
    want = torch.einsum("hij,rjhd->rihd", _one_hot_probs(H, C).double(), _eff(v, fmt).view(R, C, H, 64)).reshape(R * C, D)
    assert torch.equal(ctx.cpu().double(), want)
    pl = _row_apply16(pp, v, R, C, H, fmt, 1.0 / PS, planes=True)
    _ok(pc.check_exact(pl[0], pl[1], ctx, fmt), "one-hot P")


# ======================================================================================== rnamsm_col_attn16
@pytest.mark.parametrize("split,fmt", FORMATS)
@pytest.mark.parametrize("R,C,H", [(7, 33, 2), (130, 5, 2), (300, 4, 1), (256, 3, 2)])
def test_col_attn16_planes_against_its_fp32_context(dev, R, C, H, split, fmt):
    """test_col_attention_16bit_plane_outputs_equal_the_rounded_fp32_output of tests/test_gpu_attn16.py (kept there as it is) on
    the shared checkers and on near-tie operands.  The bars here are tighter than that test's: hi within half a 16-bit ulp plus
    one fp32 ulp (there: 2^-11 |x| (1 + 1e-3) + 1e-7), the fp16 pair within 2^-22 |x| or 2^-25 plus one fp32 ulp (there:
    2^-21 |x| + 2e-7)."""
    from rnamsm import ops
    D = 64 * H
    pl_in = ops.split_bf16(pc.near_tie(f"c16.{R}.{C}", (R * C, 3 * D), fmt).to(dev), want_lo=split == 3, fmt=fmt)
    args = (_views(pl_in, 0, D), _views(pl_in, D, 2 * D), _views(pl_in, 2 * D, 3 * D), R, C, H)
    f32 = ops.col_attn16(*args, fmt=fmt, scale=0.125)
    pl = ops.col_attn16(*args, fmt=fmt, scale=0.125, out_planes=True)
    assert (pl[1] is not None) == (split == 3)
    _near_and_shape(pl, f32, fmt, "random attention")


# ======================================================================================== rnamsm_gemm16_lnfold
@pytest.mark.parametrize("split,fmt", FORMATS)
@pytest.mark.parametrize("xscale", [1.0, 2.0 ** -12])
def test_lnfold_gemm_planes_have_the_shape_of_a_split(dev, xscale, split, fmt):
    """rnamsm_gemm16_lnfold writes planes only and has NO fp32 twin, so its conversion site gets the WEAKEST check of the ten:
    check_pair_shape (|lo| <= ulp16(hi) / 2 -- necessary, blind to a hi that took the wrong neighbour at a near-tie) and the
    rel-L2 bars of test_layernorm_folded_into_the_16bit_gemms (6e-3 bf16, 4e-5 bf16 pairs, 3e-6 fp16 pairs, unchanged) against
    fp64 on the plane values, here on near-tie x and on x in the 2^-12 regime (fp16 lo plane subnormal).  Its epilogue is the
    shared slab store of the plane GEMMs, whose other instances the check_near tests above hold to the full contract."""
    from rnamsm import ops
    from rnamsm._lib import ACT_GELU_ERF
    M, D, F = 2304, 768, 1024
    lo = split == 3
    x0 = pc.near_tie("lf.x", (M, D), fmt, xscale)
    if xscale == 1.0:
        x0 = x0 * 1.5 + 0.3
    eps = 1e-5 * xscale * xscale                  # keeps var + eps in proportion: LayerNorm of the scaled stream is the same function
    x = x0.to(dev)
    zero = (torch.zeros(M, D, dtype=torch.int16, device=dev), torch.zeros(M, D, dtype=torch.int16, device=dev) if lo else None)
    wo = ops.split_bf16(_rand("lf.wo", (D, D), 0.05).to(dev), want_lo=lo, fmt=fmt)
    xpl, part = ops.linear_planes_residual_stats(zero, wo, None, x, fmt=fmt)              # x + 0: planes and slab sums of x itself
    _ok(pc.check_exact(xpl[0], xpl[1], x0, fmt), "x planes")
    st = ops.row_stats_from_partials(part, D, eps=eps)
    g, be = (1 + 0.1 * _rand("lf.g", (D,))).to(dev), (0.1 * _rand("lf.be", (D,))).to(dev)
    xv = _eff(xpl, fmt)
    xd = x0.double()
    mean, rstd = xd.mean(1, keepdim=True), torch.rsqrt(xd.var(1, unbiased=False, keepdim=True) + eps)
    for N, act, scale_cols in ((3 * D, 0, D), (F, ACT_GELU_ERF, 0)):
        w, b = _rand(f"lf.w{N}", (N, D), 0.05).to(dev), _rand(f"lf.b{N}", (N,), 0.1).to(dev)
        wg32, _, dvec = ops.ln_fold_weights(w, b, g, be)
        wg = ops.split_bf16(wg32, want_lo=lo, fmt=fmt)
        wgv = _eff(wg, fmt)
        cvec = wgv.sum(1).float().to(dev)
        oh, ol = ops.linear_planes_lnfold(xpl, wg, cvec, dvec, st, act=act, scale=0.125, scale_cols=scale_cols, fmt=fmt)
        if ol is not None:
            _ok(pc.check_pair_shape(oh, ol, fmt), f"N = {N}")
        want = rstd * (xv @ wgv.t() - mean * wgv.sum(1)) + dvec.double().cpu()
        want[:, :scale_cols] *= 0.125
        if act:
            want = O.gelu_erf(want)
        got = _eff((oh, ol), fmt)
        assert bool(torch.isfinite(got).all())
        tol = 6e-3 if split == 1 else 4e-5 if fmt == 0 else 3e-6
        assert rel_l2(got, want) < tol, (N, rel_l2(got, want))


# ======================================================================================== consumers on subnormal-range operands
# The MFMAs and the v_cvt conversions follow the kernel's denormal mode; nothing else in the suite would notice a build flag
# or a kernel attribute that flushed fp16 subnormals.  The planes below are made by the HOST reference, the truth is fp64
# arithmetic on exactly those plane values, the bars are the ones the same entry points carry elsewhere: only flushing or a
# wrong conversion can break them.  The small operand always meets one of ordinary or large magnitude, so every fp32 product
# stays above 2^-100 (2^-18 * 2^-9 at the least) and fp32 underflow plays no part.
@pytest.mark.parametrize("split,fmt,tol", CONSUMER_MODES)
@pytest.mark.parametrize("s", SMALL)
def test_plane_gemm_on_operands_in_the_subnormal_range(dev, s, split, fmt, tol):
    from rnamsm import ops
    M, N, K = 2304, 256, 768
    for what, sa, sw in (("small A", s, 0.05), ("small W", 1.0, s)):
        a, av = _host_planes(pc.near_tie(f"cg.a.{what}", (M, K), fmt, sa), split, fmt, dev)
        w, wv = _host_planes(pc.near_tie(f"cg.w.{what}", (N, K), fmt) * sw, split, fmt, dev)
        if fmt == 1:
            assert bool(((av if sa < 1 else wv).abs() < 2.0 ** -14).any())             # subnormal halves really are there
        y = ops.linear_planes(a, w, None, fmt=fmt).cpu()
        err = rel_l2(y, av @ wv.t())
        assert err < tol, (what, err)


@pytest.mark.parametrize("split,fmt,tol", CONSUMER_MODES)
@pytest.mark.parametrize("s", SMALL)
def test_row_attention_16bit_on_operands_in_the_subnormal_range(dev, s, split, fmt, tol):
    """rnamsm_row_logits16 with q in the small regime against k of magnitude 2^10 (so that a flushed q moves the logits), and
    rnamsm_row_apply16 with v in the small regime and P * 4096 spread into fp16 subnormals."""
    from rnamsm import ops
    R, C, H = 40, 130, 2
    D = 64 * H
    q, qv = _host_planes(pc.near_tie("cr.q", (R * C, D), fmt, s), split, fmt, dev)
    k, kv = _host_planes(pc.near_tie("cr.k", (R * C, D), fmt, 2.0 ** 10), split, fmt, dev)
    partial, _ = ops.row_logits16(q, k, R, C, H, fmt=fmt, scale=0.25)
    want = 0.25 * torch.einsum("rihd,rjhd->hij", qv.view(R, C, H, 64), kv.view(R, C, H, 64))
    err = rel_l2(partial.sum(0).cpu(), want)
    assert err < tol, ("logits", err)
    PS = 4096.0
    ldp = (C + 63) // 64 * 64
    P = torch.zeros(H * C, ldp)
    P[:, :C] = torch.softmax(_rand("cr.p", (H, C, C), 6.0), -1).view(H * C, C) * PS
    pp, pv = _host_planes(P, split, fmt, dev)
    v, vv = _host_planes(pc.near_tie("cr.v", (R * C, D), fmt, s), split, fmt, dev)
    ctx = ops.row_apply16(pp, v, R, C, H, fmt=fmt, out_scale=1.0 / PS).cpu()
    want = torch.einsum("hij,rjhd->rihd", pv[:, :C].reshape(H, C, C) / PS, vv.view(R, C, H, 64)).reshape(R * C, D)
    err = rel_l2(ctx, want)
    assert err < tol, ("apply", err)


@pytest.mark.parametrize("split,fmt,tol", CONSUMER_MODES)
@pytest.mark.parametrize("s", SMALL)
def test_col_attention_16bit_on_operands_in_the_subnormal_range(dev, s, split, fmt, tol):
    """rnamsm_col_attn16 with q and v in the small regime, k of magnitude 2^12: the scores are of order 1 / 2^-6, so a flushed
    q plane flattens the softmax and a flushed v plane zeroes the context.  (Plain bf16 rounds P to bf16 inside the kernel:
    its bar against the plane values is 3e-3, as in tests/test_gpu_attn16.py.)"""
    from rnamsm import ops
    R, C, H = 40, 130, 2
    D = 64 * H
    q, qv = _host_planes(pc.near_tie("cc.q", (R * C, D), fmt, s), split, fmt, dev)
    k, kv = _host_planes(pc.near_tie("cc.k", (R * C, D), fmt, 2.0 ** 12), split, fmt, dev)
    v, vv = _host_planes(pc.near_tie("cc.v", (R * C, D), fmt, s), split, fmt, dev)
    ctx = ops.col_attn16(q, k, v, R, C, H, fmt=fmt, scale=0.125).cpu()
    sc = 0.125 * torch.einsum("ichd,jchd->hcij", qv.view(R, C, H, 64), kv.view(R, C, H, 64))
    want = torch.einsum("hcij,jchd->ichd", torch.softmax(sc, -1), vv.view(R, C, H, 64)).reshape(R * C, D)
    assert float(sc.abs().max()) > (2.0 if s > 1e-5 else 0.03)                           # q does move the softmax
    err = rel_l2(ctx, want)
    assert err < (3e-3 if split == 1 else tol), err
