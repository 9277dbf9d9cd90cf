"""Every attention-path kernel at the deepest and widest shape the API admits (R, C <= 1024), in isolation.

Two shapes, both H = 12 (D = 768): (1024, 1024) is BASELINE configs[4] itself; (1021, 1019) is ragged everywhere -- the
last slab, query block and key chunk are partial and C % 8 != 0, so plain bf16 takes the 128-tile row_logits16_kernel.
What changes at this end of the range is the code path, not only the size: the fp32 row logits write 32 partial slabs
(ROW_LOGITS_F32_MAX_ROWS) and softmax_rows holds 16 values per lane, f16x3 logits hit the row16_max_rows cap, the column
kernels' key loops run four times longer than at R = 256, plain bf16 column attention runs four 256-query blocks per
column (qb2), and col_attn_probs has all 16 key tiles live.

Two kinds of check:
  * whole-output checks that catch one wrong element anywhere in the grid: on small-integer operands the row kernels
    (fp32 and 16-bit, both modes, "attn16" 1 and 2) reproduce the integer contraction bit for bit; column attention on
    operands fp16 represents exactly: f16x3 against the exact kernel at fp32-grade distance, "col_dma" 0 / 1 and plain bf16
    with two query blocks per wave against one ("attn16" 1 / 4) bit for bit, FAST against TRACKED ("attn16" 5);
  * fp64 accuracy on random-normal operands, on a seeded sample of heads (row attention) or (column, head) problems
    (column attention) that always holds the first and the last head and the last column -- at the bars of the small-shape
    tests (tests/test_gpu_kernels.py, tests/test_gpu_attn16.py MODES) as rel-L2 per head / per problem set, plus an
    element-wise companion (10 x the rel-L2 bar, relative to the largest entry) where those tests have no element bar:
    rel-L2 alone would dilute a defect in one tile across 12 M entries.
References are fp64 torch on the device; nothing GB-sized goes to the host.  Peak device memory ~45 GB (fp32 qkv 9.7 GB,
a second fp32 copy 9.7 GB, hi/lo planes 2 x 4.8 GB, fp32 context 3.2 GB, 32 partial slabs 1.6 GB, fp64 per-head operands);
every test frees what it made.  The GEMMs at 2^20 tokens are the `slow` tier.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 12
D = 64 * H
SHAPES = [(1024, 1024), (1021, 1019)]
# (split, fmt, tolerance vs eff operands, tolerance vs fp32 operands): tests/test_gpu_attn16.py MODES
MODES = [(1, 0, 2e-6, 8e-3), (3, 1, 3e-6, 3e-6)]
TOL_PROB = 2e-5             # tests/test_gpu_kernels.py
PS = 4096.0                 # plane scale of the row probabilities (rnamsm_forward's)
LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rnamsm import _lib
    _lib.load()
    return torch.device("cuda:0")


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _ints(shape, mul, mod, off, dev):
    """tests/test_gpu_attn16.py's _int_tensor, built in row blocks (one int64 index tensor of 2.4 G entries would be 19 GB)."""
    rows, cols = shape
    out = torch.empty(rows, cols, device=dev, dtype=torch.float32)
    step = max(1, (1 << 26) // cols)
    for r0 in range(0, rows, step):
        r1 = min(rows, r0 + step)
        i = torch.arange(r0 * cols, r1 * cols, device=dev, dtype=torch.int64)
        out[r0:r1] = (((i * mul + (i // 191) * 3) % mod) - off).to(torch.float32).view(r1 - r0, cols)
    return out


def _randn(shape, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn(*shape, device=dev, generator=g)


def _heads(R, C):
    """Seeded sample of heads: the first, the last and one more."""
    rng = np.random.default_rng(R * 7919 + C)
    return sorted({0, H - 1, int(rng.integers(1, H - 1))})


def _problems(R, C, n=40):
    """Seeded sample of (column, head) problems: first column / head, last column with the first and the last head."""
    rng = np.random.default_rng(R * 104729 + C)
    cs = [0, C - 1, C - 1] + [int(x) for x in rng.integers(0, C, n - 3)]
    hs = [0, H - 1, 0] + [int(x) for x in rng.integers(0, H, n - 3)]
    return torch.tensor(cs), torch.tensor(hs)


def _check(got, want, rel_bar, max_bar, what):
    err = got.double() - want
    rel = float(err.norm() / want.norm().clamp_min(1e-300))
    mx = float(err.abs().max())
    assert rel < rel_bar and mx < max_bar, f"{what}: rel-L2 {rel:.2e} (bar {rel_bar:.0e}), max-abs {mx:.2e} (bar {max_bar:.2e})"


def _ht(fmt):
    return torch.float16 if fmt == 1 else torch.bfloat16


def _plane_views(pl, a, b):
    return (pl[0][:, a:b], None if pl[1] is None else pl[1][:, a:b])


def _plane_vals(pl, fmt, index):
    """fp64 values held by the planes at `index` (a callable on a tensor): hi, or hi + lo."""
    ht = _ht(fmt)
    v = index(pl[0]).contiguous().view(ht).double()
    if pl[1] is not None:
        v = v + index(pl[1]).contiguous().view(ht).double()
    return v


def _head_rows(x, R, C, h):
    """[R*C, H*64] view -> [C, R*64] fp64 for head h (row i of the result: token column i, all alignment rows)."""
    return x.view(R, C, H, 64)[:, :, h, :].permute(1, 0, 2).reshape(C, R * 64).double()


def _set(name, value):
    from rnamsm import ops
    ops.set_param(name, value)


# ------------------------------------------------------------------------------------------------ whole-output checks
@pytest.mark.parametrize("R,C", SHAPES)
def test_row_kernels_are_exact_on_integers_at_the_limit(dev, R, C):
    """|q.k| <= 4 * 64 R = 2^18 and |P v| <= 6 C: every partial sum is an integer below 2^24, so the fp32 logits (32 slabs of
    <= 32 rows), the fp32 apply and both 16-bit modes must equal the integer contraction -- the 16-bit kernels with the
    256x256 tiles ("attn16" = 1, where the shape takes them) and with 128x128 tiles ("attn16" = 2)."""
    from rnamsm import ops, _lib
    T = R * C
    qkv = _ints((T, 3 * D), 7, 5, 2, dev)
    assert _lib.load().rnamsm_row_logits_nsplit(R, C, H) >= 32
    p32, _ = ops.row_logits(qkv[:, :D], qkv[:, D:2 * D], R, C, H)
    s32 = p32.sum(0)
    del p32
    for h in range(H):
        qh, kh = _head_rows(qkv[:, :D], R, C, h), _head_rows(qkv[:, D:2 * D], R, C, h)
        assert torch.equal(s32[h].double(), qh @ kh.t()), h
        del qh, kh
    ldp = (C + 63) // 64 * 64
    pint = _ints((H * C, ldp), 5, 7, 3, dev)
    pint[:, C:] = 0
    c32 = ops.row_apply(pint[:, :C].reshape(H, C, C).contiguous(), qkv[:, 2 * D:], R, C, H)
    for h in range(H):
        want = pint[h * C:(h + 1) * C, :C].double() @ _head_rows(qkv[:, 2 * D:], R, C, h)
        assert torch.equal(c32.view(R, C, H, 64)[:, :, h, :].double(), want.view(C, R, 64).permute(1, 0, 2)), h
        del want
    try:
        for split, fmt, _, _ in MODES:
            pl = ops.split_bf16(qkv, want_lo=split == 3, fmt=fmt)
            pp = ops.split_bf16(pint, want_lo=split == 3, fmt=fmt)
            for var in (1, 2):
                _set("attn16", var)
                p16, _ = ops.row_logits16(_plane_views(pl, 0, D), _plane_views(pl, D, 2 * D), R, C, H, fmt=fmt)
                assert torch.equal(p16.sum(0), s32), (split, fmt, var)
                del p16
                c16 = ops.row_apply16(pp, _plane_views(pl, 2 * D, 3 * D), R, C, H, fmt=fmt)
                assert torch.equal(c16, c32), (split, fmt, var)
                del c16
            del pl, pp
    finally:
        _set("attn16", 1)
    del qkv, s32, c32, pint
    _free()


@pytest.mark.parametrize("R,C", SHAPES)
def test_col_kernels_agree_over_the_whole_grid_at_the_limit(dev, R, C):
    """Operands in multiples of 1/4 in [-1, 1] (exact in bf16 and fp16): f16x3 col_attn16 sits at fp32-grade distance from the
    exact kernel everywhere (the bars of test_full_grid_col_attention_16bit_against_the_exact_kernel); the exact kernel's two
    staging variants ("col_dma" 0 / 1) run the same arithmetic per 32-key tile and give the same bits; plain bf16 with two
    128-query blocks per wave (four 256-query blocks per column at R = 1024) gives the same bits as one block per wave
    ("attn16" = 4: every query's key loop, its FAST reference and its P rounding are the same); and the FAST loop stays within
    the fallback test's element bar (1e-2) of the TRACKED loop ("attn16" = 5).  The f16x3-vs-exact rel-L2 bar is 5e-6 here, not
    the 2e-6 of R = 256: see tests/analysis/README.md (tolerance table)."""
    from rnamsm import ops
    T = R * C
    qkv = _ints((T, 3 * D), 7, 9, 4, dev).mul_(0.25)
    pl = ops.split_bf16(qkv, fmt=1)
    v = lambda a, b: _plane_views(pl, a, b)
    c16 = ops.col_attn16(v(0, D), v(D, 2 * D), v(2 * D, 3 * D), R, C, H, fmt=1, scale=0.125)
    del pl
    qkv[:, :D] *= 0.125                                                  # exact: a power of two
    try:
        outs = {}
        for dma in (0, 1):
            _set("col_dma", dma)
            outs[dma] = ops.col_attn(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], R, C, H)
    finally:
        _set("col_dma", -1)
    assert torch.equal(outs[0], outs[1])
    c32 = outs.pop(0)
    del outs
    # (2e-6 at R = 256; over 1024 keys the exact kernel itself sits 2.4e-6 from fp64 on these operands -- torch fp32 3.0e-6, f16x3
    # 3e-7 -- so the distance of the two is the exact kernel's fp32 rounding: each is held to fp64 at its own bar instead)
    _check(c16, c32.double(), 5e-6, 2e-5, "f16x3 col_attn16 vs the exact kernel")
    cs, hs = _problems(R, C)
    want = _col_ref(*(_pick(qkv[:, a:a + D], R, C, cs, hs).double() for a in (0, D, 2 * D)))
    _check(_pick(c16, R, C, cs, hs), want, 3e-6, 10 * 3e-6 * float(want.abs().max()), "f16x3 col_attn16 vs fp64")
    _check(_pick(c32, R, C, cs, hs), want, 5e-6, 2e-5 * max(1.0, float(want.abs().max())), "exact col_attn vs fp64")
    del c16, want
    qkv[:, :D] *= 8.0
    pl = ops.split_bf16(qkv, want_lo=False, fmt=0)
    args = (_plane_views(pl, 0, D), _plane_views(pl, D, 2 * D), _plane_views(pl, 2 * D, 3 * D), R, C, H)
    try:
        b = {}
        for var in (1, 4, 5):
            _set("attn16", var)
            b[var] = ops.col_attn16(*args, fmt=0, scale=0.125)
    finally:
        _set("attn16", 1)
    assert bool(torch.isfinite(b[1]).all())
    _check(b[1], b[5].double(), 1.0, 1e-2, "bf16 FAST vs TRACKED")
    _check(b[1], c32.double(), 1.0, 1e-2, "bf16 FAST vs the exact kernel")
    _check(b[5], c32.double(), 1.0, 1e-2, "bf16 TRACKED vs the exact kernel")
    assert torch.equal(b[1], b[4])
    del b, pl, qkv, c32
    _free()


# ---------------------------------------------------------------------------------------------- fp64 accuracy: rows
@pytest.mark.parametrize("R,C", SHAPES)
def test_row_attention_fp32_against_fp64_at_the_limit(dev, R, C):
    """fp32 row_logits (32+ slabs), softmax_rows over the summed slabs -- q prescaled, the depth factor applied to the summed
    logits (logit_scale), and a key mask -- and row_apply, on the sampled heads, at tests/test_gpu_kernels.py's bars."""
    from rnamsm import ops
    T = R * C
    scaling = ops.row_scaling(R)
    qkv = _randn((T, 3 * D), 1000 + R, dev)
    qs = (qkv[:, :D] * scaling).contiguous()
    part, nsplit = ops.row_logits(qs, qkv[:, D:2 * D].contiguous(), R, C, H)
    assert nsplit >= 32
    probs = ops.softmax_rows(part)
    del part
    part2, _ = ops.row_logits(qkv[:, :D], qkv[:, D:2 * D], R, C, H)                # strided views, unscaled q
    probs_ls = ops.softmax_rows(part2, logit_scale=ops.depth_scaling(R) * 0.125)
    key_mask = (_randn((C,), 77, dev) > 1.0).to(torch.uint8)
    key_mask[0] = 0
    probs_km = ops.softmax_rows(part2, key_mask=key_mask, logit_scale=ops.depth_scaling(R) * 0.125)
    ctx = ops.row_apply(probs, qkv[:, 2 * D:], R, C, H)
    assert float((probs.sum(-1) - 1).abs().max()) < 1e-5
    for h in _heads(R, C):
        qh, kh = _head_rows(qs, R, C, h), _head_rows(qkv[:, D:2 * D], R, C, h)
        logits = qh @ kh.t()
        _check(probs[h], torch.softmax(logits, -1), 1.0, TOL_PROB, f"probs head {h}")
        lu = _head_rows(qkv[:, :D], R, C, h) @ kh.t()
        _check(part2[:, h].sum(0), lu, 5e-6, 10 * 5e-6 * float(lu.abs().max()), f"logits head {h}")
        sc = ops.depth_scaling(R) * 0.125
        _check(probs_ls[h], torch.softmax(lu * sc, -1), 1.0, TOL_PROB, f"logit_scale probs head {h}")
        _check(probs_km[h], torch.softmax((lu * sc).masked_fill(key_mask.bool()[None, :], -10000.0), -1), 1.0, TOL_PROB,
               f"masked probs head {h}")
        assert float(probs_km[h][:, key_mask.bool()].abs().max()) == 0.0
        want = (probs[h].double() @ _head_rows(qkv[:, 2 * D:], R, C, h)).view(C, R, 64).permute(1, 0, 2)
        _check(ctx.view(R, C, H, 64)[:, :, h, :], want, 5e-6, 10 * 5e-6 * float(want.abs().max()), f"ctx head {h}")
        del qh, kh, logits, lu, want
    del qkv, qs, part2, probs, probs_ls, probs_km, ctx
    _free()


@pytest.mark.parametrize("split,fmt,tol_eff,tol_f32", MODES)
@pytest.mark.parametrize("R,C", SHAPES)
def test_row_attention_16bit_against_fp64_at_the_limit(dev, R, C, split, fmt, tol_eff, tol_f32):
    """row_logits16 (f16x3: slabs capped at row16_max_rows = 32), softmax_rows_planes (P * 4096 in the planes, the pad columns
    C..ldp zero) and row_apply16, on the sampled heads, against fp64 on the values the planes hold and on the fp32 operands
    (tests/test_gpu_attn16.py's MODES and probability bars)."""
    from rnamsm import ops
    T = R * C
    scale = ops.row_scaling(R)
    qkv = _randn((T, 3 * D), 2000 + R, dev)
    pl = ops.split_bf16(qkv, want_lo=split == 3, fmt=fmt)
    partial, _ = ops.row_logits16(_plane_views(pl, 0, D), _plane_views(pl, D, 2 * D), R, C, H, fmt=fmt, scale=scale)
    probs, pp = ops.softmax_rows_planes(partial, split=split, fmt=fmt, plane_scale=PS)
    summed = partial.sum(0)
    del partial
    ht = _ht(fmt)
    ldp = (C + 63) // 64 * 64
    assert pp[0].shape == (H * C, ldp)
    assert torch.equal(pp[0][:, :C].reshape(H, C, C), (probs * PS).to(ht).view(torch.int16))          # hi = round(P * 2^12)
    assert int(pp[0][:, C:].abs().max() if ldp > C else 0) == 0
    if split == 3:
        assert int(pp[1][:, C:].abs().max() if ldp > C else 0) == 0
    ctx = ops.row_apply16(pp, _plane_views(pl, 2 * D, 3 * D), R, C, H, fmt=fmt, out_scale=1.0 / PS)
    for h in _heads(R, C):
        sl = lambda a: (lambda t: t[:, a + h * 64:a + (h + 1) * 64].reshape(R, C, 64).permute(1, 0, 2).reshape(C, R * 64))
        qe, ke, ve = (_plane_vals(pl, fmt, sl(a)) for a in (0, D, 2 * D))
        le = scale * (qe @ ke.t())
        _check(summed[h], le, tol_eff, 10 * tol_eff * float(le.abs().max()), f"logits vs eff, head {h}")
        del qe, ke, le
        lf = scale * (_head_rows(qkv[:, :D], R, C, h) @ _head_rows(qkv[:, D:2 * D], R, C, h).t())
        _check(summed[h], lf, tol_f32, 10 * tol_f32 * float(lf.abs().max()), f"logits vs fp32 operands, head {h}")
        want_p = torch.softmax(summed[h].double(), -1)
        _check(probs[h], want_p, 1.0, 2e-6, f"probs head {h}")
        rows = lambda t: t[h * C:(h + 1) * C, :C]
        p_eff = _plane_vals(pp, fmt, rows)
        if split == 3:
            assert float((p_eff / PS - probs[h].double()).abs().max()) < (2e-5 if fmt == 0 else 3e-7)
        want = ((p_eff / PS) @ ve).view(C, R, 64).permute(1, 0, 2)
        got = ctx.view(R, C, H, 64)[:, :, h, :]
        _check(got, want, tol_eff, 10 * tol_eff * float(want.abs().max()), f"ctx vs eff, head {h}")
        want = (torch.softmax(lf, -1) @ _head_rows(qkv[:, 2 * D:], R, C, h)).view(C, R, 64).permute(1, 0, 2)
        _check(got, want, tol_f32, 10 * tol_f32 * float(want.abs().max()), f"ctx vs fp32 operands, head {h}")
        del ve, lf, want_p, p_eff, want, got
    del qkv, pl, probs, pp, summed, ctx
    _free()


# ------------------------------------------------------------------------------------------- fp64 accuracy: columns
def _col_ref(q, k, v, mask=None):
    """q, k, v fp64 [R, P, 64] (q scaled); mask bool [R, P] (key padded) -> context [R, P, 64]."""
    s = torch.einsum("ipd,jpd->pij", q, k)
    if mask is not None:
        s = s.masked_fill(mask.t()[:, None, :], -10000.0)
    return torch.einsum("pij,jpd->ipd", torch.softmax(s, -1), v)


def _pick(x, R, C, cs, hs):
    """[R*C, H*64] view (fp32 or int16 planes) -> [R, P, 64] of the sampled (column, head) problems."""
    return x.view(R, C, H, 64)[:, cs, hs, :]


@pytest.mark.parametrize("R,C", SHAPES)
def test_col_attention_fp32_against_fp64_at_the_limit(dev, R, C):
    """The exact column kernel on the sampled problems: natural-domain q (both staging variants), and the log2-domain
    prescaled entry with the FAST first pass and with the online softmax only ("col_fast" 1 / 0) -- at
    tests/test_gpu_kernels.py's bars (rel-L2 5e-6, element 2e-5 x max(1, max |want|))."""
    from rnamsm import ops
    T = R * C
    cs, hs = _problems(R, C)
    qkv = _randn((T, 3 * D), 3000 + R, dev)
    qkv[:, :D] *= 0.125
    q, k, v = (_pick(qkv[:, a:a + D], R, C, cs, hs).double() for a in (0, D, 2 * D))
    want = _col_ref(q, k, v)
    bar = 2e-5 * max(1.0, float(want.abs().max()))
    try:
        for dma in (0, 1):
            _set("col_dma", dma)
            ctx = ops.col_attn(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], R, C, H)
            _check(_pick(ctx, R, C, cs, hs), want, 5e-6, bar, f"col_attn col_dma={dma}")
            del ctx
    finally:
        _set("col_dma", -1)
    qkv[:, :D] *= LOG2E
    want = _col_ref(_pick(qkv[:, :D], R, C, cs, hs).double() / LOG2E, k, v)
    try:
        for fast in (1, 0):
            _set("col_fast", fast)
            ctx = ops.col_attn(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], R, C, H, prescaled=True)
            assert bool(torch.isfinite(ctx).all())
            _check(_pick(ctx, R, C, cs, hs), want, 5e-6, bar, f"col_attn prescaled col_fast={fast}")
            del ctx
    finally:
        _set("col_fast", 1)
    del qkv, q, k, v, want
    _free()


@pytest.mark.parametrize("split,fmt,tol_eff,tol_f32", MODES)
@pytest.mark.parametrize("R,C", SHAPES)
def test_col_attention_16bit_against_fp64_at_the_limit(dev, R, C, split, fmt, tol_eff, tol_f32):
    """col_attn16 on the sampled problems, without and with a padding mask, fp32 and plane output; for plain bf16 also the
    TRACKED loop ("attn16" = 5) and the prescaled log2-domain entry -- at tests/test_gpu_attn16.py's bars (P rounded to bf16
    inside the kernel: 3e-3 against the plane values in plain bf16)."""
    from rnamsm import ops
    T = R * C
    cs, hs = _problems(R, C)
    qkv = _randn((T, 3 * D), 4000 + R, dev)
    pl = ops.split_bf16(qkv, want_lo=split == 3, fmt=fmt)
    args = (_plane_views(pl, 0, D), _plane_views(pl, D, 2 * D), _plane_views(pl, 2 * D, 3 * D), R, C, H)
    pick = lambda a: (lambda t: _pick(t[:, a:a + D], R, C, cs, hs))
    qe, ke, ve = (_plane_vals(pl, fmt, pick(a)) for a in (0, D, 2 * D))
    q, k, v = (_pick(qkv[:, a:a + D], R, C, cs, hs).double() for a in (0, D, 2 * D))
    te = 3e-3 if split == 1 else tol_eff
    want_e, want_f = _col_ref(0.125 * qe, ke, ve), _col_ref(0.125 * q, k, v)
    bar_e, bar_f = 10 * te * float(want_e.abs().max()), 10 * tol_f32 * float(want_f.abs().max())

    ctx = ops.col_attn16(*args, fmt=fmt, scale=0.125)
    assert bool(torch.isfinite(ctx).all())
    _check(_pick(ctx, R, C, cs, hs), want_e, te, bar_e, "col_attn16 vs eff")
    _check(_pick(ctx, R, C, cs, hs), want_f, tol_f32, bar_f, "col_attn16 vs fp32 operands")
    # plane output: hi = the fp32 output rounded to the format, hi + lo = it to the pair's precision (whole output)
    hi, lo = ops.col_attn16(*args, fmt=fmt, scale=0.125, out_planes=True)
    ht = _ht(fmt)
    u16 = 2.0 ** (-8 if fmt == 0 else -11)
    for r0 in range(0, T, 1 << 17):
        f = ctx[r0:r0 + (1 << 17)].double()
        h16 = hi[r0:r0 + (1 << 17)].view(ht).double()
        assert bool(((h16 - f).abs() <= u16 * f.abs() * (1 + 1e-3) + 1e-7).all()), r0
        if split == 3:
            back = h16 + lo[r0:r0 + (1 << 17)].view(ht).double()
            assert bool(((back - f).abs() <= (2.0 ** -16 if fmt == 0 else 2.0 ** -21) * f.abs() + 2e-7).all()), r0
        else:
            assert lo is None
        del f, h16
    del hi, lo, ctx
    if split == 1:
        try:
            _set("attn16", 5)
            tracked = ops.col_attn16(*args, fmt=fmt, scale=0.125)
        finally:
            _set("attn16", 1)
        _check(_pick(tracked, R, C, cs, hs), want_e, te, bar_e, "col_attn16 TRACKED vs eff")
        del tracked
    # padding mask on the keys of each column (row 0 kept: a column never loses all its keys in the reference's use)
    pad = _randn((R, C), 5000 + R, dev) > 0.85
    pad[0] = False
    ctx = ops.col_attn16(*args, fmt=fmt, scale=0.125, pad_mask=pad.to(torch.uint8).contiguous())
    assert bool(torch.isfinite(ctx).all())
    mk = pad[:, cs]
    want_m = _col_ref(0.125 * qe, ke, ve, mk)
    _check(_pick(ctx, R, C, cs, hs), want_m, te, 10 * te * float(want_m.abs().max()), "col_attn16 masked vs eff")
    del ctx, want_m
    del pl, args
    if split == 1:
        # the forward's entry in the bf16 modes: q planes hold q * dh^-0.5 * log2(e), rounded once
        qkv[:, :D] *= 0.125 * LOG2E
        pl = ops.split_bf16(qkv, want_lo=False, fmt=0)
        args = (_plane_views(pl, 0, D), _plane_views(pl, D, 2 * D), _plane_views(pl, 2 * D, 3 * D), R, C, H)
        qp = _plane_vals(pl, 0, pick(0))
        want_p = _col_ref(qp / LOG2E, ke, ve)
        try:
            for var in (1, 5):
                _set("attn16", var)
                got = ops.col_attn16(*args, fmt=0, prescaled=True)
                assert bool(torch.isfinite(got).all())
                _check(_pick(got, R, C, cs, hs), want_p, 3e-3, 10 * 3e-3 * float(want_p.abs().max()), f"prescaled attn16={var} vs eff")
                _check(_pick(got, R, C, cs, hs), want_f, 8e-3, 10 * 8e-3 * float(want_f.abs().max()), f"prescaled attn16={var} vs fp32")
                del got
        finally:
            _set("attn16", 1)
        del pl, args, qp, want_p
    del qkv, qe, ke, ve, q, k, v, want_e, want_f, pad
    _free()


@pytest.mark.parametrize("R,C", [(1024, 3), (1021, 2)])
def test_col_attn_probs_with_every_key_tile_live(dev, R, C):
    """col_attn_probs / col_attn_probs16 at R up to 1024: all CP_MAXT = 16 key tiles of a lane hold keys (the last one partial
    at R = 1021), whole output against fp64 -- fp32 operands without and with a padding mask (2e-6, tests/test_gpu_kernels.py),
    fp16 hi/lo planes (5e-6, same file), and bf16 planes against the plane values (5e-6)."""
    from rnamsm import ops
    Hs = 2
    Ds = 64 * Hs
    qkv = _randn((R * C, 2 * Ds), 6000 + R, dev)
    q = (qkv[:, :Ds].double() * 0.125).view(R, C, Hs, 64)
    k = qkv[:, Ds:].double().view(R, C, Hs, 64)
    s = torch.einsum("ichd,jchd->hcij", q, k)
    want = torch.softmax(s, -1)
    gq = qkv.clone()
    gq[:, :Ds] *= 0.125
    got = ops.col_attn_probs(gq[:, :Ds], gq[:, Ds:], R, C, Hs)
    assert got.shape == (Hs, C, R, R) and float((got.double() - want).abs().max()) < 2e-6
    pad = _randn((R, C), 6100 + R, dev) > 0.8
    pad[0] = False
    wm = torch.softmax(s.masked_fill(pad.t()[None, :, None, :], -10000.0), -1)
    got = ops.col_attn_probs(gq[:, :Ds], gq[:, Ds:], R, C, Hs, pad_mask=pad.to(torch.uint8).view(-1).contiguous())
    assert float((got.double() - wm).abs().max()) < 2e-6
    for fmt in (1, 0):
        hi, lo = ops.split_bf16(qkv, want_lo=fmt == 1, fmt=fmt)
        got = ops.col_attn_probs16((hi[:, :Ds], None if lo is None else lo[:, :Ds]), (hi[:, Ds:], None if lo is None else lo[:, Ds:]),
                                   R, C, Hs, fmt=fmt, scale=0.125)
        if fmt == 1:
            assert float((got.double() - want).abs().max()) < 5e-6
        e = hi.view(_ht(fmt)).double() + (0 if lo is None else lo.view(_ht(fmt)).double())
        se = torch.einsum("ichd,jchd->hcij", 0.125 * e[:, :Ds].view(R, C, Hs, 64), e[:, Ds:].view(R, C, Hs, 64))
        assert float((got.double() - torch.softmax(se, -1)).abs().max()) < 5e-6, fmt
        del hi, lo, got, e, se
    del qkv, gq, q, k, s, want, wm
    _free()


def test_contact_head_and_pack_outputs_at_1024(dev):
    """contact_head at C = 1024 with 120 channels (10 layers x 12 heads: configs[4]'s), O(1) weights as in
    test_contact_head_kernel_on_random_maps_with_large_weights, against the oracle's symmetrize / APC / logistic in fp64 at
    the same 2e-5 bar; every 32-row tile row of the output is live (the last one, blockIdx.y = 31, only exists for C > 993).
    And pack_outputs at that width as a pure copy."""
    from oracle import msm_oracle as O
    from rnamsm import ops
    C, nch = 1024, 120
    a = torch.softmax(_randn((nch, C, C), 7000, dev) * 3, -1)
    w = _randn((1, nch), 7001, dev) * 20
    b = torch.tensor([0.3], device=dev)
    got = ops.contact_head(a, w, b)
    want = O.contact_head(a.double(), w.double(), b.double())
    assert got.shape == (C - 1, C - 1) and float((got.double() - want).abs().max()) < 2e-5
    del got, want
    NL, R = 10, 2
    x = _randn((R * C, D), 7002, dev)
    emb, atp = ops.pack_outputs(x, a.view(NL, H, C, C), C)
    assert torch.equal(emb, x.view(R, C, D)[0, 1:])
    assert torch.equal(atp, a.view(NL, H, C, C)[..., 1:, 1:].reshape(NL * H, C - 1, C - 1))
    del a, x, emb, atp
    _free()


# --------------------------------------------------------------------------------------------------------- slow tier
@pytest.mark.slow
@pytest.mark.parametrize("N,K", [(3 * D, D), (D, 4 * D)])
def test_gemms_at_a_million_tokens_are_exact_on_integers(dev, N, K):
    """The QKV (N = 2304, K = 768) and fc2 (N = 768, K = 3072) GEMMs at 2^20 tokens on small integers: ops.linear equals the
    fp64 integer product, and linear_planes in both 16-bit modes equals ops.linear -- compared in row blocks of 128 k rows."""
    from rnamsm import ops
    M = 1 << 20
    x = _ints((M, K), 3 if K > D else 7, 7 if K > D else 13, 3 if K > D else 6, dev)
    w = _ints((N, K), 5, 11, 5, dev)
    want = ops.linear(x, w)
    wd = w.double().t()
    for r0 in range(0, M, 1 << 17):
        assert torch.equal(want[r0:r0 + (1 << 17)].double(), x[r0:r0 + (1 << 17)].double() @ wd), r0
    del wd
    for split, fmt, _, _ in MODES:
        got = ops.linear_planes(ops.split_bf16(x, want_lo=split == 3, fmt=fmt), ops.split_bf16(w, want_lo=split == 3, fmt=fmt), fmt=fmt)
        for r0 in range(0, M, 1 << 17):
            assert torch.equal(got[r0:r0 + (1 << 17)], want[r0:r0 + (1 << 17)]), (split, fmt, r0)
        del got
    del x, w, want
    _free()
