"""The two shared K loops of the 16-bit 256x256 kernels (csrc/mma16_core.h) in every loop regime, on small-integer operands.

Regimes of a loop: nk == 1 (the second start-up request is a redundant reload), nk == 2, nk >= 3 (the clamped reload in steady
state), each with a full tile grid and with a ragged edge.  Operand entries are integers in [-8, 8]: exact in bf16 and fp16 (lo
planes zero), every product exact, and with K <= 192 every fp32 partial sum stays below 2^24 -- so the result must EQUAL the integer
matmul whatever the summation order (the truth of test_row_kernels_16bit_are_exact_on_integers).  For f16x3 one case per kernel
uses n + 2^-9 m (m in [-8, 8] too): the lo planes are non-zero, all three products run; reference fp64, bar = test_gpu_attn16's
for that mode.

    kernel                  nk                                  cases
    gemm16_swp_kernel       K / 64 (bf16), K / 32 (f16x3)       M 2048 / 2300, N 256 (and 1280 for f16x3: bf16 goes to q16s there)
                            K 64 / 128 / 192: bf16 nk 1, 2, 3; f16x3 nk 2, 4, 6 (the entry point takes K % 64 == 0 only)
    gemm16_q16s_kernel      K / 64                              N 1280 (the wide-N rule) and N 256 with "gemm16_mfma16" = 2
    row_logits16q_kernel    alignment rows of a split           bf16, C 384 / 392 / 512, H 1 / 2
    row_logits16x_kernel    2 x alignment rows of a split       f16x3, C 256 / 264 / 520 (nk == 1 cannot occur)
    row_apply16x_kernel     ceil(C / 64) (bf16), / 32 (f16x3)   C 256 / 300 with R 5 (R 1 stays on the 128x128 kernel: run too)
"""
import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

FORMATS = [(1, 0), (3, 1)]                   # (split, fmt): plain bf16, f16x3
TOL_F16X3 = 3e-6                             # tests/test_gpu_attn16.py MODES, f16x3 against the values the planes hold
LOGITS_R = (1, 2, 3, 9)                      # 1, 2, 3 rows in one split; 9 = several splits
LOGITS_C = {1: (384, 392, 512), 3: (256, 264, 520)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rnamsm import _lib
    _lib.load()
    return torch.device("cuda:0")


def _ints(shape, seed, lo_part=False):
    """Integers in [-8, 8] (plus 2^-9 times such integers), asymmetric in every index, fp32 on the host."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.int64)
    x = (((i * (7 + 2 * seed) + (i // 191) * 3 + seed) % 17) - 8).astype(np.float64)
    if lo_part:
        x = x + 2.0 ** -9 * (((i * 5 + (i // 67) + 3 * seed) % 17) - 8)
    return torch.from_numpy(x.astype(np.float32)).view(*shape)


def _planes(x, split, fmt, dev):
    from rnamsm import ops
    pl = ops.split_bf16(x.to(dev), want_lo=(split == 3), fmt=fmt)
    ht = torch.float16 if fmt == 1 else torch.bfloat16
    eff = pl[0].view(ht).double() + (pl[1].view(ht).double() if pl[1] is not None else 0)
    assert torch.equal(eff.cpu(), x.double())                         # the planes hold the operands exactly
    return pl


def _values(pl, fmt):
    ht = torch.float16 if fmt == 1 else torch.bfloat16
    return pl[0].cpu().view(ht).double() + (pl[1].cpu().view(ht).double() if pl[1] is not None else 0)


def _views(pl, a, b):
    return (pl[0][:, a:b], None if pl[1] is None else pl[1][:, a:b])


@pytest.fixture(scope="module")
def gemm_truth():
    """(M, N, K, lo_part) -> (a, w, fp64 a w^T), computed once per shape and left unchanged"""
    cache = {}

    def get(M, N, K, lo_part=False):
        key = (M, N, K, lo_part)
        if key not in cache:
            a, w = _ints((M, K), 1, lo_part), _ints((N, K), 2, lo_part)
            cache[key] = (a, w, a.double() @ w.double().t())
        return cache[key]
    return get


def _gemm_checks(dev, split, fmt, M, N, K, truth):
    from rnamsm import ops
    a, w, want = truth(M, N, K)
    ap, wp = _planes(a, split, fmt, dev), _planes(w, split, fmt, dev)
    assert torch.equal(ops.linear_planes(ap, wp, None, fmt=fmt).cpu().double(), want)
    res = _ints((M, N), 3)
    assert torch.equal(ops.linear_planes(ap, wp, None, residual=res.to(dev), fmt=fmt).cpu().double(), want + res.double())
    got = _values(ops.linear_planes(ap, wp, None, out_planes=True, fmt=fmt), fmt)
    ht = torch.float16 if fmt == 1 else torch.bfloat16
    # |sums| <= 64 K <= 12288: exact as an fp16 pair; one bf16 keeps 8 bits -- the rounding of the exact value
    assert torch.equal(got, want if split == 3 else want.float().to(ht).double())


@pytest.mark.parametrize("split,fmt", FORMATS)
@pytest.mark.parametrize("N", [256, 1280])
@pytest.mark.parametrize("M", [2048, 2300])
def test_plane_gemm_loop_regimes_on_integers(dev, gemm_truth, M, N, split, fmt):
    """Plain bf16 (64-deep tiles): nk = 1, 2, 3 of the ring (N 256) and of the staged loop (N 1280).  f16x3 (32-deep tiles): nk =
    2, 4, 6 of the ring -- rnamsm_gemm_bf16 takes K % 64 == 0 only, so an odd count of 32-deep tiles (K = 96) and nk == 1 cannot
    occur in this mode."""
    for K in (64, 128, 192):
        _gemm_checks(dev, split, fmt, M, N, K, gemm_truth)


@pytest.mark.parametrize("M", [2048, 2300])
def test_staged_gemm_forced_at_narrow_n_on_integers(dev, gemm_truth, M):
    """gemm16_q16s_kernel at N = 256 ("gemm16_mfma16" = 2), nk = 1, 2, 3"""
    from rnamsm import _lib
    lib = _lib.load()
    default = lib.rnamsm_get_param(b"gemm16_mfma16")
    try:
        _lib.check(lib.rnamsm_set_param(b"gemm16_mfma16", 2))
        for K in (64, 128, 192):
            _gemm_checks(dev, 1, 0, M, 256, K, gemm_truth)
    finally:
        _lib.check(lib.rnamsm_set_param(b"gemm16_mfma16", default))


@pytest.mark.parametrize("split,fmt", FORMATS)
def test_folded_gemm_entry_points_on_integers(dev, gemm_truth, split, fmt):
    """rnamsm_gemm16_lnfold with (mean, rstd) = (0, 1), c = d = 0 and rnamsm_gemm16_residual_stats without bias: the plain sums"""
    from rnamsm import ops
    M, N, K = 2300, 256, 128
    a, w, want = gemm_truth(M, N, K)
    ap, wp = _planes(a, split, fmt, dev), _planes(w, split, fmt, dev)
    ht = torch.float16 if fmt == 1 else torch.bfloat16
    stats = torch.tensor([0.0, 1.0]).repeat(M, 1).contiguous().to(dev)
    zero = torch.zeros(N, device=dev)
    got = _values(ops.linear_planes_lnfold(ap, wp, zero, zero, stats, fmt=fmt), fmt)
    assert torch.equal(got, want if split == 3 else want.float().to(ht).double())
    res = _ints((M, N), 3)
    x = res.to(dev)
    xpl, _ = ops.linear_planes_residual_stats(ap, wp, None, x, fmt=fmt)
    assert torch.equal(x.cpu().double(), want + res.double())
    assert torch.equal(_values(xpl, fmt), (want + res.double()) if split == 3 else (want + res.double()).float().to(ht).double())


def test_f16x3_gemm_with_nonzero_lo_planes(dev, gemm_truth):
    from rnamsm import ops
    for M, N, K in ((2300, 256, 64), (2048, 1280, 128)):
        a, w, want = gemm_truth(M, N, K, True)
        got = ops.linear_planes(_planes(a, 3, 1, dev), _planes(w, 3, 1, dev), None, fmt=1).cpu()
        assert rel_l2(got, want) < TOL_F16X3


def _rows_of_splits(R, C, H, split):
    from rnamsm import _lib
    n = _lib.load().rnamsm_row_logits16_nsplit(R, C, H, split)
    rps = -(-R // n)
    return [min(R, (s + 1) * rps) - s * rps for s in range(n)]


@pytest.mark.parametrize("split", [1, 3])
def test_logits_cases_cover_every_loop_regime(dev, split):
    """1, 2 and >= 3 alignment rows per split at every (C, H): a later change of the row split cannot silently untest a regime"""
    for C in LOGITS_C[split]:
        for H in (1, 2):
            rows = {r for R in LOGITS_R for r in _rows_of_splits(R, C, H, split)}
            assert 1 in rows and 2 in rows and any(r >= 3 for r in rows), (split, C, H, sorted(rows))


def _logits_case(dev, split, fmt, R, C, H, lo_part=False):
    from rnamsm import ops
    D = 64 * H
    qk = _ints((R * C, 2 * D), 4, lo_part)
    pl = _planes(qk, split, fmt, dev)
    partial, _ = ops.row_logits16(_views(pl, 0, D), _views(pl, D, 2 * D), R, C, H, fmt=fmt)
    q, k = qk[:, :D].double().view(R, C, H, 64), qk[:, D:].double().view(R, C, H, 64)
    return partial.sum(0).cpu().double(), torch.einsum("rihd,rjhd->hij", q, k)


@pytest.mark.parametrize("split,fmt", FORMATS)
@pytest.mark.parametrize("H", [1, 2])
def test_row_logits_loop_regimes_on_integers(dev, split, fmt, H):
    """|sums| <= 64 * 64 R <= 36864 per split and 9 rows in all: exact in fp32, partial slabs included"""
    for C in LOGITS_C[split]:
        for R in LOGITS_R:
            got, want = _logits_case(dev, split, fmt, R, C, H)
            assert torch.equal(got, want), (R, C, H)


def test_f16x3_row_logits_with_nonzero_lo_planes(dev):
    got, want = _logits_case(dev, 3, 1, 3, 264, 2, True)
    assert rel_l2(got, want) < TOL_F16X3


def _apply_case(dev, split, fmt, R, C, lo_part=False):
    from rnamsm import ops
    H, D = 2, 128
    ldp = (C + 63) // 64 * 64
    p = _ints((H * C, ldp), 5, lo_part)
    p[:, C:] = 0
    v = _ints((R * C, D), 6, lo_part)
    ctx = ops.row_apply16(_planes(p, split, fmt, dev), _planes(v, split, fmt, dev), R, C, H, fmt=fmt).cpu()
    want = torch.einsum("hij,rjhd->rihd", p[:, :C].double().view(H, C, C), v.double().view(R, C, H, 64)).reshape(R * C, D)
    return ctx.double(), want


@pytest.mark.parametrize("split,fmt", FORMATS)
@pytest.mark.parametrize("R,C", [(5, 256), (5, 300), (1, 256), (1, 300)])
def test_row_apply_loop_on_integers(dev, split, fmt, R, C):
    """C = 256 is the smallest shape of row_apply16x_kernel (with R >= 4); 300 is no multiple of the key tile (64 / 32)"""
    got, want = _apply_case(dev, split, fmt, R, C)
    assert torch.equal(got, want)


def test_f16x3_row_apply_with_nonzero_lo_planes(dev):
    got, want = _apply_case(dev, 3, 1, 5, 300, True)
    assert rel_l2(got, want) < TOL_F16X3
