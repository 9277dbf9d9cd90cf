"""The exact-fp32 128x128x32 tile kernels (csrc/mma_core.h: gemm_f32.hip, row_attn.hip) in every regime of their K loop, on
small-integer operands.  The fp32 twin of tests/test_gpu_mma16_core.py.

GEMM operands are integers in [-8, 8], asymmetric in every index: |A W^T| <= 1749 at K = 224 (<= 3342 at K = 768), every product
and every partial sum is an integer far below 2^24, so the output must EQUAL the fp64 matmul of the same integers whatever the
summation order, the tile form or the block order -- no summation order is modelled here.  Scales and non-zero row factors are
powers of two, so every epilogue stays exact as well; assertions are torch.equal over the whole output.  The only tolerances:
1e-5 (centred squares of the row partial sums, test_residual_gemm_leaves_the_row_sums_of_what_it_stores), 3e-6 / 1e-4 (FOLD = 1,
where rsqrt is not exact: test_layernorm_folded_into_the_gemm) and the measured GELU bar (4 x YARD, below).

pipelined_kloop with DEPTH = 1 runs (steady pairs: `kt + 2 + DEPTH < nk`; peeled tail: `kt < nk`, a second step if `kt + 1 < nk`):

    nk             1   2   3   4   5   6   7
    steady pairs   0   0   0   1   1   2   2
    tail tiles     1   2   3   2   3   2   3

    kernel                       nk                         cases
    gemm_f32_kernel<NT = 2, 1>   K / 32                     K 32 .. 224 (nk 1 .. 7); "gemm_tile" 1 / 2 / 0; M 1 / 128 / 129 / 300 (ragged
                                                            last row panel), N 128 / 384; "gemm_group" 3 on the ragged shapes
    gemm_f32_mixed_kernel        K / 32                     "gemm_tile" 3 at (4000, 2304): 576 tiles, and (12837, 768): 606 tiles, 512 of
                                                            them full each (tile_plan's can_mix, restated and asserted here)
    every epilogue               K / 32                     M 300, N 384 at nk 1 .. 7 under both uniform tiles; the mixed shapes at
                                                            K 160 (nk 5: one steady pair, odd tail).  bias + column scale, residual
                                                            (in place too), zero_rows (always full tiles: launch_gemm), the per-row
                                                            factor, residual + row sums, folded LayerNorm with given statistics
                                                            (FOLD = 2) and self-summed (FOLD = 1), lda / ldc / ldr > the width, GELU
    row_logits_kernel            2 x rows of a split        R 1 / 2 / 3 / 5 / 9 / 17: splits of 1, 2, 3 and >= 4 rows, and of 9 and 17
                                                            rows at one tile and one head (the accumulator fold at a chain boundary,
                                                            `done % 16 == 0`, besides `done == nk`); C 65 / 128 / 130, H 1 / 2;
                                                            C 20 / 64 with "row_narrow" 0; row chunks of 9 (nk 18 and 16)
    row_logits_narrow_kernel     rows of a split            C 20 / 64 with "row_narrow" 1
    row_apply_kernel<ALIGNED>    ceil(C / 32)               C 20, 33 ("row_narrow" 0), 65, 100, 128, 130, 160, 190, 200, 224: nk 1 .. 7
                                                            (190 is the one with nk = 6), C % 4 == 0 and != 0; R 1 / 2 / 5
    row_apply_narrow_kernel      key groups of 8            C 20 / 33 with "row_narrow" 1

GELU (ACT_GELU_ERF with scale 2^-4 on every column: pre-activations v are exact multiples of 1/16).  |v| >= 6: erf rounds to +-1
in fp32 and the result must EQUAL max(v, 0) (by value: -0.0 is 0).  |v| < 6: the bar is measured, not chosen: YARD = the largest
|torch CPU fp32 gelu - fp64 gelu| over the same pre-activations (5.7e-7 over all multiples of 1/16 in (-6, 6)), and the device,
which evaluates another erf formula (Abramowitz-Stegun, one v_rcp and one v_exp), gets 4 x YARD.  Both figures are printed
(measured on an MI355X at every case: YARD 5.695e-7, device 3.831e-7).
"""
import contextlib

import numpy as np
import pytest
import torch

from conftest import rel_l2

gpu = pytest.mark.gpu

KS = (32, 64, 96, 128, 160, 192, 224)        # nk = 1 .. 7
K_STEADY = 160                               # nk = 5 at the mixed shapes: one steady pair, three peeled tiles
MIXED_SHAPES = [(4000, 2304), (12837, 768)]
# (gemm_tile, M, N, K values): where every epilogue is held to the integer truth
EPILOGUE_CASES = [(1, 300, 384, KS), (2, 300, 384, KS), (3, 4000, 2304, (K_STEADY,)), (3, 12837, 768, (K_STEADY,))]
EPILOGUE_IDS = ["full-300x384", "half-300x384", "mixed-4000x2304", "mixed-12837x768"]
TOL_CENTRED = 1e-5                           # test_residual_gemm_leaves_the_row_sums_of_what_it_stores
TOL_FOLD1_REL, TOL_FOLD1_MAX = 3e-6, 1e-4    # test_layernorm_folded_into_the_gemm
LN_EPS = 1e-5

LOGITS_R = (1, 2, 3, 5, 9, 17)
LOGITS_CH = [(65, 1), (65, 2), (128, 1), (128, 2), (130, 1), (130, 2)]
LOGITS_NARROW_CH = [(20, 1), (20, 2), (64, 1), (64, 2)]
APPLY_C = (20, 33, 65, 100, 128, 130, 160, 190, 200, 224)
APPLY_R = (1, 2, 5)


# ------------------------------------------------------------------------------------------------ host restatements (no GPU)
def _kloop_regime(nk, depth=1):
    """(steady pairs, peeled tail tiles) of pipelined_kloop: its two loop conditions, restated"""
    kt = pairs = tail = 0
    while kt + 2 + depth < nk:
        pairs += 1
        kt += 2
    while kt < nk:
        tail += 2 if kt + 1 < nk else 1
        kt += 2
    return pairs, tail


def test_k_values_cover_every_regime_of_the_pipelined_loop():
    table = {1: (0, 1), 2: (0, 2), 3: (0, 3), 4: (1, 2), 5: (1, 3), 6: (2, 2), 7: (2, 3)}
    assert [K // 32 for K in KS] == sorted(table)
    for nk, want in table.items():
        assert _kloop_regime(nk) == want, nk
        assert 2 * want[0] + want[1] == nk
    assert _kloop_regime(K_STEADY // 32)[0] >= 1
    assert {-(-C // 32) for C in APPLY_C} == set(table)                 # row_apply: nk = ceil(C / 32)
    assert {C % 4 == 0 for C in APPLY_C if C > 64} == {True, False}     # both ALIGNED instances of the tile kernel


def _mixed_full_blocks(M, N, group=0):
    """tile_plan's can_mix (csrc/gemm_f32.hip), restated: the block ids that are full tiles, 0 where tiles cannot be mixed"""
    mp, nb = -(-M // 128), N // 128
    tiles = mp * nb
    full = tiles // 512 * 512
    common = 8 * (mp // 8) * nb
    while full > common:
        full -= 512
    return full if 0 < full < tiles and tiles > 512 and group <= 0 else 0


def test_mixed_shapes_take_the_mixed_kernel():
    """"gemm_tile" = 3 falls back to full tiles where can_mix fails: a later change of the plan, or of the knob the rule reads,
    must not silently untest gemm_f32_mixed_kernel"""
    from rnamsm import _lib
    assert _lib.load().rnamsm_get_param(b"gemm_group") == 0
    assert [-(-M // 128) * (N // 128) for M, N in MIXED_SHAPES] == [576, 606]
    for M, N in MIXED_SHAPES:
        assert _mixed_full_blocks(M, N) == 512 and M % 128 != 0, (M, N)
    assert _mixed_full_blocks(300, 384) == 0 and _mixed_full_blocks(4000, 2304, group=3) == 0


def _rows_of_splits(R, C, H):
    from rnamsm import _lib
    n = _lib.load().rnamsm_row_logits_nsplit(R, C, H)
    rps = -(-R // n)
    return [min(R, (s + 1) * rps) - s * rps for s in range(n)]


def test_logits_cases_cover_every_loop_regime():
    """1, 2, 3 and >= 4 alignment rows per split (nk = 2, 4, 6, >= 8) at every (C, H), and a split of more than 8 rows -- the fold
    of the accumulators at a chain boundary with tiles still to come -- where one tile and one head leave the rows unsplit: a later
    change of the row split cannot silently untest a regime"""
    for C, H in LOGITS_CH + LOGITS_NARROW_CH:
        rows = {r for R in LOGITS_R for r in _rows_of_splits(R, C, H)}
        assert {1, 2, 3} <= rows and any(r >= 4 for r in rows), (C, H, sorted(rows))
    for C, H in [(128, 1), (64, 1)]:
        assert any(r > 8 for R in LOGITS_R for r in _rows_of_splits(R, C, H)), (C, H)


# ------------------------------------------------------------------------------------------------ operands and truths
def _ints_host(shape, seed, half=8):
    """Integers in [-half, half], asymmetric in every index (tests/test_gpu_mma16_core.py's pattern), fp32 on the host.
    7 + 2 seed must not be a multiple of 2 half + 1."""
    assert (7 + 2 * seed) % (2 * half + 1) != 0
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.int64)
    x = ((i * (7 + 2 * seed) + (i // 191) * 3 + seed) % (2 * half + 1)) - half
    return torch.from_numpy(x.astype(np.float32)).view(*shape)


SEED_A, SEED_W, SEED_BIAS, SEED_RES, SEED_C, SEED_D = 1, 2, 3, 4, 6, 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rnamsm import _lib
    _lib.load()
    return torch.device("cuda:0")


class _Bank:
    """Operands and truths, made once per shape and left unchanged (tests clone what they write into)"""

    def __init__(self, dev):
        self.dev, self._ints, self._gemm = dev, {}, {}

    def ints(self, shape, seed, half=8):
        key = (tuple(shape), seed, half)
        if key not in self._ints:
            self._ints[key] = _ints_host(shape, seed, half).to(self.dev)
        return self._ints[key]

    def gemm(self, M, N, K):
        """(a [M, K], w [N, K], fp64 a w^T) on the device; the matmul is the host's, in fp64"""
        key = (M, N, K)
        if key not in self._gemm:
            a, w = _ints_host((M, K), SEED_A), _ints_host((N, K), SEED_W)
            acc = a.double() @ w.double().t()
            assert float(acc.abs().max()) < 2 ** 24 / 64
            self._gemm[key] = (a.to(self.dev), w.to(self.dev), acc.to(self.dev))
        return self._gemm[key]


@pytest.fixture(scope="module")
def bank(dev):
    b = _Bank(dev)
    yield b
    b._ints.clear()
    b._gemm.clear()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def _knobs(**values):
    from rnamsm import ops
    before = {k: ops.get_param(k) for k in values}
    try:
        for k, v in values.items():
            ops.set_param(k, v)
        yield
    finally:
        for k, v in before.items():
            ops.set_param(k, v)


def _same(got, want):
    """the whole output EQUALS the fp64 truth (by value: -0.0 == 0.0)"""
    return got.shape == want.shape and torch.equal(got.double(), want)


# ------------------------------------------------------------------------------------------------ 1, 2: K-loop regimes x tile forms
@gpu
@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("M", [1, 128, 129, 300])
@pytest.mark.parametrize("tile", [1, 2, 0])
def test_gemm_loop_regimes_on_integers(dev, bank, tile, M, N):
    """gemm_f32_kernel, 128x128 ("gemm_tile" 1) and 128x64 (2) tiles and the plan's own choice (0), nk = 1 .. 7"""
    from rnamsm import ops
    with _knobs(gemm_tile=tile):
        for K in KS:
            a, w, acc = bank.gemm(M, N, K)
            assert _same(ops.linear(a, w), acc), K


@gpu
@pytest.mark.parametrize("M,N", MIXED_SHAPES)
def test_mixed_tile_gemm_loop_regimes_on_integers(dev, bank, M, N):
    """gemm_f32_mixed_kernel ("gemm_tile" 3: 512 full tiles, the other tile positions as 128x64 halves, ragged last row panel) and
    the plan's own choice at the same shapes, nk = 1 .. 7"""
    from rnamsm import ops
    assert _mixed_full_blocks(M, N, ops.get_param("gemm_group")) == 512
    for tile in (3, 0):
        with _knobs(gemm_tile=tile):
            for K in KS:
                a, w, acc = bank.gemm(M, N, K)
                assert _same(ops.linear(a, w), acc), (tile, K)


@gpu
@pytest.mark.parametrize("tile", [1, 2])
def test_gemm_block_order_knob_on_integers(dev, bank, tile):
    """"gemm_group" = 3 (XCD-aware order in groups of three row panels; the default deals these launches flat) on the ragged shapes"""
    from rnamsm import ops
    with _knobs(gemm_tile=tile, gemm_group=3):
        for M, N, ks in ((129, 128, KS), (300, 384, KS), (4000, 2304, (K_STEADY,))):
            for K in ks:
                a, w, acc = bank.gemm(M, N, K)
                assert _same(ops.linear(a, w), acc), (M, N, K)


# ------------------------------------------------------------------------------------------------ 3: every epilogue and entry point
def _each(bank, case):
    tile, M, N, ks = case
    for K in ks:
        yield (K,) + bank.gemm(M, N, K)


epilogues = pytest.mark.parametrize("case", EPILOGUE_CASES, ids=EPILOGUE_IDS)


@gpu
@epilogues
def test_bias_and_column_scale_on_integers(dev, bank, case):
    """scale_cols 64 lies inside a 128-wide tile and on the edge of a 64-wide one"""
    from rnamsm import ops
    N = case[2]
    bias = bank.ints((N,), SEED_BIAS)
    with _knobs(gemm_tile=case[0]):
        for K, a, w, acc in _each(bank, case):
            for sc in (0, 64, N):
                want = acc + bias.double()
                want[:, :sc] *= 0.25
                assert _same(ops.linear(a, w, bias, scale=0.25, scale_cols=sc), want), (K, sc)


@gpu
@epilogues
def test_residual_on_integers(dev, bank, case):
    from rnamsm import ops
    _, M, N, _ = case
    bias, res = bank.ints((N,), SEED_BIAS), bank.ints((M, N), SEED_RES)
    with _knobs(gemm_tile=case[0]):
        for K, a, w, acc in _each(bank, case):
            want = acc + bias.double() + res.double()
            assert _same(ops.linear(a, w, bias, residual=res), want), K
            x = res.clone()                                               # in place, as the forward runs it
            assert ops.linear(a, w, bias, residual=x, out=x).data_ptr() == x.data_ptr() and _same(x, want), K


def _flagged_rows(M):
    last = 128 * ((M - 1) // 128)                                         # first row of the last (ragged) panel
    return sorted({r for r in (127, 128, last - 1, last, M - 1) if 0 <= r < M})


@gpu
@epilogues
def test_zero_rows_on_integers(dev, bank, case):
    """Flagged rows on both sides of a panel edge, and the last row: their scaled columns are 0, nothing else is touched"""
    from rnamsm import ops
    _, M, N, _ = case
    bias = bank.ints((N,), SEED_BIAS)
    rows = _flagged_rows(M)
    assert M - 1 in rows and 127 in rows and 128 in rows
    mask = torch.zeros(M, dtype=torch.uint8, device=dev)
    mask[rows] = 1
    with _knobs(gemm_tile=case[0]):
        for K, a, w, acc in _each(bank, case):
            for sc in (64, N):
                want = acc + bias.double()
                want[:, :sc] *= 0.25
                want[rows, :sc] = 0.0
                assert _same(ops.linear(a, w, bias, scale=0.25, scale_cols=sc, zero_rows=mask), want), (K, sc)


@gpu
@epilogues
def test_row_scaled_on_integers(dev, bank, case):
    from rnamsm import ops
    _, M, N, _ = case
    bias = bank.ints((N,), SEED_BIAS)
    r = torch.arange(M, device=dev)
    factor = torch.tensor([0.0, 0.5, 1.0, 2.0], device=dev)[(3 * r + r // 5) % 4].contiguous()
    assert len(set(factor[[127, 128, M - 1]].tolist())) > 1
    with _knobs(gemm_tile=case[0]):
        for K, a, w, acc in _each(bank, case):
            for sc in (64, N):
                want = acc + bias.double()
                want[:, :sc] *= 0.25 * factor.double()[:, None]
                assert _same(ops.linear_row_scaled(a, w, bias, factor, scale=0.25, scale_cols=sc), want), (K, sc)


def _residual_stats_into(a, w, bias, x, partials):
    """x += a w^T + bias in place, the row sums into slabs of partials.shape[1] >= M rows (the C entry point itself)"""
    from rnamsm import _lib
    (M, K), N = a.shape, w.shape[0]
    _lib.check(_lib.load().rnamsm_gemm_residual_stats(a.data_ptr(), K, w.data_ptr(), bias.data_ptr(), x.data_ptr(), N, x.data_ptr(), N,
                                                      M, N, K, partials.data_ptr(), partials.shape[1], _lib.F32,
                                                      torch.cuda.current_stream().cuda_stream))


@gpu
@epilogues
def test_residual_stats_on_integers(dev, bank, case):
    """rnamsm_gemm_residual_stats: the output, and component 0 of row_partials -- 32 integers per slab, exact -- EQUAL the truth;
    component 1 (centred squares) at the bar of test_residual_gemm_leaves_the_row_sums_of_what_it_stores; rows >= M of a buffer
    with partials_ld > M keep their fill"""
    from rnamsm import ops
    _, M, N, _ = case
    bias, res = bank.ints((N,), SEED_BIAS), bank.ints((M, N), SEED_RES)
    pld = M + 5
    with _knobs(gemm_tile=case[0]):
        for K, a, w, acc in _each(bank, case):
            want = acc + bias.double() + res.double()
            slabs = want.view(M, N // 32, 32).transpose(0, 1)
            sums, centred = slabs.sum(-1), ((slabs - slabs.mean(-1, keepdim=True)) ** 2).sum(-1)
            out, part = ops.linear_residual_stats(a, w, bias, res)
            assert _same(out, want) and part.shape == (N // 32, M, 2), K
            assert _same(part[..., 0], sums), K
            assert rel_l2(part[..., 1].cpu(), centred.cpu()) < TOL_CENTRED, K
            x = res.clone()                                               # in place, slabs of pld > M rows
            wide = torch.full((N // 32, pld, 2), float("nan"), device=dev)
            _residual_stats_into(a, w, bias, x, wide)
            assert _same(x, want) and _same(wide[:, :M, 0], sums), K
            assert rel_l2(wide[:, :M, 1].cpu(), centred.cpu()) < TOL_CENTRED, K
            assert bool(torch.isnan(wide[:, M:]).all()), K


def _row_stats(T, dev):
    """(mean, rstd) per row: mean in {-2 .. 2}, rstd in {0.5, 1, 2}, neighbours differ"""
    r = torch.arange(T, device=dev)
    mean = ((3 * r + r // 7) % 5 - 2).float()
    rstd = torch.tensor([0.5, 1.0, 2.0], device=dev)[(r + r // 11) % 3]
    return torch.stack([mean, rstd], 1).contiguous()


@gpu
@epilogues
def test_lnfold_with_given_statistics_on_integers(dev, bank, case):
    """FOLD = 2 with integer c, d and power-of-two rstd: rstd (acc - mean c) + d is exact, and a statistic read from the wrong
    row changes an integer.  Also with `stats` covering more rows than x (the first rows of a longer stream)."""
    from rnamsm import ops
    _, M, N, _ = case
    c, d = bank.ints((N,), SEED_C), bank.ints((N,), SEED_D)
    longer = _row_stats(M + 7, dev)
    own = longer[:M].contiguous()
    assert not torch.equal(own[1:], own[:-1])
    mean, rstd = own[:, 0].double()[:, None], own[:, 1].double()[:, None]
    with _knobs(gemm_tile=case[0]):
        for K, a, w, acc in _each(bank, case):
            want = rstd * (acc - mean * c.double()) + d.double()
            for stats in (own, longer):
                assert _same(ops.linear_lnfold(a, w, c, d, stats), want), (K, stats.shape[0])
            want[:, :64] *= 0.25
            assert _same(ops.linear_lnfold(a, w, c, d, longer, scale=0.25, scale_cols=64), want), K


@gpu
@epilogues
def test_lnfold_summing_its_own_statistics(dev, bank, case):
    """FOLD = 1: x and x^2 are summed where the K tiles are stored to LDS -- every tile exactly once, peeled tail included -- at
    nk = 1 .. 7.  rsqrt is not exact: fp64 at the bars of test_layernorm_folded_into_the_gemm."""
    from rnamsm import ops
    _, M, N, _ = case
    c, d = bank.ints((N,), SEED_C), bank.ints((N,), SEED_D)
    with _knobs(gemm_tile=case[0]):
        for K, a, w, acc in _each(bank, case):
            x = a.double()
            mean = x.mean(1, keepdim=True)
            rstd = torch.rsqrt(x.var(1, unbiased=False, keepdim=True) + LN_EPS)
            want = rstd * (acc - mean * c.double()) + d.double()
            got = ops.linear_lnfold(a, w, c, d, None, eps=LN_EPS)
            err = got.double() - want
            rel, mx = float(err.norm() / want.norm()), float(err.abs().max())
            assert rel < TOL_FOLD1_REL and mx < TOL_FOLD1_MAX * float(want.abs().max()), (K, rel, mx)


@gpu
@epilogues
def test_leading_dimensions_on_integers(dev, bank, case):
    """A as a view with lda > K inside a NaN-filled buffer; out and residual as views with ldc, ldr > N: the gap columns and one
    guard row behind the output keep their fill"""
    from rnamsm import ops
    _, M, N, _ = case
    FILL = -77.0
    bias, res = bank.ints((N,), SEED_BIAS), bank.ints((M, N), SEED_RES)
    rbuf = torch.full((M + 1, N + 12), float("nan"), device=dev)
    rbuf[:M, 8:8 + N] = res
    with _knobs(gemm_tile=case[0]):
        for K, a, w, acc in _each(bank, case):
            abuf = torch.full((M + 1, K + 12), float("nan"), device=dev)
            abuf[:M, 4:4 + K] = a
            av = abuf[:M, 4:4 + K]
            for residual in (None, rbuf[:M, 8:8 + N]):
                obuf = torch.full((M + 1, N + 8), FILL, device=dev)
                ops.linear(av, w, bias, residual=residual, out=obuf[:M, 4:4 + N])
                want = acc + bias.double() + (0 if residual is None else res.double())
                assert _same(obuf[:M, 4:4 + N], want), (K, residual is None)
                assert bool((obuf[:, :4] == FILL).all()) and bool((obuf[:, 4 + N:] == FILL).all()) and bool((obuf[M] == FILL).all()), K
            x = rbuf.clone()                                              # in place inside the wide buffer
            ops.linear(av, w, bias, residual=x[:M, 8:8 + N], out=x[:M, 8:8 + N])
            assert _same(x[:M, 8:8 + N], acc + bias.double() + res.double()), K
            assert bool(torch.isnan(x[:, :8]).all()) and bool(torch.isnan(x[:, 8 + N:]).all()) and bool(torch.isnan(x[M]).all()), K


# ------------------------------------------------------------------------------------------------ 4: GELU on exact pre-activations
@gpu
@epilogues
def test_gelu_on_exact_preactivations(dev, bank, case):
    from rnamsm import ops
    from rnamsm._lib import ACT_GELU_ERF
    gelu = torch.nn.functional.gelu
    N = case[2]
    bias = bank.ints((N,), SEED_BIAS)
    with _knobs(gemm_tile=case[0]):
        for K, a, w, acc in _each(bank, case):
            v = (acc + bias.double()) / 16.0                             # exact multiples of 1/16
            got = ops.linear(a, w, bias, act=ACT_GELU_ERF, scale=2.0 ** -4, scale_cols=N)
            big = v.abs() >= 6.0
            small = ~big
            assert bool(big.any()) and bool(small.any()), K
            vs = v[small].cpu()
            ref = gelu(vs)                                                # fp64, erf form
            yard = float((gelu(vs.float()).double() - ref).abs().max())   # what fp32 arithmetic costs the reference itself
            worst = float((got[small].cpu().double() - ref).abs().max())
            print(f"gelu {case[1]}x{N} tile {case[0]} K {K}: |v| < 6: {vs.numel()} entries, YARD {yard:.3e}, device max {worst:.3e}"
                  f" (bar {4 * yard:.3e}); |v| >= 6: {int(big.sum())} entries")
            assert torch.equal(got[big].double(), v[big].clamp_min(0.0)), K
            assert worst <= 4.0 * yard, (K, worst, yard)


# ------------------------------------------------------------------------------------------------ 5: fp32 row tile kernels
def _logits_case(bank, R, C, H, rows_per_chunk=0):
    """q / k in [-2, 2] as strided views of one fused buffer; -> (partial slabs, fp64 truth per slab), on the host"""
    from rnamsm import ops
    D = 64 * H
    qk = bank.ints((R * C, 2 * D), 1, half=2)
    partial, n = ops.row_logits(qk[:, :D], qk[:, D:], R, C, H, rows_per_chunk=rows_per_chunk)
    q, k = (t.cpu().double().view(R, C, H, 64) for t in (qk[:, :D], qk[:, D:]))
    rows = [rows_per_chunk] * n if rows_per_chunk else _rows_of_splits(R, C, H)
    assert partial.shape == (n, H, C, C) and len(rows) == n
    rps = rows[0]
    want = torch.stack([torch.einsum("rihd,rjhd->hij", q[s * rps:(s + 1) * rps], k[s * rps:(s + 1) * rps]) for s in range(n)])
    assert torch.equal(want.sum(0), torch.einsum("rihd,rjhd->hij", q, k))
    return partial.cpu().double(), want


@gpu
@pytest.mark.parametrize("C,H", LOGITS_CH)
def test_row_logits_loop_regimes_on_integers(dev, bank, C, H):
    """|q . k| <= 4 * 64 R <= 4352: exact in fp32, each slab against its own rows' contraction and their sum against the whole"""
    for R in LOGITS_R:
        got, want = _logits_case(bank, R, C, H)
        assert torch.equal(got, want) and torch.equal(got.sum(0), want.sum(0)), R


@gpu
@pytest.mark.parametrize("narrow", [0, 1])
@pytest.mark.parametrize("C,H", LOGITS_NARROW_CH)
def test_narrow_row_logits_on_integers(dev, bank, C, H, narrow):
    """C <= 64: the tile kernel ("row_narrow" 0) and row_logits_narrow_kernel (1), each held to the integer truth itself"""
    with _knobs(row_narrow=narrow):
        for R in LOGITS_R:
            got, want = _logits_case(bank, R, C, H)
            assert torch.equal(got, want) and torch.equal(got.sum(0), want.sum(0)), R


@gpu
@pytest.mark.parametrize("C,H,narrow", [(130, 2, 1), (20, 2, 0), (20, 2, 1)])
def test_row_logits_fold_at_a_chain_boundary_on_integers(dev, bank, C, H, narrow):
    """Row chunks of 9 over 17 rows: slabs of 9 rows (nk 18: the accumulators are folded at tile 16 and at the end) and of 8
    (nk 16: both at once), at shapes whose own split never leaves more than 8 rows together"""
    with _knobs(row_narrow=narrow):
        got, want = _logits_case(bank, 17, C, H, rows_per_chunk=9)
        assert got.shape[0] == 2 and torch.equal(got, want)


def _apply_case(bank, R, C):
    """"probabilities" and v in [-3, 3] (|P v| <= 9 C), v as a strided view; -> (context, fp64 truth) on the host"""
    from rnamsm import ops
    H, D = 2, 128
    p = bank.ints((H, C, C), 2, half=3)
    kv = bank.ints((R * C, 2 * D), 3, half=3)
    ctx = ops.row_apply(p, kv[:, D:], R, C, H)
    want = torch.einsum("hij,rjhd->rihd", p.cpu().double(), kv[:, D:].cpu().double().view(R, C, H, 64)).reshape(R * C, D)
    return ctx.cpu().double(), want


@gpu
@pytest.mark.parametrize("C", APPLY_C)
def test_row_apply_loop_regimes_on_integers(dev, bank, C):
    """row_apply_kernel at nk = ceil(C / 32) = 1 .. 7, keys that are no multiple of the tile, of 4 (ALIGNED false) or of neither;
    odd R leaves the last row pair half empty.  At C <= 64 the tile kernel needs "row_narrow" 0."""
    with _knobs(row_narrow=0):
        for R in APPLY_R:
            got, want = _apply_case(bank, R, C)
            assert torch.equal(got, want), R


@gpu
@pytest.mark.parametrize("C", [c for c in APPLY_C if c <= 64])
def test_narrow_row_apply_on_integers(dev, bank, C):
    from rnamsm import ops
    assert ops.get_param("row_narrow") == 1
    for R in APPLY_R:
        got, want = _apply_case(bank, R, C)
        assert torch.equal(got, want), R
