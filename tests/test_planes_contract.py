"""CPU tests of tests/planes_contract.py: the reference split is what the contract says it is, the unmutated reference passes
every checker on the whole bit sweep, and every faulty writer (a)-(f) is reported -- on 100 % of the near-tie elements it
changes -- by the checker that is meant to see it.  Runs under -m "not gpu"."""
import numpy as np
import pytest
import torch

import planes_contract as pc

FMTS = [0, 1]


@pytest.fixture(scope="module")
def sweep():
    return pc.bit_sweep()


def test_the_sweep_has_every_upper_half_and_every_edge(sweep):
    assert sweep.numel() == 65536 * 11 == 720896
    w = sweep.view(torch.int32)
    assert len(torch.unique(w)) == 720896
    for v in (0.0, float("inf"), 2.0 ** -24, 2.0 ** -25, 2.0 ** -14):
        assert bool((sweep == v).any()), v
    e = pc.edge_values()
    for v in (65504.0, 65519.99609375, 65520.0, -65520.0, 2.0 ** -25):
        assert bool((e == v).any()), v
    assert bool(((w == -2 ** 31)).any()) and bool(torch.isnan(sweep).any())            # -0.0, NaN
    assert bool(((sweep > 65520.0) & (sweep < 65536.0)).any())                          # finite in fp32, inf in fp16
    for fmt in (0, 1):
        hi, lo = pc.split_reference(e, fmt)
        assert pc.check_near(hi, lo, e, fmt).count == 0 and pc.check_pair_shape(hi, lo, fmt).count == 0


def test_round16_bf16_is_round_to_nearest_even_by_integer_arithmetic(sweep):
    """torch's CPU cast against the textbook integer formula, so that the 'independent reference' is not taken on trust."""
    w = sweep.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    want = ((w + 0x7FFF + ((w >> 16) & 1)) >> 16) & 0xFFFF
    got = pc.bits(pc.round16(sweep, 0)).to(torch.int64) & 0xFFFF
    ok = torch.isnan(sweep) | (got == want)
    assert bool(ok.all())
    assert bool(torch.isnan(pc.round16(sweep, 0).float())[torch.isnan(sweep)].all())


def test_round16_fp16_keeps_subnormals_ties_to_even_and_overflows_at_65520():
    x = torch.tensor([2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 0.75 * 2.0 ** -24, 65519.996, 65520.0, -0.0,
                      1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], dtype=torch.float32)
    want = [2.0 ** -24, 0.0, 2.0 ** -23, 2.0 ** -23, 2.0 ** -24, 65504.0, float("inf"), -0.0, 1.0, 1.0 + 2.0 ** -9]
    got = pc.round16(x, 1).double()
    assert got.tolist() == want
    assert int(pc.bits(pc.round16(x, 1))[7]) == -0x8000                               # the sign of zero survives


@pytest.mark.parametrize("fmt", FMTS)
def test_x_minus_hi_is_exact_in_fp32_wherever_hi_is_finite(sweep, fmt):
    hi = pc.round16(sweep, fmt)
    fin = torch.isfinite(sweep) & torch.isfinite(hi.float())
    d32 = (sweep - hi.float()).double()
    d64 = sweep.double() - hi.double()
    assert bool((d32 == d64)[fin].all())
    assert int(fin.sum()) == (718074 if fmt == 0 else 402686)


@pytest.mark.parametrize("fmt", FMTS)
def test_the_reference_passes_every_checker_on_the_whole_sweep(sweep, fmt):
    hi, lo = pc.split_reference(sweep, fmt)
    for rep in (pc.check_exact(hi, lo, sweep, fmt), pc.check_exact(hi, None, sweep, fmt), pc.check_near(hi, lo, sweep, fmt),
                pc.check_near(hi, None, sweep, fmt), pc.check_pair_shape(hi, lo, fmt)):
        assert rep.total == sweep.numel()
        assert rep.count == 0, str(rep)
    # the pair bar has the margin the derivation promises: worst ratio to 2^-2m |x| at most 1/2
    xd = sweep.double()
    fin = torch.isfinite(hi.double()) & (xd != 0)
    err = (hi.double() + lo.double() - xd).abs()
    big = fin & (err > pc.subnormal_step(fmt) / 2)
    assert float((err / (xd.abs() * 2.0 ** (-2 * pc.MBITS[fmt])))[big].max()) <= 0.5


@pytest.mark.parametrize("fmt", FMTS)
def test_the_reference_passes_on_near_tie_data_in_every_regime(fmt):
    for scale in (1.0, 2.0 ** -12, 2.0 ** -18) + ((2.0 ** -120,) if fmt == 0 else ()):
        x, d = pc.near_tie(f"ref.{fmt}", (50000,), fmt, scale, with_offsets=True)
        assert 5000 < int((d != 99).sum()) < 7500                                 # about one element in eight
        hi, lo = pc.split_reference(x, fmt)
        for rep in (pc.check_near(hi, lo, x, fmt), pc.check_near(hi, None, x, fmt), pc.check_pair_shape(hi, lo, fmt)):
            assert rep.count == 0, str(rep)
    if fmt == 1:            # the small regimes really are subnormal: lo entirely, hi partly
        x = pc.near_tie("ref.sub", (50000,), 1, 2.0 ** -18)
        hi, lo = pc.split_reference(x, 1)
        assert float(lo.double().abs().max()) < 2.0 ** -14 and bool((hi.double().abs() < 2.0 ** -14).any())


def _near_tie_inputs(fmt, scale=1.0):
    x, d = pc.near_tie(f"mut.{fmt}.{scale}", (200000,), fmt, scale, with_offsets=True)
    return x.reshape(-1), d.reshape(-1)


@pytest.mark.parametrize("fmt", FMTS)
def test_mutant_a_truncated_hi_is_reported(fmt):
    x, d = _near_tie_inputs(fmt)
    hb, lb, changed = pc.mutant_truncate_hi(x, fmt)
    tie = changed & (d != 99)
    assert int(tie.sum()) > 5000
    assert bool(pc.check_exact(hb, None, x, fmt).mask[changed].all())
    assert bool(pc.check_near(hb, lb, x, fmt).mask[tie].all())                   # the pair is off by a whole 16-bit ulp
    # hi alone: a truncation is visible from the point where it costs more than the one fp32 ulp the twin may differ by
    beyond = tie & (d.abs() == 2)
    rep = pc.check_near(hb, None, x, fmt)
    assert int(beyond.sum()) > 1000 and bool(rep.mask[beyond].all())
    assert not bool(rep.mask[~changed].any())
    assert "excess" in str(rep) and len(rep.worst) == 8


@pytest.mark.parametrize("fmt", FMTS)
def test_mutant_b_lo_against_the_other_neighbour_is_reported_by_the_pair_bar_and_not_by_the_shape(fmt):
    x, d = _near_tie_inputs(fmt)
    hb, lb, changed = pc.mutant_lo_against_other_neighbour(x, fmt)
    tie = changed & (d != 99)
    assert int(tie.sum()) > 15000
    assert bool(pc.check_near(hb, lb, x, fmt).mask[tie].all())
    assert bool(pc.check_exact(hb, lb, x, fmt).mask[changed].all())
    # the warning of the module docstring: lo's own rounding lands on half an ulp, so the shape check sees few of them
    assert int(pc.check_pair_shape(hb, lb, fmt).mask[tie].sum()) < 0.5 * int(tie.sum())
    # and on the bit sweep's ties
    s = pc.bit_sweep()
    hb, lb, changed = pc.mutant_lo_against_other_neighbour(s, fmt)
    low = 0x8000 if fmt == 0 else 0x1000
    span = 0xFFFF if fmt == 0 else 0x1FFF
    # (in the format's lowest binade half an ulp is half the subnormal step: lo cannot hold it, both pairs sit AT the floor)
    at_tie = changed & (((s.view(torch.int32) & span) - low).abs() <= 1) & (s.abs() >= 2.0 ** (pc.EMIN[fmt] + 1))
    assert int(at_tie.sum()) > 10000 and bool(pc.check_near(hb, lb, s, fmt).mask[at_tie].all())


def test_mutant_c_flushed_lo_is_reported():
    # (at 2^-18 hi is subnormal itself and x - hi is at most half the subnormal step: lo is zero throughout, nothing to flush)
    assert not bool(pc.mutant_flush_lo(_near_tie_inputs(1, 2.0 ** -18)[0], 1)[2].any())
    for scale in (2.0 ** -6, 2.0 ** -12):
        x, d = _near_tie_inputs(1, scale)
        hb, lb, changed = pc.mutant_flush_lo(x, 1)
        assert int(changed.sum()) > 50000                                         # the lo plane is subnormal or zero there
        assert bool(pc.check_exact(hb, lb, x, 1).mask[changed].all())
        # check_near: wherever the lost lo is worth more than the floor plus the one fp32 ulp the twin may differ by (a lost
        # 2^-25 + 1 fp32 ulp is within the contract of a site whose x is only known to that ulp)
        lost = (x.double() - pc.values(hb, 1)).abs()
        seen = changed & (lost > 2.0 ** -25 + pc.ulp32(x))
        assert int(seen.sum()) > 0.95 * int(changed.sum())
        assert bool(pc.check_near(hb, lb, x, 1).mask[seen].all())


def test_mutant_d_flushed_hi_is_reported():
    x, d = _near_tie_inputs(1, 2.0 ** -18)
    hb, lb, changed = pc.mutant_flush_hi(x, 1)
    assert int(changed.sum()) > 100000
    assert bool(pc.check_near(hb, lb, x, 1).mask[changed].all())
    assert bool(pc.check_exact(hb, None, x, 1).mask[changed].all())
    far = changed & (x.abs() > 2.0 ** -24)                # hi alone: beyond the twin's one fp32 ulp around the 0 | 2^-24 tie
    assert bool(pc.check_near(hb, None, x, 1).mask[far].all())
    # bf16: subnormal results exist on the bit sweep only
    s = pc.bit_sweep()
    hb, lb, changed = pc.mutant_flush_hi(s, 0)
    assert int(changed.sum()) > 1000 and bool(pc.check_exact(hb, None, s, 0).mask[changed].all())


@pytest.mark.parametrize("fmt", FMTS)
def test_mutant_e_ties_away_from_zero_is_reported_by_the_exact_check_only(fmt):
    x, d = _near_tie_inputs(fmt)
    hb, lb, changed = pc.mutant_ties_away(x, fmt)
    assert bool(((d[changed] == 0) | (d[changed] == 99)).all()) and int(changed.sum()) > 1000    # exact ties, even neighbour below
    assert bool(pc.check_exact(hb, lb, x, fmt).mask[changed].all())
    assert bool(pc.check_exact(hb, None, x, fmt).mask[changed].all())
    # both neighbours of an exact tie are nearest: the numeric bars cannot and must not tell them apart
    assert pc.check_near(hb, lb, x, fmt).count == 0 and pc.check_pair_shape(hb, lb, fmt).count == 0


@pytest.mark.parametrize("fmt", FMTS)
def test_mutant_f_lost_sign_of_zero_is_reported_by_the_exact_check_only(fmt, sweep):
    hb, lb, changed = pc.mutant_drop_zero_sign(sweep, fmt)
    assert int(changed.sum()) > 100
    assert bool(pc.check_exact(hb, lb, sweep, fmt).mask[changed].all())
    assert pc.check_near(hb, lb, sweep, fmt).count == 0


@pytest.mark.parametrize("fmt", FMTS)
def test_non_finite_inputs_ask_for_non_finite_planes(fmt):
    x = torch.tensor([float("nan"), float("inf"), -float("inf"), 3.0e38 if fmt == 0 else 70000.0, 1.0], dtype=torch.float32)
    if fmt == 0:
        x[3] = torch.tensor([0x7F7FFFFF], dtype=torch.int32).view(torch.float32)[0]          # rounds up to inf in bf16
    hi, lo = pc.split_reference(x, fmt)
    assert pc.check_near(hi, lo, x, fmt).count == 0 and pc.check_exact(hi, lo, x, fmt).count == 0
    bad = pc.bits(hi).clone()
    bad[:4] = pc.bits(pc.round16(torch.tensor([1.0, 2.0, 3.0, 4.0]), fmt))                   # finite where non-finite is due
    assert pc.check_near(bad, None, x, fmt).mask.tolist() == [True, True, True, True, False]
    inf_for_nan = pc.bits(hi).clone()
    inf_for_nan[0] = pc.bits(hi)[1]
    assert pc.check_near(inf_for_nan, None, x, fmt).mask.tolist() == [True, False, False, False, False]
    assert pc.check_exact(inf_for_nan, None, x, fmt).mask.tolist() == [True, False, False, False, False]
    # a finite x with a non-finite plane is a violation too
    one = torch.ones(2)
    assert pc.check_near(pc.bits(hi)[1:3], None, one, fmt).count == 2
    assert pc.check_pair_shape(pc.bits(pc.round16(one, fmt)), pc.bits(hi)[1:3], fmt).count == 2


def test_ulps():
    assert pc.ulp16(torch.tensor([1.0, 1.5, 2.0, 0.0, 2.0 ** -14, 2.0 ** -20, 65504.0]), 1).tolist() == \
        [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 32.0]
    assert pc.ulp16(torch.tensor([1.0, 0.0, 3.0]), 0).tolist() == [2.0 ** -7, 2.0 ** -133, 2.0 ** -6]
    assert pc.ulp32(torch.tensor([1.0, 0.0, -4.0])).tolist() == [2.0 ** -23, 2.0 ** -149, 2.0 ** -21]
    assert np.isinf(pc.ulp16(torch.tensor([float("inf")]), 1).item())
