"""The per-element contract of a 16-bit plane pair, as host code (torch on the CPU; no GPU, no library).

A writer of planes turns an fp32 value x into hi = round16(x) and, in the pair mode, lo = round16(x - hi).  The fp32
subtraction x - hi is exact whenever hi is finite (tests/test_planes_contract.py verifies it on the whole bit sweep), so the
pair is a function of x alone and can be compared BIT FOR BIT with `split_reference`.

fmt 0 = bf16 (8 significand bits, fp32's exponent range), fmt 1 = fp16 (11 significand bits, subnormal step 2^-24).

Three checkers, strongest first:
  check_exact       hi, lo equal split_reference(x) bit for bit (signed zeros included; NaN compares as "is NaN").  For a
                    site whose own fp32 value x is observable (written by the same launch, or an input copied through).
  check_near        x32 comes from ANOTHER compilation of the kernel (its fp32-output twin) and may differ from the value
                    that was split by one fp32 ulp.  Every finite element:
                        |hi - x32|      <= ulp16(hi) / 2 + ulp32(x32)
                        |hi + lo - x32| <= max(2^-2m |x32|, floor) + ulp32(x32)        (pairs; m = 8 / 11)
                    floor = half the format's subnormal step (fp16: 2^-25 = 3e-8, the figure of csrc/half16.h).  Derived, not
                    measured: two roundings of m bits each leave 2^-2m relative, a subnormal lo leaves half its step.
  check_pair_shape  needs no x: |lo| <= ulp16(hi) / 2 and lo finite wherever hi is.  A NECESSARY condition only -- at a
                    near-tie lo's own rounding lands on exactly half an ulp and hides a hi that went to the wrong neighbour.
No checker skips a finite element.  An x whose reference hi is not finite (NaN, inf, |x| >= 65520 in fp16) is held to "hi is
non-finite, and NaN for NaN" instead of the numeric bars.
"""
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import torch

DTYPE = {0: torch.bfloat16, 1: torch.float16}
MBITS = {0: 8, 1: 11}            # significand bits, the implicit one included
EMIN = {0: -126, 1: -14}         # exponent of the smallest normal number
SWEEP_LOWER_HALVES = (0, 1, 0x0FFF, 0x1000, 0x1001, 0x1FFF, 0x2000, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def subnormal_step(fmt: int) -> float:
    return 2.0 ** (EMIN[fmt] - MBITS[fmt] + 1)


def round16(x: torch.Tensor, fmt: int) -> torch.Tensor:
    """The independent reference conversion: torch's CPU cast, round-to-nearest-even, subnormals kept."""
    assert x.dtype == torch.float32 and not x.is_cuda
    return x.to(DTYPE[fmt])


def split_reference(x: torch.Tensor, fmt: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(hi, lo) as tensors of the 16-bit dtype: hi = round16(x), lo = round16(x - hi) with the subtraction in fp32."""
    hi = round16(x, fmt)
    return hi, round16(x - hi.float(), fmt)


def bits(t: torch.Tensor) -> torch.Tensor:
    """A 16-bit float tensor (or int16 bits already) as flat int16 bits on the CPU."""
    t = t.detach().cpu().contiguous()
    return (t if t.dtype == torch.int16 else t.view(torch.int16)).reshape(-1)


def values(b: torch.Tensor, fmt: int) -> torch.Tensor:
    """int16 bits -> the float64 values they hold."""
    return bits(b).view(DTYPE[fmt]).double()


def _ulp(a: torch.Tensor, mbits: int, emin: int) -> torch.Tensor:
    """Spacing of a binary format with `mbits` significand bits at magnitude |a| (float64 in, float64 out); the subnormal
    step at and below the smallest normal number; inf / NaN where a is."""
    a = a.abs()
    _, e = torch.frexp(a)                                  # a = f * 2^e, f in [0.5, 1)
    e = torch.where(a == 0, torch.full_like(e, emin), e - 1).clamp(min=emin)
    u = torch.ldexp(torch.ones_like(a), e - (mbits - 1))
    return torch.where(torch.isfinite(a), u, a)


def ulp16(v: torch.Tensor, fmt: int) -> torch.Tensor:
    return _ulp(v.double(), MBITS[fmt], EMIN[fmt])


def ulp32(v: torch.Tensor) -> torch.Tensor:
    return _ulp(v.double(), 24, -126)


@dataclass
class Report:
    """Outcome of a checker: how many elements broke the contract, and the worst of them for the failure message."""
    name: str
    total: int
    count: int = 0
    mask: Optional[torch.Tensor] = None                       # bool [total]: the violating elements
    worst: List[tuple] = field(default_factory=list)          # (index, x bits, x, hi, lo, excess)

    def __bool__(self):
        return self.count == 0

    def __str__(self):
        head = f"{self.name}: {self.count} of {self.total} elements violate the contract"
        rows = [f"  [{i}] x=0x{xb:08x} ({x!r}) hi={h!r} lo={l!r} excess={ex:.3g}" for i, xb, x, h, l, ex in self.worst]
        return "\n".join([head] + rows)


def _report(name, viol, excess, x, hi_v, lo_v, keep=8) -> Report:
    n = int(viol.numel())
    rep = Report(name, n, int(viol.sum()), viol)
    if rep.count:
        score = torch.where(viol, torch.nan_to_num(excess, nan=float("inf"), posinf=float("inf")), torch.full_like(excess, -1.0))
        idx = torch.topk(score, min(keep, rep.count)).indices
        xb = None if x is None else x.contiguous().view(torch.int32)
        for i in idx.tolist():
            rep.worst.append((i, 0 if xb is None else int(xb[i]) & 0xFFFFFFFF, None if x is None else float(x[i]),
                              float(hi_v[i]), None if lo_v is None else float(lo_v[i]), float(excess[i])))
    return rep


def _flat32(x: torch.Tensor) -> torch.Tensor:
    x = x.detach().cpu().contiguous().reshape(-1)
    assert x.dtype == torch.float32
    return x


def _eq_bits_or_nan(got_bits, ref, fmt):
    got = got_bits.view(DTYPE[fmt])
    return torch.where(torch.isnan(ref), torch.isnan(got), got_bits == ref.view(torch.int16))


def check_exact(hi_bits, lo_bits, x, fmt: int) -> Report:
    """hi (and lo, unless None) equal split_reference(x) bit for bit; a NaN of the reference asks for any NaN."""
    x = _flat32(x)
    hb = bits(hi_bits)
    rh, rl = split_reference(x, fmt)
    assert hb.numel() == x.numel()
    ok = _eq_bits_or_nan(hb, rh, fmt)
    lv = None
    if lo_bits is not None:
        lb = bits(lo_bits)
        assert lb.numel() == x.numel()
        ok &= _eq_bits_or_nan(lb, rl, fmt)
        lv = values(lb, fmt)
    hv = values(hb, fmt)
    excess = torch.nan_to_num((hv + (lv if lv is not None else 0) - x.double()).abs(), nan=float("inf")) + 1e-300
    return _report(f"check_exact(fmt {fmt}{', pair' if lo_bits is not None else ''})", ~ok, excess, x, hv, lv)


def check_near(hi_bits, lo_bits, x32, fmt: int) -> Report:
    """The two derived bars of the module docstring against the fp32 twin's value x32."""
    x = _flat32(x32)
    xd = x.double()
    hv = values(hi_bits, fmt)
    assert hv.numel() == x.numel()
    ref_hi = round16(x, fmt).double()
    numeric = torch.isfinite(ref_hi)                           # x finite and inside the format's range
    slack = ulp32(x)
    bar_hi = ulp16(hv, fmt) / 2 + slack
    d_hi = (hv - xd).abs()
    viol = numeric & (~torch.isfinite(hv) | (d_hi > bar_hi))
    excess = torch.where(numeric, d_hi / bar_hi, torch.zeros_like(d_hi))
    # outside the numeric bars: hi is non-finite, and NaN for NaN
    viol |= ~numeric & (torch.isfinite(hv) | (torch.isnan(xd) & ~torch.isnan(hv)))
    lv = None
    if lo_bits is not None:
        lv = values(lo_bits, fmt)
        assert lv.numel() == x.numel()
        m = MBITS[fmt]
        bar = torch.clamp(xd.abs() * 2.0 ** (-2 * m), min=subnormal_step(fmt) / 2) + slack
        err = (hv + lv - xd).abs()
        viol |= numeric & (~torch.isfinite(lv) | (err > bar))
        excess = torch.maximum(excess, torch.where(numeric, err / bar, torch.zeros_like(err)))
    return _report(f"check_near(fmt {fmt}{', pair' if lo_bits is not None else ''})", viol, excess, x, hv, lv)


def check_pair_shape(hi_bits, lo_bits, fmt: int) -> Report:
    """|lo| <= ulp16(hi) / 2, and lo finite wherever hi is.  No x needed; necessary, not sufficient."""
    hv, lv = values(hi_bits, fmt), values(lo_bits, fmt)
    fin = torch.isfinite(hv)
    bar = ulp16(hv, fmt) / 2
    viol = fin & (~torch.isfinite(lv) | (lv.abs() > bar))
    excess = torch.where(fin, lv.abs() / bar, torch.zeros_like(lv))
    return _report(f"check_pair_shape(fmt {fmt})", viol, excess, None, hv, lv)


# ---------------------------------------------------------------------------------------------------- inputs
def bit_sweep() -> torch.Tensor:
    """All 65 536 upper halves of an fp32 word crossed with SWEEP_LOWER_HALVES: 720 896 values covering every exponent, both
    tie positions (bit 15 for bf16, bit 12 for fp16), subnormal results, the fp16 overflow edge, +-0, inf and NaN."""
    up = np.arange(65536, dtype=np.uint32) << np.uint32(16)
    words = (up[None, :] | np.asarray(SWEEP_LOWER_HALVES, dtype=np.uint32)[:, None]).reshape(-1)
    return torch.from_numpy(words.view(np.float32).copy())


def edge_values() -> torch.Tensor:
    """The fp16 overflow edge and the subnormal ties, which the sweep's eleven lower halves do not hit exactly: 65504 (largest
    fp16), the last fp32 below 65520 (rounds down), 65520 (rounds to inf), the 0 | 2^-24 tie and its neighbours; both signs."""
    v = np.array([65504.0, 65519.99609375, 65520.0, 65536.0, 2.0 ** -25, 2.0 ** -24, 2.0 ** -14, 2.0 ** -126, 2.0 ** -133, 2.0 ** -134],
                 dtype=np.float32)
    w = v.view(np.uint32)
    w = np.concatenate([w - 1, w, w + 1]).astype(np.uint32)
    x = w.view(np.float32)
    return torch.from_numpy(np.concatenate([x, -x]).copy())


def near_tie(key: str, shape, fmt: int, scale: float = 1.0, every: int = 8, with_offsets: bool = False):
    """Seeded standard-normal fp32 values (times `scale`, a power of two, so the mantissas stay) in which about one element
    in `every` has its low mantissa bits overwritten to lie d fp32 ulps from a tie of the 16-bit grid, d in -2..2 (a tie:
    low 16 bits 0x8000 for bf16, low 13 bits 0x1000 for fp16 -- for values inside the format's normal range).
    with_offsets: also returns d per element as int8, 99 where the element was left alone."""
    from rnamsm import synthetic
    n = int(np.prod(shape))
    v = synthetic.normal(key, 29, (n,)).astype(np.float32)
    w = v.view(np.uint32).copy()
    sel = synthetic._uniform_bits(np.uint64(0x9E37) ^ synthetic._fnv1a64(key), n, 3)
    pick = (sel % np.uint64(every)) == 0
    d = ((sel >> np.uint64(8)) % np.uint64(5)).astype(np.int64) - 2
    low = 16 if fmt == 0 else 13
    tie = np.int64(1) << (low - 1)
    w64 = w.astype(np.int64)
    w64 = np.where(pick, ((w64 >> low) << low) + tie + d, w64)
    x = w64.astype(np.uint32).view(np.float32) * np.float32(scale)
    t = torch.from_numpy(x.copy()).view(*shape)
    if with_offsets:
        return t, torch.from_numpy(np.where(pick, d, 99).astype(np.int8)).view(*shape)
    return t


# ---------------------------------------------------------------------------------------------------- mutants
# Faulty writers, applied to split_reference's output: each returns (hi_bits, lo_bits, changed mask).  For
# tests/test_planes_contract.py, which proves that the checkers report them.
def _mag_step(b: torch.Tensor, step: int) -> torch.Tensor:
    """Sign-magnitude bits moved `step` codes away from (+) or toward (-) zero."""
    i = b.to(torch.int32) & 0xFFFF
    out = (i & 0x8000) | (((i & 0x7FFF) + step) & 0x7FFF)
    return torch.where(out >= 0x8000, out - 0x10000, out).to(torch.int16)


def _usable(x, hi):
    return torch.isfinite(x) & torch.isfinite(hi.float()) & (x != 0)


def _toward_zero(x: torch.Tensor, fmt: int) -> torch.Tensor:
    """Bits of the 16-bit neighbour of x on the side of zero (x itself where it is representable)."""
    hi = round16(x, fmt)
    hb = bits(hi)
    over = hi.double().abs() > x.double().abs()
    return torch.where(over & _usable(x, hi), _mag_step(hb, -1), hb)


def mutant_truncate_hi(x, fmt):
    """(a) hi truncated toward zero instead of rounded; lo as the correct writer left it."""
    hi, lo = split_reference(x, fmt)
    hb = _toward_zero(x, fmt)
    return hb, bits(lo), hb != bits(hi)


def mutant_lo_against_other_neighbour(x, fmt):
    """(b) the round-4 bug: the stored hi is right, the hi inside the lo term is the OTHER neighbour of x."""
    hi, lo = split_reference(x, fmt)
    hb = bits(hi)
    down = _toward_zero(x, fmt)
    other = torch.where(down != hb, down, _mag_step(hb, +1))
    other_v = other.view(DTYPE[fmt]).float()
    ok = _usable(x, hi) & torch.isfinite(other_v) & (hi.float() != x)
    lb = torch.where(ok, bits(round16(x - other_v, fmt)), bits(lo))
    return hb, lb, lb != bits(lo)


def _flush_subnormal(b: torch.Tensor, fmt: int) -> torch.Tensor:
    i = b.to(torch.int32) & 0xFFFF
    expmask = 0x7F80 if fmt == 0 else 0x7C00
    sub = ((i & expmask) == 0) & ((i & 0x7FFF) != 0)
    out = torch.where(sub, i & 0x8000, i)
    return torch.where(out >= 0x8000, out - 0x10000, out).to(torch.int16)


def mutant_flush_lo(x, fmt):
    """(c) lo flushed to (signed) zero when subnormal."""
    hi, lo = split_reference(x, fmt)
    lb = _flush_subnormal(bits(lo), fmt)
    return bits(hi), lb, lb != bits(lo)


def mutant_flush_hi(x, fmt):
    """(d) hi flushed to (signed) zero when subnormal; lo as the correct writer left it."""
    hi, lo = split_reference(x, fmt)
    hb = _flush_subnormal(bits(hi), fmt)
    return hb, bits(lo), hb != bits(hi)


def mutant_ties_away(x, fmt):
    """(e) exact ties rounded away from zero instead of to even; lo recomputed against that hi (a self-consistent pair)."""
    hi, lo = split_reference(x, fmt)
    down = _toward_zero(x, fmt)
    up = _mag_step(down, +1)
    dv, uv, xd = down.view(DTYPE[fmt]).double(), up.view(DTYPE[fmt]).double(), x.double()
    tie = _usable(x, hi) & torch.isfinite(uv) & (dv != xd) & ((xd - dv).abs() == (uv - xd).abs())
    hb = torch.where(tie, up, bits(hi))
    lb = torch.where(tie, bits(round16(x - hb.view(DTYPE[fmt]).float(), fmt)), bits(lo))
    return hb, lb, hb != bits(hi)


def mutant_drop_zero_sign(x, fmt):
    """(f) -0.0 stored as +0.0, in either plane."""
    hi, lo = split_reference(x, fmt)
    hb, lb = bits(hi), bits(lo)
    neg0 = torch.tensor(-0x8000, dtype=torch.int16)
    h2, l2 = torch.where(hb == neg0, torch.zeros_like(hb), hb), torch.where(lb == neg0, torch.zeros_like(lb), lb)
    return h2, l2, (h2 != hb) | (l2 != lb)
