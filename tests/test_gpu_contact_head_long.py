"""The contact head on a stitched long alignment (rnamsm_contact_head_long, ops.contact_head_long): up to L = 1023 the bits of
ops.contact_head_atp, planes read in place; beyond, an fp64 restatement of symmetrise + APC + regression + sigmoid in torch on the
device.  The bar there: the rel-L2 of the fp32 torch restatement of the same formula against that fp64, times 2 -- the factor the
project holds a kernel to against its fp32 restatement."""
import numpy as np
import pytest
import torch

from rnamsm import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _regression(nch: int, seed: int):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(nch, device=DEV, generator=g), torch.randn(1, device=DEV, generator=g) * 0.1


def _stitched_like(nch: int, L: int, seed: int, band: int) -> torch.Tensor:
    """Maps like a stitched atp: attention-sized values inside the band |i - j| < band, +0.0 outside (pairs no window holds)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    atp = torch.rand(nch, L, L, device=DEV, generator=g).mul_(2.0 / L)
    idx = torch.arange(L, device=DEV)
    atp.mul_(((idx[:, None] - idx[None, :]).abs() < band).to(atp.dtype))
    return atp


def _restated(atp: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, dtype) -> torch.Tensor:
    """sigmoid(b + sum_ch w[ch] apc(symmetrize(atp[ch]))) channel by channel in `dtype` (utils/tensor.py:98-113)."""
    L = atp.shape[-1]
    acc = torch.zeros(L, L, device=atp.device, dtype=dtype)
    for ch in range(atp.shape[0]):
        x = atp[ch].to(dtype)
        s = x + x.T
        a1, a2 = s.sum(-1, keepdim=True), s.sum(-2, keepdim=True)
        acc += weight[ch].to(dtype) * (s - a1 * a2 / s.sum())
    return torch.sigmoid(acc + bias.to(dtype))


@pytest.mark.parametrize("L", [1, 33, 257, 1023])
def test_up_to_1023_the_bits_are_those_of_the_existing_head_on_planes_read_in_place(L):
    nch = 120
    weight, bias = _regression(nch, L)
    wide = torch.full((nch, L * L + 5), float("nan"), device=DEV)        # NaN in the gaps between the planes
    atp = wide[:, :L * L].view(nch, L, L)
    atp.copy_(_stitched_like(nch, L, L, max(2, L // 3)))
    assert atp.stride(0) == L * L + 5
    got, want = ops.contact_head_long(atp, weight, bias), ops.contact_head_atp(atp, weight, bias)
    assert got.shape == (L, L) and bool(torch.isfinite(got).all())
    assert (got.cpu().numpy().view(np.uint32) == want.cpu().numpy().view(np.uint32)).all()


@pytest.mark.parametrize("L,nch", [(1025, 120), (4096, 40)])
def test_beyond_1023_against_fp64(L, nch):
    """L = 4096, nch = 40: the last plane starts beyond 2^31 bytes."""
    weight, bias = _regression(nch, L)
    atp = _stitched_like(nch, L, L, 1023)
    got = ops.contact_head_long(atp, weight, bias).double()
    t64 = _restated(atp, weight, bias, torch.float64)
    t32 = _restated(atp, weight, bias, torch.float32).double()
    err, drift = (float((v - t64).norm() / t64.norm()) for v in (got, t32))
    print(f"contact_head_long L={L} nch={nch}: rel-L2 vs fp64 {err:.3e}, fp32 restatement {drift:.3e}, ratio {err / drift:.2f}")
    assert bool(torch.isfinite(got).all()) and drift > 0
    assert err <= 2 * drift, (err, drift)
    # APC over the whole map: a pair outside the band takes part as 0, so its contact is the regression of the correction term alone
    assert float((got[0, L - 1] - t64[0, L - 1]).abs()) < 1e-5


def test_the_limits():
    weight, bias = _regression(4, 1)
    one = torch.zeros(1, device=DEV)
    with pytest.raises(ValueError, match=r"\[1, 4096\]"):
        ops.contact_head_long(one.expand(4, 4097, 4097), weight, bias)
    with pytest.raises(ValueError, match=r"\[1, 1023\]"):
        ops.contact_head_atp(torch.zeros(4, 1024, 1024, device=DEV), weight, bias)
