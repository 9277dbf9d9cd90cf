"""The stages of the contact head (csrc/contact_head.hip) held to truths that do not depend on the code under test
(tests/contact_truth.py, proved on the CPU by tests/test_contact_truth.py): the row sums rs [nch, T] and the totals tot [nch] are
read from the workspace after the call (include/rnamsm.h states the layout), the contacts from the output.

1. Exact stages.  On contact_truth.exact_case every sum has one correct fp32 value whatever its order, so rs and tot must be the
   truth's BITS on every route, and the logit is exact; the contacts are then within SIGMOID_ULPS of the fp64 sigmoid of that
   logit.  The budget of 1 / (1 + expf(-z)): expf 1 ulp -- the bound of the published HIP math API reference; the ROCm
   installation this was written against carries no math accuracy document of its own -- which is up to 2 ulps of the quotient, the
   add and the correctly rounded divide half an ulp each, and one of slack: 4.
2. Real-valued stages.  On loud_maps + loud_regression (row sums that vary by a decade, loud elements at the 32- and 256-seams, the
   sigmoid on its slope) rs, tot and the contacts are as close to fp64 as the fp32 restatement with the library's own sums:
   ss_truth.compare with its own multiples (rel-L2 2 x, element-wise 4 x, its floors).
3. Packed slabs.  Each member's slab and contacts are the lone call's bits in both orders; nothing behind the last slab, nothing in
   the NaN gaps between strided planes.

The truths are computed on the CPU, beyond T = 1023 with torch on the device (16 M pixels per channel)."""
import functools

import numpy as np
import pytest
import torch

import contact_routes as R
import contact_truth as CT
import ss_truth

pytestmark = pytest.mark.gpu
SIGMOID_ULPS = 4.0


def _truth_device(T):
    return R.DEV if T > 1023 else "cpu"


def _routes(T):
    if T > 1023:
        return ("long",)
    return ("atp", "long") + (("unstripped",) if T in CT.UNSTRIPPED_TS else ())


@functools.lru_cache(maxsize=3)
def _exact(T, nch):
    atp, w, b = CT.exact_case(nch, T, CT.case_seed(T, nch), band=CT.band_of(T))
    return atp, w, b, CT.stages(atp, w, b, torch.float64, _truth_device(T))


@functools.lru_cache(maxsize=2)
def _loud(T, nch):
    atp = CT.loud_maps(nch, T, CT.case_seed(T, nch), band=CT.band_of(T))
    dev = _truth_device(T)
    src = torch.from_numpy(atp).to(dev) if dev != "cpu" else atp
    w, b = CT.loud_regression(src, CT.case_seed(T, nch) + 1, dev)
    t64, t32 = CT.stages(src, w, b, torch.float64, dev), CT.stages(src, w, b, torch.float32, dev)
    return atp, w, b, t64, t32


def _check_exact(got, t64, label):
    for key in ("rs", "tot"):
        want = t64[key].astype(np.float32)
        assert np.array_equal(want.astype(np.float64), t64[key])
        diff = R.bits(got[key]) != R.bits(want)
        assert not diff.any(), (f"{label}: {key} differs from the exact value at {int(diff.sum())} of {diff.size} entries, first at "
                                f"{tuple(int(v) for v in np.argwhere(diff)[0])}: got {got[key][diff][0]!r}, exact {want[diff][0]!r}")
    z = t64["logits"]
    want = 1.0 / (1.0 + np.exp(-z))
    ulps = CT.ulps_f32(got["contacts"], want)
    worst = np.unravel_index(int(np.argmax(ulps)), ulps.shape)
    print(f"{label}: contacts within {ulps.max():.2f} ulps of sigmoid(exact z) (z = {z[worst]:.4f} there)")
    assert np.isfinite(got["contacts"]).all() and ulps.max() <= SIGMOID_ULPS, (label, float(ulps.max()), worst)


@pytest.mark.parametrize("T, nch", CT.shapes("exact"))
def test_exact_stages(T, nch):
    """rs and tot bit for bit, the contacts within 4 ulps of the fp64 sigmoid of the exact logit, on every lone route.  Nothing here
    depends on how the kernels order their sums."""
    atp, w, b, t64 = _exact(T, nch)
    for route in _routes(T):
        src = R.strided(atp, 5) if route == "atp" else atp
        _check_exact(R.lone(route, src, w, b), t64, f"exact T={T} nch={nch} {route}")
        if route == "atp":
            assert R.gaps_untouched(src)


@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("nch", CT.NCHS)
def test_exact_stages_packed(nch, order):
    Ts = CT.PACKED_TS if order == "forward" else CT.PACKED_TS[::-1]
    cases = [CT.exact_case(nch, T, CT.case_seed(T, nch)) for T in Ts]
    w, b = cases[0][1], cases[0][2]                          # one regression per packed call: +-1 weights serve every member
    got = R.packed([c[0] for c in cases], w, b)
    for T, c, g in zip(Ts, cases, got):
        _check_exact(g, CT.stages(c[0], w, b, torch.float64), f"exact packed {order} T={T} nch={nch}")


def _seam_report(d, T):
    idx = np.arange(T)
    out = []
    for period in (32, 256):
        m = CT.seam_mask(T, period)
        out.append(float(d[m[:, None] | m[None, :]].max()))
    edge = np.isin(idx, (0, T - 1))
    out.append(float(d[edge[:, None] | edge[None, :]].max()))
    return out


@pytest.mark.parametrize("T, nch", CT.shapes("loud"))
def test_real_valued_stages(T, nch):
    """rs, tot and the contacts against fp64 with the fp32 restatement (the library's own sums) as the yardstick.

    Measured on the MI355X.  With one sequential chain per row sum, rs was 3.7 x (T = 255) to 7 x (T = 1023) the
    restatement's rel-L2 and the contacts 2.3 x to 4.8 x: every case from T = 255 on failed.  With the sums in blocks of 64 rs is at
    most 1.8 x (T = 4096) and tot at most 1.5 x.

    Two cases of one and four pixels then still failed: [1-7], contacts max-abs 4.03e-07 against a bar of 2.30e-07 (the
    restatement's 1.39e-08), and [2-120], contacts rel-L2 4.83e-07 against 2 x 2.08e-07.  The regression formed
    s - (r_i r_j) fl(1 / tot) where the reference and the restatement divide; at T = 1 the quotient is exactly s and the true logit
    the bias alone, while each channel left up to an ulp of s.  With a correctly rounded division in contact_regress_kernel they
    measure 1.39e-08 (the restatement's own value) and 2.30e-07, and the contacts are at most 1.35 x the restatement's rel-L2 and
    0.82 of the element-wise bar over all shapes."""
    atp, w, b, t64, t32 = _loud(T, nch)
    assert float((np.abs(t64["logits"]) <= 8).mean()) >= 0.99                      # the condition (tests/test_contact_truth.py)
    for route in _routes(T):
        got = R.lone(route, atp, w, b)
        label = f"loud T={T} nch={nch} {route}"
        failures = []
        for key in ("rs", "tot", "contacts"):
            try:
                ss_truth.compare(got[key], t64[key], t32[key], f"{label} {key}", seams=False)
            except AssertionError as e:                                            # every stage's figures before the first failure
                failures.append(str(e))
        d = np.abs(got["contacts"].astype(np.float64) - t64["contacts"])
        s32, s256, edge = _seam_report(d, T)
        print(f"{label} contacts: worst |err| {d.max():.2e}; on index mod 32 in {{0, 31}} {s32:.2e}, mod 256 in {{0, 255}} {s256:.2e}, "
              f"on 0 / T-1 {edge:.2e}")
        assert not failures, "\n".join(failures)


@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("nch", CT.NCHS)
def test_packed_slabs_are_the_lone_calls(nch, order):
    """Members of T <= 256 and T > 256 in one call, planes strided with NaN in the gaps: each slab (rs, tot) and each output is the
    lone call's, bit for bit; the guard behind the last slab and the gaps stay as they were (contact_routes checks the guard)."""
    Ts = CT.PACKED_TS if order == "forward" else CT.PACKED_TS[::-1]
    w = np.random.default_rng(nch).standard_normal(nch).astype(np.float32) * np.float32(3)
    b = np.array([0.3], np.float32)
    atps = [CT.loud_maps(nch, T, CT.case_seed(T, nch)) for T in Ts]
    views = [R.strided(a, pad) for a, pad in zip(atps, (3, 1, 7, 2, 5))]
    got = R.packed(views, w, b)
    for T, a, v, g in zip(Ts, atps, views, got):
        want = R.lone("atp", a, w, b)
        for key in ("rs", "tot", "contacts"):
            assert np.isfinite(g[key]).all() and np.array_equal(R.bits(g[key]), R.bits(want[key])), (order, nch, T, key)
        assert R.gaps_untouched(v)
