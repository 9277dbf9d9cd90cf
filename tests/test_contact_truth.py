"""tests/contact_truth.py on the CPU: `stages` in fp64 is oracle.msm_oracle.contact_head; the generators meet the conditions the GPU
tests rest on, at every shape those tests use -- exact_case has one correct fp32 value per stage whatever the order of the sums
(fp64, fp32 ascending and fp32 shuffled give the same values), loud_regression keeps the sigmoid off its plateaus -- and the fp64
truth has the NaN / inf semantics tests/test_gpu_contact_head_nonfinite.py holds the kernels to."""
import numpy as np
import pytest
import torch

from oracle import msm_oracle as O
import contact_truth as CT

NAN, INF = float("nan"), float("inf")


def test_the_shape_lists_are_covered():
    assert set(CT.PACKED_TS) <= set(CT.ATP_TS) and set(CT.UNSTRIPPED_TS) <= set(CT.ATP_TS)
    assert min(CT.PACKED_TS) <= 256 < max(CT.PACKED_TS)
    assert (4096, 8) in CT.shapes("exact") and (4096, 40) in CT.shapes("loud") and (1023, 7) in CT.shapes("exact")
    assert 40 * 4096 * 4096 * 4 > 2 ** 31 + 4096 * 4096 * 4              # the last of 40 planes starts beyond 2^31 bytes


@pytest.mark.parametrize("T, nch", [(1, 7), (5, 120), (33, 7), (70, 120)])
def test_fp64_stages_are_the_oracle_on_the_unstripped_maps(T, nch):
    atp = CT.loud_maps(nch, T, seed=T)
    w, b = CT.loud_regression(atp, seed=T + 1)
    maps = np.random.default_rng(T).random((nch, T + 1, T + 1))         # row and column 0 (<cls>): anything
    maps[:, 1:, 1:] = atp
    want = O.contact_head(torch.from_numpy(maps), torch.from_numpy(w.astype(np.float64)), torch.from_numpy(b.astype(np.float64)))
    st = CT.stages(atp, w, b, torch.float64)
    assert st["contacts"].shape == (T, T) and st["rs"].shape == (nch, T) and st["tot"].shape == (nch,)
    assert float(np.abs(st["contacts"] - want.numpy()).max()) <= 1e-12
    s = atp.astype(np.float64) + atp.astype(np.float64).transpose(0, 2, 1)
    assert np.allclose(st["rs"], s.sum(-1), rtol=1e-13, atol=0) and np.allclose(st["tot"], s.sum((-1, -2)), rtol=1e-13, atol=0)
    assert float(np.abs(CT.stages(atp, w, b, torch.float32)["contacts"] - st["contacts"]).max()) < 1e-5


def test_loud_maps_are_loud():
    L, nch = 300, 3
    x = CT.loud_maps(nch, L, seed=5).astype(np.float64)
    assert x.dtype == np.float64 and (x > 0).all() and CT.loud_maps(nch, L, seed=5).dtype == np.float32
    inner = ~(CT.seam_mask(L, 32) | np.isin(np.arange(L), (0, L - 1)))
    for ch in range(nch):
        r = (x[ch] + x[ch].T).sum(-1)[inner]
        rows, cols = x[ch][inner][:, inner].sum(1), x[ch][inner][:, inner].sum(0)
        assert rows.max() / rows.min() >= 10 and cols.max() / cols.min() >= 10           # a decade of scale factors
        assert r.max() / r.min() >= 4
        assert np.abs(x[ch] - x[ch].T).mean() > 0.3 * x[ch].mean()                        # asymmetric
    many = np.log(CT.loud_maps(24, L, seed=6).astype(np.float64))      # geometric means: the scale factors average out over channels
    typical = many[:, inner][:, :, inner].mean()
    for edge in (0, L - 1, 31, 32, 255, 256):
        assert many[:, edge, inner].mean() > typical + np.log(3) and many[:, inner, edge].mean() > typical + np.log(3)
    band = CT.loud_maps(nch, L, seed=5, band=100)
    far = np.abs(np.arange(L)[:, None] - np.arange(L)[None, :]) >= 100
    assert (band[:, far].view(np.uint32) == 0).all() and (band[:, ~far] > 0).all()         # +0.0, bit for bit
    assert np.array_equal(band[:, ~far], CT.loud_maps(nch, L, seed=5)[:, ~far])


@pytest.mark.parametrize("T, nch", CT.shapes("loud"))
def test_loud_regression_keeps_the_sigmoid_on_its_slope(T, nch):
    """The condition of the real-valued GPU cases, on the fp64 truth alone: at least 99 % of the pixels with |z64| <= 8."""
    atp = CT.loud_maps(nch, T, CT.case_seed(T, nch), band=CT.band_of(T))
    w, b = CT.loud_regression(atp, CT.case_seed(T, nch) + 1)
    assert w.dtype == np.float32 and w.shape == (nch,) and b.shape == (1,)
    z = CT.stages(atp, w, b, torch.float64)["logits"]
    share, sd = float((np.abs(z) <= 8).mean()), float(z.std())
    print(f"loud T={T} nch={nch}: std(z64) {sd:.2f}, |z64| <= 8 on {share:.4f}")
    assert share >= 0.99
    assert T == 1 or 1.0 <= sd <= 2.0


@pytest.mark.parametrize("T, nch", CT.shapes("exact"))
def test_exact_case_has_one_value_in_every_order(T, nch):
    atp, w, b = CT.exact_case(nch, T, CT.case_seed(T, nch), band=CT.band_of(T))
    assert atp.dtype == np.float32 and set(np.unique(np.abs(w))) == {1.0} and float(b[0]) == 0.25
    c = float(atp[atp > 0].min())
    ints = atp / np.float32(c)
    assert np.log2(c) == np.round(np.log2(c)) and np.array_equal(ints, np.round(ints)) and ints.max() <= 3 and ints.min() >= 0
    if CT.band_of(T):
        idx = np.arange(T)
        assert (atp[:, np.abs(idx[:, None] - idx[None, :]) >= CT.band_of(T)].view(np.uint32) == 0).all()
    t64 = CT.stages(atp, w, b, torch.float64)
    assert (np.log2(t64["tot"]) == np.round(np.log2(t64["tot"]))).all()                    # every tot a power of two
    seam = CT.seam_mask(T, 32) | np.isin(np.arange(T), (0, T - 1))
    for ch in range(nch):                                                                  # the top-up element lies at a seam
        i, j = np.unravel_index(int(np.argmax(atp[ch])), (T, T))
        assert ints[ch].max() == 1 or (ints[ch, i, j] == 3 and seam[i] and seam[j] and i != j and (ints[ch] == 3).sum() == 1)
    rng = np.random.default_rng(T + nch)
    evals = {"fp32, the library's sum": CT.stages(atp, w, b, torch.float32),
             "fp32 sequential, ascending": CT.stages_in_order(atp, w, b),
             "fp32 sequential, shuffled": CT.stages_in_order(atp, w, b, rng.permutation(T), rng.permutation(nch))}
    for name, got in evals.items():
        for key in ("rs", "tot", "logits"):
            assert got[key].dtype == np.float32
            assert np.array_equal(got[key].astype(np.float64), t64[key]), (T, nch, name, key)
    for ch in range(nch):                                                                  # every r_i r_j within 24 bits
        r = np.unique(t64["rs"][ch])
        rr = r[:, None] * r[None, :]
        assert np.array_equal(rr.astype(np.float32).astype(np.float64), rr)
    share = float((np.abs(t64["logits"]) <= 12).mean())
    print(f"exact T={T} nch={nch}: c {c}, tot {t64['tot'][0]}, std(z) {t64['logits'].std():.2f}, |z| <= 12 on {share:.4f}")
    assert share >= 0.90


# ------------------------------------------------------------------ NaN and inf in the fp64 truth
def _pattern(T, pixel):
    """bool [T, T]: the rows and columns i and j of the pixel (i, j)."""
    m = np.zeros((T, T), bool)
    for k in pixel:
        m[k, :] = True
        m[:, k] = True
    return m


@pytest.mark.parametrize("T", [40, 300])
def test_nonfinite_semantics_of_the_truth(T):
    nch, plane = 7, 3
    atp = CT.loud_maps(nch, T, CT.case_seed(T, nch))
    w, b = CT.loud_regression(atp, CT.case_seed(T, nch) + 1)
    clean = CT.stages(atp, w, b, torch.float64)["contacts"]

    def run(bad, weight=w):
        return [CT.stages(bad, weight, b, dt)["contacts"] for dt in (torch.float64, torch.float32)]

    def poison(*spots):
        bad = atp.copy()
        for (i, j), v in spots:
            bad[plane, i, j] = v
        return bad

    for pixel in ((T // 2, T // 2 + 3), (0, T - 1), (31, 32)):
        for t in run(poison((pixel, NAN))):
            assert np.isnan(t).all()
        for value in (INF, -INF):
            t64, t32 = run(poison((pixel, value)))
            want = _pattern(T, pixel)
            assert np.array_equal(np.isnan(t64), want) and np.array_equal(np.isnan(t32), want)
            assert np.isfinite(t64[~want]).all() and float((~want).mean()) >= ((T - 2) / T) ** 2 - 1e-12
            # 1 / tot = 0 takes the channel's APC term away: elsewhere the channel adds w s, not w (s - r r^T / tot)
            other = CT.stages(np.delete(atp, plane, 0), np.delete(w, plane), b, torch.float64)["logits"]
            s = atp[plane].astype(np.float64) + atp[plane].astype(np.float64).T
            assert np.allclose(t64[~want], 1 / (1 + np.exp(-(other + float(w[plane]) * s)[~want])), rtol=1e-12, atol=0)
            assert np.abs(t64[~want] - clean[~want]).max() > 1e-3
        far = (pixel[0] + 5, (pixel[1] + 9) % T)
        for t in run(poison((pixel, INF), (far, -INF))):
            assert np.isnan(t).all()
        w0 = w.copy()
        w0[plane] = 0.0
        for t in run(poison((pixel, NAN)), w0):                  # 0 x NaN
            assert np.isnan(t).all()
    zero = atp.copy()
    zero[plane] = 0.0
    for t in run(zero):                                          # tot = 0: 0 / 0
        assert np.isnan(t).all()
