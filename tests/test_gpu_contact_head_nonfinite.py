"""The contact head on the GPU with a NaN, an inf or an all-zero plane in its input, against the fp64 truth of the same input
(tests/contact_truth.py; its semantics are pinned on the CPU by tests/test_contact_truth.py).  One NaN pixel makes a channel's total
NaN and with it every contact; one inf pixel (i, j) makes the total inf, so 1 / tot = 0 removes that channel's APC term everywhere
but on the rows and columns i and j, where inf x 0 is NaN; +inf and -inf together, or an all-zero plane (0 / 0), are NaN everywhere
-- also under a weight of 0.  The kernels must show exactly the truth's NaN pattern, no inf, and the truth's bars on the finite rest
(ss_truth.compare_masked).  T = 40 finishes the total inside the sums kernel, T = 300 in contact_tot_kernel; the pixel lies once
in the interior, once at (0, T - 1) and once on a 32-seam."""
import numpy as np
import pytest
import torch

import contact_routes as R
import contact_truth as CT
import ss_truth

pytestmark = pytest.mark.gpu
NCH, PLANE = 7, 3
NAN, INF = float("nan"), float("inf")
TS = (40, 300)


def _pixels(T):
    return {"interior": (T // 2, T // 2 + 3), "corner": (0, T - 1), "seam": (31, 32)}


class _Case:
    def __init__(self, T):
        self.T = T
        self.atp = CT.loud_maps(NCH, T, CT.case_seed(T, NCH))
        self.w, self.b = CT.loud_regression(self.atp, CT.case_seed(T, NCH) + 1)

    def check(self, bad, label, min_finite, weight=None):
        w = self.w if weight is None else weight
        t64 = CT.stages(bad, w, self.b, torch.float64)["contacts"]
        t32 = CT.stages(bad, w, self.b, torch.float32)["contacts"]
        for route in ("atp", "unstripped"):
            got = R.lone(route, bad, w, self.b)["contacts"]
            ss_truth.compare_masked(got, t64, t32, f"{label} {route}", min_finite=min_finite, expect_nan=True)
        return t64


_cases = {}


def _case(T):
    if T not in _cases:
        _cases[T] = _Case(T)
    return _cases[T]


@pytest.mark.parametrize("where", ["interior", "corner", "seam"])
@pytest.mark.parametrize("T", TS)
def test_one_nan_pixel_makes_every_contact_nan(T, where):
    c = _case(T)
    t64 = c.check(ss_truth.poisoned(c.atp, PLANE, _pixels(T)[where], NAN), f"T={T} nan {where}", 0.0)
    assert np.isnan(t64).all()


@pytest.mark.parametrize("name, value", [("+inf", INF), ("-inf", -INF)])
@pytest.mark.parametrize("where", ["interior", "corner", "seam"])
@pytest.mark.parametrize("T", TS)
def test_one_inf_pixel_is_nan_on_its_rows_and_columns_only(T, where, name, value):
    c = _case(T)
    i, j = _pixels(T)[where]
    min_finite = np.floor(1000 * ((T - 2) / T) ** 2) / 1000             # the truth: everything but rows / columns i and j
    t64 = c.check(ss_truth.poisoned(c.atp, PLANE, (i, j), value), f"T={T} {name} {where}", min_finite)
    want = np.zeros((T, T), bool)
    want[[i, j], :] = True
    want[:, [i, j]] = True
    assert np.array_equal(np.isnan(t64), want)


@pytest.mark.parametrize("T", TS)
def test_both_infinities_in_one_plane_are_nan_everywhere(T):
    c = _case(T)
    bad = ss_truth.poisoned(ss_truth.poisoned(c.atp, PLANE, _pixels(T)["interior"], INF), PLANE, (3, 11), -INF)
    assert np.isnan(c.check(bad, f"T={T} +inf and -inf", 0.0)).all()


@pytest.mark.parametrize("T", TS)
def test_an_all_zero_plane_is_nan_everywhere(T):
    c = _case(T)
    bad = c.atp.copy()
    bad[PLANE] = 0.0
    assert np.isnan(c.check(bad, f"T={T} zero plane", 0.0)).all()


@pytest.mark.parametrize("T", TS)
def test_a_poisoned_plane_of_weight_zero_is_still_nan(T):
    c = _case(T)
    w0 = c.w.copy()
    w0[PLANE] = 0.0
    for name, value in (("nan", NAN), ("+inf", INF)):
        bad = ss_truth.poisoned(c.atp, PLANE, _pixels(T)["seam"], value)
        t64 = c.check(bad, f"T={T} {name}, weight 0", 0.0 if name == "nan" else 0.9, weight=w0)
        assert np.isnan(t64).any()


@pytest.mark.parametrize("reverse", [False, True], ids=["in-order", "reversed"])
def test_a_poisoned_member_of_a_batch_stays_alone(reverse):
    """Members of T = 40, 300, 33, 257: the second carries a NaN pixel, the fourth an inf pixel.  The clean members keep the bits of
    their clean lone calls (contacts and slabs), the poisoned ones are their own lone poisoned calls, NaN positions included."""
    Ts = [40, 300, 33, 257]
    atps = [CT.loud_maps(NCH, T, CT.case_seed(T, NCH)) for T in Ts]
    w, b = _case(40).w, _case(40).b
    atps[1] = ss_truth.poisoned(atps[1], PLANE, (0, 299), NAN)
    atps[3] = ss_truth.poisoned(atps[3], 0, (255, 256), INF)
    lone = [R.lone("atp", a, w, b) for a in atps]
    assert np.isnan(lone[1]["contacts"]).all() and np.isnan(lone[3]["contacts"]).sum() == 4 * 257 - 4
    order = list(reversed(range(4))) if reverse else list(range(4))
    got = R.packed([atps[k] for k in order], w, b)
    for slot, k in enumerate(order):
        for key in ("contacts", "rs", "tot"):
            if k in (0, 2):
                assert np.isfinite(got[slot][key]).all(), f"member {k} {key}: a poisoned neighbour leaked"
            assert np.array_equal(R.bits(got[slot][key]), R.bits(lone[k][key])), f"member {k} (T = {Ts[k]}) in slot {slot}: {key}"
