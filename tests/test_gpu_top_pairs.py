"""rnamsm_top_pairs_f64 / _f32 on the GPU (csrc/top_pairs.hip; ops.top_pairs, rnamsm.contacts.top_pairs) against the numpy statement
of the rule (tests/top_pairs_truth.py): pairs, the scores' bits and count are compared exactly -- no tolerance anywhere.  Every call
goes through buffers with canaries on both sides of pairs, scores, count and the workspace, and the regions the rule says are never
read (the diagonal, the lower triangle, the band closer than min_sep, the padding beyond column L) are full of +inf and NaN."""
import numpy as np
import pytest
import torch

from rnamsm import _lib, contacts, ops
import top_pairs_truth as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                       # canary elements on either side of every buffer
CANARY32, CANARY64, CANARY8 = 0x5A5A1234, 0x7FF8DEADBEEF1234, 0xA5
KS = (1, 2, 7, 64, 1000, 65536)
DTYPES = {"f64": np.float64, "f32": np.float32}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def poisoned(vals: np.ndarray, min_sep: int, pad: int = 5) -> np.ndarray:
    """[L, L + pad]: the candidates' positions hold vals, every other element -- diagonal, lower triangle, the band closer than
    min_sep -- is +inf and the padding alternates NaN and +inf."""
    L = vals.shape[0]
    x = np.full((L, L + pad), np.inf, dtype=vals.dtype)
    i, j = np.triu_indices(L, k=min_sep)
    x[i, j] = vals[i, j]
    x[:, L::2] = np.nan
    return x


class Call:
    """One call of the library on guarded buffers; .pairs / .scores / .count are the outputs on the host, .raw every byte written."""

    def __init__(self, lib, x: np.ndarray, L: int, k: int, min_sep: int, stream=None, ws_short: int = 0, expect_ok: bool = True,
                 ld=None):
        xd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
        kk = max(min(k, 65536), 1)
        self.k = kk
        self.pairs_buf = torch.full((2 * kk + 2 * GUARD,), CANARY32, dtype=torch.int32, device=DEV)
        self.scores_buf = torch.full((kk + 2 * GUARD,), CANARY64, dtype=torch.int64, device=DEV)
        self.count_buf = torch.full((1 + 2 * GUARD,), CANARY32, dtype=torch.int32, device=DEV)
        need = lib.rnamsm_top_pairs_workspace_bytes(L, k) or 4096
        self.need = need
        self.ws_buf = torch.full((need + 512,), CANARY8, dtype=torch.uint8, device=DEV)
        assert self.ws_buf.data_ptr() % 256 == 0
        fn = lib.rnamsm_top_pairs_f64 if x.dtype == np.float64 else lib.rnamsm_top_pairs_f32
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            self.rc = fn(xd.data_ptr(), L, x.shape[1] if ld is None else ld, min_sep, k, self.pairs_buf[GUARD:].data_ptr(),
                         self.scores_buf[GUARD:].data_ptr(), self.count_buf[GUARD:].data_ptr(), self.ws_buf[256:].data_ptr(),
                         need - ws_short, s.cuda_stream)
        self.msg = lib.rnamsm_last_error().decode()
        s.synchronize()
        if expect_ok:
            assert self.rc == 0, self.msg
        p, sc, c, w = (b.cpu().numpy() for b in (self.pairs_buf, self.scores_buf, self.count_buf, self.ws_buf))
        # the canaries on both sides of every buffer
        self.guards_ok = bool(np.all(p[:GUARD] == CANARY32) and np.all(p[GUARD + 2 * kk:] == CANARY32) and np.all(sc[:GUARD] == CANARY64) and np.all(sc[GUARD + kk:] == CANARY64)
                              and np.all(c[:GUARD] == CANARY32) and np.all(c[GUARD + 1:] == CANARY32)
                              and np.all(w[:256] == CANARY8) and np.all(w[256 + need:] == CANARY8))
        self.pairs = p[GUARD:GUARD + 2 * kk].reshape(kk, 2)
        self.scores = sc[GUARD:GUARD + kk].view(np.float64)
        self.count = int(c[GUARD])
        self.untouched = bool(np.all(p == CANARY32) and np.all(sc == CANARY64) and np.all(c == CANARY32) and np.all(w == CANARY8))
        self.raw = p[GUARD:GUARD + 2 * kk].tobytes() + sc[GUARD:GUARD + kk].tobytes() + c[GUARD:GUARD + 1].tobytes()


def check(call: Call, ranked, k: int, min_sep: int, L: int, what):
    """The device's outputs against the ranked list of every candidate, exactly."""
    want_p, want_s, n = T.padded(ranked[0], ranked[1], k)
    assert call.guards_ok, what
    assert call.count == n, (what, call.count, n)
    got_p, got_s = call.pairs, call.scores
    assert np.all(got_p[n:] == -1) and np.all(got_s[n:].view(np.int64) == np.float64(np.nan).view(np.int64)), what
    if n:                                                   # nothing of the regions that are never read
        assert np.all(got_p[:n, 0] >= 0) and np.all(got_p[:n, 1] < L) and np.all(got_p[:n, 1] - got_p[:n, 0] >= min_sep), what
    bad = np.flatnonzero((got_p != want_p).any(1) | (got_s.view(np.int64) != want_s.view(np.int64)))
    assert len(bad) == 0, (what, "first differing row", int(bad[0]), got_p[bad[0]], got_s[bad[0]], want_p[bad[0]], want_s[bad[0]])


# ---- shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("L", [2, 3, 17, 64, 65, 257, 1024])
def test_every_shape_min_sep_and_k(lib, L, dtype):
    rng = np.random.default_rng(1000 + L)
    vals = rng.standard_normal((L, L)).astype(DTYPES[dtype])
    for min_sep in sorted({1, 2, 4, L - 1, L}):
        x = poisoned(vals, min_sep)                         # ld = L + 5; everything that is no candidate is +inf or NaN
        ranked = T.ranked(x[:, :L], min_sep)
        assert len(ranked[1]) == max(L - min_sep, 0) * (max(L - min_sep, 0) + 1) // 2
        for k in KS:
            check(Call(lib, x, L, k, min_sep), ranked, k, min_sep, L, (L, dtype, min_sep, k))


# ---- ties --------------------------------------------------------------------------------------------------------------------------
def test_all_zero_map_takes_the_first_pairs_in_row_major_order(lib):
    L = 1024
    x = np.zeros((L, L))
    c = Call(lib, x, L, 1000, 1)
    assert c.count == 1000 and np.array_equal(c.pairs[:, 0], np.zeros(1000)) and np.array_equal(c.pairs[:, 1], np.arange(1, 1001))
    assert np.all(c.scores.view(np.int64) == 0) and c.guards_ok
    # ... and with few candidates a row, so that the 1000 ties span some fifty blocks; and 65536 of them, over many rows
    for min_sep, k in ((1000, 1000), (1, 65536), (700, 65536)):
        check(Call(lib, x, L, k, min_sep), T.ranked(x, min_sep), k, min_sep, L, ("zeros", min_sep, k))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_ties_across_the_column_segments_of_one_row(lib, dtype):
    L = 2050                                               # a row of more than 2048 columns is read by two blocks
    x = np.zeros((L, L), dtype=DTYPES[dtype])
    x[:, 1::2] = -0.0
    ranked = T.ranked(x, 1)
    for k in (2047, 3000, 65536):
        check(Call(lib, x, L, k, 1), ranked, k, 1, L, ("segments", dtype, k))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_the_threshold_inside_a_run_of_equal_scores(lib, dtype):
    L, min_sep = 65, 2
    rng = np.random.default_rng(5)
    two = np.where(rng.random((L, L)) < 0.3, 2.5, -1.25).astype(DTYPES[dtype])          # some 600 of 2016 candidates are the higher value
    small = rng.integers(0, 8, (L, L)).astype(DTYPES[dtype])
    zeros = np.where(rng.random((L, L)) < 0.5, 0.0, -0.0).astype(DTYPES[dtype])
    for name, vals in (("two values", two), ("integers", small), ("signed zeros", zeros)):
        x = poisoned(vals, min_sep)
        ranked = T.ranked(x[:, :L], min_sep)
        for k in (1, 7, 64, 300, 601, 1000, 1500, 2015, 2016, 2017):
            check(Call(lib, x, L, k, min_sep), ranked, k, min_sep, L, (name, dtype, k))
    got = Call(lib, poisoned(zeros, min_sep), L, 2016, min_sep)
    assert np.all(got.scores.view(np.int64) == 0)                                        # a zero is written as +0.0


# ---- the key's digits --------------------------------------------------------------------------------------------------------------
def _digit_maps(dtype):
    L = 65
    rng = np.random.default_rng(77)
    ft = DTYPES[dtype]
    it, nmant = (np.uint64, 52) if dtype == "f64" else (np.uint32, 23)
    out = {}
    one = np.array(1.0, dtype=ft).view(it)
    out["last mantissa bit"] = (one + rng.integers(0, 2, (L, L)).astype(it)).view(ft)
    out["low bits only"] = (one + rng.integers(0, 1 << (32 if dtype == "f64" else 8), (L, L)).astype(it)).view(ft)   # f64: the upper 32 bits are equal
    out["all negative"] = -np.abs(rng.standard_normal((L, L))).astype(ft) - ft(1e-3)
    tiny = np.array(1, dtype=it).view(ft)                                                # the smallest denormal
    mixed = rng.standard_normal((L, L)).astype(ft)
    sel = rng.integers(0, 4, (L, L))
    mixed = np.where(sel == 0, tiny * rng.integers(-9, 10, (L, L)).astype(ft), mixed).astype(ft)
    out["mixed signs with denormals"] = mixed
    infs = rng.standard_normal((L, L)).astype(ft)
    infs[rng.random((L, L)) < 0.1] = np.inf
    infs[rng.random((L, L)) < 0.1] = -np.inf
    out["infinities"] = infs
    nans = rng.standard_normal((L, L)).astype(ft)
    nans[rng.random((L, L)) < 0.3] = np.nan
    out["NaN sprinkled"] = nans
    out["all NaN"] = np.full((L, L), np.nan, dtype=ft)
    big = rng.standard_normal((L, L)) * 1e300 if dtype == "f64" else rng.standard_normal((L, L)) * 1e38
    out["huge"] = big.astype(ft)
    return out


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_values_that_differ_in_every_digit_of_the_key(lib, dtype):
    L, min_sep = 65, 2
    with np.errstate(all="ignore"):
        maps = _digit_maps(dtype)
    for name, vals in maps.items():
        assert vals.dtype == DTYPES[dtype], name
        x = poisoned(vals, min_sep)
        ranked = T.ranked(x[:, :L], min_sep)
        if name == "all NaN":
            assert len(ranked[1]) == 0
        if name == "NaN sprinkled":
            assert 1000 < len(ranked[1]) < 2016 and Call(lib, x, L, 65536, min_sep).count == len(ranked[1])
        for k in (1, 7, 64, 1000, 65536):
            check(Call(lib, x, L, k, min_sep), ranked, k, min_sep, L, (name, dtype, k))


# ---- outputs -----------------------------------------------------------------------------------------------------------------------
def test_a_second_run_and_another_stream_give_the_same_bytes(lib):
    L, min_sep, k = 257, 3, 1000
    rng = np.random.default_rng(9)
    x = poisoned(rng.integers(0, 50, (L, L)).astype(np.float64), min_sep)
    a, b = Call(lib, x, L, k, min_sep), Call(lib, x, L, k, min_sep)
    side = Call(lib, x, L, k, min_sep, stream=torch.cuda.Stream(DEV))
    assert a.raw == b.raw == side.raw and a.guards_ok and side.guards_ok
    check(side, T.ranked(x[:, :L], min_sep), k, min_sep, L, "side stream")


def test_a_float32_map_gives_the_scores_of_its_float64_widening(lib):
    L, min_sep, k = 65, 1, 3000
    x32 = np.random.default_rng(10).standard_normal((L, L)).astype(np.float32)
    a, b = Call(lib, x32, L, k, min_sep), Call(lib, x32.astype(np.float64), L, k, min_sep)
    assert a.raw == b.raw and a.count == L * (L - 1) // 2
    assert np.array_equal(a.scores[:a.count], x32[a.pairs[:a.count, 0], a.pairs[:a.count, 1]].astype(np.float64))


def test_the_python_wrappers(lib):
    L = 33
    rng = np.random.default_rng(12)
    wide = torch.from_numpy(rng.integers(0, 9, (L, L + 7)).astype(np.float64)).to(DEV)
    view = wide[:, :L]                                      # read where it lies: ld = L + 7
    rec = ops.top_pairs(view, 40, 2)
    want_p, want_s, n = T.padded(*T.truth(view.cpu().numpy(), 40, 2), 40)
    assert rec.pairs.dtype == torch.int32 and rec.scores.dtype == torch.float64 and rec.count.dtype == torch.int32
    assert int(rec.count) == n == 40 and np.array_equal(rec.pairs.cpu().numpy(), want_p)
    assert rec.scores.cpu().numpy().tobytes() == want_s.tobytes()
    with pytest.raises(ValueError, match="not contiguous"):
        ops.top_pairs(view.t(), 5)                          # square, but its last dimension strides over rows
    with pytest.raises(ValueError, match="square"):
        ops.top_pairs(wide, 5)
    with pytest.raises(TypeError):
        ops.top_pairs(view.to(torch.float16), 5)
    with pytest.raises(_lib.RnamsmError, match=r"k=0 outside \[1, 65536\]"):
        ops.top_pairs(view, 0)
    # rnamsm.contacts.top_pairs: numpy or tensor in, trimmed numpy out
    x = rng.standard_normal((L, L)).astype(np.float32)
    for arg, device in ((x, DEV), (torch.from_numpy(x).to(DEV), None)):
        p, s = contacts.top_pairs(arg, 1000, 4, device=device)
        tp, ts = T.truth(x, 1000, 4)
        assert p.dtype == np.int64 and s.dtype == np.float64 and len(s) == (L - 4) * (L - 3) // 2
        assert np.array_equal(p, tp) and s.tobytes() == ts.tobytes()
    p, s = contacts.top_pairs(x, 5, L, device=DEV)          # min_sep >= L is legal: nothing
    assert p.shape == (0, 2) and s.shape == (0,)


# ---- size --------------------------------------------------------------------------------------------------------------------------
def test_a_map_of_4096_positions(lib):
    L, min_sep, k = 4096, 4, 65536
    x = np.random.default_rng(4096).standard_normal((L, L))
    check(Call(lib, x, L, k, min_sep), T.ranked(x, min_sep), k, min_sep, L, "L=4096")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_every_refusal_leaves_the_outputs_untouched(lib, dtype):
    name = "top_pairs_" + dtype
    x = np.ones((9, 12), dtype=DTYPES[dtype])
    for kw, text in ((dict(L=1), f"{name}: L=1 outside [2, 32768]"),
                     (dict(L=32769, ld=32769), f"{name}: L=32769 outside [2, 32768]"),
                     (dict(k=0), f"{name}: k=0 outside [1, 65536]"),
                     (dict(k=65537), f"{name}: k=65537 outside [1, 65536]"),
                     (dict(min_sep=0), f"{name}: min_sep=0 outside [1, 32768]"),
                     (dict(ld=8), f"{name}: ld=8 is smaller than L=9"),
                     (dict(ws_short=1), None)):
        a = dict(dict(L=9, k=5, min_sep=1, ld=None, ws_short=0), **kw)
        c = Call(lib, x, a["L"], a["k"], a["min_sep"], ws_short=a["ws_short"], expect_ok=False, ld=a["ld"])
        if text is None:
            text = f"{name}: workspace of {c.need - 1} bytes is smaller than the {c.need} that L=9, k=5 need"
        assert c.rc == -1 and c.msg == text, (kw, c.rc, c.msg)
        assert c.untouched, kw
