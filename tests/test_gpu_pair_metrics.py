"""rnamsm_pair_sweep_* and rnamsm_pair_precision_* on the GPU (csrc/pair_metrics.hip; ops.pair_sweep, ops.pair_precision) against the
numpy statements of the two rules (tests/pair_metrics_truth.py).  Every comparison is exact: int64 counts, int32 hits and count, the
pairs and the scores' bits.  Every call goes through buffers with canaries on both sides of every output and of the workspace; every
element of x the rule says is never read (the diagonal, the lower triangle, the band closer than min_sep, the padding) is NaN or +inf,
and every such target byte is 1 or -1: reading any of them changes a count."""
import numpy as np
import pytest
import torch

from rnamsm import _lib, metrics, ops
import pair_metrics_truth as T
import top_pairs_truth as TP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
CANARY32, CANARY64, CANARY8 = 0x5A5A1234, 0x7FF8DEADBEEF1234, 0xA5
DTYPES = {"f64": np.float64, "f32": np.float32}
TH = metrics.sweep_thresholds()


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def poisoned(vals: np.ndarray, tgt: np.ndarray, min_sep: int):
    """x [L, L + 5] and target [L, L + 3]: the candidates' positions hold vals / tgt; everything else of x alternates NaN and +inf,
    everything else of the target 1 and -1."""
    L = vals.shape[0]
    x = np.full((L, L + 5), np.inf, dtype=vals.dtype)
    x[:, ::2] = np.nan
    t = np.ones((L, L + 3), dtype=np.int8)
    t[:, 1::2] = -1
    i, j = np.triu_indices(L, k=min_sep)
    x[i, j] = vals[i, j]
    t[i, j] = tgt[i, j]
    return x, t


def random_target(rng, L):
    t = (rng.random((L, L)) < 0.2).astype(np.int8)
    return t


class Sweep:
    def __init__(self, lib, x, t, th, min_sep, skip=None, stream=None, expect_ok=True, ws_short=0, L=None):
        L = x.shape[0] if L is None else L
        nt = len(th)
        xd, td = torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(np.ascontiguousarray(t)).to(DEV)
        thd = torch.from_numpy(np.ascontiguousarray(th, dtype=np.float64)).to(DEV)
        sd = torch.from_numpy(np.ascontiguousarray(skip).astype(np.uint8)).to(DEV) if skip is not None else None
        n_out = 4 * max(min(nt, 4096), 1)
        self.out = torch.full((n_out + 2 * GUARD,), CANARY64, dtype=torch.int64, device=DEV)
        need = lib.rnamsm_pair_sweep_workspace_bytes(nt) or 4096
        self.ws = torch.full((need + 512,), CANARY8, dtype=torch.uint8, device=DEV)
        assert self.ws.data_ptr() % 256 == 0
        fn = lib.rnamsm_pair_sweep_f64 if x.dtype == np.float64 else lib.rnamsm_pair_sweep_f32
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            self.rc = fn(xd.data_ptr(), L, x.shape[1], td.data_ptr(), t.shape[1], sd.data_ptr() if sd is not None else None, min_sep,
                         thd.data_ptr(), nt, self.out[GUARD:].data_ptr(), self.ws[256:].data_ptr(), need - ws_short, s.cuda_stream)
        self.msg = lib.rnamsm_last_error().decode()
        s.synchronize()
        if expect_ok:
            assert self.rc == 0, self.msg
        o, w = self.out.cpu().numpy(), self.ws.cpu().numpy()
        self.guards_ok = bool(np.all(o[:GUARD] == CANARY64) and np.all(o[GUARD + n_out:] == CANARY64) and np.all(w[:256] == CANARY8)
                              and np.all(w[256 + need:] == CANARY8))
        self.untouched = bool(np.all(o == CANARY64) and np.all(w == CANARY8))
        self.counts = o[GUARD:GUARD + n_out].reshape(4, -1)


def check_sweep(lib, x, t, th, min_sep, skip=None, what=None, L=None):
    L = x.shape[0] if L is None else L
    got = Sweep(lib, x, t, th, min_sep, skip)
    want = T.sweep_hist(x[:, :L], t[:, :L], th, min_sep, skip)
    assert got.guards_ok, what
    assert np.array_equal(got.counts, want), (what, np.flatnonzero((got.counts != want).any(0))[:5])
    return got


class Prec:
    def __init__(self, lib, x, t, k, cuts, min_sep, max_sep=0, stream=None, expect_ok=True, ws_short=0, want_pairs=True):
        L = x.shape[0]
        xd, td = torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(np.ascontiguousarray(t)).to(DEV)
        cd = torch.from_numpy(np.ascontiguousarray(cuts, dtype=np.int32)).to(DEV)
        nc, kk = max(min(len(cuts), 64), 1), max(min(k, 65536), 1)
        self.nc, self.kk = nc, kk
        self.hits_buf = torch.full((nc + 2 * GUARD,), CANARY32, dtype=torch.int32, device=DEV)
        self.count_buf = torch.full((1 + 2 * GUARD,), CANARY32, dtype=torch.int32, device=DEV)
        self.pairs_buf = torch.full((2 * kk + 2 * GUARD,), CANARY32, dtype=torch.int32, device=DEV)
        self.scores_buf = torch.full((kk + 2 * GUARD,), CANARY64, dtype=torch.int64, device=DEV)
        need = lib.rnamsm_pair_precision_workspace_bytes(L, k, x.dtype.itemsize) or 4096
        self.need = need
        self.ws = torch.full((need + 512,), CANARY8, dtype=torch.uint8, device=DEV)
        assert self.ws.data_ptr() % 256 == 0
        fn = lib.rnamsm_pair_precision_f64 if x.dtype == np.float64 else lib.rnamsm_pair_precision_f32
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            self.rc = fn(xd.data_ptr(), L, x.shape[1], td.data_ptr(), t.shape[1], min_sep, max_sep, k, cd.data_ptr(), len(cuts),
                         self.hits_buf[GUARD:].data_ptr(), self.count_buf[GUARD:].data_ptr(),
                         self.pairs_buf[GUARD:].data_ptr() if want_pairs else None, self.scores_buf[GUARD:].data_ptr() if want_pairs else None,
                         self.ws[256:].data_ptr(), need - ws_short, s.cuda_stream)
        self.msg = lib.rnamsm_last_error().decode()
        s.synchronize()
        if expect_ok:
            assert self.rc == 0, self.msg
        h, c, p, sc, w = (b.cpu().numpy() for b in (self.hits_buf, self.count_buf, self.pairs_buf, self.scores_buf, self.ws))
        self.guards_ok = bool(np.all(h[:GUARD] == CANARY32) and np.all(h[GUARD + nc:] == CANARY32) and np.all(c[:GUARD] == CANARY32)
                              and np.all(c[GUARD + 1:] == CANARY32) and np.all(p[:GUARD] == CANARY32) and np.all(p[GUARD + 2 * kk:] == CANARY32)
                              and np.all(sc[:GUARD] == CANARY64) and np.all(sc[GUARD + kk:] == CANARY64) and np.all(w[:256] == CANARY8)
                              and np.all(w[256 + need:] == CANARY8))
        self.untouched = bool(np.all(h == CANARY32) and np.all(c == CANARY32) and np.all(p == CANARY32) and np.all(sc == CANARY64)
                              and np.all(w == CANARY8))
        self.lists_untouched = bool(np.all(p == CANARY32) and np.all(sc == CANARY64))
        self.hits, self.count = h[GUARD:GUARD + nc].copy(), int(c[GUARD])
        self.pairs, self.scores = p[GUARD:GUARD + 2 * kk].reshape(kk, 2), sc[GUARD:GUARD + kk].view(np.float64)
        self.raw = self.hits.tobytes() + c[GUARD:GUARD + 1].tobytes() + self.pairs.tobytes() + self.scores.tobytes()


def check_prec(lib, x, t, k, cuts, min_sep, max_sep=0, what=None):
    L = x.shape[0]
    got = Prec(lib, x, t, k, cuts, min_sep, max_sep)
    hits, n, pairs, scores = T.precision_ranked(x[:, :L], t[:, :L], k, cuts, min_sep, max_sep)
    want_p, want_s, _ = TP.padded(pairs, scores, k)
    assert got.guards_ok, what
    assert got.count == n, (what, got.count, n)
    assert np.array_equal(got.hits, hits), (what, got.hits, hits)
    assert np.array_equal(got.pairs, want_p) and got.scores.tobytes() == want_s.tobytes(), what
    return got


# ---- the grid ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("L", [2, 3, 17, 64, 65, 257, 1024])
def test_every_shape_and_min_sep(lib, L, dtype):
    rng = np.random.default_rng(2000 + L)
    vals = rng.random((L, L)).astype(DTYPES[dtype])
    vals[rng.random((L, L)) < 0.5] *= 0.01
    tgt = random_target(rng, L)
    tgt_p = tgt.copy()
    tgt_p[rng.random((L, L)) < 0.1] = -1
    k = L
    cuts = np.unique(np.clip((np.arange(1, 11) * L) // 10, 1, k)).astype(np.int32)
    for min_sep in sorted({1, 2, 4, max(L - 1, 1), L}):
        x, t = poisoned(vals, tgt, min_sep)
        check_sweep(lib, x, t, TH, min_sep, what=(L, dtype, min_sep), L=L)
        x, t = poisoned(vals, tgt_p, min_sep)
        check_prec(lib, x, t, k, cuts, min_sep, what=(L, dtype, min_sep))
        # rnamsm_top_pairs_* on the same map is what it was
        xd = torch.from_numpy(x).to(DEV)
        rec = ops.top_pairs(xd[:, :L], 7, min_sep)
        want_p, want_s, n = TP.padded(*TP.truth(x[:, :L], 7, min_sep), 7)
        assert int(rec.count) == n and np.array_equal(rec.pairs.cpu().numpy(), want_p) and rec.scores.cpu().numpy().tobytes() == want_s.tobytes()


# ---- threshold edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_values_on_and_beside_the_thresholds(lib, dtype):
    dt = DTYPES[dtype]
    L = 65
    rng = np.random.default_rng(7)
    on = TH.astype(dt)                                                     # float32(0.001 t) against the float64 table
    cand = np.concatenate([on, np.nextafter(on, dt(np.inf)), np.nextafter(on, dt(-np.inf)),
                           np.array([-1.0, -1e-30, -0.0, 0.0, 1.0, 1.5, 1e30, np.inf, -np.inf, np.nan], dtype=dt)])
    if dt == np.float64:
        cand = np.concatenate([cand, TH.astype(np.float32).astype(np.float64)])
    vals = rng.choice(cand, (L, L)).astype(dt)
    tgt = random_target(rng, L)
    tgt[rng.random((L, L)) < 0.1] = 2                                      # bytes 2 and -1 are positive in the sweep
    tgt[rng.random((L, L)) < 0.1] = -1
    x, t = poisoned(vals, tgt, 1)
    got = check_sweep(lib, x, t, TH, 1, what=("edges", dtype), L=L)
    assert np.array_equal(got.counts, T.sweep_broadcast(x[:, :L], t[:, :L], TH, 1))
    pos = (tgt[np.triu_indices(L, 1)] != 0).sum()
    assert got.counts[0, 0] + got.counts[3, 0] == pos and (tgt[np.triu_indices(L, 1)] == -1).any()


@pytest.mark.parametrize("T_", [1, 2, 4095, 4096])
def test_table_sizes(lib, T_):
    L = 64
    rng = np.random.default_rng(T_)
    th = np.sort(rng.random(T_)) if T_ > 2 else np.array([0.5, 0.75][:T_])
    assert len(np.unique(th)) == T_
    vals = rng.random((L, L))
    idx = rng.integers(0, T_, (L, L))
    vals = np.where(rng.random((L, L)) < 0.5, th[idx], vals)               # half of the values lie exactly on a threshold
    x, t = poisoned(vals, random_target(rng, L), 1)
    check_sweep(lib, x, t, th, 1, what=("T", T_), L=L)


def test_a_non_uniform_table(lib):
    L = 65
    rng = np.random.default_rng(5)
    th = np.array([-np.finfo(np.float64).max, -3.0, -1e-300, 0.0, 5e-324, 1e-9, 0.5, 1.0, 7.0, np.finfo(np.float64).max])
    vals = rng.choice(np.concatenate([th, [-np.inf, np.inf, np.nan, -0.0, 2.0, -2.0]]), (L, L))
    x, t = poisoned(vals, random_target(rng, L), 2)
    got = check_sweep(lib, x, t, th, 2, what="non-uniform", L=L)
    assert np.array_equal(got.counts, T.sweep_broadcast(x[:, :L], t[:, :L], th, 2))


# ---- contention --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_all_zero_and_two_valued_maps(lib, dtype):
    L = 1024
    rng = np.random.default_rng(3)
    tgt = random_target(rng, L)
    z = np.zeros((L, L), dtype=DTYPES[dtype])
    got = check_sweep(lib, z, tgt, TH, 1, what="zeros")
    n = L * (L - 1) // 2
    assert got.counts[0, 0] + got.counts[1, 0] == n and got.counts[0, 1] + got.counts[1, 1] == 0
    two = np.where(rng.random((L, L)) < 0.5, 0.25, 0.75).astype(DTYPES[dtype])
    check_sweep(lib, two, tgt, TH, 1, what="two values")
    rows = np.where(np.arange(L)[:, None] % 2 == 0, 0.25, 0.75).astype(DTYPES[dtype]) * np.ones((1, L), dtype=DTYPES[dtype])
    check_sweep(lib, rows, tgt, TH, 3, what="two values by row")


# ---- skip --------------------------------------------------------------------------------------------------------------------------
def test_skipped_positions(lib):
    L = 65
    rng = np.random.default_rng(9)
    vals = rng.random((L, L)).astype(np.float32)
    tgt = random_target(rng, L)
    x, t = poisoned(vals, tgt, 2)
    for where in ([0], [L - 1], [0, L - 1], [3, 4, 5, 40, 63], list(range(L)), []):
        skip = np.zeros(L, dtype=np.uint8)
        skip[where] = 7
        xs, ts = x.copy(), t.copy()
        xs[where, :] = np.nan                                              # a skipped row or column is not read either
        xs[:, where] = np.inf
        ts[where, :] = 1
        ts[:, where] = -1
        got = Sweep(lib, xs, ts, TH, 2, skip, L=L)
        want = T.sweep_hist(x[:, :L], t[:, :L], TH, 2, skip)
        assert got.guards_ok and np.array_equal(got.counts, want), where


# ---- precision ---------------------------------------------------------------------------------------------------------------------
def test_precision_ties_negative_targets_max_sep_and_short_lists(lib):
    rng = np.random.default_rng(21)
    L = 65
    tgt = random_target(rng, L)
    tgt[rng.random((L, L)) < 0.2] = -1
    cuts10 = metrics.precision_cuts(L)
    for name, vals in (("zeros", np.zeros((L, L))), ("small integers", rng.integers(0, 4, (L, L)).astype(np.float64)),
                       ("f32 integers", rng.integers(0, 3, (L, L)).astype(np.float32))):
        x, t = poisoned(vals, tgt, 1)
        for max_sep in (0, 1, 2, 24, L, L + 9):
            check_prec(lib, x, t, L, cuts10, 1, max_sep, what=(name, max_sep))
    # a loop's statement of the rule on a small map
    Ls = 17
    vs, ts = rng.integers(0, 3, (Ls, Ls)).astype(np.float64), tgt[:Ls, :Ls]
    x, t = poisoned(vs, ts, 2)
    got = check_prec(lib, x, t, 40, [1, 5, 17, 40], 2, 9, what="loop")
    hits, n, pairs, _ = T.precision_loop(x[:, :Ls], t[:, :Ls], 40, [1, 5, 17, 40], 2, 9)
    assert np.array_equal(got.hits, hits) and got.count == n and np.array_equal(got.pairs[:n], pairs)
    # fewer than k candidates: count = n and the later cuts saturate
    x, t = poisoned(rng.random((L, L)), tgt, 60)
    got = check_prec(lib, x, t, 1000, [1, 2, 9, 10, 15, 500, 1000], 60, what="short")
    assert got.count <= 15 and got.hits[-1] == got.hits[-2] == got.hits[-3]
    allneg = np.full((L, L), -1, dtype=np.int8)
    got = check_prec(lib, *poisoned(rng.random((L, L)), allneg, 1), 10, [1, 10], 1, what="no candidate")
    assert got.count == 0 and np.array_equal(got.hits, [0, 0])


@pytest.mark.parametrize("ncuts", [1, 64])
def test_number_of_cuts_and_many_ranks(lib, ncuts):
    L = 257
    rng = np.random.default_rng(ncuts)
    tgt = random_target(rng, L)
    x, t = poisoned(rng.random((L, L)).astype(np.float32), tgt, 1)
    k = 5000                                                               # five rounds of the scan
    cuts = np.sort(rng.choice(np.arange(1, k + 1), ncuts, replace=False)) if ncuts > 1 else [1024]
    check_prec(lib, x, t, k, cuts, 1, what=ncuts)
    check_prec(lib, x, t, k, [1, 1023, 1024, 1025, 2048, 4096, 4097, k] if ncuts > 1 else [k], 1, what="scan seams")


def test_optional_lists(lib):
    L = 64
    rng = np.random.default_rng(8)
    x, t = poisoned(rng.random((L, L)), random_target(rng, L), 1)
    a, b = Prec(lib, x, t, L, [6, 32, 64], 1), Prec(lib, x, t, L, [6, 32, 64], 1, want_pairs=False)
    assert b.guards_ok and b.lists_untouched and np.array_equal(a.hits, b.hits) and a.count == b.count


# ---- determinism, a side stream, refusals -------------------------------------------------------------------------------------------
def test_reruns_and_a_side_stream_give_the_same_bytes(lib):
    L = 257
    rng = np.random.default_rng(13)
    vals = np.round(rng.random((L, L)) * 8) / 8
    x, t = poisoned(vals, random_target(rng, L), 1)
    side = torch.cuda.Stream(device=DEV)
    s0 = Sweep(lib, x, t, TH, 1, L=L)
    p0 = Prec(lib, x, t, 300, [1, 100, 300], 1)
    for stream in (None, side, None):
        s1, p1 = Sweep(lib, x, t, TH, 1, stream=stream, L=L), Prec(lib, x, t, 300, [1, 100, 300], 1, stream=stream)
        assert s1.guards_ok and p1.guards_ok and s1.counts.tobytes() == s0.counts.tobytes() and p1.raw == p0.raw


def test_refusals_touch_no_output(lib):
    L = 17
    rng = np.random.default_rng(1)
    x, t = poisoned(rng.random((L, L)), random_target(rng, L), 1)
    c = Sweep(lib, x, t, TH, 0, expect_ok=False, L=L)
    assert c.rc == -1 and c.untouched and c.msg == "pair_sweep_f64: min_sep=0 outside [1, 32768]"
    c = Sweep(lib, x, t, TH, 1, expect_ok=False, ws_short=1, L=L)
    assert c.rc == -1 and c.untouched and "workspace of" in c.msg
    c = Sweep(lib, x, t, np.arange(4097) / 4097.0, 1, expect_ok=False, L=L)
    assert c.rc == -1 and c.untouched and c.msg == "pair_sweep_f64: T=4097 outside [1, 4096]"
    c = Sweep(lib, x, t, TH, 1, expect_ok=False, L=L + 6)                   # ld = L + 5 < the L it is told
    assert c.rc == -1 and c.untouched and c.msg == f"pair_sweep_f64: ld={L + 5} is smaller than L={L + 6}"
    p = Prec(lib, x, t, 0, [1], 1, expect_ok=False)
    assert p.rc == -1 and p.untouched and p.msg == "pair_precision_f64: k=0 outside [1, 65536]"
    p = Prec(lib, x, t, 5, list(range(1, 6)) * 13, 1, expect_ok=False)
    assert p.rc == -1 and p.untouched and p.msg == "pair_precision_f64: ncuts=65 outside [1, 64]"
    p = Prec(lib, x, t, 5, [1], 1, -2, expect_ok=False)
    assert p.rc == -1 and p.untouched and p.msg == "pair_precision_f64: max_sep=-2 is negative (0 = no upper limit)"
    p = Prec(lib, x, t, 5, [1], 1, expect_ok=False, ws_short=1)
    assert p.rc == -1 and p.untouched and "workspace of" in p.msg


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_ops_on_views_and_their_refusals():
    L = 65
    rng = np.random.default_rng(17)
    vals, tgt = rng.random((L, L)).astype(np.float32), random_target(rng, L)
    x, t = poisoned(vals, tgt, 3)
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    skip = torch.zeros(L, dtype=torch.bool, device=DEV)
    skip[5] = True
    counts = ops.pair_sweep(xd[:, :L], td[:, :L], TH, 3, skip)
    assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), T.sweep_hist(x[:, :L], t[:, :L], TH, 3, skip.cpu().numpy()))
    cuts = metrics.precision_cuts(L)
    hits, count = ops.pair_precision(xd[:, :L], td[:, :L], L, cuts, 3)
    want = T.precision_ranked(x[:, :L], t[:, :L], L, cuts, 3)
    assert np.array_equal(hits.cpu().numpy(), want[0]) and int(count) == want[1]
    rec, top = ops.pair_precision(xd[:, :L], td[:, :L], L, cuts, 3, 30, want_pairs=True)
    want = T.precision_ranked(x[:, :L], t[:, :L], L, cuts, 3, 30)
    assert np.array_equal(rec.hits.cpu().numpy(), want[0]) and np.array_equal(top.pairs.cpu().numpy()[:want[1]], want[2])
    with pytest.raises(ValueError, match="not contiguous"):
        ops.pair_sweep(xd[:, :L].t(), td[:, :L], TH)
    with pytest.raises(ValueError, match="not contiguous"):
        ops.pair_precision(xd[:, :L], td[:, :L].t(), L, cuts, 1)
    with pytest.raises(ValueError, match="not strictly ascending at index 2"):
        ops.pair_sweep(xd[:, :L], td[:, :L], [0.1, 0.2, 0.2])
    with pytest.raises(ValueError, match="is not finite"):
        ops.pair_sweep(xd[:, :L], td[:, :L], [0.1, np.inf])
    with pytest.raises(ValueError, match=r"outside \[1, k=65\]"):
        ops.pair_precision(xd[:, :L], td[:, :L], L, [1, 66], 1)
    with pytest.raises(ValueError, match="not ascending"):
        ops.pair_precision(xd[:, :L], td[:, :L], L, [5, 4], 1)
    with pytest.raises(_lib.RnamsmError, match="min_sep=0 outside"):
        ops.pair_sweep(xd[:, :L], td[:, :L], TH, 0)


# ---- the stitched limit -------------------------------------------------------------------------------------------------------------
def test_l4096_against_the_histogram_truth(lib):
    L = 4096
    rng = np.random.default_rng(4096)
    x = rng.random((L, L), dtype=np.float32)
    x[rng.random((L, L)) < 0.9] = 0
    t = (rng.random((L, L)) < 0.01).astype(np.int8)
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    counts = ops.pair_sweep(xd, td, TH, 1).cpu().numpy()
    assert np.array_equal(counts, T.sweep_hist(x, t, TH, 1))
    cuts = metrics.precision_cuts(L)
    hits, count = ops.pair_precision(xd, td, L, cuts, 4)
    want = T.precision_ranked(x, t, L, cuts, 4)
    assert np.array_equal(hits.cpu().numpy(), want[0]) and int(count) == want[1] == L
