"""GPU tests of the sub-sampling kernels (csrc/greedy_select.hip, f3 of include/rnamsm.h) at the limits the header
documents: rnamsm_greedy_select (num_seqs <= 2048, L < 65536) and rnamsm_msa_weights (L <= 32768).

The contract is not a tolerance: the device repeats the reference's float64 arithmetic, so indices and weights are compared
with np.array_equal against the host implementation (rnamsm.msa, pinned to the reference's fixtures by the CPU suite) and
against independent forms written out here.  tests/test_pairwise_order.py holds the summation model the deep-history
cases are chosen with.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ERR_INVALID = -1                  # RNAMSM_ERR_INVALID
SCHEMES = (0, 2)                  # greedy_fused: three launches per step (a thread per row) / one (a wave per row)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rnamsm import _lib
    _lib.load()
    return torch.device("cuda:0")


def _tokens(body):
    """uint8 body [N, L] -> the int64 token matrix the host functions take (a <cls> column in front)."""
    return np.concatenate([np.zeros((body.shape[0], 1), np.int64), body.astype(np.int64)], 1)


def _host_select(body, num_seqs, mode):
    from rnamsm import msa
    return msa.greedy_select(_tokens(body), num_seqs, mode)


def _dev_select(msa_u8, num_seqs, mode, scheme=1):
    """ops.greedy_select under a given greedy_fused (1 = the default rule: by depth), restored afterwards."""
    from rnamsm import ops
    try:
        ops.set_param("greedy_fused", scheme)
        return ops.greedy_select(msa_u8, num_seqs, mode).cpu().numpy()
    finally:
        ops.set_param("greedy_fused", 1)


def _check_select(body, num_seqs, dev, schemes=(1,) + SCHEMES, modes=("max", "min")):
    t = torch.from_numpy(body).to(dev)
    for mode in modes:
        want = _host_select(body, num_seqs, mode)
        for scheme in schemes:
            assert np.array_equal(_dev_select(t, num_seqs, mode, scheme), want), (body.shape, num_seqs, mode, scheme)


# ---- deep histories ----------------------------------------------------------------------------------------------------
def _leaf(h):
    """numpy's unrolled leaf over the columns of h [rows, n], every row at once."""
    n = h.shape[1]
    if n < 8:
        res = np.zeros(h.shape[0])
        for i in range(n):
            res = res + h[:, i]
        return res
    full = n - n % 8
    r = h[:, :8].copy()
    for i in range(8, full, 8):
        r += h[:, i:i + 8]
    res = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
    for i in range(full, n):
        res = res + h[:, i]
    return res


def _sum_levels(h, levels):
    """numpy's pairwise sum along axis 1, the recursion cut off after `levels` levels (test_pairwise_order.py's model,
    vectorised over the rows): five levels are numpy's order for n <= 2047, four are one too few from n = 1929 on."""
    n = h.shape[1]
    if n <= 128 or levels == 0:
        return _leaf(h)
    n2 = n // 2
    n2 -= n2 % 8
    return _sum_levels(h[:, :n2], levels - 1) + _sum_levels(h[:, n2:], levels - 1)


def _pick_order(body, num_seqs, mode, probe_from=None):
    """The greedy rule with rnamsm.msa.greedy_select's structure, returning the pick ORDER (so the selection for any
    K <= num_seqs is sorted(order[:K])), and the first step >= probe_from at which a four-level summation of the same
    histories would have picked another row (None: never)."""
    N = body.shape[0]
    pick = np.argmax if mode == "max" else np.argmin
    order = [0]
    taken = np.zeros(N, dtype=bool)
    taken[0] = True
    hist = np.empty((N, num_seqs - 1), dtype=np.float64)             # [candidate, step]: step axis contiguous
    diverged = None
    for step in range(1, num_seqs):
        hist[:, step - 1] = (body != body[order[-1]][None, :]).mean(1)
        cand = np.flatnonzero(~taken)
        h = hist[cand, :step]
        total = h.sum(1)
        best = cand[pick(total / step)]                               # ties: first index
        if probe_from is not None and diverged is None and step >= probe_from:
            assert np.array_equal(_sum_levels(h, 5), total), step     # the model IS numpy's order
            if cand[pick(_sum_levels(h, 4) / step)] != best:
                diverged = step
        order.append(int(best))
        taken[best] = True
    return order, diverged


DEEP_N, DEEP_L = 2200, 7          # close to the smallest alignment with 2047 steps and candidates left; m / 7 is inexact
# The step at which a four-level recursion (exact up to 1928 terms, tests/test_pairwise_order.py) first picks another row
# than numpy's order on the alignment below, found by _pick_order's probe and asserted by the `deep` fixture; the index
# set that ENDS at that pick (num_seqs = step + 1) is the one that shows it -- a row passed over among tied candidates is
# usually picked a few steps later, so later sets agree again.
DEEP_DIVERGES = {"min": 1953, "max": 2043}
DEEP_NUM_SEQS = (1929, 1954, 2044, 2048)
WIDE_N = 3073                     # one row past the default switch to a thread per row (N > 3072)


def _deep_body(n, seed):
    return np.random.RandomState(seed).choice([4, 5, 6, 7, 10], size=(n, DEEP_L), p=[.3, .3, .2, .1, .1]).astype(np.uint8)


@pytest.fixture(scope="module")
def deep(dev):
    """The pick order to num_seqs = 2048 per mode, computed once, and the alignment on the device."""
    body = _deep_body(DEEP_N, 0)
    orders = {}
    for mode in ("max", "min"):
        orders[mode], diverged = _pick_order(body, 2048, mode, probe_from=1929)
        assert diverged == DEEP_DIVERGES[mode], (mode, diverged)
        assert diverged + 1 in DEEP_NUM_SEQS
    return body, torch.from_numpy(body).to(dev), orders


def test_pick_order_is_the_host_path(deep):
    """Ties the truth of the deep-history cases to rnamsm.msa.greedy_select (which the CPU suite pins to the reference)."""
    body, _, orders = deep
    assert np.array_equal(sorted(orders["min"][:1954]), _host_select(body, 1954, "min"))
    assert np.array_equal(sorted(orders["max"][:300]), _host_select(body, 300, "max"))


@pytest.mark.parametrize("num_seqs", DEEP_NUM_SEQS)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("mode", ["max", "min"])
def test_deep_history(deep, mode, scheme, num_seqs):
    """Histories of up to 2047 terms, past the 1928 a four-level recursion sums in numpy's order: both kernels that
    re-reduce a history pick numpy's rows, at the num_seqs where another order shows (1954 for min, 2044 for max), at
    the first depth that needs the fifth level (1929) and at the limit (2048)."""
    _, t, orders = deep
    want = np.array(sorted(orders[mode][:num_seqs]))
    got = _dev_select(t, num_seqs, mode, scheme)
    assert np.array_equal(got, want), (mode, scheme, num_seqs, np.setdiff1d(got, want), np.setdiff1d(want, got))


def test_deep_history_on_the_default_route_to_a_thread_per_row(dev, deep):
    """N = 3073 at the default knob: the depth rule itself sends the call to the per-thread kernel.  The alignment is the
    deep one with 873 rows appended that differ from every other row in every column.  Their distance to any pick is
    7 / 7, so their mean is exactly 1.0 at every step, no candidate's mean is larger, and ties go to the first index: in
    mode "min" none of them is picked while an original row is left, and the pick order is the deep alignment's."""
    body, _, orders = deep
    wide = np.concatenate([body, np.full((WIDE_N - DEEP_N, DEEP_L), 99, np.uint8)])
    assert np.array_equal(_host_select(wide, 300, "min"), sorted(orders["min"][:300]))
    num_seqs = DEEP_DIVERGES["min"] + 1
    want = np.array(sorted(orders["min"][:num_seqs]))
    assert np.array_equal(_dev_select(torch.from_numpy(wide).to(dev), num_seqs, "min"), want)


@pytest.mark.parametrize("N", [3072, 3073])
def test_both_sides_of_the_default_switch(dev, N):
    rng = np.random.RandomState(N)
    body = rng.choice([4, 5, 6, 7, 10], size=(N, 12), p=[.3, .3, .2, .1, .1]).astype(np.uint8)
    body[rng.randint(0, N, N // 3)] = body[0]                         # exact ties: the first index must win
    _check_select(body, 40, dev)


# ---- byte values, alignment of the input, odd shapes ---------------------------------------------------------------------
def _founder_body(rng, N, L, founders=4, rate=0.15):
    """Rows from a few founders over all of 0..255, each with a random subset of its bytes (`rate` of them) changed ONLY
    in bit 7 and another ONLY in bit 0, plus a few rewritten bytes: ties and near-ties everywhere, every byte value in play."""
    f = rng.randint(0, 256, size=(founders, L))
    body = f[rng.randint(0, founders, size=N)]
    body = body ^ (0x80 * (rng.random_sample((N, L)) < rate)) ^ (0x01 * (rng.random_sample((N, L)) < rate))
    flips = rng.random_sample((N, L)) < rate / 3
    body[flips] = rng.randint(0, 256, size=int(flips.sum()))
    return body.astype(np.uint8)


def test_every_byte_value_counts_as_one_mismatch(dev):
    """The fused kernel compares four bytes at a time (L % 4 == 0, aligned input): bytes that differ only in bit 7 or only
    in bit 0, and 0x00 / 0xff / 0x7f / 0x80 against each other, are one mismatch each."""
    rng = np.random.RandomState(7)
    body = _founder_body(rng, 131, 8)
    body[1] = body[0] ^ 0x80                                          # bit 7 only, every byte
    body[2] = body[0] ^ 0x01                                          # bit 0 only, every byte
    body[3] = body[0] ^ np.array([0x80, 0, 0x01, 0, 0, 0x80, 0, 0x01], np.uint8)
    body[4] = 0x00
    body[5] = 0xff
    body[6] = 0x7f
    body[7] = 0x80
    body[8] = [0x00, 0xff, 0x7f, 0x80, 0x01, 0xfe, 0x00, 0xff]
    for num_seqs in (9, 60, 130):
        _check_select(body, num_seqs, dev, schemes=SCHEMES)


@pytest.mark.parametrize("L", [4, 8, 36, 256])
def test_input_at_every_byte_offset(dev, L):
    """The packed compare needs a 4-byte aligned matrix; at offsets 1..3 of a buffer the kernel must take the byte path
    and give the indices of offset 0 and of the host."""
    N, num_seqs = 54, 23
    body = _founder_body(np.random.RandomState(L), N, L)
    flat = torch.from_numpy(body.reshape(-1)).to(dev)
    for mode in ("max", "min"):
        want = _host_select(body, num_seqs, mode)
        for off in range(4):
            buf = torch.zeros(N * L + 8, dtype=torch.uint8, device=dev)
            assert buf.data_ptr() % 4 == 0
            buf[off:off + N * L].copy_(flat)
            t = buf[off:off + N * L].view(N, L)
            assert t.is_contiguous() and t.data_ptr() % 4 == off
            for scheme in SCHEMES:
                assert np.array_equal(_dev_select(t, num_seqs, mode, scheme), want), (L, mode, off, scheme)


@pytest.mark.parametrize("L", [1, 3, 5, 63, 65])
def test_widths_of_the_byte_path(dev, L):
    _check_select(_founder_body(np.random.RandomState(100 + L), 77, L), 31, dev, schemes=SCHEMES)


@pytest.mark.parametrize("N", [41, 42, 43])
def test_row_counts_that_do_not_fill_the_last_block(dev, N):
    body = _founder_body(np.random.RandomState(N), N, 12)
    _check_select(body, 17, dev, schemes=SCHEMES)
    _check_select(body, N - 1, dev, schemes=SCHEMES)


# ---- limits --------------------------------------------------------------------------------------------------------------
def test_longest_rows_do_not_wrap_the_history(dev):
    """L = 65535: mismatch counts of 65535, 65534 and 32768 in a uint16 history.  Against row 0 the rows count 65535, 65534,
    32768, 10 and 5: read as signed 16-bit they would be -1, -2, -32768, 10, 5 and both the max and the min pick change."""
    L = 65535
    body = np.zeros((6, L), np.uint8)
    body[1] = 1                                                       # 65535 columns differ from row 0
    body[2, :L - 1] = 1                                               # 65534
    body[3, :32768] = 2                                               # 32768
    body[4, :10] = 3
    body[5, :5] = 3
    m0 = (body != body[0]).sum(1)
    assert m0.tolist() == [0, 65535, 65534, 32768, 10, 5]
    assert _host_select(body, 2, "max").tolist() == [0, 1] and _host_select(body, 2, "min").tolist() == [0, 5]
    for num_seqs in (2, 4):
        _check_select(body, num_seqs, dev, schemes=SCHEMES)


def test_smallest_shapes(dev):
    from rnamsm import ops
    rng = np.random.RandomState(11)
    _check_select(rng.randint(0, 256, size=(37, 1)).astype(np.uint8), 10, dev, schemes=SCHEMES)     # L = 1
    one = torch.from_numpy(rng.randint(0, 256, size=(1, 5)).astype(np.uint8)).to(dev)               # N = 1
    for scheme in SCHEMES:
        assert _dev_select(one, 1, "max", scheme).tolist() == [0]
    # num_seqs == N, which rnamsm.msa.greedy_select_device answers without a launch: through the op itself
    full = torch.from_numpy(_founder_body(rng, 33, 9)).to(dev)
    for mode in ("max", "min"):
        for scheme in SCHEMES:
            assert np.array_equal(_dev_select(full, 33, mode, scheme), np.arange(33)), (mode, scheme)
    assert ops.get_param("greedy_fused") == 1


# ---- the C entry point: workspace, refusals --------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def test_workspace_is_reinitialised_and_nothing_else_is_written(dev):
    """A workspace of exactly the advertised size, pre-filled with 0xff and reused for other alignments without clearing:
    the ticket counter, `taken` and `chosen` start afresh each call; canaries around workspace and output stay."""
    from rnamsm import _lib, ops
    lib = _lib.load()
    rng = np.random.RandomState(13)
    shapes = [(203, 12, 50, "max"), (203, 12, 50, "min"), (101, 5, 30, "max"), (203, 12, 203, "min")]
    ws_bytes = lib.rnamsm_greedy_select_workspace_bytes(203, 12, 203)
    G = 256                                                           # canary width; keeps every piece 8-byte aligned
    ws_off = G
    out_off = ws_off + (ws_bytes + 7) // 8 * 8 + G
    buf = torch.full((out_off + 203 * 4 + G,), 0xA5, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 8 == 0
    for scheme in SCHEMES:
        buf[ws_off:ws_off + ws_bytes] = 0xFF
        try:
            ops.set_param("greedy_fused", scheme)
            for N, L, K, mode in shapes:
                body = _founder_body(rng, N, L)
                need = lib.rnamsm_greedy_select_workspace_bytes(N, L, K)
                assert 0 < need <= ws_bytes and (need == ws_bytes) == (K == 203)
                before = buf.cpu().numpy()
                t = torch.from_numpy(body).to(dev)
                rc = lib.rnamsm_greedy_select(t.data_ptr(), N, L, K, int(mode == "min"),
                                              buf.data_ptr() + out_off, buf.data_ptr() + ws_off, need, _stream())
                assert rc == 0, lib.rnamsm_last_error()
                torch.cuda.synchronize()
                after = buf.cpu().numpy()
                got = after[out_off:out_off + K * 4].view(np.int32)
                assert np.array_equal(got, _host_select(body, K, mode)), (scheme, N, L, K, mode)
                # nothing outside the `need` bytes handed over and the K indices has changed, the canaries included
                for lo, hi in ((0, ws_off), (ws_off + need, out_off), (out_off + K * 4, len(after))):
                    assert np.array_equal(after[lo:hi], before[lo:hi]), (scheme, N, L, K, lo, hi)
                assert (after[:ws_off] == 0xA5).all() and (after[out_off - G:out_off] == 0xA5).all()
                assert (after[-G:] == 0xA5).all()
        finally:
            ops.set_param("greedy_fused", 1)


def test_greedy_select_refusals(dev):
    """Every documented limit is refused with RNAMSM_ERR_INVALID before anything is launched: the output keeps its sentinel."""
    from rnamsm import _lib
    lib = _lib.load()
    wsb = lib.rnamsm_greedy_select_workspace_bytes
    assert wsb(0, 8, 4) == 0 and wsb(8, 0, 4) == 0 and wsb(8, 8, 0) == 0 and wsb(-1, 8, 4) == 0 and wsb(8, 8, -3) == 0
    N, L, K = 2100, 8, 16
    msa_t = torch.from_numpy(_founder_body(np.random.RandomState(17), N, L)).to(dev)
    wide = torch.zeros(2 * 65536, dtype=torch.uint8, device=dev)
    out = torch.full((2100,), -7, dtype=torch.int32, device=dev)
    ws = torch.zeros(max(wsb(N, L, 2049), wsb(2, 65536, 2)) + 64, dtype=torch.uint8, device=dev)
    m, o, w, s = msa_t.data_ptr(), out.data_ptr(), ws.data_ptr(), _stream()
    assert w % 8 == 0
    need = wsb(N, L, K)
    cases = {
        "num_seqs > N": (m, 100, L, 101, 0, o, w, ws.numel(), s),
        "num_seqs = 2049": (m, N, L, 2049, 0, o, w, ws.numel(), s),
        "L = 65536": (wide.data_ptr(), 2, 65536, 2, 0, o, w, ws.numel(), s),
        "null msa": (None, N, L, K, 0, o, w, ws.numel(), s),
        "null output": (m, N, L, K, 0, None, w, ws.numel(), s),
        "null workspace": (m, N, L, K, 0, o, None, ws.numel(), s),
        "workspace one byte short": (m, N, L, K, 0, o, w, need - 1, s),
        "workspace offset by 4 bytes": (m, N, L, K, 0, o, w + 4, ws.numel() - 4, s),
    }
    for what, args in cases.items():
        assert lib.rnamsm_greedy_select(*args) == ERR_INVALID, what
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    # and the same call with nothing wrong is accepted (the refusals above are not an always-refuse)
    assert lib.rnamsm_greedy_select(m, N, L, K, 0, o, w, need, s) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out[:K].cpu().numpy(), _host_select(msa_t.cpu().numpy(), K, "max"))
    assert bool((out[K:] == -7).all())


# ---- rnamsm_msa_weights -----------------------------------------------------------------------------------------------------
def _integer_weights(a, cutoff):
    """weights = 1 / #{ j : mismatches(i, j) / L < cutoff }, from integer mismatch counts, blockwise over i."""
    N, L = a.shape
    counts = np.zeros(N, dtype=np.int64)
    blk = max(1, (1 << 22) // max(1, N * L))
    for i0 in range(0, N, blk):
        m = (a[i0:i0 + blk, None, :] != a[None, :, :]).sum(-1)
        counts[i0:i0 + blk] = (m / L < cutoff).sum(1)
    with np.errstate(divide="ignore"):
        return 1 / counts


def _check_weights(body, cutoff, dev):
    from rnamsm import msa, ops
    got = ops.msa_weights(torch.from_numpy(body).to(dev), cutoff).cpu().numpy()
    with np.errstate(divide="ignore"):
        host = msa.msa_weights(_tokens(body), cutoff)
    assert got.dtype == np.float64
    assert np.array_equal(got, host), (body.shape, cutoff)
    assert np.array_equal(got, _integer_weights(body, cutoff)), (body.shape, cutoff)
    return got


@pytest.mark.parametrize("L", [1, 2, 3, 5, 9, 17, 33, 65, 255, 257])
def test_msa_weights_at_every_lane_group_width(dev, L):
    """G = the power of two >= min(L, 64) lanes share a row: every width and the lengths next to it, N around the 256
    threads of a block, bytes from all of 0..255, clusters of rows on both sides of the cutoff."""
    for N in (1, 255, 256, 257):
        rng = np.random.RandomState(1000 * L + N)
        body = _founder_body(rng, N, L, founders=3, rate=0.04)
        for cutoff in (0.2, 0.35):
            w = _check_weights(body, cutoff, dev)
            if N > 1 and L >= 9:
                assert w.min() < 1 and len(np.unique(w)) > 1, (N, L)  # rows do fall on both sides of the cutoff


def test_msa_weights_cutoff_on_a_representable_distance(dev):
    """m / L < cutoff is strict: rows at EXACTLY the cutoff (1/5 and 2/5 of 5 columns, 1/4 of 4) are not neighbours."""
    for L, cutoff, m_at in ((5, 0.2, 1), (5, 0.4, 2), (4, 0.25, 1)):
        assert m_at / L == cutoff
        base = np.arange(10, 10 + L)
        rows = [base.copy()]
        for m in range(L + 1):                                        # rows at every distance 0..L from the base, twice
            for rep in range(2):
                r = base.copy()
                r[:m] = 200 + rep                                     # the two copies differ from each other in m columns too
                rows.append(r)
        body = np.array(rows, dtype=np.uint8)
        w = _check_weights(body, cutoff, dev)
        near = ((body != body[0]).sum(1) < m_at).sum()                # strictly closer than the cutoff distance
        assert w[0] == 1 / near
        assert _check_weights(body, np.nextafter(cutoff, 1.0), dev)[0] < w[0]      # one ulp more lets them in
    pair = np.array([[1, 2, 3, 4, 5], [9, 2, 3, 4, 5]], dtype=np.uint8)            # distance exactly 1/5
    assert _check_weights(pair, 0.2, dev).tolist() == [1.0, 1.0]
    assert _check_weights(pair, np.nextafter(0.2, 1.0), dev).tolist() == [0.5, 0.5]


def test_msa_weights_cutoffs_beyond_every_distance(dev):
    body = _founder_body(np.random.RandomState(23), 300, 21, rate=0.04)
    assert np.array_equal(_check_weights(body, 2.0, dev), np.full(300, 1 / 300))
    w = _check_weights(body, 0.0, dev)                                # no row is nearer than 0, itself included
    assert np.isposinf(w).all()


def test_msa_weights_at_the_length_limit(dev):
    """L = 32768 (the row under comparison fills half the LDS) is served; L = 32769 is refused, output untouched."""
    from rnamsm import _lib
    L = 32768
    rng = np.random.RandomState(29)
    body = np.repeat(rng.randint(0, 256, size=(1, L)), 5, 0).astype(np.uint8)
    body[1, :6553] ^= 0x80                                            # 6553 / 32768 < 0.2
    body[2, :6554] ^= 0x01                                            # 6554 / 32768 > 0.2
    body[3] = rng.randint(0, 256, size=L)
    body[4, L - 1] ^= 0xff
    assert 6553 / L < 0.2 < 6554 / L
    w = _check_weights(body, 0.2, dev)
    assert w[0] == 1 / 3 and w[3] == 1.0
    lib = _lib.load()
    out = torch.full((5,), -7.0, dtype=torch.float64, device=dev)
    big = torch.zeros(5 * (L + 1), dtype=torch.uint8, device=dev)
    assert lib.rnamsm_msa_weights(big.data_ptr(), 5, L + 1, 0.2, out.data_ptr(), _stream()) == ERR_INVALID
    assert lib.rnamsm_msa_weights(None, 5, L, 0.2, out.data_ptr(), _stream()) == ERR_INVALID
    assert lib.rnamsm_msa_weights(big.data_ptr(), 5, L, 0.2, None, _stream()) == ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
