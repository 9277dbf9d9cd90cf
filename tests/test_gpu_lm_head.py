"""The LM head's kernels (rnamsm_lm_head / rnamsm_lm_head_packed) on the GPU: accuracy against the fp64 truth with the fp32
restatement as the yardstick (tests/lm_truth.py, bars of tests/ss_truth.py), the gather, the output subsets, the wild-type column,
large logits, non-finite rows and the packed call's bit identity."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import lm_truth
import ss_truth
from rnamsm import _lib, ops, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTS = _lib.LM_OUTPUTS


@pytest.fixture(scope="module")
def full_state():
    return synthetic.make_state_dict(seed=0)


def weights_of(state: dict) -> ops.LMWeights:
    return ops.lm_weights(*(torch.from_numpy(state["lm_head." + n]).to(DEV) for n in lm_truth.NAMES))


def features(n: int, D: int, seed: int) -> np.ndarray:
    return np.random.RandomState(seed).standard_normal((n, D)).astype(np.float32)


def run(x, rows, wt, W, want=None) -> dict:
    out = ops.lm_head_rows(x if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(DEV), rows, wt, W, want)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(a: dict, b: dict, label=""):
    assert a.keys() == b.keys(), label
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (label, k)


def check_against_truth(got: dict, x, state, wt, label: str):
    t64, t32 = lm_truth.head(x, state, wt), lm_truth.head(x, state, wt, dtype=torch.float32)
    for k in OUTS:
        if k == "nll" and len(wt) == 1:
            continue            # one number: its restatement error is one rounding sample; it is -logp[wt] exactly (asserted below)
        ss_truth.compare(got[k], t64[k], t32[k], f"{label} {k}")
    n = len(wt)
    assert (got["scores"][np.arange(n), wt] == 0.0).all(), label
    assert got["nll"].tobytes() == (-got["logp"][np.arange(n), wt]).tobytes(), label


@pytest.mark.parametrize("D,V,n", [(768, 12, 1), (768, 12, 31), (768, 12, 32), (768, 12, 33), (768, 12, 65), (768, 12, 1023),
                                   (128, 12, 37), (128, 1, 37), (128, 64, 37)])
def test_the_head_is_as_close_to_fp64_as_the_fp32_restatement(full_state, D, V, n):
    state = lm_truth.state_of(full_state) if (D, V) == (768, 12) else lm_truth.head_state(D, V, 10 * D + V)
    x = features(n, D, n + V)
    wt = np.random.RandomState(n).randint(0, V, n)
    got = run(x, None, torch.from_numpy(wt), weights_of(state))
    assert got["logits"].shape == got["logp"].shape == got["scores"].shape == (n, V) and got["nll"].shape == (n,)
    check_against_truth(got, x, state, wt, f"D={D} V={V} n={n}")
    same_bits(got, run(x, None, torch.from_numpy(wt), weights_of(state)), "second run")                # two runs, the same bits


def test_gather_reads_the_chosen_rows_where_they_lie_and_nothing_else(full_state):
    state = lm_truth.state_of(full_state)
    W = weights_of(state)
    D, N = 768, 90
    wide = torch.full((N, D + 72), float("nan"), device=DEV)                  # every gap and every unselected row is NaN
    rows = [70, 3, 41, 3, 89, 0, 40, 42] + list(range(10, 37))               # out of order, row 3 twice, 35 rows: two tiles
    x = features(N, D, 1)
    sel = sorted(set(rows))
    wide[sel, 8:8 + D] = torch.from_numpy(x[sel]).to(DEV)
    view = wide[:, 8:8 + D]                                                   # ld = D + 72 > D, 32 bytes into the buffer
    assert view.stride(0) == D + 72 and view.data_ptr() % 16 == 0
    wt = np.random.RandomState(2).randint(0, 12, len(rows))
    got = run(view, rows, wt, W)
    assert all(np.isfinite(v).all() for v in got.values())
    check_against_truth(got, x[rows], state, wt, "gather")
    for k in ("logits", "logp"):
        assert got[k][1].tobytes() == got[k][3].tobytes()                     # the repeated row: equal bits
    same_bits(got, run(np.ascontiguousarray(x[rows]), None, wt, W), "gathered vs contiguous")
    n = 40
    dense = torch.from_numpy(x[:n]).to(DEV)
    wt40 = np.resize(wt, n)
    same_bits(run(dense, None, wt40, W), run(dense, torch.arange(n, dtype=torch.int32, device=DEV), wt40, W), "rows = arange")
    with pytest.raises(IndexError):
        ops.lm_head_rows(dense, [0, n], None, W)


def _raw_lone(x: torch.Tensor, wt: torch.Tensor, W: ops.LMWeights, want) -> dict:
    """rnamsm_lm_head itself on caller-made output buffers, all four pre-filled with NaN: -> every buffer after the call."""
    n, V = x.shape[0], W.V
    bufs = {k: torch.full((n,) if k == "nll" else (n, V), float("nan"), device=DEV) for k in OUTS}
    lib = _lib.load()
    ws = torch.full((lib.rnamsm_lm_head_workspace_bytes(n, W.D) // 4,), float("nan"), device=DEV)
    item = _lib.LmItem(x.data_ptr(), x.stride(0), None, wt.data_ptr(), n, *(bufs[k].data_ptr() if k in want else None for k in OUTS))
    _lib.check(lib.rnamsm_lm_head(ctypes.byref(item), W.D, V, W.ptrs, W.eps, ws.data_ptr(), ws.numel() * 4,
                                  torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def test_every_subset_of_the_outputs_has_the_bits_of_all_four_and_writes_nothing_else(full_state):
    W = weights_of(lm_truth.state_of(full_state))
    n = 37
    x = torch.from_numpy(features(n, 768, 4)).to(DEV)
    wt = torch.from_numpy(np.random.RandomState(4).randint(0, 12, n).astype(np.int32)).to(DEV)
    full = _raw_lone(x, wt, W, OUTS)
    assert all(np.isfinite(v).all() for v in full.values())
    for r in (1, 2, 3):
        for want in itertools.combinations(OUTS, r):
            got = _raw_lone(x, wt, W, want)
            for k in OUTS:
                if k in want:
                    assert got[k].tobytes() == full[k].tobytes(), (want, k)
                else:
                    assert np.isnan(got[k]).all(), (want, k)                  # not asked for: the NaN fill is still there


def test_a_wild_type_outside_the_vocabulary_gives_a_nan_row_and_touches_nothing_else(full_state):
    state = lm_truth.state_of(full_state)
    W = weights_of(state)
    n = 35
    x = features(n, 768, 5)
    wt = np.random.RandomState(5).randint(0, 12, n)
    good = run(x, None, wt, W)
    bad_wt = wt.copy()
    bad_wt[[0, 7, 33, 34]] = [-1, 12, -2 ** 31, 2 ** 31 - 1]
    got = run(x, None, bad_wt, W)
    bad = np.isin(np.arange(n), [0, 7, 33, 34])
    assert np.isnan(got["scores"][bad]).all() and np.isnan(got["nll"][bad]).all()
    assert np.isfinite(got["logits"]).all() and np.isfinite(got["logp"]).all()
    for k in ("logits", "logp"):
        assert got[k].tobytes() == good[k].tobytes()
    for k in ("scores", "nll"):
        assert got[k][~bad].tobytes() == good[k][~bad].tobytes()


def test_large_logits_keep_logp_finite_and_within_the_bars(full_state):
    state = lm_truth.state_of(full_state, proj_scale=100.0)
    n = 33
    x = features(n, 768, 6)
    wt = np.random.RandomState(6).randint(0, 12, n)
    got = run(x, None, wt, weights_of(state))
    assert np.abs(got["logits"]).max() > 100.0                               # exp() of these overflows without the max subtraction
    assert all(np.isfinite(v).all() for v in got.values())
    check_against_truth(got, x, state, wt, "projection x100")


def test_a_nan_row_and_an_inf_row_stay_to_themselves(full_state):
    W = weights_of(lm_truth.state_of(full_state))
    n = 70
    x = features(n, 768, 7)
    wt = np.random.RandomState(7).randint(0, 12, n)
    clean = run(x, None, wt, W)
    dirty = x.copy()
    dirty[5, 100], dirty[40, 767] = np.nan, np.inf                           # both inside a tile that other rows share
    got = run(dirty, None, wt, W)
    keep = ~np.isin(np.arange(n), [5, 40])
    for k in OUTS:
        assert not np.isfinite(got[k][5]).any() and not np.isfinite(got[k][40]).any(), k
        assert got[k][keep].tobytes() == clean[k][keep].tobytes(), k


def test_a_packed_member_has_the_bits_of_its_lone_call(full_state):
    W = weights_of(lm_truth.state_of(full_state))
    ns = [1, 32, 33, 200, 7]
    D, V = 768, 12
    buf = torch.from_numpy(features(sum(ns), D, 8)).to(DEV)
    starts = np.cumsum([0] + ns)
    xs = [buf[s:s + n] for s, n in zip(starts, ns)]                           # slices of one buffer
    wts = [torch.from_numpy(np.random.RandomState(b).randint(0, V, n).astype(np.int32)).to(DEV) for b, n in enumerate(ns)]
    lone = [run(x, None, w, W) for x, w in zip(xs, wts)]
    via_ops = ops.lm_head_packed(xs, None, wts, W)
    for b in range(len(ns)):
        same_bits({k: v.cpu().numpy() for k, v in via_ops[b].items()}, lone[b], f"member {b}")
    back = ops.lm_head_packed(xs[::-1], None, wts[::-1], W)[::-1]             # the order reversed: another place, the same bits
    for b in range(len(ns)):
        same_bits({k: v.cpu().numpy() for k, v in back[b].items()}, lone[b], f"reversed, member {b}")
    # the call itself on a workspace full of NaN with a word of its own behind the last slab
    lib = _lib.load()
    B = len(ns)
    nbytes = lib.rnamsm_lm_head_packed_workspace_bytes(B, (ctypes.c_int * B)(*ns), D)
    assert nbytes == 2 * 512 + sum(ns) * D * 4                                # two tables of 5 x 64 bytes, each padded to 256
    ws = torch.full((nbytes // 4 + 1,), float("nan"), device=DEV)
    guard = ws[-1:].view(torch.int32)
    guard.fill_(0x5CA1AB1E)
    outs = [{k: torch.full((n,) if k == "nll" else (n, V), float("nan"), device=DEV) for k in OUTS} for n in ns]
    items = (_lib.LmItem * B)(*(_lib.LmItem(x.data_ptr(), x.stride(0), None, w.data_ptr(), n, *(o[k].data_ptr() for k in OUTS))
                                for x, w, n, o in zip(xs, wts, ns, outs)))
    _lib.check(lib.rnamsm_lm_head_packed(items, B, D, V, W.ptrs, W.eps, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert int(guard.item()) == 0x5CA1AB1E
    for b in range(B):
        same_bits({k: v.cpu().numpy() for k, v in outs[b].items()}, lone[b], f"raw, member {b}")
