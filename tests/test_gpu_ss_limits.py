"""RNA-MSM-SS head (rnamsm_ss_head) where tiled kernels go wrong, against the fp64 restatement (tests/ss_truth.py) with the
fp32 restatement on the same pixels as the yardstick, by rel-L2 and element-wise (ss_truth.compare): L around every 16-pixel
tile seam up to a third tile, the head's limit L = 1024 and two ragged last tiles (windows of the map, exact by the receptive
margin: ss_truth.logits_window), 1, 3 and 64 blocks, LayerNorm inputs with a large common offset or constant across the
channels, both output pointers through the C ABI, base codes outside A, C, G, U, and the layouts ops.ss_head reads in place
or copies.  Bars and measured values: tests/analysis/README.md."""
import ctypes

import numpy as np
import pytest
import torch

from rnamsm import _lib, ss
import ss_truth
from test_gpu_ss_head import _case, _predictor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 16
TRUTH_DEV = "cpu"       # where the fp64 / fp32 restatements run (tests/analysis/README.md: measured against the GPU's fp64)


def _truth(x, state):
    return (ss_truth.logits(x, state, torch.float64, TRUTH_DEV),
            ss_truth.logits(x, state, torch.float32, TRUTH_DEV).astype(np.float64))


def _full_check(L, state, num_blocks, atp, seq, label, seams=False, l2_mult=ss_truth.L2_MULT):
    """Whole [L, L] map of the HIP head against fp64; returns the HIP logits."""
    got = _predictor(state, num_blocks).logits(torch.from_numpy(atp).to(DEV), seq).cpu().numpy()
    t64, t32 = _truth(ss_truth.features(atp, seq), state)
    ss_truth.compare(got, t64, t32, label, seams=seams, l2_mult=l2_mult)
    return got


SEAM_L = [3, 15, 16, 31, 32, 33, 47, 48, 49, 63, 65, 95, 97, 112, 113, 127, 128, 143]


@pytest.mark.parametrize("L", SEAM_L)
def test_tile_seams_against_fp64(L):
    """16k - 1, 16k and 16k + 1 around the second to ninth tile: the halo, the oy / ox < L store guards and the zero padding
    meet there.  Worst border and seam errors are reported beside the whole map's."""
    atp, seq = _case(L, 200 + L)
    _full_check(L, ss_truth.make_state(16, seed=300 + L), 16, atp, seq, f"L={L}", seams=True)


def _limit_windows(L, rng):
    """Up to 32 x 32: the four corners (the last two tile rows / columns, the ragged one included), a window centred on an
    interior seam crossing (16k - 16 .. 16k + 16) and one random interior tile."""
    tiles = -(-L // TILE)
    lo = TILE * (tiles - 2)                      # start of the second-to-last tile row / column
    k = int(rng.randint(2, tiles - 2))
    ty, tx = (int(v) for v in rng.randint(1, tiles - 1, size=2))
    return {"top-left": ((0, 32), (0, 32)), "top-right": ((0, 32), (lo, L)), "bottom-left": ((lo, L), (0, 32)),
            "bottom-right": ((lo, L), (lo, L)), f"seam {TILE * k}": ((TILE * k - 16, TILE * k + 16),) * 2,
            f"tile ({ty}, {tx})": ((TILE * ty, TILE * ty + TILE), (TILE * tx, TILE * tx + TILE))}


@pytest.mark.parametrize("L", [1024, 1021, 1009])
def test_at_the_limit_by_windows(L):
    """64 full tiles, a last tile 13 pixels wide, a last tile 1 pixel wide: one run of the head per L on maps made on the
    device; the fp64 truth of each window from its crop alone (exact: tests/test_ss_truth.py)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(L)
    atp = torch.empty(120, L, L, device=DEV).exponential_(generator=g)
    atp /= atp.sum(-1, keepdim=True)
    rng = np.random.RandomState(L)
    seq = "".join(rng.choice(list("ACGUN"), L))
    state = ss_truth.make_state(16, seed=L)
    got = _predictor(state, 16).logits(atp, seq)
    for name, (rows, cols) in _limit_windows(L, rng).items():
        assert 0 < rows[1] - rows[0] <= 32 and 0 < cols[1] - cols[0] <= 32
        t64 = ss_truth.logits_window(atp, seq, state, rows, cols, torch.float64, TRUTH_DEV)
        t32 = ss_truth.logits_window(atp, seq, state, rows, cols, torch.float32, TRUTH_DEV)
        ss_truth.compare(got[rows[0]:rows[1], cols[0]:cols[1]].cpu().numpy(), t64, t32, f"L={L} {name} {rows} x {cols}")


@pytest.mark.parametrize("num_blocks", [1, 3, 64])
@pytest.mark.parametrize("L", [33, 49])
def test_block_counts_against_fp64(num_blocks, L):
    atp, seq = _case(L, 400 + L)
    _full_check(L, ss_truth.make_state(num_blocks, seed=num_blocks), num_blocks, atp, seq, f"B={num_blocks} L={L}")


def test_layernorm_input_with_a_large_common_offset():
    """A stem bias 1e3 above zero on every channel: the residual stream carries the offset into every LayerNorm.  E[v^2] -
    mean^2 in fp32 cancels catastrophically there; the two-pass variance (and both restatements) does not."""
    state = ss_truth.make_state(4, seed=21)
    state["conv1.bias"] = state["conv1.bias"] + np.float32(1000.0)
    atp, seq = _case(40, 22)
    _full_check(40, state, 4, atp, seq, "offset 1e3")


def test_layernorm_input_constant_across_the_channels():
    """Exactly constant LayerNorm inputs: the stem has zero weights over the 120 map channels and one bias for all 48
    channels, so every pixel whose 3 x 3 neighbourhood has unknown row and column bases is that bias alone; block 1 has
    all-zero 3x3 weights, so its t is 0 everywhere.  LN then gives relu(beta) -- eps inside the square root, no NaN."""
    state = ss_truth.make_state(3, seed=23, beta_scale=1.0)
    w = state["conv1.weight"].copy()
    w[:, 8:] = 0.0
    state["conv1.weight"] = w
    state["conv1.bias"] = np.full(48, 0.75, dtype=np.float32)
    state["layer1.1.conv1.weight"] = np.zeros_like(state["layer1.1.conv1.weight"])
    L = 41
    atp, seq = _case(L, 24)
    seq = seq[:8] + "N" * 20 + seq[28:]                          # rows / columns 9..26: constant stem output
    assert not ss_truth.features(atp, seq)[:8, 8:28, 8:28].any()
    # rel-L2 at 4 x, not 2 x: the FINDING of the tolerance table -- the kernel's mean s * fl(1/48) is not exactly the constant,
    # and 1/sqrt(eps) amplifies that rounding on flat pixels (torch's fp32 LayerNorm returns beta exactly there)
    _full_check(L, state, 3, atp, seq, "constant LN input", l2_mult=4.0)


def test_logits_and_probs_together_through_the_c_abi():
    """Both output pointers at once give the bits of each alone; probs is sigmoid(logits) within the sigmoid's own slope
    (<= 1/4) times the logits' error plus a few fp32 roundings."""
    L, nb = 49, 4
    state = ss_truth.make_state(nb, seed=31)
    model = _predictor(state, nb)
    atp, seq = _case(L, 32)
    a = torch.from_numpy(atp).to(DEV)
    codes = torch.from_numpy(ss.base_codes(seq)).to(DEV)
    lib = _lib.load()
    ptrs, _ = model._packed_weights()
    ws = torch.empty(lib.rnamsm_ss_head_workspace_bytes(L), dtype=torch.uint8, device=DEV)
    lg = torch.full((L, L), float("nan"), device=DEV)
    pr = torch.full((L, L), float("nan"), device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    assert lib.rnamsm_ss_head(a.data_ptr(), L * L, codes.data_ptr(), L, nb, ptrs, lg.data_ptr(), pr.data_ptr(), ws.data_ptr(),
                              ws.numel(), s) == 0
    lg, pr = lg.cpu().numpy(), pr.cpu().numpy()
    alone_l = model.logits(a, seq).cpu().numpy()
    alone_p = model.predict(a, seq).cpu().numpy()
    assert np.array_equal(lg.view(np.uint32), alone_l.view(np.uint32))
    assert np.array_equal(pr.view(np.uint32), alone_p.view(np.uint32))
    t64, t32 = _truth(ss_truth.features(atp, seq), state)
    err = ss_truth.compare(lg, t64, t32, "logits")
    p64 = 1.0 / (1.0 + np.exp(-t64))
    perr = float(np.abs(pr.astype(np.float64) - p64).max())
    print(f"probs max-abs vs fp64 sigmoid {perr:.2e} (bar {0.25 * err + 5e-7:.2e})")
    assert perr <= 0.25 * err + 5e-7


def test_num_blocks_refusals():
    """num_blocks 0 and 65 (RNAMSM_SS_MAX_BLOCKS = 64): -1 and nothing launched; SSPredictor refuses them too."""
    for nb in (0, 65):
        with pytest.raises(ValueError, match="num_blocks"):
            ss.SSPredictor(nb)
    L = 20
    model = _predictor(ss_truth.make_state(1, seed=41), 1)
    ptrs, _ = model._packed_weights()
    stem, block, head = list(ptrs[:4]), list(ptrs[4:10]), list(ptrs[10:12])
    atp, seq = _case(L, 42)
    a = torch.from_numpy(atp).to(DEV)
    codes = torch.from_numpy(ss.base_codes(seq)).to(DEV)
    lib = _lib.load()
    ws = torch.empty(lib.rnamsm_ss_head_workspace_bytes(L), dtype=torch.uint8, device=DEV)
    out = torch.full((L, L), float("nan"), device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    for nb in (0, 65):
        table = stem + block * nb + head           # valid pointers for every block the count names
        arr = (ctypes.c_void_p * len(table))(*table)
        assert lib.rnamsm_ss_head(a.data_ptr(), L * L, codes.data_ptr(), L, nb, arr, out.data_ptr(), None, ws.data_ptr(),
                                  ws.numel(), s) == -1
        assert b"num_blocks" in lib.rnamsm_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


@pytest.mark.parametrize("kind", ["all 255", "codes 4..254"])
def test_unknown_base_codes_against_fp64(kind):
    L = 35
    atp, _ = _case(L, 51)
    rng = np.random.RandomState(52)
    codes = np.full(L, 255, np.uint8) if kind == "all 255" else rng.randint(4, 255, size=L).astype(np.uint8)
    state = ss_truth.make_state(4, seed=53)
    got = _predictor(state, 4).logits(torch.from_numpy(atp).to(DEV), torch.from_numpy(codes).to(DEV)).cpu().numpy()
    t64, t32 = _truth(ss_truth.features(atp, codes), state)
    ss_truth.compare(got, t64, t32, kind)


@pytest.mark.parametrize("base", list("ACGU"))
def test_single_base_against_fp64(base):
    """L = 1: the one pixel sees only its own base's one-hot planes (zero padding all around); a wrong code is off by O(0.1)."""
    atp = np.ones((120, 1, 1), dtype=np.float32)
    state = ss_truth.make_state(4, seed=61)
    got = _predictor(state, 4).logits(torch.from_numpy(atp).to(DEV), base).cpu().numpy()
    t64, t32 = _truth(ss_truth.features(atp, base), state)
    ss_truth.compare(got, t64, t32, f"L=1 {base}", floor=2.0 ** -20)     # one pixel: 16 fp32 ulps (README tolerance table)


def test_input_layouts_give_the_same_bits():
    """Member b > 0 of a [B, 120, L, L] buffer (read in place at its offset) and a [120, L, L] view cut from a
    [120, L + 3, L + 3] frame (row stride != L: ops.ss_head copies it) give the bits of the contiguous maps."""
    L = 37
    atp, seq = _case(L, 71)
    model = _predictor(ss_truth.make_state(2, seed=72), 2)
    want = model.logits(torch.from_numpy(atp).to(DEV), seq).cpu().numpy()
    buf = torch.full((3, 120, L, L), float("nan"), device=DEV)
    buf[2] = torch.from_numpy(atp)
    member = buf[2]
    assert member.is_contiguous() and member.storage_offset() == 2 * 120 * L * L
    frame = torch.full((120, L + 3, L + 3), float("nan"), device=DEV)
    frame[:, 1:L + 1, 2:L + 2] = torch.from_numpy(atp)
    view = frame[:, 1:L + 1, 2:L + 2]
    assert view.stride(1) == L + 3
    for name, t in (("batch member", member), ("framed view", view)):
        got = model.logits(t, seq).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
