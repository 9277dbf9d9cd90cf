"""The bf16 SS head (rnamsm_ss_head16, rnamsm_ss_head16_packed) held to its arithmetic contract stage by stage: tests/ss16_contract.py
applied to the head's OWN intermediate images, read from the workspace the test hands to the C entry point.

Teacher forcing with prefix block counts: the head's bits do not change from run to run (test_gpu_ss_head16.py), so a run with k
blocks leaves X_k -- the residual image after k blocks -- in the workspace's first image, and a run with k + 1 blocks (the same
first k blocks' weights) leaves T_{k+1} in the second and X_{k+1} in the first.  X_0, the stem's output, comes from a 1-block run
whose 5x5 weights are zero (X_1 = 0 + X_0); that run's T_1 has the bits of the ordinary 1-block run's.  Every stage is then the
contract applied to the head's own input image of that stage, so nothing cascades: stem, each block's 3x3 (T_{k+1} from X_k) and
5x5 + residual (X_{k+1} from T_{k+1} and X_k), the output pass (logits from X_nb).  tests/test_ss16_contract_host.py shows on the
CPU that the same calls fail every breach of the contract.  Measured values: tests/analysis/README.md."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from rnamsm import _lib, ss
import ss16_contract as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CH = 48
NB = C.CASE_BLOCKS


def _predictor(state, num_blocks):
    m = ss.SSPredictor(num_blocks, gemm_dtype="bf16")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV)


def _prefix_table(model, k):
    """The weight table of the first k blocks of `model`: stem, k blocks, fc1 (include/rnamsm.h)."""
    ptrs, _ = model._packed_weights()
    vals = [ptrs[i] for i in range(len(ptrs))]
    ns, nblk = len(_lib.W_SS_STEM), len(_lib.W_SS_BLOCK)
    assert len(vals) == ns + nblk * model.num_blocks + len(_lib.W_SS_HEAD)
    sel = vals[:ns + nblk * k] + vals[-len(_lib.W_SS_HEAD):]
    return (ctypes.c_void_p * len(sel))(*sel)


def _zero_5x5(state):
    """The 1-block prefix of `state` with block 0's 5x5 weights zero."""
    out = {k: v for k, v in state.items() if not k.startswith("layer1.") or k.startswith("layer1.0.")}
    out["layer1.0.conv2.weight"] = np.zeros_like(state["layer1.0.conv2.weight"])
    return out


def _run(table, nb, a, codes):
    """One lone call on the test's own workspace -> (logits [L, L], X [L, L, 48], T [L, L, 48]): views of device tensors; the
    workspace holds the residual image first and the middle image second (ss16_launch)."""
    lib = _lib.load()
    L = a.shape[-1]
    assert a.stride(1) == L and a.stride(2) == 1
    ws = torch.full((lib.rnamsm_ss_head16_workspace_bytes(L) // 4,), float("nan"), device=DEV)
    assert ws.numel() == 2 * L * L * CH
    lg = torch.full((L, L), float("nan"), device=DEV)
    rc = lib.rnamsm_ss_head16(a.data_ptr(), a.stride(0), codes.data_ptr(), L, nb, table, lg.data_ptr(), None, ws.data_ptr(),
                              ws.numel() * 4, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.rnamsm_last_error().decode()
    torch.cuda.synchronize()
    imgs = ws.view(2, L, L, CH)
    return lg, imgs[0], imgs[1]


def _chw(img, rows=None, cols=None):
    """A device image [L, L, 48] (or its crop) -> host [48, H, W]."""
    if rows is not None:
        img = img[rows[0]:rows[1], cols[0]:cols[1]]
    return img.permute(2, 0, 1).contiguous().cpu()


def _same_bits(a, b):
    """Bit identity of two fp32 device tensors of one size (NaN payloads and signed zeros included), compared where they lie."""
    return a.numel() == b.numel() and torch.equal(a.contiguous().view(torch.int32).reshape(-1), b.contiguous().view(torch.int32).reshape(-1))


def _chain_runs(state, atp, seq, nb):
    """The nb + 1 runs of a case -> (images X0, T1, X1, ..., on the device, [L, L, 48]; the logits of every ordinary run)."""
    a = atp if isinstance(atp, torch.Tensor) else torch.from_numpy(atp).to(DEV)
    codes = torch.from_numpy(C.codes_of(seq)).to(DEV)
    model, zero = _predictor(state, nb), _predictor(_zero_5x5(state), 1)
    _, x0, t1z = _run(_prefix_table(zero, 1), 1, a, codes)
    images, logits = {"X0": x0}, {}
    for k in range(1, nb + 1):
        logits[k], images[f"X{k}"], images[f"T{k}"] = _run(_prefix_table(model, k), k, a, codes)
    assert _same_bits(t1z, images["T1"]), "T_1 of the zero-weight run differs from the ordinary run's"
    assert not _same_bits(x0, images["X1"])
    return images, logits


# ---------------------------------------------------------------------- the small cases
@functools.lru_cache(maxsize=None)
def _cases():
    return C.small_cases()


@pytest.mark.parametrize("label", list(C.small_cases()))
def test_every_stage_holds_the_contract(label):
    L, state, atp, seq = _cases()[label]
    dev, logits = _chain_runs(state, atp, seq, NB)
    images = {k: _chw(v) for k, v in dev.items()}
    lg = {k: v.cpu() for k, v in logits.items()}
    # the reading of the workspace: the first image is the residual stream, the second is not
    assert C.check_out(lg[NB], images[f"X{NB}"], state, f"{label} output pass of the first image").passed
    assert not C.check_out(lg[NB], images[f"T{NB}"], state, f"{label} output pass of the SECOND image", assert_=False).passed
    # the same pass on the 1-block run's image: asserted from 225 pixels on.  At L = 1 and L = 2 the yardstick's rel-L2 is 1 and 4
    # rounding samples (under ss_truth's floor: the L = 1 row of the tolerance table); measured there 2.04e-7 against a bar of 2.00e-7
    (C.check_out if L >= 15 else functools.partial(C.check_out, assert_=False))(
        lg[1], images["X1"], state, f"{label} output pass after 1 block")
    reps = C.check_chain(images, C.features32(atp, seq), state, NB, label, logits=lg[NB])
    assert len(reps) == 2 + 2 * NB and all(r.passed for r in reps)


def test_a_padded_plane_stride_gives_the_same_stem_bits():
    L, state, atp, seq = _cases()["L=17"]
    a = torch.from_numpy(atp).to(DEV)
    wide = torch.full((120, L * L + 13), float("nan"), device=DEV)
    wide[:, :L * L] = a.reshape(120, -1)
    view = wide[:, :L * L].view(120, L, L)
    assert view.stride() == (L * L + 13, L, 1)
    codes = torch.from_numpy(C.codes_of(seq)).to(DEV)
    zero = _predictor(_zero_5x5(state), 1)
    table = _prefix_table(zero, 1)
    lg_v, x0_v, t1_v = _run(table, 1, view, codes)
    lg_c, x0_c, t1_c = _run(table, 1, a, codes)
    assert torch.isfinite(x0_v).all()
    for name, v, c in (("X_0", x0_v, x0_c), ("T_1", t1_v, t1_c), ("logits", lg_v, lg_c)):
        assert _same_bits(v, c), name
    C.check_stem(_chw(x0_v), C.features32(atp, seq), state, "strided view, stem")


# ---------------------------------------------------------------------- the limit
TILE = 16


def _limit_windows(L):
    """16 x 16 windows (the ragged last tile: 16 x 13): the four corners, whose far ones are the last tile, and an interior seam
    crossing (rows 504..519 x columns 520..535: the seams at row 512 and column 528)."""
    lo = TILE * ((L - 1) // TILE)                         # 1008: the last tile's first row / column
    return {"top-left": ((0, 16), (0, 16)), "top-right": ((0, 16), (lo, L)), "bottom-left": ((lo, L), (0, 16)),
            "bottom-right (the last tile)": ((lo, L), (lo, L)), "interior seam": ((504, 520), (520, 536))}


@pytest.mark.parametrize("L", [1024, 1021])
def test_at_the_limit_by_windows(L):
    """One block at the head's limit and at a ragged last tile: the zero-weight run and the ordinary run on maps made on the device;
    each window's stages from crops that hold the window and a two-pixel halo (exact: teacher forcing needs no more)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(L)
    atp = torch.empty(120, L, L, device=DEV).exponential_(generator=g)
    atp /= atp.sum(-1, keepdim=True)
    seq = "".join(np.random.RandomState(L).choice(list("ACGUN"), L))
    state = C.limit_state()
    dev, logits = _chain_runs(state, atp, seq, 1)
    assert 2 * L * L * CH * 4 > 2 ** 28                    # 400 MB of workspace: the pixel offsets pass 2^27 floats
    for name, (rows, cols) in _limit_windows(L).items():
        (R0, R1), (C0, C1), inner = C.region(L, rows, cols)
        images = {k: _chw(v, (R0, R1), (C0, C1)) for k, v in dev.items()}
        feat = C.features32(atp[:, R0:R1, C0:C1], seq, (R0, R1), (C0, C1))
        lg = logits[1][R0:R1, C0:C1].cpu()
        reps = C.check_chain(images, feat, state, 1, f"L={L} {name} {rows} x {cols}", inner, logits=lg)
        assert len(reps) == 4 and all(r.passed for r in reps)


# ---------------------------------------------------------------------- the packed call
def test_a_packed_member_s_images_have_the_lone_call_s_bits():
    """rnamsm_ss_head16_packed with Ls (17, 1, 35): member b's two images lie pix0 x 48 floats behind the descriptor table, in the
    first and in the second image of the whole batch.  A pix0 or tile0 slip that cancels in the logits shows here."""
    lib = _lib.load()
    Ls = (17, 1, 35)
    state = _cases()["L=35"][1]
    model = _predictor(state, NB)
    table = _prefix_table(model, NB)
    members = [C.case(L, 300 + i) for i, L in enumerate(Ls)]
    atps = [torch.from_numpy(a).to(DEV) for a, _ in members]
    codes = [torch.from_numpy(C.codes_of(s)).to(DEV) for _, s in members]
    B, pixels = len(Ls), sum(L * L for L in Ls)
    total = lib.rnamsm_ss_head16_packed_workspace_bytes(B, (ctypes.c_int * B)(*Ls))
    table_bytes = total - 2 * pixels * CH * 4              # ss_members_bytes(B): the size function's own difference
    assert table_bytes >= 64 * B and table_bytes % 256 == 0
    ws = torch.full((total // 4,), float("nan"), device=DEV)
    outs = [torch.full((L, L), float("nan"), device=DEV) for L in Ls]
    items = (_lib.SsItem * B)()
    for b, L in enumerate(Ls):
        items[b] = _lib.SsItem(atps[b].data_ptr(), L * L, codes[b].data_ptr(), L, outs[b].data_ptr(), None)
    rc = lib.rnamsm_ss_head16_packed(items, B, NB, table, ws.data_ptr(), total, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.rnamsm_last_error().decode()
    torch.cuda.synchronize()
    imgs = ws[table_bytes // 4:].view(2, pixels, CH)
    pix0 = 0
    for b, L in enumerate(Ls):
        lg, x, t = _run(table, NB, atps[b], codes[b])
        assert torch.isfinite(x).all() and torch.isfinite(t).all()
        for name, got, want in (("X", imgs[0, pix0:pix0 + L * L], x), ("T", imgs[1, pix0:pix0 + L * L], t), ("logits", outs[b], lg)):
            assert _same_bits(got, want), f"member {b} (L={L}): {name}"
        pix0 += L * L
