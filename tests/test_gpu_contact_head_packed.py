"""The contact head on the stripped maps, lone and packed (rnamsm_contact_head_atp, rnamsm_contact_head_packed): every result the
BITS of rnamsm_contact_head on the un-stripped [nch, L+1, L+1] maps of that alignment alone -- whatever the member's company, its
place in the batch, its plane stride and the contents of the workspace.  Bits are compared as int32, so that a NaN compares too.
The anchor that does not depend on the code under test is the fp64 oracle at L = 257, under the bar of
test_gpu_forward.py::test_contact_head_kernel_on_random_maps_with_large_weights."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import msm_oracle as O
from rnamsm import _lib, ops, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LONE_LS = (1, 2, 31, 32, 33, 255, 256, 257)      # the 32-tile seam of the regression, the 256-row stride of the sums
NCHS = (120, 7)
_cache = {}


def _maps(L: int, nch: int, tag: str = "") -> torch.Tensor:
    """Softmax-like [nch, L+1, L+1] maps on the device (the existing kernel test's recipe), made once per (L, nch, tag)."""
    key = (L, nch, tag)
    if key not in _cache:
        C = L + 1
        _cache[key] = torch.softmax(torch.from_numpy(synthetic.normal(f"ct{tag}{C}_{nch}", 5, (nch, C, C))).float() * 3, -1).to(DEV)
    return _cache[key]


def _regression(nch: int):
    """O(1) regression weights: the synthetic checkpoint's are small and would leave every contact near 0.5."""
    w = torch.from_numpy(synthetic.normal(f"ctw{nch}", 5, (1, nch))).float() * 20
    return w.to(DEV), torch.tensor([0.3], device=DEV)


def _strip(maps: torch.Tensor) -> torch.Tensor:
    return maps[:, 1:, 1:].contiguous()


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _same_bits(got: torch.Tensor, want: torch.Tensor, what) -> None:
    assert got.shape == want.shape and got.dtype == torch.float32, what
    g, w = _bits(got), _bits(want)
    assert np.array_equal(g, w), (what, int((g != w).sum()), float(np.nanmax(np.abs(got.cpu().numpy() - want.cpu().numpy()))))


def _lone(maps: torch.Tensor, w, b) -> torch.Tensor:
    """The yardstick: the existing entry point on the un-stripped maps of one alignment."""
    return ops.contact_head(maps, w, b)


# ------------------------------------------------------------------ the lone entry on the stripped maps
@pytest.mark.parametrize("nch", NCHS)
@pytest.mark.parametrize("L", LONE_LS)
def test_atp_entry_has_the_bits_of_the_unstripped_entry(L, nch):
    maps, (w, b) = _maps(L, nch), _regression(nch)
    want = _lone(maps, w, b)
    got = ops.contact_head_atp(_strip(maps), w, b)
    assert got.shape == (L, L)
    _same_bits(got, want, (L, nch))
    if L == 257:         # the anchor outside the code under test
        ref = O.contact_head(maps.cpu().double(), w.cpu().double(), b.cpu().double()).numpy()
        err = float(np.abs(got.cpu().numpy() - ref).max())
        print(f"L = 257, nch = {nch}: max |contact_head_atp - fp64 oracle| = {err:.3e}")
        assert err < 2e-5, (nch, err)


def test_atp_entry_reads_planes_of_a_wider_buffer_in_place():
    L, nch = 33, 7
    maps, (w, b) = _maps(L, nch), _regression(nch)
    stride = L * L + 5
    buf = torch.full((nch * stride,), float("nan"), device=DEV)
    view = buf.as_strided((nch, L, L), (stride, L, 1))
    view.copy_(_strip(maps))
    got = ops.contact_head_atp(view, w, b)
    _same_bits(got, _lone(maps, w, b), "strided planes")
    # the library itself on the view's own pointer and stride: the planes are read where they lie
    lib = _lib.load()
    ws = torch.empty(lib.rnamsm_contact_head_workspace_bytes(L + 1, nch), dtype=torch.uint8, device=DEV)
    out = torch.empty(L, L, device=DEV)
    _lib.check(lib.rnamsm_contact_head_atp(view.data_ptr(), stride, L, nch, w.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                           ws.numel(), torch.cuda.current_stream().cuda_stream))
    _same_bits(out, got, "library, strided planes")


# ------------------------------------------------------------------ the packed call
def _packed_raw(atps, strides, Ls, nch, w, b, tail: int = 256):
    """rnamsm_contact_head_packed itself on a NaN-filled workspace with `tail` guard bytes of 0xA5 behind the last slab.
    -> the members' outputs (each prefilled with NaN), the guard bytes after the call."""
    lib = _lib.load()
    B = len(Ls)
    nbytes = lib.rnamsm_contact_head_packed_workspace_bytes(B, (ctypes.c_int * B)(*Ls), nch)
    assert nbytes == -(-B * 64 // 256) * 256 + sum(4 * (nch * L + nch) for L in Ls)
    ws = torch.empty(nbytes + tail, dtype=torch.uint8, device=DEV)
    ws[:nbytes].view(torch.float32).fill_(float("nan"))
    ws[nbytes:] = 0xA5
    outs = [torch.full((L, L), float("nan"), device=DEV) for L in Ls]
    items = (_lib.ContactItem * B)(*(_lib.ContactItem(a.data_ptr(), s, L, o.data_ptr()) for a, s, L, o in zip(atps, strides, Ls, outs)))
    _lib.check(lib.rnamsm_contact_head_packed(items, B, nch, w.data_ptr(), b.data_ptr(), ws.data_ptr(), nbytes,
                                              torch.cuda.current_stream().cuda_stream))
    return outs, ws[nbytes:].cpu()


@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("nch", NCHS)
def test_packed_members_have_their_lone_bits_in_both_orders(nch, order):
    Ls = [1, 33, 257, 32, 2]
    if order == "reversed":
        Ls = Ls[::-1]
    w, b = _regression(nch)
    maps = [_maps(L, nch) for L in Ls]
    got = ops.contact_head_packed([_strip(m) for m in maps], w, b)
    assert len(got) == len(Ls)
    for k, (g, m) in enumerate(zip(got, maps)):
        _same_bits(g, _lone(m, w, b), (order, k, Ls[k]))
    # the library itself: a NaN-filled workspace, nothing written behind the last slab
    atps = [_strip(m) for m in maps]
    raw, guard = _packed_raw(atps, [L * L for L in Ls], Ls, nch, w, b)
    for k, (g, r) in enumerate(zip(got, raw)):
        _same_bits(r, g, ("raw", order, k))
    assert bool((guard == 0xA5).all())


def test_packed_more_members_than_one_descriptor_launch():
    nch = 7
    Ls = list(range(5, 38))                     # 33 members: the table goes up in two launches
    w, b = _regression(nch)
    maps = [_maps(L, nch) for L in Ls]
    got = ops.contact_head_packed([_strip(m) for m in maps], w, b)
    for k, (g, m) in enumerate(zip(got, maps)):
        _same_bits(g, _lone(m, w, b), (k, Ls[k]))


def test_packed_neighbours_do_not_reach_a_member():
    """Neighbours scaled by 1e6 and one all-NaN neighbour: every member keeps the bits of its own lone call (the NaN member's are NaN
    there too)."""
    nch = 120
    Ls = [33, 257, 32, 2, 31]
    w, b = _regression(nch)
    maps = [_maps(L, nch).clone() for L in Ls]
    maps[0] *= 1e6
    maps[2] *= 1e6
    maps[3].fill_(float("nan"))
    got = ops.contact_head_packed([_strip(m) for m in maps], w, b)
    for k, (g, m) in enumerate(zip(got, maps)):
        _same_bits(g, _lone(m, w, b), (k, Ls[k]))
    assert bool(torch.isnan(got[3]).all())
    for k in (1, 4):                             # the unscaled members are the plain case's
        assert bool(torch.isfinite(got[k]).all())
        _same_bits(got[k], _lone(_maps(Ls[k], nch), w, b), ("plain", k))


def test_packed_members_as_slices_of_one_buffer_with_nan_in_the_gaps():
    nch = 7
    Ls = [33, 2, 257, 1, 32]
    w, b = _regression(nch)
    maps = [_maps(L, nch) for L in Ls]
    pads = [3, 1, 7, 2, 5]
    strides = [L * L + p for L, p in zip(Ls, pads)]
    starts = np.concatenate([[0], np.cumsum([nch * s for s in strides])])
    buf = torch.full((int(starts[-1]) + 11,), float("nan"), device=DEV)
    views = []
    for m, L, s, st in zip(maps, Ls, strides, starts):
        v = buf[int(st):int(st) + nch * s].as_strided((nch, L, L), (s, L, 1))
        v.copy_(_strip(m))
        views.append(v)
    got = ops.contact_head_packed(views, w, b)
    for k, (g, m) in enumerate(zip(got, maps)):
        _same_bits(g, _lone(m, w, b), (k, Ls[k]))
    raw, guard = _packed_raw(views, strides, Ls, nch, w, b)       # read in place: the views' own pointers and strides
    for k, (g, r) in enumerate(zip(got, raw)):
        _same_bits(r, g, ("raw", k))
    assert bool((guard == 0xA5).all())


# ------------------------------------------------------------------ refusals
def test_refusals_name_the_member_and_leave_the_outputs_untouched():
    lib = _lib.load()
    nch, Ls = 7, [5, 9, 3]
    w, b = _regression(nch)
    atps = [_strip(_maps(L, nch)) for L in Ls]
    outs = [torch.full((L, L), -7.0, device=DEV) for L in Ls]
    nbytes = lib.rnamsm_contact_head_packed_workspace_bytes(3, (ctypes.c_int * 3)(*Ls), nch)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def items(change=None, n=3):
        rows = [[a.data_ptr(), L * L, L, o.data_ptr()] for a, L, o in zip(atps, Ls, outs)]
        if change:
            k, field, value = change
            rows[k][field] = value
        rows = (rows * (n // 3 + 1))[:n]
        return (_lib.ContactItem * n)(*(_lib.ContactItem(*r) for r in rows))

    def refused(rc, *words):
        assert rc == -1, rc                                        # RNAMSM_ERR_INVALID
        msg = lib.rnamsm_last_error().decode()
        assert "contact_head_packed" in msg and all(x in msg for x in words), msg

    call = lib.rnamsm_contact_head_packed
    refused(call(items(), 0, nch, w.data_ptr(), b.data_ptr(), ws.data_ptr(), nbytes, stream), "B=0")
    refused(call(items(n=1025), 1025, nch, w.data_ptr(), b.data_ptr(), ws.data_ptr(), 1 << 40, stream), "B=1025")
    refused(call(items((1, 2, 0)), 3, nch, w.data_ptr(), b.data_ptr(), ws.data_ptr(), nbytes, stream), "member 1", "L=0")
    refused(call(items((2, 2, 1024)), 3, nch, w.data_ptr(), b.data_ptr(), ws.data_ptr(), 1 << 40, stream), "member 2", "L=1024")
    refused(call(items(), 3, 0, w.data_ptr(), b.data_ptr(), ws.data_ptr(), nbytes, stream), "nch=0")
    refused(call(items(), 3, -3, w.data_ptr(), b.data_ptr(), ws.data_ptr(), nbytes, stream), "nch=-3")
    refused(call(None, 3, nch, w.data_ptr(), b.data_ptr(), ws.data_ptr(), nbytes, stream), "null")
    refused(call(items(), 3, nch, None, b.data_ptr(), ws.data_ptr(), nbytes, stream), "null")
    refused(call(items(), 3, nch, w.data_ptr(), None, ws.data_ptr(), nbytes, stream), "null")
    refused(call(items(), 3, nch, w.data_ptr(), b.data_ptr(), None, nbytes, stream), "null")
    refused(call(items((1, 0, None)), 3, nch, w.data_ptr(), b.data_ptr(), ws.data_ptr(), nbytes, stream), "member 1", "null")
    refused(call(items((2, 3, None)), 3, nch, w.data_ptr(), b.data_ptr(), ws.data_ptr(), nbytes, stream), "member 2", "null")
    refused(call(items((1, 1, 80)), 3, nch, w.data_ptr(), b.data_ptr(), ws.data_ptr(), nbytes, stream), "member 1", "plane stride")
    refused(call(items(), 3, nch, w.data_ptr(), b.data_ptr(), ws.data_ptr(), nbytes - 1, stream), "workspace too small")
    # the lone entry's own refusals
    lone, a0, o0 = lib.rnamsm_contact_head_atp, atps[0], outs[0]
    lone_bytes = lib.rnamsm_contact_head_workspace_bytes(Ls[0] + 1, nch)

    def lone_refused(rc, *words):
        assert rc == -1, rc
        msg = lib.rnamsm_last_error().decode()
        assert "contact_head_atp" in msg and all(x in msg for x in words), msg

    lone_refused(lone(a0.data_ptr(), 25, 0, nch, w.data_ptr(), b.data_ptr(), o0.data_ptr(), ws.data_ptr(), nbytes, stream), "L=0")
    lone_refused(lone(a0.data_ptr(), 1 << 21, 1024, nch, w.data_ptr(), b.data_ptr(), o0.data_ptr(), ws.data_ptr(), 1 << 40, stream), "L=1024")
    lone_refused(lone(a0.data_ptr(), 25, 5, 0, w.data_ptr(), b.data_ptr(), o0.data_ptr(), ws.data_ptr(), nbytes, stream), "nch=0")
    lone_refused(lone(None, 25, 5, nch, w.data_ptr(), b.data_ptr(), o0.data_ptr(), ws.data_ptr(), nbytes, stream), "null")
    lone_refused(lone(a0.data_ptr(), 25, 5, nch, w.data_ptr(), b.data_ptr(), None, ws.data_ptr(), nbytes, stream), "null")
    lone_refused(lone(a0.data_ptr(), 24, 5, nch, w.data_ptr(), b.data_ptr(), o0.data_ptr(), ws.data_ptr(), nbytes, stream), "plane stride")
    lone_refused(lone(a0.data_ptr(), 25, 5, nch, w.data_ptr(), b.data_ptr(), o0.data_ptr(), ws.data_ptr(), lone_bytes - 1, stream),
                 "workspace too small")
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs)              # nothing was enqueued
    assert lib.rnamsm_contact_head_packed_workspace_bytes(0, (ctypes.c_int * 3)(*Ls), nch) == 0
    assert lib.rnamsm_contact_head_packed_workspace_bytes(3, None, nch) == 0
    assert lib.rnamsm_contact_head_packed_workspace_bytes(3, (ctypes.c_int * 3)(5, 1024, 3), nch) == 0
    assert lib.rnamsm_contact_head_packed_workspace_bytes(3, (ctypes.c_int * 3)(*Ls), 0) == 0
    # the Python layer refuses too
    with pytest.raises(ValueError):
        ops.contact_head_packed([atps[0][:5], atps[1]], w, b)       # unlike channel counts
    assert ops.contact_head_packed([], w, b) == []


# ------------------------------------------------------------------ the model's batch
def test_forward_return_contacts_on_a_batch_equals_the_lone_forwards():
    from rnamsm.model import MSATransformer
    state = synthetic.make_state_dict(seed=0)
    m = MSATransformer(num_layers=10)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    m = m.eval().to(DEV)
    toks = torch.stack([torch.from_numpy(synthetic.make_tokens(4, 9, seed)) for seed in (1, 2, 3)]).to(DEV)
    assert toks.shape == (3, 4, 9)
    calls = []
    real = ops.contact_head_packed
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(ops, "contact_head_packed", lambda atps, *a, **k: calls.append(len(atps)) or real(atps, *a, **k))
        with torch.no_grad():
            batch = m(toks, return_contacts=True)["contacts"]
    finally:
        mp.undo()
    assert calls == [3] and batch.shape == (3, 8, 8)
    with torch.no_grad():
        for k in range(3):
            _same_bits(batch[k], m(toks[k:k + 1], return_contacts=True)["contacts"][0], k)
