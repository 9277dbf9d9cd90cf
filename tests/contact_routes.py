"""The contact head's entry points called through the C ABI on a workspace the test owns, so that the stages the kernels leave there
can be read after the call (include/rnamsm.h: a member's slab is rs [nch, T], then tot [nch]; packed, the slabs follow the
256-byte-padded descriptor table in member order).  Every workspace is NaN-filled before the call and followed by guard bytes.
For tests/test_gpu_contact_head_stages.py and tests/test_gpu_contact_head_nonfinite.py.  Test infrastructure only."""
import ctypes

import numpy as np
import torch

from rnamsm import _lib

DEV = "cuda:0"
GUARD = 256
NAN = float("nan")


def _workspace(nbytes: int) -> torch.Tensor:
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
    ws[:nbytes].view(torch.float32).fill_(NAN)
    ws[nbytes:] = 0xA5
    return ws


def _slab(ws: torch.Tensor, start: int, T: int, nch: int):
    """(rs [nch, T], tot [nch]) as numpy, from the slab that begins `start` bytes into ws."""
    f = ws[start:start + 4 * (nch * T + nch)].view(torch.float32).cpu().numpy()
    return f[:nch * T].reshape(nch, T).copy(), f[nch * T:].copy()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def strided(atp: np.ndarray, pad: int) -> torch.Tensor:
    """The planes on the device `pad` floats apart beyond T * T, the gaps NaN: a [nch, T, T] view of the wider buffer."""
    nch, T = atp.shape[0], atp.shape[-1]
    wide = torch.full((nch, T * T + pad), NAN, device=DEV)
    wide[:, :T * T] = torch.from_numpy(atp).to(DEV).reshape(nch, T * T)
    return wide[:, :T * T].view(nch, T, T)


def gaps_untouched(view: torch.Tensor) -> bool:
    nch, T = view.shape[0], view.shape[-1]
    pad = view.stride(0) - T * T
    if pad == 0:
        return True
    wide = torch.as_strided(view, (nch, T * T + pad), (view.stride(0), 1))
    return bool(torch.isnan(wide[:, T * T:]).all())


def lone(route: str, atp, weight: np.ndarray, bias: np.ndarray) -> dict:
    """One lone call -> {contacts [T, T], rs [nch, T], tot [nch]} as numpy, the guard checked.  route: "atp"
    (rnamsm_contact_head_atp), "long" (rnamsm_contact_head_long) -- atp a numpy array or a device view whose planes may lie apart --
    or "unstripped" (rnamsm_contact_head on [nch, T + 1, T + 1] maps whose row and column 0 hold NaN: off = 1)."""
    lib = _lib.load()
    a = atp if isinstance(atp, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(atp)).to(DEV)
    nch, T = int(a.shape[0]), int(a.shape[-1])
    w, b = torch.from_numpy(np.asarray(weight, np.float32)).to(DEV), torch.from_numpy(np.asarray(bias, np.float32)).to(DEV)
    out = torch.full((T, T), NAN, device=DEV)
    if route == "unstripped":
        maps = torch.full((nch, T + 1, T + 1), NAN, device=DEV)
        maps[:, 1:, 1:] = a
        nbytes = lib.rnamsm_contact_head_workspace_bytes(T + 1, nch)
        ws = _workspace(nbytes)
        rc = lib.rnamsm_contact_head(maps.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, T + 1, nch,
                                     _stream())
    else:
        assert a.stride(1) == T and a.stride(2) == 1
        if route == "atp":
            nbytes, fn = lib.rnamsm_contact_head_workspace_bytes(T + 1, nch), lib.rnamsm_contact_head_atp
        else:
            assert route == "long", route
            nbytes, fn = lib.rnamsm_contact_head_long_workspace_bytes(T, nch), lib.rnamsm_contact_head_long
        ws = _workspace(nbytes)
        rc = fn(a.data_ptr(), a.stride(0), T, nch, w.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, _stream())
    _lib.check(rc)
    torch.cuda.synchronize()
    assert nbytes == 4 * (nch * T + nch), (route, T, nch, nbytes)
    assert bool((ws[nbytes:] == 0xA5).all()), f"{route}: written behind the workspace"
    rs, tot = _slab(ws, 0, T, nch)
    return {"contacts": out.cpu().numpy(), "rs": rs, "tot": tot}


def packed(atps, weight: np.ndarray, bias: np.ndarray) -> list:
    """One rnamsm_contact_head_packed call over the members atps (numpy arrays or device views) -> a list of {contacts, rs, tot},
    the slabs read from behind the descriptor table in member order, the guard behind the last slab checked."""
    lib = _lib.load()
    views = [a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in atps]
    B, nch = len(views), int(views[0].shape[0])
    Ls = [int(v.shape[-1]) for v in views]
    w, b = torch.from_numpy(np.asarray(weight, np.float32)).to(DEV), torch.from_numpy(np.asarray(bias, np.float32)).to(DEV)
    nbytes = lib.rnamsm_contact_head_packed_workspace_bytes(B, (ctypes.c_int * B)(*Ls), nch)
    table = -(-B * 64 // 256) * 256
    assert nbytes == table + sum(4 * (nch * L + nch) for L in Ls)
    ws = _workspace(nbytes)
    outs = [torch.full((L, L), NAN, device=DEV) for L in Ls]
    items = (_lib.ContactItem * B)(*(_lib.ContactItem(v.data_ptr(), v.stride(0), L, o.data_ptr()) for v, L, o in zip(views, Ls, outs)))
    _lib.check(lib.rnamsm_contact_head_packed(items, B, nch, w.data_ptr(), b.data_ptr(), ws.data_ptr(), nbytes, _stream()))
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all()), "packed: written behind the last slab"
    res, start = [], table
    for L, o in zip(Ls, outs):
        rs, tot = _slab(ws, start, L, nch)
        res.append({"contacts": o.cpu().numpy(), "rs": rs, "tot": tot})
        start += 4 * (nch * L + nch)
    assert start == nbytes
    return res


def bits(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)
