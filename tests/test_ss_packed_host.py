"""The batched SS head without a GPU (rnamsm_ss_head_packed, rnamsm.ss.plan_ss_chunks, SSPredictor.predict_many): the
workspace size, every argument refusal of the C entry point (made before anything is enqueued, so they run on a host without
a device, on fabricated aligned addresses that are never dereferenced), the chunk planner's invariants and the Python
refusals."""
import ctypes

import numpy as np
import pytest
import torch

from rnamsm import _lib, ss

PIXEL_BYTES = 48 * 4                       # one NHWC pixel of a workspace image
NUM_BLOCKS = 4
FAKE = 0x10000                             # "device addresses": non-null, 16-byte aligned, never read on the host


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _size(lib, Ls):
    return lib.rnamsm_ss_head_packed_workspace_bytes(len(Ls), (ctypes.c_int * max(len(Ls), 1))(*Ls))


def test_symbols_and_limits():
    assert {"rnamsm_ss_head_packed", "rnamsm_ss_head_packed_workspace_bytes"} <= set(_lib.EXPORTED_SYMBOLS)
    assert _lib.SS_MAX_BATCH == 1024 and ctypes.sizeof(_lib.SsItem) == 48


def test_workspace_bytes(lib):
    rng = np.random.RandomState(0)
    for _ in range(20):
        Ls = [int(v) for v in rng.randint(1, 1025, size=rng.randint(1, 40))]
        n = _size(lib, Ls)
        assert n >= 2 * sum(L * L for L in Ls) * PIXEL_BYTES
        assert n % 16 == 0
        more = _size(lib, Ls + [int(rng.randint(1, 1025))])
        assert more > n                                   # monotone when a member is added
    assert _size(lib, [1024] * 1024) >= 2 * 1024 * 1024 * 1024 * PIXEL_BYTES         # the largest batch: no 32-bit overflow
    assert _size(lib, []) == 0                                                       # B = 0
    assert _size(lib, [8] * 1025) == 0                                               # B = 1025
    assert _size(lib, [8, 0, 8]) == 0 and _size(lib, [8, 1025]) == 0                  # L = 0, L = 1025
    assert lib.rnamsm_ss_head_packed_workspace_bytes(2, None) == 0                   # null Ls


def _weights(n_blocks=NUM_BLOCKS):
    n = len(_lib.W_SS_STEM) + n_blocks * len(_lib.W_SS_BLOCK) + len(_lib.W_SS_HEAD)
    return (ctypes.c_void_p * n)(*[FAKE * (i + 1) for i in range(n)])


def _items(Ls):
    items = (_lib.SsItem * len(Ls))()
    for b, L in enumerate(Ls):
        base = FAKE * 1000 * (b + 1)
        items[b] = _lib.SsItem(base, L * L, base + FAKE, L, base + 2 * FAKE, base + 3 * FAKE)
    return items


LS = [17, 40, 16]


def _call(lib, items=None, B=None, num_blocks=NUM_BLOCKS, weights=None, ws=FAKE * 5000, ws_bytes=None, Ls=LS):
    items = _items(Ls) if items is None else items
    B = len(Ls) if B is None else B
    ws_bytes = _size(lib, Ls) if ws_bytes is None else ws_bytes
    return lib.rnamsm_ss_head_packed(items, B, num_blocks, _weights() if weights is None else weights, ws, ws_bytes, None)


def _refused(lib, rc, *needles):
    assert rc == -1, rc                                   # RNAMSM_ERR_INVALID
    msg = lib.rnamsm_last_error().decode()
    for n in needles:
        assert n in msg, (n, msg)


def test_refusals_on_a_host_without_a_gpu(lib):
    assert _size(lib, LS) > 0
    # the batch size
    _refused(lib, _call(lib, B=0), "B=0")
    big = [4] * 1025
    _refused(lib, lib.rnamsm_ss_head_packed(_items(big), 1025, NUM_BLOCKS, _weights(), FAKE * 5000, 1 << 40, None), "B=1025")
    # num_blocks
    _refused(lib, _call(lib, num_blocks=0), "num_blocks=0")
    _refused(lib, _call(lib, num_blocks=65, weights=_weights(65)), "num_blocks=65")
    # null table pointers
    assert lib.rnamsm_ss_head_packed(None, 3, NUM_BLOCKS, _weights(), FAKE * 5000, 1 << 40, None) == -1
    assert lib.rnamsm_ss_head_packed(_items(LS), 3, NUM_BLOCKS, None, FAKE * 5000, 1 << 40, None) == -1
    _refused(lib, _call(lib, ws=None), "null")
    # per member, each naming the member at fault
    for member in range(len(LS)):
        for field, value, needle in (("L", 0, "L=0"), ("L", 1025, "L=1025"), ("atp", None, "null"), ("base_codes", None, "null"),
                                     ("atp", FAKE + 2, "aligned"), ("logits", FAKE + 1, "aligned"), ("probs", FAKE + 3, "aligned"),
                                     ("atp_plane_stride", LS[member] ** 2 - 1, "stride")):
            items = _items(LS)
            setattr(items[member], field, value)
            _refused(lib, _call(lib, items=items, ws_bytes=1 << 40), f"member {member}", needle)
        items = _items(LS)
        items[member].logits = None
        items[member].probs = None
        _refused(lib, _call(lib, items=items), f"member {member}", "neither")
        for only in ("logits", "probs"):                  # one of the two is enough: the argument checks pass and ...
            items = _items(LS)
            setattr(items[member], only, None)
            _refused(lib, _call(lib, items=items, ws_bytes=_size(lib, LS) - 1), "workspace")      # ... the short workspace is what stops it
    # the workspace: short, misaligned
    _refused(lib, _call(lib, ws_bytes=_size(lib, LS) - 1), "workspace")
    _refused(lib, _call(lib, ws_bytes=_size(lib, LS[:2])), "workspace")
    _refused(lib, _call(lib, ws=FAKE * 5000 + 8), "alignment")
    # the weight table
    bad = _weights()
    bad[7] = None
    _refused(lib, _call(lib, weights=bad), "weight pointer 7")
    bad = _weights()
    bad[9] = FAKE + 4
    _refused(lib, _call(lib, weights=bad), "weight pointer 9")


def _merged_ok(a, b, Ls, budget, max_batch):
    return sum(Ls[i] ** 2 for i in a + b) <= budget and len(a) + len(b) <= max_batch


def test_plan_ss_chunks_on_random_lists():
    rng = np.random.RandomState(20260)
    for trial in range(200):
        n = int(rng.randint(0, 60))
        top = int(rng.choice([8, 64, 300, 1024]))
        Ls = [int(v) for v in rng.randint(1, top + 1, size=n)]
        budget = int(rng.choice([top * top, 2 * top * top, 1024 * 1024]))
        max_batch = int(rng.choice([1, 3, 16, 1024]))
        chunks = ss.plan_ss_chunks(Ls, max_pixels=budget, max_batch=max_batch)
        assert [i for c in chunks for i in c] == list(range(n)), (trial, chunks)          # a partition, consecutive, in order
        assert all(c for c in chunks)
        for c in chunks:
            assert sum(Ls[i] ** 2 for i in c) <= budget and len(c) <= max_batch, (trial, c)
        for a, b in zip(chunks, chunks[1:]):
            assert not _merged_ok(a, b, Ls, budget, max_batch), (trial, a, b)
    # the defaults: one lone L = 1024 call's worth of pixels, RNAMSM_SS_MAX_BATCH members
    assert ss.plan_ss_chunks([1024, 1024, 1]) == [[0], [1], [2]]          # 1024^2 + 1 pixels are one too many
    assert ss.plan_ss_chunks([1024, 1023, 1]) == [[0], [1, 2]]
    assert ss.plan_ss_chunks([512] * 5) == [[0, 1, 2, 3], [4]]
    assert [len(c) for c in ss.plan_ss_chunks([1] * 2500)] == [1024, 1024, 452]
    assert ss.plan_ss_chunks([]) == []


def test_predict_many_refusals_without_a_device():
    model = ss.SSPredictor(2).eval()
    atp = torch.rand(120, 6, 6)
    for call in (model.predict_many, model.logits_many):
        with pytest.raises(_lib.RnamsmError, match="no CPU path"):
            call([atp, atp], ["ACGUAC", "ACGUAC"])
        with pytest.raises(ValueError, match="2 attention maps for 1 sequences"):
            call([atp, atp], ["ACGUAC"])
        with pytest.raises(ValueError, match=r"seqs\[1\] has length 5"):
            call([atp, atp], ["ACGUAC", "ACGUA"])
        with pytest.raises(ValueError, match=r"atps\[0\] must be"):
            call([torch.rand(119, 6, 6)], ["ACGUAC"])
