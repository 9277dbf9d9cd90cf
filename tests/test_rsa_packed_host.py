"""The batched RSA ensemble without a GPU (rnamsm_rsa_head_packed, rnamsm.rsa.plan_rsa_chunks, RSAEnsemble.predict_many): the
workspace size, every argument refusal of the C entry point (made before anything is enqueued, so they run on a host without
a device, on fabricated aligned addresses that are never dereferenced), the chunk planner's invariants and the Python
refusals."""
import ctypes

import numpy as np
import pytest
import torch

import rsa_truth as T
from rnamsm import _lib, rsa

K = 3
FAKE = 0x10000                             # "device addresses": non-null, 16-byte aligned, never read on the host
DESCRIPTOR_BYTES = 64


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _size(lib, Ls, k=K):
    return lib.rnamsm_rsa_head_packed_workspace_bytes(len(Ls), (ctypes.c_int * max(len(Ls), 1))(*Ls), k)


def test_symbols_and_limits():
    assert {"rnamsm_rsa_head_packed", "rnamsm_rsa_head_packed_workspace_bytes"} <= set(_lib.EXPORTED_SYMBOLS)
    assert _lib.RSA_MAX_BATCH == 1024 and ctypes.sizeof(_lib.RsaItem) == 48
    assert [f[0] for f in _lib.RsaItem._fields_] == ["emb", "emb_row_stride", "base_codes", "L", "probs", "logits"]


def test_workspace_bytes(lib):
    # a known list: the descriptor table (64 bytes per member, rounded up to 256) plus the lone sizes, in order
    Ls = [35, 1, 64, 1024, 97]
    table = (len(Ls) * DESCRIPTOR_BYTES + 255) // 256 * 256
    assert table == 512
    for k in (1, 3, 8):
        assert _size(lib, Ls, k) == table + sum(lib.rnamsm_rsa_head_workspace_bytes(L, k) for L in Ls)
    assert _size(lib, [35]) == 256 + lib.rnamsm_rsa_head_workspace_bytes(35, K)
    assert _size(lib, [8] * 4) - _size(lib, [8] * 3) == lib.rnamsm_rsa_head_workspace_bytes(8, K)          # 4 x 64 = one 256
    rng = np.random.RandomState(0)
    for _ in range(20):
        Ls = [int(v) for v in rng.randint(1, 1025, size=rng.randint(1, 40))]
        n = _size(lib, Ls)
        assert n > 0 and n % 16 == 0
        assert _size(lib, Ls + [int(rng.randint(1, 1025))]) > n                        # monotone in B
        sizes = [_size(lib, Ls, k) for k in range(1, 9)]
        assert all(a < b for a, b in zip(sizes, sizes[1:]))                            # ... and in K
    assert _size(lib, [1024] * 1024, 8) == 1024 * 64 + 1024 * lib.rnamsm_rsa_head_workspace_bytes(1024, 8)  # 15 GB: no 32-bit overflow
    assert _size(lib, []) == 0                                                       # B = 0
    assert _size(lib, [8] * 1025) == 0                                               # B = 1025
    assert _size(lib, [8, 0, 8]) == 0 and _size(lib, [8, 1025]) == 0                  # L = 0, L = 1025
    assert _size(lib, [8, 8], 0) == 0 and _size(lib, [8, 8], 9) == 0                  # n_models = 0, 9
    assert lib.rnamsm_rsa_head_packed_workspace_bytes(2, None, K) == 0               # null Ls


def _weights(k=K):
    n = len(_lib.W_RSA_GLOBAL) + k * len(_lib.W_RSA_MODEL)
    return (ctypes.c_void_p * n)(*[FAKE * (i + 1) for i in range(n)])


def _items(Ls):
    items = (_lib.RsaItem * len(Ls))()
    for b, L in enumerate(Ls):
        base = FAKE * 1000 * (b + 1)
        items[b] = _lib.RsaItem(base, 768, base + FAKE, L, base + 2 * FAKE, base + 3 * FAKE)
    return items


LS = [17, 40, 32]


def _call(lib, items=None, B=None, k=K, onehot=1, weights=None, ws=FAKE * 5000, ws_bytes=None, Ls=LS):
    items = _items(Ls) if items is None else items
    B = len(Ls) if B is None else B
    ws_bytes = _size(lib, Ls) if ws_bytes is None else ws_bytes
    return lib.rnamsm_rsa_head_packed(items, B, k, onehot, _weights(max(k, 1)) if weights is None else weights, ws, ws_bytes, None)


def _refused(lib, rc, *needles):
    assert rc == -1, rc                                   # RNAMSM_ERR_INVALID
    msg = lib.rnamsm_last_error().decode()
    assert "rsa_head_packed" in msg, msg
    for n in needles:
        assert n in msg, (n, msg)


def test_refusals_on_a_host_without_a_gpu(lib):
    assert _size(lib, LS) > 0
    # the batch size
    _refused(lib, _call(lib, B=0), "B=0")
    big = [4] * 1025
    _refused(lib, lib.rnamsm_rsa_head_packed(_items(big), 1025, K, 1, _weights(), FAKE * 5000, 1 << 40, None), "B=1025")
    # n_models
    _refused(lib, _call(lib, k=0, ws_bytes=1 << 40), "n_models=0")
    _refused(lib, _call(lib, k=9, ws_bytes=1 << 40), "n_models=9")
    # null table pointers
    _refused(lib, lib.rnamsm_rsa_head_packed(None, 3, K, 1, _weights(), FAKE * 5000, 1 << 40, None), "null")
    _refused(lib, lib.rnamsm_rsa_head_packed(_items(LS), 3, K, 1, None, FAKE * 5000, 1 << 40, None), "null")
    _refused(lib, _call(lib, ws=None), "null")
    # per member, each naming the member at fault
    for member in range(len(LS)):
        for field, value, needle in (("L", 0, "L=0"), ("L", 1025, "L=1025"), ("L", -3, "L=-3"), ("emb", None, "null"),
                                     ("base_codes", None, "null"), ("emb", FAKE + 4, "aligned"), ("emb", FAKE + 8, "aligned"),
                                     ("logits", FAKE + 1, "aligned"), ("probs", FAKE + 2, "aligned"),
                                     ("emb_row_stride", 767, "stride"), ("emb_row_stride", 0, "stride"),
                                     ("emb_row_stride", -768, "stride")):
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
    _refused(lib, _call(lib, ws_bytes=_size(lib, LS, 2)), "workspace")               # sized for two models, called with three
    _refused(lib, _call(lib, ws_bytes=0), "workspace")
    _refused(lib, _call(lib, ws=FAKE * 5000 + 8), "alignment")
    # the weight table: the lone call's rules
    bad = _weights()
    bad[7] = None
    _refused(lib, _call(lib, weights=bad), "weight pointer 7")
    bad = _weights()
    bad[9] = FAKE + 4
    _refused(lib, _call(lib, weights=bad), "weight pointer 9")
    for i in (2, 3):                                      # the one-hot statistics: needed with use_onehot, not read without
        bad = _weights()
        bad[i] = None
        _refused(lib, _call(lib, weights=bad), f"weight pointer {i}")
        # ... without use_onehot the same table passes the weight checks: the short workspace is what stops the call
        _refused(lib, _call(lib, weights=bad, onehot=0, ws_bytes=_size(lib, LS) - 1), "workspace")


def _merged_ok(a, b, Ls, budget, max_batch):
    return sum(Ls[i] for i in a + b) <= budget and len(a) + len(b) <= max_batch


def test_plan_rsa_chunks_on_random_lists():
    rng = np.random.RandomState(20261)
    for trial in range(200):
        n = int(rng.randint(0, 60))
        top = int(rng.choice([8, 64, 300, 1024]))
        Ls = [int(v) for v in rng.randint(1, top + 1, size=n)]
        budget = int(rng.choice([top, 3 * top, 32768]))
        max_batch = int(rng.choice([1, 3, 16, 1024]))
        chunks = rsa.plan_rsa_chunks(Ls, max_positions=budget, max_batch=max_batch)
        assert [i for c in chunks for i in c] == list(range(n)), (trial, chunks)          # a partition, consecutive, in order
        assert all(c for c in chunks)
        for c in chunks:
            assert sum(Ls[i] for i in c) <= budget and len(c) <= max_batch, (trial, c)
        for a, b in zip(chunks, chunks[1:]):
            assert not _merged_ok(a, b, Ls, budget, max_batch), (trial, a, b)
    # the defaults: 32768 positions, RNAMSM_RSA_MAX_BATCH members
    assert rsa.plan_rsa_chunks.__defaults__ == (32768, _lib.RSA_MAX_BATCH)
    assert rsa.plan_rsa_chunks([]) == []
    assert rsa.plan_rsa_chunks([1024]) == [[0]]
    assert rsa.plan_rsa_chunks([1024], max_positions=10) == [[0]]                     # a lone member is always admitted
    assert rsa.plan_rsa_chunks([5, 1024, 5], max_positions=10) == [[0], [1], [2]]
    assert [len(c) for c in rsa.plan_rsa_chunks([1] * 2500)] == [1024, 1024, 452]
    assert rsa.plan_rsa_chunks([1024] * 32 + [1]) == [list(range(32)), [32]]          # the running sum hits 32768 exactly, then one over
    assert rsa.plan_rsa_chunks([1024] * 31 + [1023, 1]) == [list(range(33))]
    assert rsa.plan_rsa_chunks([1024] * 31 + [1023, 1, 1]) == [list(range(33)), [33]]


def _ensemble():
    members = [rsa.RSAPredictor.from_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in T.make_state(11 + k).items()})
               for k in range(2)]
    st = T.load_stats("oh")
    return rsa.RSAEnsemble(members, {"emb": (st["emb_mu"], st["emb_std"]), "oh": (st["oh_mu"], st["oh_std"])}).eval()


def test_predict_many_refusals_without_a_device():
    ens = _ensemble()
    emb = torch.rand(6, 768)
    for call in (ens.predict_many, ens.logits_many):
        assert call([], []) == []
        with pytest.raises(_lib.RnamsmError, match=r"embs\[0\].*no CPU path"):
            call([emb, emb], ["ACGUAC", "ACGUAC"])
        with pytest.raises(_lib.RnamsmError, match=r"embs\[1\].*no CPU path"):
            call([emb, emb.numpy()], ["ACGUAC", "ACGUAC"])
        with pytest.raises(ValueError, match="2 embeddings for 1 sequences"):
            call([emb, emb], ["ACGUAC"])
        with pytest.raises(ValueError, match=r"seqs\[1\] has length 5"):
            call([emb, emb], ["ACGUAC", "ACGUA"])
        with pytest.raises(ValueError, match=r"seqs\[1\] has length 7"):
            call([emb, emb], ["ACGUAC", np.zeros(7, dtype=np.uint8)])
        with pytest.raises(ValueError, match=r"seqs\[0\] has length 4"):
            call([emb], [torch.zeros(4, dtype=torch.uint8)])
        with pytest.raises(ValueError, match=r"embs\[1\] must be \[L, 768\]"):
            call([emb, torch.rand(6, 767)], ["ACGUAC", "ACGUAC"])
        with pytest.raises(ValueError, match=r"embs\[0\] must be"):
            call([torch.rand(1, 6, 768)], ["ACGUAC"])
        with pytest.raises(ValueError, match=r"embs\[1\]: L = 1025 outside"):
            call([emb, torch.zeros(1025, 768)], ["ACGUAC", "A" * 1025])
        with pytest.raises(ValueError, match=r"embs\[0\]: L = 0 outside"):
            call([torch.zeros(0, 768)], [""])
