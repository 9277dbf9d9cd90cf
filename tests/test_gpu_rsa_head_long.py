"""The RSA head on long alignments on the GPU (rnamsm_rsa_head_long / rnamsm_rsa_text_long; RSAEnsemble.predict_long, logits_long,
ops.rsa_text_long), L up to 4096.

Up to L = 1024 the long entry points give the existing ones' bits and bytes.  Beyond, the logits are held to the fp64 restatement
(tests/rsa_truth.py) by rsa_truth.compare unchanged: rel-L2 and max-abs within 2 x the fp32 CPU restatement's own distance to fp64.
The lengths: 1025 (the first position of tile 33), 1056, 1057 and 2081 (the seams on both sides of a second and a third group of 32
tile sums: 33, 34 and 66 tiles), 4096 (128 tiles, 64 key chunks).  The inputs need the long part: positions of 8 x the size on both
sides of position 1024 and of every group seam (rsa_stages.halo_case's construction), and -- asserted on the fp64 restatement's
own q and k -- attention rows whose maximum lies in a key chunk beyond key 1024; the single members are rsa_stages.peaked_state
(scaled logits of several hundred: a maximum taken over the first 1024 keys only would overflow the exponentials).
One call on a NaN-filled long workspace at L = 1057 pins the layout: per model seven [L][64] images, then 128 rows of tile sums of
which 34 are written, and the squeeze mean in the documented order (one ascending chain per group of 32 tile sums, the group sums
ascending).  The text is the host writer's at L = 1025 and 4096, byte for byte.
Measured ratios: DESIGN 3.15."""
import numpy as np
import pytest
import torch

import rsa_stages as S
import rsa_text_cases as C
import rsa_truth as T
from rnamsm import _lib, ops, rsa, ss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
PLANES, TILE, GROUP, LONG_TILES = 64, 32, 32, 128
GUARD = 4096
SEAMS = (1024, 2048, 3072)              # position 1024 = the first of tile 32 = the first of the second group of tile sums; ...


def _states(which):
    if which == "rand3":               # the reference-made random state and two make_state members
        return [T.load_random_state(), T.make_state(12), T.make_state(13)], "oh"
    if which == "emb1":                # the shipped embedding-only model
        return [T.load_state("state_emb_0")], "emb"
    if which == "peaked1":
        return [S.peaked_state()], "oh"
    assert which == "gated_peaked"
    return [S.gated_state(), S.peaked_state()], "oh"


_ENS = {}


def _ensemble(which):
    """(ensemble on the device, the members' states, kind), built once and left unchanged."""
    if which not in _ENS:
        states, kind = _states(which)
        st = T.load_stats(kind)
        stats = {"emb": (st["emb_mu"], st["emb_std"])}
        if kind == "oh":
            stats["oh"] = (st["oh_mu"], st["oh_std"])
        members = [rsa.RSAPredictor.from_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}) for sd in states]
        _ENS[which] = (rsa.RSAEnsemble(members, stats).eval().to(DEV), states, kind)
    return _ENS[which]


def _long_case(L):
    """rsa_stages.halo_case, with the positions on both sides of position 1024 and of every seam between two groups of 32 tile
    sums multiplied by 8 as well."""
    emb, seq = S.halo_case(L, 900 + L)
    for s in SEAMS:
        for p in (s - 1, s):
            if p < L:
                emb[p] *= np.float32(S.HALO_GAIN)
    return emb, seq


# ---------------------------------------------------------------------- bits up to 1024
@pytest.mark.parametrize("L", [1, 31, 33, 65, 1024])
@pytest.mark.parametrize("which", ["rand3", "emb1"])
def test_up_to_1024_the_long_entry_gives_the_existing_one_s_bits(which, L):
    ens, _, _ = _ensemble(which)
    emb, seq = S.case(L, 40 + L)
    e = torch.from_numpy(emb).to(DEV)
    z, p = ens.logits(e, seq), ens.predict(e, seq)
    assert torch.equal(ens.logits_long(e, seq), z) and torch.equal(ens.predict_long(e, seq), p)
    assert z.shape == (len(ens), L) and bool(torch.isfinite(z).all())
    if L == 65:                         # a row slice of a wider buffer, read in place
        wide = torch.randn(L, 1000, device=DEV)
        wide[:, 8:776] = e
        view = wide[:, 8:776]
        assert not view.is_contiguous()
        assert torch.equal(ens.logits_long(view, seq), z) and torch.equal(ens.predict_long(view, seq), p)


# ---------------------------------------------------------------------- beyond 1024 against fp64
def _rows_with_a_late_maximum(x, state, L, rows=256):
    """Of the first and the last `rows` queries of the fp64 restatement: how many (head, query) rows have their largest scaled logit
    at a key >= 1024."""
    sd = S.tensors(state, F64)
    xt = torch.as_tensor(x).to(F64)
    h1, sh = S.stem(xt, sd)
    h2, sums = S.conv2(h1, sd)
    _, q, k, _ = S.mix(sh, h2, sums, sd)
    pick = torch.cat([torch.arange(0, min(rows, L)), torch.arange(max(L - rows, 0), L)]).unique()
    where = S.attn_scores(q[pick], k).argmax(dim=-1)
    return int((where >= 1024).sum()), where.numel()


@pytest.mark.parametrize("which, L", [("peaked1", 1025), ("peaked1", 1056), ("rand3", 1057), ("peaked1", 2081), ("peaked1", 4096)])
def test_beyond_1024_against_fp64(which, L):
    ens, states, kind = _ensemble(which)
    emb, seq = _long_case(L)
    assert all(float(np.abs(emb[p]).mean()) > 4 * float(np.abs(emb[p - 2]).mean()) for s in SEAMS for p in (s - 1, s) if p < L)
    x = T.features(emb, seq, T.load_stats(kind), use_onehot=kind == "oh")
    for m, sd in enumerate(states):
        late, n = _rows_with_a_late_maximum(x, sd, L)
        print(f"{which} L={L} model {m}: {late} of {n} sampled attention rows have their maximum at a key >= 1024")
        assert late > 0
    got = ens.logits_long(torch.from_numpy(emb).to(DEV), seq).cpu().numpy()
    assert got.shape == (len(states), L)
    for m, sd in enumerate(states):    # one member at a time: the fp64 score tensor is 1 GB at L = 4096
        t64, t32 = T.logits(x, sd, F64), T.logits(x, sd, F32).astype(np.float64)
        T.compare(got[m], t64, t32, f"long {which} L={L} model {m}")


@pytest.mark.parametrize("L", [1057, 4096])
def test_two_long_runs_give_identical_bits(L):
    ens, _, _ = _ensemble("rand3")
    emb, seq = _long_case(L)
    e = torch.from_numpy(emb).to(DEV)
    assert torch.equal(ens.logits_long(e, seq), ens.logits_long(e, seq))


# ---------------------------------------------------------------------- the stages through the long workspace
def _chain(rows):
    """One ascending chain over the rows of a [n][64] tensor, in its dtype."""
    s = rows[0]
    for i in range(1, rows.shape[0]):
        s = s + rows[i]
    return s


def test_stages_through_the_long_workspace_at_1057():
    ens, states, kind = _ensemble("gated_peaked")
    lib = _lib.load()
    K, L = len(ens), 1057
    tiles = (L + TILE - 1) // TILE
    assert tiles == 34
    emb, seq = _long_case(L)
    mf = 7 * L * PLANES + LONG_TILES * PLANES
    nbytes = lib.rnamsm_rsa_head_long_workspace_bytes(L, K)
    assert nbytes == 4 * K * mf
    ws = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)          # 0xFFFFFFFF: a NaN in every float
    logits = torch.full((K, L), float("nan"), device=DEV)
    e = torch.from_numpy(emb).to(DEV)
    codes = torch.from_numpy(ss.base_codes(seq)).to(DEV)
    ptrs, _ = ens._packed_weights()
    _lib.check(lib.rnamsm_rsa_head_long(e.data_ptr(), 768, codes.data_ptr(), L, K, 1, ptrs, None, logits.data_ptr(), ws.data_ptr(),
                                        nbytes, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    host = ws.cpu()
    assert bool((host[nbytes:] == 0xFF).all()), "bytes behind the workspace were written"
    assert bool(torch.isfinite(logits).all())
    assert torch.equal(logits, ens.logits_long(e, seq))
    floats = host[:nbytes].view(F32)
    for m, state in enumerate(states):
        slab = floats[m * mf:(m + 1) * mf]
        imgs = slab[:7 * L * PLANES].view(7, L, PLANES)
        sums = slab[7 * L * PLANES:].view(LONG_TILES, PLANES)
        assert bool(torch.isfinite(imgs).all()), f"model {m}: images"
        assert bool(torch.isfinite(sums[:tiles]).all()), f"model {m}: tile-sum rows [0, {tiles})"
        assert bool(torch.isnan(sums[tiles:]).all()), f"model {m}: tile-sum rows [{tiles}, {LONG_TILES}) were written"
        dev = {n: imgs[i] for i, n in enumerate(S.IMAGES)}
        S.check_tile_sums(sums[:tiles], dev["h2"], f"long L={L} model {m} conv2")
        # the squeeze mean in the documented order: the group sums, each an ascending chain, handed to the restatement, which adds
        # its rows ascending (rsa_stages.se_gate)
        t = {}
        for dtype in (F64, F32):
            groups = torch.stack([_chain(sums[g:min(g + GROUP, tiles)].to(dtype)) for g in range(0, tiles, GROUP)])
            assert groups.shape == (2, PLANES)
            t[dtype] = S.mix(dev["shortcut"], dev["h2"], groups, state, dtype)
        for i, n in enumerate(("y", "q", "k", "v")):
            S.check_stage(dev[n], t[F64][i], t[F32][i], f"long L={L} model {m} mix {n}")
        if m == 0:                      # (what the order is worth: one chain over all 34 tile sums gives other fp32 sums)
            grouped = _chain(torch.stack([_chain(sums[g:min(g + GROUP, tiles)]) for g in range(0, tiles, GROUP)]))
            print(f"long L={L}: channels whose fp32 sum differs between the two orders: {int((grouped != _chain(sums[:tiles])).sum())} of 64")


# ---------------------------------------------------------------------- non-finite inputs
def test_a_nan_in_the_last_position_reaches_every_output_and_unread_columns_none():
    ens, _, _ = _ensemble("rand3")
    L = 4096
    emb, seq = S.case(L, 7)
    wide = torch.full((L, 1000), float("nan"), device=DEV)          # NaN in every column the head does not read
    wide[:, 8:776] = torch.from_numpy(emb).to(DEV)
    view = wide[:, 8:776]
    clean = ens.logits_long(view.contiguous(), seq)
    assert bool(torch.isfinite(clean).all())
    assert torch.equal(ens.logits_long(view, seq), clean) and torch.equal(ens.predict_long(view, seq), ens.predict_long(view.contiguous(), seq))
    wide[L - 1, 8 + 767] = float("nan")
    for out in (ens.logits_long(view, seq), ens.predict_long(view, seq)):
        assert out.shape == (3, L)
        assert bool(torch.isnan(out).all()) and not bool(torch.isinf(out).any())      # the squeeze mean and the attention carry it everywhere


# ---------------------------------------------------------------------- the text
def _dev_text(fn, values, seq):
    text, counts, ens = fn(torch.from_numpy(values).to(DEV), torch.from_numpy(ss.letter_codes(seq)).to(DEV))
    return text.cpu().numpy(), counts.cpu().numpy(), ens.cpu().numpy()


@pytest.mark.parametrize("L", [35, 1024])
@pytest.mark.parametrize("K", [1, 3])
def test_text_up_to_1024_is_the_existing_entry_s_bytes(K, L):
    values, seq = C.special_table(K, L, K + L), C.seq_for(L, L)
    a, b = _dev_text(ops.rsa_text_long, values, seq), _dev_text(ops.rsa_text, values, seq)
    assert np.array_equal(a[1], b[1]) and a[1][K + 1] == 0 and a[1][K + 2] == 0
    assert C.split_text(a[0], a[1], K, L) == C.split_text(b[0], b[1], K, L)
    assert a[2].tobytes() == b[2].tobytes()


@pytest.mark.parametrize("K, L", [(3, 1025), (1, 4096), (3, 4096), (8, 4096)])
def test_text_beyond_1024_is_the_host_writer_s(K, L):
    values, seq = C.special_table(K, L, K + L), C.seq_for(L, L)
    text, counts, ens = _dev_text(ops.rsa_text_long, values, seq)
    want, want_ens = C.expected_bodies(values, seq)
    assert counts[K + 1] == 0 and counts[K + 2] == 0
    assert counts[:K + 1].tolist() == [len(b) for b in want]
    assert C.split_text(text, counts, K, L) == want
    assert want[K].splitlines()[-1].startswith(f"{L}\t\t".encode())
    assert ens.dtype == np.float64 and ens.tobytes() == want_ens.tobytes()


def test_text_flag_words_at_the_long_limit():
    K, L = 3, 4096
    good, seq = C.uniform_values(K, L, 5), C.seq_for(L, 5)
    assert _dev_text(ops.rsa_text_long, good, seq)[1][K + 1:].tolist() == [0, 0]
    v = good.copy()
    v[2, 4095] = np.nan
    assert _dev_text(ops.rsa_text_long, v, seq)[1][K + 1] == 1
    assert _dev_text(ops.rsa_text_long, good, seq[:4095] + "X")[1][K + 1] == 1          # a letter X at position 4096
    v = good.copy()
    v[1, 4095] = 0.0
    assert _dev_text(ops.rsa_text_long, v, seq)[1][K + 1:].tolist() == [0, 1]              # an exact 0: the zero word
    v = good.copy()
    v[0, 1024] = 0.0
    assert _dev_text(ops.rsa_text_long, v, seq)[1][K + 1:].tolist() == [0, 1]


def _same_record(a, b, K, L) -> bool:
    """Two text records agree in their counts, their ensemble and the bytes their counts cover (nothing behind them is written)."""
    a, b = ([t.cpu().numpy() for t in r] for r in (a, b))
    return np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes() and C.split_text(a[0], a[1], K, L) == C.split_text(b[0], b[1], K, L)


def test_predict_text_long_and_the_head_s_record():
    """predict_text_long is predict_long and table_text_long; RSAHead.one_long makes the record one() makes where both accept the L."""
    import random
    from rnamsm.alphabet import RNAAlphabet
    ens, _, _ = _ensemble("rand3")
    L = 1057
    emb, seq = S.case(L, 3)
    seq = seq.replace("N", "A").replace("t", "U")
    e = torch.from_numpy(emb).to(DEV)
    values, text = ens.predict_text_long(e, seq)
    assert torch.equal(values, ens.predict_long(e, seq))
    want = ops.rsa_text_long(values, torch.from_numpy(ss.letter_codes(seq)).to(DEV))
    assert _same_record(text, want, 3, L)
    alphabet = RNAAlphabet.from_architecture("rna language")
    head = rsa.RSAHead(ens, alphabet, ss.token_base_codes(alphabet, DEV), random.Random(2022), text_on=True, device=DEV)
    toks = torch.tensor([alphabet.get_idx(c) for c in seq], device=DEV)
    rec = head.one_long(e, None, toks)
    assert torch.equal(rec.values, values) and _same_record(rec.text, want, 3, L)
    short, ref = head.one_long(e[:70], None, toks[:70]), head.one(e[:70], None, toks[:70])
    assert torch.equal(short.values, ref.values) and _same_record(short.text, ref.text, 3, 70)


def test_out_of_range_lengths_raise_on_the_device_too():
    ens, _, _ = _ensemble("rand3")
    with pytest.raises(ValueError, match="4097"):
        ens.predict_long(torch.zeros(4097, 768, device=DEV), "A" * 4097)
    with pytest.raises(ValueError, match="4097"):
        ops.rsa_text_long(torch.zeros(3, 4097, device=DEV), torch.zeros(4097, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):                                     # the existing method keeps its range
        ens.predict(torch.zeros(1025, 768, device=DEV), "A" * 1025)
