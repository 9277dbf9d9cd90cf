"""The `.prob` text written on the GPU (rnamsm_ss_prob_text / _packed, rnamsm.ss.prob_text, write_ss_files(prob_text=...), the
CLI key data.ss_prob_text).  The expected bytes are always np.savetxt of the same host array into a BytesIO; every comparison
is == on bytes."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from rnamsm import _lib, ops, ss, synthetic
import dec19_cases as C
import ss_truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _text(prob: np.ndarray):
    """ops.ss_prob_text of a host matrix -> (bytes, fallback word)."""
    text, fb = ops.ss_prob_text(torch.from_numpy(np.ascontiguousarray(prob)).to(DEV))
    assert text.dtype == torch.uint8 and text.shape == (25 * prob.shape[0] ** 2,)
    assert fb.dtype == torch.int32 and fb.shape == (1,)
    return text.cpu().numpy().tobytes(), int(fb.item())


def _sigmoid_case(L: int, seed: int) -> np.ndarray:
    """Sigmoid outputs of logits N(-6, 6) in fp32: down to subnormal probabilities, up to 1.0 itself."""
    z = torch.from_numpy(np.random.RandomState(seed).normal(-6.0, 6.0, size=(L, L)).astype(np.float32))
    return torch.sigmoid(z).numpy()


@pytest.fixture(scope="module")
def special():
    return C.floats_of(C.special_values())


# ------------------------------------------------------------------ lone call
@pytest.mark.parametrize("L", [1, 2, 15, 16, 17, 35])
def test_special_values(special, L):
    """The special-value set of the host test, laid row by row into [L, L] matrices.  L >= 15: consecutive matrices cover the
    whole set (the last one wraps round to its start); L = 1 and L = 2: 64 matrices spread evenly over the set, 0.0 and 1.0
    among them, so that the smallest shapes stay a handful of launches."""
    n = L * L
    if L >= 15:
        starts = range(0, len(special), n)
    else:
        zero, one = int(np.flatnonzero(special == 0.0)[0]), int(np.flatnonzero(special == 1.0)[0])
        starts = sorted(set(np.linspace(0, len(special) - n, 62).astype(int).tolist() + [zero, one]))
    for s0 in starts:
        prob = np.take(special, np.arange(s0, s0 + n), mode="wrap").reshape(L, L)
        got, fb = _text(prob)
        assert fb == 0, (L, s0)
        assert got == C.savetxt_bytes(prob), (L, s0)


def test_the_random_patterns_of_the_host_test(special):
    """All 2^16 random patterns and the special values in one matrix (L = 263, zero-filled to the square)."""
    vals = np.concatenate([C.floats_of(C.random_patterns()), special])
    L = int(np.ceil(np.sqrt(len(vals))))
    prob = np.zeros(L * L, dtype=np.float32)
    prob[:len(vals)] = vals
    prob = prob.reshape(L, L)
    got, fb = _text(prob)
    assert fb == 0 and got == C.savetxt_bytes(prob)


@pytest.mark.parametrize("L", [100, 257])
def test_block_edges(L):
    """L^2 = 10 000 and 66 049: both sides of a multiple of the 256-element block (39 x 256 + 16, 258 x 256 + 1), rows that
    straddle blocks, a last block whose bytes are no multiple of 16.  (Logits N(-6, 6) spread the probabilities over some
    fifteen decades; the subnormal ones are in the special-value set above.)"""
    prob = _sigmoid_case(L, 1000 + L)
    got, fb = _text(prob)
    assert fb == 0 and len(got) == 25 * L * L
    assert got == C.savetxt_bytes(prob)


def test_text_bytes():
    lib = _lib.load()
    for L in (1, 35, 128, 512, 1024):
        assert lib.rnamsm_ss_prob_text_bytes(L) == 25 * L * L
    assert lib.rnamsm_ss_prob_text_bytes(0) == 0 and lib.rnamsm_ss_prob_text_bytes(1025) == 0
    assert lib.rnamsm_ss_prob_text_bytes(-1) == 0


# ------------------------------------------------------------------ packed call
PACKED_LS = [1, 17, 2, 35, 16, 100]


@pytest.fixture(scope="module")
def packed_cases():
    """The members, their lone texts and their np.savetxt bytes, computed once."""
    probs = [_sigmoid_case(L, 2000 + i) for i, L in enumerate(PACKED_LS)]
    lone = [_text(p) for p in probs]
    want = [C.savetxt_bytes(p) for p in probs]
    return probs, lone, want


def _packed(probs):
    out = ops.ss_prob_text_packed([torch.from_numpy(np.ascontiguousarray(p)).to(DEV) for p in probs])
    return [(t.cpu().numpy().tobytes(), int(w.item())) for t, w in out]


@pytest.mark.parametrize("reverse", [False, True])
def test_every_member_has_the_lone_call_s_bytes(packed_cases, reverse):
    probs, lone, want = (list(reversed(v)) if reverse else v for v in packed_cases)
    got = _packed(probs)
    assert len(got) == len(probs)
    for b, L in enumerate(p.shape[0] for p in probs):
        assert got[b][1] == 0 and lone[b][1] == 0, (b, L)
        assert got[b][0] == lone[b][0], (b, L)
        assert got[b][0] == want[b], (b, L)


def test_more_members_than_one_descriptor_chunk():
    """33 members of L = 3: 32 descriptors travel per launch, so the last member is a launch of its own."""
    probs = [_sigmoid_case(3, 3000 + i) for i in range(33)]
    got = _packed(probs)
    assert len(got) == 33
    for b, p in enumerate(probs):
        assert got[b] == (C.savetxt_bytes(p), 0), b
    many = ss.prob_text_many([torch.from_numpy(p).to(DEV) for p in probs])
    assert [t.cpu().numpy().tobytes() for t, _ in many] == [g for g, _ in got]


def test_a_member_outside_the_domain_marks_its_own_word_only(packed_cases):
    probs, lone, want = (list(v) for v in packed_cases)
    probs = [p.copy() for p in probs]
    probs[1][16, 16] = np.nan                                              # L = 17: the last element
    probs[3][0, 0] = -0.0                                                  # L = 35: the first
    probs[5][50, 99] = np.float32(1.0000001)                               # L = 100: the end of a row
    assert probs[5][50, 99] > 1.0
    got = _packed(probs)
    assert [w for _, w in got] == [0, 1, 0, 1, 0, 1]
    for b in (0, 2, 4):
        assert got[b][0] == want[b], b
    for b in (1, 3, 5):                                                    # the lone call says the same of each
        assert _text(probs[b])[1] == 1, b
    for bad in (np.inf, -1.0, 2.0, -np.nan):
        p = probs[2].copy()
        p[1, 0] = bad
        assert _text(p)[1] == 1, bad


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched():
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    probs = torch.full((4, 4), 0.5, device=DEV)
    text = torch.full((25 * 16 + 16,), 7, dtype=torch.uint8, device=DEV)
    word = torch.full((1,), 7, dtype=torch.int32, device=DEV)

    def refused(rc, *needles):
        assert rc == -1, rc
        msg = lib.rnamsm_last_error().decode()
        for n in needles:
            assert n in msg, (n, msg)

    refused(lib.rnamsm_ss_prob_text(probs.data_ptr(), 0, text.data_ptr(), word.data_ptr(), stream), "L=0")
    refused(lib.rnamsm_ss_prob_text(probs.data_ptr(), 1025, text.data_ptr(), word.data_ptr(), stream), "L=1025")
    refused(lib.rnamsm_ss_prob_text(None, 4, text.data_ptr(), word.data_ptr(), stream), "null")
    refused(lib.rnamsm_ss_prob_text(probs.data_ptr(), 4, None, word.data_ptr(), stream), "null")
    refused(lib.rnamsm_ss_prob_text(probs.data_ptr(), 4, text.data_ptr(), None, stream), "null")
    refused(lib.rnamsm_ss_prob_text(probs.data_ptr(), 4, text.data_ptr() + 1, word.data_ptr(), stream), "aligned")

    def items(n, L=4):
        arr = (_lib.SsTextItem * n)()
        for b in range(n):
            arr[b] = _lib.SsTextItem(probs.data_ptr(), L, text.data_ptr(), word.data_ptr())
        return arr

    refused(lib.rnamsm_ss_prob_text_packed(items(1), 0, stream), "B=0")
    refused(lib.rnamsm_ss_prob_text_packed(items(1025), 1025, stream), "B=1025")
    refused(lib.rnamsm_ss_prob_text_packed(None, 2, stream), "null")
    for member in range(3):
        for field, value, needle in (("L", 0, "L=0"), ("L", 1025, "L=1025"), ("probs", None, "null"), ("text", None, "null"),
                                     ("fallback", None, "null")):
            arr = items(3)
            setattr(arr[member], field, value)
            refused(lib.rnamsm_ss_prob_text_packed(arr, 3, stream), f"member {member}", needle)
    torch.cuda.synchronize()
    assert bool((text == 7).all()) and int(word.item()) == 7              # nothing was launched
    with pytest.raises(_lib.RnamsmError):
        ops.ss_prob_text(torch.zeros(4, 4))                                # no CPU path
    with pytest.raises(ValueError):
        ops.ss_prob_text(torch.zeros(4, 5, device=DEV))
    with pytest.raises(ValueError):
        ops.ss_prob_text(torch.zeros(1025, 1025, device=DEV))


# ------------------------------------------------------------------ write_ss_files
def _files(root):
    return {ext: (root / "SS_result" / f"x.{ext}").read_bytes() for ext in ("ct", "bpseq", "prob")}


def test_write_ss_files_with_the_head_s_own_output(tmp_path):
    """Real head output at L = 35 (the golden maps of 2DRB_1): the three files with the device text equal those without it; with
    fallback = 1 a text is ignored, whatever it holds."""
    atp = torch.from_numpy(np.load(os.path.join(GOLDEN, "ss", "2DRB_1_atp.npy"))).to(DEV)
    L = atp.shape[-1]
    assert L == 35
    seq = "".join(np.random.RandomState(5).choice(list("ACGU"), L))
    head = ss.SSPredictor(4)
    head.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ss_truth.make_state(4, seed=21).items()}, strict=True)
    probs = head.eval().to(DEV).predict(atp, seq)
    text, fb = ss.prob_text(probs)
    prob, text, fb = probs.cpu().numpy(), text.cpu().numpy(), int(fb.item())
    assert fb == 0
    pairs0 = ss.write_ss_files(prob, seq, "x", tmp_path / "host")
    pairs1 = ss.write_ss_files(prob, seq, "x", tmp_path / "device", prob_text=text, fallback=fb)
    garbage = np.full_like(text, ord("?"))
    pairs2 = ss.write_ss_files(prob, seq, "x", tmp_path / "ignored", prob_text=garbage, fallback=1)
    want = _files(tmp_path / "host")
    assert want["prob"] == C.savetxt_bytes(prob)
    assert _files(tmp_path / "device") == want and _files(tmp_path / "ignored") == want
    assert pairs0 == pairs1 == pairs2
    with pytest.raises(ValueError):
        ss.write_ss_files(prob, seq, "x", tmp_path / "short", prob_text=text[:-1], fallback=0)


def test_a_nan_poisoned_map_takes_the_savetxt_path(tmp_path):
    """A NaN in the probabilities: the word reads 1 and write_ss_files formats on the host, `nan` fields as before."""
    prob = _sigmoid_case(35, 77)
    prob[3, 4] = np.nan
    text, fb = ss.prob_text(torch.from_numpy(prob).to(DEV))
    assert int(fb.item()) == 1
    seq = "ACGU" * 8 + "ACG"
    ss.write_ss_files(prob, seq, "x", tmp_path / "host")
    ss.write_ss_files(prob, seq, "x", tmp_path / "device", prob_text=text.cpu().numpy(), fallback=int(fb.item()))
    assert _files(tmp_path / "device") == _files(tmp_path / "host")
    assert b"nan" in _files(tmp_path / "device")["prob"]


# ------------------------------------------------------------------ CLI
def test_cli_files_do_not_depend_on_the_key(tmp_path, monkeypatch):
    """Four synthetic alignments with the SS head on, one above the size up to which an alignment waits for company (it runs
    alone) and three that share a packed group: SS_result/*.{prob,ct,bpseq} byte-identical with data.ss_prob_text on (the default) and off; on, the lone
    formatter runs once and the packed one once over the three; off, neither runs."""
    sys.path.insert(0, ROOT)
    import RNA_MSM_Inference as cli
    state = synthetic.make_state_dict(seed=0, num_layers=10)
    ckpt = tmp_path / "model.ckpt"
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in state.items()}}, ckpt)
    ss_pt = tmp_path / "model" / "rna-msm_attention.pt"
    ss_pt.parent.mkdir(parents=True)
    torch.save({k: torch.from_numpy(v) for k, v in ss_truth.make_state(4, seed=5).items()}, ss_pt)
    real_load = ss.load_predictor
    monkeypatch.setattr(ss, "load_predictor", lambda path, device, num_blocks=4: real_load(path, device, num_blocks))
    from rnamsm import inference
    assert 170 * 101 > inference.PACKED_SMALL_TOKENS
    rng = np.random.RandomState(92)
    shapes = [(170, 100), (4, 12), (8, 40), (5, 17)]         # 170 x 101 = 17 170 tokens > PACKED_SMALL_TOKENS: alone; the rest wait for company
    ids = [f"rna{k}" for k in range(len(shapes))]
    texts = {i: "".join(f">s{r}\n{''.join(rng.choice(list('ACGU'), L))}\n" for r in range(R)) for i, (R, L) in zip(ids, shapes)}
    (tmp_path / "rna_id.txt").write_text("\n".join(ids) + "\n")
    lone_calls, packed_calls = [], []
    real_lone, real_packed = ops.ss_prob_text, ops.ss_prob_text_packed
    monkeypatch.setattr(ops, "ss_prob_text", lambda p: lone_calls.append(p.shape[0]) or real_lone(p))
    monkeypatch.setattr(ops, "ss_prob_text_packed", lambda ps: packed_calls.append(len(ps)) or real_packed(ps))

    def run(name, extra):
        res = tmp_path / name
        res.mkdir()
        for i in ids:
            (res / f"{i}.a2m_msa2").write_text(texts[i])
        cli.main([f"data.root_path={tmp_path}", f"data.MSA_path={name}", f"data.model_path={ckpt}", "data.MSA_list=rna_id.txt",
                  "data.max_seqs_per_msa=256", "data.sample_method=first", f"data.ss_model_path={ss_pt}"] + extra)
        return res

    on = run("on", [])
    assert lone_calls == [100] and packed_calls == [3], (lone_calls, packed_calls)
    del lone_calls[:], packed_calls[:]
    off = run("off", ["data.ss_prob_text=false"])
    assert lone_calls == [] and packed_calls == []
    for i, (_, L) in zip(ids, shapes):
        for ext in ("prob", "ct", "bpseq"):
            a, b = (on / "SS_result" / f"{i}.{ext}").read_bytes(), (off / "SS_result" / f"{i}.{ext}").read_bytes()
            assert a and a == b, (i, ext)
        assert len((on / "SS_result" / f"{i}.prob").read_bytes()) == 25 * L * L
