"""The LM head's route without a GPU: the ABI's declarations, the sizes and every refusal that needs no device (each comes before the
first launch), the config key, the two plans and the truth helper."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lm_truth
from oracle import msm_oracle as O
from rnamsm import _lib, likelihood, lm, synthetic
from rnamsm.config import Config, parse_overrides

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rnamsm_lm_head", "rnamsm_lm_head_packed", "rnamsm_lm_head_workspace_bytes", "rnamsm_lm_head_packed_workspace_bytes")


def test_the_new_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnamsm.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\b(rnamsm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header, flags=re.S))
    lib = _lib.load()
    for name in NEW:
        assert name in protos and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert len(protos[name].split(",")) == len(_lib._SIGNATURES[name][1]), name
    for macro, value in (("MAX_D", _lib.LM_MAX_D), ("MAX_V", _lib.LM_MAX_V), ("MAX_BATCH", _lib.LM_MAX_BATCH),
                         ("MAX_ROWS", _lib.LM_MAX_ROWS), ("NUM_WEIGHTS", len(_lib.W_LM))):
        assert re.search(rf"#define RNAMSM_LM_{macro} {value}\b", header), macro
    assert (_lib.LM_MAX_D, _lib.LM_MAX_V, _lib.LM_MAX_BATCH, _lib.LM_MAX_ROWS) == (1024, 64, 1024, 2 ** 24)
    assert "#define RNAMSM_VERSION 600" in header and lib.rnamsm_version() == 600
    # rnamsm_lm_item as the header lays it out against the ctypes structure: names, order, offsets of a natural C layout
    item = re.search(r"typedef struct \{([^}]*)\} rnamsm_lm_item;", header).group(1)
    fields = [f.split() for f in item.split(";") if f.strip()]
    assert [f[-1] for f in fields] == [n for n, _ in _lib.LmItem._fields_]
    off = 0
    for f in fields:
        size = 8 if ("*" in "".join(f[:-1]) or "int64_t" in f) else 4
        assert "*" in "".join(f[:-1]) or f[0] in ("int64_t", "int32_t"), f
        off = -(-off // size) * size
        assert getattr(_lib.LmItem, f[-1]).offset == off, f
        off += size
    assert ctypes.sizeof(_lib.LmItem) == -(-off // 8) * 8 == 72


def test_sizes_and_refusals_that_need_no_device():
    lib = _lib.load()
    one, many = lib.rnamsm_lm_head_workspace_bytes, lib.rnamsm_lm_head_packed_workspace_bytes
    assert one(37, 768) == 37 * 768 * 4 and one(1, 64) == 256 and one(2 ** 24, 1024) == 2 ** 24 * 4096
    assert one(0, 768) == 0 and one(5, 96) == 0 and one(5, 1088) == 0 and one(5, 0) == 0 and one(2 ** 24 + 1, 64) == 0
    ns = (ctypes.c_int * 3)(5, 300, 1)
    assert many(3, ns, 768) == 2 * 256 + 306 * 768 * 4
    assert many(3, ns, 768) - 512 == sum(one(n, 768) for n in (5, 300, 1))
    assert many(5, (ctypes.c_int * 5)(1, 1, 1, 1, 1), 64) == 2 * 512 + 5 * 256              # the tables: 64 bytes a member, to 256
    assert many(0, ns, 768) == 0 and many(1025, ns, 768) == 0 and many(3, None, 768) == 0 and many(3, ns, 100) == 0
    assert many(3, (ctypes.c_int * 3)(5, 0, 1), 768) == 0 and many(2, (ctypes.c_int * 2)(2 ** 24, 1), 768) == 0

    A = 0x10000                                     # fabricated addresses: never dereferenced, every call below is refused
    w6 = (ctypes.c_void_p * 6)(*(A * (i + 1) for i in range(6)))
    ws = ctypes.c_void_p(0x900000)
    big = 1 << 40

    def item(**kw):
        f = dict(x=A, ld=768, rows=None, wt=0x20000, n=5, logits=0x30000, logp=0x40000, scores=0x50000, nll=0x60000)
        f.update(kw)
        return _lib.LmItem(*(f[n] for n, _ in _lib.LmItem._fields_))

    def refused(rc, *words):
        assert rc == -1, rc
        msg = lib.rnamsm_last_error().decode()
        assert all(w in msg for w in words), msg

    def lone(it, D=768, V=12, weights=w6, wsp=ws, nbytes=big):
        return lib.rnamsm_lm_head(ctypes.byref(it) if it is not None else None, D, V, weights, 1e-5, wsp, nbytes, None)

    def packed(its, D=768, V=12, weights=w6, wsp=ws, nbytes=big, B=None):
        arr = (_lib.LmItem * len(its))(*its)
        return lib.rnamsm_lm_head_packed(arr, len(its) if B is None else B, D, V, weights, 1e-5, wsp, nbytes, None)

    # null pointers
    refused(lone(None), "lm_head", "null pointer")
    refused(lone(item(), weights=None), "null pointer")
    refused(lone(item(), wsp=None), "null pointer")
    refused(lone(item(x=None)), "null pointer")
    refused(lone(item(), weights=(ctypes.c_void_p * 6)(A, A, None, A, A, A)), "weight pointer 2", "null")
    refused(lone(item(), weights=(ctypes.c_void_p * 6)(A, A, A, A, A + 4, A)), "weight pointer 4", "16-byte")
    refused(packed([item(), item(x=None)]), "lm_head_packed", "member 1", "null pointer")
    # the limits
    for D in (0, 32, 96, 1088):
        refused(lone(item(ld=2048), D=D), "D=")
    for V in (0, 65):
        refused(lone(item(), V=V), "V=")
    refused(packed([item()], B=0), "B=0")
    refused(packed([item()], B=1025), "B=1025")
    refused(lone(item(n=0)), "n=0")
    refused(packed([item(), item(), item(n=-3)]), "member 2", "n=-3")
    refused(lone(item(n=2 ** 24 + 1)), "rows")
    refused(packed([item(n=2 ** 23), item(n=2 ** 23), item(n=1)]), "member 2", "rows")
    # the operand rules
    refused(lone(item(ld=767)), "ld=767")
    refused(packed([item(), item(ld=700)]), "member 1", "ld=700")
    refused(lone(item(ld=770)), "multiple of 4")
    refused(lone(item(x=A + 4)), "16-byte")
    refused(lone(item(wt=None)), "without wt")
    refused(lone(item(wt=None, scores=None)), "without wt")                                 # nll alone needs it too
    refused(packed([item(), item(wt=None, nll=None)]), "member 1", "without wt")
    refused(lone(item(logits=None, logp=None, scores=None, nll=None)), "every output")
    refused(packed([item(logits=None, logp=None, scores=None, nll=None, wt=None)]), "member 0", "every output")
    refused(lone(item(logits=0x30002)), "4-byte")
    refused(lone(item(rows=0x70001)), "4-byte")
    # the workspace
    refused(lone(item(), nbytes=5 * 768 * 4 - 1), "workspace too small")
    refused(lone(item(), wsp=ctypes.c_void_p(0x900004)), "16-byte")
    refused(packed([item(), item()], nbytes=512 + 10 * 768 * 4 - 1), "workspace too small")
    refused(packed([item()], wsp=ctypes.c_void_p(0x900008)), "16-byte")


def test_the_config_key_parses_and_defaults_to_off():
    assert Config().data.lm_scores == "" and parse_overrides([]).data.lm_scores == ""
    for mode in ("", "wt", "masked"):
        assert parse_overrides([f"data.lm_scores={mode}"]).data.lm_scores == mode
    for bad in ("all", "WT", "true"):
        with pytest.raises(ValueError, match="lm_scores"):
            parse_overrides([f"data.lm_scores={bad}"])
    with pytest.raises(ValueError):
        lm.LMHead(None, "")


def _plan_is_greedy(chunks, weights, budget, cap):
    assert [i for c in chunks for i in c] == list(range(len(weights)))                      # every index once, in order
    for c in chunks:
        assert 1 <= len(c) <= cap
        assert sum(weights[i] for i in c) <= budget or len(c) == 1                          # an oversized item is alone
    for a, b in zip(chunks, chunks[1:]):                                                    # no two neighbours could be one
        assert len(a) + 1 > cap or sum(weights[i] for i in a) + weights[b[0]] > budget


def test_plan_lm_chunks_and_plan_scan_calls():
    Ls = [35, 64, 1, 128, 256, 7, 1023, 2, 2, 2]
    for budget, cap in ((lm.LM_CHUNK_ROWS, _lib.LM_MAX_BATCH), (300, 1024), (10 ** 9, 3), (1, 1024), (1100, 2)):
        _plan_is_greedy(lm.plan_lm_chunks(Ls, budget, cap), Ls, budget, cap)
    assert lm.plan_lm_chunks([]) == []
    assert lm.plan_lm_chunks([5] * 1500) == [list(range(1024)), list(range(1024, 1500))]
    assert lm.LM_CHUNK_ROWS <= _lib.LM_MAX_ROWS
    for n, R, C, budget in ((11, 5, 12, 120), (11, 5, 12, 119), (511, 256, 512, 32768), (7, 8, 17, 32768), (3, 70, 64, 4480),
                            (1, 1, 2, 0), (0, 4, 4, 100), (9, 3, 3, 9 * 9)):
        calls = likelihood.plan_scan_calls(n, R, C, budget)
        per = max(1, budget // (R * C))
        chunks = [list(range(s, e)) for s, e in calls]
        _plan_is_greedy(chunks, [R * C] * n, max(budget, R * C), per)
        assert all(e - s == per for s, e in calls[:-1]) and (not calls or 1 <= calls[-1][1] - calls[-1][0] <= per)
        assert len(calls) == -(-n // per)
    assert likelihood.plan_scan_calls(11, 5, 12, 120) == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10), (10, 11)]
    assert likelihood.plan_scan_calls(511, 256, 512, 32768) == [(i, i + 1) for i in range(511)]   # 131072 tokens: one copy per call
    with pytest.raises(ValueError):
        likelihood.plan_scan_calls(3, 0, 5, 10)


def test_scan_refuses_the_cls_column_and_past_the_end_before_touching_the_device():
    class Vocab:
        prepend_bos, append_eos = True, False
    class M:
        vocab = Vocab()
    toks = torch.zeros(3, 9, dtype=torch.int64)
    assert likelihood._scan_indices(M(), toks, None) == list(range(1, 9))
    assert likelihood._scan_indices(M(), toks, torch.tensor([8, 1, 1])) == [8, 1, 1]
    for bad in ([0], [3, 9], [-1], np.array([2, 0])):
        with pytest.raises(ValueError, match="sequence_logits"):
            likelihood._scan_indices(M(), toks, bad)


def test_lm_truth_is_the_oracle_and_its_fp32_drift_is_not_zero():
    """lm_truth.head in fp64 against oracle.lm_head in fp64 on a synthetic.make_state_dict model, and -- so that the GPU tests' bars
    are the restatement's own error and not their floors -- the fp32 restatement's distance from the truth at the GPU tests' shapes."""
    full = synthetic.make_state_dict(seed=0)
    sd = lm_truth.state_of(full)
    rng = np.random.RandomState(3)
    x = rng.standard_normal((33, 768)).astype(np.float32)
    wt = rng.randint(0, 12, 33)
    t64 = lm_truth.head(x, sd, wt)
    want = O.lm_head(torch.from_numpy(x).double(), O.to_torch_params(full, dtype=torch.float64))
    assert t64["logits"].dtype == np.float64 and np.array_equal(t64["logits"], want.numpy())
    lp = want.log_softmax(-1)
    ref = lp[torch.arange(33), torch.from_numpy(wt)]
    assert np.array_equal(t64["logp"], lp.numpy()) and np.array_equal(t64["nll"], -ref.numpy())
    assert np.array_equal(t64["scores"], (lp - ref[:, None]).numpy()) and (t64["scores"][np.arange(33), wt] == 0).all()
    bad = lm_truth.head(x[:3], sd, [-1, 12, 4])
    assert np.isnan(bad["scores"][:2]).all() and np.isnan(bad["nll"][:2]).all() and np.isfinite(bad["scores"][2]).all()
    assert np.isfinite(bad["logp"]).all()
    for D, V, n, state in ((768, 12, 33, sd), (768, 12, 1, sd), (128, 1, 37, lm_truth.head_state(128, 1, 5)),
                           (128, 64, 37, lm_truth.head_state(128, 64, 6)), (768, 12, 33, lm_truth.state_of(full, 100.0))):
        xs = np.random.RandomState(n + D).standard_normal((n, D)).astype(np.float32)
        a, b = lm_truth.head(xs, state), lm_truth.head(xs, state, dtype=torch.float32)
        assert b["logits"].dtype == np.float32
        drift = np.abs(b["logits"] - a["logits"]).max() / np.abs(a["logits"]).max()
        assert 1e-8 < drift < 1e-5, (D, V, n, drift)
