"""The CLI loop's ordering rules (rnamsm.inference._Scheduler) on the host: a fake model, fake heads and a fake sink share one trace,
and every expected trace below was written down from the loop as it stood before it was split into a scheduler and a sink (one
function, `extract_feat`, with the same names as closures) -- not from what the scheduler does.

The token limits are shrunk by assigning the module's constants, the way tools/cli_throughput.py does: an alignment of 2 x 10 = 20
tokens is small, one of 5 x 30 = 150 is not.  One departure from the issue's list of cases: a pool of THREE alignments that is
dealt in two is always a group of two and a group of one (plan_packed_groups), so "dealt in two" uses four, and three is the
"group of one" case.
"""
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from rnamsm import _lib, contacts, inference, lm, rsa, ss
from rnamsm.config import Config

PAD = 1
SMALL, BIG = (2, 10), (5, 30)


def tokens_of(idx, shape, pad=False):
    t = np.full(shape, 4, dtype=np.int64)
    t[0, 0] = 100 + idx                 # the fakes read the alignment's index here
    if pad:
        t[-1, -1] = PAD
    return t


def ident(t):
    return int(t[0, 0]) - 100


class FakeModel:
    fold_layernorm = False              # (run_pool then asks the library for nothing)

    def __init__(self, trace, max_seqlen=64, finish_fails=None):
        self.trace, self.max_seqlen = trace, max_seqlen
        self.finish_fails = finish_fails or {}          # first member's index -> "index" | "none"
        self.begin_raises = None

    def out(self, t):
        return {"emb": torch.full((t.shape[1] - 1, 1), float(ident(t))), "atp": torch.zeros(1)}

    def forward_one(self, t, has_pad, need_repr=True):
        self.trace.append(("forward_one", ident(t), has_pad))
        return self.out(t)

    def finish_forward_one(self, t, out, has_pad, need_repr=True, what=None, after=None):
        self.trace.append(("finish_forward_one", ident(t), what))
        return out

    def checked_forward_one(self, t, has_pad=False, need_repr=True, what=None):
        self.trace.append(("checked_forward_one", ident(t), what))
        return self.out(t)

    def forward_ragged(self, toks, packed=True):
        self.trace.append(("forward_ragged", [ident(t) for t in toks], packed))
        return [self.out(t) for t in toks]

    def forward_ragged_begin(self, toks):
        if self.begin_raises is not None:
            raise self.begin_raises
        self.trace.append(("forward_ragged_begin", [ident(t) for t in toks]))
        return [self.out(t) for t in toks], "mode"

    def forward_ragged_finish(self, toks, res, mode, after=None):
        assert mode == "mode" and after is not None
        self.trace.append(("forward_ragged_finish", [ident(t) for t in toks]))
        fail = self.finish_fails.get(ident(toks[0]))
        if fail == "index":
            raise IndexError("token out of range")
        return None if fail == "none" else res

    def forward_windows(self, t, stride, what=None):
        self.trace.append(("forward_windows", ident(t), what))
        return self.out(t)


class FakeHead:
    n_tensors = 1

    def __init__(self, trace, name, whole_tokens=False, stitched="one_long"):
        self.trace, self.name, self.whole_tokens, self.stitched = trace, name, whole_tokens, stitched

    def _call(self, method, emb, tokens):
        self.trace.append((method, self.name, int(emb[0, 0]), "whole" if tokens.dim() == 2 else "query"))
        return (self.name, int(emb[0, 0]))

    def one(self, emb, atp, tokens):
        return self._call("one", emb, tokens)

    def one_long(self, emb, atp, tokens):
        return self._call("one_long", emb, tokens)

    def many(self, embs, atps, tokens):
        self.trace.append(("many", self.name, [int(e[0, 0]) for e in embs], ["whole" if t.dim() == 2 else "query" for t in tokens]))
        return [(self.name, int(e[0, 0])) for e in embs]

    def stitched_route(self, L, long_on):
        self.trace.append(("stitched_route", self.name, L, long_on))
        return getattr(self, self.stitched) if self.stitched in ("one", "one_long") else self.stitched


class FakeSink:
    def __init__(self, trace):
        self.trace = trace

    def deliver(self, idx, emb, atp, after, records):
        assert int(emb[0, 0]) == idx
        self.trace.append(("deliver", idx, after is not None, records))

    def finish(self):
        self.trace.append(("sink.finish",))


class Loop:
    """A scheduler over a list of (shape, pad) alignments; `fails`: index -> the exception read() raises there."""

    def __init__(self, monkeypatch, items, *, gathering=False, heads=(), sink=None, reader=None, fails=None, max_seqlen=64,
                 trace_settle=False, **data_keys):
        monkeypatch.setattr(inference, "PACKED_SMALL_TOKENS", 100)
        monkeypatch.setattr(inference, "PIPELINE_SPLIT_TOKENS", 50)
        cfg = Config()
        for k, v in data_keys.items():
            setattr(cfg.data, k, v)
        self.trace = trace = []
        self.sw = inference.read_switches(cfg, gathering)
        assert self.sw.small_limit == 100               # the assigned constant took effect
        self.model = FakeModel(trace, max_seqlen)
        self.heads = [FakeHead(trace, *h) if isinstance(h, tuple) else h for h in heads]
        self.ids = [f"id{i}" for i in range(len(items))]
        fails = fails or {}

        def read(idx):
            if idx in fails:
                raise fails[idx]
            return tokens_of(idx, *items[idx])

        def record_event():
            return object()

        outer = self

        class Traced(inference._Scheduler):
            def settle(self):
                if trace_settle:
                    outer.trace.append(("settle",))
                super().settle()

        self.sched = Traced(self.model, self.heads, sink or FakeSink(trace), self.sw, self.ids, list(range(len(items))), read, reader,
                            PAD, torch.from_numpy, record_event)

    def run(self):
        self.sched.run()
        return self.trace

    def delivered(self):
        return [e[1] for e in self.trace if e[0] == "deliver"]


def small(n):
    return [(SMALL, False)] * n


def test_pool_dealt_in_two(monkeypatch):
    loop = Loop(monkeypatch, small(4))                  # 80 tokens >= PIPELINE_SPLIT_TOKENS: two groups of two
    for idx in range(4):
        loop.sched.step(idx, tokens_of(idx, SMALL))
    assert loop.trace == [] and len(loop.sched.pool) == 4
    loop.sched.run_pool()
    assert loop.trace == [("forward_ragged_begin", [0, 1]), ("forward_ragged_begin", [2, 3]), ("forward_ragged_finish", [0, 1]),
                          ("deliver", 0, True, []), ("deliver", 1, True, [])]
    assert loop.sched.inflight is not None and loop.sched.pool == []      # the last group stays in flight
    loop.sched.settle()
    assert loop.trace[5:] == [("forward_ragged_finish", [2, 3]), ("deliver", 2, True, []), ("deliver", 3, True, [])]
    assert loop.sched.inflight is None


def test_pool_dealt_in_two_with_heads(monkeypatch):
    trace = Loop(monkeypatch, small(4), heads=[("A",), ("B", True)]).run()
    group = lambda a, b: [("forward_ragged_finish", [a, b]), ("many", "A", [a, b], ["query", "query"]),      # noqa: E731
                          ("many", "B", [a, b], ["whole", "whole"]),
                          ("deliver", a, True, [("A", a), ("B", a)]), ("deliver", b, True, [("A", b), ("B", b)])]
    assert trace == ([("forward_ragged_begin", [0, 1]), ("forward_ragged_begin", [2, 3])] + group(0, 1) + group(2, 3)
                     + [("sink.finish",)])


def test_full_pool_starts_before_the_next_read(monkeypatch):
    monkeypatch.setattr(inference, "PACKED_TOKENS", 40)                  # two alignments of 20 tokens fill a group
    loop = Loop(monkeypatch, small(4))
    monkeypatch.setattr(inference, "PIPELINE_SPLIT_TOKENS", 0)
    loop.sched.step(0, tokens_of(0, SMALL))
    assert loop.trace == []
    loop.sched.step(1, tokens_of(1, SMALL))
    assert loop.trace == [("forward_ragged_begin", [0, 1])]
    loop.sched.step(2, tokens_of(2, SMALL))
    loop.sched.step(3, tokens_of(3, SMALL))
    assert loop.trace[1:] == [("forward_ragged_begin", [2, 3]), ("forward_ragged_finish", [0, 1]), ("deliver", 0, True, []),
                              ("deliver", 1, True, [])]
    loop.sched.drain()
    assert loop.delivered() == [0, 1, 2, 3]


def test_group_of_one_goes_alone(monkeypatch):
    trace = Loop(monkeypatch, small(3)).run()           # 60 tokens: dealt into [0, 1] and [2]
    assert trace == [("forward_ragged_begin", [0, 1]), ("forward_ragged_finish", [0, 1]), ("deliver", 0, True, []),
                     ("deliver", 1, True, []), ("checked_forward_one", 2, "id2"), ("deliver", 2, False, []), ("sink.finish",)]


def test_group_of_one_finishes_what_is_in_flight_first(monkeypatch):
    loop = Loop(monkeypatch, [(BIG, False)] + small(3))
    assert loop.run() == [("forward_one", 0, False), ("forward_ragged_begin", [1, 2]), ("finish_forward_one", 0, "id0"),
                          ("deliver", 0, True, []), ("forward_ragged_finish", [1, 2]), ("deliver", 1, True, []),
                          ("deliver", 2, True, []), ("checked_forward_one", 3, "id3"), ("deliver", 3, False, []), ("sink.finish",)]


@pytest.mark.parametrize("threaded", [False, True])
def test_two_lone_alignments(monkeypatch, threaded):
    reader = ThreadPoolExecutor(1) if threaded else None
    try:
        trace = Loop(monkeypatch, [(BIG, False)] * 2, heads=[("A",)], reader=reader).run()
    finally:
        if reader is not None:
            reader.shutdown(wait=True)
    assert trace == [("forward_one", 0, False), ("forward_one", 1, False),
                     ("finish_forward_one", 0, "id0"), ("one", "A", 0, "query"), ("deliver", 0, True, [("A", 0)]),
                     ("finish_forward_one", 1, "id1"), ("one", "A", 1, "query"), ("deliver", 1, True, [("A", 1)]), ("sink.finish",)]


def test_gatherer_present(monkeypatch):
    loop = Loop(monkeypatch, small(2) + [(BIG, False)] + small(1), gathering=True, trace_settle=True)
    assert not loop.sw.pooled
    trace = loop.run()
    assert trace == [("forward_ragged", [0, 1], True), ("deliver", 0, False, []), ("deliver", 1, False, []),
                     ("settle",), ("checked_forward_one", 2, "id2"), ("deliver", 2, False, []),
                     ("checked_forward_one", 3, "id3"), ("deliver", 3, False, []), ("settle",), ("sink.finish",)]
    assert loop.delivered() == [0, 1, 2, 3]             # this rank's items in list order


def test_wide_alignment_under_windows(monkeypatch, capsys):
    lone, wide = ((10, 12), False), ((2, 20), False)    # 120 tokens: not small; 40 tokens, but wider than the model: never in a group
    loop = Loop(monkeypatch, [lone, wide, wide], max_seqlen=16, trace_settle=True, long_msa="windows", long_heads="stitched",
                window_stride=7, heads=[("A", False, "one_long"), ("B", True, "one"), ("C", False, "no route")])
    trace = loop.run()
    asked = [e for e in trace if e[0] == "stitched_route"]
    assert set(asked) == {("stitched_route", n, 19, True) for n in "ABC"}       # only the stitched alignments ask the heads
    one_wide = lambda i: [("forward_windows", i, f"id{i}"), ("one_long", "A", i, "query"), ("one", "B", i, "whole"),      # noqa: E731
                          ("deliver", i, False, [("A", i), ("B", i), None])]
    assert [e for e in trace if e not in asked] == (
        [("forward_one", 0, False), ("settle",), ("settle",), ("finish_forward_one", 0, "id0"), ("one", "A", 0, "query"),
         ("one", "B", 0, "whole"), ("one", "C", 0, "query"), ("deliver", 0, True, [("A", 0), ("B", 0), ("C", 0)])]
        + one_wide(1) + [("settle",)] + one_wide(2) + [("settle",), ("sink.finish",)])
    assert capsys.readouterr().out == "".join(
        f"id{i}: L=19 is stitched from windows (data.long_msa=windows); FakeHead is skipped for it (no route)\n" for i in (1, 2))


class _Alphabet:
    all_toks = ["<cls>", "<pad>", "<eos>", "<unk>", "A", "G", "C", "U", "X", "N", "-"]


class _Predictor:
    def __init__(self, gemm_dtype):
        self.gemm_dtype = gemm_dtype


def real_heads(ss_dtype="f32", lm_mode="masked"):
    """The four head classes, as far as their stitched answer goes (nothing of them is run)."""
    lm_head = lm.LMHead.__new__(lm.LMHead)
    lm_head.mode = lm_mode
    return [ss.SSHead(_Predictor(ss_dtype), _Alphabet, None, "cpu", text_on=False, pairs_on=False),
            rsa.RSAHead(None, _Alphabet, None, None, model_names=["m"]),
            contacts.ContactHead(torch.zeros(4), torch.zeros(1)), lm_head]


def test_stitched_route_table():
    """Today's runner or reason for every combination: the masked LM reason before the LONG_MAX_L one, the SS gemm_dtype one after it."""
    at, above = _lib.LONG_MAX_L, _lib.LONG_MAX_L + 1
    limit = f"L exceeds the long heads' limit of {_lib.LONG_MAX_L}"
    masked = "the masked scan would run L forwards per window"
    for ss_dtype in ("f32", "bf16"):
        for lm_mode in ("wt", "masked"):
            s, r, c, m = real_heads(ss_dtype, lm_mode)
            for L in (at, above):
                assert [h.stitched_route(L, False) for h in (s, r, c)] == ["", "", ""]
                assert m.stitched_route(L, False) == (m.one if lm_mode == "wt" else "")
                assert m.stitched_route(L, True) == (m.one if lm_mode == "wt" else masked)
            no_ss = f"there is no long SS head under data.ss_gemm_dtype={ss_dtype}"
            assert s.stitched_route(at, True) == (s.one_long if ss_dtype == "f32" else no_ss)
            assert [r.stitched_route(at, True), c.stitched_route(at, True)] == [r.one_long, c.one_long]
            assert [h.stitched_route(above, True) for h in (s, r, c)] == [limit] * 3
    assert lm.LMHead.skip_suffix == "(masked)"


@pytest.mark.parametrize("long_heads, columns, ss_dtype, expected", [
    ("skip", 20, "f32", ["SSHead", "RSAHead", "ContactHead", "LMHead(masked)"]),
    ("stitched", 20, "bf16", ["SSHead (there is no long SS head under data.ss_gemm_dtype=bf16)", None, None,
                              "LMHead(masked) (the masked scan would run L forwards per window)"]),
    ("stitched", _lib.LONG_MAX_L + 2, "f32", [f"{n} (L exceeds the long heads' limit of {_lib.LONG_MAX_L})"
                                              for n in ("SSHead", "RSAHead", "ContactHead")]
     + ["LMHead(masked) (the masked scan would run L forwards per window)"])])
def test_skip_lines_of_the_real_heads(monkeypatch, capsys, long_heads, columns, ss_dtype, expected):
    heads = [h for h, e in zip(real_heads(ss_dtype), expected) if e is not None]        # (a head that would run needs the device)
    loop = Loop(monkeypatch, [((1, columns), False)], heads=heads, max_seqlen=16, long_msa="windows", long_heads=long_heads)
    assert loop.run() == [("forward_windows", 0, "id0"), ("deliver", 0, False, [None] * len(heads)), ("sink.finish",)]
    lines = []
    for e in expected:
        if e is not None:
            name, _, why = e.partition(" ")
            lines.append(f"id0: L={columns - 1} is stitched from windows (data.long_msa=windows); {name} is skipped for it{' ' + why if why else ''}\n")
    assert capsys.readouterr().out == "".join(lines)


def test_padded_alignment_goes_alone(monkeypatch):
    trace = Loop(monkeypatch, [(SMALL, False), (SMALL, True), (SMALL, False)]).run()
    assert trace == [("forward_one", 1, True), ("forward_ragged_begin", [0, 2]), ("finish_forward_one", 1, "id1"), ("deliver", 1, True, []),
                     ("forward_ragged_finish", [0, 2]), ("deliver", 0, True, []), ("deliver", 2, True, []), ("sink.finish",)]


@pytest.mark.parametrize("fail, rerun", [
    ("none", [("forward_ragged", [0, 1], False)]),
    ("index", [("checked_forward_one", 0, "id0"), ("checked_forward_one", 1, "id1")])])
def test_packed_group_rerun(monkeypatch, fail, rerun):
    loop = Loop(monkeypatch, small(4))
    loop.model.finish_fails = {0: fail}
    assert loop.run() == ([("forward_ragged_begin", [0, 1]), ("forward_ragged_begin", [2, 3]), ("forward_ragged_finish", [0, 1])] + rerun
                          + [("deliver", 0, False, []), ("deliver", 1, False, []),          # a rerun's outputs wait for everything enqueued
                             ("forward_ragged_finish", [2, 3]), ("deliver", 2, True, []), ("deliver", 3, True, []), ("sink.finish",)])


def test_salvage_delivers_what_waits_then_raises(monkeypatch):
    loop = Loop(monkeypatch, [(BIG, False)] + small(4), fails={3: ValueError("bad alignment")})
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError, match="bad alignment"):
            loop.run()
    assert loop.trace == [("forward_one", 0, False), ("forward_ragged_begin", [1, 2]), ("finish_forward_one", 0, "id0"),
                          ("deliver", 0, True, []), ("forward_ragged_finish", [1, 2]), ("deliver", 1, True, []), ("deliver", 2, True, [])]
    assert loop.sched.pool == [] and loop.sched.group == [] and loop.sched.inflight is None


def test_second_failure_in_the_salvage_is_a_warning(monkeypatch):
    loop = Loop(monkeypatch, small(3), fails={2: ValueError("bad alignment")})
    loop.model.begin_raises = RuntimeError("second")
    with pytest.warns(UserWarning, match="while writing the results computed before the error: RuntimeError: second"):
        with pytest.raises(ValueError, match="bad alignment"):
            loop.run()


def test_no_salvage_under_a_gatherer(monkeypatch):
    loop = Loop(monkeypatch, small(3), gathering=True, fails={2: ValueError("bad alignment")})
    with pytest.raises(ValueError, match="bad alignment"):
        loop.run()
    assert loop.trace == [] and len(loop.sched.group) == 2


def test_keyboard_interrupt_is_not_caught(monkeypatch):
    loop = Loop(monkeypatch, small(3), fails={2: KeyboardInterrupt()})
    with pytest.raises(KeyboardInterrupt):
        loop.run()
    assert loop.trace == [] and len(loop.sched.pool) == 2


@pytest.mark.parametrize("items", [small(4), small(3), [(BIG, False)] + small(3), [(BIG, False)] * 2,
                                   [(SMALL, False), (SMALL, True), (SMALL, False)], [(SMALL, False), (BIG, False), (SMALL, False)]])
def test_every_index_is_delivered_exactly_once(monkeypatch, items):
    loop = Loop(monkeypatch, items)
    loop.run()
    assert sorted(loop.delivered()) == list(range(len(items)))


def test_real_sink_returns_list_order(monkeypatch, tmp_path):
    """The sink's sequential route (async_io=False) needs no device: the files land, and the ids come back in list order although
    the large alignment in the middle is delivered first."""
    ids = ["id0", "id1", "id2"]
    sw = inference.read_switches(Config(), False)
    sink = inference._Sink(ids, [], tmp_path, sw, 64, None, 0, async_io=False)
    loop = Loop(monkeypatch, [(SMALL, False), (BIG, False), (SMALL, False)], sink=sink)
    loop.run()
    assert sink.written == ["id1", "id0", "id2"]
    assert sink.written_in_list_order() == ids
    sink.close()
    for i, name in enumerate(ids):
        assert np.load(tmp_path / f"{name}_emb.npy")[0, 0] == i and (tmp_path / f"{name}_atp.npy").exists()
