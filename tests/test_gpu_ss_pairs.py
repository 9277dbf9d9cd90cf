"""The structure decoded on the GPU (rnamsm_ss_pairs / _packed, rnamsm.ss.structure, SSPredictor.predict_structure,
write_ss_files(partner=..., ...), the CLI key data.ss_pairs_device).  Expected values are always the host path called the old way
(ss.secondary_structure, ss.write_ss_files(prob, seq, name, dir)) or the reference-made fixtures; every comparison is == on
integers or bytes."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from rnamsm import _lib, ops, ss, synthetic
import ss_pairs_cases as C
import ss_truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(prob: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(prob, dtype=np.float32)).to(DEV)


def _letters(seq: str) -> torch.Tensor:
    return torch.from_numpy(ss.letter_codes(seq)).to(DEV)


def _host(out):
    """One (partner, counts, ct body, bpseq body) of the device -> (partner list, counts list, ct bytes, bpseq bytes); the bytes
    behind the counts must have been left alone by the kernel only as far as the buffers' bounds go: shapes are checked here."""
    partner, counts, ct, bp = (t.cpu().numpy() for t in out)
    L = partner.shape[0]
    assert partner.dtype == np.int32 and counts.dtype == np.int32 and counts.shape == (4,)
    assert ct.shape == (32 * L,) and bp.shape == (12 * L,) and ct.dtype == np.uint8
    assert 0 < counts[1] <= 32 * L and 0 < counts[2] <= 12 * L
    return partner.tolist(), counts.tolist(), ct[:counts[1]].tobytes(), bp[:counts[2]].tobytes()


def _lone(prob: np.ndarray, seq: str):
    return _host(ops.ss_pairs(_dev(prob), _letters(seq)))


def _check(key: str, prob: np.ndarray, seq: str, got=None, expect_prob=None):
    """The device's outputs for (prob, seq) against the host path on expect_prob (default: prob itself)."""
    pairs, partner, ct, bp, _, _ = C.expected(key, prob if expect_prob is None else expect_prob, seq)
    g_partner, g_counts, g_ct, g_bp = got if got is not None else _lone(prob, seq)
    assert g_partner == partner.tolist(), key
    assert ss.pairs_from_partner(np.array(g_partner)) == pairs, key
    assert g_counts == [len(pairs), len(ct), len(bp), 0], key
    assert g_ct == ct, key
    assert g_bp == bp, key
    return pairs


# ------------------------------------------------------------------ lone call
@pytest.mark.parametrize("L", [1, 2, 3, 35, 63, 64, 65, 128, 129])
def test_lone_call_equals_the_host_path(L):
    """Sigmoid outputs of logits N(-4, 3): a tenth of the pairs above the threshold, multiplets at every L >= 35; the ballot-word
    seam at 63 / 64 / 65 and 128 / 129."""
    prob, seq = C.random_sigmoid(L, 100 + L, -4.0), C.seq_for(L, L)
    pairs = _check(f"random_{L}", prob, seq)
    if L >= 35:
        assert 0 < len(pairs) < int((prob[np.triu_indices(L, k=1)] > np.float32(0.516)).sum())


def test_lone_call_at_the_limit_with_planted_multiplets():
    prob, seq = C.helix_noise_1024(), C.seq_for(1024, 9)
    pairs = _check("helix_1024", prob, seq)
    assert len(pairs) < int((prob[np.triu_indices(1024, k=1)] > np.float32(0.516)).sum())      # the host function removed pairs
    assert (300, 802) in pairs and (300, 800) not in pairs and (300, 801) not in pairs          # ... over two rounds


@pytest.mark.parametrize("L", [65, 129])
def test_all_equal_dense_matrix_runs_l_minus_2_rounds(L):
    pairs = _check(f"dense_{L}", C.dense(L), C.seq_for(L, L))
    assert len(pairs) == 1


def test_quantised_ties():
    prob, seq = C.standard_cases()["ties_65"]
    _check("ties_65", prob, seq)


@pytest.mark.parametrize("kind", ["nan", "one", "transposed"])
def test_only_the_upper_triangle_is_read(kind):
    prob, seq = C.random_sigmoid(70, 31, -3.0), C.seq_for(70, 31)
    _check("upper_70", C.with_garbage_below(prob, kind), seq, expect_prob=np.triu(prob, k=1))


@pytest.mark.parametrize("key", ["sprinkled_1", "sprinkled_17", "sprinkled_64", "sprinkled_70"])
def test_nan_and_inf_have_a_defined_outcome(key):
    prob, seq = C.standard_cases()[key]
    assert key == "sprinkled_1" or (np.isnan(prob).any() and np.isposinf(prob).any() and np.isneginf(prob).any())
    _check(key, prob, seq)


@pytest.mark.parametrize("case", C.FIXTURE_CASES)
def test_fixture_cases_equal_their_stored_tables(case, tmp_path):
    prob, seq, ct_file, bp_file = C.fixture(case)
    partner, counts, ct, bp = (t.cpu().numpy() for t in ss.structure(_dev(prob), _letters(seq)))
    pairs = ss.write_ss_files(None, seq, case, tmp_path, prob_text=b"0" * (25 * len(seq) ** 2), partner=partner, counts=counts,
                              ct_body=ct, bpseq_body=bp)
    assert (tmp_path / "SS_result" / f"{case}.ct").read_bytes() == ct_file
    assert (tmp_path / "SS_result" / f"{case}.bpseq").read_bytes() == bp_file
    assert pairs == ss.secondary_structure(prob)


def test_the_iterative_case_and_its_transpose():
    for key in ("iterative_6x6", "iterative_6x6_T"):
        prob, seq = C.standard_cases()[key]
        _check(key, prob, seq)
    assert _lone(C.iterative_6x6(), "ACGUAC")[0] == [4, 0, 5, 1, 3, 0]
    assert _lone(C.iterative_6x6().T.copy(), "ACGUAC")[0] == [0] * 6


# ------------------------------------------------------------------ packed call
PACKED_LS = [1, 35, 64, 65, 129, 2]


@pytest.fixture(scope="module")
def packed_cases():
    """The members and their lone outputs, computed once."""
    members = [(C.random_sigmoid(L, 100 + L, -4.0), C.seq_for(L, L)) for L in PACKED_LS]
    return members, [_lone(p, s) for p, s in members]


def _packed(members):
    return [_host(o) for o in ops.ss_pairs_packed([_dev(p) for p, _ in members], [_letters(s) for _, s in members])]


@pytest.mark.parametrize("reverse", [False, True])
def test_every_member_has_the_lone_call_s_bytes(packed_cases, reverse):
    members, lone = (list(reversed(v)) if reverse else v for v in packed_cases)
    got = _packed(members)
    assert len(got) == len(members)
    for b, (prob, seq) in enumerate(members):
        assert got[b] == lone[b], (b, len(seq))
        _check(f"random_{len(seq)}", prob, seq, got=got[b])


def test_more_members_than_one_descriptor_chunk():
    """33 members of L = 5 .. 37: 32 descriptors travel per launch, so the last member is a launch of its own."""
    members = [(C.random_sigmoid(5 + i, 400 + i, -2.0), C.seq_for(5 + i, i)) for i in range(33)]
    got = _packed(members)
    assert len(got) == 33
    for b, (prob, seq) in enumerate(members):
        assert got[b] == _lone(prob, seq), b
        _check(f"chunk_{b}", prob, seq, got=got[b])
    many = ss.structure_many([_dev(p) for p, _ in members], [_letters(s) for _, s in members])
    assert [_host(o) for o in many] == got


def test_a_dense_member_leaves_its_neighbours_alone(packed_cases):
    members, lone = (list(v) for v in packed_cases)
    members[2] = (C.dense(64), members[2][1])
    got = _packed(members)
    for b in (0, 1, 3, 4, 5):
        assert got[b] == lone[b], b
    assert got[2][1][0] == 1 and got[2] == _lone(*members[2])


def test_the_workspace_s_contents_do_not_matter(packed_cases):
    """The C ABI itself on a workspace pre-filled with 0xFF (and outputs pre-filled too): the lone outputs again."""
    members, lone = packed_cases
    lib = _lib.load()
    B, Ls = len(members), [len(s) for _, s in members]
    ws = torch.full((lib.rnamsm_ss_pairs_workspace_bytes(B, (_lib.c_int * B)(*Ls)),), 0xFF, dtype=torch.uint8, device=DEV)
    keep, outs = [], []
    items = (_lib.SsPairsItem * B)()
    for b, (prob, seq) in enumerate(members):
        L = Ls[b]
        p, l = _dev(prob), _letters(seq)
        o = (torch.full((L,), -1, dtype=torch.int32, device=DEV), torch.full((4,), -1, dtype=torch.int32, device=DEV),
             torch.full((32 * L,), 0xFF, dtype=torch.uint8, device=DEV), torch.full((12 * L,), 0xFF, dtype=torch.uint8, device=DEV))
        keep += [p, l]
        outs.append(o)
        items[b] = _lib.SsPairsItem(p.data_ptr(), l.data_ptr(), L, *[t.data_ptr() for t in o])
    _lib.check(lib.rnamsm_ss_pairs_packed(items, B, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for b, o in enumerate(outs):
        assert _host(o) == lone[b], b
        n_ct, n_bp = lone[b][1][1], lone[b][1][2]
        assert bool((o[2][n_ct:] == 0xFF).all()) and bool((o[3][n_bp:] == 0xFF).all()), b       # nothing behind the counts


# ------------------------------------------------------------------ letters
def test_a_letter_outside_ascii_marks_its_own_member_only(packed_cases, tmp_path):
    members, lone = (list(v) for v in packed_cases)
    letters = [_letters(s) for _, s in members]
    letters[1] = letters[1].clone()
    letters[1][7] = 0
    letters[3] = letters[3].clone()
    letters[3][64] = 200
    got = [_host(o) for o in ops.ss_pairs_packed([_dev(p) for p, _ in members], letters)]
    assert [g[1][3] for g in got] == [0, 1, 0, 1, 0, 0]
    for b in range(len(members)):
        assert got[b][0] == lone[b][0] and got[b][1][0] == lone[b][1][0], b                       # the partners stay right
    for b in (0, 2, 4, 5):
        assert got[b] == lone[b], b
    # write_ss_files then builds the host tables from the partner vector
    prob, seq = members[1]
    g = got[1]
    ss.write_ss_files(prob, seq, "x", tmp_path / "host")
    ss.write_ss_files(prob, seq, "x", tmp_path / "dev", partner=np.array(g[0]), counts=np.array(g[1]),
                      ct_body=np.full(32 * 35, ord("?"), dtype=np.uint8), bpseq_body=np.full(12 * 35, ord("?"), dtype=np.uint8))
    for ext in ("ct", "bpseq", "prob"):
        assert (tmp_path / "dev" / "SS_result" / f"x.{ext}").read_bytes() == (tmp_path / "host" / "SS_result" / f"x.{ext}").read_bytes()


# ------------------------------------------------------------------ predictor
@pytest.fixture(scope="module")
def head():
    model = ss.SSPredictor(4)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ss_truth.make_state(4, seed=21).items()}, strict=True)
    return model.eval().to(DEV)


def _files(root, name="x"):
    return {ext: (root / "SS_result" / f"{name}.{ext}").read_bytes() for ext in ("ct", "bpseq", "prob")}


def test_predict_structure_is_predict_plus_the_host_path(head, tmp_path):
    atp = torch.from_numpy(np.load(os.path.join(GOLDEN, "ss", "2DRB_1_atp.npy"))).to(DEV)
    L = atp.shape[-1]
    seqs = ["".join(np.random.RandomState(5 + k).choice(list("ACGU"), L)) for k in range(2)]
    want = [head.predict(atp, s).cpu().numpy() for s in seqs]
    lone = [head.predict_structure(atp, s) for s in seqs]
    many = head.predict_structure_many([atp, atp], seqs)
    for k, seq in enumerate(seqs):
        ss.write_ss_files(want[k], seq, "x", tmp_path / f"host{k}")
        for tag, out in (("lone", lone[k]), ("many", many[k])):
            prob, partner, counts, ct, bp = (t.cpu().numpy() for t in out)
            assert np.array_equal(prob, want[k])
            pairs = ss.write_ss_files(prob, seq, "x", tmp_path / f"{tag}{k}", partner=partner, counts=counts, ct_body=ct, bpseq_body=bp)
            assert pairs == ss.secondary_structure(want[k]) and counts[3] == 0
            assert _files(tmp_path / f"{tag}{k}") == _files(tmp_path / f"host{k}")
    codes = torch.from_numpy(ss.base_codes(seqs[0]))
    with pytest.raises(ValueError):
        head.predict_structure(atp, codes)                                      # base codes carry no letters
    out = head.predict_structure(atp, codes, letters=ss.letter_codes(seqs[0]))
    assert torch.equal(out[0], lone[0][0]) and _host(out[1:]) == _host(lone[0][1:])      # the bodies as far as their counts go


# ------------------------------------------------------------------ misuse
def test_misuse_is_refused_before_any_launch():
    ok_l = torch.zeros(4, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.RnamsmError):
        ops.ss_pairs(torch.zeros(4, 4), ok_l)                                   # no CPU path
    with pytest.raises(_lib.RnamsmError):
        ops.ss_pairs(torch.zeros(4, 4, device=DEV), torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.ss_pairs(torch.zeros(4, 5, device=DEV), ok_l)
    with pytest.raises(ValueError):
        ops.ss_pairs(torch.zeros(4, 4, device=DEV), torch.zeros(5, dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError):
        ops.ss_pairs(torch.zeros(4, 4, device=DEV), ok_l.to(torch.int32))
    with pytest.raises(ValueError):
        ops.ss_pairs(torch.zeros(1025, 1025, device=DEV), torch.zeros(1025, dtype=torch.uint8, device=DEV))
    one = torch.zeros(1, 1, device=DEV)
    with pytest.raises(ValueError):
        ops.ss_pairs_packed([one] * 1025, [ok_l[:1]] * 1025)
    with pytest.raises(ValueError):
        ops.ss_pairs_packed([one, one], [ok_l[:1]])
    assert ops.ss_pairs_packed([], []) == []
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    probs = torch.full((4, 4), 0.9, device=DEV)
    outs = (torch.full((4,), 7, dtype=torch.int32, device=DEV), torch.full((4,), 7, dtype=torch.int32, device=DEV),
            torch.full((128,), 7, dtype=torch.uint8, device=DEV), torch.full((48,), 7, dtype=torch.uint8, device=DEV))
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    args = [probs.data_ptr(), ok_l.data_ptr(), 4] + [t.data_ptr() for t in outs] + [ws.data_ptr(), 256, stream]
    for pos, value, needle in ((2, 0, "L=0"), (2, 1025, "L=1025"), (0, None, "null"), (7, None, "null"), (8, 255, "256 needed"),
                               (7, ws.data_ptr() + 8, "16-byte"), (3, outs[0].data_ptr() + 2, "4-byte")):
        bad = list(args)
        bad[pos] = value
        assert lib.rnamsm_ss_pairs(*bad) == -1
        assert needle in lib.rnamsm_last_error().decode(), needle
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outs)                              # nothing was launched


# ------------------------------------------------------------------ CLI
SHAPES = [(170, 100), (4, 12), (8, 40), (5, 17)]      # 170 x 101 tokens: alone; the rest share a packed group
IDS = [f"rna{k}" for k in range(len(SHAPES))]


@pytest.fixture(scope="module")
def cli_setup(tmp_path_factory):
    """The four-alignment setup of test_gpu_ss_text.py::test_cli_files_do_not_depend_on_the_key."""
    root = tmp_path_factory.mktemp("ss_pairs_cli")
    state = synthetic.make_state_dict(seed=0, num_layers=10)
    ckpt = root / "model.ckpt"
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in state.items()}}, ckpt)
    ss_pt = root / "model" / "rna-msm_attention.pt"
    ss_pt.parent.mkdir(parents=True)
    torch.save({k: torch.from_numpy(v) for k, v in ss_truth.make_state(4, seed=5).items()}, ss_pt)
    rng = np.random.RandomState(92)
    texts = {i: "".join(f">s{r}\n{''.join(rng.choice(list('ACGU'), L))}\n" for r in range(R)) for i, (R, L) in zip(IDS, SHAPES)}
    (root / "rna_id.txt").write_text("\n".join(IDS) + "\n")
    return root, ckpt, ss_pt, texts


def _run_cli(setup, monkeypatch, name, extra):
    root, ckpt, ss_pt, texts = setup
    sys.path.insert(0, ROOT)
    import RNA_MSM_Inference as cli
    real_load = ss.load_predictor
    monkeypatch.setattr(ss, "load_predictor", lambda path, device, num_blocks=4: real_load(path, device, num_blocks))
    res = root / name
    res.mkdir()
    for i in IDS:
        (res / f"{i}.a2m_msa2").write_text(texts[i])
    cli.main([f"data.root_path={root}", f"data.MSA_path={name}", f"data.model_path={ckpt}", "data.MSA_list=rna_id.txt",
              "data.max_seqs_per_msa=256", "data.sample_method=first", f"data.ss_model_path={ss_pt}"] + extra)
    return {(i, ext): (res / "SS_result" / f"{i}.{ext}").read_bytes() for i in IDS for ext in ("prob", "ct", "bpseq")}


@pytest.fixture(scope="module")
def cli_host_files(cli_setup):
    """The parent's path: both keys off."""
    mp = pytest.MonkeyPatch()
    try:
        files = _run_cli(cli_setup, mp, "host", ["data.ss_pairs_device=false", "data.ss_prob_text=false"])
    finally:
        mp.undo()
    assert all(files.values())
    return files


def _count_calls(monkeypatch):
    lone_calls, packed_calls, jobs = [], [], []
    real_lone, real_packed = ops.ss_pairs, ops.ss_pairs_packed
    monkeypatch.setattr(ops, "ss_pairs", lambda p, l: lone_calls.append(p.shape[0]) or real_lone(p, l))
    monkeypatch.setattr(ops, "ss_pairs_packed", lambda ps, ls: packed_calls.append(len(ps)) or real_packed(ps, ls))
    from rnamsm import inference
    real_submit = inference._AsyncNpyWriter.submit

    def submit(self, job_list, done, after=None):
        for _, t in job_list:                   # every tensor of a job: a head's job carries a tuple of them
            jobs.extend((tuple(x.shape), x.dtype) for x in (t if isinstance(t, tuple) else (t,)))
        return real_submit(self, job_list, done, after=after)

    monkeypatch.setattr(inference._AsyncNpyWriter, "submit", submit)
    return lone_calls, packed_calls, jobs


def _square_float_jobs(jobs):
    return [j for j in jobs if len(j[0]) == 2 and j[0][0] == j[0][1] and j[1] == torch.float32]


@pytest.mark.parametrize("pairs_on, text_on", [(True, True), (True, False), (False, True)])
def test_cli_files_do_not_depend_on_the_keys(cli_setup, cli_host_files, monkeypatch, pairs_on, text_on):
    lone_calls, packed_calls, jobs = _count_calls(monkeypatch)
    files = _run_cli(cli_setup, monkeypatch, f"p{int(pairs_on)}t{int(text_on)}",
                     [f"data.ss_pairs_device={str(pairs_on).lower()}", f"data.ss_prob_text={str(text_on).lower()}"])
    assert files == cli_host_files
    if pairs_on:
        assert lone_calls == [100] and packed_calls == [3], (lone_calls, packed_calls)
    else:
        assert lone_calls == [] and packed_calls == []
    if pairs_on and text_on:
        assert _square_float_jobs(jobs) == [], jobs                             # no [L, L] float copy was enqueued
    else:
        assert sorted(j[0][0] for j in _square_float_jobs(jobs)) == sorted(L for _, L in SHAPES)


def test_cli_nan_poisoned_structures_get_the_host_path_s_files(cli_setup, monkeypatch):
    """A NaN in the lone structure's probabilities and in one of the packed group's: with both keys on (the default) the files are
    those of the host path on the same poisoned maps."""
    real_head, real_packed = ops.ss_head, ops.ss_head_packed

    def head(*a, **k):
        out = real_head(*a, **k)
        out[3, 4] = float("nan")
        return out

    def head_packed(*a, **k):
        outs = real_packed(*a, **k)
        outs[1][2, 5] = float("nan")
        return outs

    monkeypatch.setattr(ops, "ss_head", head)
    monkeypatch.setattr(ops, "ss_head_packed", head_packed)
    host = _run_cli(cli_setup, monkeypatch, "nan_host", ["data.ss_pairs_device=false", "data.ss_prob_text=false"])
    lone_calls, packed_calls, jobs = _count_calls(monkeypatch)
    dev = _run_cli(cli_setup, monkeypatch, "nan_dev", [])
    assert dev == host
    assert sum(b"nan" in v for (i, ext), v in dev.items() if ext == "prob") == 2
    assert lone_calls == [100] and packed_calls == [3] and _square_float_jobs(jobs) == []
