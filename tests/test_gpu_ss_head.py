"""RNA-MSM-SS head on the GPU (rnamsm.ss -> rnamsm_ss_head): parity with the reference's own network (ss_head_b2_l35.npz),
16 random-weight blocks against the fp64 restatement (tests/ss_truth.py) from L = 1 to 1024, the zero padding of the conv
inputs, run-to-run bits, the forward's device-resident maps, the CLI key data.ss_model_path, SS_predict.py and the refusals."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, golden, rel_l2
from rnamsm import _lib, ss, synthetic
import ss_truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SS_DIR = os.path.join(GOLDEN, "ss")


def _predictor(state, num_blocks):
    m = ss.SSPredictor(num_blocks)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV)


def _case(L, seed):
    """Attention-like maps (rows on the simplex) and a sequence with one character outside A, C, G, U."""
    rng = np.random.RandomState(seed)
    atp = rng.exponential(size=(120, L, L)).astype(np.float32)
    atp /= atp.sum(-1, keepdims=True)
    seq = "".join(rng.choice(list("ACGU"), L))
    if L > 3:
        seq = seq[:2] + "N" + seq[3:]
    return atp, seq


def _check(L, state, num_blocks, seed, device="cpu"):
    atp, seq = _case(L, seed)
    got = _predictor(state, num_blocks).logits(torch.from_numpy(atp).to(DEV), seq).cpu().numpy().astype(np.float64)
    x = ss_truth.features(atp, seq)
    t64 = ss_truth.logits(x, state, torch.float64, device)
    t32 = ss_truth.logits(x, state, torch.float32, device).astype(np.float64)
    assert got.shape == (L, L)
    ss_truth.compare(got, t64, t32, f"L={L}", seams=True)      # rel-L2 <= 2 x the restatement's, and element-wise
    return got


def test_matches_the_reference_network_fixture():
    g = golden("ss_head_b2_l35.npz")
    state = {k[3:]: g[k] for k in g.files if k.startswith("sd/")}
    atp = np.load(os.path.join(SS_DIR, "2DRB_1_atp.npy"))
    model = _predictor(state, 2)
    got = model.logits(torch.from_numpy(atp).to(DEV), str(g["seq"])).cpu().numpy().astype(np.float64)
    ref32, ref64 = g["logits"].astype(np.float64), g["logits_f64"]
    print(f"fixture: max-abs vs reference fp64 {np.abs(got - ref64).max():.2e}, reference fp32 vs fp64 "
          f"{np.abs(ref32 - ref64).max():.2e}")
    assert np.abs(got - ref64).max() <= 2 * np.abs(ref32 - ref64).max()
    assert rel_l2(got, ref64) <= 2 * rel_l2(ref32, ref64)
    probs = model.predict(torch.from_numpy(atp).to(DEV), str(g["seq"])).cpu().numpy()
    np.testing.assert_allclose(probs, 1 / (1 + np.exp(-got)), rtol=0, atol=1e-6)


@pytest.mark.parametrize("L", [1, 2, 5, 17, 35, 64, 100, 129, 256])
def test_sixteen_blocks_against_fp64(L):
    _check(L, ss_truth.make_state(16, seed=L), 16, seed=100 + L)


@pytest.mark.slow
@pytest.mark.parametrize("L", [512, 1024])
def test_sixteen_blocks_against_fp64_full_size(L):
    _check(L, ss_truth.make_state(16, seed=L), 16, seed=100 + L, device=DEV)


@pytest.mark.parametrize("L", [17, 40])
def test_zero_padding_of_the_normalised_input(L):
    """Large LayerNorm betas: relu(LN(0)) = relu(beta) is far from 0, so padding the RAW input would move every border pixel."""
    _check(L, ss_truth.make_state(4, seed=7, beta_scale=5.0), 4, seed=9)


def test_two_runs_give_the_same_bits():
    atp, seq = _case(100, 3)
    model = _predictor(ss_truth.make_state(16, seed=3), 16)
    a = torch.from_numpy(atp).to(DEV)
    r1, r2 = model.predict(a, seq).cpu().numpy(), model.predict(a, seq).cpu().numpy()
    assert np.array_equal(r1.view(np.uint32), r2.view(np.uint32))


def test_forward_atp_on_the_device_equals_the_host_round_trip():
    from rnamsm.model import MSATransformer
    state = synthetic.make_state_dict(seed=0)
    msa = MSATransformer(num_layers=10)
    msa.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    msa = msa.eval().to(DEV)
    toks = torch.from_numpy(golden("tokens_2DRB_1_first64.npz")["tokens"][:32]).to(DEV)
    with torch.no_grad():
        atp = msa.forward_one(toks)["atp"]
    L = atp.shape[-1]
    letters = {4: "A", 5: "G", 6: "C", 7: "U"}
    seq = "".join(letters.get(int(t), "X") for t in toks[0, 1:].cpu())
    head = _predictor(ss_truth.make_state(16, seed=11), 16)
    dev = head.predict(atp, seq).cpu().numpy()
    host = head.predict(torch.from_numpy(atp.cpu().numpy()).to(DEV), seq).cpu().numpy()
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))
    # planes further apart than L*L (a slice of a wider buffer) are read in place, same bits
    wide = torch.full((120, L * L + 13), float("nan"), device=DEV)
    wide[:, :L * L] = atp.reshape(120, -1)
    view = wide[:, :L * L].view(120, L, L)
    assert view.stride() == (L * L + 13, L, 1)
    strided = head.predict(view, seq).cpu().numpy()
    assert np.array_equal(strided.view(np.uint32), dev.view(np.uint32))


def _ss_state_file(root, num_blocks=16, seed=5):
    path = root / "model" / "rna-msm_attention.pt"
    path.parent.mkdir(parents=True, exist_ok=True)
    torch.save({k: torch.from_numpy(v) for k, v in ss_truth.make_state(num_blocks, seed).items()}, path)
    return path


def _ss_predict(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "SS_predict.py")] + list(args), capture_output=True, text=True,
                          timeout=300)


def test_ss_predict_writes_the_three_files(tmp_path):
    feat = tmp_path / "feat"
    feat.mkdir()
    for f in ("2DRB_1.fasta", "2DRB_1_atp.npy"):
        shutil.copy(os.path.join(SS_DIR, f), feat / f)
    _ss_state_file(tmp_path)
    r = _ss_predict("--rootdir", str(tmp_path), "--featdir", str(feat), "--rnaid", "2DRB_1", "--device", "cuda")
    assert r.returncode == 0, r.stderr[-2000:]
    prob = np.loadtxt(feat / "SS_result" / "2DRB_1.prob", delimiter="\t")
    assert prob.shape == (35, 35) and ((prob > 0) & (prob < 1)).all()
    ct = (feat / "SS_result" / "2DRB_1.ct").read_text().split("\n")
    assert ct[0] == "35\t\t2DRB_1\t\tRNAMSM_SS output" and len((feat / "SS_result" / "2DRB_1.bpseq").read_text().split("\n")) == 37


@pytest.mark.parametrize("batching", [True, False])
def test_cli_key_writes_ss_results_equal_to_ss_predict(tmp_path, batching):
    sys.path.insert(0, ROOT)
    import RNA_MSM_Inference as cli
    state = synthetic.make_state_dict(seed=0)
    ckpt = tmp_path / "model.ckpt"
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in state.items()}}, ckpt)
    ss_pt = _ss_state_file(tmp_path)
    ids = ["2DRB_1", "2DRB_1b"]                        # two small alignments: one packed group when batching
    outs = {}
    for key in (False, True):
        res = tmp_path / ("with" if key else "without")
        res.mkdir()
        for i in ids:
            shutil.copy(os.path.join(GOLDEN, "2DRB_1_first64.a2m_msa2"), res / f"{i}.a2m_msa2")
        (tmp_path / "rna_id.txt").write_text("\n".join(ids) + "\n")
        cli.main([f"data.root_path={tmp_path}", f"data.MSA_path={res.name}", f"data.model_path={ckpt}", "data.MSA_list=rna_id.txt",
                  "data.max_seqs_per_msa=32", "data.sample_method=first", f"data.batch_small_msas={batching}"]
                 + ([f"data.ss_model_path={ss_pt}"] if key else []))
        outs[key] = res
    assert not (outs[False] / "SS_result").exists()
    for i in ids:                                      # the .npy files do not change with the key
        for kind in ("atp", "emb"):
            assert (outs[False] / f"{i}_{kind}.npy").read_bytes() == (outs[True] / f"{i}_{kind}.npy").read_bytes()
    toks = golden("tokens_2DRB_1_first64.npz")["tokens"]
    letters = {4: "A", 5: "G", 6: "C", 7: "U", 8: "X", 10: "-"}
    seq = "".join(letters[int(t)] for t in toks[0, 1:])
    for i in ids:
        for ext in ("ct", "bpseq", "prob"):
            assert (outs[True] / "SS_result" / f"{i}.{ext}").is_file()
        feat = tmp_path / f"feat_{i}"
        feat.mkdir()
        shutil.copy(outs[True] / f"{i}_atp.npy", feat / f"{i}_atp.npy")
        (feat / f"{i}.fasta").write_text(f">{i}\n{seq}\n")
        r = _ss_predict("--rootdir", str(tmp_path), "--featdir", str(feat), "--rnaid", i)
        assert r.returncode == 0, r.stderr[-2000:]
        for ext in ("prob", "bpseq", "ct"):
            assert (feat / "SS_result" / f"{i}.{ext}").read_bytes() == (outs[True] / "SS_result" / f"{i}.{ext}").read_bytes(), ext


def test_cli_key_pairs_every_alignment_with_its_own_maps_and_tokens(tmp_path):
    """Three alignments whose L and query differ pairwise (35, 12 with T, X and - in its query, 50 random): in the packed
    loop (one group) and the one-by-one loop, every SS_result file is what write_ss_files writes from SSPredictor.predict on
    that alignment's own _atp.npy and the letters of its own query tokens (a T of the alignment reads as U), so a swap of
    maps, tokens or ids between members fails."""
    sys.path.insert(0, ROOT)
    import RNA_MSM_Inference as cli
    from conftest import _LETTER
    state = synthetic.make_state_dict(seed=0)
    ckpt = tmp_path / "model.ckpt"
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in state.items()}}, ckpt)
    ss_pt = _ss_state_file(tmp_path)
    rng = np.random.RandomState(81)
    rand_rows = ["".join(rng.choice(list("ACGU"), 50)) for _ in range(6)]
    sources = {"rnaP": (open(os.path.join(GOLDEN, "2DRB_1_first64.a2m_msa2")).read(), "tokens_2DRB_1_first64.npz"),
               "rnaQ": (open(os.path.join(GOLDEN, "synthetic_chars.a2m_msa2")).read(), "tokens_synthetic_chars.npz"),
               "rnaR": ("".join(f">r{i}\n{row}\n" for i, row in enumerate(rand_rows)), None)}
    seqs = {i: ("".join(_LETTER[int(t)] for t in golden(tok)["tokens"][0, 1:]) if tok else rand_rows[0])
            for i, (_, tok) in sources.items()}
    assert [len(s) for s in seqs.values()] == [35, 12, 50] and seqs["rnaQ"] == "ACGU-XACGUUU"
    ids = list(sources)
    outs = {}
    for batching in (True, False):
        res = tmp_path / f"batch_{batching}"
        res.mkdir()
        for i, (text, _) in sources.items():
            (res / f"{i}.a2m_msa2").write_text(text)
        (tmp_path / "rna_id.txt").write_text("\n".join(ids) + "\n")
        cli.main([f"data.root_path={tmp_path}", f"data.MSA_path={res.name}", f"data.model_path={ckpt}", "data.MSA_list=rna_id.txt",
                  "data.max_seqs_per_msa=32", "data.sample_method=first", f"data.batch_small_msas={batching}",
                  f"data.ss_model_path={ss_pt}"])
        outs[batching] = res
    head = ss.load_predictor(ss_pt, DEV)
    for i in ids:
        atp = np.load(outs[False] / f"{i}_atp.npy")
        assert atp.shape == (120, len(seqs[i]), len(seqs[i]))
        want_dir = tmp_path / f"want_{i}"
        ss.write_ss_files(head.predict(torch.from_numpy(atp).to(DEV), seqs[i]).cpu().numpy(), seqs[i], i, want_dir)
        for ext in ("ct", "bpseq", "prob"):
            want = (want_dir / "SS_result" / f"{i}.{ext}").read_bytes()
            for batching, res in outs.items():
                assert (res / "SS_result" / f"{i}.{ext}").read_bytes() == want, (i, ext, batching)


def test_refusals(tmp_path):
    atp, seq = _case(20, 1)
    a = torch.from_numpy(atp).to(DEV)
    model = _predictor(ss_truth.make_state(2, seed=1), 2)
    with pytest.raises(ValueError, match="length 19"):
        model.predict(a, seq[:19])
    with pytest.raises(ValueError, match="exceeds"):
        model.predict(torch.zeros(120, 1025, 1025, device=DEV), "A" * 1025)
    # the C ABI itself: L > 1024, a null weight pointer, a short workspace -> RNAMSM_ERR_INVALID, nothing launched
    lib = _lib.load()
    ptrs, _ = model._packed_weights()
    codes = torch.zeros(2048, dtype=torch.uint8, device=DEV)
    out = torch.empty(64, device=DEV)
    ws = torch.empty(lib.rnamsm_ss_head_workspace_bytes(20), dtype=torch.uint8, device=DEV)
    assert lib.rnamsm_ss_head_workspace_bytes(1025) == 0
    s = torch.cuda.current_stream().cuda_stream
    assert lib.rnamsm_ss_head(a.data_ptr(), 1025 * 1025, codes.data_ptr(), 1025, 2, ptrs, None, out.data_ptr(), ws.data_ptr(),
                              ws.numel(), s) == -1
    assert lib.rnamsm_ss_head(a.data_ptr(), 400, codes.data_ptr(), 20, 2, ptrs, None, out.data_ptr(), ws.data_ptr(),
                              ws.numel() - 1, s) == -1
    assert lib.rnamsm_ss_head(a.data_ptr(), 399, codes.data_ptr(), 20, 2, ptrs, None, out.data_ptr(), ws.data_ptr(),
                              ws.numel(), s) == -1
    bad = (ctypes.c_void_p * len(ptrs))(*ptrs)
    bad[5] = None
    assert lib.rnamsm_ss_head(a.data_ptr(), 400, codes.data_ptr(), 20, 2, bad, None, out.data_ptr(), ws.data_ptr(), ws.numel(),
                              s) == -1
    assert b"weight pointer 5" in lib.rnamsm_last_error()
    # SS_predict.py: a sequence whose length is not the maps' L, weights of the wrong shape
    feat = tmp_path / "feat"
    feat.mkdir()
    shutil.copy(os.path.join(SS_DIR, "2DRB_1_atp.npy"), feat / "2DRB_1_atp.npy")
    (feat / "2DRB_1.fasta").write_text(">2DRB_1\nGGCCCGGGGCGG\n")
    _ss_state_file(tmp_path)
    r = _ss_predict("--rootdir", str(tmp_path), "--featdir", str(feat))
    assert r.returncode != 0 and "length 12" in r.stderr and "L = 35" in r.stderr
    shutil.copy(os.path.join(SS_DIR, "2DRB_1.fasta"), feat / "2DRB_1.fasta")
    _ss_state_file(tmp_path, num_blocks=3)
    r = _ss_predict("--rootdir", str(tmp_path), "--featdir", str(feat))
    assert r.returncode != 0 and "Missing key" in r.stderr
    assert not (feat / "SS_result").exists()
