"""Covariance contacts on the GPU (csrc/invcov.hip: rnamsm_msa_invcov through ops.msa_invcov and rnamsm.msa.msa_invcov; data.invcov).

Stage 1, the pair counts, is integer work and is held bit for bit to numpy's integer counts (tests/invcov_truth.pair_counts).  The
map is held to the fp64 truth (invcov_truth.invcov: np.cov + numpy's SVD norm, which tests/test_invcov_host.py ties to the
reference's own MSA.invcov).  Its bar is derived, not chosen: YARD = the largest elementwise distance between two fp64 restatements
on the CPU -- numpy's SVD norm and sqrt(eigvalsh(B^T B).max()) -- over the cases, relative to each map's largest entry; the device's
one-sided Jacobi is a third algorithm of the same conditioning and gets 4 x YARD.  Measured on the CPU: YARD = 1.12e-15 (the K = 16
case of 9 columns), so the bar is 4.47e-15 of the largest entry.  Measured on an MI355X: the device's largest distance is 3.17e-15
(that K = 16 case, on its diagonal) and 3.16e-15 on the deeper case, where the device's own formula evaluated in numpy with numpy's
SVD is 3.03e-15 from the truth (np.cov's rounding, not the Jacobi's).  Every test prints its figures before it asserts."""
import contextlib
import io

import numpy as np
import pytest
import torch

import invcov_truth as T
from rnamsm import _lib, msa, ops, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = sorted(T.cases())


@pytest.fixture(scope="module")
def yard():
    y = T.yardstick()
    print(f"yardstick (SVD norm vs sqrt(eigvalsh)) over {len(CASES)} cases: {y:.3e}; the device's bar: {4 * y:.3e}")
    assert 1e-16 < y < 1e-14                      # two fp64 algorithms: a few ulps, or the yardstick itself is broken
    return y


@pytest.fixture(scope="module")
def device_results():
    """name -> (map, counts, symbols) of every case, computed once."""
    out = {}
    for name, t in T.cases().items():
        m, c, s = ops.msa_invcov(torch.from_numpy(np.array(t)).to(DEV), T.GAP, want_counts=True)
        out[name] = (m.cpu().numpy(), c.cpu().numpy(), s.cpu().numpy())
    return out


def _check_map(name, got, t, yard):
    want = T.invcov(t)
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.isfinite(got).all(), name
    assert np.array_equal(got, got.T), name                               # exactly symmetric
    top = want.max()
    if top == 0:
        assert np.all(got == 0), name
        return 0.0
    eye = np.eye(len(want), dtype=bool)
    d_diag = float(np.abs(got - want)[eye].max() / top)
    d_off = float(np.abs(got - want)[~eye].max() / top) if len(want) > 1 else 0.0
    print(f"{name}: diagonal {d_diag:.3e}, off-diagonal {d_off:.3e} of the largest entry {top:.4f} (bar {4 * yard:.3e})")
    assert d_diag <= 4 * yard and d_off <= 4 * yard, name
    return max(d_diag, d_off)


@pytest.mark.parametrize("name", CASES)
def test_counts_equal_numpys_integer_counts(device_results, name):
    t = T.cases()[name]
    _, counts, syms = device_results[name]
    want = T.pair_counts(t)
    assert np.array_equal(syms, T.symbols(t).astype(np.int32))
    assert counts.dtype == np.int32 and counts.shape == want.shape
    assert np.array_equal(counts, want), name


@pytest.mark.parametrize("N", [65, 1023, 1024, 1025])
def test_counts_on_both_sides_of_a_step_of_sixteen_words(N):
    """The count kernel stages 16 words = 1024 alignment rows per step: one step short by a row, one step exactly, one step and a
    row; N = 65 is one word and a row.  rnamsm_msa_mi counts through the same launch."""
    t = T.random_alignment(np.random.RandomState(N), N, 5, 4, gaps=0.15)
    _, counts, syms = ops.msa_invcov(torch.from_numpy(t).to(DEV), T.GAP, want_counts=True)
    assert np.array_equal(syms.cpu().numpy(), T.symbols(t).astype(np.int32))
    assert np.array_equal(counts.cpu().numpy(), T.pair_counts(t))


@pytest.mark.parametrize("name", CASES)
def test_map_against_the_fp64_truth(device_results, yard, name):
    t = T.cases()[name]
    got = device_results[name][0]
    _check_map(name, got, t, yard)
    # without the counts (tiles below the diagonal are skipped then): the same bits
    again = ops.msa_invcov(torch.from_numpy(np.array(t)).to(DEV), T.GAP).cpu().numpy()
    assert again.tobytes() == got.tobytes(), name


def test_blocks_of_rank_zero_are_exactly_zero(device_results):
    got = device_results["N66_L19_K4_constant"][0]
    assert np.all(got[11] == 0) and np.all(got[:, 11] == 0) and got.max() > 0.1
    deg = device_results["N66_L19_K4_degenerate"][0]
    assert np.all(deg[3] == 0) and np.all(deg[:, 3] == 0)                 # the all-gap column
    for name in CASES:                                                    # K = 1 without gaps: every column constant
        if T.invcov(T.cases()[name]).max() == 0:
            assert np.all(device_results[name][0] == 0), name


def test_rows_with_a_leading_dimension_larger_than_l(device_results):
    for name in ("N129_L7_K4", "N70_L13_K5", "N70_L65_K1"):
        t = T.cases()[name]
        N, L = t.shape
        wide = torch.full((N, L + 13), 77, dtype=torch.uint8, device=DEV)      # 77: a value the view must never show
        wide[:, 5:5 + L] = torch.from_numpy(np.array(t)).to(DEV)
        view = wide[:, 5:5 + L]
        assert view.stride(0) == L + 13
        m, c, s = ops.msa_invcov(view, T.GAP, want_counts=True)
        assert np.array_equal(c.cpu().numpy(), device_results[name][1]) and np.array_equal(s.cpu().numpy(), device_results[name][2])
        assert m.cpu().numpy().tobytes() == device_results[name][0].tobytes()


def test_one_deeper_alignment(yard):
    """N = 5000, L = 33 from a seeded two-state mixture: counts exact, the map within the same bar, two runs bit-identical."""
    t = T.mixture_alignment()
    dev_t = torch.from_numpy(t).to(DEV)
    m, c, _ = ops.msa_invcov(dev_t, T.GAP, want_counts=True)
    assert np.array_equal(c.cpu().numpy(), T.pair_counts(t))
    got = m.cpu().numpy()
    _check_map("mixture N5000 L33", got, t, yard)
    off = got[~np.eye(33, dtype=bool)]
    assert off.max() > 5 * np.median(off)                                  # some column pairs do co-vary
    m2, c2, _ = ops.msa_invcov(dev_t, T.GAP, want_counts=True)
    assert m2.cpu().numpy().tobytes() == got.tobytes() and torch.equal(c, c2)
    assert ops.msa_invcov(dev_t, T.GAP).cpu().numpy().tobytes() == got.tobytes()


def test_counts_made_in_two_bands_give_the_bits_of_one(yard):
    """Without the caller's counts buffer the counts of L * L * K * K * 4 > 256 MB are made a band of columns at a time (a multiple of
    64 columns: here 1984 + 116 at L = 2100, K = 4); with it, in one piece.  The same map either way, and sampled blocks agree with
    the truth of their two columns."""
    rng = np.random.RandomState(9)
    N, L = 3, 2100
    t = T.random_alignment(rng, N, L, 4, gaps=0.1)
    assert L * L * 16 * 4 > 1 << 28
    dev_t = torch.from_numpy(t).to(DEV)
    banded = ops.msa_invcov(dev_t, T.GAP).cpu().numpy()
    whole, counts, syms = ops.msa_invcov(dev_t, T.GAP, want_counts=True)
    assert whole.cpu().numpy().tobytes() == banded.tobytes()
    assert np.array_equal(banded, banded.T) and np.isfinite(banded).all()
    vals = T.symbols(t)
    assert np.array_equal(syms.cpu().numpy(), vals)
    worst = 0.0
    for i, j in [(0, 0), (0, 2099), (1983, 1984), (1984, 1984), (2099, 2099), (1983, 5), (2050, 1990)] + [
            tuple(p) for p in rng.randint(0, L, size=(40, 2))]:
        pair = t[:, [i, j]]
        onehot = (pair[:, :, None] == vals[None, None, :]).astype(np.int64)
        assert np.array_equal(counts[i, j].cpu().numpy(), onehot[:, 0].T @ onehot[:, 1]), (i, j)
        c = np.cov(onehot.reshape(N, 8).T.astype(np.float64)).reshape(2, 4, 2, 4)[0, :, 1, :]
        worst = max(worst, abs(banded[i, j] - np.linalg.norm(c, ord=2)))
    print(f"two bands, 47 sampled blocks: max abs {worst:.3e} (bar {4 * yard:.3e} of the largest entry {banded.max():.4f})")
    assert worst <= 4 * yard * banded.max()


def test_refusals_that_need_the_device():
    rng = np.random.RandomState(3)
    many = torch.from_numpy(rng.randint(20, 37, size=(40, 6)).astype(np.uint8)).to(DEV)      # 17 distinct values
    many[:17, 0] = torch.arange(20, 37, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.RnamsmError, match="msa_invcov: 17 distinct non-gap values, more than 16"):
        ops.msa_invcov(many, T.GAP)
    with pytest.raises(_lib.RnamsmError, match="17 distinct"):
        ops.msa_invcov(many, T.GAP, want_counts=True)
    m = ops.msa_invcov(many, 36)                                           # one of the 17 is the gap: 16 symbols, accepted
    assert np.isfinite(m.cpu().numpy()).all()
    gaps = torch.full((5, 4), T.GAP, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.RnamsmError, match=r"nothing but the gap value 10 \(K = 0\)"):
        ops.msa_invcov(gaps, T.GAP)
    with pytest.raises(_lib.RnamsmError, match=r"N=1 outside \[2, 1048576\]"):
        ops.msa_invcov(gaps[:1], T.GAP)
    with pytest.raises(_lib.RnamsmError, match=r"L=4097 outside \[1, 4096\]"):
        ops.msa_invcov(torch.zeros((2, 4097), dtype=torch.uint8, device=DEV), T.GAP)


def test_msa_invcov_drops_cls(device_results):
    t = T.cases()["N70_L17_K4"]
    with_cls = np.concatenate([np.zeros((70, 1), dtype=np.int64), t.astype(np.int64)], 1)
    got = msa.msa_invcov(with_cls, T.GAP, DEV)
    assert got.dtype == np.float64 and got.tobytes() == device_results["N70_L17_K4"][0].tobytes()


# ---- the CLI key ------------------------------------------------------------------------------------------------------------
MAX_SEQLEN = 33
SHAPES = {"rnaLong": (5, 70), "rnaA": (3, 20), "rnaB": (9, 32), "rnaOne": (1, 12)}


@pytest.fixture(scope="module")
def model():
    from rnamsm.model import MSATransformer
    state = synthetic.make_state_dict(seed=0, max_seqlen=MAX_SEQLEN)
    m = MSATransformer(num_layers=10, max_seqlen=MAX_SEQLEN)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV)


def _run(model, root, overrides):
    """-> (files, printed with the run's own directory taken out)"""
    from rnamsm.config import Config, parse_overrides
    from rnamsm.inference import extract_feat
    rng = np.random.RandomState(11)
    (root / "results").mkdir(parents=True)
    for i, (depth, length) in SHAPES.items():
        text = "".join(f">s{r}\n{''.join(rng.choice(list('ACGU-'), length, p=[.23, .23, .22, .22, .1]))}\n" for r in range(depth))
        (root / "results" / f"{i}.a2m_msa2").write_text(text)
    (root / "rna_id.txt").write_text("\n".join(SHAPES) + "\n")
    cfg = Config()
    cfg.data.root_path, cfg.data.MSA_path, cfg.data.MSA_list = str(root), "results", "rna_id.txt"
    cfg.data.sample_method, cfg.data.max_seqs_per_msa = "first", 4            # rnaB and rnaLong lose rows to the sub-sampling
    cfg = parse_overrides([f"data.max_seqlen={MAX_SEQLEN}"] + list(overrides), cfg)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        assert extract_feat(cfg, model=model) == sorted(SHAPES)
    files = {str(f.relative_to(root / "results")): f.read_bytes() for f in sorted((root / "results").rglob("*"))
             if f.is_file() and f.suffix != ".a2m_msa2"}
    return files, printed.getvalue().replace(str(root), "<root>")


@pytest.fixture(scope="module")
def runs(model, tmp_path_factory):
    root = tmp_path_factory.mktemp("invcov_cli")
    return root, {name: _run(model, root / name, keys) for name, keys in (
        ("windows", ["data.long_msa=windows", "data.invcov=true"]), ("crop", ["data.invcov=true"]),
        ("absent", []), ("false", ["data.invcov=false"]))}


def _tokens_of(path):
    from rnamsm.alphabet import RNAAlphabet
    from rnamsm.msa import load_msa_tokens
    return load_msa_tokens(path, RNAAlphabet(), None, "first")


@pytest.mark.parametrize("mode", ["windows", "crop"])
def test_cli_writes_the_map_of_the_alignment_as_read(runs, mode):
    root, by = runs
    files, printed = by[mode]
    for i, (depth, length) in SHAPES.items():
        if i == "rnaOne":
            continue
        got = np.load(root / mode / "results" / f"{i}_invcov.npy")
        assert got.shape == (length, length) and got.dtype == np.float64, i          # the full width, whatever max_seqlen says
        tokens = _tokens_of(root / mode / "results" / f"{i}.a2m_msa2")
        assert tokens.shape == (depth, length + 1)                                   # every row, before the sub-sampling to 4
        assert got.tobytes() == msa.msa_invcov(tokens, T.GAP, DEV).tobytes(), i
    # the alignment of one row is refused with one line that names the reason; its other files are written
    assert "rnaOne_invcov.npy" not in files and "rnaOne_emb.npy" in files and "rnaOne_atp.npy" in files
    lines = [ln for ln in printed.splitlines() if "rnaOne" in ln and "data.invcov" in ln]
    assert len(lines) == 1 and "N=1 outside [2, 1048576]" in lines[0], printed
    emb = np.load(root / mode / "results" / "rnaLong_emb.npy")
    assert emb.shape[0] == (70 if mode == "windows" else MAX_SEQLEN - 1)


def test_cli_with_the_key_off_is_what_it_was(runs):
    _, by = runs
    assert by["absent"] == by["false"]                                               # the file set, every byte, and stdout
    files, printed = by["absent"]
    assert not any("invcov" in f for f in files) and "invcov" not in printed
    on = by["crop"][0]
    assert {f: d for f, d in on.items() if "invcov" not in f} == files               # the key adds files and changes none
    assert sorted(set(on) - set(files)) == ["rnaA_invcov.npy", "rnaB_invcov.npy", "rnaLong_invcov.npy"]
