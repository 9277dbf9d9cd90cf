"""Alignment statistics on the GPU (csrc/msa_pdist.hip: rnamsm_msa_pdist, rnamsm_msa_neff, rnamsm_msa_coverage through rnamsm.ops and
rnamsm.msa).  Counts, distances, neighbour counts, weights and coverage are exact quantities -- integer counts and one IEEE division
-- so every comparison is of bits: against the numpy restatement (tests/msa_stats_truth.py), scipy, the existing one-block-per-row
kernel (ops.msa_weights) and the reference's own MSA class (tests/golden/msa_stats_reference_2drb64.npz).  Neff alone is a float64
sum in the device's own order; its bar is N * 2^-53 * fsum(weights), the worst case of ANY order of N - 1 additions of positive
terms (each addition rounds by at most 2^-53 of a partial sum, and no partial sum exceeds the total) -- derived, not measured; the
observed distance is printed."""
import math

import numpy as np
import pytest
import torch

import msa_stats_truth as T
from conftest import golden
from rnamsm import _lib, msa, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def cases():
    """(N, L) -> (alignment, truth counts, device dist, device counts), computed once."""
    out = {}
    for n, (N, L) in enumerate(T.SHAPES):
        a = T.alignment(N, L, 100 + n)
        d, c = ops.msa_pdist(dev(a), "both")
        out[(N, L)] = (a, T.counts(a), d.cpu().numpy(), c.cpu().numpy())
    return out


@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: f"N{s[0]}_L{s[1]}")
def test_counts_and_distances_equal_the_restatement(cases, shape):
    a, want, d, c = cases[shape]
    assert c.dtype == np.int32 and d.dtype == np.float64 and c.shape == d.shape == (shape[0], shape[0])
    assert np.array_equal(c, want)
    assert np.array_equal(d, want / np.float64(shape[1]))
    assert np.array_equal(d, d.T) and np.array_equal(c, c.T) and not d.diagonal().any() and not c.diagonal().any()


@pytest.mark.parametrize("shape", [(2, 7), (65, 64), (129, 513), (200, 9)], ids=lambda s: f"N{s[0]}_L{s[1]}")
def test_distances_equal_scipy(cases, shape):
    sp = pytest.importorskip("scipy.spatial.distance")
    a, _, d, _ = cases[shape]
    assert np.array_equal(d, sp.squareform(sp.pdist(a, "hamming")))


@pytest.mark.parametrize("want", ["dist", "counts"])
def test_one_output_alone(cases, want):
    a, truth, d, c = cases[(129, 7)]
    got = ops.msa_pdist(dev(a), want).cpu().numpy()
    assert np.array_equal(got, d if want == "dist" else c)


@pytest.mark.parametrize("shape,ld", [((65, 9), 16), ((129, 63), 64), ((64, 64), 71), ((3, 1), 5)])
def test_bytes_past_L_are_not_data(shape, ld):
    """Rows inside a wider buffer whose guard bytes differ from row to row: read as data they would change every count."""
    N, L = shape
    a = T.alignment(N, L, 7)
    rng = np.random.RandomState(8)
    wide = rng.randint(0, 256, size=(N, ld)).astype(np.uint8)
    wide[:, :L] = a
    view = dev(wide)[:, :L]
    assert view.stride(0) == ld
    want = T.counts(a)
    assert not np.array_equal(T.counts(wide), want)
    d, c = ops.msa_pdist(view, "both")
    assert np.array_equal(c.cpu().numpy(), want) and np.array_equal(d.cpu().numpy(), want / np.float64(L))
    rec = ops.msa_neff(view, 0.3)
    assert np.array_equal(rec.n_neighbors.cpu().numpy(), T.n_neighbors(a, 0.3))
    assert np.array_equal(ops.msa_coverage(view, T.GAP).cpu().numpy(), T.coverage(a))


def test_byte_values_that_break_a_swar_mask():
    """Rows over {0x00, 0x01, 0x7f, 0x80, 0xff}: every ordered pair of the five meets in some column of some pair of rows."""
    vals = np.array([0x00, 0x01, 0x7F, 0x80, 0xFF], dtype=np.uint8)
    a = vals[np.random.RandomState(3).randint(0, 5, size=(40, 67))]
    met = {(int(p), int(q)) for i in range(40) for p, q in zip(a[i], a[(i + 1) % 40])}
    assert len(met) == 25
    c = ops.msa_pdist(dev(a), "counts").cpu().numpy()
    assert np.array_equal(c, T.counts(a))
    # each single pair of values, alone in a row of one column and as a whole row of nine
    for L in (1, 9):
        b = np.repeat(vals[:, None], L, axis=1)
        d = ops.msa_pdist(dev(b), "dist").cpu().numpy()
        assert np.array_equal(d, 1.0 - np.eye(5)), L


def test_forty_distinct_values():
    rng = np.random.RandomState(4)
    vals = rng.choice(256, size=40, replace=False).astype(np.uint8)
    a = vals[rng.randint(0, 40, size=(70, 33))]
    assert len(np.unique(a)) == 40
    d, c = ops.msa_pdist(dev(a), "both")
    assert np.array_equal(c.cpu().numpy(), T.counts(a)) and np.array_equal(d.cpu().numpy(), T.dist(a))
    assert np.array_equal(ops.msa_neff(dev(a), 0.95).weights.cpu().numpy(), T.weights(a, 0.95))


def test_identical_rows_give_zero_and_rows_that_differ_everywhere_give_one():
    a = T.alignment(66, 37, 5)
    a[65] = a[0]                                   # across a tile seam
    a[64] = np.where(a[0] == 4, 5, 4)              # differs from row 0 (and from row 65) in every column
    d = ops.msa_pdist(dev(a), "dist").cpu().numpy()
    assert d[0, 65] == 0.0 and d[65, 0] == 0.0 and d[0, 64] == 1.0 and d[64, 65] == 1.0 and d[65, 64] == 1.0


# ---- neighbours, weights, Neff ------------------------------------------------------------------------------------------------
NEFF_SHAPES = [(1, 64), (2, 7), (63, 65), (64, 9), (65, 1), (65, 7), (65, 63), (65, 64), (65, 65), (129, 513), (200, 63), (200, 65)]


def _cutoffs(a):
    d = T.dist(a)
    off = d[~np.eye(len(a), dtype=bool)]
    occurring = float(np.sort(off)[len(off) // 2]) if off.size else 0.5      # the comparison is strict: a value that occurs
    return [0.0, 0.2, 1.0, occurring]


def _neff_bar(w):
    total = math.fsum(w)
    return total, len(w) * 2.0 ** -53 * total


@pytest.mark.parametrize("shape", NEFF_SHAPES, ids=lambda s: f"N{s[0]}_L{s[1]}")
def test_neighbours_and_weights_equal_the_restatement_and_the_existing_kernel(shape):
    a = T.alignment(*shape, seed=31)
    for cutoff in _cutoffs(a):
        rec = ops.msa_neff(dev(a), cutoff)
        n, w, neff = rec.n_neighbors.cpu().numpy(), rec.weights.cpu().numpy(), float(rec.neff.item())
        assert n.dtype == np.int32 and w.dtype == np.float64
        assert np.array_equal(n, T.n_neighbors(a, cutoff)), cutoff
        assert np.array_equal(w, T.weights(a, cutoff)), cutoff
        assert np.array_equal(w, ops.msa_weights(dev(a), cutoff).cpu().numpy()), cutoff
        if cutoff == 0.0:
            assert (n == 0).all() and np.isinf(w).all() and neff == math.inf      # the strict comparison admits not even the row itself
            continue
        total, bar = _neff_bar(w)
        print(f"N={shape[0]} L={shape[1]} cutoff={cutoff:.6f}: neff {neff!r}, fsum {total!r}, distance {abs(neff - total):.3e}, bar {bar:.3e}")
        assert abs(neff - total) <= bar


@pytest.mark.parametrize("shape", [(200, 65), (129, 513), (65, 1)], ids=lambda s: f"N{s[0]}_L{s[1]}")
def test_every_workspace_size_gives_the_same_bits(shape):
    """At the minimum the partial table holds one row block: N = 200 runs in four bands, and in two at a size in between."""
    N, L = shape
    a = T.alignment(N, L, 32)
    lib = _lib.load()
    least, default = lib.rnamsm_msa_neff_min_workspace_bytes(N, L), lib.rnamsm_msa_neff_workspace_bytes(N, L)
    blocks = -(-N // 64)
    assert 0 < least < default and (default - least) % (blocks - 1) == 0       # one slab of the table per further row block
    slab = (default - least) // (blocks - 1)
    for cutoff in (0.2, 0.5):
        ref = ops.msa_neff(dev(a), cutoff)
        for size in (least, least + slab, least + slab + 1, default + 4096):
            got = ops.msa_neff(dev(a), cutoff, workspace_bytes=size)
            assert torch.equal(got.n_neighbors, ref.n_neighbors) and torch.equal(got.weights, ref.weights), (cutoff, size)
            assert got.neff.cpu().numpy().tobytes() == ref.neff.cpu().numpy().tobytes(), (cutoff, size)
        assert np.array_equal(ref.n_neighbors.cpu().numpy(), T.n_neighbors(a, cutoff))


def test_one_output_of_neff_alone():
    a = T.alignment(70, 20, 33)
    lib = _lib.load()
    u8 = dev(a)
    ws = torch.empty(lib.rnamsm_msa_neff_workspace_bytes(70, 20), dtype=torch.uint8, device=DEV)
    neff = torch.full((), -1.0, dtype=torch.float64, device=DEV)
    _lib.check(lib.rnamsm_msa_neff(u8.data_ptr(), 70, 20, 20, 0.2, None, None, neff.data_ptr(), ws.data_ptr(), ws.numel(), None))
    torch.cuda.synchronize()
    assert neff.cpu().numpy().tobytes() == ops.msa_neff(u8, 0.2).neff.cpu().numpy().tobytes()


# ---- coverage -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 9), (2, 64), (17, 65), (200, 130), (1000, 3)], ids=lambda s: f"N{s[0]}_L{s[1]}")
def test_coverage_equals_the_restatement(shape):
    a = T.alignment(*shape, seed=41)
    a[:, shape[1] // 2] = T.GAP                                    # an all-gap column: exactly 0
    got = ops.msa_coverage(dev(a), T.GAP).cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got, T.coverage(a)) and got[shape[1] // 2] == 0.0
    assert np.array_equal(ops.msa_coverage(dev(a), 255).cpu().numpy(), np.ones(shape[1]))      # a gap value that does not occur


# ---- the reference's own values ---------------------------------------------------------------------------------------------------
def test_the_references_own_values_on_the_shipped_excerpt():
    g = golden("msa_stats_reference_2drb64.npz")
    tokens = golden("tokens_2DRB_1_first64.npz")["tokens"]
    assert tokens.shape == (64, g["coverage"].shape[0] + 1)
    L = tokens.shape[1] - 1
    assert np.array_equal(msa.msa_pdist(tokens, DEV), g["pdist"])
    rec = ops.msa_neff(dev(tokens[:, 1:].astype(np.uint8)), float(g["seqid_cutoff"]))
    assert np.array_equal(rec.weights.cpu().numpy(), g["weights"])
    assert np.array_equal(msa.msa_coverage(tokens, T.GAP, DEV), g["coverage"])
    neff = msa.msa_neff(tokens, float(g["seqid_cutoff"]), "none", DEV)
    total, bar = _neff_bar(g["weights"])
    print(f"neff {neff!r}, the reference's {float(g['neff_none'])!r}, fsum {total!r}, bar {bar:.3e}")
    assert neff == float(rec.neff.item()) and abs(neff - total) <= bar and abs(neff - float(g["neff_none"])) <= bar
    # the normalisations are one host division of that sum each
    assert msa.msa_neff(tokens, 0.2, "sqrt", DEV) == neff / math.sqrt(L) and msa.msa_neff(tokens, 0.2, "seqlen", DEV) == neff / L
    assert msa.msa_neff(tokens, 0.2, 3.0, DEV) == neff / 3.0
    assert abs(msa.msa_neff(tokens, 0.2, "sqrt", DEV) - float(g["neff_sqrt"])) <= bar
    assert abs(msa.msa_neff(tokens, 0.2, "seqlen", DEV) - float(g["neff_seqlen"])) <= bar
    with pytest.raises(ValueError, match="normalization="):
        msa.msa_neff(tokens, 0.2, "mean", DEV)


# ---- refusals: before the first launch, the outputs untouched -------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    N, L = 70, 20
    lib = _lib.load()
    u8 = dev(T.alignment(N, L, 51))
    big = torch.empty(max(lib.rnamsm_msa_neff_workspace_bytes(N, L), lib.rnamsm_msa_pdist_workspace_bytes(N, L)), dtype=torch.uint8, device=DEV)
    counts = torch.full((N, N), -7, dtype=torch.int32, device=DEV)
    dist = torch.full((N, N), -7.0, dtype=torch.float64, device=DEV)
    nn = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    w = torch.full((N,), -7.0, dtype=torch.float64, device=DEV)
    neff = torch.full((), -7.0, dtype=torch.float64, device=DEV)
    cov = torch.full((L,), -7.0, dtype=torch.float64, device=DEV)
    p_need, n_least = lib.rnamsm_msa_pdist_workspace_bytes(N, L), lib.rnamsm_msa_neff_min_workspace_bytes(N, L)

    def pdist(**kw):
        a = dict(N=N, L=L, ld=L, counts=counts.data_ptr(), dist=dist.data_ptr(), wsb=p_need)
        a.update(kw)
        rc = lib.rnamsm_msa_pdist(u8.data_ptr(), a["N"], a["L"], a["ld"], a["counts"], a["dist"], big.data_ptr(), a["wsb"], None)
        return rc, lib.rnamsm_last_error().decode()

    def neff_call(**kw):
        a = dict(N=N, L=L, ld=L, cutoff=0.2, nn=nn.data_ptr(), w=w.data_ptr(), neff=neff.data_ptr(), wsb=n_least)
        a.update(kw)
        rc = lib.rnamsm_msa_neff(u8.data_ptr(), a["N"], a["L"], a["ld"], a["cutoff"], a["nn"], a["w"], a["neff"], big.data_ptr(), a["wsb"], None)
        return rc, lib.rnamsm_last_error().decode()

    def coverage(**kw):
        a = dict(N=N, L=L, ld=L, gap=10)
        a.update(kw)
        return lib.rnamsm_msa_coverage(u8.data_ptr(), a["N"], a["L"], a["ld"], a["gap"], cov.data_ptr(), None), lib.rnamsm_last_error().decode()

    for call, kw, text in (
            (pdist, dict(N=0), "msa_pdist: N=0 outside [1, 16384]"),
            (pdist, dict(N=16385), "msa_pdist: N=16385 outside [1, 16384]"),
            (pdist, dict(L=0), "msa_pdist: L=0 outside [1, 32768]"),
            (pdist, dict(L=32769, ld=32769), "msa_pdist: L=32769 outside [1, 32768]"),
            (pdist, dict(ld=L - 1), "msa_pdist: ld=19 is smaller than L=20"),
            (pdist, dict(counts=None, dist=None), "msa_pdist: counts and dist are both null"),
            (pdist, dict(wsb=p_need - 1), f"msa_pdist: workspace of {p_need - 1} bytes too small"),
            (neff_call, dict(N=0), "msa_neff: N=0 outside [1, 1048576]"),
            (neff_call, dict(N=(1 << 20) + 1), "msa_neff: N=1048577 outside [1, 1048576]"),
            (neff_call, dict(L=0), "msa_neff: L=0 outside [1, 32768]"),
            (neff_call, dict(L=32769, ld=32769), "msa_neff: L=32769 outside [1, 32768]"),
            (neff_call, dict(ld=L - 1), "msa_neff: ld=19 is smaller than L=20"),
            (neff_call, dict(cutoff=-0.125), "msa_neff: seqid_cutoff=-0.125 outside [0, 1]"),
            (neff_call, dict(cutoff=1.5), "msa_neff: seqid_cutoff=1.5 outside [0, 1]"),
            (neff_call, dict(cutoff=math.nan), "outside [0, 1]"),
            (neff_call, dict(nn=None, w=None, neff=None), "msa_neff: n_neighbors, weights and neff are all null"),
            (neff_call, dict(wsb=n_least - 1), f"msa_neff: workspace of {n_least - 1} bytes too small"),
            (coverage, dict(N=0), "msa_coverage: N=0 outside [1, 1048576]"),
            (coverage, dict(L=0), "msa_coverage: L=0 outside [1, 32768]"),
            (coverage, dict(L=32769, ld=32769), "msa_coverage: L=32769 outside [1, 32768]"),
            (coverage, dict(ld=L - 1), "msa_coverage: ld=19 is smaller than L=20"),
            (coverage, dict(gap=256), "msa_coverage: gap=256 is not a byte value")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    for t in (counts, nn):
        assert bool((t == -7).all())
    for t in (dist, w, neff, cov):
        assert bool((t == -7.0).all())
    # and the same calls with nothing wrong write all of them
    for call in (pdist, neff_call, coverage):
        assert call()[0] == 0
    torch.cuda.synchronize()
    assert not bool((counts == -7).any()) and not bool((dist == -7.0).any()) and not bool((nn == -7).any())
    assert not bool((w == -7.0).any()) and float(neff.item()) > 0 and not bool((cov == -7.0).any())


def test_a_device_that_is_no_hip_device_is_refused():
    tokens = np.full((3, 5), 4, dtype=np.int64)
    for fn, args in ((msa.msa_pdist, (tokens, "cpu")), (msa.msa_coverage, (tokens, 10, "cpu")), (msa.msa_pdist, (tokens, None))):
        with pytest.raises(_lib.RnamsmError, match="not a HIP device"):
            fn(*args)
    with pytest.raises(_lib.RnamsmError, match="not a HIP device"):
        msa.msa_neff(tokens, 0.2, "none", "cpu")
