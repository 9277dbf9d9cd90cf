"""rnamsm_seqid_filter on the device against the plain-loop restatement (tests/seqid_filter_truth.py): the kept indices and kept_at,
exact integer comparisons throughout.  Shapes on every side of the 64-row tile and the 8-byte word; chains A - B - C (B redundant to
A, C to B, C not to A: A and C are kept) inside a chunk, across a chunk boundary and across the 64-row seam of the walk over the kept
rows; exact equality of 100 * same and t * both and one match fewer; pairs without a common column; all-gap rows; byte values 0 and
255 as symbol and as gap; padded rows; the order argument and its refusal; the passes; the chunk parameter; two runs; the 1176-row
2DRB_1 alignment."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden
from rnamsm import _lib, ops
import seqid_filter_truth as T

pytestmark = pytest.mark.gpu
GAP = 10
DEV = "cuda:0"


def device(a, gap, num_seqs, *args, order=None, ld=None):
    """ops.seqid_filter on alignment a (numpy uint8 [N, L]); ld: the rows inside a wider buffer of random bytes."""
    N, L = a.shape
    if ld is None:
        u8 = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    else:
        wide = np.random.RandomState(N * 1000 + L).randint(0, 256, size=(N, ld)).astype(np.uint8)
        wide[:, :L] = a
        u8 = torch.from_numpy(wide).to(DEV)[:, :L]
        assert u8.stride(0) == ld
    if order is not None:
        order = torch.from_numpy(np.asarray(order, dtype=np.int32)).to(DEV)
    rec = ops.seqid_filter(u8, gap, num_seqs, *args, order=order)
    assert rec.indices.dtype == torch.int32 and rec.kept_at.dtype == torch.int32 and rec.kept_at.shape == (N,)
    return rec.indices.cpu().numpy().astype(np.int64), rec.kept_at.cpu().numpy()


def same_as_truth(a, gap, num_seqs, *args, order=None, ld=None, memo=None):
    ti, tat, passes = T.seqid_filter(a, gap, num_seqs, *args, order=order, memo=memo)
    di, dat = device(a, gap, num_seqs, *args, order=order, ld=ld)
    assert np.array_equal(di, ti), (a.shape, num_seqs, args, di[:10], ti[:10])
    assert np.array_equal(dat, tat), (a.shape, num_seqs, args)
    return ti, tat, passes


@pytest.fixture
def chunk():
    """Sets "seqid_filter_chunk"; the default comes back afterwards."""
    default = ops.get_param("seqid_filter_chunk")
    assert default == 256
    try:
        yield lambda v: ops.set_param("seqid_filter_chunk", v)
    finally:
        ops.set_param("seqid_filter_chunk", default)


SCHEDULE = (35, 95, 15)            # passes at 35, 50, 65, 80, 95: four symbols agree in a quarter of the columns by chance


def planted(N, L, seed):
    """Four symbols plus gaps, near copies at every distance: something is rejected and something kept in every pass where the shape
    has room for that (every ninth row is an exact copy of an earlier one, so the last pass rejects something too)."""
    a = T.alignment(N, L, seed, p_mut=0.4)
    for i in range(8, N, 9):
        a[i] = a[i - 3]
    return a


@pytest.mark.parametrize("L", [1, 7, 8, 9, 63, 64, 65, 100])
@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 130, 257])
def test_shapes(N, L):
    a = planted(N, L, 7 * N + L)
    memo = {}
    _, _, passes = same_as_truth(a, GAP, N, *SCHEDULE, memo=memo)              # num_seqs = N: every pass, unless nothing is rejected
    if N >= 63 and L >= 64:
        counts = [n for _, n in passes]
        assert len(counts) == 5 and all(x < y for x, y in zip(counts, counts[1:])) and counts[0] > 1 and counts[-1] < N, passes
    same_as_truth(a, GAP, 0, memo=memo)
    same_as_truth(a, GAP, max(1, N // 4), memo=memo)


@pytest.mark.parametrize("L", [1, 7, 63, 64, 65])
def test_the_second_pass_gathers_a_second_block_of_kept_rows(L):
    """130 rows: 100 mutually dissimilar ones (120 symbols; at L = 1 a hundred different bytes), then 30 copies of rows 5, 8, .., 92,
    every second copy with a seventh of its columns changed where L > 1.  The pass at 50 keeps the hundred; the pass at 90 then
    gathers them as a block of 64 and a block of 36 padded to 64, and keeps the changed copies only."""
    rng = np.random.RandomState(900 + L)
    a = np.empty((130, L), dtype=np.uint8)
    a[:100] = 20 + (rng.permutation(120)[:100, None] if L == 1 else rng.randint(0, 120, size=(100, L)))
    for k in range(30):
        a[100 + k] = a[5 + 3 * k]
        if k % 2 and L > 1:
            a[100 + k, :(L + 6) // 7] = 200 + k
    kept, at, passes = same_as_truth(a, 255, 130, 50, 90, 40)      # (no row has a gap: the default order is the rows as given)
    assert [t for t, _ in passes] == [50, 90] and 64 < passes[0][1] < 128 and 64 < len(kept) < 128, passes
    assert passes[0][1] == 100 and len(kept) == (100 if L == 1 else 115)


def chains(N, places, L=16, t=75):
    """N rows of L columns, no gaps, so the default order is the rows as given.  Fillers draw from 16 symbols of their own (two of
    them agree in 12 of 16 columns practically never: every filler is kept); chain k stands at places[k] = (pa, pb, pc) over four
    symbols of its own: B = A with 4 columns changed (12 / 16: exactly t = 75), C = B with 4 other columns changed (12 / 16 to B,
    8 / 16 to A)."""
    rng = np.random.RandomState(N + len(places))
    a = rng.randint(100, 116, size=(N, L)).astype(np.uint8)
    for k, (pa, pb, pc) in enumerate(places):
        s = 20 + 8 * k
        A = rng.randint(s, s + 4, size=L).astype(np.uint8)
        B = A.copy()
        B[:4] = s + 4
        C = B.copy()
        C[4:8] = s + 5
        a[pa], a[pb], a[pc] = A, B, C
    return a


@pytest.mark.parametrize("size", [64, 128, 256])
@pytest.mark.parametrize("name, places", [
    ("inside one tile of one chunk", [(10, 20, 30)]),
    ("inside one chunk of 256, over its tiles", [(10, 70, 130)]),
    ("across the chunk boundaries", [(60, 62, 66), (61, 130, 140), (126, 127, 128), (250, 255, 256)]),
    ("A at the seam of the walk over the kept rows", [(63, 200, 210), (64, 201, 211), (127, 202, 212), (128, 203, 213)])])
def test_chains_keep_the_ends_and_drop_the_middle(chunk, size, name, places):
    chunk(size)
    a = chains(257, places)
    kept, at, _ = same_as_truth(a, 255, 0, 20, 75, 5)
    for pa, pb, pc in places:
        assert pa in kept and pc in kept and pb not in kept, (name, size, pa, pb, pc)
    assert len(kept) == 257 - len(places)                 # every filler is kept: the kept list's index of a filler is its position
    kept76, _, _ = same_as_truth(a, 255, 0, 20, 76, 5)     # one point higher and B is no longer redundant to A
    assert len(kept76) == 257


def test_exact_equality_is_redundant_and_one_match_fewer_is_not():
    L = 30
    A = np.full(L, 4, dtype=np.uint8)
    A[20:] = GAP                                           # both = 20 against every row below
    B = A.copy(); B[:2] = 5                                # 18 of 20: 100 * 18 == 90 * 20
    C = A.copy(); C[2:5] = 6                               # 17 of 20 against A, 15 of 20 against B
    D = A.copy(); D[5:7] = 7; D[25:] = 5                   # 18 of 20 against A over the common columns; its own residues beyond count nothing
    a = np.stack([A, B, C, D])
    kept, at, _ = same_as_truth(a, GAP, 0, 20, 90, 5, order=[0, 1, 2, 3])
    assert list(kept) == [0, 2] and list(at) == [90, -1, 90, -1]
    kept, _, _ = same_as_truth(a, GAP, 0, 20, 91, 5, order=[0, 1, 2, 3])
    assert list(kept) == [0, 1, 2, 3]
    # the largest products: L = 32768 columns, all equal but one -- 100 * 32767 < 100 * 32768 in int32
    big = np.full((2, 32768), 7, dtype=np.uint8)
    big[1, 12345] = 6
    di, dat = device(big, GAP, 0, 20, 100, 5)
    assert list(di) == [0, 1] and list(dat) == [100, 100]
    di, _ = device(big, GAP, 0, 20, 99, 5)
    assert list(di) == [0]


def test_rows_without_a_common_column_are_never_redundant():
    a = np.full((3, 20), GAP, dtype=np.uint8)
    a[0, :5], a[1, 5:10], a[2, 12:17] = 4, 4, 4
    kept, at, _ = same_as_truth(a, GAP, 0, 1, 1, 1)         # threshold 1 %: anything with a common column would be redundant
    assert list(kept) == [0, 1, 2] and list(at) == [1, 1, 1]
    a[2, 4] = 4                                             # one common column with row 0, equal: 100 %
    kept, _, _ = same_as_truth(a, GAP, 0, 1, 100, 1)
    assert list(kept) == [0, 1]


def test_all_gap_rows():
    a = planted(70, 12, 3)
    a[[5, 64, 69]] = GAP
    kept, at, _ = same_as_truth(a, GAP, 70, *SCHEDULE)
    assert not {5, 64, 69} & set(kept) and (at[[5, 64, 69]] == -1).all()
    a[0] = GAP                                              # ... but the first of the order is kept, and makes nothing redundant
    kept, at, _ = same_as_truth(a, GAP, 70, *SCHEDULE)
    assert kept[0] == 0 and at[0] == 35 and len(kept) > 1
    only = np.full((3, 9), GAP, dtype=np.uint8)
    kept, at, _ = same_as_truth(only, GAP, 0)
    assert list(kept) == [0] and list(at) == [90, -1, -1]


@pytest.mark.parametrize("gap, symbols", [(0, (1, 2, 255, 128)), (255, (0, 1, 127, 128)), (45, (0, 255, 65, 67)), (128, (0, 127, 129, 255))])
def test_byte_values_and_padded_rows(gap, symbols):
    for N, L in ((40, 9), (130, 65)):
        a = T.alignment(N, L, gap + N, gap=gap, symbols=symbols, p_mut=0.4)
        memo = {}
        want = same_as_truth(a, gap, N, *SCHEDULE, memo=memo)[0]
        got = same_as_truth(a, gap, N, *SCHEDULE, ld=L + 11, memo=memo)[0]     # garbage behind every row
        assert np.array_equal(want, got) and 1 < len(want) < N


def test_a_fragment_falls_to_the_longer_row_unless_the_order_puts_it_first():
    rng = np.random.RandomState(5)
    L = 40
    a = np.full((4, L), GAP, dtype=np.uint8)
    a[0] = rng.randint(20, 24, size=L)                      # the query: symbols of its own
    a[1, :30] = rng.randint(4, 8, size=30)                  # a fragment of the long row, ahead of it in the file
    a[2] = np.concatenate([a[1, :30], rng.randint(4, 8, size=10)])
    a[3, 10:25] = a[2, 10:25]
    kept, at, _ = same_as_truth(a, GAP, 0)                  # default order 0, 2, 1, 3: the long row first
    assert list(kept) == [0, 2] and list(at) == [90, -1, 90, -1]
    kept, _, _ = same_as_truth(a, GAP, 0, order=[0, 3, 1, 2])
    assert list(kept) == [0, 3]                             # ... and now both longer rows fall to the short fragment
    kept, _, _ = same_as_truth(a, GAP, 0, order=[1, 0, 2, 3])
    assert list(kept) == [0, 1]


def test_an_order_entry_outside_the_rows_is_refused_and_nothing_is_written():
    lib = _lib.load()
    N, L = 70, 12
    a = torch.from_numpy(planted(N, L, 1)).to(DEV)
    ws = torch.empty(lib.rnamsm_seqid_filter_workspace_bytes(N, L), dtype=torch.uint8, device=DEV)
    for bad in ({3: N}, {69: -1}, {40: 1 << 30, 17: -5, 66: N + 3}):
        order = np.arange(N, dtype=np.int32)
        for p, v in bad.items():
            order[p] = v
        idx = torch.full((N,), -77, dtype=torch.int32, device=DEV)
        at = torch.full((N,), -88, dtype=torch.int32, device=DEV)
        n_kept = ctypes.c_int(-99)
        with torch.cuda.device(DEV):
            rc = lib.rnamsm_seqid_filter(a.data_ptr(), N, L, L, GAP, torch.from_numpy(order).to(DEV).data_ptr(), 16, 20, 90, 5,
                                         idx.data_ptr(), at.data_ptr(), ctypes.addressof(n_kept), ws.data_ptr(), ws.numel(),
                                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == -1 and f"seqid_filter: order[{min(bad)}] lies outside [0, {N})" in lib.rnamsm_last_error().decode()
        assert n_kept.value == -99 and (idx == -77).all() and (at == -88).all()
    with pytest.raises(_lib.RnamsmError, match=r"order\[3\] lies outside"):
        ops.seqid_filter(a, GAP, 16, order=torch.tensor([0, 1, 2, N] + list(range(4, N)), dtype=torch.int32, device=DEV))
    same_as_truth(a.cpu().numpy(), GAP, 16, order=np.arange(N)[::-1])         # a valid order of the same rows goes through


def test_the_passes():
    a = planted(200, 64, 11)
    memo = {}
    kept, at, passes = same_as_truth(a, GAP, 200, memo=memo)
    assert len(passes) == 15 and len(set(at[at >= 0])) > 3 and at[0] == 20          # rows rejected at 20 are kept at later thresholds
    later = [i for i in kept if at[i] > 20]
    assert later and all(i not in T.seqid_filter(a, GAP, 0, 20, 20, 5, memo=memo)[0] for i in later[:5])
    # the walk stops at the first pass that reaches num_seqs
    target = passes[7][1]
    assert passes[6][1] < target
    kept8, at8, passes8 = same_as_truth(a, GAP, target, memo=memo)
    assert passes8 == passes[:8] and len(kept8) == target and at8.max() == passes[7][0]
    kept8m, _, passes8m = same_as_truth(a, GAP, passes[6][1] + 1, memo=memo)
    assert passes8m == passes[:8] and np.array_equal(kept8m, kept8)                 # more than num_seqs rows may come back
    # num_seqs = 0 is one pass at max_seqid
    kept0, at0, passes0 = same_as_truth(a, GAP, 0, memo=memo)
    assert passes0 == [(90, len(kept0))] and set(at0) == {-1, 90}


def test_every_chunk_size_and_every_run_give_the_same_outputs(chunk):
    a = planted(257, 100, 13)
    want = T.seqid_filter(a, GAP, 257, *SCHEDULE)
    want0 = T.seqid_filter(a, GAP, 0)
    assert 1 < len(want0[0]) < 257
    for size in (64, 128, 256, 512, 64):
        chunk(size)
        for _ in range(2):
            di, dat = device(a, GAP, 257, *SCHEDULE)
            assert np.array_equal(di, want[0]) and np.array_equal(dat, want[1]), size
            di, dat = device(a, GAP, 0)
            assert np.array_equal(di, want0[0]) and np.array_equal(dat, want0[1]), size


def test_several_chunks_of_the_default_size():
    a = T.alignment(900, 70, 21, families=40, p_mut=0.3)
    _, _, passes = same_as_truth(a, GAP, 100)
    assert passes[-1][1] >= 100 and len(passes) > 3


@pytest.fixture(scope="module")
def full():
    a = golden("tokens_2DRB_1_full.npz")["all_tokens"][:, 1:].astype(np.uint8)
    assert a.shape == (1176, 35)
    return a, {}


@pytest.mark.parametrize("num_seqs, n", [(0, 275), (64, 93), (512, 308)])
def test_the_full_2drb1_alignment(full, num_seqs, n):
    kept, _, _ = same_as_truth(full[0], GAP, num_seqs, memo=full[1])
    assert len(kept) == n
