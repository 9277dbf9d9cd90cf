"""Truth for the contact head (csrc/contact_head.hip): symmetrize + APC (utils/tensor.py:98-113), the 120 -> 1 regression and the
sigmoid (modules.py:344-366) restated stage by stage on the stripped maps atp [nch, T, T], at any dtype -- fp64 is the truth, fp32
the yardstick of the GPU tests' bars (tests/ss_truth.py: compare).  The fp32 version sums with the library's own `sum`; nothing
here imitates the order of the kernels.  tests/test_contact_truth.py ties `stages` to oracle.msm_oracle.contact_head and proves the
conditions of the generators below at every shape the GPU tests use.  Test infrastructure only."""
import numpy as np
import torch

# ------------------------------------------------------------------ the shapes of the GPU tests (tests/test_gpu_contact_head_*.py)
ATP_TS = (1, 2, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1023)      # through rnamsm_contact_head_atp
UNSTRIPPED_TS = (1, 32, 256, 257, 1023)                              # also as C = T + 1 through rnamsm_contact_head (off = 1)
LONG_TS = (1025, 4096)                                               # through rnamsm_contact_head_long, in a band of LONG_BAND
LONG_BAND = 1023
PACKED_TS = (257, 1, 256, 513, 33)                                   # one packed call, forward and reversed
NCHS = (120, 7)


def exact_nch(T: int, nch: int) -> int:
    """Channels of the exact case: at most 8 at T = 4096 (tot = 2^17 leaves the channel sum 24 - 17 bits)."""
    return min(nch, 8) if T > 2048 else nch


def loud_nch(T: int, nch: int) -> int:
    """Channels of the real-valued case: 40 for 120 at T = 4096, where the last plane still starts beyond 2^31 bytes."""
    return min(nch, 40) if T > 2048 else nch


def band_of(T: int):
    return LONG_BAND if T > 1023 else None


def shapes(kind: str) -> list:
    """The (T, nch) of the lone GPU cases, kind "exact" or "loud": both channel counts, at T = 4096 the one the kind allows."""
    cap = exact_nch if kind == "exact" else loud_nch
    return [(T, cap(T, nch)) for T in ATP_TS + LONG_TS for nch in (NCHS if T <= 2048 else NCHS[:1])]


def case_seed(T: int, nch: int) -> int:
    return 7000 + 131 * T + nch


# ------------------------------------------------------------------ the stages
def stages(atp, weight, bias, dtype=torch.float64, device="cpu") -> dict:
    """{rs [nch, T], tot [nch], logits [T, T], contacts [T, T]} of the stripped maps atp [nch, T, T] (numpy or torch, any
    device) as numpy arrays of `dtype`, channel by channel on `device`:
        s = x + x^T;  rs = s.sum(-1) (= s.sum(-2): s is symmetric);  tot = s.sum();  n = s - rs rs^T / tot
        logits = bias + sum_ch weight[ch] n_ch;  contacts = sigmoid(logits)."""
    a = atp if isinstance(atp, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(atp))
    nch, T = int(a.shape[0]), int(a.shape[-1])
    w = torch.as_tensor(np.asarray(weight, dtype=np.float64).reshape(-1)).to(device=device, dtype=dtype)
    b = torch.as_tensor(np.asarray(bias, dtype=np.float64).reshape(())).to(device=device, dtype=dtype)
    assert a.shape == (nch, T, T) and w.shape == (nch,)
    rs = torch.empty(nch, T, dtype=dtype, device=device)
    tot = torch.empty(nch, dtype=dtype, device=device)
    z = torch.zeros(T, T, dtype=dtype, device=device)
    for ch in range(nch):
        x = a[ch].to(device=device, dtype=dtype)
        s = x + x.T
        a1, a2, a12 = s.sum(-1, keepdim=True), s.sum(-2, keepdim=True), s.sum()
        rs[ch], tot[ch] = a1[:, 0], a12
        z += w[ch] * (s - (a1 * a2) / a12)
    z = z + b
    out = {"rs": rs, "tot": tot, "logits": z, "contacts": torch.sigmoid(z)}
    return {k: v.cpu().numpy() for k, v in out.items()}


def stages_in_order(atp, weight, bias, order=None, ch_order=None) -> dict:
    """The same four in float32 numpy with every sum SEQUENTIAL (np.cumsum) in a chosen order: positions in `order` (a permutation of
    range(T) applied to rows and columns alike; default ascending), channels in `ch_order`.  The APC term in its other
    spelling, s - (r_i r_j) (1 / tot), where `stages` and the kernel divide.  For tests/test_contact_truth.py: on exact_case every order must give the fp64 values."""
    atp = np.asarray(atp, dtype=np.float32)
    nch, T = atp.shape[0], atp.shape[-1]
    p = np.arange(T) if order is None else np.asarray(order)
    f32 = np.float32
    rs, tot, zp = np.empty((nch, T), f32), np.empty(nch, f32), np.zeros((T, T), f32)
    with np.errstate(all="ignore"):
        for ch in (range(nch) if ch_order is None else ch_order):
            x = atp[ch][p][:, p]
            r = np.cumsum(x, axis=1, dtype=f32)[:, -1] + np.cumsum(x, axis=0, dtype=f32)[-1, :]
            t = np.cumsum(r, dtype=f32)[-1]
            rs[ch, p], tot[ch] = r, t
            zp += f32(weight[ch]) * ((x + x.T) - (r[:, None] * r[None, :]) * (f32(1) / t))
        z = np.empty_like(zp)
        z[np.ix_(p, p)] = zp + f32(np.asarray(bias).reshape(-1)[0])
        return {"rs": rs, "tot": tot, "logits": z, "contacts": (f32(1) / (f32(1) + np.exp(-z))).astype(f32)}


# ------------------------------------------------------------------ real-valued inputs that make an indexing fault loud
def seam_mask(T: int, period: int) -> np.ndarray:
    """bool [T]: the positions next to a multiple of `period` (index mod period in {0, period - 1})."""
    idx = np.arange(T)
    return np.isin(idx % period, (0, period - 1))


def loud_maps(nch: int, L: int, seed: int, band=None) -> np.ndarray:
    """Non-negative float32 [nch, L, L], attention-sized (about 1 / L): x[ch, i, j] = a[ch, i] b[ch, j] u[ch, i, j] boost[i, j] / L.
    a and b are log-uniform over 10^+-0.6 (a factor 16), so the row sums r_i vary strongly with i and the maps are asymmetric; u is
    uniform in [0.25, 1); boost is 4 on the rows and columns next to a multiple of 32, 8 on those next to a multiple of 256 and on
    0 and L - 1, 1 elsewhere (the larger of the row's and the column's).  band: +0.0 outside |i - j| < band, like a stitched atp."""
    rng = np.random.default_rng(seed)
    idx = np.arange(L)
    b1 = np.where(seam_mask(L, 256) | (idx == 0) | (idx == L - 1), 8.0, np.where(seam_mask(L, 32), 4.0, 1.0)).astype(np.float32)
    boost = np.maximum(b1[:, None], b1[None, :]) / np.float32(L)
    if band is not None:
        boost = boost * (np.abs(idx[:, None] - idx[None, :]) < band)
    out = np.empty((nch, L, L), np.float32)
    for ch in range(nch):
        a = (10.0 ** rng.uniform(-0.6, 0.6, L)).astype(np.float32)
        b = (10.0 ** rng.uniform(-0.6, 0.6, L)).astype(np.float32)
        u = rng.random((L, L), dtype=np.float32) * np.float32(0.75) + np.float32(0.25)
        u *= boost
        u *= a[:, None]
        u *= b[None, :]
        out[ch] = u
    return out


LOUD_STD = 1.5


def loud_regression(atp, seed: int, device="cpu"):
    """(weight [nch], bias [1]) float32: normal weights scaled from the fp64 stages so that the fp64 logits of `atp` have a standard
    deviation of LOUD_STD (the logits are linear in the weights), bias 0.3: the sigmoid works on its slope, not on its plateaus."""
    nch = int(atp.shape[0])
    w0 = np.random.default_rng(seed).standard_normal(nch)
    z0 = stages(atp, w0, 0.0, torch.float64, device)["logits"]
    sd = float(z0.std())
    scale = LOUD_STD / sd if sd > 0 else 1.0                 # T = 1: the one logit is the bias, whatever the weights
    return (w0 * scale).astype(np.float32), np.array([0.3], np.float32)


# ------------------------------------------------------------------ inputs on which every stage has ONE correct fp32 value
def exact_case(nch: int, L: int, seed: int, band=None):
    """(atp [nch, L, L], weight [nch], bias [1]) float32 on which rs, tot and the logits are exactly representable however they
    are summed.  A plane is c x {0, 1} with c a power of two, except one top-up element of c x 3 (c x 1 on the tiniest planes) that
    lies off the diagonal at a 32- or 256-seam or in a corner; the number of ones is chosen so that sum(x) = c 2^(k - 1), hence
    tot = c 2^k and 1 / tot is exact.  k is the largest with density <= 1/2, k <= 18 and k + bits(2 nch) <= 24: a channel's term
    s - r_i r_j / 2^k is a multiple of 2^-k of size about 2 at most, so a prefix of sum_ch +-term stays within 24 bits; c puts the
    logits' spread between 1.5 and 3.  weight is +-1, bias 1/4.  That is the intent; the proof is tests/test_contact_truth.py,
    which evaluates every shape in fp64 and in two fp32 orders."""
    rng = np.random.default_rng(seed)
    idx = np.arange(L)
    allowed = np.ones((L, L), bool) if band is None else (np.abs(idx[:, None] - idx[None, :]) < band)
    flat = np.flatnonzero(allowed.ravel())
    n_allowed = flat.size
    k_bits = 24 - int(np.ceil(np.log2(2 * nch + 1)))                     # nch = 120: 16; 7 or 8: 20, capped at 18
    k = 1 + max(0, min(k_bits - 1, 17, int(np.floor(np.log2(max(n_allowed / 2.0, 1.0))))))
    ones_total = 1 << (k - 1)                                            # sum of a plane in units of c
    topup = 3 if ones_total >= 8 else 1
    spots = [(0, L - 1), (L - 1, 0), (31, 32), (32, 31), (255, 256), (256, 255), (0, 32), (31, L - 1)]
    spots = [(i, j) for i, j in spots if 0 <= i < L and 0 <= j < L and i != j and allowed[i, j]] or [(0, 0)]
    dens = ones_total / max(n_allowed, 1)
    sigma0 = np.sqrt(max(nch * 2.0 * dens * (1.0 - min(dens, 1.0)), 1e-30))
    c = np.float32(2.0 ** int(np.clip(np.floor(np.log2(3.0 / sigma0)), -3, 3)))
    atp = np.zeros((nch, L, L), np.float32)
    for ch in range(nch):
        ti, tj = spots[ch % len(spots)]
        pool = flat[flat != ti * L + tj]
        n = ones_total - topup
        assert 0 <= n <= pool.size, (L, nch, k, n, pool.size)
        plane = atp[ch].reshape(-1)
        plane[rng.choice(pool, size=n, replace=False, shuffle=False)] = c
        plane[ti * L + tj] = c * np.float32(topup)
    # the signs depend on nch alone: the members of a packed call share one regression, and each is proved with these weights
    weight = np.where(np.random.default_rng(1000 + nch).random(nch) < 0.5, -1.0, 1.0).astype(np.float32)
    return atp, weight, np.array([0.25], np.float32)


# ------------------------------------------------------------------ fp32 ulps
def ulps_f32(got, want64) -> np.ndarray:
    """|got - want64| in units of the fp32 spacing at |want64| (rounded to fp32), element-wise, float64."""
    want64 = np.asarray(want64, np.float64)
    spacing = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - want64) / spacing
