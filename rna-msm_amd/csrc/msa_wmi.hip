// Sequence-weighted mutual information of an alignment on the device (rnamsm_msa_wmi): rnamsm_msa_mi's two maps with every row n
// counted w[n] times instead of once,
//   c(i,a; j,b) = sum over rows n of w[n] * [x(n,i) = a] * [x(n,j) = b]        float64,
// the pair frequencies that covariation tools reweight by MSA.weights (1 / neighbours within a Hamming distance).  A weighted count
// is no popcount: it is the contraction C = Y^T diag(w) Y of the one-hot matrix Y [N, L*S] with fp64 accumulation, and it runs on
// the fp64 matrix pipe (v_mfma_f64_16x16x4_f64).
//
// Data flow (all on the caller's stream; every buffer in the caller's workspace):
//   verdict    the first row whose weight is not finite or not > 0, or -1                wmi_check_kernel -> read back with K
//   stage 1    invcov.hip's: presence, table (host reads K), bit planes P[w][i*K + a], integer marginals (unused here)
//   states     Q[w][i*S + a]: P's planes, and in gap mode "state" one more plane per column, a = K: "row n holds a gap in column i"
//              = the rows of the word that no symbol plane has (K <= 16 is checked: every other value is a symbol), counted
//              directly, not by subtraction.  S = K + 1 there, S = K in "pairwise".  Word-major like P, L*S rows padded to a
//              multiple of 64 plus 64 more (a tile that starts at any row reads inside the buffer), zero where nothing was
//              written                                                                                        wmi_states_kernel
//   counts     a band of columns i at a time, [i - i0][j][a][b] float64                                       wmi_count_kernel
//   profile    wmarg[i][a] = c(i,a; i,a), read off the band                                                 wmi_profile_kernel
//   mi         one thread per (i, j >= i) on the S x S table of doubles, mirrored on write                    wmi_pair_kernel
//   mip        apc.hip's rnamsm_apc_f64 of the map with a zero diagonal
//
// The contraction.  A block of 256 threads (4 waves, 2 x 2) owns a 64 x 64 tile of the (L*S) x (L*S) result over ALL N rows: no
// atomics, no split over N.  A wave owns 32 x 32 of it as 2 x 2 MFMA tiles: 4 accumulators of 4 doubles, 32 registers (the
// compiler keeps them in AGPRs; 38 VGPRs beside them).  One MFMA step contracts 4 alignment rows: lane l supplies A[row l & 15][k = l >> 4] and B[k = l >> 4][column l & 15], one double each, and holds
// D[row (l >> 4) + 4 * reg][column l & 15] in register reg (the f64 layout; the f32 maps of mma_core.h do not apply).  A is formed
// from the planes and the weights -- bit set -> w[n], else 0.0 -- by a SELECT, never a product, so a weight is read as it is and
// rows past N never count; B is 1.0 / 0.0.  Every product is exact (w * 1 or 0): the only rounding is the accumulation's.
// Staging: 4 words = 256 alignment rows per step in LDS -- the tile's 64 + 64 plane words each (2 x 2 KB) and the 256 weights
// (2 KB), 6 KB a block, single-buffered between two barriers; a step is 256 MFMAs a wave, and several blocks share a CU.
// Order of summation of one result, fixed and the same for every tile position, band and run: the rows in groups of four,
// n = 4g .. 4g + 3, g ascending from an accumulator of 0.0; within a group the instruction's own order of its four products.  Rows
// whose bit is clear add an exact 0.0.  c(i,a; j,b) and c(j,b; i,a) add the same values in the same order: equal bit for bit.
// Tiles wholly below the diagonal are skipped unless the caller asked for the counts.
#include "block_scan.h"
#include "invcov_stage1.h"

namespace rnamsm {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int WM_TILE = 64;        // (column, state) rows of a count tile, each way
constexpr int WM_WORDS = 4;        // words staged per step: 256 alignment rows (IC_WK is a multiple of it)
constexpr int WM_MAX_S = IC_MAX_K + 1;
constexpr size_t WM_BAND_BYTES = (size_t)1 << 28;      // counts of one band of columns i, by default
static_assert(IC_WK % WM_WORDS == 0, "the planes' word padding covers whole steps");

// one block of 1024: the lowest row whose weight is NaN, +-inf, zero or negative; -1 when there is none
__global__ __launch_bounds__(1024) void wmi_check_kernel(const double* __restrict__ w, int N, int32_t* __restrict__ verdict) {
    const int first = block_first_index(N, [&](int n) { return !(w[n] > 0.0 && w[n] < INFINITY); });      // (NaN fails both comparisons)
    if (threadIdx.x == 0) *verdict = first;
}

// Q[w][i*S + a] from P[w][i*K + a]; one thread per (word, column, state).  S == K + 1: state K is the word's rows without a symbol.
__global__ __launch_bounds__(256) void wmi_states_kernel(const uint64_t* __restrict__ P, int64_t Rp, int N, int W, int L, int K, int S,
                                                         int64_t Rq, uint64_t* __restrict__ Q) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int w = blockIdx.y;
    if (r >= (int64_t)L * S || w >= W) return;
    const int i = (int)(r / S), a = (int)(r - (int64_t)i * S);
    const uint64_t* p = P + (int64_t)w * Rp + (int64_t)i * K;
    uint64_t v;
    if (a < K) {
        v = p[a];
    } else {
        const int left = N - w * 64;                                    // rows of this word: 1 .. 64 and more
        v = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
        for (int q = 0; q < K; ++q) v &= ~p[q];
    }
    Q[(int64_t)w * Rq + r] = v;
}

__device__ __forceinline__ f64x4 mfma_f64(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// grid (column tiles, row tiles of the band).  row0: first (column, state) row of the band, ANY row; rows_end: one past its last.
// cnt: the band's counts, [i - i0][j][a][b].  Wp: words, a multiple of WM_WORDS.  R = L * S; Rq >= round_up(R, 64) + 64.
__global__ __launch_bounds__(256) void wmi_count_kernel(const uint64_t* __restrict__ Q, const double* __restrict__ wgt, int N, int Wp,
                                                        int64_t Rq, int64_t R, int S, int L, int64_t row0, int64_t rows_end, int i0,
                                                        int full, double* __restrict__ cnt) {
    __shared__ uint64_t sA[WM_WORDS][WM_TILE];
    __shared__ uint64_t sB[WM_WORDS][WM_TILE];
    __shared__ double sW[WM_WORDS * 64];
    const int64_t rb = row0 + (int64_t)blockIdx.y * WM_TILE, cb = (int64_t)blockIdx.x * WM_TILE;
    if (!full) {                                       // every pair of the tile has j < i: the pair kernel reads the upper triangle only
        const int64_t last_c = cb + WM_TILE - 1 < R - 1 ? cb + WM_TILE - 1 : R - 1;
        if (last_c / S < rb / S) return;
    }
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;             // the wave's 32 x 32 of the tile
    const int lr = lane & 15, kq = lane >> 4;
    f64x4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = (f64x4)(0.0);

    for (int w0 = 0; w0 < Wp; w0 += WM_WORDS) {
        {
            const uint64_t* base = Q + (int64_t)(w0 + wave) * Rq;      // thread t: word t / 64, tile row t % 64
            sA[wave][lane] = base[rb + lane];
            sB[wave][lane] = base[cb + lane];
            const int64_t n = (int64_t)w0 * 64 + t;
            sW[t] = n < N ? wgt[n] : 0.0;
        }
        __syncthreads();
#pragma unroll 1
        for (int wi = 0; wi < WM_WORDS; ++wi) {
            const uint64_t a0 = sA[wi][wr + lr] >> kq, a1 = sA[wi][wr + 16 + lr] >> kq;
            const uint64_t b0 = sB[wi][wc + lr] >> kq, b1 = sB[wi][wc + 16 + lr] >> kq;
#pragma unroll
            for (int g = 0; g < 16; ++g) {                             // rows 64 (w0 + wi) + 4 g + kq
                const double wv = sW[wi * 64 + 4 * g + kq];
                const double A0 = ((a0 >> (4 * g)) & 1ull) ? wv : 0.0, A1 = ((a1 >> (4 * g)) & 1ull) ? wv : 0.0;
                const double B0 = ((b0 >> (4 * g)) & 1ull) ? 1.0 : 0.0, B1 = ((b1 >> (4 * g)) & 1ull) ? 1.0 : 0.0;
                acc[0][0] = mfma_f64(A0, B0, acc[0][0]);
                acc[0][1] = mfma_f64(A0, B1, acc[0][1]);
                acc[1][0] = mfma_f64(A1, B0, acc[1][0]);
                acc[1][1] = mfma_f64(A1, B1, acc[1][1]);
            }
        }
        __syncthreads();
    }
    const int64_t SS = (int64_t)S * S;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t r = rb + wr + x * 16 + kq + 4 * reg;         // D: row (lane >> 4) + 4 reg, column lane & 15
            if (r >= rows_end) continue;
            const int i = (int)(r / S), a = (int)(r - (int64_t)i * S);
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                const int64_t col = cb + wc + y * 16 + lr;
                if (col >= R) continue;
                const int j = (int)(col / S), b = (int)(col - (int64_t)j * S);
                cnt[((int64_t)(i - i0) * L + j) * SS + a * S + b] = acc[x][y][reg];
            }
        }
}

// wmarg[i][a] = c(i,a; i,a) of the band's columns
__global__ __launch_bounds__(256) void wmi_profile_kernel(const double* __restrict__ cnt, int L, int S, int i0, int i1,
                                                          double* __restrict__ wmarg) {
    const int64_t r = (int64_t)i0 * S + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (int64_t)i1 * S) return;
    const int i = (int)(r / S), a = (int)(r - (int64_t)i * S);
    wmarg[r] = cnt[((int64_t)(i - i0) * L + i) * S * S + a * S + a];
}

// ---- mutual information of a band of weighted counts -------------------------------------------------------------------------------
// One thread per (i, j >= i): mi_pair_kernel's formula and order with doubles in place of integers.  On the pair's table c[a][b],
// a, b < S (in "state" mode the gap is state K, counted like any other):
//   s_b = sum_a c[a][b], a ascending;  r_a = sum_b c[a][b], b ascending;  n = sum_b s_b, b ascending;
//   mi = sum over a then b ascending, the entries with c > 0 only, of (c / n) * log((c * n) / (r_a * s_b)),
// one operation at a time (no contraction); n = 0 gives 0.  s_b is kept in LDS, element-major [b][thread]: conflict-free, and a
// thread reads only what it wrote, so there is no barrier.  With every weight 1.0 all of these are integers below 2^53 and the
// value is mi_pair_kernel's, bit for bit, in both gap modes.  The value goes to (i, j) and (j, i).
__global__ __launch_bounds__(256) void wmi_pair_kernel(const double* __restrict__ cnt, int L, int S, int i0, int i1,
                                                       double* __restrict__ mi) {
    __shared__ double s_col[WM_MAX_S * 256];
    const int t = threadIdx.x;
    const int j = blockIdx.x * 256 + t, i = i0 + blockIdx.y;
    if (i >= i1 || j >= L || j < i) return;                       // (no barrier below)
    const double* cb = cnt + ((int64_t)(i - i0) * L + j) * S * S;
    double n = 0.0;
    for (int b = 0; b < S; ++b) {
        double s = 0.0;
        for (int a = 0; a < S; ++a) s += cb[a * S + b];
        s_col[b * 256 + t] = s;
        n += s;
    }
    double sum = 0.0;
    if (n > 0.0) {
        for (int a = 0; a < S; ++a) {
            double r = 0.0;
            for (int b = 0; b < S; ++b) r += cb[a * S + b];
            for (int b = 0; b < S; ++b) {
                const double c = cb[a * S + b];
                if (c > 0.0) {
                    const double ratio = (c * n) / (r * s_col[b * 256 + t]);
                    const double w = c / n;
                    sum += w * log(ratio);
                }
            }
        }
    }
    mi[(int64_t)i * L + j] = sum;
    mi[(int64_t)j * L + i] = sum;
}

struct WmiWs {
    size_t verdict, states, map, apc, band, per_col_max, total;     // behind stage 1's bytes up to the end of its planes
    int64_t Rq;                                                     // rows of Q, laid out for S = 17
};
static int64_t wmi_rows(int L, int S) { return ((int64_t)L * S + WM_TILE - 1) / WM_TILE * WM_TILE + WM_TILE; }
static WmiWs wmi_ws(int N, int L) {
    const InvcovWs s1 = invcov_ws(N, L, IC_MAX_K);
    WmiWs w;
    w.Rq = wmi_rows(L, WM_MAX_S);
    size_t off = s1.band;                                           // (256-aligned: the end of the planes)
    w.verdict = off; off += 256;
    w.states = off;  off += (size_t)s1.Wp * (size_t)w.Rq * 8;
    off = (off + 255) & ~(size_t)255;
    w.map = off;     off += (((size_t)L * L * 8) + 255) & ~(size_t)255;
    w.apc = off;     off += (rnamsm_apc_f64_workspace_bytes(L) + 255) & ~(size_t)255;
    w.band = off;
    w.per_col_max = (size_t)L * WM_MAX_S * WM_MAX_S * 8;            // one column i of counts at S = 17
    const size_t whole = w.per_col_max * L;
    w.total = off + (whole < WM_BAND_BYTES ? whole : WM_BAND_BYTES);   // (per_col_max <= 9.1 MB: at least 28 columns)
    return w;
}
static bool wmi_shape_ok(int N, int L) { return N >= 2 && N <= IC_MAX_N && L >= 1 && L <= RNAMSM_LONG_MAX_L; }

}  // namespace rnamsm

using namespace rnamsm;

extern "C" size_t rnamsm_msa_wmi_workspace_bytes(int N, int L) {
    if (!wmi_shape_ok(N, L)) return 0;
    return wmi_ws(N, L).total;
}

extern "C" size_t rnamsm_msa_wmi_min_workspace_bytes(int N, int L) {
    if (!wmi_shape_ok(N, L)) return 0;
    const WmiWs w = wmi_ws(N, L);
    return w.band + w.per_col_max;
}

extern "C" int rnamsm_msa_wmi(const uint8_t* tokens, int N, int L, int64_t ld, int gap, int gap_mode, const double* weights,
                              double* mi, double* mip, double* wcounts, double* wmarg, int32_t* meta, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (int rc = stage1_check("msa_wmi", tokens && workspace && weights, N, L, ld, gap)) return rc;
    RNAMSM_CHECK_ARG(gap_mode == RNAMSM_MI_GAPS_PAIRWISE || gap_mode == RNAMSM_MI_GAPS_STATE,
                     "msa_wmi: gap_mode=%d is not 0 (pairwise) or 1 (state)", gap_mode);
    RNAMSM_CHECK_ARG(mi || mip || wcounts, "msa_wmi: mi, mip and wcounts are all NULL: nothing to compute");
    const WmiWs ww = wmi_ws(N, L);
    const size_t need = ww.band + ww.per_col_max;
    RNAMSM_CHECK_ARG(workspace_bytes >= need, "msa_wmi: workspace of %zu bytes is smaller than the %zu that N=%d, L=%d need at least",
                     workspace_bytes, need, N, L);
    RNAMSM_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "msa_wmi: workspace misaligned (256 bytes)");
    RNAMSM_CHECK_ARG((reinterpret_cast<uintptr_t>(weights) & 7u) == 0 && (reinterpret_cast<uintptr_t>(mi) & 7u) == 0 &&
                         (reinterpret_cast<uintptr_t>(mip) & 7u) == 0 && (reinterpret_cast<uintptr_t>(wcounts) & 7u) == 0 &&
                         (reinterpret_cast<uintptr_t>(wmarg) & 7u) == 0 && (reinterpret_cast<uintptr_t>(meta) & 3u) == 0 &&
                         (!mi || mi != mip),
                     "msa_wmi: weights / mi / mip / wcounts / wmarg / meta misaligned, or one buffer for mi and mip");
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);

    // ---- the weights' verdict travels with K: one wait for the stream
    int32_t* verdict = reinterpret_cast<int32_t*>(ws + ww.verdict);
    hipLaunchKernelGGL(wmi_check_kernel, dim3(1), dim3(1024), 0, s, weights, N, verdict);
    Stage1 st;
    Stage1Verdict sv{verdict, -1};
    if (int rc = stage1_planes("msa_wmi", tokens, N, L, ld, gap, ws, s, &st, &sv)) return rc;
    RNAMSM_CHECK_ARG(sv.host < 0, "msa_wmi: weights[%d] is not finite and > 0 (the first such row)", sv.host);

    const int K = st.K, S = gap_mode == RNAMSM_MI_GAPS_STATE ? K + 1 : K;
    const int64_t R = (int64_t)L * S, Rq = wmi_rows(L, S);
    uint64_t* Q = reinterpret_cast<uint64_t*>(ws + ww.states);
    if (hipMemsetAsync(Q, 0, (size_t)st.w.Wp * (size_t)Rq * 8, s) != hipSuccess) return fail(RNAMSM_ERR_HIP, "msa_wmi: hipMemsetAsync failed");
    hipLaunchKernelGGL(wmi_states_kernel, dim3((unsigned)((R + 255) / 256), st.w.W), dim3(256), 0, s, st.P, st.w.Rp, N, st.w.W, L, K, S, Rq, Q);
    if (meta && hipMemcpyAsync(meta, st.meta, IC_META * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return fail(RNAMSM_ERR_HIP, "msa_wmi: hipMemcpyAsync failed");

    // the band: as many columns i as the workspace has room for behind its fixed part -- a function of workspace_bytes (and S) alone
    const size_t per_col = (size_t)L * S * S * 8;
    const size_t room = (workspace_bytes - ww.band) / per_col;
    const int band = wcounts ? L : (room > (size_t)L ? L : (int)room);          // >= 1: per_col <= per_col_max
    double* map = mi ? mi : reinterpret_cast<double*>(ws + ww.map);
    for (int i0 = 0; i0 < L; i0 += band) {
        const int i1 = i0 + band < L ? i0 + band : L;
        double* cnt = wcounts ? wcounts : reinterpret_cast<double*>(ws + ww.band);
        const int64_t row0 = (int64_t)i0 * S, rows_end = (int64_t)i1 * S;
        hipLaunchKernelGGL(wmi_count_kernel, dim3((unsigned)((R + WM_TILE - 1) / WM_TILE), (unsigned)((rows_end - row0 + WM_TILE - 1) / WM_TILE)),
                           dim3(256), 0, s, Q, weights, N, st.w.Wp, Rq, R, S, L, row0, rows_end, i0, wcounts ? 1 : 0, cnt);
        if (wmarg)
            hipLaunchKernelGGL(wmi_profile_kernel, dim3((unsigned)((rows_end - row0 + 255) / 256)), dim3(256), 0, s, cnt, L, S, i0, i1, wmarg);
        if (mi || mip)
            hipLaunchKernelGGL(wmi_pair_kernel, dim3((L + 255) / 256, i1 - i0), dim3(256), 0, s, cnt, L, S, i0, i1, map);
    }
    RNAMSM_CHECK_LAUNCH("msa_wmi");
    if (!mip) return RNAMSM_OK;
    return rnamsm_apc_f64(map, L, L, 1, mip, ws + ww.apc, rnamsm_apc_f64_workspace_bytes(L), stream);      // mip = apc(mi with a zero diagonal)
}
