// Covariance contacts of an alignment on the device (MSA.invcov, utils/align.py:183-193): the classical co-evolution map,
//   out[i, j] = || cov(onehot column i, onehot column j) ||_2     float64 [L, L],
// from the raw alignment, without the network.  The reference one-hot encodes the N x L characters over the K distinct non-gap
// values that occur (ascending; a gap is all zeros), takes np.cov of the [N, L*K] matrix (N - 1 in the denominator) and the
// spectral norm of every K x K block.  An entry of that covariance is a rational function of INTEGER counts,
//   c[(i,a),(j,b)] = (n_ab(i,j) - n_a(i) * n_b(j) / N) / (N - 1),      n_ab(i,j) = #{rows with a in column i and b in column j},
// n_a(i) = n_aa(i,i), so the O(L^2 N) part is exact integer work and the N x L x K one-hot never exists.
//
// Data flow (all on the caller's stream; every buffer in the caller's workspace):
//   presence   which of the 256 byte values occur                                       invcov_presence_kernel
//   table      byte -> symbol index (0xFF: the gap or absent), K and the K symbols      invcov_table_kernel   -> host reads K
//   planes     P[w][i*K + a]: bit n % 64 of word n / 64 says "row n has symbol a in column i"; word-major, rows padded with
//              zero words to a multiple of 64, words to a multiple of 16; bits past N are zero       invcov_planes_kernel
//   marginals  n_a(i) = sum_w popcount(P[w][i*K + a])                                    invcov_marginals_kernel
//   counts     n_ab(i,j) = sum_w popcount(P[w][i*K+a] & P[w][j*K+b]), int32, a band of columns i at a time    invcov_count_kernel
//   norm       the block in fp64, one-sided Jacobi, the upper triangle mirrored         invcov_norm_kernel
// The count kernel sees the planes as a bit matrix of R = L*K rows and computes R x R popcount inner products by word_tile.h's tile
// loop, 16 words per step (2 x 8 KB of LDS): a block owns 64 x 64 of them (64 / K alignment columns each way: the tile is counted in
// (column, symbol) rows, so any K in 1..16 runs the same code).  Tiles wholly below the diagonal are skipped unless the caller asked
// for the counts.
//
// Mutual information (rnamsm_msa_mi) runs the same stage 1 and replaces the norm by mi_pair_kernel, a per-pair fp64 sum over the
// integer table; its corrected map is apc.hip's rnamsm_apc_f64 of the map with a zero diagonal.
#include "invcov_stage1.h"
#include "word_tile.h"

namespace rnamsm {

// ---- which byte values occur ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void invcov_presence_kernel(const uint8_t* __restrict__ tok, int N, int L, int64_t ld,
                                                              uint32_t* __restrict__ present) {
    __shared__ uint32_t seen[256];
    seen[threadIdx.x] = 0;
    __syncthreads();
    for (int n = blockIdx.x; n < N; n += gridDim.x)
        for (int c = threadIdx.x; c < L; c += 256) seen[tok[(int64_t)n * ld + c]] = 1u;      // racing stores of the same value
    __syncthreads();
    if (seen[threadIdx.x]) present[threadIdx.x] = 1u;
}

// one block of 256: rank of every present non-gap byte among them = its symbol index
__global__ __launch_bounds__(256) void invcov_table_kernel(const uint32_t* __restrict__ present, int gap, uint8_t* __restrict__ lut,
                                                           int32_t* __restrict__ meta) {
    __shared__ int flag[256];
    const int b = threadIdx.x;
    flag[b] = (present[b] != 0u && b != gap) ? 1 : 0;
    if (b < IC_META) meta[b] = 0;
    __syncthreads();
    int rank = 0, total = 0;
    for (int q = 0; q < 256; ++q) {
        rank += q < b ? flag[q] : 0;
        total += flag[q];
    }
    lut[b] = (flag[b] && rank < IC_MAX_K) ? (uint8_t)rank : (uint8_t)0xFF;
    if (flag[b] && rank < IC_MAX_K) meta[1 + rank] = b;
    if (b == 0) meta[0] = total;
}

// ---- bit planes: block = word w (64 alignment rows) x 256 columns; lane = row, one ballot per symbol ---------------
constexpr int IP_COLS = 256, IP_PITCH = 260;         // pitch 65 dwords: a wave's 64 rows of one column hit 64 banks
__global__ __launch_bounds__(256) void invcov_planes_kernel(const uint8_t* __restrict__ tok, int N, int L, int64_t ld,
                                                            const uint8_t* __restrict__ lut, int K, int64_t Rp,
                                                            uint64_t* __restrict__ P) {
    __shared__ uint8_t sym[64 * IP_PITCH];
    __shared__ uint8_t slut[256];
    const int w = blockIdx.y, c0 = blockIdx.x * IP_COLS;
    slut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    for (int r = 0; r < 64; ++r) {
        const int64_t n = (int64_t)w * 64 + r;
        const int c = c0 + threadIdx.x;
        sym[r * IP_PITCH + threadIdx.x] = (n < N && c < L) ? slut[tok[n * ld + c]] : (uint8_t)0xFF;
    }
    __syncthreads();
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int c = wv; c < IP_COLS && c0 + c < L; c += 4) {        // wave-uniform
        const int s = sym[lane * IP_PITCH + c];
        uint64_t mine = 0;
        for (int a = 0; a < K; ++a) {
            const uint64_t m = __ballot(s == a);
            if (lane == a) mine = m;
        }
        if (lane < K) P[(int64_t)w * Rp + (int64_t)(c0 + c) * K + lane] = mine;
    }
}

__global__ __launch_bounds__(256) void invcov_marginals_kernel(const uint64_t* __restrict__ P, int W, int64_t Rp, int R,
                                                               int32_t* __restrict__ marg) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    int m = 0;
    for (int w = 0; w < W; ++w) m += __popcll(P[(int64_t)w * Rp + r]);
    marg[r] = m;
}

// ---- stage 1: pair counts ---------------------------------------------------------------------------------------------
// grid (column tiles, row tiles of the band).  row0: first (column, symbol) row of the band, a multiple of 64; rows_end: one
// past its last.  cnt: the band's counts, [i - i0][j][a][b].  Wp: words, a multiple of IC_WK.  Rp: padded rows, a multiple of 64.
__global__ __launch_bounds__(256) void invcov_count_kernel(const uint64_t* __restrict__ P, int Wp, int64_t Rp, int R, int K, int L,
                                                           int64_t row0, int64_t rows_end, int i0, int full,
                                                           int32_t* __restrict__ cnt) {
    __shared__ __attribute__((aligned(16))) uint64_t sA[IC_WK][IC_TILE];
    __shared__ __attribute__((aligned(16))) uint64_t sB[IC_WK][IC_TILE];
    const int64_t rb = row0 + (int64_t)blockIdx.y * IC_TILE, cb = (int64_t)blockIdx.x * IC_TILE;
    if (!full) {                                       // every pair of the tile has j < i: the norm reads the upper triangle only
        const int64_t last_c = cb + IC_TILE - 1 < R - 1 ? cb + IC_TILE - 1 : R - 1;
        if (last_c / K < rb / K) return;
    }
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    int c[4][4];
    word_tile_loop<IC_WK, false, AndPopcountOp>(P, Wp, Rp, rb, cb, nullptr, sA, sB, c);
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const int64_t r = rb + ty * 4 + x;
        if (r >= rows_end) continue;
        const int i = (int)(r / K), a = (int)(r - (int64_t)i * K);
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const int64_t col = cb + tx * 4 + y;
            if (col >= R) continue;
            const int j = (int)(col / K), b = (int)(col - (int64_t)j * K);
            cnt[(((int64_t)(i - i0) * L + j) * K + a) * K + b] = c[x][y];
        }
    }
}

// ---- stage 2: the covariance block and its spectral norm --------------------------------------------------------------------
// One thread per (i, j >= i).  B[a][b] = ((double)n_ab - ((double)n_a * (double)n_b) / N) / (N - 1), in that order: the product is
// exact (N <= 2^20), then one division, one subtraction, one division (compiled without contraction).  The largest singular value
// by one-sided Jacobi (Hestenes) on the columns of B, held in LDS element-major ([a*K + b][thread]: conflict-free): cyclic sweeps
// over the column pairs, a pair is rotated while |<p, q>| > 2^-52 |p| |q|; it stops after a sweep without a rotation, or after
// IC_SWEEPS.  A zero block rotates nothing and gives exactly 0; no finite block gives NaN (the rotation divides by 2 <p, q> != 0
// only, and an overflowing cotangent gives t = 0).  ||B(j,i)|| = ||B(i,j)^T|| = ||B(i,j)||: the value is written to both places.
constexpr int IC_SWEEPS = 40;
__global__ __launch_bounds__(256) void invcov_norm_kernel(const int32_t* __restrict__ cnt, const int32_t* __restrict__ marg, int N,
                                                          int L, int K, int i0, int i1, double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int T = blockDim.x, t = threadIdx.x;
    const int j = blockIdx.x * T + t, i = i0 + blockIdx.y;
    if (i >= i1 || j >= L || j < i) return;                       // (no barrier below: a thread's matrix is its own)
    double* B = sm + t;
    const int32_t* cb = cnt + ((int64_t)(i - i0) * L + j) * K * K;
    const double dn = (double)N, dn1 = (double)(N - 1);
    for (int a = 0; a < K; ++a) {
        const double na = (double)marg[i * K + a];
        for (int b = 0; b < K; ++b) {
            const double nb = (double)marg[j * K + b];
            const double prod = na * nb;
            const double mean = prod / dn;
            const double diff = (double)cb[a * K + b] - mean;
            B[(a * K + b) * T] = diff / dn1;
        }
    }
    for (int sweep = 0; sweep < IC_SWEEPS; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < K - 1; ++p)
            for (int q = p + 1; q < K; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int k = 0; k < K; ++k) {
                    const double x = B[(k * K + p) * T], y = B[(k * K + q) * T];
                    alpha += x * x;
                    beta += y * y;
                    gamma += x * y;
                }
                if (!(fabs(gamma) > 2.220446049250313e-16 * sqrt(alpha * beta))) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
                for (int k = 0; k < K; ++k) {
                    const double x = B[(k * K + p) * T], y = B[(k * K + q) * T];
                    B[(k * K + p) * T] = cs * x - sn * y;
                    B[(k * K + q) * T] = sn * x + cs * y;
                }
            }
        if (!rotated) break;
    }
    double best = 0.0;
    for (int p = 0; p < K; ++p) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) {
            const double x = B[(k * K + p) * T];
            s += x * x;
        }
        best = s > best ? s : best;
    }
    const double v = sqrt(best);
    out[(int64_t)i * L + j] = v;
    out[(int64_t)j * L + i] = v;
}

// (InvcovWs, Stage1 and the constants: invcov_stage1.h)
InvcovWs invcov_ws(int N, int L, int K) {
    InvcovWs w;
    w.W = (N + 63) / 64;
    w.Wp = (w.W + IC_WK - 1) / IC_WK * IC_WK;
    w.Rp = ((int64_t)L * K + IC_TILE - 1) / IC_TILE * IC_TILE;
    size_t off = 0;
    w.present = off; off += 256 * 4;
    w.lut = off;     off += 256;
    w.meta = off;    off += IC_META * 4;
    w.marg = off;    off += (((size_t)L * IC_MAX_K * 4) + 255) & ~(size_t)255;
    off = (off + 255) & ~(size_t)255;
    w.planes = off;  off += (size_t)w.Wp * (size_t)w.Rp * 8;
    off = (off + 255) & ~(size_t)255;
    const size_t whole = (size_t)L * L * IC_MAX_K * IC_MAX_K * 4;
    w.band = off;    off += whole < IC_BAND_BYTES ? whole : IC_BAND_BYTES;
    w.total = off;
    return w;
}

// ---- stage 1 as its entry points (rnamsm_msa_invcov, rnamsm_msa_mi, msa_wmi.hip's rnamsm_msa_wmi) run it ----------------------------
// `who` is the entry point's name in every message.
int stage1_check(const char* who, bool pointers, int N, int L, int64_t ld, int gap) {
    RNAMSM_CHECK_ARG(pointers, "%s: null pointer", who);
    RNAMSM_CHECK_ARG(N >= 2 && N <= IC_MAX_N, "%s: N=%d outside [2, %d]", who, N, IC_MAX_N);
    RNAMSM_CHECK_ARG(L >= 1 && L <= RNAMSM_LONG_MAX_L, "%s: L=%d outside [1, %d]", who, L, RNAMSM_LONG_MAX_L);
    RNAMSM_CHECK_ARG(ld >= L, "%s: ld=%lld is smaller than L=%d", who, (long long)ld, L);
    RNAMSM_CHECK_ARG(gap >= 0 && gap <= 255, "%s: gap=%d is not a byte value", who, gap);
    return RNAMSM_OK;
}

// presence, table (the one wait for the stream: K is read back, and a caller's verdict with it), planes, marginals
int stage1_planes(const char* who, const uint8_t* tokens, int N, int L, int64_t ld, int gap, char* ws, hipStream_t s, Stage1* st,
                  Stage1Verdict* verdict) {
    const InvcovWs full_ws = invcov_ws(N, L, IC_MAX_K);
    uint32_t* present = reinterpret_cast<uint32_t*>(ws + full_ws.present);
    uint8_t* lut = reinterpret_cast<uint8_t*>(ws + full_ws.lut);
    st->meta = reinterpret_cast<int32_t*>(ws + full_ws.meta);
    st->marg = reinterpret_cast<int32_t*>(ws + full_ws.marg);
    st->band = reinterpret_cast<int32_t*>(ws + full_ws.band);

    // ---- the symbols that occur: the one place where the host waits for the stream (K decides the layout and two refusals)
    if (hipMemsetAsync(present, 0, 256 * 4, s) != hipSuccess) return fail(RNAMSM_ERR_HIP, "%s: hipMemsetAsync failed", who);
    hipLaunchKernelGGL(invcov_presence_kernel, dim3(N < 2048 ? N : 2048), dim3(256), 0, s, tokens, N, L, ld, present);
    hipLaunchKernelGGL(invcov_table_kernel, dim3(1), dim3(256), 0, s, present, gap, lut, st->meta);
    RNAMSM_CHECK_LAUNCH(who);
    int32_t host_meta[IC_META];
    if (hipMemcpyAsync(host_meta, st->meta, sizeof(host_meta), hipMemcpyDeviceToHost, s) != hipSuccess ||
        (verdict && hipMemcpyAsync(&verdict->host, verdict->dev, 4, hipMemcpyDeviceToHost, s) != hipSuccess) ||
        hipStreamSynchronize(s) != hipSuccess)
        return fail(RNAMSM_ERR_HIP, "%s: reading the symbol table back failed: %s", who, hipGetErrorString(hipGetLastError()));
    const int K = host_meta[0];
    RNAMSM_CHECK_ARG(K >= 1, "%s: the alignment holds nothing but the gap value %d (K = 0)", who, gap);
    RNAMSM_CHECK_ARG(K <= IC_MAX_K, "%s: %d distinct non-gap values, more than %d", who, K, IC_MAX_K);

    st->w = invcov_ws(N, L, K);                          // (every offset up to the planes is independent of K)
    st->K = K;
    st->R = L * K;
    st->P = reinterpret_cast<uint64_t*>(ws + st->w.planes);
    if (hipMemsetAsync(st->P, 0, (size_t)st->w.Wp * (size_t)st->w.Rp * 8, s) != hipSuccess)
        return fail(RNAMSM_ERR_HIP, "%s: hipMemsetAsync failed", who);
    hipLaunchKernelGGL(invcov_planes_kernel, dim3((L + IP_COLS - 1) / IP_COLS, st->w.W), dim3(256), 0, s, tokens, N, L, ld, lut, K,
                       st->w.Rp, st->P);
    hipLaunchKernelGGL(invcov_marginals_kernel, dim3((st->R + 255) / 256), dim3(256), 0, s, st->P, st->w.W, st->w.Rp, st->R, st->marg);
    return RNAMSM_OK;
}

// columns i per band of counts held in the workspace: all of them, or a multiple of 64 (tile-aligned rows)
int stage1_band(int L, int K) {
    const size_t per_col = (size_t)L * K * K * 4;
    return per_col * L > IC_BAND_BYTES ? (int)(IC_BAND_BYTES / per_col / 64) * 64 : L;      // >= 64: per_col <= 2^22
}

// the counts of columns [i0, i1) into cnt as [i - i0][j][a][b]; full = 0: tiles wholly below the diagonal are left out
void stage1_count(const Stage1& st, int L, int i0, int i1, int full, int32_t* cnt, hipStream_t s) {
    const int64_t row0 = (int64_t)i0 * st.K, rows_end = (int64_t)i1 * st.K;
    hipLaunchKernelGGL(invcov_count_kernel, dim3((unsigned)(st.w.Rp / IC_TILE), (unsigned)((rows_end - row0 + IC_TILE - 1) / IC_TILE)),
                       dim3(256), 0, s, st.P, st.w.Wp, st.w.Rp, st.R, st.K, L, row0, rows_end, i0, full, cnt);
}

// ---- mutual information of a band of counts ------------------------------------------------------------------------------------------
// One thread per (i, j >= i), the counterpart of invcov_norm_kernel.  The pair's integer table c[a][b] over the K symbols is its
// K x K block of counts; MODE 1 ("state") adds the gap as state K, from the marginals in integers: c[a][K] = n_a(i) - sum_b n_ab,
// c[K][b] = n_b(j) - sum_a n_ab, c[K][K] = N - the rest, so n = N, r_a = n_a(i), s_b = n_b(j).  MODE 0 ("pairwise") leaves the rows with
// a gap in either column out: n, r_a, s_b are the block's own sums (s_b is kept in LDS, element-major [b][thread]: conflict-free, and
// a thread reads only what it wrote, so there is no barrier).
//   mi = sum over a then b ascending, the entries with c > 0 only, of ((double)c / (double)n) * log((double)(c * n) / (double)(r_a * s_b))
// both products exact in int64 (below 2^40), one division each, no contraction.  n = 0 gives 0.  The value goes to (i, j) and (j, i).
__device__ __forceinline__ double mi_term(int c, int64_t n, double dn, int r, int s) {
    const double ratio = (double)((int64_t)c * n) / (double)((int64_t)r * (int64_t)s);
    const double w = (double)c / dn;
    return w * log(ratio);
}

template <int MODE>
__global__ __launch_bounds__(256) void mi_pair_kernel(const int32_t* __restrict__ cnt, const int32_t* __restrict__ marg, int N, int L,
                                                      int K, int i0, int i1, double* __restrict__ mi) {
    __shared__ int s_col[MODE == 0 ? IC_MAX_K * 256 : 1];
    const int t = threadIdx.x;
    const int j = blockIdx.x * 256 + t, i = i0 + blockIdx.y;
    if (i >= i1 || j >= L || j < i) return;                       // (no barrier below)
    const int32_t* cb = cnt + ((int64_t)(i - i0) * L + j) * K * K;
    const int32_t* mi_i = marg + (int64_t)i * K;
    const int32_t* mj = marg + (int64_t)j * K;
    int64_t n = N;
    if (MODE == 0) {
        n = 0;
        for (int b = 0; b < K; ++b) {
            int s = 0;
            for (int a = 0; a < K; ++a) s += cb[a * K + b];
            s_col[b * 256 + t] = s;
            n += s;
        }
    }
    double sum = 0.0;
    if (n > 0) {
        const double dn = (double)n;
        int all = 0, gaps_i = N, gaps_j = N;                      // MODE 1: sum of the block, rows with a gap in column i, in column j
        if (MODE == 1)
            for (int b = 0; b < K; ++b) gaps_j -= mj[b];
        for (int a = 0; a < K; ++a) {
            int row = 0;
            for (int b = 0; b < K; ++b) row += cb[a * K + b];
            const int r = MODE == 1 ? mi_i[a] : row;
            for (int b = 0; b < K; ++b) {
                const int c = cb[a * K + b];
                if (c > 0) sum += mi_term(c, n, dn, r, MODE == 1 ? mj[b] : s_col[b * 256 + t]);
            }
            if (MODE == 1) {
                const int c = r - row;                            // symbol a in column i, a gap in column j
                if (c > 0) sum += mi_term(c, n, dn, r, gaps_j);
                all += row;
                gaps_i -= r;
            }
        }
        if (MODE == 1) {
            for (int b = 0; b < K; ++b) {
                int col = 0;
                for (int a = 0; a < K; ++a) col += cb[a * K + b];
                const int c = mj[b] - col;                        // a gap in column i, symbol b in column j
                if (c > 0) sum += mi_term(c, n, dn, gaps_i, mj[b]);
            }
            const int c = gaps_i - ((N - gaps_j) - all);          // a gap in both: N - the rest
            if (c > 0) sum += mi_term(c, n, dn, gaps_i, gaps_j);
        }
    }
    mi[(int64_t)i * L + j] = sum;
    mi[(int64_t)j * L + i] = sum;
}

struct MiWs {
    size_t map, apc, total;          // behind stage 1's bytes, which start at 0
};
static MiWs mi_ws(int N, int L) {
    MiWs w;
    w.map = (invcov_ws(N, L, IC_MAX_K).total + 255) & ~(size_t)255;                  // mi where the caller wants mip alone
    w.apc = w.map + ((((size_t)L * L * 8) + 255) & ~(size_t)255);
    w.total = w.apc + rnamsm_apc_f64_workspace_bytes(L);
    return w;
}

}  // namespace rnamsm

using namespace rnamsm;

extern "C" size_t rnamsm_msa_invcov_workspace_bytes(int N, int L) {
    if (N < 2 || N > IC_MAX_N || L < 1 || L > RNAMSM_LONG_MAX_L) return 0;
    return invcov_ws(N, L, IC_MAX_K).total;
}

extern "C" int rnamsm_msa_invcov(const uint8_t* tokens, int N, int L, int64_t ld, int gap, double* out, int32_t* counts,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = stage1_check("msa_invcov", tokens && out && workspace, N, L, ld, gap)) return rc;
    RNAMSM_CHECK_ARG(workspace_bytes >= invcov_ws(N, L, IC_MAX_K).total && (reinterpret_cast<uintptr_t>(workspace) & 255u) == 0,
                     "msa_invcov: workspace too small or misaligned (256 bytes)");
    RNAMSM_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 7u) == 0 && (reinterpret_cast<uintptr_t>(counts) & 3u) == 0,
                     "msa_invcov: out / counts misaligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Stage1 st;
    if (int rc = stage1_planes("msa_invcov", tokens, N, L, ld, gap, static_cast<char*>(workspace), s, &st)) return rc;
    const int K = st.K;
    int32_t* body = st.band;
    int band = L;
    if (counts) {
        if (hipMemcpyAsync(counts, st.meta, IC_META * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(RNAMSM_ERR_HIP, "msa_invcov: hipMemcpyAsync failed");
        body = counts + IC_META;
    } else {
        band = stage1_band(L, K);
    }
    const int T = K <= 4 ? 256 : (K <= 8 ? 64 : 32);     // K^2 doubles per thread in LDS: at most 64 KB a block
    for (int i0 = 0; i0 < L; i0 += band) {
        const int i1 = i0 + band < L ? i0 + band : L;
        int32_t* cnt = counts ? body + (int64_t)i0 * L * K * K : body;
        stage1_count(st, L, i0, i1, counts ? 1 : 0, cnt, s);
        hipLaunchKernelGGL(invcov_norm_kernel, dim3((L + T - 1) / T, i1 - i0), dim3(T), (size_t)K * K * T * 8, s, cnt, st.marg, N, L, K,
                           i0, i1, out);
    }
    RNAMSM_CHECK_LAUNCH("msa_invcov");
    return RNAMSM_OK;
}

extern "C" size_t rnamsm_msa_mi_workspace_bytes(int N, int L) {
    if (N < 2 || N > IC_MAX_N || L < 1 || L > RNAMSM_LONG_MAX_L) return 0;
    return mi_ws(N, L).total;
}

extern "C" int rnamsm_msa_mi(const uint8_t* tokens, int N, int L, int64_t ld, int gap, int gap_mode, double* mi, double* mip,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = stage1_check("msa_mi", tokens && workspace, N, L, ld, gap)) return rc;
    RNAMSM_CHECK_ARG(gap_mode == RNAMSM_MI_GAPS_PAIRWISE || gap_mode == RNAMSM_MI_GAPS_STATE,
                     "msa_mi: gap_mode=%d is not 0 (pairwise) or 1 (state)", gap_mode);
    RNAMSM_CHECK_ARG(mi || mip, "msa_mi: mi and mip are both NULL: nothing to compute");
    const MiWs mw = mi_ws(N, L);
    RNAMSM_CHECK_ARG(workspace_bytes >= mw.total, "msa_mi: workspace of %zu bytes is smaller than the %zu that N=%d, L=%d need",
                     workspace_bytes, mw.total, N, L);
    RNAMSM_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "msa_mi: workspace misaligned (256 bytes)");
    RNAMSM_CHECK_ARG((reinterpret_cast<uintptr_t>(mi) & 7u) == 0 && (reinterpret_cast<uintptr_t>(mip) & 7u) == 0 && (!mi || mi != mip),
                     "msa_mi: mi / mip misaligned, or one buffer for both");
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    Stage1 st;
    if (int rc = stage1_planes("msa_mi", tokens, N, L, ld, gap, ws, s, &st)) return rc;
    double* map = mi ? mi : reinterpret_cast<double*>(ws + mw.map);
    const int band = stage1_band(L, st.K);
    for (int i0 = 0; i0 < L; i0 += band) {
        const int i1 = i0 + band < L ? i0 + band : L;
        stage1_count(st, L, i0, i1, 0, st.band, s);
        const dim3 grid((L + 255) / 256, i1 - i0);
        if (gap_mode == RNAMSM_MI_GAPS_STATE)
            hipLaunchKernelGGL(mi_pair_kernel<1>, grid, dim3(256), 0, s, st.band, st.marg, N, L, st.K, i0, i1, map);
        else
            hipLaunchKernelGGL(mi_pair_kernel<0>, grid, dim3(256), 0, s, st.band, st.marg, N, L, st.K, i0, i1, map);
    }
    RNAMSM_CHECK_LAUNCH("msa_mi");
    if (!mip) return RNAMSM_OK;
    return rnamsm_apc_f64(map, L, L, 1, mip, ws + mw.apc, mw.total - mw.apc, stream);      // mip = apc(mi with a zero diagonal)
}
