// Alignment statistics on the device, built on the pairwise Hamming matrix (utils/align.py): MSA.pdist (:121-126), MSA.weights /
// MSA.neff (:250-269) and the coverage property (:242-247).  Everything rests on one exact quantity,
//   m(i, j) = the number of columns in which rows i and j differ                                   int32,
// and the reference's float64 forms of it: dist = (double)m / (double)L (scipy's pdist "hamming"), a neighbour is a row with
// (double)m / (double)L < seqid_cutoff (strict; the row itself has m = 0 and counts unless the cutoff is 0), weights = 1 / neighbours,
// Neff = the weights' sum.
//
// Data flow (all on the caller's stream; every buffer in the caller's workspace):
//   pack    P[w][i] = the bytes of columns 8w .. 8w + 7 of row i as one 64-bit word (msa_words.h with gap = 0: the bytes as they
//           are, zero past L), word-major; rows padded with zero words to a multiple of 64, words to a multiple of 8
//                                                                                                  word_tile.h: words_pack_kernel
//   pairs   m(i, j) = sum_w nonzero_bytes(P[w][i] ^ P[w][j]) by word_tile.h's tile loop, 8 words per step (2 x 4 KB of LDS).  Only
//           tiles on or above the diagonal run.                                                               pdist_pair_kernel
//   the kernel has two epilogues (a template parameter):
//   matrix       the tile goes through LDS and is written twice, as it is and transposed: rows of 64 consecutive elements either
//                way, and the lower triangle is a copy of the upper -- exactly symmetric, the diagonal exactly 0 (x ^ x = 0)
//   neighbours   the tile is thresholded; its row sums are the hits of its 64 rows against its column block, its column sums the
//                hits of its 64 columns against its row block (an off-diagonal tile feeds both).  Each goes to its own int32 slot
//                of a partial table, one slot per (row, block), written exactly once; pdist_reduce_kernel adds a row's slots up.
//                The N x N matrix never exists on this route.
//   a band is a run of row blocks whose partial table fits the workspace the caller gave: the pair kernel and the reduction run once
//   per band and the per-row totals accumulate in int32 -- integer sums, so any band count gives the same bits.
//   finish  n_neighbors and weights[i] = 1.0 / (double)n_neighbors[i]                                       pdist_finish_kernel
//           neff in ONE order: a block of 1024 threads, thread t adds the weights of rows t, t + 1024, ... in ascending order from
//           0.0, then the 1024 sums are folded in halves (s[t] += s[t + 512], then + 256, ..., + 1)         pdist_neff_kernel
//   coverage[c] = (double)#{rows with msa[r][c] != gap} / (double)N: 64 columns x 16 row lanes a block, integer counts, the 16
//           lanes' counts added in LDS, one division                                                         msa_coverage_kernel
#include "word_tile.h"

namespace rnamsm {

constexpr int PD_TILE = WT_TILE;   // rows of a pair tile, each way
constexpr int PD_WK = 8;           // words staged per step
constexpr int PD_PITCH = PD_TILE + 1;
constexpr int PD_MAX_L = 32768;
constexpr int PD_MAX_N_MATRIX = 16384;
constexpr int PD_MAX_N = 1 << 20;
constexpr size_t PD_PARTIAL_BYTES = (size_t)1 << 28;       // the partial table of the default workspace: at most 256 MB

// P[w][p] = the recoded word (msa_words.h: pack_word) of columns 8w .. 8w + 7 of row order[p] -- of row p without an order; gap = 0:
// the bytes as they are.  A position past N, or an order entry outside [0, N), packs as a row of zero words and reads nothing.  One
// thread per (position, word), the words of a position on neighbouring threads.
__global__ __launch_bounds__(256) void words_pack_kernel(const uint8_t* __restrict__ msa, int N, int L, int64_t ld, int gap,
                                                         const int32_t* __restrict__ order, int Wp, int64_t Np, uint64_t* __restrict__ P) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= Np * Wp) return;
    const int64_t pos = idx / Wp;
    const int w = (int)(idx - pos * Wp);
    int64_t row = -1;
    if (pos < N) row = order ? (int64_t)order[pos] : pos;
    P[(int64_t)w * Np + pos] = (row >= 0 && row < N) ? pack_word(msa + row * ld, 8 * w, L - 8 * w, gap) : 0ull;
}
void words_pack(const uint8_t* msa, int N, int L, int64_t ld, int gap, const int32_t* order, int Wp, int64_t Np, uint64_t* P, hipStream_t s) {
    hipLaunchKernelGGL(words_pack_kernel, dim3((unsigned)((Np * Wp + 255) / 256)), dim3(256), 0, s, msa, N, L, ld, gap, order, Wp, Np, P);
}

// MODE 0: the matrix (counts and / or dist, [N, N]).  MODE 1: the neighbour partials of the band of row blocks b0 .. b0 + nb - 1:
//   pr[t][r]  hits of the band's row r (row b0 * 64 + r of the alignment) against row block t, for t >= the row's own block
//   pc[k][j]  hits of row j against row block b0 + k, for j in a block behind b0 + k
// grid (column blocks from b0 on, row blocks of the band); a tile below the diagonal returns at once.
template <int MODE>
__global__ __launch_bounds__(256) void pdist_pair_kernel(const uint64_t* __restrict__ P, int Wp, int64_t Np, int N, int L, int b0, int nb,
                                                         int32_t* __restrict__ counts, double* __restrict__ dist, double cutoff,
                                                         int32_t* __restrict__ pr, int32_t* __restrict__ pc) {
    // the staged words (2 x PD_WK x 64 x 8 bytes) and, after the loop, the tile as int32 [64][65]
    __shared__ __attribute__((aligned(16))) unsigned char raw[PD_TILE * PD_PITCH * 4];
    static_assert(sizeof(raw) >= 2 * PD_WK * PD_TILE * 8, "the word panels fit the tile's bytes");
    uint64_t(*sA)[PD_TILE] = reinterpret_cast<uint64_t(*)[PD_TILE]>(raw);
    uint64_t(*sB)[PD_TILE] = sA + PD_WK;
    int32_t(*tile)[PD_PITCH] = reinterpret_cast<int32_t(*)[PD_PITCH]>(raw);
    const int bi = b0 + (int)blockIdx.y, bj = b0 + (int)blockIdx.x;
    if (bj < bi) return;
    const int64_t rb = (int64_t)bi * PD_TILE, cb = (int64_t)bj * PD_TILE;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    int c[4][4];
    word_tile_loop<PD_WK, false, MismatchOp>(P, Wp, Np, rb, cb, nullptr, sA, sB, c);

    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (MODE == 0) {
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) tile[ty * 4 + x][tx * 4 + y] = c[x][y];
        __syncthreads();
        const double dl = (double)L;
#pragma unroll 2
        for (int r = wv; r < PD_TILE; r += 4) {
            const int64_t i = rb + r, j = cb + lane;
            if (i < N && j < N) {
                const int m = tile[r][lane];
                if (counts) counts[i * N + j] = m;
                if (dist) dist[i * N + j] = (double)m / dl;
            }
        }
        if (bi != bj)                                           // the mirror image: row cb + r, columns rb .. rb + 63
#pragma unroll 2
            for (int r = wv; r < PD_TILE; r += 4) {
                const int64_t i = cb + r, j = rb + lane;
                if (i < N && j < N) {
                    const int m = tile[lane][r];
                    if (counts) counts[i * N + j] = m;
                    if (dist) dist[i * N + j] = (double)m / dl;
                }
            }
    } else {
        const double dl = (double)L;
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) {
                const bool real = rb + ty * 4 + x < N && cb + tx * 4 + y < N;
                tile[ty * 4 + x][tx * 4 + y] = (real && (double)c[x][y] / dl < cutoff) ? 1 : 0;
            }
        __syncthreads();
        const int t = threadIdx.x;
        if (t < PD_TILE) {
            int s = 0;
            for (int k = 0; k < PD_TILE; ++k) s += tile[t][k];
            pr[(int64_t)bj * ((int64_t)nb * PD_TILE) + (rb - (int64_t)b0 * PD_TILE) + t] = s;
        } else if (t < 2 * PD_TILE && bi != bj) {
            const int q = t - PD_TILE;
            int s = 0;
            for (int k = 0; k < PD_TILE; ++k) s += tile[k][q];
            pc[(int64_t)(bi - b0) * Np + cb + q] = s;
        }
    }
}

// one thread per (padded) row: the band's slots of the row, in ascending block order; first: the band that starts the totals
__global__ __launch_bounds__(256) void pdist_reduce_kernel(const int32_t* __restrict__ pr, const int32_t* __restrict__ pc, int64_t Np, int T,
                                                           int b0, int nb, int first, int32_t* __restrict__ acc) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= Np) return;
    const int bj = (int)(j / PD_TILE);
    int add = 0;
    for (int k = 0; k < nb && b0 + k < bj; ++k) add += pc[(int64_t)k * Np + j];
    if (bj >= b0 && bj < b0 + nb) {
        const int64_t rows = (int64_t)nb * PD_TILE, r = j - (int64_t)b0 * PD_TILE;
        for (int t = bj; t < T; ++t) add += pr[(int64_t)t * rows + r];
    }
    acc[j] = (first ? 0 : acc[j]) + add;
}

__global__ __launch_bounds__(256) void pdist_finish_kernel(const int32_t* __restrict__ acc, int N, int32_t* __restrict__ n_neighbors,
                                                           double* __restrict__ weights) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int n = acc[i];
    if (n_neighbors) n_neighbors[i] = n;
    if (weights) weights[i] = 1.0 / (double)n;
}

// one block of 1024; the order of the additions is stated at the top of this file
__global__ __launch_bounds__(1024) void pdist_neff_kernel(const int32_t* __restrict__ acc, int N, double* __restrict__ neff) {
    __shared__ double s[1024];
    double mine = 0.0;
    for (int i = threadIdx.x; i < N; i += 1024) mine += 1.0 / (double)acc[i];
    s[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *neff = s[0];
}

// block = 64 columns x 16 row lanes
__global__ __launch_bounds__(1024) void msa_coverage_kernel(const uint8_t* __restrict__ msa, int N, int L, int64_t ld, int gap,
                                                            double* __restrict__ coverage) {
    __shared__ int part[16][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + cl;
    int n = 0;
    if (col < L)
        for (int r = rl; r < N; r += 16) n += msa[(int64_t)r * ld + col] != gap;
    part[rl][cl] = n;
    __syncthreads();
    if (rl == 0 && col < L) {
        int total = 0;
        for (int q = 0; q < 16; ++q) total += part[q][cl];
        coverage[col] = (double)total / (double)N;
    }
}

struct PdistWs {
    size_t pack, acc, partial, fixed;      // offsets; fixed = the bytes in front of the partial table
    size_t per_block;                      // bytes of the partial table per row block of a band
    int T, Wp;
    int64_t Np;
};
static PdistWs pdist_ws(int N, int L) {
    PdistWs w;
    const WordDims d = word_dims(N, L, PD_WK);
    w.Np = d.Np;
    w.Wp = d.Wp;
    w.T = (int)(d.Np / PD_TILE);
    w.pack = 0;
    w.acc = (size_t)w.Wp * (size_t)w.Np * 8;                  // (a multiple of 256: Np * 8 is one of 512)
    w.partial = w.fixed = w.acc + (size_t)w.Np * 4;
    w.per_block = (size_t)w.Np * 8;                           // pr and pc: 64 * T and Np int32 each
    return w;
}
static bool pdist_shape_ok(int N, int L, int max_n) { return N >= 1 && N <= max_n && L >= 1 && L <= PD_MAX_L; }

}  // namespace rnamsm

using namespace rnamsm;

extern "C" size_t rnamsm_msa_pdist_workspace_bytes(int N, int L) {
    if (!pdist_shape_ok(N, L, PD_MAX_N_MATRIX)) return 0;
    return pdist_ws(N, L).acc;
}

extern "C" int rnamsm_msa_pdist(const uint8_t* msa, int N, int L, int64_t ld, int32_t* counts, double* dist, void* workspace,
                                size_t workspace_bytes, void* stream) {
    RNAMSM_CHECK_ARG(msa && workspace, "msa_pdist: null pointer");
    RNAMSM_CHECK_ARG(N >= 1 && N <= PD_MAX_N_MATRIX, "msa_pdist: N=%d outside [1, %d]", N, PD_MAX_N_MATRIX);
    RNAMSM_CHECK_ARG(L >= 1 && L <= PD_MAX_L, "msa_pdist: L=%d outside [1, %d]", L, PD_MAX_L);
    RNAMSM_CHECK_ARG(ld >= L, "msa_pdist: ld=%lld is smaller than L=%d", (long long)ld, L);
    RNAMSM_CHECK_ARG(counts || dist, "msa_pdist: counts and dist are both null: nothing to write");
    const PdistWs w = pdist_ws(N, L);
    RNAMSM_CHECK_ARG(workspace_bytes >= w.acc && (reinterpret_cast<uintptr_t>(workspace) & 255u) == 0,
                     "msa_pdist: workspace of %zu bytes too small (%zu) or misaligned (256 bytes)", workspace_bytes, w.acc);
    RNAMSM_CHECK_ARG((reinterpret_cast<uintptr_t>(dist) & 7u) == 0 && (reinterpret_cast<uintptr_t>(counts) & 3u) == 0,
                     "msa_pdist: counts / dist misaligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint64_t* P = reinterpret_cast<uint64_t*>(workspace);
    words_pack(msa, N, L, ld, 0, nullptr, w.Wp, w.Np, P, s);
    hipLaunchKernelGGL(pdist_pair_kernel<0>, dim3(w.T, w.T), dim3(256), 0, s, P, w.Wp, w.Np, N, L, 0, w.T, counts, dist, 0.0,
                       (int32_t*)nullptr, (int32_t*)nullptr);
    RNAMSM_CHECK_LAUNCH("msa_pdist");
    return RNAMSM_OK;
}

extern "C" size_t rnamsm_msa_neff_min_workspace_bytes(int N, int L) {
    if (!pdist_shape_ok(N, L, PD_MAX_N)) return 0;
    const PdistWs w = pdist_ws(N, L);
    return w.fixed + w.per_block;
}

extern "C" size_t rnamsm_msa_neff_workspace_bytes(int N, int L) {
    if (!pdist_shape_ok(N, L, PD_MAX_N)) return 0;
    const PdistWs w = pdist_ws(N, L);
    size_t nb = PD_PARTIAL_BYTES / w.per_block;
    nb = nb < 1 ? 1 : (nb > (size_t)w.T ? (size_t)w.T : nb);
    return w.fixed + nb * w.per_block;
}

extern "C" int rnamsm_msa_neff(const uint8_t* msa, int N, int L, int64_t ld, double seqid_cutoff, int32_t* n_neighbors, double* weights,
                               double* neff, void* workspace, size_t workspace_bytes, void* stream) {
    RNAMSM_CHECK_ARG(msa && workspace, "msa_neff: null pointer");
    RNAMSM_CHECK_ARG(N >= 1 && N <= PD_MAX_N, "msa_neff: N=%d outside [1, %d]", N, PD_MAX_N);
    RNAMSM_CHECK_ARG(L >= 1 && L <= PD_MAX_L, "msa_neff: L=%d outside [1, %d]", L, PD_MAX_L);
    RNAMSM_CHECK_ARG(ld >= L, "msa_neff: ld=%lld is smaller than L=%d", (long long)ld, L);
    RNAMSM_CHECK_ARG(seqid_cutoff >= 0.0 && seqid_cutoff <= 1.0, "msa_neff: seqid_cutoff=%g outside [0, 1]", seqid_cutoff);
    RNAMSM_CHECK_ARG(n_neighbors || weights || neff, "msa_neff: n_neighbors, weights and neff are all null: nothing to write");
    const PdistWs w = pdist_ws(N, L);
    const size_t need = w.fixed + w.per_block;
    RNAMSM_CHECK_ARG(workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 255u) == 0,
                     "msa_neff: workspace of %zu bytes too small (%zu at least) or misaligned (256 bytes)", workspace_bytes, need);
    RNAMSM_CHECK_ARG((reinterpret_cast<uintptr_t>(weights) & 7u) == 0 && (reinterpret_cast<uintptr_t>(neff) & 7u) == 0 &&
                         (reinterpret_cast<uintptr_t>(n_neighbors) & 3u) == 0,
                     "msa_neff: n_neighbors / weights / neff misaligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    uint64_t* P = reinterpret_cast<uint64_t*>(ws + w.pack);
    int32_t* acc = reinterpret_cast<int32_t*>(ws + w.acc);
    // the band: as many row blocks as the partial table has room for -- a function of workspace_bytes alone
    size_t room = (workspace_bytes - w.fixed) / w.per_block;
    const int band = room > (size_t)w.T ? w.T : (int)room;
    int32_t* pr = reinterpret_cast<int32_t*>(ws + w.partial);
    int32_t* pc = pr + (int64_t)band * w.Np;                   // pr: T x (band * 64) slots = band * Np
    words_pack(msa, N, L, ld, 0, nullptr, w.Wp, w.Np, P, s);
    for (int b0 = 0; b0 < w.T; b0 += band) {
        const int nb = b0 + band < w.T ? band : w.T - b0;
        hipLaunchKernelGGL(pdist_pair_kernel<1>, dim3(w.T - b0, nb), dim3(256), 0, s, P, w.Wp, w.Np, N, L, b0, nb, (int32_t*)nullptr,
                           (double*)nullptr, seqid_cutoff, pr, pc);
        hipLaunchKernelGGL(pdist_reduce_kernel, dim3((unsigned)((w.Np + 255) / 256)), dim3(256), 0, s, pr, pc, w.Np, w.T, b0, nb,
                           b0 == 0 ? 1 : 0, acc);
    }
    if (n_neighbors || weights)
        hipLaunchKernelGGL(pdist_finish_kernel, dim3((N + 255) / 256), dim3(256), 0, s, acc, N, n_neighbors, weights);
    if (neff) hipLaunchKernelGGL(pdist_neff_kernel, dim3(1), dim3(1024), 0, s, acc, N, neff);
    RNAMSM_CHECK_LAUNCH("msa_neff");
    return RNAMSM_OK;
}

extern "C" int rnamsm_msa_coverage(const uint8_t* msa, int N, int L, int64_t ld, int gap, double* coverage, void* stream) {
    RNAMSM_CHECK_ARG(msa && coverage, "msa_coverage: null pointer");
    RNAMSM_CHECK_ARG(N >= 1 && N <= PD_MAX_N, "msa_coverage: N=%d outside [1, %d]", N, PD_MAX_N);
    RNAMSM_CHECK_ARG(L >= 1 && L <= PD_MAX_L, "msa_coverage: L=%d outside [1, %d]", L, PD_MAX_L);
    RNAMSM_CHECK_ARG(ld >= L, "msa_coverage: ld=%lld is smaller than L=%d", (long long)ld, L);
    RNAMSM_CHECK_ARG(gap >= 0 && gap <= 255, "msa_coverage: gap=%d is not a byte value", gap);
    RNAMSM_CHECK_ARG((reinterpret_cast<uintptr_t>(coverage) & 7u) == 0, "msa_coverage: coverage misaligned");
    hipLaunchKernelGGL(msa_coverage_kernel, dim3((L + 63) / 64), dim3(1024), 0, static_cast<hipStream_t>(stream), msa, N, L, ld, gap,
                       coverage);
    RNAMSM_CHECK_LAUNCH("msa_coverage");
    return RNAMSM_OK;
}
