// The identity redundancy filter on the device: a row sub-sampling rule of this project's own, modelled on what the reference asks of
// the external hhfilter binary (`-id 90 -diff num_seqs`, utils/align.py:68-102, 165-173).  It is NOT that binary's algorithm: hhfilter's
// -diff counts sequences per window of 50 columns and has its own threshold schedule; this rule counts over the whole alignment.
//
// The rule, all in integers.  Per pair of rows, both = the columns where neither has the gap, same = those of them
// where the bytes are equal, nres(i) = both(i, i).  Row k is REDUNDANT to row j at threshold t iff both > 0 and 100 * same >= t * both.
// The rows are walked in `order`, one pass per threshold (msa_words.h: sq_thresholds): a row not kept yet is kept iff it is
// redundant to no kept row -- of an earlier pass, or earlier in this one; a row without residues is never kept unless it is the first
// of the order, which always is.  The walk stops after the first pass that leaves num_seqs rows kept (num_seqs > 0), or after the
// last threshold.
//
// Data flow (all on the caller's stream, every buffer in the caller's workspace).  Everything past the pack works on POSITIONS of
// the order, not on row indices: position p holds row order[p], so a chunk of the walk is a run of consecutive positions.
//   check    the lowest position whose order entry lies outside [0, N), or -1: one block, one slot          seqid_order_check_kernel
//   pack     P[w][p] = the recoded bytes of columns 8w .. 8w + 7 of row order[p] as a 64-bit word (msa_words.h), word-major, the
//            positions padded to a multiple of 64 and the words to a multiple of 8 with zero words; an entry outside [0, N) packs
//            as a row of gaps and reads nothing                                                 word_tile.h: words_pack_kernel
//   nres     per position, from its words; kept_at = -1; the kept count = 0                                  seqid_nres_kernel
//   then, per pass at threshold t and per chunk of `chunk` positions, two launches ordered by the stream:
//   cand     a block owns 64 positions of the chunk.  A CANDIDATE is a position not kept yet with residues (or position 0).  The
//            block walks the kept list 64 at a time -- the kept count is read from device memory, so it holds what earlier chunks of
//            this pass kept -- and accumulates both and same of its 64 x 64 pairs by word_tile.h's tile loop, 8 words per step, the
//            kept rows' words GATHERED through the kept list.  Each pair is thresholded, a candidate redundant to any kept row is
//            rejected; a block whose 64 positions are all rejected or no candidates stops walking.  rej[p] = 1 for a rejected
//            position or one that is no candidate, else 0: one slot per position, written once a launch      seqid_cand_kernel
//   resolve  one block per chunk.  The chunk's survivors (rej = 0) as bit masks; the predicate of every pair of the chunk whose
//            64 x 64 tile has survivors on both sides, on or above the diagonal, by the same tile loop, as a bit matrix in LDS
//            (chunk x chunk bits).  Then ONE WAVE walks the chunk in order: the lowest survivor still alive is kept -- appended
//            to the kept list, kept_at = t -- and every later survivor redundant to it is struck, lane l holding the alive bits
//            of positions 64 l .. 64 l + 63.  This kernel carries the rule's sequential dependence        seqid_resolve_kernel
//   The host reads the kept count back ONCE PER PASS (with the order's verdict after the first) to decide whether to stop; within
//   a pass nothing is read back.  A chunk's kept rows are exactly those the walk would keep row by row: a survivor is redundant to
//   no row kept before the chunk (cand) and to no row kept earlier in the chunk (resolve), so ANY chunk size gives the same list.
//   finish   the kept positions -> row flags and kept_at per row (each kept row written once), then the flags -> ascending
//            indices by a block-wide scan                          seqid_scatter_kernel, block_scan.h: compact_flags_kernel
// No atomics anywhere; integer sums in a fixed order; the same indices on every run.
#include "block_scan.h"
#include "word_tile.h"

namespace rnamsm {

constexpr int SQ_TILE = WT_TILE;     // positions of a pair tile, each way
constexpr int SQ_WK = 8;             // words staged per step
constexpr int SQ_MAX_L = 32768;
constexpr int SQ_MAX_N = 1 << 20;
constexpr int SQ_MAX_CHUNK = 512;    // the bit matrix of a chunk: 512 x 512 bits = 32 KB of LDS
constexpr int SQ_MAX_TILES = SQ_MAX_CHUNK / SQ_TILE;

// meta[0] = the kept count, meta[1] = the lowest position with an order entry outside [0, N), or -1
__global__ __launch_bounds__(1024) void seqid_order_check_kernel(const int32_t* __restrict__ order, int N, int32_t* __restrict__ meta) {
    const int bad = block_first_index(order ? N : 0, [&](int p) { return order[p] < 0 || order[p] >= N; });
    if (threadIdx.x == 0) meta[1] = bad;
}

// one thread per (padded) position
__global__ __launch_bounds__(256) void seqid_nres_kernel(const uint64_t* __restrict__ P, int Wp, int64_t Np, int32_t* __restrict__ nres,
                                                         int32_t* __restrict__ kept_at, int32_t* __restrict__ meta) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p == 0) meta[0] = 0;
    if (p >= Np) return;
    int n = 0;
    for (int w = 0; w < Wp; ++w) n += sq_residues(P[(int64_t)w * Np + p]);
    nres[p] = n;
    kept_at[p] = -1;
}

// grid = the 64-position tiles of the chunk that starts at position c0
__global__ __launch_bounds__(256) void seqid_cand_kernel(const uint64_t* __restrict__ P, int Wp, int64_t Np, int N, int64_t c0, int t,
                                                         const int32_t* __restrict__ nres, const int32_t* __restrict__ kept_at,
                                                         const int32_t* __restrict__ kept_pos, const int32_t* __restrict__ meta,
                                                         int32_t* __restrict__ rej) {
    __shared__ __attribute__((aligned(16))) uint64_t sA[SQ_WK][SQ_TILE];
    __shared__ __attribute__((aligned(16))) uint64_t sB[SQ_WK][SQ_TILE];
    __shared__ int s_rej[SQ_TILE];
    __shared__ int s_idx[SQ_TILE];
    const int64_t ra = c0 + (int64_t)blockIdx.x * SQ_TILE;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < SQ_TILE) {
        const int64_t p = ra + threadIdx.x;
        const bool cand = p < N && kept_at[p] < 0 && (nres[p] > 0 || p == 0);
        s_rej[threadIdx.x] = cand ? 0 : 1;
    }
    __syncthreads();
    const int nk = meta[0];
    const int ty = threadIdx.x >> 4;
    for (int k0 = 0; k0 < nk; k0 += SQ_TILE) {
        // (every wave reads the same 64 flags: the decision is uniform over the block)
        if (__ballot(s_rej[lane] != 0) == ~0ull) break;
        if (threadIdx.x < SQ_TILE) s_idx[threadIdx.x] = k0 + (int)threadIdx.x < nk ? kept_pos[k0 + threadIdx.x] : -1;
        __syncthreads();
        ResiduePairOp::Acc c[4][4];
        word_tile_loop<SQ_WK, true, ResiduePairOp>(P, Wp, Np, ra, 0, s_idx, sA, sB, c);
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            bool hit = false;
#pragma unroll
            for (int y = 0; y < 4; ++y) hit = hit || sq_redundant(c[x][y].both, c[x][y].same, t);
            if (hit) s_rej[ty * 4 + x] = 1;          // several threads may store the same 1
        }
        __syncthreads();
    }
    if (threadIdx.x < SQ_TILE) rej[ra + threadIdx.x] = s_rej[threadIdx.x];
}

// one block; the chunk = positions c0 .. c0 + 64 * tiles - 1 (tiles <= SQ_MAX_TILES)
__global__ __launch_bounds__(256) void seqid_resolve_kernel(const uint64_t* __restrict__ P, int Wp, int64_t Np, int64_t c0, int tiles, int t,
                                                            const int32_t* __restrict__ rej, int32_t* __restrict__ kept_at,
                                                            int32_t* __restrict__ kept_pos, int32_t* __restrict__ meta) {
    __shared__ __attribute__((aligned(16))) uint64_t sA[SQ_WK][SQ_TILE];
    __shared__ __attribute__((aligned(16))) uint64_t sB[SQ_WK][SQ_TILE];
    __shared__ uint64_t s_bits[SQ_MAX_CHUNK][SQ_MAX_TILES];      // s_bits[i][l]: bit q = position i of the chunk is redundant to 64 l + q
    __shared__ uint64_t s_surv[SQ_MAX_TILES];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int l = wv; l < tiles; l += 4) {
        const uint64_t m = __ballot(rej[c0 + (int64_t)l * SQ_TILE + lane] == 0);
        if (lane == 0) s_surv[l] = m;
    }
    __syncthreads();
    uint64_t any = 0;
    for (int l = 0; l < tiles; ++l) any |= s_surv[l];
    if (!any) return;

    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    for (int ti = 0; ti < tiles; ++ti) {
        if (!s_surv[ti]) continue;
        for (int tj = ti; tj < tiles; ++tj) {
            if (!s_surv[tj]) continue;
            ResiduePairOp::Acc c[4][4];
            word_tile_loop<SQ_WK, false, ResiduePairOp>(P, Wp, Np, c0 + (int64_t)ti * SQ_TILE, c0 + (int64_t)tj * SQ_TILE, nullptr, sA, sB, c);
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                uint32_t nib = 0;
#pragma unroll
                for (int y = 0; y < 4; ++y) nib |= sq_redundant(c[x][y].both, c[x][y].same, t) ? 1u << y : 0u;
                // the 16 threads of a row (neighbouring lanes) OR their nibbles into one 64-bit word, as two halves
                uint32_t lo = tx < 8 ? nib << (4 * tx) : 0u, hi = tx >= 8 ? nib << (4 * (tx - 8)) : 0u;
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) {
                    lo |= (uint32_t)__shfl_xor((int)lo, off, 64);
                    hi |= (uint32_t)__shfl_xor((int)hi, off, 64);
                }
                if (tx == 0) s_bits[ti * SQ_TILE + ty * 4 + x][tj] = ((uint64_t)hi << 32) | lo;
            }
        }
    }
    __syncthreads();
    if (wv != 0) return;

    // the walk: lane l holds the survivors of positions 64 l .. 64 l + 63 that are still alive
    uint64_t alive = lane < tiles ? s_surv[lane] : 0ull;
    int nk = meta[0];
    for (;;) {
        const uint64_t holders = __ballot(alive != 0);
        if (!holders) break;
        const int wl = __ffsll((unsigned long long)holders) - 1;
        const uint32_t alo = (uint32_t)__shfl((int)(uint32_t)alive, wl, 64), ahi = (uint32_t)__shfl((int)(uint32_t)(alive >> 32), wl, 64);
        const uint64_t aw = ((uint64_t)ahi << 32) | alo;
        const int b = __ffsll((unsigned long long)aw) - 1;
        const int i = wl * SQ_TILE + b;                           // the lowest survivor alive: kept
        if (lane == 0) {
            kept_pos[nk] = (int32_t)(c0 + i);
            kept_at[c0 + i] = t;
        }
        ++nk;
        // strike what is redundant to it; words below wl hold nothing alive, in word wl the row itself and everything before it goes
        uint64_t strike = (lane < tiles && lane >= wl) ? s_bits[i][lane] : 0ull;
        if (lane == wl) strike |= b == 63 ? ~0ull : ((2ull << b) - 1ull);
        alive &= ~strike;
    }
    if (lane == 0) meta[0] = nk;
}

// Finish.  flags / kept_at_out are per ROW: cleared for every row, then set from the kept list (a row is kept at most once, so every
// slot is written once).
__global__ __launch_bounds__(256) void seqid_clear_kernel(int N, int32_t* __restrict__ flags, int32_t* __restrict__ kept_at_out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    flags[r] = 0;
    if (kept_at_out) kept_at_out[r] = -1;
}
__global__ __launch_bounds__(256) void seqid_scatter_kernel(int nk, const int32_t* __restrict__ kept_pos, const int32_t* __restrict__ kept_at,
                                                            const int32_t* __restrict__ order, int32_t* __restrict__ flags,
                                                            int32_t* __restrict__ kept_at_out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nk) return;
    const int p = kept_pos[k];
    const int r = order ? order[p] : p;
    flags[r] = 1;
    if (kept_at_out) kept_at_out[r] = kept_at[p];
}
struct SeqidWs {
    size_t pack, nres, kept_at, kept_pos, rej, meta, total;      // offsets, each a multiple of 256
    int Wp;
    int64_t Np;
};
static SeqidWs seqid_ws(int N, int L) {
    SeqidWs w;
    const WordDims d = word_dims(N, L, SQ_WK);
    w.Np = d.Np;
    w.Wp = d.Wp;
    const size_t ints = (size_t)w.Np * 4;                         // (a multiple of 256: Np is one of 64)
    w.pack = 0;
    w.nres = (size_t)w.Wp * (size_t)w.Np * 8;
    w.kept_at = w.nres + ints;
    w.kept_pos = w.kept_at + ints;
    w.rej = w.kept_pos + ints;
    w.meta = w.rej + ints;
    w.total = w.meta + 256;
    return w;
}
static bool seqid_shape_ok(int N, int L) { return N >= 1 && N <= SQ_MAX_N && L >= 1 && L <= SQ_MAX_L; }

}  // namespace rnamsm

using namespace rnamsm;

extern "C" size_t rnamsm_seqid_filter_workspace_bytes(int N, int L) {
    if (!seqid_shape_ok(N, L)) return 0;
    return seqid_ws(N, L).total;
}

extern "C" int rnamsm_seqid_filter(const uint8_t* msa, int N, int L, int64_t ld, int gap, const int32_t* order, int num_seqs,
                                   int min_seqid, int max_seqid, int step, int32_t* kept_indices, int32_t* kept_at, int* n_kept,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    RNAMSM_CHECK_ARG(msa && kept_indices && n_kept && workspace, "seqid_filter: null pointer");
    RNAMSM_CHECK_ARG(N >= 1 && N <= SQ_MAX_N, "seqid_filter: N=%d outside [1, %d]", N, SQ_MAX_N);
    RNAMSM_CHECK_ARG(L >= 1 && L <= SQ_MAX_L, "seqid_filter: L=%d outside [1, %d]", L, SQ_MAX_L);
    RNAMSM_CHECK_ARG(ld >= L, "seqid_filter: ld=%lld is smaller than L=%d", (long long)ld, L);
    RNAMSM_CHECK_ARG(gap >= 0 && gap <= 255, "seqid_filter: gap=%d is not a byte value", gap);
    RNAMSM_CHECK_ARG(num_seqs >= 0, "seqid_filter: num_seqs=%d is negative", num_seqs);
    RNAMSM_CHECK_ARG(min_seqid >= 1, "seqid_filter: min_seqid=%d is below 1", min_seqid);
    RNAMSM_CHECK_ARG(max_seqid >= 1 && max_seqid <= 100, "seqid_filter: max_seqid=%d outside [1, 100]", max_seqid);
    RNAMSM_CHECK_ARG(step >= 1, "seqid_filter: step=%d is below 1", step);
    const SeqidWs w = seqid_ws(N, L);
    RNAMSM_CHECK_ARG(workspace_bytes >= w.total && (reinterpret_cast<uintptr_t>(workspace) & 255u) == 0,
                     "seqid_filter: workspace of %zu bytes too small (%zu) or misaligned (256 bytes)", workspace_bytes, w.total);
    RNAMSM_CHECK_ARG((reinterpret_cast<uintptr_t>(kept_indices) & 3u) == 0 && (reinterpret_cast<uintptr_t>(kept_at) & 3u) == 0 &&
                         (reinterpret_cast<uintptr_t>(order) & 3u) == 0,
                     "seqid_filter: order / kept_indices / kept_at misaligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    uint64_t* P = reinterpret_cast<uint64_t*>(ws + w.pack);
    int32_t* nres = reinterpret_cast<int32_t*>(ws + w.nres);
    int32_t* at = reinterpret_cast<int32_t*>(ws + w.kept_at);
    int32_t* kept_pos = reinterpret_cast<int32_t*>(ws + w.kept_pos);
    int32_t* rej = reinterpret_cast<int32_t*>(ws + w.rej);
    int32_t* meta = reinterpret_cast<int32_t*>(ws + w.meta);
    int thresholds[100];
    const int n_thr = sq_thresholds(num_seqs, min_seqid, max_seqid, step, thresholds);
    const int chunk = tuning().seqid_filter_chunk;

    hipLaunchKernelGGL(seqid_order_check_kernel, dim3(1), dim3(1024), 0, s, order, N, meta);
    words_pack(msa, N, L, ld, gap, order, w.Wp, w.Np, P, s);
    hipLaunchKernelGGL(seqid_nres_kernel, dim3((unsigned)((w.Np + 255) / 256)), dim3(256), 0, s, P, w.Wp, w.Np, nres, at, meta);
    RNAMSM_CHECK_LAUNCH("seqid_filter");
    int host_meta[2] = {0, -1};
    for (int pass = 0; pass < n_thr; ++pass) {
        const int t = thresholds[pass];
        for (int64_t c0 = 0; c0 < w.Np; c0 += chunk) {
            const int tiles = (int)((w.Np - c0 < chunk ? w.Np - c0 : chunk) / SQ_TILE);
            hipLaunchKernelGGL(seqid_cand_kernel, dim3(tiles), dim3(256), 0, s, P, w.Wp, w.Np, N, c0, t, nres, at, kept_pos, meta, rej);
            hipLaunchKernelGGL(seqid_resolve_kernel, dim3(1), dim3(256), 0, s, P, w.Wp, w.Np, c0, tiles, t, rej, at, kept_pos, meta);
        }
        RNAMSM_CHECK_LAUNCH("seqid_filter");
        // the one read-back of the pass: the kept count, and (once) the verdict on the order
        hipError_t e = hipMemcpyAsync(host_meta, meta, sizeof(host_meta), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(RNAMSM_ERR_HIP, "seqid_filter: reading the kept count back: %s", hipGetErrorString(e));
        RNAMSM_CHECK_ARG(host_meta[1] < 0, "seqid_filter: order[%d] lies outside [0, %d)", host_meta[1], N);
        if (num_seqs > 0 && host_meta[0] >= num_seqs) break;
    }
    const int nk = host_meta[0];
    hipLaunchKernelGGL(seqid_clear_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, rej, kept_at);
    hipLaunchKernelGGL(seqid_scatter_kernel, dim3((nk + 255) / 256), dim3(256), 0, s, nk, kept_pos, at, order, rej, kept_at);
    hipLaunchKernelGGL(compact_flags_kernel<int32_t>, dim3(1), dim3(1024), 0, s, rej, N, kept_indices);
    RNAMSM_CHECK_LAUNCH("seqid_filter");
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(RNAMSM_ERR_HIP, "seqid_filter: waiting for the stream: %s", hipGetErrorString(e));
    *n_kept = nk;
    return RNAMSM_OK;
}
