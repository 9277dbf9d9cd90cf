// The identity redundancy filter on the device: a row sub-sampling rule of this project's own, modelled on what the reference asks of
// the external hhfilter binary (`-id 90 -diff num_seqs`, utils/align.py:68-102, 165-173).  It is NOT that binary's algorithm: hhfilter's
// -diff counts sequences per window of 50 columns and has its own threshold schedule; this rule counts over the whole alignment.
//
// The rule, all in integers.  Per pair of rows, both = the columns where neither has the gap, same = those of them
// where the bytes are equal, nres(i) = both(i, i).  Row k is REDUNDANT to row j at threshold t iff both > 0 and 100 * same >= t * both.
// The rows are walked in `order`, one pass per threshold (seqid_words.h: sq_thresholds): a row not kept yet is kept iff it is
// redundant to no kept row -- of an earlier pass, or earlier in this one; a row without residues is never kept unless it is the first
// of the order, which always is.  The walk stops after the first pass that leaves num_seqs rows kept (num_seqs > 0), or after the
// last threshold.
//
// Data flow (all on the caller's stream, every buffer in the caller's workspace).  Everything past the pack works on POSITIONS of
// the order, not on row indices: position p holds row order[p], so a chunk of the walk is a run of consecutive positions.
//   check    the lowest position whose order entry lies outside [0, N), or -1: one block, one slot          seqid_order_check_kernel
//   pack     P[w][p] = the recoded bytes of columns 8w .. 8w + 7 of row order[p] as a 64-bit word (seqid_words.h), word-major, the
//            positions padded to a multiple of 64 and the words to a multiple of 8 with zero words; an entry outside [0, N) packs
//            as a row of gaps and reads nothing                                                              seqid_pack_kernel
//   nres     per position, from its words; kept_at = -1; the kept count = 0                                  seqid_nres_kernel
//   then, per pass at threshold t and per chunk of `chunk` positions, two launches ordered by the stream:
//   cand     a block owns 64 positions of the chunk.  A CANDIDATE is a position not kept yet with residues (or position 0).  The
//            block walks the kept list 64 at a time -- the kept count is read from device memory, so it holds what earlier chunks of
//            this pass kept -- and accumulates both and same of its 64 x 64 pairs like pdist_pair_kernel accumulates m: 256 threads,
//            a 4 x 4 register tile per thread, two int32 each, 8 words of the 64 + 64 rows staged in LDS per step.  The kept rows'
//            words are GATHERED through the kept list (8-byte reads; no second copy of the rows).  Each pair is thresholded, a
//            candidate redundant to any kept row is rejected; a block whose 64 positions are all rejected or no candidates stops
//            walking.  rej[p] = 1 for a rejected position or one that is no candidate, else 0: one slot per position, written
//            once a launch                                                                                   seqid_cand_kernel
//   resolve  one block per chunk.  The chunk's survivors (rej = 0) as bit masks; the predicate of every pair of the chunk whose
//            64 x 64 tile has survivors on both sides, on or above the diagonal, by the same tile loop, as a bit matrix in LDS
//            (chunk x chunk bits).  Then ONE WAVE walks the chunk in order: the lowest survivor still alive is kept -- appended
//            to the kept list, kept_at = t -- and every later survivor redundant to it is struck, lane l holding the alive bits
//            of positions 64 l .. 64 l + 63.  This kernel carries the rule's sequential dependence        seqid_resolve_kernel
//   The host reads the kept count back ONCE PER PASS (with the order's verdict after the first) to decide whether to stop; within
//   a pass nothing is read back.  A chunk's kept rows are exactly those the walk would keep row by row: a survivor is redundant to
//   no row kept before the chunk (cand) and to no row kept earlier in the chunk (resolve), so ANY chunk size gives the same list.
//   finish   the kept positions -> row flags and kept_at per row (each kept row written once), then the flags -> ascending
//            indices by a block-wide scan                                        seqid_scatter_kernel, seqid_compact_kernel
// No atomics anywhere; integer sums in a fixed order; the same indices on every run.
#include "common.h"
#include "seqid_words.h"

namespace rnamsm {

constexpr int SQ_TILE = 64;          // positions of a pair tile, each way
constexpr int SQ_WK = 8;             // words staged per step
constexpr int SQ_MAX_L = 32768;
constexpr int SQ_MAX_N = 1 << 20;
constexpr int SQ_MAX_CHUNK = 512;    // the bit matrix of a chunk: 512 x 512 bits = 32 KB of LDS
constexpr int SQ_MAX_TILES = SQ_MAX_CHUNK / SQ_TILE;

// meta[0] = the kept count, meta[1] = the lowest position with an order entry outside [0, N), or -1
__global__ __launch_bounds__(1024) void seqid_order_check_kernel(const int32_t* __restrict__ order, int N, int32_t* __restrict__ meta) {
    __shared__ int s[1024];
    int bad = 0x7fffffff;
    if (order)
        for (int p = threadIdx.x; p < N; p += 1024) {
            const int r = order[p];
            if ((r < 0 || r >= N) && p < bad) bad = p;
        }
    s[threadIdx.x] = bad;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off && s[threadIdx.x + off] < s[threadIdx.x]) s[threadIdx.x] = s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) meta[1] = s[0] == 0x7fffffff ? -1 : s[0];
}

// one thread per (position, word), the words of a position on neighbouring threads
__global__ __launch_bounds__(256) void seqid_pack_kernel(const uint8_t* __restrict__ msa, int N, int L, int64_t ld, int gap,
                                                         const int32_t* __restrict__ order, int Wp, int64_t Np, uint64_t* __restrict__ P) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= Np * Wp) return;
    const int64_t pos = idx / Wp;
    const int w = (int)(idx - pos * Wp);
    int64_t row = -1;
    if (pos < N) row = order ? (int64_t)order[pos] : pos;
    P[(int64_t)w * Np + pos] = (row >= 0 && row < N) ? sq_pack_word(msa + row * ld, 8 * w, L - 8 * w, gap) : 0ull;
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

// acc + the set bits of mask in one instruction (msa_pdist.hip: pd_count_add)
__device__ __forceinline__ int sq_count_add(uint32_t mask, int acc) {
    int out;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(out) : "v"(mask), "v"(acc));
    return out;
}

// The tile loop both kernels share: both and same of 64 x 64 pairs over all Wp words.  Side A is the 64 consecutive positions from
// `ra`; side B is the 64 consecutive positions from `rb` (idxB == nullptr) or the positions idxB[0 .. 63] (LDS; -1 = no row: zero
// words, so both = 0 and the pair is never redundant).  Thread (ty, tx) = (threadIdx.x / 16, % 16) owns the pairs
// (ty * 4 + x, tx * 4 + y).  Ends with a barrier: the panels are free again.
__device__ __forceinline__ void sq_tile_counts(const uint64_t* __restrict__ P, int Wp, int64_t Np, int64_t ra, int64_t rb, const int* idxB,
                                               uint64_t (*sA)[SQ_TILE], uint64_t (*sB)[SQ_TILE], int (&both)[4][4], int (&same)[4][4]) {
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) both[x][y] = same[x][y] = 0;
    const int sw = threadIdx.x >> 5, sp = (threadIdx.x & 31) * 2;       // this thread's vector of a panel: word sw, rows sp, sp + 1
    int64_t g0 = 0, g1 = 0;
    if (idxB) { g0 = idxB[sp]; g1 = idxB[sp + 1]; }
    for (int w0 = 0; w0 < Wp; w0 += SQ_WK) {
        const uint64_t* base = P + (int64_t)(w0 + sw) * Np;
        *reinterpret_cast<uint4*>(&sA[sw][sp]) = *reinterpret_cast<const uint4*>(base + ra + sp);
        if (idxB) {
            sB[sw][sp] = g0 >= 0 ? base[g0] : 0ull;
            sB[sw][sp + 1] = g1 >= 0 ? base[g1] : 0ull;
        } else {
            *reinterpret_cast<uint4*>(&sB[sw][sp]) = *reinterpret_cast<const uint4*>(base + rb + sp);
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < SQ_WK; ++w) {
            uint64_t a[4], b[4];
            uint32_t al[4], ah[4], bl[4], bh[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                a[x] = sA[w][ty * 4 + x];
                b[x] = sB[w][tx * 4 + x];
                al[x] = sq_residues_lo(a[x]); ah[x] = sq_residues_hi(a[x]);
                bl[x] = sq_residues_lo(b[x]); bh[x] = sq_residues_hi(b[x]);
            }
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) {
                    const uint64_t d = a[x] ^ b[y];
                    const uint32_t ml = al[x] & bl[y], mh = ah[x] & bh[y];
                    both[x][y] = sq_count_add(mh, sq_count_add(ml, both[x][y]));
                    same[x][y] = sq_count_add(mh & ~sq_residues_hi(d), sq_count_add(ml & ~sq_residues_lo(d), same[x][y]));
                }
        }
        __syncthreads();
    }
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
        int both[4][4], same[4][4];
        sq_tile_counts(P, Wp, Np, ra, 0, s_idx, sA, sB, both, same);
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            bool hit = false;
#pragma unroll
            for (int y = 0; y < 4; ++y) hit = hit || sq_redundant(both[x][y], same[x][y], t);
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
            int both[4][4], same[4][4];
            sq_tile_counts(P, Wp, Np, c0 + (int64_t)ti * SQ_TILE, c0 + (int64_t)tj * SQ_TILE, nullptr, sA, sB, both, same);
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                uint32_t nib = 0;
#pragma unroll
                for (int y = 0; y < 4; ++y) nib |= sq_redundant(both[x][y], same[x][y], t) ? 1u << y : 0u;
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
// single block: row flags -> ascending index list (greedy_compact_kernel's scan)
__global__ __launch_bounds__(1024) void seqid_compact_kernel(const int32_t* __restrict__ flags, int N, int32_t* __restrict__ out) {
    __shared__ int base;
    __shared__ int cnt[1024];
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int start = 0; start < N; start += 1024) {
        const int n = start + threadIdx.x;
        const int f = (n < N && flags[n]) ? 1 : 0;
        cnt[threadIdx.x] = f;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {                        // inclusive scan
            const int v = (int)threadIdx.x >= off ? cnt[threadIdx.x - off] : 0;
            __syncthreads();
            cnt[threadIdx.x] += v;
            __syncthreads();
        }
        if (f) out[base + cnt[threadIdx.x] - 1] = n;
        __syncthreads();
        if (threadIdx.x == 1023) base += cnt[1023];
        __syncthreads();
    }
}

struct SeqidWs {
    size_t pack, nres, kept_at, kept_pos, rej, meta, total;      // offsets, each a multiple of 256
    int Wp;
    int64_t Np;
};
static SeqidWs seqid_ws(int N, int L) {
    SeqidWs w;
    w.Np = ((int64_t)N + SQ_TILE - 1) / SQ_TILE * SQ_TILE;
    w.Wp = ((L + 7) / 8 + SQ_WK - 1) / SQ_WK * SQ_WK;
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
    const int64_t total = w.Np * w.Wp;
    hipLaunchKernelGGL(seqid_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, msa, N, L, ld, gap, order, w.Wp, w.Np, P);
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
    hipLaunchKernelGGL(seqid_compact_kernel, dim3(1), dim3(1024), 0, s, rej, N, kept_indices);
    RNAMSM_CHECK_LAUNCH("seqid_filter");
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(RNAMSM_ERR_HIP, "seqid_filter: waiting for the stream: %s", hipGetErrorString(e));
    *n_kept = nk;
    return RNAMSM_OK;
}
