// RNA-MSM-SS: the predicted structure of a LONG alignment on the device -- rnamsm_ss_pairs for L up to RNAMSM_LONG_MAX_L = 4096,
// where ss_pairs.hip's one thread per base ends at the workgroup limit (1024).  The same graph process and the same lines
// (ss_pairs.h), with several bases per thread (ss_pairs_long.h): the same bytes as rnamsm_ss_pairs where both run.
// Two launches:
//   1. the adjacency bit matrix, across the grid: a wave per row, a lane per partner, one __ballot per 64 partners; rows dealt over
//      ceil(L / 4) blocks of 4 waves.  The only L^2 part (67 MB of probabilities at the limit): HBM-bound.
//   2. the rounds and the lines, in ONE workgroup of 1024 threads, each owning ceil(L / 1024) consecutive bases.  A round touches
//      edges, not pixels -- a base's row is ceil(L / 64) words and it reads one probability per partner -- so what a grid-wide
//      barrier per round would cost (a cooperative launch, an agent-scope release/acquire per round) buys nothing here.  mark[4096]
//      lies in LDS (16 KB); thread t marks for its bases, a block-wide "any mark" ends the loop, then it clears its own rows: a
//      thread writes only its own bases' rows and marks -- no atomics, the same bits on every run.
//      The lines: .ct can reach 32 L = 131072 bytes, beyond the 16-bit halves ss_pairs.hip packs into one word: one 64-bit scan over
//      THREADS (a thread's bases are contiguous, so are its lines) carries both offsets and the pair count in 21-bit fields.
#include "common.h"
#include "ss_pairs_long.h"

namespace rnamsm {
namespace {

static_assert(sspairs::LONG_MAX_L == RNAMSM_LONG_MAX_L, "one limit");
constexpr int SPL_ADJ_WAVES = 4;       // rows of one block of launch 1

struct SsPairsLong {
    const float* probs;      // [L, L]
    const uint8_t* letters;  // [L]
    uint64_t* adj;           // [L, words(L)]: the workspace
    int32_t* partner;        // [L]
    int32_t* counts;         // [4]
    uint8_t* ct;             // [32 L]
    uint8_t* bpseq;          // [12 L]
    int32_t L;
};

__global__ __launch_bounds__(64 * SPL_ADJ_WAVES) void ss_pairs_long_adj_kernel(const SsPairsLong m) {
    const int L = m.L, W = sspairs::words(L);
    const int lane = threadIdx.x & 63, b = (int)blockIdx.x * SPL_ADJ_WAVES + ((int)threadIdx.x >> 6);
    if (b >= L) return;                                   // wave-uniform
    for (int k = 0; k < W; ++k) {
        const uint64_t bits = __ballot(sspairs::edge_at(m.probs, L, b, 64 * k + lane));
        if (lane == 0) m.adj[(size_t)b * W + k] = bits;
    }
}

__global__ __launch_bounds__(sspairs::LONG_THREADS) void ss_pairs_long_rounds_kernel(const SsPairsLong m) {
    __shared__ int32_t mark[sspairs::LONG_MAX_L];
    __shared__ uint64_t wave_total[sspairs::LONG_THREADS / 64];
    const int L = m.L, W = sspairs::words(L);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    constexpr int NW = sspairs::LONG_THREADS / 64;

    for (int round = 0; round < L; ++round) {          // ends after at most L - 2 rounds by itself
        const bool any = sspairs::thread_mark(m.adj, W, t, m.probs, L, mark);
        if (!__syncthreads_or(any)) break;
        sspairs::thread_remove(m.adj, W, t, L, mark);
        __syncthreads();
    }

    bool bad = false;
    const uint64_t len = sspairs::thread_measure(m.adj, W, t, L, m.letters, m.partner, &bad);
    const int any_bad = __syncthreads_or(bad);
    uint64_t incl = len;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t up = (uint64_t)__shfl_up((unsigned long long)incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint64_t before = 0, total = 0;
    for (int w = 0; w < NW; ++w) {
        const uint64_t s = wave_total[w];
        if (w < wave) before += s;
        total += s;
    }
    // partner[b] of a thread's own bases: written above by this thread
    sspairs::thread_put_lines(t, L, m.letters, m.partner, before + incl - len, m.ct, m.bpseq);
    if (t == 0) {
        m.counts[0] = sspairs::pairs_of(total);
        m.counts[1] = sspairs::ct_of(total);
        m.counts[2] = sspairs::bpseq_of(total);
        m.counts[3] = any_bad ? 1 : 0;
    }
}

size_t adj_long_bytes(int L) { return ((size_t)L * sspairs::words(L) * 8 + 255) & ~(size_t)255; }

}  // namespace
}  // namespace rnamsm

using namespace rnamsm;

extern "C" size_t rnamsm_ss_pairs_long_workspace_bytes(int L) {
    if (L < 1 || L > RNAMSM_LONG_MAX_L) return 0;
    return adj_long_bytes(L);
}

extern "C" int rnamsm_ss_struct_text_long_bytes(int L, size_t* ct_bytes, size_t* bpseq_bytes) {
    RNAMSM_CHECK_ARG(L >= 1 && L <= RNAMSM_LONG_MAX_L, "ss_struct_text_long_bytes: L=%d outside [1, %d]", L, RNAMSM_LONG_MAX_L);
    RNAMSM_CHECK_ARG(ct_bytes && bpseq_bytes, "ss_struct_text_long_bytes: null pointer");
    *ct_bytes = (size_t)sspairs::CT_LINE_MAX * L;
    *bpseq_bytes = (size_t)sspairs::BPSEQ_LINE_MAX * L;
    return RNAMSM_OK;
}

extern "C" int rnamsm_ss_pairs_long(const float* probs, const uint8_t* letters, int L, int32_t* partner, int32_t* counts, uint8_t* ct,
                                    uint8_t* bpseq, void* workspace, size_t workspace_bytes, void* stream) {
    // every refusal comes before the first launch: a refused call leaves the stream and the outputs untouched
    RNAMSM_CHECK_ARG(L >= 1 && L <= RNAMSM_LONG_MAX_L, "ss_pairs_long: L=%d outside [1, %d]", L, RNAMSM_LONG_MAX_L);
    RNAMSM_CHECK_ARG(probs, "ss_pairs_long: null pointer (probs)");
    RNAMSM_CHECK_ARG(letters, "ss_pairs_long: null pointer (letters)");
    RNAMSM_CHECK_ARG(partner, "ss_pairs_long: null pointer (partner)");
    RNAMSM_CHECK_ARG(counts, "ss_pairs_long: null pointer (counts)");
    RNAMSM_CHECK_ARG(ct, "ss_pairs_long: null pointer (ct)");
    RNAMSM_CHECK_ARG(bpseq, "ss_pairs_long: null pointer (bpseq)");
    RNAMSM_CHECK_ARG(workspace, "ss_pairs_long: null pointer (workspace)");
    RNAMSM_CHECK_ARG(((uintptr_t)probs & 3u) == 0, "ss_pairs_long: probs is not 4-byte aligned");
    RNAMSM_CHECK_ARG(((uintptr_t)partner & 3u) == 0, "ss_pairs_long: partner is not 4-byte aligned");
    RNAMSM_CHECK_ARG(((uintptr_t)counts & 3u) == 0, "ss_pairs_long: counts is not 4-byte aligned");
    RNAMSM_CHECK_ARG(aligned16(workspace), "ss_pairs_long: workspace is not 16-byte aligned");
    RNAMSM_CHECK_ARG(workspace_bytes >= adj_long_bytes(L), "ss_pairs_long: workspace of %zu bytes, %zu needed", workspace_bytes,
                     adj_long_bytes(L));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const SsPairsLong m = {probs, letters, static_cast<uint64_t*>(workspace), partner, counts, ct, bpseq, L};
    hipLaunchKernelGGL(ss_pairs_long_adj_kernel, dim3((unsigned)((L + SPL_ADJ_WAVES - 1) / SPL_ADJ_WAVES)), dim3(64 * SPL_ADJ_WAVES), 0, s, m);
    RNAMSM_CHECK_LAUNCH("ss_pairs_long_adj");
    hipLaunchKernelGGL(ss_pairs_long_rounds_kernel, dim3(1), dim3(sspairs::LONG_THREADS), 0, s, m);
    RNAMSM_CHECK_LAUNCH("ss_pairs_long_rounds");
    return RNAMSM_OK;
}
