// RNA-MSM-SS: the predicted structure of a LONG alignment on the device -- rnamsm_ss_pairs for L up to RNAMSM_LONG_MAX_L = 4096,
// where ss_pairs.hip's one thread per base ends at the workgroup limit (1024).  The same graph process and the same lines
// (ss_pairs.h, struct_text.h), with several bases per thread (ss_pairs_long.h): the same bytes as rnamsm_ss_pairs where both run.
// Two launches:
//   1. the adjacency bit matrix, across the grid: a wave per row, a lane per partner, one __ballot per 64 partners; rows dealt over
//      ceil(L / 4) blocks of 4 waves.  The only L^2 part (67 MB of probabilities at the limit): HBM-bound.
//   2. the rounds and the lines, in ONE workgroup of 1024 threads, each owning ceil(L / 1024) consecutive bases.  A round touches
//      edges, not pixels -- a base's row is ceil(L / 64) words and it reads one probability per partner -- so what a grid-wide
//      barrier per round would cost (a cooperative launch, an agent-scope release/acquire per round) buys nothing here.  mark[4096]
//      lies in LDS (16 KB); thread t marks for its bases, a block-wide "any mark" ends the loop, then it clears its own rows: a
//      thread writes only its own bases' rows and marks -- no atomics, the same bits on every run.
//      Then every thread writes its bases' partners, and the kernel ends in the tail every decoder shares (struct_text.h:
//      emit_struct_text), which reads them back.
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
    __shared__ uint64_t scan[sspairs::LONG_THREADS / 64];
    const int L = m.L, W = sspairs::words(L), t = threadIdx.x;

    for (int round = 0; round < L; ++round) {          // ends after at most L - 2 rounds by itself
        const bool any = sspairs::thread_mark(m.adj, W, t, m.probs, L, mark);
        if (!__syncthreads_or(any)) break;
        sspairs::thread_remove(m.adj, W, t, L, mark);
        __syncthreads();
    }

    sspairs::thread_partners(m.adj, W, t, L, m.partner);
    // partner[b] of a thread's own bases: written above by this thread
    emit_struct_text(L, sspairs::first_base(t, L, sspairs::LONG_THREADS), sspairs::end_base(t, L, sspairs::LONG_THREADS),
                     [&](int b) { return m.partner[b]; }, m.letters, m.ct, m.bpseq, m.counts, scan);
}

}  // namespace
}  // namespace rnamsm

using namespace rnamsm;

extern "C" size_t rnamsm_ss_pairs_long_workspace_bytes(int L) {
    if (L < 1 || L > RNAMSM_LONG_MAX_L) return 0;
    return sspairs::adj_bytes(L);
}

extern "C" int rnamsm_ss_struct_text_long_bytes(int L, size_t* ct_bytes, size_t* bpseq_bytes) {
    return struct_text_bytes("ss_struct_text_long_bytes", RNAMSM_LONG_MAX_L, L, ct_bytes, bpseq_bytes);
}

extern "C" int rnamsm_ss_pairs_long(const float* probs, const uint8_t* letters, int L, int32_t* partner, int32_t* counts, uint8_t* ct,
                                    uint8_t* bpseq, void* workspace, size_t workspace_bytes, void* stream) {
    // every refusal comes before the first launch: a refused call leaves the stream and the outputs untouched
    const rnamsm_ss_pairs_item item = {probs, letters, L, partner, counts, ct, bpseq};
    if (int rc = check_struct_item("ss_pairs_long", "", RNAMSM_LONG_MAX_L, item)) return rc;
    if (int rc = check_struct_workspace("ss_pairs_long", workspace, workspace_bytes, sspairs::adj_bytes(L))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const SsPairsLong m = {probs, letters, static_cast<uint64_t*>(workspace), partner, counts, ct, bpseq, L};
    hipLaunchKernelGGL(ss_pairs_long_adj_kernel, dim3((unsigned)((L + SPL_ADJ_WAVES - 1) / SPL_ADJ_WAVES)), dim3(64 * SPL_ADJ_WAVES), 0, s, m);
    RNAMSM_CHECK_LAUNCH("ss_pairs_long_adj");
    hipLaunchKernelGGL(ss_pairs_long_rounds_kernel, dim3(1), dim3(sspairs::LONG_THREADS), 0, s, m);
    RNAMSM_CHECK_LAUNCH("ss_pairs_long_rounds");
    return RNAMSM_OK;
}
