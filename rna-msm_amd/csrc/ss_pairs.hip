// RNA-MSM-SS: the predicted structure on the device -- the [L, L] probabilities of the head become the partner vector and the
// bodies of `<name>.ct` / `<name>.bpseq` (ss_pairs.h: the decoding as a graph process; struct_text.h: the lines), so that nothing of
// size L^2 has to reach the host for them.
// One workgroup per structure, one thread per base (L <= 1024 = the workgroup limit: no grid-wide synchronisation).  The adjacency
// bit matrix (L x ceil(L / 64) words, 128 KB at L = 1024) lies in the caller's workspace: one code path for every L, no dynamic LDS
// to configure per device, and a member's rows stay in L2.  Building it: a wave per row, a lane per partner, one __ballot per 64
// partners.  A round: thread b marks (LDS), a block-wide "any mark" ends the loop, then thread b clears its own row -- a thread
// writes its own row and its own mark only: no atomics, the same bits on every run.
// The kernel ends in the tail every decoder shares (struct_text.h: emit_struct_text), with thread b's partner in a register.
// The lone entry point and the packed one run the same kernel: the descriptors travel as kernel arguments, 32 per launch
// (common.h: MemberChunk, member_chunk); a block's member is its index in the chunk, and the lone call is a chunk of one.
#include "common.h"
#include "ss_pairs.h"

namespace rnamsm {
namespace {

static_assert(sspairs::MAX_L == RNAMSM_SS_MAX_L, "one limit");

struct SsPairsMember {       // 64 bytes
    const float* probs;      // [L, L]
    const uint8_t* letters;  // [L]
    uint64_t* adj;           // [L, words(L)] inside the workspace
    int32_t* partner;        // [L]
    int32_t* counts;         // [4]
    uint8_t* ct;             // [ct bound]
    uint8_t* bpseq;          // [bpseq bound]
    int32_t L, pad_;
};
static_assert(sizeof(SsPairsMember) == 64, "SsPairsMember layout");

__global__ __launch_bounds__(1024) void ss_pairs_kernel(const MemberChunk<SsPairsMember> chunk) {
    __shared__ alignas(8) int32_t mark[sspairs::MAX_L];      // and, behind the rounds, the scan's 16 words
    const SsPairsMember m = chunk.m[blockIdx.x];
    const int L = m.L, W = sspairs::words(L);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nw = blockDim.x >> 6;      // blockDim: a multiple of 64, >= L

    for (int b = wave; b < L; b += nw)
        for (int k = 0; k < W; ++k) {
            const uint64_t bits = __ballot(sspairs::edge_at(m.probs, L, b, 64 * k + lane));
            if (lane == 0) m.adj[b * W + k] = bits;
        }
    __syncthreads();

    uint64_t* row = m.adj + (t < L ? t : 0) * W;
    for (int round = 0; round < L; ++round) {          // ends after at most L - 2 rounds by itself
        const int mine = t < L ? sspairs::pick_mark(row, W, t, m.probs, L) : -1;
        mark[t] = mine;
        if (!__syncthreads_or(mine >= 0)) break;
        if (t < L) sspairs::remove_marked(row, W, t, mark);
        __syncthreads();
    }

    const int b0 = sspairs::first_base(t, L, blockDim.x), b1 = sspairs::end_base(t, L, blockDim.x);      // base t, or none
    int partner = 0;
    if (b0 < b1) {
        partner = sspairs::partner_of(row, W);
        m.partner[t] = partner;
    }
    // mark is free: nobody reads it after the barrier that ended the rounds, and the scan writes behind another one
    emit_struct_text(L, b0, b1, [partner](int) { return partner; }, m.letters, m.ct, m.bpseq, m.counts,
                     reinterpret_cast<uint64_t*>(mark));
}

// Every refusal, then the launches.  who: the entry point's name; lone: the one item is the call's own arguments, not "member 0".
int ss_pairs_run(const char* who, bool lone, const rnamsm_ss_pairs_item* items, int B, void* workspace, size_t workspace_bytes,
                 hipStream_t s) {
    char where[32] = "";
    size_t need = 0;
    for (int b = 0; b < B; ++b) {
        if (!lone) snprintf(where, sizeof(where), "member %d: ", b);
        if (int rc = check_struct_item(who, where, RNAMSM_SS_MAX_L, items[b])) return rc;
        need += sspairs::adj_bytes(items[b].L);
    }
    if (int rc = check_struct_workspace(who, workspace, workspace_bytes, need)) return rc;
    size_t off = 0;
    for (int b0 = 0; b0 < B; b0 += 32) {
        int n, max_L = 1;
        auto fill = [&](int b) {
            const rnamsm_ss_pairs_item& it = items[b];
            SsPairsMember m = {it.probs, it.letters, reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(workspace) + off),
                               it.partner, it.counts, it.ct, it.bpseq, it.L, 0};
            off += sspairs::adj_bytes(it.L);
            if (it.L > max_L) max_L = it.L;
            return m;
        };
        const MemberChunk<SsPairsMember> chunk = member_chunk<SsPairsMember>(b0, B, fill, n);
        hipLaunchKernelGGL(ss_pairs_kernel, dim3((unsigned)n), dim3((unsigned)((max_L + 63) & ~63)), 0, s, chunk);
        RNAMSM_CHECK_LAUNCH("ss_pairs");
    }
    return RNAMSM_OK;
}

}  // namespace
}  // namespace rnamsm

using namespace rnamsm;

extern "C" size_t rnamsm_ss_pairs_workspace_bytes(int B, const int* Ls) {
    if (B < 1 || B > RNAMSM_SS_MAX_BATCH || !Ls) return 0;
    size_t n = 0;
    for (int b = 0; b < B; ++b) {
        if (Ls[b] < 1 || Ls[b] > RNAMSM_SS_MAX_L) return 0;
        n += sspairs::adj_bytes(Ls[b]);
    }
    return n;
}

extern "C" int rnamsm_ss_struct_text_bytes(int L, size_t* ct_bytes, size_t* bpseq_bytes) {
    return struct_text_bytes("ss_struct_text_bytes", RNAMSM_SS_MAX_L, L, ct_bytes, bpseq_bytes);
}

extern "C" int rnamsm_ss_pairs(const float* probs, const uint8_t* letters, int L, int32_t* partner, int32_t* counts, uint8_t* ct,
                               uint8_t* bpseq, void* workspace, size_t workspace_bytes, void* stream) {
    const rnamsm_ss_pairs_item item = {probs, letters, L, partner, counts, ct, bpseq};
    return ss_pairs_run("ss_pairs", true, &item, 1, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int rnamsm_ss_pairs_packed(const rnamsm_ss_pairs_item* items, int B, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    // every refusal comes before the first launch: a refused call leaves the stream and the outputs untouched
    RNAMSM_CHECK_ARG(items, "ss_pairs_packed: null pointer");
    RNAMSM_CHECK_ARG(B >= 1 && B <= RNAMSM_SS_MAX_BATCH, "ss_pairs_packed: B=%d outside [1, %d]", B, RNAMSM_SS_MAX_BATCH);
    return ss_pairs_run("ss_pairs_packed", false, items, B, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}
