// RNA-MSM-SS: the predicted structure on the device -- the [L, L] probabilities of the head become the partner vector and the
// bodies of `<name>.ct` / `<name>.bpseq` (ss_pairs.h: the decoding as a graph process, and the lines), so that nothing of size L^2
// has to reach the host for them.
// One workgroup per structure, one thread per base (L <= 1024 = the workgroup limit: no grid-wide synchronisation).  The adjacency
// bit matrix (L x ceil(L / 64) words, 128 KB at L = 1024) lies in the caller's workspace: one code path for every L, no dynamic LDS
// to configure per device, and a member's rows stay in L2.  Building it: a wave per row, a lane per partner, one __ballot per 64
// partners.  A round: thread b marks (LDS), a block-wide "any mark" ends the loop, then thread b clears its own row -- a thread
// writes its own row and its own mark only: no atomics, the same bits on every run.
// The lines have variable width: a block prefix scan of the lengths gives every thread its offsets, and it writes its bytes itself.
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
    __shared__ int32_t mark[sspairs::MAX_L];
    __shared__ uint32_t wave_total[16];
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

    int partner = 0, ct_len = 0, bp_len = 0;
    uint8_t letter = 0;
    bool bad = false;
    if (t < L) {
        partner = sspairs::partner_of(row, W);
        m.partner[t] = partner;
        letter = m.letters[t];
        bad = sspairs::letter_needs_host(letter);
        ct_len = sspairs::ct_line_len(t + 1, L, partner);
        bp_len = sspairs::bpseq_line_len(t + 1, partner);
    }
    const int n_pairs = __syncthreads_count(partner > t + 1);
    const int any_bad = __syncthreads_or(bad);
    // both lengths in one word: ct <= 32 L < 2^16 in the low half, bpseq <= 12 L in the high half
    const uint32_t len = (uint32_t)ct_len | (uint32_t)bp_len << 16;
    uint32_t incl = len;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int w = 0; w < nw; ++w) {
        const uint32_t s = wave_total[w];
        if (w < wave) before += s;
        total += s;
    }
    const uint32_t at = before + incl - len;
    if (t < L) {
        sspairs::put_ct_line(m.ct + (at & 0xffffu), t + 1, letter, L, partner);
        sspairs::put_bpseq_line(m.bpseq + (at >> 16), t + 1, letter, partner);
    }
    if (t == 0) {
        m.counts[0] = n_pairs;
        m.counts[1] = (int32_t)(total & 0xffffu);
        m.counts[2] = (int32_t)(total >> 16);
        m.counts[3] = any_bad ? 1 : 0;
    }
}

size_t adj_bytes(int L) { return ((size_t)L * sspairs::words(L) * 8 + 255) & ~(size_t)255; }

// Every refusal, then the launches.  who: the entry point's name; lone: the one item is the call's own arguments, not "member 0".
int ss_pairs_run(const char* who, bool lone, const rnamsm_ss_pairs_item* items, int B, void* workspace, size_t workspace_bytes,
                 hipStream_t s) {
    char where[32] = "";
    size_t need = 0;
    for (int b = 0; b < B; ++b) {
        const rnamsm_ss_pairs_item& it = items[b];
        if (!lone) snprintf(where, sizeof(where), "member %d: ", b);
        RNAMSM_CHECK_ARG(it.L >= 1 && it.L <= RNAMSM_SS_MAX_L, "%s: %sL=%d outside [1, %d]", who, where, it.L, RNAMSM_SS_MAX_L);
        RNAMSM_CHECK_ARG(it.probs && it.letters && it.partner && it.counts && it.ct && it.bpseq, "%s: %snull pointer", who, where);
        RNAMSM_CHECK_ARG(((uintptr_t)it.probs & 3u) == 0 && ((uintptr_t)it.partner & 3u) == 0 && ((uintptr_t)it.counts & 3u) == 0,
                         "%s: %sprobs, partner or counts is not 4-byte aligned", who, where);
        need += adj_bytes(it.L);
    }
    RNAMSM_CHECK_ARG(workspace, "%s: null pointer (workspace)", who);
    RNAMSM_CHECK_ARG(aligned16(workspace), "%s: workspace is not 16-byte aligned", who);
    RNAMSM_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    size_t off = 0;
    for (int b0 = 0; b0 < B; b0 += 32) {
        int n, max_L = 1;
        auto fill = [&](int b) {
            const rnamsm_ss_pairs_item& it = items[b];
            SsPairsMember m = {it.probs, it.letters, reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(workspace) + off),
                               it.partner, it.counts, it.ct, it.bpseq, it.L, 0};
            off += adj_bytes(it.L);
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
        n += adj_bytes(Ls[b]);
    }
    return n;
}

extern "C" int rnamsm_ss_struct_text_bytes(int L, size_t* ct_bytes, size_t* bpseq_bytes) {
    RNAMSM_CHECK_ARG(L >= 1 && L <= RNAMSM_SS_MAX_L, "ss_struct_text_bytes: L=%d outside [1, %d]", L, RNAMSM_SS_MAX_L);
    RNAMSM_CHECK_ARG(ct_bytes && bpseq_bytes, "ss_struct_text_bytes: null pointer");
    *ct_bytes = (size_t)sspairs::CT_LINE_MAX * L;
    *bpseq_bytes = (size_t)sspairs::BPSEQ_LINE_MAX * L;
    return RNAMSM_OK;
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
