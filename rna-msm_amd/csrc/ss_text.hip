// RNA-MSM-SS: the text of `<name>.prob` written on the device -- np.savetxt(path, probs, delimiter="\t") of the head's [L, L]
// probabilities, byte for byte.  A sigmoid's output lies in [0, 1], where "%.18e" is always 24 characters (dec19.h: the digits
// as an exact integer computation); behind each comes one '\t', or '\n' behind a row's last column: a flat stream of L*L records
// of 25 bytes.
// One thread per element; a block of 256 consecutive elements owns 6400 contiguous bytes of its member's stream.  The records are
// not 4-byte aligned, so a block stages them in LDS (byte stores there) and sends them out as aligned 16-byte vector stores:
// 6400 = 400 x 16, so every block of a 16-byte aligned text starts on a vector; only the last block of a member has a tail of
// up to 15 single bytes.
// An element outside [0, 1] (sign bit set, -0.0 included; above 1.0; NaN; inf) has no 24-character form: its thread stores 1 to
// the member's fallback word (a plain store of the same value from every such thread: no atomics) and the caller formats that
// matrix on the host.  What is written for such an element is the record of 0.0; the member's text is then unspecified.
// The lone entry point and the packed one run the same kernel: the descriptors travel as kernel arguments, 32 per launch
// (common.h: MemberChunk, member_chunk), and a block finds its member by a search over the block prefix sums (member_of); the
// lone call is a chunk of one.  The entry points take no workspace, so there is no device table: a batch of more than 32 members
// is one pair of launches per 32.
#include "common.h"
#include "dec19.h"

namespace rnamsm {
namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_RECORD = dec19::CHARS + 1;                 // 25: the number and its separator
constexpr int ST_BLOCK_BYTES = ST_THREADS * ST_RECORD;      // 6400
static_assert(ST_BLOCK_BYTES % 16 == 0, "a block's bytes are whole 16-byte vectors");

struct SsTextMember {        // 64 bytes
    const float* probs;      // [L, L]
    uint8_t* text;           // [25 L^2], 16-byte aligned
    int32_t* fallback;
    int32_t L, elems;        // elems = L^2 <= 2^20 (rnamsm_ss_prob_text_long: 2^24)
    int32_t block0;          // blocks of the chunk's members before it
    int32_t pad_[7];
};
static_assert(sizeof(SsTextMember) == 64, "SsTextMember layout");

// the fallback words of a chunk's members, before the first ss_text_kernel of the call
__global__ void ss_text_zero_kernel(const MemberChunk<SsTextMember> chunk, int n) {
    if ((int)threadIdx.x < n) *chunk.m[threadIdx.x].fallback = 0;
}

__global__ __launch_bounds__(ST_THREADS) void ss_text_kernel(const MemberChunk<SsTextMember> chunk, int n) {
    __shared__ uint4 stage4[ST_BLOCK_BYTES / 16];
    uint8_t* stage = reinterpret_cast<uint8_t*>(stage4);
    const SsTextMember m = chunk.m[member_of(chunk.m, n, (int)blockIdx.x, &SsTextMember::block0)];
    const int t = threadIdx.x;
    const int e0 = ((int)blockIdx.x - m.block0) * ST_THREADS;            // the block's first element; e0 < elems by the grid
    const int cnt = m.elems - e0 < ST_THREADS ? m.elems - e0 : ST_THREADS;
    if (t < cnt) {
        const int e = e0 + t;
        uint32_t bits = __float_as_uint(m.probs[e]);
        if (bits > dec19::MAX_BITS) {          // unsigned: the sign bit, NaN and inf are all above 1.0f
            *m.fallback = 1;
            bits = 0;
        }
        uint8_t* rec = stage + t * ST_RECORD;
        dec19::format(bits, rec);
        rec[dec19::CHARS] = e % m.L == m.L - 1 ? '\n' : '\t';
    }
    __syncthreads();
    const int nbytes = cnt * ST_RECORD, nvec = nbytes >> 4;
    uint8_t* out = m.text + (size_t)e0 * ST_RECORD;                       // 6400 x the block's index: 16-byte aligned
    uint4* out4 = reinterpret_cast<uint4*>(out);
    for (int i = t; i < nvec; i += ST_THREADS) out4[i] = stage4[i];
    for (int i = 16 * nvec + t; i < nbytes; i += ST_THREADS) out[i] = stage[i];
}

// Every refusal, then the launches.  who: the entry point's name; lone: the one item is the call's own arguments, not "member 0".
// max_L: the entry point's limit (rnamsm_ss_prob_text_long: RNAMSM_LONG_MAX_L -- elems = L^2 <= 2^24 and the 2^16 blocks of 256
// elements stay int32; a block's byte offset e0 * 25, up to 419 MB, is taken in size_t).
int ss_text_run(const char* who, bool lone, const rnamsm_ss_text_item* items, int B, hipStream_t s, int max_L = RNAMSM_SS_MAX_L) {
    char where[32] = "";
    for (int b = 0; b < B; ++b) {
        const rnamsm_ss_text_item& it = items[b];
        if (!lone) snprintf(where, sizeof(where), "member %d: ", b);
        RNAMSM_CHECK_ARG(it.L >= 1 && it.L <= max_L, "%s: %sL=%d outside [1, %d]", who, where, it.L, max_L);
        RNAMSM_CHECK_ARG(it.probs && it.text && it.fallback, "%s: %snull pointer", who, where);
        RNAMSM_CHECK_ARG(((uintptr_t)it.probs & 3u) == 0 && ((uintptr_t)it.fallback & 3u) == 0,
                         "%s: %sprobs or fallback is not 4-byte aligned", who, where);
        RNAMSM_CHECK_ARG(aligned16(it.text), "%s: %stext is not 16-byte aligned", who, where);
    }
    // the members of chunk b0 .. ; blocks: their blocks in all
    auto chunk_of = [&](int b0, int& n, int& blocks) {
        blocks = 0;
        auto fill = [&](int b) {
            const rnamsm_ss_text_item& it = items[b];
            SsTextMember m = {it.probs, it.text, it.fallback, it.L, it.L * it.L, blocks, {0}};
            blocks += (m.elems + ST_THREADS - 1) / ST_THREADS;
            return m;
        };
        return member_chunk<SsTextMember>(b0, B, fill, n);
    };
    int n, blocks;
    for (int b0 = 0; b0 < B; b0 += 32) {          // every word is zero before any block can set one: members may share a word
        const MemberChunk<SsTextMember> chunk = chunk_of(b0, n, blocks);
        hipLaunchKernelGGL(ss_text_zero_kernel, dim3(1), dim3(32), 0, s, chunk, n);
        RNAMSM_CHECK_LAUNCH("ss_text_zero");
    }
    for (int b0 = 0; b0 < B; b0 += 32) {
        const MemberChunk<SsTextMember> chunk = chunk_of(b0, n, blocks);
        hipLaunchKernelGGL(ss_text_kernel, dim3((unsigned)blocks), dim3(ST_THREADS), 0, s, chunk, n);
        RNAMSM_CHECK_LAUNCH("ss_text");
    }
    return RNAMSM_OK;
}

}  // namespace
}  // namespace rnamsm

using namespace rnamsm;

extern "C" size_t rnamsm_ss_prob_text_bytes(int L) {
    if (L < 1 || L > RNAMSM_SS_MAX_L) return 0;
    return (size_t)ST_RECORD * L * L;
}

extern "C" int rnamsm_ss_prob_text(const float* probs, int L, uint8_t* text, int32_t* fallback, void* stream) {
    const rnamsm_ss_text_item item = {probs, L, text, fallback};
    return ss_text_run("ss_prob_text", true, &item, 1, static_cast<hipStream_t>(stream));
}

// The lone call for L up to RNAMSM_LONG_MAX_L: the same kernel, so the same bytes where both run.
extern "C" size_t rnamsm_ss_prob_text_long_bytes(int L) {
    if (L < 1 || L > RNAMSM_LONG_MAX_L) return 0;
    return (size_t)ST_RECORD * L * L;
}

extern "C" int rnamsm_ss_prob_text_long(const float* probs, int L, uint8_t* text, int32_t* fallback, void* stream) {
    const rnamsm_ss_text_item item = {probs, L, text, fallback};
    return ss_text_run("ss_prob_text_long", true, &item, 1, static_cast<hipStream_t>(stream), RNAMSM_LONG_MAX_L);
}

extern "C" int rnamsm_ss_prob_text_packed(const rnamsm_ss_text_item* items, int B, void* stream) {
    // every refusal comes before the first launch: a refused call leaves the stream and the outputs untouched
    RNAMSM_CHECK_ARG(items, "ss_prob_text_packed: null pointer");
    RNAMSM_CHECK_ARG(B >= 1 && B <= RNAMSM_SS_MAX_BATCH, "ss_prob_text_packed: B=%d outside [1, %d]", B, RNAMSM_SS_MAX_BATCH);
    return ss_text_run("ss_prob_text_packed", false, items, B, static_cast<hipStream_t>(stream));
}
