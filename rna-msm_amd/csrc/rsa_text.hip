// RNA-MSM RSA: the bodies of the `RSA_result` tables written on the device -- the K member tables and the ensemble table of
// write_rsa_files (rnamsm/rsa.py), byte for byte: the float64 arithmetic and the lines are rsa_text.h's.
// One workgroup per (alignment, table), 256 threads, a thread per position and as many passes of 256 positions as L needs.  The
// lines have unlike lengths (1 to 4 index digits, 4 to 6 ASA characters): within a pass a block prefix scan of the lengths gives
// every thread its offset (block_scan.h: block_exclusive_sum), a running base carries over from pass to pass, and the thread writes
// its bytes itself.
// The ensemble table's workgroup recomputes the K products from the members' values: no workgroup reads what another wrote, and
// one launch does everything.  It reads every value and every letter of the alignment, so it alone decides the two flag words and
// writes each once (plain stores, no atomics, nothing to zero first).
// A value outside [0, 1] (sign bit set, NaN, inf) is formatted as 1.0 and a letter outside ACGUT scaled as U: every line then still
// fits its bound (and no zero is made up); the fallback word says that the bodies are not to be used.
// The lone entry point and the packed one run the same kernel: the descriptors travel as kernel arguments, 32 per launch
// (common.h: MemberChunk, member_chunk); workgroup b serves table b % (K + 1) of the chunk's member b / (K + 1).
#include "block_scan.h"
#include "common.h"
#include "rsa_text.h"

namespace rnamsm {
namespace {

static_assert(rsatext::MAX_L == RNAMSM_RSA_MAX_L && rsatext::MAX_MODELS == RNAMSM_RSA_MAX_MODELS, "one set of limits");
static_assert(rsatext::LINE_BYTES == RNAMSM_RSA_TEXT_LINE_MAX, "one bound");
static_assert(rsatext::LONG_MAX_L == RNAMSM_LONG_MAX_L, "one long limit");
// the kernel's running base and prefix scan are uint32 byte counts within one body, and k * L + p an int index of the values
static_assert((uint64_t)rsatext::LINE_BYTES * rsatext::LONG_MAX_L < (1ull << 31) &&
              (uint64_t)rsatext::MAX_MODELS * rsatext::LONG_MAX_L < (1ull << 31), "32-bit offsets at the long limit");

constexpr int RT_THREADS = 256;

struct RsaTextMember {       // 64 bytes
    const float* rsa;        // [K, L]
    const uint8_t* letters;  // [L]
    uint8_t* text;           // [(K + 1) x LINE_BYTES L]
    int32_t* counts;         // [K + 3]
    double* ens;             // [2, L] or null
    int32_t L;
    int32_t pad_[5];
};
static_assert(sizeof(RsaTextMember) == 64, "RsaTextMember layout");

__global__ __launch_bounds__(RT_THREADS) void rsa_text_kernel(const MemberChunk<RsaTextMember> chunk, int K) {
    __shared__ uint32_t scan[RT_THREADS / 64];
    const int tables = K + 1;
    const RsaTextMember m = chunk.m[blockIdx.x / tables];
    const int f = blockIdx.x % tables, L = m.L;
    const int t = threadIdx.x;
    const bool ensemble = f == K;
    uint8_t* body = m.text + (size_t)f * rsatext::LINE_BYTES * L;
    const uint32_t* rsa_bits = reinterpret_cast<const uint32_t*>(m.rsa);

    uint32_t base = 0;
    bool bad = false, zero = false;
    for (int p0 = 0; p0 < L; p0 += RT_THREADS) {            // uniform: every thread takes every pass
        const int p = p0 + t;
        uint8_t letter = 0;
        rsatext::Line ln = {0u, 0u};
        uint32_t len = 0;
        if (p < L) {
            letter = m.letters[p];
            int scale = rsatext::scale_of(letter);
            if (!scale) {
                bad = true;
                scale = 350;
            }
            double asa, rsa;
            if (ensemble) {
                auto value_of = [&](int k) {
                    uint32_t bits = rsa_bits[k * L + p];
                    if (rsatext::outside_domain(bits)) {
                        bad = true;
                        bits = rsatext::ONE_BITS;
                    }
                    return rsatext::float_of(bits);
                };
                rsatext::ensemble_values(value_of, K, scale, asa, rsa, zero);
                if (m.ens) {
                    m.ens[p] = asa;
                    m.ens[L + p] = rsa;
                }
            } else {
                uint32_t bits = rsa_bits[f * L + p];
                if (rsatext::outside_domain(bits)) bits = rsatext::ONE_BITS;
                rsatext::member_values(rsatext::float_of(bits), scale, asa, rsa);
            }
            ln = rsatext::line_of(asa, rsa);
            len = (uint32_t)rsatext::line_len(p + 1, ln);
        }
        uint32_t total;
        const uint32_t before = block_exclusive_sum(len, scan, total);
        if (p < L) rsatext::put_line(body + (base + before), p + 1, letter, ln);      // base + before + len <= LINE_BYTES L
        base += total;
        __syncthreads();                                      // the scan's words are written again in the next pass
    }
    if (t == 0) m.counts[f] = (int32_t)base;
    if (ensemble) {                                           // block-uniform
        const int any_bad = __syncthreads_or(bad), any_zero = __syncthreads_or(zero);
        if (t == 0) {
            m.counts[K + 1] = any_bad ? 1 : 0;
            m.counts[K + 2] = any_zero ? 1 : 0;
        }
    }
}

// Every refusal, then the launches.  who: the entry point's name; lone: the one item is the call's own arguments, not "member 0";
// max_L: the entry point's limit (the kernel is one for every L: as many passes of 256 positions as L needs).
int rsa_text_run(const char* who, bool lone, const rnamsm_rsa_text_item* items, int B, int n_models, hipStream_t s,
                 int max_L = RNAMSM_RSA_MAX_L) {
    RNAMSM_CHECK_ARG(n_models >= 1 && n_models <= RNAMSM_RSA_MAX_MODELS, "%s: n_models=%d outside [1, %d]", who, n_models,
                     RNAMSM_RSA_MAX_MODELS);
    char where[32] = "";
    for (int b = 0; b < B; ++b) {
        const rnamsm_rsa_text_item& it = items[b];
        if (!lone) snprintf(where, sizeof(where), "member %d: ", b);
        RNAMSM_CHECK_ARG(it.L >= 1 && it.L <= max_L, "%s: %sL=%d outside [1, %d]", who, where, it.L, max_L);
        RNAMSM_CHECK_ARG(it.rsa && it.letters && it.text && it.counts, "%s: %snull pointer", who, where);
        RNAMSM_CHECK_ARG(((uintptr_t)it.rsa & 3u) == 0 && ((uintptr_t)it.counts & 3u) == 0, "%s: %srsa or counts is not 4-byte aligned",
                         who, where);
        RNAMSM_CHECK_ARG(((uintptr_t)it.ens & 7u) == 0, "%s: %sens is not 8-byte aligned", who, where);
        RNAMSM_CHECK_ARG(aligned16(it.text), "%s: %stext is not 16-byte aligned", who, where);
    }
    for (int b0 = 0; b0 < B; b0 += 32) {
        int n;
        auto fill = [&](int b) {
            const rnamsm_rsa_text_item& it = items[b];
            return RsaTextMember{it.rsa, it.letters, it.text, it.counts, it.ens, it.L, {0}};
        };
        const MemberChunk<RsaTextMember> chunk = member_chunk<RsaTextMember>(b0, B, fill, n);
        hipLaunchKernelGGL(rsa_text_kernel, dim3((unsigned)(n * (n_models + 1))), dim3(RT_THREADS), 0, s, chunk, n_models);
        RNAMSM_CHECK_LAUNCH("rsa_text");
    }
    return RNAMSM_OK;
}

}  // namespace
}  // namespace rnamsm

using namespace rnamsm;

extern "C" size_t rnamsm_rsa_text_bytes(int L, int n_models) {
    if (L < 1 || L > RNAMSM_RSA_MAX_L || n_models < 1 || n_models > RNAMSM_RSA_MAX_MODELS) return 0;
    return (size_t)(n_models + 1) * RNAMSM_RSA_TEXT_LINE_MAX * L;
}

extern "C" int rnamsm_rsa_text(const float* rsa, const uint8_t* letters, int L, int n_models, uint8_t* text, int32_t* counts,
                               double* ens, void* stream) {
    const rnamsm_rsa_text_item item = {rsa, letters, L, text, counts, ens};
    return rsa_text_run("rsa_text", true, &item, 1, n_models, static_cast<hipStream_t>(stream));
}

extern "C" size_t rnamsm_rsa_text_long_bytes(int L, int n_models) {
    if (L < 1 || L > RNAMSM_LONG_MAX_L || n_models < 1 || n_models > RNAMSM_RSA_MAX_MODELS) return 0;
    return (size_t)(n_models + 1) * RNAMSM_RSA_TEXT_LINE_MAX * L;
}

extern "C" int rnamsm_rsa_text_long(const float* rsa, const uint8_t* letters, int L, int n_models, uint8_t* text, int32_t* counts,
                                    double* ens, void* stream) {
    const rnamsm_rsa_text_item item = {rsa, letters, L, text, counts, ens};
    return rsa_text_run("rsa_text_long", true, &item, 1, n_models, static_cast<hipStream_t>(stream), RNAMSM_LONG_MAX_L);
}

extern "C" int rnamsm_rsa_text_packed(const rnamsm_rsa_text_item* items, int B, int n_models, void* stream) {
    // every refusal comes before the first launch: a refused call leaves the stream and the outputs untouched
    RNAMSM_CHECK_ARG(items, "rsa_text_packed: null pointer");
    RNAMSM_CHECK_ARG(B >= 1 && B <= RNAMSM_RSA_MAX_BATCH, "rsa_text_packed: B=%d outside [1, %d]", B, RNAMSM_RSA_MAX_BATCH);
    return rsa_text_run("rsa_text_packed", false, items, B, n_models, static_cast<hipStream_t>(stream));
}
