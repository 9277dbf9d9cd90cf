// RNA-MSM-SS: the bodies of `<name>.ct` / `<name>.bpseq` from a partner vector -- everything about the two texts that is not the
// decoding, stated once for ss_pairs.hip, ss_pairs_long.hip and ss_nested.hip.
// The upper part is plain C++: g++ compiles it for the host tests (tests/native/struct_text_check.cpp, and the serial models of the
// three decoders), hipcc for the kernels.  The lower part (hipcc only) is the tail every decoding kernel ends in, and what the three
// entry points refuse alike.
// The lines have variable width.  A thread owns a contiguous run of bases, so its lines are one contiguous run of bytes in either
// body: it measures them (measure_lines), a prefix scan over the threads of the packed lengths gives it its two offsets, and it
// writes its bytes itself (put_lines).  The three sums of a structure -- bytes of the .ct body (<= 32 L = 2^17 at L = 4096), bytes
// of the .bpseq body (<= 12 L), pairs (<= L / 2) -- share one 64-bit word, 21 bits each (pairs: 22).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SSP_HD __host__ __device__
#else
#define SSP_HD
#endif

namespace sspairs {

constexpr int LONG_MAX_L = 4096;                          // the greatest L of any structure
constexpr int CT_LINE_MAX = 32, BPSEQ_LINE_MAX = 12;      // bytes of the longest line at L = LONG_MAX_L

// ---- the lines: "%d\t\t%c\t\t%d\t\t%d\t\t%d\t\t%d\n" of (i, letter, i - 1, i + 1 or 0 on the last line, partner, i) and "%d %c %d\n"
static_assert(LONG_MAX_L <= 9999, "digits() covers four decimal digits");
SSP_HD inline int digits(int v) { return 1 + (v >= 10) + (v >= 100) + (v >= 1000); }      // 0 <= v <= 9999
SSP_HD inline uint8_t* put_int(uint8_t* dst, int v) {
    const int n = digits(v);
    for (int k = n - 1; k >= 0; --k) {
        dst[k] = (uint8_t)('0' + v % 10);
        v /= 10;
    }
    return dst + n;
}
SSP_HD inline uint8_t* put_tabs(uint8_t* dst) {
    dst[0] = '\t';
    dst[1] = '\t';
    return dst + 2;
}
SSP_HD inline int ct_next(int i, int L) { return i == L ? 0 : i + 1; }
SSP_HD inline int ct_line_len(int i, int L, int partner) {
    return 2 * digits(i) + digits(i - 1) + digits(ct_next(i, L)) + digits(partner) + 12;      // ten tabs, the letter, '\n'
}
SSP_HD inline int bpseq_line_len(int i, int partner) { return digits(i) + digits(partner) + 4; }
// i: 1-based; both write exactly *_line_len bytes
SSP_HD inline void put_ct_line(uint8_t* d, int i, uint8_t letter, int L, int partner) {
    d = put_tabs(put_int(d, i));
    *d++ = letter;
    d = put_tabs(d);
    d = put_tabs(put_int(d, i - 1));
    d = put_tabs(put_int(d, ct_next(i, L)));
    d = put_tabs(put_int(d, partner));
    d = put_int(d, i);
    *d = '\n';
}
SSP_HD inline void put_bpseq_line(uint8_t* d, int i, uint8_t letter, int partner) {
    d = put_int(d, i);
    d[0] = ' ';
    d[1] = letter;
    d[2] = ' ';
    d = put_int(d + 3, partner);
    *d = '\n';
}
// a letter the host writer would not print as this one byte: the structure's two tables then come from the host path
SSP_HD inline bool letter_needs_host(uint8_t c) { return c == 0 || c >= 128; }

// ---- who writes what: thread t of T owns the bases [first_base, end_base), ceil(L / T) of them (thread t is base t when L <= T),
// fewer or none for the last threads
SSP_HD inline int bases_per_thread(int L, int T) { return (L + T - 1) / T; }
SSP_HD inline int first_base(int t, int L, int T) {
    const int b = t * bases_per_thread(L, T);
    return b < L ? b : L;
}
SSP_HD inline int end_base(int t, int L, int T) { return first_base(t + 1, L, T); }

// ---- the packed sums
constexpr int FIELD_BITS = 21;
constexpr uint64_t FIELD_MASK = (1ull << FIELD_BITS) - 1;
static_assert((uint64_t)CT_LINE_MAX * LONG_MAX_L <= FIELD_MASK && (uint64_t)BPSEQ_LINE_MAX * LONG_MAX_L <= FIELD_MASK,
              "a body's length fits its field");
SSP_HD inline uint64_t pack_lens(int ct, int bpseq, int pairs) {
    return (uint64_t)ct | (uint64_t)bpseq << FIELD_BITS | (uint64_t)pairs << (2 * FIELD_BITS);
}
SSP_HD inline int ct_of(uint64_t v) { return (int)(v & FIELD_MASK); }
SSP_HD inline int bpseq_of(uint64_t v) { return (int)(v >> FIELD_BITS & FIELD_MASK); }
SSP_HD inline int pairs_of(uint64_t v) { return (int)(v >> (2 * FIELD_BITS)); }
// counts[0 .. 3] of a structure from the sum over all its bases
SSP_HD inline void put_counts(int32_t* counts, uint64_t total, bool bad) {
    counts[0] = pairs_of(total);
    counts[1] = ct_of(total);
    counts[2] = bpseq_of(total);
    counts[3] = bad ? 1 : 0;
}

// The packed lengths of the lines of bases [b0, b1) and their count of pairs (each pair counted at its lower base); *bad is set when
// one of their letters needs the host writer.  partner(b): 0 or the 1-based partner of base b.
template <class Partner>
SSP_HD inline uint64_t measure_lines(int b0, int b1, int L, Partner partner, const uint8_t* letters, bool* bad) {
    int ct = 0, bp = 0, pairs = 0;
    for (int b = b0; b < b1; ++b) {
        const int p = partner(b);
        pairs += p > b + 1;
        ct += ct_line_len(b + 1, L, p);
        bp += bpseq_line_len(b + 1, p);
        if (letter_needs_host(letters[b])) *bad = true;
    }
    return pack_lens(ct, bp, pairs);
}

// The lines of bases [b0, b1), from the offsets in `before`: the packed sum of measure_lines over the bases below b0.
template <class Partner>
SSP_HD inline void put_lines(int b0, int b1, int L, Partner partner, const uint8_t* letters, uint64_t before, uint8_t* ct,
                             uint8_t* bpseq) {
    uint8_t* c = ct + ct_of(before);
    uint8_t* q = bpseq + bpseq_of(before);
    for (int b = b0; b < b1; ++b) {
        const int p = partner(b);
        put_ct_line(c, b + 1, letters[b], L, p);
        put_bpseq_line(q, b + 1, letters[b], p);
        c += ct_line_len(b + 1, L, p);
        q += bpseq_line_len(b + 1, p);
    }
}

}  // namespace sspairs

#if defined(__HIPCC__)
#include "block_scan.h"

namespace rnamsm {

// The tail of a decoding kernel, called by every thread of the block: the thread's bases [b0, b1) become their lines in the two
// bodies, and thread 0 writes counts[0 .. 3].  scan: blockDim.x / 64 words of LDS, free again after the caller's next barrier.
template <class Partner>
__device__ __forceinline__ void emit_struct_text(int L, int b0, int b1, Partner partner, const uint8_t* letters, uint8_t* ct,
                                                 uint8_t* bpseq, int32_t* counts, uint64_t* scan) {
    bool bad = false;
    const uint64_t len = sspairs::measure_lines(b0, b1, L, partner, letters, &bad);
    const int any_bad = __syncthreads_or(bad);
    uint64_t total;
    const uint64_t before = block_exclusive_sum(len, scan, total);
    sspairs::put_lines(b0, b1, L, partner, letters, before, ct, bpseq);
    if (threadIdx.x == 0) sspairs::put_counts(counts, total, any_bad != 0);
}

// ---- what the entry points of the three decoders refuse alike (host code)
// One structure: L within the entry point's limit, the six pointers of the item (and dbn, where the entry point has one: pass its
// address), the three 4-byte alignments.  who: the entry point's name; where: "" or "member b: ".
inline int check_struct_item(const char* who, const char* where, int max_L, const rnamsm_ss_pairs_item& it,
                             const uint8_t* const* dbn = nullptr) {
    RNAMSM_CHECK_ARG(it.L >= 1 && it.L <= max_L, "%s: %sL=%d outside [1, %d]", who, where, it.L, max_L);
    const struct {
        const char* name;
        const void* p;
        bool words;
    } ptrs[7] = {{"probs", it.probs, true}, {"letters", it.letters, false}, {"partner", it.partner, true}, {"counts", it.counts, true},
                 {"ct", it.ct, false},      {"bpseq", it.bpseq, false},     {"dbn", dbn ? *dbn : nullptr, false}};
    const int n = dbn ? 7 : 6;
    for (int k = 0; k < n; ++k) RNAMSM_CHECK_ARG(ptrs[k].p, "%s: %snull pointer (%s)", who, where, ptrs[k].name);
    for (int k = 0; k < n; ++k)
        RNAMSM_CHECK_ARG(!ptrs[k].words || ((uintptr_t)ptrs[k].p & 3u) == 0, "%s: %s%s is not 4-byte aligned", who, where, ptrs[k].name);
    return RNAMSM_OK;
}
// The call's workspace, once the items have passed: need = the bytes they ask for.
inline int check_struct_workspace(const char* who, const void* workspace, size_t workspace_bytes, size_t need) {
    RNAMSM_CHECK_ARG(workspace, "%s: null pointer (workspace)", who);
    RNAMSM_CHECK_ARG(aligned16(workspace), "%s: workspace is not 16-byte aligned", who);
    RNAMSM_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    return RNAMSM_OK;
}
// rnamsm_ss_struct_text_bytes / rnamsm_ss_struct_text_long_bytes
inline int struct_text_bytes(const char* who, int max_L, int L, size_t* ct_bytes, size_t* bpseq_bytes) {
    RNAMSM_CHECK_ARG(L >= 1 && L <= max_L, "%s: L=%d outside [1, %d]", who, L, max_L);
    RNAMSM_CHECK_ARG(ct_bytes && bpseq_bytes, "%s: null pointer", who);
    *ct_bytes = (size_t)sspairs::CT_LINE_MAX * L;
    *bpseq_bytes = (size_t)sspairs::BPSEQ_LINE_MAX * L;
    return RNAMSM_OK;
}

}  // namespace rnamsm
#endif
