// RNA-MSM-SS: the structure decoding beyond one base per thread -- the core of ss_pairs_long.hip (rnamsm_ss_pairs_long, L up to
// LONG_MAX_L = 4096).  Plain C++ over ss_pairs.h, which stays as it is: g++ compiles this header for the host test
// (tests/native/ss_pairs_long_check.cpp, which runs the block's LONG_THREADS "threads" serially), hipcc for the kernel.
// One workgroup of LONG_THREADS threads; thread t owns the contiguous bases [first_base(t, L), end_base(t, L)): per = ceil(L /
// LONG_THREADS) of them (1 up to L = 1024 -- thread t is then base t, the existing kernel's assignment --, 4 at the limit), fewer or
// none for the last threads.  A round is ss_pairs.h's, one call per owned base: thread_mark (pick_mark into mark[]), a block-wide
// "any mark", thread_remove (remove_marked).  A thread writes only its own bases' rows and marks.
// The lines: a thread's bases are contiguous, so its lines are one contiguous run of bytes in either body and a prefix scan over
// THREADS of thread_measure's packed lengths gives every thread its two offsets.  The three sums of a structure -- bytes of the .ct
// body (<= 32 L = 2^17), bytes of the .bpseq body (<= 12 L), pairs (<= L / 2) -- share one 64-bit word, 21 bits each (pairs: 22).
#pragma once
#include "ss_pairs.h"

namespace sspairs {

constexpr int LONG_MAX_L = 4096;
constexpr int LONG_THREADS = 1024;
constexpr int LONG_FIELD_BITS = 21;
constexpr uint64_t LONG_FIELD_MASK = (1ull << LONG_FIELD_BITS) - 1;
static_assert((uint64_t)CT_LINE_MAX * LONG_MAX_L <= LONG_FIELD_MASK && (uint64_t)BPSEQ_LINE_MAX * LONG_MAX_L <= LONG_FIELD_MASK,
              "a body's length fits its field");
static_assert(LONG_MAX_L <= 9999, "digits() covers four decimal digits");

SSP_HD inline int bases_per_thread(int L) { return (L + LONG_THREADS - 1) / LONG_THREADS; }
SSP_HD inline int first_base(int t, int L) {
    const int b = t * bases_per_thread(L);
    return b < L ? b : L;
}
SSP_HD inline int end_base(int t, int L) { return first_base(t + 1, L); }

SSP_HD inline uint64_t pack_lens(int ct, int bpseq, int pairs) {
    return (uint64_t)ct | (uint64_t)bpseq << LONG_FIELD_BITS | (uint64_t)pairs << (2 * LONG_FIELD_BITS);
}
SSP_HD inline int ct_of(uint64_t v) { return (int)(v & LONG_FIELD_MASK); }
SSP_HD inline int bpseq_of(uint64_t v) { return (int)(v >> LONG_FIELD_BITS & LONG_FIELD_MASK); }
SSP_HD inline int pairs_of(uint64_t v) { return (int)(v >> (2 * LONG_FIELD_BITS)); }

// First half of a round: thread t marks for each of its bases; true when any of them marked.
template <class M>
SSP_HD inline bool thread_mark(const uint64_t* adj, int W, int t, const float* P, int L, M* mark) {
    bool any = false;
    for (int b = first_base(t, L), e = end_base(t, L); b < e; ++b) {
        const int mine = pick_mark(adj + (size_t)b * W, W, b, P, L);
        mark[b] = mine;
        any = any || mine >= 0;
    }
    return any;
}

// Second half, behind the barrier: thread t clears its own bases' rows.
template <class M>
SSP_HD inline void thread_remove(uint64_t* adj, int W, int t, int L, const M* mark) {
    for (int b = first_base(t, L), e = end_base(t, L); b < e; ++b) remove_marked(adj + (size_t)b * W, W, b, mark);
}

// Once no base has two partners: thread t writes its bases' partners and returns the packed lengths of its lines and its count of
// pairs (each pair counted at its lower base); *bad is set when one of its letters needs the host writer.
SSP_HD inline uint64_t thread_measure(const uint64_t* adj, int W, int t, int L, const uint8_t* letters, int32_t* partner, bool* bad) {
    int ct = 0, bp = 0, pairs = 0;
    for (int b = first_base(t, L), e = end_base(t, L); b < e; ++b) {
        const int p = partner_of(adj + (size_t)b * W, W);
        partner[b] = p;
        pairs += p > b + 1;
        ct += ct_line_len(b + 1, L, p);
        bp += bpseq_line_len(b + 1, p);
        if (letter_needs_host(letters[b])) *bad = true;
    }
    return pack_lens(ct, bp, pairs);
}

// Thread t's lines, from the offsets the scan gave it (before: the packed sums of the threads below t).
SSP_HD inline void thread_put_lines(int t, int L, const uint8_t* letters, const int32_t* partner, uint64_t before, uint8_t* ct,
                                    uint8_t* bpseq) {
    uint8_t* c = ct + ct_of(before);
    uint8_t* q = bpseq + bpseq_of(before);
    for (int b = first_base(t, L), e = end_base(t, L); b < e; ++b) {
        const int p = partner[b];
        put_ct_line(c, b + 1, letters[b], L, p);
        put_bpseq_line(q, b + 1, letters[b], p);
        c += ct_line_len(b + 1, L, p);
        q += bpseq_line_len(b + 1, p);
    }
}

}  // namespace sspairs
