// RNA-MSM-SS: the structure decoding beyond one base per thread -- the core of ss_pairs_long.hip (rnamsm_ss_pairs_long, L up to
// LONG_MAX_L = 4096).  Plain C++ over ss_pairs.h, which stays as it is: g++ compiles this header for the host test
// (tests/native/ss_pairs_long_check.cpp, which runs the block's LONG_THREADS "threads" serially), hipcc for the kernel.
// One workgroup of LONG_THREADS threads; thread t owns the contiguous bases struct_text.h's rule gives it: ceil(L / LONG_THREADS) of
// them (1 up to L = 1024 -- thread t is then base t, the existing kernel's assignment --, 4 at the limit), fewer or none for the last
// threads.  A round is ss_pairs.h's, one call per owned base: thread_mark (pick_mark into mark[]), a block-wide "any mark",
// thread_remove (remove_marked).  A thread writes only its own bases' rows and marks.  Once no base has two partners, thread_partners
// writes the partner vector, and the lines follow from it (struct_text.h).
#pragma once
#include "ss_pairs.h"

namespace sspairs {

constexpr int LONG_THREADS = 1024;

// First half of a round: thread t marks for each of its bases; true when any of them marked.
template <class M>
SSP_HD inline bool thread_mark(const uint64_t* adj, int W, int t, const float* P, int L, M* mark) {
    bool any = false;
    for (int b = first_base(t, L, LONG_THREADS), e = end_base(t, L, LONG_THREADS); b < e; ++b) {
        const int mine = pick_mark(adj + (size_t)b * W, W, b, P, L);
        mark[b] = mine;
        any = any || mine >= 0;
    }
    return any;
}

// Second half, behind the barrier: thread t clears its own bases' rows.
template <class M>
SSP_HD inline void thread_remove(uint64_t* adj, int W, int t, int L, const M* mark) {
    for (int b = first_base(t, L, LONG_THREADS), e = end_base(t, L, LONG_THREADS); b < e; ++b)
        remove_marked(adj + (size_t)b * W, W, b, mark);
}

// Once no base has two partners: thread t writes its bases' partners.
SSP_HD inline void thread_partners(const uint64_t* adj, int W, int t, int L, int32_t* partner) {
    for (int b = first_base(t, L, LONG_THREADS), e = end_base(t, L, LONG_THREADS); b < e; ++b)
        partner[b] = partner_of(adj + (size_t)b * W, W);
}

}  // namespace sspairs
