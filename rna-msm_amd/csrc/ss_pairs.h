// RNA-MSM-SS: base pairs from the [L, L] probabilities -- the core of ss_pairs.hip (the lines of `<name>.ct` / `<name>.bpseq` that
// follow from them: struct_text.h).  Plain C++: g++ compiles it for the host test (tests/native/ss_pairs_check.cpp, which runs the
// round logic serially over the "threads"), hipcc for the kernel.
// The reference's post-processing (processing_output.py: the upper triangle above 0.516, then multiplets_free_bp) as a graph process:
//   edges    {i, j}, i < j, iff P[i, j] > float32(0.516), compared in float32 (0.515999972... lies below the double 0.516, so the
//            reference's float64 compare of a float32 agrees on every pattern); NaN is never an edge, +inf is one
//   a round  every base of degree >= 2 marks its incident edge of lowest probability, on equal values the one to the lowest partner
//            (vals.index(min(vals)) over the base's pairs in np.triu_indices order = its partners in ascending order); all marked
//            edges go at once
//   until no base has degree >= 2: at most L - 2 rounds, since every round lowers the largest degree by one.
// The adjacency is a symmetric bit matrix, row b = words(L) 64-bit words; base b's "thread" reads P, its own row and everybody's mark,
// and writes its own row and its own mark only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "struct_text.h"

namespace sspairs {

constexpr int MAX_L = 1024;
constexpr float THRESHOLD = 0.516f;

SSP_HD inline int words(int L) { return (L + 63) >> 6; }
// the workspace of one structure: its adjacency matrix, rounded up to 256 bytes
SSP_HD inline size_t adj_bytes(int L) { return ((size_t)L * words(L) * 8 + 255) & ~(size_t)255; }
// only the upper triangle is ever read
SSP_HD inline float pair_prob(const float* P, int L, int a, int b) { return a < b ? P[a * L + b] : P[b * L + a]; }
SSP_HD inline bool edge_at(const float* P, int L, int b, int p) { return p < L && p != b && pair_prob(P, L, b, p) > THRESHOLD; }

// The partner base b marks this round, or -1 when its degree is below 2.
SSP_HD inline int pick_mark(const uint64_t* row, int W, int b, const float* P, int L) {
    int deg = 0;
    for (int w = 0; w < W; ++w) deg += __builtin_popcountll(row[w]);
    if (deg < 2) return -1;
    int best = -1;
    float best_v = 0.f;
    for (int w = 0; w < W; ++w)
        for (uint64_t m = row[w]; m; m &= m - 1) {
            const int p = 64 * w + __builtin_ctzll(m);
            const float v = pair_prob(P, L, b, p);
            if (best < 0 || v < best_v) {          // strict: the lowest partner keeps an equal value
                best = p;
                best_v = v;
            }
        }
    return best;
}

// Base b's row after the round: without the edge it marked and without every edge a neighbour marked towards it.
template <class M>
SSP_HD inline void remove_marked(uint64_t* row, int W, int b, const M* mark) {
    const int mine = mark[b];
    for (int w = 0; w < W; ++w) {
        uint64_t keep = row[w];
        for (uint64_t m = keep; m; m &= m - 1) {
            const int bit = __builtin_ctzll(m), p = 64 * w + bit;
            if (p == mine || mark[p] == b) keep &= ~(1ull << bit);
        }
        row[w] = keep;
    }
}

// The .ct / .bpseq column of base b once no base has two partners: 0 = unpaired, else the partner's 1-based index.
SSP_HD inline int partner_of(const uint64_t* row, int W) {
    for (int w = 0; w < W; ++w)
        if (row[w]) return 64 * w + __builtin_ctzll(row[w]) + 1;
    return 0;
}

}  // namespace sspairs
