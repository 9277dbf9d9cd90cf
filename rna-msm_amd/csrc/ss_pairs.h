// RNA-MSM-SS: base pairs from the [L, L] probabilities, and the lines of `<name>.ct` / `<name>.bpseq` -- the core of ss_pairs.hip.
// Plain C++: g++ compiles it for the host test (tests/native/ss_pairs_check.cpp, which runs the round logic serially over the
// "threads"), hipcc for the kernel.
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
#include <stdint.h>

#if defined(__HIPCC__)
#define SSP_HD __host__ __device__
#else
#define SSP_HD
#endif

namespace sspairs {

constexpr int MAX_L = 1024;
constexpr float THRESHOLD = 0.516f;
constexpr int CT_LINE_MAX = 32, BPSEQ_LINE_MAX = 12;      // bytes of the longest line at L = MAX_L

SSP_HD inline int words(int L) { return (L + 63) >> 6; }
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

// ---- the lines: "%d\t\t%c\t\t%d\t\t%d\t\t%d\t\t%d\n" of (i, letter, i - 1, i + 1 or 0 on the last line, partner, i) and "%d %c %d\n"
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

}  // namespace sspairs
