// The word form of csrc/seqid_filter.hip and its per-word pair counts, compilable on the host (tests/native/seqid_words_check.cpp
// runs it against a byte loop under AddressSanitizer + UBSan).
//
// A row of the alignment is kept eight bytes to a 64-bit word -- byte k of word w (bits 8k .. 8k + 7) is column 8w + k -- after a
// recoding that makes the GAP the zero byte: the gap's value becomes 0, a zero byte takes the gap's value, every other byte stays.
// The recoding is one-to-one, so two bytes are equal after it iff they were before, and a column past L, a zero byte in every row,
// counts as a gap.  Per pair of words, with nz(x) = bit 7 of every non-zero byte of x:
//   both = popcount(nz(a) & nz(b))                   columns where neither row has the gap
//   same = popcount(nz(a) & nz(b) & ~nz(a ^ b))      ... and the two bytes are equal
// Sums of these over a row's words are both(i, j) and same(i, j) of the filter's rule: integers, no symbol table, any byte values.
#pragma once
#include <stdint.h>

#include "msa_pdist_words.h"

namespace rnamsm {

// one byte, recoded: gap -> 0, 0 -> gap, anything else as it is (gap = 0: nothing changes)
PD_HD uint8_t sq_recode(uint8_t b, int gap) { return b == (uint8_t)gap ? (uint8_t)0 : (b == 0 ? (uint8_t)gap : b); }

// the recoded word of the columns c0 .. c0 + 7 of a row whose first column is at `row`: the n = min(8, L - c0) bytes that exist
// (n <= 0: none), zeros -- gaps -- above them.  Nothing at or past row[c0 + n] is read.
PD_HD uint64_t sq_pack_word(const uint8_t* row, int c0, int n, int gap) {
    uint64_t w = 0;
    for (int k = 0; k < 8; ++k)
        if (k < n) w |= (uint64_t)sq_recode(row[c0 + k], gap) << (8 * k);
    return w;
}

// bit 7 of every non-zero byte of x, as two halves
PD_HD uint32_t sq_residues_lo(uint64_t x) { return pd_nonzero_bytes32((uint32_t)x); }
PD_HD uint32_t sq_residues_hi(uint64_t x) { return pd_nonzero_bytes32((uint32_t)(x >> 32)); }

// the number of residues (non-gap bytes) of a word, 0 .. 8
PD_HD int sq_residues(uint64_t a) { return __builtin_popcount(sq_residues_lo(a)) + __builtin_popcount(sq_residues_hi(a)); }

// both and same of a pair of words, 0 .. 8 each, same <= both
PD_HD void sq_pair(uint64_t a, uint64_t b, int* both, int* same) {
    const uint64_t x = a ^ b;
    const uint32_t ml = sq_residues_lo(a) & sq_residues_lo(b), mh = sq_residues_hi(a) & sq_residues_hi(b);
    *both = __builtin_popcount(ml) + __builtin_popcount(mh);
    *same = __builtin_popcount(ml & ~sq_residues_lo(x)) + __builtin_popcount(mh & ~sq_residues_hi(x));
}

// row k is redundant to row j at threshold t (a percentage): int32 throughout -- same <= both <= 32768, t <= 100
PD_HD bool sq_redundant(int both, int same, int t) { return both > 0 && 100 * same >= t * both; }

// The thresholds of the walk, ascending: num_seqs > 0: min_seqid, min_seqid + step, ... while below max_seqid, then max_seqid;
// num_seqs == 0, or min_seqid >= max_seqid: max_seqid alone.  out holds at most 100 (1 <= min_seqid, max_seqid <= 100, step >= 1).
inline int sq_thresholds(int num_seqs, int min_seqid, int max_seqid, int step, int* out) {
    int n = 0;
    if (num_seqs > 0)
        for (int t = min_seqid; t < max_seqid; t += step) out[n++] = t;
    out[n++] = max_seqid;
    return n;
}

}  // namespace rnamsm
