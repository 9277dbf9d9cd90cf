// The word form of an alignment's rows and the per-word counts of csrc/msa_pdist.hip and csrc/seqid_filter.hip, compilable on the
// host (tests/native/msa_pdist_words_check.cpp and tests/native/seqid_words_check.cpp run it against byte loops under
// AddressSanitizer + UBSan).
//
// A row of the alignment is kept eight bytes to a 64-bit word: byte k of word w (bits 8k .. 8k + 7) is column 8w + k, and a column
// past L is a zero byte in every row.  The bytes go through a recoding that makes the GAP the zero byte: the gap's value becomes 0, a
// zero byte takes the gap's value, every other byte stays.  The recoding is one-to-one, so two bytes are equal after it iff they were
// before; with gap = 0 it changes nothing and the word holds the bytes AS THEY ARE.  With nz(x) = bit 7 of every non-zero byte of x:
//   mismatches = popcount(nz(a ^ b))                 columns where the rows differ (any gap, the zero tail counts nothing)
//   both = popcount(nz(a) & nz(b))                   columns where neither row has the gap (a column past L counts as a gap)
//   same = popcount(nz(a) & nz(b) & ~nz(a ^ b))      ... and the two bytes are equal
// Sums of these over a row's words are m(i, j) of the Hamming matrix and both(i, j), same(i, j) of the filter's rule: integers, no
// symbol table, any byte values, any number of them.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MW_HD __host__ __device__ __forceinline__
#else
#define MW_HD inline
#endif

namespace rnamsm {

// bit 7 of every byte of x that is not zero.  Per byte: the low seven bits plus 0x7f carry into bit 7 iff one of them is set (the
// sum is at most 0xfe: nothing crosses into the next byte), and the OR with x brings in a byte whose only set bit is bit 7 itself.
MW_HD uint32_t nonzero_bytes32(uint32_t x) { return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }

// one byte, recoded: gap -> 0, 0 -> gap, anything else as it is (gap = 0: nothing changes)
MW_HD uint8_t recode(uint8_t b, int gap) { return b == (uint8_t)gap ? (uint8_t)0 : (b == 0 ? (uint8_t)gap : b); }

// the recoded word of the columns c0 .. c0 + 7 of a row whose first column is at `row`: the n = min(8, L - c0) bytes that exist
// (n <= 0: none), zeros -- gaps -- above them.  Nothing at or past row[c0 + n] is read.
MW_HD uint64_t pack_word(const uint8_t* row, int c0, int n, int gap) {
    uint64_t w = 0;
    for (int k = 0; k < 8; ++k)
        if (k < n) w |= (uint64_t)recode(row[c0 + k], gap) << (8 * k);
    return w;
}

// padded rows and words of the word-major planes P[w][row] that a 64 x 64 tile loop of WK words per step reads
struct WordDims {
    int64_t Np;      // rows, a multiple of 64
    int Wp;          // words, a multiple of WK
};
inline WordDims word_dims(int N, int L, int WK) { return {((int64_t)N + 63) / 64 * 64, ((L + 7) / 8 + WK - 1) / WK * WK}; }

// the number of byte positions in which a and b differ, 0 .. 8
MW_HD int pd_mismatches(uint64_t a, uint64_t b) {
    const uint64_t x = a ^ b;
    return __builtin_popcount(nonzero_bytes32((uint32_t)x)) + __builtin_popcount(nonzero_bytes32((uint32_t)(x >> 32)));
}

// bit 7 of every non-zero byte of x, as two halves
MW_HD uint32_t sq_residues_lo(uint64_t x) { return nonzero_bytes32((uint32_t)x); }
MW_HD uint32_t sq_residues_hi(uint64_t x) { return nonzero_bytes32((uint32_t)(x >> 32)); }

// the number of residues (non-gap bytes) of a word, 0 .. 8
MW_HD int sq_residues(uint64_t a) { return __builtin_popcount(sq_residues_lo(a)) + __builtin_popcount(sq_residues_hi(a)); }

// both and same of a pair of words, 0 .. 8 each, same <= both
MW_HD void sq_pair(uint64_t a, uint64_t b, int* both, int* same) {
    const uint64_t x = a ^ b;
    const uint32_t ml = sq_residues_lo(a) & sq_residues_lo(b), mh = sq_residues_hi(a) & sq_residues_hi(b);
    *both = __builtin_popcount(ml) + __builtin_popcount(mh);
    *same = __builtin_popcount(ml & ~sq_residues_lo(x)) + __builtin_popcount(mh & ~sq_residues_hi(x));
}

// row k is redundant to row j at threshold t (a percentage): int32 throughout -- same <= both <= 32768, t <= 100
MW_HD bool sq_redundant(int both, int same, int t) { return both > 0 && 100 * same >= t * both; }

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
