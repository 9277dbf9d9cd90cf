// The word form of csrc/msa_pdist.hip and its per-word mismatch count, compilable on the host (tests/native/msa_pdist_words_check.cpp
// runs it against a byte loop under AddressSanitizer + UBSan).
//
// A row of the alignment is kept as its bytes AS THEY ARE, eight per 64-bit word: byte k of word w (bits 8k .. 8k + 7) is column
// 8w + k, and a column past L is a zero byte in every row.  Two rows differ in a column iff the XOR of their words has a non-zero
// byte there, so m(i, j) = sum over the words of "non-zero bytes of a ^ b": no symbol table, any byte values, any number of them, and
// the zero tail counts nothing.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PD_HD __host__ __device__ __forceinline__
#else
#define PD_HD inline
#endif

namespace rnamsm {

// bit 7 of every byte of x that is not zero.  Per byte: the low seven bits plus 0x7f carry into bit 7 iff one of them is set (the
// sum is at most 0xfe: nothing crosses into the next byte), and the OR with x brings in a byte whose only set bit is bit 7 itself.
PD_HD uint32_t pd_nonzero_bytes32(uint32_t x) { return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }

// the number of byte positions in which a and b differ, 0 .. 8
PD_HD int pd_mismatches(uint64_t a, uint64_t b) {
    const uint64_t x = a ^ b;
    return __builtin_popcount(pd_nonzero_bytes32((uint32_t)x)) + __builtin_popcount(pd_nonzero_bytes32((uint32_t)(x >> 32)));
}

// the word of the columns c0 .. c0 + 7 of a row whose first column is at `row`: the n = min(8, L - c0) bytes that exist (n <= 0:
// none), zeros above them.  Nothing at or past row[c0 + n] is read.
PD_HD uint64_t pd_pack_word(const uint8_t* row, int c0, int n) {
    uint64_t w = 0;
    for (int k = 0; k < 8; ++k)
        if (k < n) w |= (uint64_t)row[c0 + k] << (8 * k);
    return w;
}

}  // namespace rnamsm
