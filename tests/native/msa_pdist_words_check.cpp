// Host check of csrc/msa_words.h with gap = 0, the word form and the per-word mismatch count of csrc/msa_pdist.hip, against a byte loop.
// Built by tests/test_msa_stats_host.py with g++ -fsanitize=address,undefined and run as a program of its own.
//   1. every one of the 65 536 pairs of byte values in every one of the eight lanes of a word, the other lanes equal (count 0 or 1)
//      and the other lanes all different (count 7 or 8);
//   2. rows of every length L = 1 .. 40 (every L mod 8, more than one word) in buffers of exactly L bytes -- AddressSanitizer
//      sees a read past a row -- packed and counted against the byte loop, over the byte values that break a SWAR mask;
//   3. the same rows inside a wider buffer whose bytes past L differ: the tail counts nothing;
//   4. every tail length n = 0 .. 8 (and below 0): pack_word with gap = 0 is the bytes as they are, zeros above them, from a buffer
//      of exactly n bytes.
// Prints "ok <checks>" and exits 0, or the first difference and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../rna-msm_amd/csrc/msa_words.h"

using namespace rnamsm;

static long checks = 0;

static int fail(const char* what, long a, long b, long c, long d) {
    printf("FAIL %s: %ld %ld got %ld want %ld\n", what, a, b, c, d);
    return 1;
}

static int count_row(const uint8_t* a, const uint8_t* b, int L) {
    int m = 0;
    for (int w = 0; 8 * w < L; ++w) m += pd_mismatches(pack_word(a, 8 * w, L - 8 * w, 0), pack_word(b, 8 * w, L - 8 * w, 0));
    return m;
}

int main() {
    // 1. all byte pairs, all lanes
    for (int lane = 0; lane < 8; ++lane)
        for (int p = 0; p < 256; ++p)
            for (int q = 0; q < 256; ++q) {
                const uint64_t same = 0x8000ff017f80a55aull & ~(0xffull << (8 * lane));
                const uint64_t a = same | ((uint64_t)p << (8 * lane)), b = same | ((uint64_t)q << (8 * lane));
                int got = pd_mismatches(a, b), want = p != q;
                if (got != want) return fail("lane, others equal", p, q, got, want);
                // the other lanes all different, by bit 7 alone or by bit 0 alone (0x80 / 0x00, 0x01 / 0x00, 0xff / 0x7f, ...)
                const uint64_t oa = 0x8001ff7f00ff8001ull & ~(0xffull << (8 * lane));
                const uint64_t od = (oa ^ 0x8001800180018001ull) & ~(0xffull << (8 * lane));
                got = pd_mismatches(oa | ((uint64_t)p << (8 * lane)), od | ((uint64_t)q << (8 * lane)));
                want = 7 + (p != q);
                if (got != want) return fail("lane, others differ", p, q, got, want);
                checks += 2;
            }
    // 2. and 3. rows of every length, exact buffers and padded ones
    const uint8_t vals[6] = {0x00, 0x01, 0x7f, 0x80, 0xff, 0x2d};
    uint32_t state = 12345u;
    for (int L = 1; L <= 40; ++L)
        for (int rep = 0; rep < 200; ++rep) {
            std::vector<uint8_t> a(L), b(L);
            int want = 0;
            for (int c = 0; c < L; ++c) {
                state = state * 1664525u + 1013904223u;
                a[c] = vals[(state >> 16) % 6];
                state = state * 1664525u + 1013904223u;
                b[c] = (state >> 28) < 6 ? a[c] : vals[(state >> 16) % 6];
                want += a[c] != b[c];
            }
            int got = count_row(a.data(), b.data(), L);
            if (got != want) return fail("exact rows", L, rep, got, want);
            std::vector<uint8_t> pa(L + 9, 0xee), pb(L + 9, 0x11);       // guard bytes that differ everywhere
            for (int c = 0; c < L; ++c) { pa[c] = a[c]; pb[c] = b[c]; }
            got = count_row(pa.data(), pb.data(), L);
            if (got != want) return fail("padded rows", L, rep, got, want);
            checks += 2;
        }
    // 4. gap = 0 packs the bytes as they are: every tail length, exact buffers, every byte value in every lane
    for (int n = -3; n <= 8; ++n)
        for (int rep = 0; rep < 256; ++rep) {
            const int len = n < 0 ? 0 : n;
            std::vector<uint8_t> buf(len);
            uint64_t want = 0;
            for (int k = 0; k < len; ++k) {
                state = state * 1664525u + 1013904223u;
                buf[k] = k == rep % 8 ? (uint8_t)rep : (uint8_t)(state >> 16);
                want |= (uint64_t)buf[k] << (8 * k);
            }
            const uint64_t got = pack_word(buf.data(), 0, n, 0);
            if (got != want) return fail("gap 0 tail", n, rep, (long)got, (long)want);
            ++checks;
        }
    printf("ok %ld\n", checks);
    return 0;
}
