// Host check of csrc/ss_pairs_long.h (tests/test_long_heads_host.py builds it with g++ -fsanitize=address,undefined): the long
// kernel's per-thread round logic and the line scan of struct_text.h, run serially over the LONG_THREADS "threads" of its one
// workgroup, on heap buffers of exactly the documented sizes.
//   ss_pairs_long_check IN OUT     IN: records of { int32 L; uint8 letters[L]; float probs[L * L] }, L <= LONG_MAX_L
//                                  OUT: per record { int32 partner[L]; int32 counts[4]; ct bytes; bpseq bytes }
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../../rna-msm_amd/csrc/ss_pairs_long.h"

using namespace sspairs;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t L;
    while (fread(&L, 4, 1, in) == 1) {
        if (L < 1 || L > LONG_MAX_L) return 2;
        std::vector<uint8_t> letters(L);
        std::vector<float> P((size_t)L * L);
        if (fread(letters.data(), 1, L, in) != (size_t)L || fread(P.data(), 4, P.size(), in) != P.size()) return 2;
        const int W = words(L);
        // every base has exactly one owner, and the owners' runs tile [0, L) in thread order
        int next = 0;
        for (int t = 0; t < LONG_THREADS; ++t) {
            const int b0 = first_base(t, L, LONG_THREADS), b1 = end_base(t, L, LONG_THREADS);
            if (b0 != next || b1 < next || b1 - next > bases_per_thread(L, LONG_THREADS)) return 5;
            next = b1;
        }
        if (next != L) return 5;
        std::vector<uint64_t> adj((size_t)L * W, ~0ull);          // the workspace's contents on entry do not matter
        std::vector<int32_t> mark(L), partner(L);                 // mark: exactly L entries -- no thread touches a base it does not own
        for (int b = 0; b < L; ++b)                               // launch 1: a wave per row
            for (int k = 0; k < W; ++k) {
                uint64_t bits = 0;
                for (int lane = 0; lane < 64; ++lane) bits |= (uint64_t)edge_at(P.data(), L, b, 64 * k + lane) << lane;
                adj[(size_t)b * W + k] = bits;
            }
        int rounds = 0;
        for (; rounds < L; ++rounds) {
            bool any = false;
            for (int t = 0; t < LONG_THREADS; ++t) any |= thread_mark(adj.data(), W, t, P.data(), L, mark.data());      // then the barrier
            if (!any) break;
            for (int t = 0; t < LONG_THREADS; ++t) thread_remove(adj.data(), W, t, L, mark.data());
        }
        if (rounds > (L > 2 ? L - 2 : 0)) return 4;
        std::vector<uint64_t> len(LONG_THREADS);
        bool bad = false;
        const auto at = [&](int b) { return partner[b]; };
        for (int t = 0; t < LONG_THREADS; ++t) {
            thread_partners(adj.data(), W, t, L, partner.data());
            len[t] = measure_lines(first_base(t, L, LONG_THREADS), end_base(t, L, LONG_THREADS), L, at, letters.data(), &bad);
        }
        uint64_t total = 0;
        for (int t = 0; t < LONG_THREADS; ++t) total += len[t];
        // the bodies: exactly the bytes the counts announce -- a line put at a wrong offset is a heap overflow or a gap
        std::vector<uint8_t> ct(ct_of(total), 0xee), bp(bpseq_of(total), 0xee);
        if (ct.size() > (size_t)CT_LINE_MAX * L || bp.size() > (size_t)BPSEQ_LINE_MAX * L) return 3;
        uint64_t before = 0;                                      // the scan over threads
        for (int t = 0; t < LONG_THREADS; ++t) {
            put_lines(first_base(t, L, LONG_THREADS), end_base(t, L, LONG_THREADS), L, at, letters.data(), before, ct.data(), bp.data());
            before += len[t];
        }
        int32_t counts[4];
        put_counts(counts, total, bad);
        fwrite(partner.data(), 4, L, out);
        fwrite(counts, 4, 4, out);
        fwrite(ct.data(), 1, ct.size(), out);
        fwrite(bp.data(), 1, bp.size(), out);
    }
    fclose(in);
    return fclose(out) ? 2 : 0;
}
