// Host check of csrc/ss_pairs.h (tests/test_ss_pairs_host.py builds it with g++ -fsanitize=address,undefined): the kernel's round
// logic run serially over its "threads", and the line formatter, on heap buffers of exactly the documented sizes.
//   ss_pairs_check IN OUT     IN: records of { int32 L; uint8 letters[L]; float probs[L * L] }
//                             OUT: per record { int32 partner[L]; int32 counts[4]; ct bytes; bpseq bytes }
//   ss_pairs_check --lines    stdin: lines "i L partner letter-code"; stdout: the .ct line and the .bpseq line of each
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../../rna-msm_amd/csrc/ss_pairs.h"

using namespace sspairs;

static int lines_mode() {
    int i, L, partner, letter;
    while (scanf("%d %d %d %d", &i, &L, &partner, &letter) == 4) {
        const int nc = ct_line_len(i, L, partner), nb = bpseq_line_len(i, partner);
        if (nc > CT_LINE_MAX || nb > BPSEQ_LINE_MAX) return 3;
        std::vector<uint8_t> ct(nc), bp(nb);          // exact: a byte too many is a heap overflow
        put_ct_line(ct.data(), i, (uint8_t)letter, L, partner);
        put_bpseq_line(bp.data(), i, (uint8_t)letter, partner);
        fwrite(ct.data(), 1, nc, stdout);
        fwrite(bp.data(), 1, nb, stdout);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--lines")) return lines_mode();
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t L;
    while (fread(&L, 4, 1, in) == 1) {
        if (L < 1 || L > MAX_L) return 2;
        std::vector<uint8_t> letters(L);
        std::vector<float> P((size_t)L * L);
        if (fread(letters.data(), 1, L, in) != (size_t)L || fread(P.data(), 4, P.size(), in) != P.size()) return 2;
        const int W = words(L);
        std::vector<uint64_t> adj((size_t)L * W, ~0ull);          // the workspace's contents on entry do not matter
        std::vector<int32_t> mark(L), partner(L);
        for (int b = 0; b < L; ++b)
            for (int k = 0; k < W; ++k) {
                uint64_t bits = 0;                                 // the wave's ballot
                for (int lane = 0; lane < 64; ++lane) bits |= (uint64_t)edge_at(P.data(), L, b, 64 * k + lane) << lane;
                adj[(size_t)b * W + k] = bits;
            }
        int rounds = 0;
        for (; rounds < L; ++rounds) {
            bool any = false;
            for (int b = 0; b < L; ++b) {          // every thread marks, then the barrier
                mark[b] = pick_mark(&adj[(size_t)b * W], W, b, P.data(), L);
                any |= mark[b] >= 0;
            }
            if (!any) break;
            for (int b = 0; b < L; ++b) remove_marked(&adj[(size_t)b * W], W, b, mark.data());
        }
        if (rounds > (L > 2 ? L - 2 : 0)) return 4;
        std::vector<uint8_t> ct((size_t)CT_LINE_MAX * L), bp((size_t)BPSEQ_LINE_MAX * L);
        for (int b = 0; b < L; ++b) partner[b] = partner_of(&adj[(size_t)b * W], W);
        const auto at = [&](int b) { return partner[b]; };          // the kernel's tail with one "thread" that owns every base
        int32_t counts[4];
        bool bad = false;
        const uint64_t total = measure_lines(0, L, L, at, letters.data(), &bad);
        put_lines(0, L, L, at, letters.data(), 0, ct.data(), bp.data());
        put_counts(counts, total, bad);
        fwrite(partner.data(), 4, L, out);
        fwrite(counts, 4, 4, out);
        fwrite(ct.data(), 1, counts[1], out);
        fwrite(bp.data(), 1, counts[2], out);
    }
    fclose(in);
    return fclose(out) ? 2 : 0;
}
