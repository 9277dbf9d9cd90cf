// Host check of csrc/struct_text.h (tests/test_struct_text_host.py builds it with g++ -fsanitize=address,undefined): the tail of the
// decoding kernels -- ownership, measure_lines, a scan over the threads, put_lines -- run serially over T "threads" for every block
// size in use, against a single pass over all bases, on heap buffers of exactly the announced sizes.
//   struct_text_check IN OUT     IN: records of { int32 L; uint8 letters[L]; int32 partner[L] }, L <= LONG_MAX_L
//                                OUT: per record { int32 counts[4]; ct bytes; bpseq bytes } of the single pass
// Exit codes: 2 usage or input, 3 a body beyond its bound, 5 ownership, 6 the threads' bytes or counts differ from the single pass,
// 7 the packed total does not unpack to the three sums.
#include <memory>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../../rna-msm_amd/csrc/struct_text.h"

using namespace sspairs;

// exactly n bytes: a line put at a wrong offset is a heap overflow or leaves a 0xee behind
static std::unique_ptr<uint8_t[]> body(int n) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n]);
    memset(p.get(), 0xee, n);
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t L;
    while (fread(&L, 4, 1, in) == 1) {
        if (L < 1 || L > LONG_MAX_L) return 2;
        std::vector<uint8_t> letters(L);
        std::vector<int32_t> partner(L);
        if (fread(letters.data(), 1, L, in) != (size_t)L || fread(partner.data(), 4, L, in) != (size_t)L) return 2;
        const auto at = [&](int b) { return partner[b]; };

        int sum_ct = 0, sum_bp = 0, sum_pairs = 0;
        bool any_bad = false;
        for (int b = 0; b < L; ++b) {
            sum_ct += ct_line_len(b + 1, L, partner[b]);
            sum_bp += bpseq_line_len(b + 1, partner[b]);
            sum_pairs += partner[b] > b + 1;
            any_bad |= letter_needs_host(letters[b]);
        }
        if (sum_ct > CT_LINE_MAX * L || sum_bp > BPSEQ_LINE_MAX * L) return 3;

        // T = 1 comes first: one "thread" owns every base, and its bytes are what every block size has to write
        std::unique_ptr<uint8_t[]> ct1, bp1;
        int32_t counts1[4];
        for (int T : {1, 64, 128, 960, 1024}) {
            if (T > 1 && L > 4 * T) continue;
            // every base has exactly one owner, and the owners' runs tile [0, L) in thread order
            int next = 0;
            for (int t = 0; t < T; ++t) {
                const int b0 = first_base(t, L, T), b1 = end_base(t, L, T);
                if (b0 != next || b1 < next || b1 - next > bases_per_thread(L, T)) return 5;
                next = b1;
            }
            if (next != L) return 5;
            std::vector<uint64_t> len(T);
            bool bad = false;
            uint64_t total = 0;
            for (int t = 0; t < T; ++t) {
                len[t] = measure_lines(first_base(t, L, T), end_base(t, L, T), L, at, letters.data(), &bad);
                total += len[t];
            }
            if (ct_of(total) != sum_ct || bpseq_of(total) != sum_bp || pairs_of(total) != sum_pairs || bad != any_bad) return 7;
            auto ct = body(ct_of(total)), bp = body(bpseq_of(total));
            uint64_t before = 0;                                  // the scan over threads
            for (int t = 0; t < T; ++t) {
                put_lines(first_base(t, L, T), end_base(t, L, T), L, at, letters.data(), before, ct.get(), bp.get());
                before += len[t];
            }
            int32_t counts[4];
            put_counts(counts, total, bad);
            if (T == 1) {
                memcpy(counts1, counts, sizeof(counts));
                ct1 = std::move(ct);
                bp1 = std::move(bp);
            } else if (memcmp(counts, counts1, sizeof(counts)) || memcmp(ct.get(), ct1.get(), sum_ct) ||
                       memcmp(bp.get(), bp1.get(), sum_bp)) {
                return 6;
            }
        }
        fwrite(counts1, 4, 4, out);
        fwrite(ct1.get(), 1, sum_ct, out);
        fwrite(bp1.get(), 1, sum_bp, out);
    }
    fclose(in);
    return fclose(out) ? 2 : 0;
}
