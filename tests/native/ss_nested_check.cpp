// Host check of csrc/ss_nested.h (tests/test_ss_nested_host.py builds it with g++ -fsanitize=address,undefined; tools/
// ss_nested_timing.py with -O2 to time the serial model): the kernels' tile schedule and the traceback run serially over their
// "threads", on heap buffers of exactly the documented sizes.
//   ss_nested_check IN OUT [REPEAT]
//     IN:  records of { int32 L; float theta; int32 min_loop; uint8 letters[L]; float probs[L * L] }
//     OUT: per record { int32 partner[L]; int32 counts[5]; ct bytes; bpseq bytes; uint8 dbn[L] }
//     REPEAT: decode every record that many times (1 by default) and print the seconds of one decode per record
#include <chrono>
#include <memory>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../rna-msm_amd/csrc/ss_nested.h"

using namespace ssnested;

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) return 2;
    const int repeat = argc == 4 ? atoi(argv[3]) : 1;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out || repeat < 1) return 2;
    int32_t L, min_loop;
    float theta;
    auto mem = std::make_unique<TileMem>();
    while (fread(&L, 4, 1, in) == 1) {
        if (fread(&theta, 4, 1, in) != 1 || fread(&min_loop, 4, 1, in) != 1) return 2;
        if (L < 1 || L > MAX_L || !(theta >= 0.f && theta < 1.f) || min_loop < 0 || min_loop > MAX_LOOP) return 2;
        std::vector<uint8_t> letters(L);
        std::vector<float> P((size_t)L * L);
        if (fread(letters.data(), 1, L, in) != (size_t)L || fread(P.data(), 4, P.size(), in) != P.size()) return 2;
        const size_t Lp = padded(L);
        std::vector<int32_t> N(Lp * Lp, 0x5a5a5a5a), M(Lp * Lp, 0x5a5a5a5a);      // the workspace's contents on entry do not matter
        std::vector<int32_t> stack(2 * ((size_t)L + 2)), partner(L);
        std::vector<uint8_t> ct((size_t)sspairs::CT_LINE_MAX * L), bp((size_t)sspairs::BPSEQ_LINE_MAX * L), dbn(L);
        int32_t counts[5];
        const auto t0 = std::chrono::steady_clock::now();
        for (int rep = 0; rep < repeat; ++rep) {
            fill_serial(P.data(), L, params(theta, min_loop), N.data(), M.data(), *mem);
            if (!trace_serial(N.data(), M.data(), L, min_loop, letters.data(), stack.data(), partner.data(), counts, ct.data(), bp.data(),
                              dbn.data()))
                return 4;
        }
        if (argc == 4)
            printf("%d %.6f\n", L, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / repeat);
        fwrite(partner.data(), 4, L, out);
        fwrite(counts, 4, 5, out);
        fwrite(ct.data(), 1, counts[1], out);
        fwrite(bp.data(), 1, counts[2], out);
        fwrite(dbn.data(), 1, L, out);
    }
    fclose(in);
    return fclose(out) ? 2 : 0;
}
