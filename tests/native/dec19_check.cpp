// Host check of csrc/dec19.h (the digit core of the SS head's .prob text), a program of its own so that it can run under the
// host sanitizers:  g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread dec19_check.cpp -o dec19_check
//   dec19_check          reads float32 bit patterns (hex, one per line) from stdin, prints the 24 characters of each
//   dec19_check --all [threads]   every pattern of [0, 1] (0 .. 0x3f800000) against snprintf("%.18e"); prints the number of
//                        mismatches and the wall time, exit status 1 when there is one (threads: at most 16)
#include <chrono>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <vector>

#include "../../rna-msm_amd/csrc/dec19.h"

static long long check_range(uint32_t lo, uint32_t hi, uint32_t* first_bad) {      // [lo, hi)
    long long bad = 0;
    char mine[dec19::CHARS + 1], libc[64];
    mine[dec19::CHARS] = 0;
    for (uint32_t bits = lo; bits < hi; ++bits) {
        float v;
        memcpy(&v, &bits, 4);
        dec19::format(bits, mine);
        const int n = snprintf(libc, sizeof(libc), "%.18e", (double)v);
        if (n != dec19::CHARS || memcmp(mine, libc, dec19::CHARS) != 0) {
            if (!bad) *first_bad = bits;
            ++bad;
        }
    }
    return bad;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "--all")) {
        int nt = argc >= 3 ? atoi(argv[2]) : 16;
        nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
        const uint64_t total = (uint64_t)dec19::MAX_BITS + 1;
        std::vector<long long> bad(nt, 0);
        std::vector<uint32_t> first(nt, 0);
        std::vector<std::thread> th;
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < nt; ++i)
            th.emplace_back([&, i] {
                bad[i] = check_range((uint32_t)(total * i / nt), (uint32_t)(total * (i + 1) / nt), &first[i]);
            });
        for (auto& t : th) t.join();
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        long long sum = 0;
        for (int i = 0; i < nt; ++i) {
            if (bad[i]) printf("first mismatch of thread %d: 0x%08x\n", i, first[i]);
            sum += bad[i];
        }
        printf("patterns %llu mismatches %lld threads %d seconds %.1f\n", (unsigned long long)total, sum, nt, secs);
        return sum ? 1 : 0;
    }
    char line[64], out[dec19::CHARS + 1];
    out[dec19::CHARS] = 0;
    while (fgets(line, sizeof(line), stdin)) {
        const unsigned long bits = strtoul(line, nullptr, 16);
        if (bits > dec19::MAX_BITS) {
            fprintf(stderr, "0x%lx is outside [0, 0x3f800000]\n", bits);
            return 2;
        }
        dec19::format((uint32_t)bits, out);
        puts(out);
    }
    return 0;
}
