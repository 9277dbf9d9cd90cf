// The order key of csrc/top_pairs_key.h on the host: strictly monotone over the edge values, both zeros on one key, the inverse exact,
// and the same on seeded pairs of arbitrary bit patterns.  Prints "ok <checks>".
// host sanitizers:  g++ -std=c++17 -O1 -g -fsanitize=address,undefined top_pairs_key_check.cpp -o top_pairs_key_check
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rna-msm_amd/csrc/top_pairs_key.h"

using rnamsm::tp_key;
using rnamsm::tp_value;

static long checks = 0;
static int failures = 0;

static void expect(bool ok, const char* what, double a, double b) {
    ++checks;
    if (!ok && failures++ < 20) std::printf("FAIL %s: %.17g (%016llx) vs %.17g (%016llx)\n", what, a, (unsigned long long)tp_key(a), b,
                                            (unsigned long long)tp_key(b));
}

static uint64_t bits_of(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}
static double from_bits(uint64_t b) {
    double v;
    std::memcpy(&v, &b, 8);
    return v;
}

// key order == value order, equal keys == equal values, the inverse gives the value back (a zero as +0.0)
static void pair(double a, double b) {
    expect((a < b) == (tp_key(a) < tp_key(b)), "a < b", a, b);
    expect((a > b) == (tp_key(a) > tp_key(b)), "a > b", a, b);
    expect((a == b) == (tp_key(a) == tp_key(b)), "a == b", a, b);
    const double back = tp_value(tp_key(a));
    expect(back == a && (a != 0.0 || bits_of(back) == 0), "inverse", a, back);
}

static uint64_t next(uint64_t& s) {       // splitmix64
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

int main() {
    const double inf = INFINITY, dmin = 4.9406564584124654e-324;      // the smallest denormal
    // ascending; the two zeros are equal and share a key
    const std::vector<double> edge = {-inf, -DBL_MAX, -1.0, -DBL_MIN, -from_bits(0x000fffffffffffffull), -2 * dmin, -dmin, -0.0, dmin, 2 * dmin,
                                      from_bits(0x000fffffffffffffull), DBL_MIN, 1.0, std::nextafter(1.0, 2.0), DBL_MAX, inf};
    for (size_t a = 0; a + 1 < edge.size(); ++a) {
        expect(edge[a] < edge[a + 1], "the edge list ascends", edge[a], edge[a + 1]);
        expect(tp_key(edge[a]) < tp_key(edge[a + 1]), "strictly monotone", edge[a], edge[a + 1]);
    }
    for (double a : edge)
        for (double b : edge) pair(a, b);
    expect(tp_key(-0.0) == tp_key(0.0), "-0.0 == +0.0", -0.0, 0.0);
    expect(bits_of(tp_value(tp_key(-0.0))) == 0, "a zero comes back as +0.0", -0.0, tp_value(tp_key(-0.0)));
    expect(tp_key(-inf) > 0, "no value has key 0", -inf, -inf);

    uint64_t seed = 2024;
    int done = 0;
    while (done < 5000) {
        double a = from_bits(next(seed)), b = from_bits(next(seed));
        if (done % 3 == 1) b = from_bits(bits_of(a) ^ (next(seed) & 0xffull));       // neighbours: equal but for the low bits
        if (done % 3 == 2) b = from_bits(bits_of(a) ^ (1ull << 63));                 // the same magnitude, the other sign
        if (a != a || b != b) continue;                                              // NaN has no key
        pair(a, b);
        pair(b, a);
        ++done;
    }
    if (failures) {
        std::printf("%d failures in %ld checks\n", failures, checks);
        return 1;
    }
    std::printf("ok %ld\n", checks);
    return 0;
}
