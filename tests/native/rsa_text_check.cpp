// Host check of rna-msm_amd/csrc/rsa_text.h: "%.2f" / "%.3f" of a double computed in integers (fixed_point, put_fixed2, put_fixed3)
// and whole table lines (line_len, put_line) against the C library's snprintf, which rounds the exact binary value half to even as
// Python's % operator does.  Every field is written into a heap block of exactly its announced length, so a sanitizer build stops
// at the first byte too many.
//   rsa_text_check [count]      count: seeded float32 values of the sweep (default 2500000: four products / quotients each)
// Exit status 0 and one summary line when everything agrees; 1 and the first mismatches otherwise.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../rna-msm_amd/csrc/rsa_text.h"

namespace {

long long checked = 0, failed = 0;

void report(const char* what, double v, const std::string& got, const char* want) {
    if (++failed <= 10) fprintf(stderr, "MISMATCH %s of %a (%.20g): got '%s', snprintf '%s'\n", what, v, v, got.c_str(), want);
}

std::string fixed2(double v) {
    const uint32_t q = rsatext::fixed_point(v, 2);
    const int n = rsatext::fixed2_len(q);
    char* buf = (char*)malloc(n);
    char* end = rsatext::put_fixed2(buf, q);
    std::string s(buf, n);
    if (end != buf + n) s += "<length>";
    free(buf);
    return s;
}
std::string fixed3(double v) {
    const uint32_t q = rsatext::fixed_point(v, 3);
    const int n = rsatext::fixed3_len(q);
    char* buf = (char*)malloc(n);
    char* end = rsatext::put_fixed3(buf, q);
    std::string s(buf, n);
    if (end != buf + n) s += "<length>";
    free(buf);
    return s;
}

// v: finite, in [0, 512)
void check(double v) {
    char want[64];
    ++checked;
    snprintf(want, sizeof(want), "%.2f", v);
    const std::string a = fixed2(v);
    if (a != want) report("%.2f", v, a, want);
    snprintf(want, sizeof(want), "%.3f", v);
    const std::string b = fixed3(v);
    if (b != want) report("%.3f", v, b, want);
}
void check_around(double v) {
    check(v);
    check(std::nextafter(v, 1e9));
    if (v > 0) check(std::nextafter(v, -1.0));
}

void check_line(int index, char letter, double asa, double rsa) {
    char want[96];
    const int wn = snprintf(want, sizeof(want), "%d\t\t%c\t\t%.2f\t\t%.3f\n", index, letter, asa, rsa);
    const rsatext::Line ln = rsatext::line_of(asa, rsa);
    const int n = rsatext::line_len(index, ln);
    uint8_t* buf = (uint8_t*)malloc(n);
    rsatext::put_line(buf, index, (uint8_t)letter, ln);
    ++checked;
    if (n != wn || memcmp(buf, want, n) != 0) report("line", asa, std::string((char*)buf, n), want);
    if (n > rsatext::LINE_BYTES) report("line bound", asa, std::to_string(n), "23");
    free(buf);
}

uint64_t state = 0x9e3779b97f4a7c15ull;
uint64_t next_u64() {          // splitmix64
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

void expect(double v, const char* want2, const char* want3) {
    ++checked;
    if (fixed2(v) != want2) report("%.2f (fixed expectation)", v, fixed2(v), want2);
    if (want3 && fixed3(v) != want3) report("%.3f (fixed expectation)", v, fixed3(v), want3);
}

}  // namespace

int main(int argc, char** argv) {
    const long long count = argc > 1 ? atoll(argv[1]) : 2500000;

    // the ties: v 100 = n + 1/2 needs v = j / 8, v 1000 = n + 1/2 needs v = j / 16 (j odd); every one below 512, and both neighbours
    for (int j = 0; j < 8 * 512; ++j) check_around(j / 8.0);
    for (int j = 0; j < 16 * 512; ++j) check_around(j / 16.0);
    expect(0.125, "0.12", "0.125");
    expect(0.375, "0.38", "0.375");
    expect(0.0625, "0.06", "0.062");
    expect(0.1875, "0.19", "0.188");
    // carries into the next digit and the next field width
    const double carries[] = {399.995, 399.99499999999995, 399.99500000000006, 0.9995, 0.99949999999999994, 0.99950000000000006, 9.995,
                              99.995, 0.995, 0.005, 0.0005, 0.00049999999999999, 9.9949999999999992, 99.994999999999990, 349.995, 350.0,
                              349.99999999999994, 1.0, 400.0, 0.0, 511.99, 0.5, 0.05, 0.015, 0.025, 0.035, 0.0015, 0.0025};
    for (double v : carries) check_around(v);
    expect(std::nextafter(399.995, 1e9), "400.00", nullptr);
    expect(400.0, "400.00", nullptr);
    expect(1.0, "1.00", "1.000");
    expect(std::nextafter(0.9995, 1e9), "1.00", "1.000");
    expect(0.0, "0.00", "0.000");
    // the smallest normal, subnormals, and everything with a shift of 64 and more
    expect(2.2250738585072014e-308, "0.00", "0.000");
    expect(4.9406564584124654e-324, "0.00", "0.000");
    expect(1e-310, "0.00", "0.000");
    for (int e = -1074; e <= -1; ++e) check_around(std::ldexp(1.0, e));
    for (int e = -30; e <= 8; ++e) check_around(std::ldexp(1.5, e));

    // every float32 of a few dense windows, as RSA values and as their ASA
    const uint32_t windows[][2] = {{0x3f7f0000u, 0x3f800000u}, {0x3f000000u - 0x8000u, 0x3f000000u + 0x8000u},
                                   {0x3a83126fu - 0x8000u, 0x3a83126fu + 0x8000u}, {0x00000000u, 0x00010000u},
                                   {0x3dcccccdu - 0x8000u, 0x3dcccccdu + 0x8000u}};
    for (const auto& w : windows)
        for (uint32_t b = w[0]; b <= w[1]; ++b) {
            const double r = (double)rsatext::float_of(b);
            check(r);
            check(rsatext::member_asa(rsatext::float_of(b), 350));
            check(rsatext::member_asa(rsatext::float_of(b), 400));
        }

    // the seeded sweep: float32 in (0, 1] (uniform, and uniform over the bit patterns), x 350 and x 400, and the quotients by 3
    for (long long i = 0; i < count; ++i) {
        const uint64_t r = next_u64();
        const uint32_t bits = (i & 1) ? 1u + (uint32_t)(r % rsatext::ONE_BITS) : 0u;
        const float f = (i & 1) ? rsatext::float_of(bits) : (float)(((r >> 40) + 1) * 0x1p-24);
        const double a350 = rsatext::member_asa(f, 350), a400 = rsatext::member_asa(f, 400);
        check(a350);
        check(a400);
        check(a350 / 3.0);
        check(a400 / 3.0);
        if ((i & 15) == 0) {
            check((double)f);
            check(a350 / 3.0 / 350.0);
            check_line(1 + (int)(r % 1024), "ACGUT"[r % 5], a400 / 3.0, a400 / 3.0 / 400.0);
        }
    }
    // lines at the index widths and the bound
    const int idx[] = {1, 9, 10, 99, 100, 999, 1000, 1024};
    for (int i : idx) {
        check_line(i, 'G', 400.0, 1.0);
        check_line(i, 'U', 0.125, 0.0625);
        check_line(i, 'T', 99.995, 0.2857);
    }
    if (failed) {
        fprintf(stderr, "%lld of %lld checks failed\n", failed, checked);
        return 1;
    }
    printf("rsa_text_check: %lld values and lines agree with snprintf\n", checked);
    return 0;
}
