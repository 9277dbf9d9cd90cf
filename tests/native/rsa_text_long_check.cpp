// Host check of rna-msm_amd/csrc/rsa_text.h at the long limit (rnamsm_rsa_text_long, L up to rsatext::LONG_MAX_L = 4096): whole
// table lines (line_len, put_line) at every index width and on both sides of 1024 against the C library's snprintf, with the tie
// and carry values of rsa_text_check.cpp as the numbers.  Every line is written into a heap block of exactly its announced length,
// so a sanitizer build stops at the first byte too many; every length is held to rsatext::LINE_BYTES, and the sum of a whole body's
// longest lines to the 32-bit running base of the kernel.
// Exit status 0 and one summary line when everything agrees; 1 and the first mismatches otherwise.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../rna-msm_amd/csrc/rsa_text.h"

namespace {

long long checked = 0, failed = 0;

void report(const char* what, int index, double v, const std::string& got, const char* want) {
    if (++failed <= 10) fprintf(stderr, "MISMATCH %s at index %d of %a (%.20g): got '%s', snprintf '%s'\n", what, index, v, v, got.c_str(), want);
}

// -> the line's length
int check_line(int index, char letter, double asa, double rsa) {
    char want[96];
    const int wn = snprintf(want, sizeof(want), "%d\t\t%c\t\t%.2f\t\t%.3f\n", index, letter, asa, rsa);
    const rsatext::Line ln = rsatext::line_of(asa, rsa);
    const int n = rsatext::line_len(index, ln);
    uint8_t* buf = (uint8_t*)malloc(n);
    rsatext::put_line(buf, index, (uint8_t)letter, ln);
    ++checked;
    if (n != wn || memcmp(buf, want, n) != 0) report("line", index, asa, std::string((char*)buf, n), want);
    if (n > rsatext::LINE_BYTES) report("line bound", index, asa, std::to_string(n), "23");
    free(buf);
    return n;
}

void check_around(int index, char letter, double v, int scale) {
    const double vs[] = {v, std::nextafter(v, 1e9), v > 0 ? std::nextafter(v, -1.0) : v};
    for (double a : vs) {
        check_line(index, letter, a, a / scale);        // an ASA and the RSA the ensemble table prints for it
        if (a <= 1.0) check_line(index, letter, a * scale, a);      // the same number as an RSA
    }
}

}  // namespace

int main() {
    static_assert(rsatext::LONG_MAX_L == 4096 && rsatext::MAX_L == 1024 && rsatext::LINE_BYTES == 23, "the limits this program checks");
    const int idx[] = {1, 9, 10, 99, 100, 999, 1000, 1024, 1025, 4095, 4096};
    // the ties of rsa_text_check.cpp's fixed expectations and its carries into the next digit and the next field width
    const double values[] = {0.125, 0.375, 0.0625, 0.1875, 399.995, 399.99499999999995, 399.99500000000006, 0.9995,
                             0.99949999999999994, 0.99950000000000006, 9.995, 99.995, 0.995, 0.005, 0.0005, 0.00049999999999999,
                             9.9949999999999992, 99.994999999999990, 349.995, 350.0, 349.99999999999994, 1.0, 400.0, 0.0, 0.5, 0.05,
                             0.015, 0.025, 0.035, 0.0015, 0.0025};
    for (int i : idx) {
        if (check_line(i, 'G', 400.0, 1.0) != rsatext::digits((uint32_t)i) + 19) report("longest line", i, 400.0, "", "digits + 19");
        check_line(i, 'U', 0.125, 0.0625);
        check_line(i, 'T', 99.995, 0.2857);
        check_line(i, 'C', std::nextafter(399.995, 1e9), std::nextafter(0.9995, 1e9));
        for (double v : values) {
            check_around(i, 'A', v, 400);
            if (v <= 350.0) check_around(i, 'C', v, 350);
        }
    }
    // every tie j / 8 and j / 16 below 400 at the two indices on both sides of the old limit and at the new one
    const int seam[] = {1024, 1025, 4096};
    for (int i : seam)
        for (int j = 0; j <= 16 * 400; ++j) check_line(i, 'G', j / 16.0, j / 16.0 / 400.0);
    // a whole body of longest lines: the kernel's running base is a uint32 byte count, the body's bound LINE_BYTES x L
    unsigned long long total = 0;
    for (int i = 1; i <= rsatext::LONG_MAX_L; ++i) total += (unsigned long long)rsatext::line_len(i, rsatext::line_of(400.0, 1.0));
    ++checked;
    if (total > (unsigned long long)rsatext::LINE_BYTES * rsatext::LONG_MAX_L || total != 94208ull - (9 * 3 + 90 * 2 + 900)) {
        ++failed;
        fprintf(stderr, "a body of 4096 longest lines has %llu bytes\n", total);
    }
    if (failed) {
        fprintf(stderr, "%lld of %lld checks failed\n", failed, checked);
        return 1;
    }
    printf("rsa_text_long_check: %lld lines agree with snprintf\n", checked);
    return 0;
}
