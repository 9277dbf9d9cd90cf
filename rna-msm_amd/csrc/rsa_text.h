// RNA-MSM RSA: the arithmetic and the lines of the `RSA_result` tables -- the core of rsa_text.hip.
// Plain C++: g++ compiles it for the host test (tests/native/rsa_text_check.cpp), hipcc for the kernel.
// The reference's doSavePredict_single (rnamsm/rsa.py: _save_single, write_rsa_files) per position p:
//   member k    asa_k = double(rsa[k][p]) * scale[p], scale = 400 for A / G, 350 for C / U / T;  rsa_k = double(rsa[k][p])
//   ensemble    asa_e = (((asa_0 + asa_1) + ...) + asa_{K-1}) / K  (numpy's axis-0 sum, then its division);  rsa_e = asa_e / scale[p]
//   the line    "%d\t\t%c\t\t%.2f\t\t%.3f\n" of (p + 1, letter[p], asa, rsa)
// "%.2f" / "%.3f" of a double are its exact binary value rounded half to even at that decimal: v = m 2^-s with m < 2^53, and for
// v < 512 the shift s is at least 44, so round_half_even(m 10^d / 2^s), d <= 3, is one product below 2^63, one shift and a test of
// what fell off (fixed_point).  No floating point is used for the digits.
// A float32 product with 350 or 400 is exact in double (24 + 9 bits), so a fused multiply-add could not change asa_e; the product is
// pinned all the same, so that the sum reads as numpy's whatever -ffp-contract says.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RSAT_HD __host__ __device__
#else
#define RSAT_HD
#endif

namespace rsatext {

constexpr int MAX_L = 1024, MAX_MODELS = 8;
constexpr int LONG_MAX_L = 4096;                  // the long entry (rnamsm_rsa_text_long): still four index digits
constexpr int LINE_BYTES = 23;                    // "1024\t\tG\t\t400.00\t\t1.000\n": bytes of the longest line at L = MAX_L
static_assert(LONG_MAX_L <= 9999, "a line of LINE_BYTES bytes holds four index digits");
constexpr uint32_t ONE_BITS = 0x3f800000u;      // 1.0f: a member value's domain is the bit patterns [0, ONE_BITS]

// the per-base scale of the letter as the table prints it (T scales as U); 0: a letter the host path replaces by a drawn base
RSAT_HD inline int scale_of(uint8_t c) { return c == 'A' || c == 'G' ? 400 : c == 'C' || c == 'U' || c == 'T' ? 350 : 0; }
// sign bit (-0.0 included), above 1.0, NaN, inf: all above ONE_BITS as unsigned patterns
RSAT_HD inline bool outside_domain(uint32_t bits) { return bits > ONE_BITS; }

RSAT_HD inline double pinned(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(x));
#else
    asm("" : "+m"(x));
#endif
    return x;
}
RSAT_HD inline float float_of(uint32_t bits) {
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}
RSAT_HD inline double member_asa(float rsa, int scale) { return pinned((double)rsa * (double)scale); }

// round_half_even(v 10^d) for a finite v in [0, 512) and d <= 3
RSAT_HD inline uint32_t fixed_point(double v, int d) {
    uint64_t bits;
    __builtin_memcpy(&bits, &v, 8);
    const uint32_t E = (uint32_t)(bits >> 52) & 0x7ffu;
    const uint64_t F = bits & 0xfffffffffffffull;
    const uint64_t m = E ? (F | (1ull << 52)) : F;                  // v = m 2^-s
    const int s = 1075 - (int)(E ? E : 1u);                         // v < 2^9: s >= 44
    const uint64_t n = m * (d == 3 ? 1000u : d == 2 ? 100u : d == 1 ? 10u : 1u);      // < 2^53 x 1000 < 2^63
    if (s >= 64) return 0;                                          // n 2^-64 < 1/2
    const uint64_t q = n >> s, rem = n & ((1ull << s) - 1ull), half = 1ull << (s - 1);
    return (uint32_t)q + (rem > half || (rem == half && (q & 1ull)) ? 1u : 0u);
}

RSAT_HD inline int digits(uint32_t v) { return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u); }      // v <= 9999
template <class Byte>
RSAT_HD inline Byte* put_int(Byte* dst, uint32_t v) {
    const int n = digits(v);
    for (int k = n - 1; k >= 0; --k) {
        dst[k] = (Byte)('0' + v % 10u);
        v /= 10u;
    }
    return dst + n;
}
template <class Byte>
RSAT_HD inline Byte* put_tabs(Byte* dst) {
    dst[0] = (Byte)'\t';
    dst[1] = (Byte)'\t';
    return dst + 2;
}
// "%.2f" from q2 = fixed_point(v, 2) and "%.3f" from q3 = fixed_point(v, 3); both return the byte behind the field
RSAT_HD inline int fixed2_len(uint32_t q2) { return digits(q2 / 100u) + 3; }
RSAT_HD inline int fixed3_len(uint32_t q3) { return digits(q3 / 1000u) + 4; }
template <class Byte>
RSAT_HD inline Byte* put_fixed2(Byte* dst, uint32_t q2) {
    dst = put_int(dst, q2 / 100u);
    dst[0] = (Byte)'.';
    dst[1] = (Byte)('0' + q2 / 10u % 10u);
    dst[2] = (Byte)('0' + q2 % 10u);
    return dst + 3;
}
template <class Byte>
RSAT_HD inline Byte* put_fixed3(Byte* dst, uint32_t q3) {
    dst = put_int(dst, q3 / 1000u);
    dst[0] = (Byte)'.';
    dst[1] = (Byte)('0' + q3 / 100u % 10u);
    dst[2] = (Byte)('0' + q3 / 10u % 10u);
    dst[3] = (Byte)('0' + q3 % 10u);
    return dst + 4;
}

// One line of a table, its numbers already in fixed point.  index: 1-based, <= 9999.
struct Line {
    uint32_t asa2, rsa3;        // fixed_point(asa, 2), fixed_point(rsa, 3)
};
RSAT_HD inline int line_len(int index, Line ln) { return digits((uint32_t)index) + fixed2_len(ln.asa2) + fixed3_len(ln.rsa3) + 8; }
// writes exactly line_len bytes
template <class Byte>
RSAT_HD inline void put_line(Byte* d, int index, uint8_t letter, Line ln) {
    d = put_tabs(put_int(d, (uint32_t)index));
    *d++ = (Byte)letter;
    d = put_tabs(d);
    d = put_tabs(put_fixed2(d, ln.asa2));
    d = put_fixed3(d, ln.rsa3);
    *d = (Byte)'\n';
}

// The numbers of position p in table f of K members' values (f < K: member f; f == K: the ensemble).  rsa: [K, L] bit patterns
// inside the domain or already replaced; scale: 350 or 400.  asa / rsa_out: the doubles the line prints.
RSAT_HD inline void member_values(float v, int scale, double& asa, double& rsa_out) {
    asa = member_asa(v, scale);
    rsa_out = (double)v;
}
template <class Load>
RSAT_HD inline void ensemble_values(Load value_of, int K, int scale, double& asa, double& rsa_out, bool& any_zero) {
    double sum = 0.0;                                   // 0 + asa_0 is asa_0: numpy starts from the first row
    for (int k = 0; k < K; ++k) {
        const double a = member_asa(value_of(k), scale);
        any_zero = any_zero || a == 0.0;
        sum = k ? sum + a : a;
    }
    asa = sum / (double)K;
    rsa_out = asa / (double)scale;
    any_zero = any_zero || asa == 0.0;
}
RSAT_HD inline Line line_of(double asa, double rsa) { return Line{fixed_point(asa, 2), fixed_point(rsa, 3)}; }

}  // namespace rsatext
