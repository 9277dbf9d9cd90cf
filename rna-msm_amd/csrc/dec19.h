// "%.18e" of a float32 in [0, 1] as an exact integer computation: the 24 characters C's printf (and so Python's % operator and
// np.savetxt's default format) gives for it.  Plain C++ with no floating point anywhere: g++ compiles it for the host test
// (tests/native/dec19_check.cpp), hipcc for the kernel that writes the SS head's .prob text (ss_text.hip).
//   bits -> v = m 2^e, m < 2^24 (subnormals: e = -149);  d = floor(log10 v), p = 18 - d, 18 <= p <= 63
//   the 19 digits = round_half_even(v 10^p) = round_half_even(m 5^p / 2^s), s = -(e + p) >= 5: always a shift to the right
// m 5^p has at most 24 + 147 = 171 bits: six 32-bit words.  d is first floor(log10 2^b) for the top bit b of v, which is d or
// d - 1; when the 19 digits come out as 10^19 or more it was d - 1, and the product is taken again with the next lower power.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DEC19_HD __host__ __device__
#else
#define DEC19_HD
#endif

namespace dec19 {

constexpr int CHARS = 24;                       // d.dddddddddddddddddde-XX
constexpr uint32_t MAX_BITS = 0x3f800000u;      // 1.0f: the domain is the bit patterns [0, MAX_BITS]
constexpr uint64_t TEN18 = 1000000000000000000ull, TEN19 = 10000000000000000000ull;

// 5^18 .. 5^63, least significant word first
static constexpr uint32_t POW5[46][5] = {
    {0x2dace9d9u, 0x00000378u, 0x00000000u, 0x00000000u, 0x00000000u},   // 5^18
    {0xe460913du, 0x00001158u, 0x00000000u, 0x00000000u, 0x00000000u},   // 5^19
    {0x75e2d631u, 0x000056bcu, 0x00000000u, 0x00000000u, 0x00000000u},   // 5^20
    {0x4d6e2ef5u, 0x0001b1aeu, 0x00000000u, 0x00000000u, 0x00000000u},   // 5^21
    {0x8326eac9u, 0x00087867u, 0x00000000u, 0x00000000u, 0x00000000u},   // 5^22
    {0x8fc295edu, 0x002a5a05u, 0x00000000u, 0x00000000u, 0x00000000u},   // 5^23
    {0xcecceda1u, 0x00d3c21bu, 0x00000000u, 0x00000000u, 0x00000000u},   // 5^24
    {0x0a00a425u, 0x0422ca8bu, 0x00000000u, 0x00000000u, 0x00000000u},   // 5^25
    {0x320334b9u, 0x14adf4b7u, 0x00000000u, 0x00000000u, 0x00000000u},   // 5^26
    {0xfa10079du, 0x6765c793u, 0x00000000u, 0x00000000u, 0x00000000u},   // 5^27
    {0xe2502611u, 0x04fce5e3u, 0x00000002u, 0x00000000u, 0x00000000u},   // 5^28
    {0x6b90be55u, 0x18f07d73u, 0x0000000au, 0x00000000u, 0x00000000u},   // 5^29
    {0x19d3b7a9u, 0x7cb27341u, 0x00000032u, 0x00000000u, 0x00000000u},   // 5^30
    {0x8122964du, 0x6f7c4045u, 0x000000fcu, 0x00000000u, 0x00000000u},   // 5^31
    {0x85acef81u, 0x2d6d415bu, 0x000004eeu, 0x00000000u, 0x00000000u},   // 5^32
    {0x9c60ad85u, 0xe32246c9u, 0x000018a6u, 0x00000000u, 0x00000000u},   // 5^33
    {0x0de36399u, 0x6fab61f0u, 0x00007b42u, 0x00000000u, 0x00000000u},   // 5^34
    {0x4570f1fdu, 0x2e58e9b0u, 0x0002684cu, 0x00000000u, 0x00000000u},   // 5^35
    {0x5b34b9f1u, 0xe7bc9071u, 0x000c097cu, 0x00000000u, 0x00000000u},   // 5^36
    {0xc807a1b5u, 0x86aed236u, 0x003c2f70u, 0x00000000u, 0x00000000u},   // 5^37
    {0xe8262889u, 0xa16a1b11u, 0x012ced32u, 0x00000000u, 0x00000000u},   // 5^38
    {0x88becaadu, 0x27128759u, 0x05e0a1fdu, 0x00000000u, 0x00000000u},   // 5^39
    {0xabb9f561u, 0xc35ca4bfu, 0x1d6329f1u, 0x00000000u, 0x00000000u},   // 5^40
    {0x5aa1cae5u, 0xd0cf37beu, 0x92efd1b8u, 0x00000000u, 0x00000000u},   // 5^41
    {0xc528f679u, 0x140c16b7u, 0xdeaf189cu, 0x00000002u, 0x00000000u},   // 5^42
    {0xd9ccd05du, 0x643c7196u, 0x596b7b0cu, 0x0000000eu, 0x00000000u},   // 5^43
    {0x410011d1u, 0xf52e37f2u, 0xbf19673du, 0x00000047u, 0x00000000u},   // 5^44
    {0x45005915u, 0xc9e717bbu, 0xbb7f0435u, 0x00000166u, 0x00000000u},   // 5^45
    {0x5901bd69u, 0xf18376a8u, 0xa97b150cu, 0x00000701u, 0x00000000u},   // 5^46
    {0xbd08b30du, 0xb7915149u, 0x4f676940u, 0x00002308u, 0x00000000u},   // 5^47
    {0xb12b7f41u, 0x95d69670u, 0x8d050e43u, 0x0000af29u, 0x00000000u},   // 5^48
    {0x75d97c45u, 0xed30f033u, 0xc1194751u, 0x00036bcfu, 0x00000000u},   // 5^49
    {0x4d3f6d59u, 0xa1f4b101u, 0xc57e6499u, 0x00111b0eu, 0x00000000u},   // 5^50
    {0x823d22bdu, 0x29c77506u, 0xdb77f700u, 0x00558749u, 0x00000000u},   // 5^51
    {0x8b31adb1u, 0xd0e54920u, 0x4957d300u, 0x01aba471u, 0x00000000u},   // 5^52
    {0xb7f86475u, 0x147a6da2u, 0x6eb71f04u, 0x085a3636u, 0x00000000u},   // 5^53
    {0x97d9f649u, 0x6664242du, 0x29939b14u, 0x29c30f10u, 0x00000000u},   // 5^54
    {0xf741cf6du, 0xfff4b4e3u, 0xcfe20765u, 0xd0cf4b50u, 0x00000000u},   // 5^55
    {0xd4490d21u, 0xffc78873u, 0x0f6a24fdu, 0x140c7894u, 0x00000004u},   // 5^56
    {0x256d41a5u, 0xfee5aa43u, 0x4d12b8f5u, 0x643e5ae4u, 0x00000014u},   // 5^57
    {0xbb224839u, 0xfa7c534fu, 0x815d9ccdu, 0xf537c675u, 0x00000065u},   // 5^58
    {0xa7ab691du, 0xe46da08eu, 0x86d41005u, 0xca16e04bu, 0x000001fdu},   // 5^59
    {0x46590d91u, 0x762422c9u, 0xa224501du, 0xf2726179u, 0x000009f4u},   // 5^60
    {0x5fbd43d5u, 0x4eb4adeeu, 0x2ab59093u, 0xbc3be760u, 0x000031c8u},   // 5^61
    {0xdeb25329u, 0x898765a7u, 0xd58bd2e0u, 0xad2b84e0u, 0x0000f8ebu},   // 5^62
    {0x597b9fcdu, 0xafa4fc47u, 0x2bbb1e62u, 0x61d99864u, 0x0004dc9au},   // 5^63
};

// N = round_half_even(m 5^p / 2^s), 1 <= s <= 96; true (N left at its floor) when the quotient is 10^19 or more
DEC19_HD inline bool scaled(uint32_t m, int p, int s, uint64_t& N) {
    const uint32_t* w5 = POW5[p - 18];
    uint32_t w[6];
    uint64_t c = 0;
    for (int i = 0; i < 5; ++i) {
        c += (uint64_t)m * w5[i];
        w[i] = (uint32_t)c;
        c >>= 32;
    }
    w[5] = (uint32_t)c;
    // shift by s - 1 first: bit 0 of what is left is the rounding bit, everything that fell off is sticky
    const int ws = (s - 1) >> 5, bs = (s - 1) & 31;
    uint32_t sticky = 0;
    for (int k = 0; k < 2; ++k)
        if (ws > k) {
            sticky |= w[0];
            for (int i = 0; i < 5; ++i) w[i] = w[i + 1];
            w[5] = 0;
        }
    sticky |= w[0] & ((1u << bs) - 1u);
    const uint32_t t0 = (uint32_t)((((uint64_t)w[1] << 32) | w[0]) >> bs);
    const uint32_t t1 = (uint32_t)((((uint64_t)w[2] << 32) | w[1]) >> bs);
    const uint32_t t2 = (uint32_t)((((uint64_t)w[3] << 32) | w[2]) >> bs);      // the quotient is below 2 10^19 < 2^65: nothing above
    N = ((uint64_t)t2 << 63) | ((uint64_t)t1 << 31) | (t0 >> 1);
    if ((t2 >> 1) || N >= TEN19) return true;
    if ((t0 & 1u) && (sticky || (N & 1u))) ++N;
    return false;
}

// the 24 characters of "%.18e" for the float32 with these bits; bits in [0, MAX_BITS]
template <class Byte>
DEC19_HD inline void format(uint32_t bits, Byte* out) {
    const uint32_t E = bits >> 23, F = bits & 0x7fffffu;
    const uint32_t m = E ? (F | 0x800000u) : F;
    const int e = E ? (int)E - 150 : -149;
    uint64_t N = 0;
    int d = 0;
    if (m) {
        const int nb = -(e + 31 - __builtin_clz(m));       // v in [2^-nb, 2^(1-nb)), 0 <= nb <= 149
        d = -((nb * 1233 + 4095) >> 12);                    // floor(log10 2^-nb) = -ceil(nb log10 2), exact for nb <= 149
        if (scaled(m, 18 - d, -(e + 18 - d), N)) {          // v >= 10^(d+1): the estimate was one short
            ++d;
            scaled(m, 18 - d, -(e + 18 - d), N);
        }
        if (N == TEN19) {                                   // 9.99..9|5.. rounded up into the next decade
            N = TEN18;
            ++d;
        }
    }
    const uint64_t q = N / 1000000000u;
    uint32_t lo = (uint32_t)(N - q * 1000000000u);
    const uint32_t top = (uint32_t)(q / 1000000000u);
    uint32_t mid = (uint32_t)(q - (uint64_t)top * 1000000000u);
    out[0] = (Byte)('0' + top);
    out[1] = (Byte)'.';
    for (int i = 8; i >= 0; --i) {
        out[2 + i] = (Byte)('0' + mid % 10u);
        mid /= 10u;
        out[11 + i] = (Byte)('0' + lo % 10u);
        lo /= 10u;
    }
    const uint32_t nd = (uint32_t)(-d);                     // 0 .. 45
    out[20] = (Byte)'e';
    out[21] = (Byte)(nd ? '-' : '+');
    out[22] = (Byte)('0' + nd / 10u);
    out[23] = (Byte)('0' + nd % 10u);
}

}  // namespace dec19
