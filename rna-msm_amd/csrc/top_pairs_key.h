// The order key of csrc/top_pairs.hip, compilable on the host (tests/native/top_pairs_key_check.cpp runs it over the edge values and
// seeded pairs under AddressSanitizer + UBSan).
//
// A value that is not NaN maps to a 64-bit unsigned key that is STRICTLY monotone in the value, with -0.0 and +0.0 on one key:
//   zero of either sign -> the bits of +0.0;  then  negative: every bit flipped,  non-negative: the sign bit flipped.
// So -inf < -DBL_MAX < ... < -denormals < 0 < denormals < ... < DBL_MAX < +inf in key order as in value order, and a larger key is a
// larger value.  tp_value undoes it (a zero comes back as +0.0).  NaN has no key: the caller leaves it out before asking.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TP_HD __host__ __device__ __forceinline__
#else
#define TP_HD inline
#endif

namespace rnamsm {

constexpr uint64_t TP_SIGN = 0x8000000000000000ull;

TP_HD uint64_t tp_key(double v) {
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    if ((b << 1) == 0) b = 0;                    // -0.0 counts as +0.0
    return (b & TP_SIGN) ? ~b : (b | TP_SIGN);
}

TP_HD double tp_value(uint64_t key) {
    const uint64_t b = (key & TP_SIGN) ? (key ^ TP_SIGN) : ~key;
    double v;
    __builtin_memcpy(&v, &b, 8);
    return v;
}

}  // namespace rnamsm
