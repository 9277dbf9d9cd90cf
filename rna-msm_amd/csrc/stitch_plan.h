// The window plan of a long alignment and its blend weights, shared by the device stitcher (stitch.hip) and the
// host check (tests/native/stitch_plan_check.cpp): integers and one IEEE fp32 division, the same on both sides.
//   L body columns, windows of W < L columns, stride in [ceil(W / 2), W]; n = ceil((L - W) / stride) + 1 windows,
//   window k starts at k * stride, the last one at L - W (right-aligned): starts ascend strictly, every window is W wide.
//   u_k(i), i in [0, W): ramp = W - stride; 1 where ramp == 0, else min(left, right, ramp) / ramp with left = ramp in the first
//   window, else i + 1, and right = ramp in the last window, else W - i.  Never zero: min(...) >= 1.
// The windows that contain a column are a run lo .. hi of at most STITCH_MAX_COVER: two of the regular ones (their starts are
// stride >= W / 2 apart) and the right-aligned last one.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define STITCH_HD __host__ __device__ __forceinline__
#else
#define STITCH_HD inline
#endif

namespace rnamsm {

constexpr int STITCH_MAX_COVER = 3;

struct StitchPlan {
    int32_t L, W, stride, n, ramp;
};

STITCH_HD bool stitch_plan_ok(int64_t L, int64_t W, int64_t stride) { return W >= 1 && L > W && stride <= W && 2 * stride >= W; }

STITCH_HD StitchPlan stitch_plan(int L, int W, int stride) {
    StitchPlan pl;
    pl.L = L;
    pl.W = W;
    pl.stride = stride;
    pl.n = (L - W + stride - 1) / stride + 1;
    pl.ramp = W - stride;
    return pl;
}

STITCH_HD int stitch_start(const StitchPlan& pl, int k) { return k < pl.n - 1 ? k * pl.stride : pl.L - pl.W; }

// u_k(i): one division, correctly rounded (no reciprocal: the file that includes this is built with contraction off and hipcc's
// default correctly rounded fp32 division).
STITCH_HD float stitch_weight(const StitchPlan& pl, int k, int i) {
    if (pl.ramp == 0) return 1.0f;
    const int left = k == 0 ? pl.ramp : i + 1;
    const int right = k == pl.n - 1 ? pl.ramp : pl.W - i;
    int m = left < right ? left : right;
    if (pl.ramp < m) m = pl.ramp;
    return (float)m / (float)pl.ramp;
}

// The windows lo .. hi that contain column p (0 <= p < L): never empty.
STITCH_HD void stitch_cover(const StitchPlan& pl, int p, int& lo, int& hi) {
    // regular windows k <= n - 2: k * stride <= p < k * stride + W
    hi = p / pl.stride;
    if (hi > pl.n - 2) hi = pl.n - 2;
    lo = p >= pl.W ? (p - pl.W) / pl.stride + 1 : 0;
    if (p >= pl.L - pl.W) {               // the right-aligned last window
        if (lo > hi) lo = pl.n - 1;
        hi = pl.n - 1;
    }
}

}  // namespace rnamsm
