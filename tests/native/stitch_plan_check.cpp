// Host check of rna-msm_amd/csrc/stitch_plan.h, the header the device stitcher computes its window plan with.
//   stitch_plan_check                 every plan of W <= 24 (all admissible strides, L up to 3 W + 5) against a brute-force
//                                     restatement: starts, window count, the windows that contain a column, the weights' ranges;
//                                     then a few hand-computed plans.  Prints "plans ok"; exit 1 with a message otherwise.
//   stitch_plan_check L W stride      prints the starts, then every window's weights as fp32 bit patterns (hex), one per line.
// Built by tests/test_windows_host.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../rna-msm_amd/csrc/stitch_plan.h"

using namespace rnamsm;

static int fail(const char* what, int L, int W, int stride, int at) {
    std::fprintf(stderr, "%s: L=%d W=%d stride=%d at %d\n", what, L, W, stride, at);
    return 1;
}

static int check(int L, int W, int stride) {
    if (!stitch_plan_ok(L, W, stride)) return fail("refused", L, W, stride, 0);
    const StitchPlan pl = stitch_plan(L, W, stride);
    int n = 1;
    while ((n - 1) * stride < L - W) ++n;                       // ceil((L - W) / stride) + 1, counted
    if (pl.n != n || pl.ramp != W - stride) return fail("window count", L, W, stride, pl.n);
    std::vector<int> st(n);
    for (int k = 0; k < n; ++k) {
        st[k] = stitch_start(pl, k);
        if (st[k] != (k < n - 1 ? k * stride : L - W) || st[k] < 0 || st[k] + W > L) return fail("start", L, W, stride, k);
        if (k && st[k] <= st[k - 1]) return fail("starts ascend", L, W, stride, k);
    }
    for (int p = 0; p < L; ++p) {
        int lo, hi, blo = -1, bhi = -1, cnt = 0;
        stitch_cover(pl, p, lo, hi);
        for (int k = 0; k < n; ++k)
            if (st[k] <= p && p < st[k] + W) {
                if (blo < 0) blo = k;
                bhi = k;
                ++cnt;
            }
        if (cnt < 1 || cnt > STITCH_MAX_COVER || cnt != bhi - blo + 1) return fail("coverage", L, W, stride, p);
        if (lo != blo || hi != bhi) return fail("cover run", L, W, stride, p);
        for (int k = lo; k <= hi; ++k) {
            const float u = stitch_weight(pl, k, p - st[k]);
            if (!(u > 0.f && u <= 1.f)) return fail("weight range", L, W, stride, p);
            if (cnt == 1 && u != 1.f) return fail("singly covered weight", L, W, stride, p);
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4) {
        const int L = std::atoi(argv[1]), W = std::atoi(argv[2]), stride = std::atoi(argv[3]);
        if (!stitch_plan_ok(L, W, stride)) return 2;
        const StitchPlan pl = stitch_plan(L, W, stride);
        for (int k = 0; k < pl.n; ++k) std::printf("%d\n", stitch_start(pl, k));
        for (int k = 0; k < pl.n; ++k)
            for (int i = 0; i < W; ++i) {
                const float u = stitch_weight(pl, k, i);
                uint32_t b;
                std::memcpy(&b, &u, 4);
                std::printf("%08x\n", b);
            }
        return 0;
    }
    long plans = 0;
    for (int W = 1; W <= 24; ++W)
        for (int stride = (W + 1) / 2; stride <= W; ++stride)
            for (int L = W + 1; L <= 3 * W + 5; ++L, ++plans)
                if (check(L, W, stride)) return 1;
    // refusals
    if (stitch_plan_ok(32, 32, 16) || stitch_plan_ok(70, 32, 15) || stitch_plan_ok(70, 32, 33) || stitch_plan_ok(5, 0, 0)) return fail("accepted", 0, 0, 0, 0);
    // hand-computed: W = 32, stride = 16, L = 70 -> starts 0 16 32 38; column 40 lies in windows 1, 2 and 3
    {
        const StitchPlan pl = stitch_plan(70, 32, 16);
        const int want[4] = {0, 16, 32, 38};
        if (pl.n != 4) return fail("hand: n", 70, 32, 16, pl.n);
        for (int k = 0; k < 4; ++k)
            if (stitch_start(pl, k) != want[k]) return fail("hand: start", 70, 32, 16, k);
        int lo, hi;
        stitch_cover(pl, 40, lo, hi);
        if (lo != 1 || hi != 3) return fail("hand: cover of 40", 70, 32, 16, lo * 10 + hi);
        stitch_cover(pl, 5, lo, hi);
        if (lo != 0 || hi != 0) return fail("hand: cover of 5", 70, 32, 16, lo * 10 + hi);
        // window 1 at its local column 24 (global 40): left 25, right 8, ramp 16 -> 8 / 16; window 3 (last): left 3 -> 3 / 16
        if (stitch_weight(pl, 1, 24) != 0.5f || stitch_weight(pl, 3, 2) != 3.0f / 16.0f || stitch_weight(pl, 2, 8) != 9.0f / 16.0f)
            return fail("hand: weights", 70, 32, 16, 40);
        if (stitch_weight(pl, 0, 0) != 1.0f || stitch_weight(pl, 3, 31) != 1.0f) return fail("hand: ends", 70, 32, 16, 0);
    }
    // the shipped model: W = 1023, default stride 512, L = 3000 -> 5 windows, the last at 1977
    {
        const StitchPlan pl = stitch_plan(3000, 1023, 512);
        if (pl.n != 5 || stitch_start(pl, 3) != 1536 || stitch_start(pl, 4) != 1977) return fail("hand: 3000", 3000, 1023, 512, pl.n);
    }
    std::printf("%ld plans ok\n", plans);
    return 0;
}
