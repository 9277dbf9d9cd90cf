// Host check of rna-msm_amd/csrc/stitch_plan.h, the header the device stitcher computes its window plan with.
//   stitch_plan_check                 every plan of W <= 24 (all admissible strides, L up to 3 W + 5) against a brute-force
//                                     restatement: starts, window count, the windows that contain a column, the weights' ranges;
//                                     then a few hand-computed plans; then the same brute force at the shipped width (W = 1023,
//                                     L up to 4096) and at the length limit RNAMSM_STITCH_MAX_L = 2^19 (windows of 2^18 columns, and
//                                     1024 windows of 1023, there on the columns near both ends and every 97th in between).
//                                     Prints "plans ok"; exit 1 with a message otherwise.
//   stitch_plan_check L W stride      prints the starts, then every window's weights as fp32 bit patterns (hex), one per line.
// Built by tests/test_windows_host.py and by `make check-asan` with -fsanitize=address,undefined.
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

// sampled: the columns within 2 W of either end and every 97th in between (the plan is periodic in between); else every column.
static int check(int L, int W, int stride, bool sampled = false) {
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
        if (sampled && p >= 2 * W && p < L - 2 * W && p % 97) continue;
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
    // the shipped width up to RNAMSM_LONG_MAX_L, and the length limit of the stitcher
    {
        const int strides[3] = {512, 700, 1023}, lengths[4] = {1024, 1535, 2047, 4096};
        for (int s = 0; s < 3; ++s)
            for (int l = 0; l < 4; ++l, ++plans)
                if (check(lengths[l], 1023, strides[s])) return 1;
        const int LMAX = 1 << 19;
        if (check(LMAX, (1 << 18) + 1, (1 << 17) + 1) || check(LMAX - 3, 300001, 150001)) return 1;
        if (stitch_plan(LMAX, 1023, 512).n != 1024 || check(LMAX, 1023, 512, true)) return 1;
        plans += 3;
        const StitchPlan pl = stitch_plan(LMAX, (1 << 18) + 1, (1 << 17) + 1);        // starts 0, 2^17 + 1, 2^18 - 1; ramp 2^17
        if (pl.n != 3 || stitch_start(pl, 1) != 131073 || stitch_start(pl, 2) != 262143 || pl.ramp != 131072)
            return fail("hand: 2^19", LMAX, pl.W, pl.stride, pl.n);
        // column 2^18 lies in all three; in window 1 (local 131071) left 131072, right 131074 -> 1; in window 2 (local 1) left 2 -> 2^-16
        int lo, hi;
        stitch_cover(pl, 1 << 18, lo, hi);
        if (lo != 0 || hi != 2) return fail("hand: cover of 2^18", LMAX, pl.W, pl.stride, lo * 10 + hi);
        if (stitch_weight(pl, 0, 1 << 18) != 1.0f / 131072.0f || stitch_weight(pl, 1, 131071) != 1.0f ||
            stitch_weight(pl, 2, 1) != 2.0f / 131072.0f)
            return fail("hand: weights at 2^18", LMAX, pl.W, pl.stride, 1 << 18);
    }
    std::printf("%ld plans ok\n", plans);
    return 0;
}
