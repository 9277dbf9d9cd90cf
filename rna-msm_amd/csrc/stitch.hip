// Long alignments: the outputs of overlapping windows blended into full-length emb / atp on the device.
//   rows   emb[p, d]    = (sum_w u_w(p) x_w[p - s_w, d]) / (sum_w u_w(p))
//   pairs  atp[h, p, q] = (sum_w (u_w(p) u_w(q)) a_w[h, p - s_w, q - s_w]) / (sum_w u_w(p) u_w(q)),  +0.0 where no window holds both
// over the windows w that contain p (and q), ascending, starting from the first term; every product, sum and quotient is rounded
// on its own (this file is built with contraction off; the plan and the weights are stitch_plan.h's).
// A call applies the windows k0 .. k0 + nb - 1 of the plan -- one window of a one-by-one run, or all of a batched forward -- so
// only one call's windows and the stitched output are ever resident.  Calls come in ascending k0 and together cover 0 .. n - 1.
// One launch per call, one thread per output element of the rows the call's windows span, the element's windows in a loop:
//   - the element's first window in the plan is in this call: the sum starts from its term (what the buffer held is not read);
//     else it continues from the running sum the earlier calls left in the output;
//   - its last window is in this call: the sum is divided by the normalising sum, recomputed here from (L, W, stride) in the same
//     order -- nothing is stored per element;
//   - a pair no window holds is written as +0.0 by the call that applies the first window of its row.
// So every output element is written by exactly one thread of a launch, without atomics, an output full of garbage is defined
// after the last call, and a non-finite value of a window reaches the elements that window covers and no others (u is never 0).
// HBM-bound streaming: a window element is read once; an output element is written once, and read and written once more per
// further call that covers it.  A block is one output row p and 256 consecutive q (rows: the whole of D): a wave reads and writes
// 256 contiguous bytes per instruction; a thread's weights -- u(p) u(q) per window and their sum -- live in registers across its
// loop over the H planes.
#include "common.h"
#include "stitch_plan.h"

#pragma clang fp contract(off)

namespace rnamsm {
namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_PLANE_GROUPS = 8;      // a block walks every 8th plane: the weights are computed once per 15 elements at H = 120

__global__ __launch_bounds__(ST_THREADS) void stitch_rows_kernel(const float* __restrict__ x, int64_t win_stride, int64_t ld,
                                                                 const StitchPlan pl, int k0, int nb, int D, float* __restrict__ out,
                                                                 int p0) {
    const int p = p0 + (int)blockIdx.x;
    int lo, hi;
    stitch_cover(pl, p, lo, hi);
    const int c_lo = lo > k0 ? lo : k0, c_hi = hi < k0 + nb - 1 ? hi : k0 + nb - 1;
    if (c_lo > c_hi) return;                                  // block-uniform (cannot happen inside the call's span)
    float u[STITCH_MAX_COVER], den = 0.f;
    const float* src[STITCH_MAX_COVER];
#pragma unroll
    for (int j = 0; j < STITCH_MAX_COVER; ++j) {
        u[j] = 0.f;
        src[j] = x;
    }
    for (int k = lo; k <= hi; ++k) {
        const int i = p - stitch_start(pl, k);
        const float uk = stitch_weight(pl, k, i);
        den = k == lo ? uk : den + uk;
        const int j = k - c_lo;
        if (j >= 0 && k <= c_hi) {
#pragma unroll
            for (int t = 0; t < STITCH_MAX_COVER; ++t)
                if (t == j) {
                    u[t] = uk;
                    src[t] = x + (int64_t)(k - k0) * win_stride + (int64_t)i * ld;
                }
        }
    }
    const int cnt = c_hi - c_lo + 1;
    const bool from_out = lo < k0, fin = hi < k0 + nb;
    float* o = out + (int64_t)p * D;
    for (int d = threadIdx.x; d < D; d += ST_THREADS) {
        float acc = from_out ? o[d] : 0.f;
#pragma unroll
        for (int j = 0; j < STITCH_MAX_COVER; ++j)
            if (j < cnt) {
                const float t = u[j] * src[j][d];
                acc = (j == 0 && !from_out) ? t : acc + t;
            }
        if (fin && den != 1.0f) acc = acc / den;              // (x / 1 is x: the singly covered columns skip the division)
        o[d] = acc;
    }
}

// Block id = (row of the span) * qtiles + q tile; blockIdx.y = the first plane of the block's walk.
__global__ __launch_bounds__(ST_THREADS) void stitch_pairs_kernel(const float* __restrict__ a, int64_t win_stride, int64_t plane_stride,
                                                                  int64_t ld, int off, const StitchPlan pl, int k0, int nb, int H,
                                                                  float* __restrict__ out, int p0, int qtiles) {
    const int p = p0 + (int)(blockIdx.x / (unsigned)qtiles);
    const int q = (int)(blockIdx.x % (unsigned)qtiles) * ST_THREADS + (int)threadIdx.x;
    if (q >= pl.L) return;
    int lp, hp, lq, hq;
    stitch_cover(pl, p, lp, hp);
    stitch_cover(pl, q, lq, hq);
    const int lo = lp > lq ? lp : lq, hi = hp < hq ? hp : hq;     // the windows that hold both: a run, or none
    const int64_t LL = (int64_t)pl.L * pl.L;
    float* o = out + (int64_t)p * pl.L + q;
    if (lo > hi) {
        if (lp >= k0 && lp < k0 + nb)
            for (int h = blockIdx.y; h < H; h += gridDim.y) o[(int64_t)h * LL] = 0.f;
        return;
    }
    const int c_lo = lo > k0 ? lo : k0, c_hi = hi < k0 + nb - 1 ? hi : k0 + nb - 1;
    if (c_lo > c_hi) return;                                  // another call's element
    float w[STITCH_MAX_COVER], den = 0.f;
    const float* src[STITCH_MAX_COVER];
#pragma unroll
    for (int j = 0; j < STITCH_MAX_COVER; ++j) {
        w[j] = 0.f;
        src[j] = a;
    }
    for (int k = lo; k <= hi; ++k) {
        const int s = stitch_start(pl, k);
        const float wk = stitch_weight(pl, k, p - s) * stitch_weight(pl, k, q - s);
        den = k == lo ? wk : den + wk;
        const int j = k - c_lo;
        if (j >= 0 && k <= c_hi) {
#pragma unroll
            for (int t = 0; t < STITCH_MAX_COVER; ++t)
                if (t == j) {
                    w[t] = wk;
                    src[t] = a + (int64_t)(k - k0) * win_stride + (int64_t)(p - s + off) * ld + (q - s + off);
                }
        }
    }
    const int cnt = c_hi - c_lo + 1;
    const bool from_out = lo < k0, fin = hi < k0 + nb && den != 1.0f;
#pragma unroll 2
    for (int h = blockIdx.y; h < H; h += gridDim.y) {
        float acc = from_out ? o[(int64_t)h * LL] : 0.f;
#pragma unroll
        for (int j = 0; j < STITCH_MAX_COVER; ++j)
            if (j < cnt) {
                const float t = w[j] * src[j][(int64_t)h * plane_stride];
                acc = (j == 0 && !from_out) ? t : acc + t;
            }
        if (fin) acc = acc / den;
        o[(int64_t)h * LL] = acc;
    }
}

inline bool st_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// The checks both entry points share; on success *pl is the plan.
int stitch_check_plan(const char* who, int L, int W, int stride, int k0, int nb, StitchPlan* pl) {
    RNAMSM_CHECK_ARG(W >= 1 && L > W, "%s: L=%d W=%d: the stitcher serves L > W >= 1 (a shorter alignment is one forward)", who, L, W);
    RNAMSM_CHECK_ARG(L <= RNAMSM_STITCH_MAX_L, "%s: L=%d above %d", who, L, RNAMSM_STITCH_MAX_L);
    RNAMSM_CHECK_ARG(stitch_plan_ok(L, W, stride), "%s: stride=%d outside [ceil(W / 2), W] = [%d, %d]", who, stride, (W + 1) / 2, W);
    *pl = stitch_plan(L, W, stride);
    RNAMSM_CHECK_ARG(k0 >= 0 && nb >= 1 && nb <= pl->n - k0, "%s: windows k0=%d nb=%d outside the plan's %d", who, k0, nb, pl->n);
    return RNAMSM_OK;
}

}  // namespace
}  // namespace rnamsm

using namespace rnamsm;

extern "C" int rnamsm_stitch_num_windows(int L, int W, int stride) {
    if (W < 1 || L <= W || L > RNAMSM_STITCH_MAX_L || !stitch_plan_ok(L, W, stride)) return 0;
    return stitch_plan(L, W, stride).n;
}

extern "C" int rnamsm_stitch_rows(const float* x, int64_t win_stride, int64_t ld, int L, int W, int stride, int k0, int nb, int D,
                                  float* out, void* stream) {
    // every refusal comes before the launch: a refused call leaves the stream and the output untouched
    RNAMSM_CHECK_ARG(x && out, "stitch_rows: null pointer");
    StitchPlan pl;
    const int rc = stitch_check_plan("stitch_rows", L, W, stride, k0, nb, &pl);
    if (rc != RNAMSM_OK) return rc;
    RNAMSM_CHECK_ARG(D >= 1 && ld >= D, "stitch_rows: D=%d ld=%lld", D, (long long)ld);
    RNAMSM_CHECK_ARG(nb == 1 || win_stride >= (int64_t)(W - 1) * ld + D, "stitch_rows: window stride %lld below a window's extent",
                     (long long)win_stride);
    RNAMSM_CHECK_ARG(st_aligned4(x) && st_aligned4(out), "stitch_rows: a pointer is not 4-byte aligned");
    const int p0 = stitch_start(pl, k0), p1 = stitch_start(pl, k0 + nb - 1) + W;
    hipLaunchKernelGGL(stitch_rows_kernel, dim3((unsigned)(p1 - p0)), dim3(ST_THREADS), 0, static_cast<hipStream_t>(stream), x,
                       win_stride, ld, pl, k0, nb, D, out, p0);
    RNAMSM_CHECK_LAUNCH("stitch_rows");
    return RNAMSM_OK;
}

extern "C" int rnamsm_stitch_pairs(const float* a, int64_t win_stride, int64_t plane_stride, int64_t ld, int off, int L, int W,
                                   int stride, int k0, int nb, int H, float* out, void* stream) {
    RNAMSM_CHECK_ARG(a && out, "stitch_pairs: null pointer");
    StitchPlan pl;
    const int rc = stitch_check_plan("stitch_pairs", L, W, stride, k0, nb, &pl);
    if (rc != RNAMSM_OK) return rc;
    RNAMSM_CHECK_ARG(H >= 1 && H <= RNAMSM_STITCH_MAX_H, "stitch_pairs: H=%d outside [1, %d]", H, RNAMSM_STITCH_MAX_H);
    RNAMSM_CHECK_ARG(off >= 0 && off <= RNAMSM_STITCH_MAX_L && ld >= (int64_t)W + off, "stitch_pairs: off=%d ld=%lld for windows of W=%d",
                     off, (long long)ld, W);
    RNAMSM_CHECK_ARG(plane_stride >= (int64_t)(W + off - 1) * ld + W + off, "stitch_pairs: plane stride %lld below a plane's extent",
                     (long long)plane_stride);
    RNAMSM_CHECK_ARG(nb == 1 || win_stride >= (int64_t)H * plane_stride, "stitch_pairs: window stride %lld below H planes",
                     (long long)win_stride);
    RNAMSM_CHECK_ARG(st_aligned4(a) && st_aligned4(out), "stitch_pairs: a pointer is not 4-byte aligned");
    const int p0 = stitch_start(pl, k0), p1 = stitch_start(pl, k0 + nb - 1) + W;
    const int qtiles = (L + ST_THREADS - 1) / ST_THREADS;
    const int groups = H < ST_PLANE_GROUPS ? H : ST_PLANE_GROUPS;
    hipLaunchKernelGGL(stitch_pairs_kernel, dim3((unsigned)((int64_t)(p1 - p0) * qtiles), (unsigned)groups), dim3(ST_THREADS), 0,
                       static_cast<hipStream_t>(stream), a, win_stride, plane_stride, ld, off, pl, k0, nb, H, out, p0, qtiles);
    RNAMSM_CHECK_LAUNCH("stitch_pairs");
    return RNAMSM_OK;
}
