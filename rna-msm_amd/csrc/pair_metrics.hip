// A pair map against a target structure, counted on the device (include/rnamsm.h states both rules).
//
// sweep      the reference's threshold sweep (utils/metrics.py rna_compute_precisions: predictions[n, 1] >= T[1, 1001], four sums over
//            n) without the n x T array: a candidate's BIN is the number of thresholds it reaches, so tp[t] / fp[t] are the positives /
//            negatives whose bin is above t -- one histogram of 2 * (T + 1) integer bins and one suffix sum.
//   ps_init_kernel    clears the global table
//   ps_hist_kernel    block b streams the row pieces b, b + gridDim.x, ... (a piece = 2048 consecutive columns of one row, thread t the
//                     columns seg * 2048 + e * 256 + t as in top_pairs.hip; a piece left of the band or of a skipped row is passed over).
//                     The thresholds lie in LDS once per block; a value takes one comparison with the last threshold and a binary search
//                     of 12 steps over the others; the block's histogram lies in LDS beside them.  Equal bins are added once per wave
//                     (two rounds of "the first lane's bin and everyone who shares it", then one add per lane that is left: a map that
//                     is all one value, or two, costs one or two LDS adds per wave and row piece).  At the end one 64-bit integer add
//                     per used bin into the global table: integer adds commute, no output bit depends on their order.
//   ps_finish_kernel  one block: the inclusive sums of both halves of the table (block_scan.h, in 64 bits), then tp, fp, tn = N - fp, fn = P - tp.
//
// precision  the reference's compute_precisions: the hits among the first cuts[c] pairs of the ranked list.
//   pp_mask_kernel    a copy of the candidate band with NaN at every excluded pair (negative target, j - i >= max_sep): exclusion is
//                     then top_pairs' own NaN rule and the selection is rnamsm_top_pairs_f64 / _f32 itself, called as it is
//   pp_hits_kernel    one block: the target at the n listed pairs, 1024 ranks at a time, one inclusive scan (block_scan.h) and the running
//                     sum read at the cuts.
#include "common.h"
#include "block_scan.h"

namespace rnamsm {

constexpr int PM_MAX_L = 32768, PM_MAX_K = 65536, PM_MAX_SEP = 32768, PM_MAX_T = 4096, PM_MAX_CUTS = 64;
constexpr int PM_THREADS = 256, PM_PER = 8, PM_SEG = PM_THREADS * PM_PER;
constexpr int PS_MAX_BLOCKS = 1024;

static size_t pm_round(size_t n) { return (n + 255) & ~(size_t)255; }

// ---- the sweep -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ps_init_kernel(unsigned long long* __restrict__ table, int nb) {
    for (int q = threadIdx.x; q < nb; q += 256) table[q] = 0;
}

// the number of thresholds v reaches: th[0 .. nt - 1) ascending in LDS, `top` = the last one.  NaN reaches none.
__device__ __forceinline__ int ps_bin(const double* s_th, double top, int nt, double v) {
    if (v >= top) return nt;
    int pos = 0;                                                             // v >= th[pos - 1], or pos = 0
#pragma unroll
    for (int step = PM_MAX_T / 2; step > 0; step >>= 1) {
        const int q = pos + step;
        if (q < nt && v >= s_th[q - 1]) pos = q;
    }
    return pos;
}

// one count into bin h of the block's histogram for every lane with m set; h is in range in every lane
__device__ __forceinline__ void ps_add(unsigned* s_hist, bool m, int h, int lane) {
    uint64_t act = __ballot(m);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (!act) break;                                                     // (the same for the whole wave)
        const int lead = __ffsll((unsigned long long)act) - 1;
        const int h0 = __shfl(h, lead, 64);
        const uint64_t same = __ballot(m && h == h0);
        if (lane == lead) atomicAdd(&s_hist[h0], (unsigned)__popcll(same));
        if (h == h0) m = false;
        act &= ~same;
    }
    if (m) atomicAdd(&s_hist[h], 1u);
}

// grid min(pieces, 1024); dynamic LDS: (nt - 1) doubles, then 2 * (nt + 1) counters (64 KiB at nt = 4096)
template <class T>
__global__ __launch_bounds__(PM_THREADS) void ps_hist_kernel(const T* __restrict__ x, int L, int64_t ld, const int8_t* __restrict__ target,
                                                             int64_t ld_t, const uint8_t* __restrict__ skip, int min_sep,
                                                             const double* __restrict__ thresholds, int nt, int pieces, int nseg,
                                                             unsigned long long* __restrict__ table) {
    extern __shared__ double ps_lds[];
    double* s_th = ps_lds;
    unsigned* s_hist = reinterpret_cast<unsigned*>(ps_lds + (nt - 1));
    const int t = threadIdx.x, lane = t & 63, nb = 2 * (nt + 1);
    for (int q = t; q < nt - 1; q += PM_THREADS) s_th[q] = thresholds[q];
    for (int q = t; q < nb; q += PM_THREADS) s_hist[q] = 0;
    const double top = thresholds[nt - 1];
    __syncthreads();
    for (int p = blockIdx.x; p < pieces; p += gridDim.x) {
        const int i = p / nseg, seg = p - i * nseg;
        if ((seg + 1) * PM_SEG <= i + min_sep) continue;                     // the piece lies left of the band
        if (skip && skip[i]) continue;
        const T* row = x + (int64_t)i * ld;
        const int8_t* trow = target + (int64_t)i * ld_t;
        const int j0 = seg * PM_SEG + t, first = i + min_sep;
        T raw[PM_PER];
        int8_t tg[PM_PER];
        unsigned in = 0;
#pragma unroll
        for (int e = 0; e < PM_PER; ++e) {
            const int j = j0 + e * PM_THREADS;
            const bool v = j >= first && j < L && !(skip && skip[j]);
            raw[e] = v ? row[j] : (T)0;
            tg[e] = v ? trow[j] : (int8_t)0;
            in |= v ? 1u << e : 0u;
        }
#pragma unroll
        for (int e = 0; e < PM_PER; ++e) {
            const bool m = (in >> e) & 1u;
            const int h = ps_bin(s_th, top, nt, (double)raw[e]) + (tg[e] != 0 ? nt + 1 : 0);
            ps_add(s_hist, m, h, lane);
        }
    }
    __syncthreads();
    for (int q = t; q < nb; q += PM_THREADS)
        if (s_hist[q]) atomicAdd(&table[q], (unsigned long long)s_hist[q]);
}

// one block: table = [negatives by bin (nt + 1), positives by bin (nt + 1)] -> counts int64 [4, nt]: tp, fp, tn, fn
__global__ __launch_bounds__(1024) void ps_finish_kernel(const unsigned long long* __restrict__ table, int nt, long long* __restrict__ counts) {
    __shared__ unsigned long long s[1024];
    __shared__ unsigned long long s_total[2];
    const int t = threadIdx.x, nb1 = nt + 1;
    const int per = (nb1 + 1023) / 1024;
    const int lo = t * per < nb1 ? t * per : nb1, hi = lo + per < nb1 ? lo + per : nb1;
    unsigned long long upto[2][(PM_MAX_T + 1 + 1023) / 1024];                // inclusive sums of this thread's bins, per half
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const unsigned long long* h = table + half * nb1;
        unsigned long long sum = 0;
#pragma unroll
        for (int q = 0; q < (PM_MAX_T + 1 + 1023) / 1024; ++q) {
            if (lo + q < hi) sum += h[lo + q];
            upto[half][q] = sum;
        }
        const unsigned long long incl = block_inclusive_sum(sum, s);
        if (t == 1023) s_total[half] = incl;
#pragma unroll
        for (int q = 0; q < (PM_MAX_T + 1 + 1023) / 1024; ++q) upto[half][q] += incl - sum;
    }
    __syncthreads();
    const unsigned long long N = s_total[0], P = s_total[1];
#pragma unroll
    for (int q = 0; q < (PM_MAX_T + 1 + 1023) / 1024; ++q) {
        const int b = lo + q;                                                // threshold b: the candidates whose bin is above b
        if (b < hi && b < nt) {
            const unsigned long long fp = N - upto[0][q], tp = P - upto[1][q];
            counts[b] = (long long)tp;
            counts[(size_t)nt + b] = (long long)fp;
            counts[2 * (size_t)nt + b] = (long long)(N - fp);
            counts[3 * (size_t)nt + b] = (long long)(P - tp);
        }
    }
}

template <class T>
static int ps_run(const char* name, const T* x, int L, int64_t ld, const int8_t* target, int64_t ld_t, const uint8_t* skip, int min_sep,
                  const double* thresholds, int nt, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    RNAMSM_CHECK_ARG(x && target && thresholds && counts && workspace, "%s: null pointer", name);
    RNAMSM_CHECK_ARG(L >= 2 && L <= PM_MAX_L, "%s: L=%d outside [2, %d]", name, L, PM_MAX_L);
    RNAMSM_CHECK_ARG(nt >= 1 && nt <= PM_MAX_T, "%s: T=%d outside [1, %d]", name, nt, PM_MAX_T);
    RNAMSM_CHECK_ARG(min_sep >= 1 && min_sep <= PM_MAX_SEP, "%s: min_sep=%d outside [1, %d]", name, min_sep, PM_MAX_SEP);
    RNAMSM_CHECK_ARG(ld >= L, "%s: ld=%lld is smaller than L=%d", name, (long long)ld, L);
    RNAMSM_CHECK_ARG(ld_t >= L, "%s: ld_t=%lld is smaller than L=%d", name, (long long)ld_t, L);
    const size_t need = rnamsm_pair_sweep_workspace_bytes(nt);
    RNAMSM_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes is smaller than the %zu that T=%d needs", name, workspace_bytes,
                     need, nt);
    RNAMSM_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "%s: workspace misaligned (256 bytes)", name);
    RNAMSM_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & (sizeof(T) - 1)) == 0 && (reinterpret_cast<uintptr_t>(thresholds) & 7u) == 0 &&
                         (reinterpret_cast<uintptr_t>(counts) & 7u) == 0,
                     "%s: x / thresholds / counts misaligned", name);
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long* table = static_cast<unsigned long long*>(workspace);
    const int nb = 2 * (nt + 1);
    const int nseg = (L + PM_SEG - 1) / PM_SEG;
    const int rows = L - min_sep > 1 ? L - min_sep : 1;                      // rows from L - min_sep on hold no candidate
    const int pieces = rows * nseg;
    const int grid = pieces < PS_MAX_BLOCKS ? pieces : PS_MAX_BLOCKS;
    const size_t lds = (size_t)(nt - 1) * 8 + (size_t)nb * 4;                // <= 65536: no attribute to set
    hipLaunchKernelGGL(ps_init_kernel, dim3(1), dim3(256), 0, s, table, nb);
    hipLaunchKernelGGL(ps_hist_kernel<T>, dim3(grid), dim3(PM_THREADS), lds, s, x, L, ld, target, ld_t, skip, min_sep, thresholds, nt,
                       pieces, nseg, table);
    hipLaunchKernelGGL(ps_finish_kernel, dim3(1), dim3(1024), 0, s, table, nt, reinterpret_cast<long long*>(counts));
    RNAMSM_CHECK_LAUNCH(name);
    return RNAMSM_OK;
}

// ---- precision at the cuts -------------------------------------------------------------------------------------------------------
// grid (nseg, rows): masked [L, L] (leading dimension L) gets the band's values, NaN where the pair is excluded.  Only the band is
// written -- top_pairs reads nothing else -- and x is read only where the pair is a candidate.
template <class T>
__global__ __launch_bounds__(PM_THREADS) void pp_mask_kernel(const T* __restrict__ x, int L, int64_t ld, const int8_t* __restrict__ target,
                                                             int64_t ld_t, int min_sep, int max_sep, T* __restrict__ masked) {
    const int i = blockIdx.y, seg = blockIdx.x, t = threadIdx.x;
    if ((seg + 1) * PM_SEG <= i + min_sep) return;
    const T* row = x + (int64_t)i * ld;
    const int8_t* trow = target + (int64_t)i * ld_t;
    T* out = masked + (int64_t)i * L;
    const int first = i + min_sep;
#pragma unroll
    for (int e = 0; e < PM_PER; ++e) {
        const int j = seg * PM_SEG + e * PM_THREADS + t;
        if (j < first || j >= L) continue;
        const bool ok = (max_sep <= 0 || j - i < max_sep) && trow[j] >= 0;
        out[j] = ok ? row[j] : (T)__builtin_nan("");
    }
}

// one block of 1024 threads
__global__ __launch_bounds__(1024) void pp_hits_kernel(const int32_t* __restrict__ pairs, const int32_t* __restrict__ count, int k,
                                                       const int8_t* __restrict__ target, int64_t ld_t, const int32_t* __restrict__ cuts,
                                                       int ncuts, int32_t* __restrict__ hits) {
    __shared__ int s[1024];
    __shared__ int s_cut[PM_MAX_CUTS];
    __shared__ int s_base;
    const int t = threadIdx.x;
    int n = *count;
    n = n < 0 ? 0 : (n > k ? k : n);
    if (t < ncuts) {
        int c = cuts[t];
        c = c < 0 ? 0 : (c > n ? n : c);                                     // the first min(cuts[c], n) pairs
        s_cut[t] = c;
        if (c == 0) hits[t] = 0;
    }
    if (t == 0) s_base = 0;
    __syncthreads();
    for (int start = 0; start < n; start += 1024) {
        const int r = start + t;
        int f = 0;
        if (r < n) f = target[(int64_t)pairs[2 * (size_t)r] * ld_t + pairs[2 * (size_t)r + 1]] > 0 ? 1 : 0;
        const int upto = s_base + block_inclusive_sum(f, s);                 // the hits among the ranks 0 .. r
        for (int c = 0; c < ncuts; ++c)
            if (s_cut[c] - 1 == r) hits[c] = upto;
        __syncthreads();
        if (t == 1023) s_base = upto;
        __syncthreads();
    }
}

struct PpWs {
    size_t masked, pairs, scores, top, total, top_bytes;     // offsets, each a multiple of 256
};
static PpWs pp_ws(int L, int k, int elem_bytes) {
    PpWs w;
    w.masked = 0;
    w.pairs = pm_round((size_t)L * L * elem_bytes);
    w.scores = w.pairs + pm_round((size_t)k * 8);
    w.top = w.scores + pm_round((size_t)k * 8);
    w.top_bytes = rnamsm_top_pairs_workspace_bytes(L, k);
    w.total = w.top + w.top_bytes;
    return w;
}
static bool pp_shape_ok(int L, int k, int elem_bytes) {
    return L >= 2 && L <= PM_MAX_L && k >= 1 && k <= PM_MAX_K && (elem_bytes == 4 || elem_bytes == 8);
}

static int pp_top(const double* m, int L, int min_sep, int k, int32_t* pairs, double* scores, int32_t* count, void* ws, size_t bytes, void* s) {
    return rnamsm_top_pairs_f64(m, L, L, min_sep, k, pairs, scores, count, ws, bytes, s);
}
static int pp_top(const float* m, int L, int min_sep, int k, int32_t* pairs, double* scores, int32_t* count, void* ws, size_t bytes, void* s) {
    return rnamsm_top_pairs_f32(m, L, L, min_sep, k, pairs, scores, count, ws, bytes, s);
}

template <class T>
static int pp_run(const char* name, const T* x, int L, int64_t ld, const int8_t* target, int64_t ld_t, int min_sep, int max_sep, int k,
                  const int32_t* cuts, int ncuts, int32_t* hits, int32_t* count, int32_t* pairs, double* scores, void* workspace,
                  size_t workspace_bytes, void* stream) {
    RNAMSM_CHECK_ARG(x && target && cuts && hits && count && workspace, "%s: null pointer", name);
    RNAMSM_CHECK_ARG(L >= 2 && L <= PM_MAX_L, "%s: L=%d outside [2, %d]", name, L, PM_MAX_L);
    RNAMSM_CHECK_ARG(k >= 1 && k <= PM_MAX_K, "%s: k=%d outside [1, %d]", name, k, PM_MAX_K);
    RNAMSM_CHECK_ARG(ncuts >= 1 && ncuts <= PM_MAX_CUTS, "%s: ncuts=%d outside [1, %d]", name, ncuts, PM_MAX_CUTS);
    RNAMSM_CHECK_ARG(min_sep >= 1 && min_sep <= PM_MAX_SEP, "%s: min_sep=%d outside [1, %d]", name, min_sep, PM_MAX_SEP);
    RNAMSM_CHECK_ARG(max_sep >= 0, "%s: max_sep=%d is negative (0 = no upper limit)", name, max_sep);
    RNAMSM_CHECK_ARG(ld >= L, "%s: ld=%lld is smaller than L=%d", name, (long long)ld, L);
    RNAMSM_CHECK_ARG(ld_t >= L, "%s: ld_t=%lld is smaller than L=%d", name, (long long)ld_t, L);
    const PpWs w = pp_ws(L, k, (int)sizeof(T));
    // (what rnamsm_top_pairs_* itself checks -- L, k, min_sep, its workspace's size and alignment -- is settled here, before the first
    // launch: its size function answers 0 for a shape it would refuse, and its share of the workspace starts on a multiple of 256)
    RNAMSM_CHECK_ARG(w.top_bytes > 0 && w.top % 256 == 0, "%s: L=%d, k=%d are outside what the selection takes", name, L, k);
    RNAMSM_CHECK_ARG(workspace_bytes >= w.total, "%s: workspace of %zu bytes is smaller than the %zu that L=%d, k=%d need", name,
                     workspace_bytes, w.total, L, k);
    RNAMSM_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "%s: workspace misaligned (256 bytes)", name);
    RNAMSM_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & (sizeof(T) - 1)) == 0 && (reinterpret_cast<uintptr_t>(cuts) & 3u) == 0 &&
                         (reinterpret_cast<uintptr_t>(hits) & 3u) == 0 && (reinterpret_cast<uintptr_t>(count) & 3u) == 0 &&
                         (reinterpret_cast<uintptr_t>(pairs) & 3u) == 0 && (reinterpret_cast<uintptr_t>(scores) & 7u) == 0,
                     "%s: x / cuts / hits / count / pairs / scores misaligned", name);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    T* masked = reinterpret_cast<T*>(ws + w.masked);
    if (!pairs) pairs = reinterpret_cast<int32_t*>(ws + w.pairs);
    if (!scores) scores = reinterpret_cast<double*>(ws + w.scores);
    const int nseg = (L + PM_SEG - 1) / PM_SEG;
    const int rows = L - min_sep > 1 ? L - min_sep : 1;
    hipLaunchKernelGGL(pp_mask_kernel<T>, dim3(nseg, rows), dim3(PM_THREADS), 0, s, x, L, ld, target, ld_t, min_sep, max_sep, masked);
    RNAMSM_CHECK_LAUNCH(name);
    const int rc = pp_top(masked, L, min_sep, k, pairs, scores, count, ws + w.top, w.top_bytes, stream);   // (every argument was checked above)
    if (rc != RNAMSM_OK) return rc;
    hipLaunchKernelGGL(pp_hits_kernel, dim3(1), dim3(1024), 0, s, pairs, count, k, target, ld_t, cuts, ncuts, hits);
    RNAMSM_CHECK_LAUNCH(name);
    return RNAMSM_OK;
}

}  // namespace rnamsm

using namespace rnamsm;

extern "C" size_t rnamsm_pair_sweep_workspace_bytes(int T) {
    if (T < 1 || T > PM_MAX_T) return 0;
    return pm_round((size_t)2 * (T + 1) * 8);
}

extern "C" int rnamsm_pair_sweep_f64(const double* x, int L, int64_t ld, const int8_t* target, int64_t ld_t, const uint8_t* skip,
                                     int min_sep, const double* thresholds, int T, int64_t* counts, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    return ps_run<double>("pair_sweep_f64", x, L, ld, target, ld_t, skip, min_sep, thresholds, T, counts, workspace, workspace_bytes, stream);
}

extern "C" int rnamsm_pair_sweep_f32(const float* x, int L, int64_t ld, const int8_t* target, int64_t ld_t, const uint8_t* skip,
                                     int min_sep, const double* thresholds, int T, int64_t* counts, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    return ps_run<float>("pair_sweep_f32", x, L, ld, target, ld_t, skip, min_sep, thresholds, T, counts, workspace, workspace_bytes, stream);
}

extern "C" size_t rnamsm_pair_precision_workspace_bytes(int L, int k, int elem_bytes) {
    if (!pp_shape_ok(L, k, elem_bytes)) return 0;
    return pp_ws(L, k, elem_bytes).total;
}

extern "C" int rnamsm_pair_precision_f64(const double* x, int L, int64_t ld, const int8_t* target, int64_t ld_t, int min_sep, int max_sep,
                                         int k, const int32_t* cuts, int ncuts, int32_t* hits, int32_t* count, int32_t* pairs,
                                         double* scores, void* workspace, size_t workspace_bytes, void* stream) {
    return pp_run<double>("pair_precision_f64", x, L, ld, target, ld_t, min_sep, max_sep, k, cuts, ncuts, hits, count, pairs, scores,
                          workspace, workspace_bytes, stream);
}

extern "C" int rnamsm_pair_precision_f32(const float* x, int L, int64_t ld, const int8_t* target, int64_t ld_t, int min_sep, int max_sep,
                                         int k, const int32_t* cuts, int ncuts, int32_t* hits, int32_t* count, int32_t* pairs,
                                         double* scores, void* workspace, size_t workspace_bytes, void* stream) {
    return pp_run<float>("pair_precision_f32", x, L, ld, target, ld_t, min_sep, max_sep, k, cuts, ncuts, hits, count, pairs, scores,
                         workspace, workspace_bytes, stream);
}
