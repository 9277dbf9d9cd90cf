// The top-k ranked pairs of an L x L map on the device (include/rnamsm.h states the rule).
//
// Candidates: the pairs (i, j), i < j, j - i >= min_sep, x[i, j] not NaN -- nothing else of x is read.  The order is total: larger
// value first (-0.0 as +0.0), then smaller i, then smaller j, i.e. larger key (top_pairs_key.h) first, then smaller row-major index
// i * L + j.  All of it in integers; nothing in the result depends on the order in which an atomic lands.
//
// Data flow, every launch on the caller's stream, every buffer in the caller's workspace, nothing read back:
//   A block of the streaming kernels owns TP_SEG = 2048 consecutive columns of ONE row: block (seg, i), linear id i * nseg + seg, so
//   block ids ascend with the row-major index.  Thread t reads the columns seg * 2048 + e * 256 + t, e = 0 .. 7 (one coalesced row
//   piece per e).  A block whose columns all lie left of i + min_sep returns at once; only rows below L - min_sep are launched.
//   select   the k-th largest key by radix select, 8-bit digits from the top: per pass a histogram of the digit over the candidates
//            whose higher digits equal the prefix chosen so far (LDS counters per block, one 64-bit integer add per used bin into
//            the global table: integer adds commute), then one block walks the 256 bins from the top and fixes the next digit.  The
//            prefix and the number still wanted stay in device memory (TpState).  Pass 0 also gives the number of candidates, hence
//            n = min(k, candidates).                                                              tp_hist_kernel, tp_select_kernel
//   count    with the threshold key T complete: records strictly above T (fewer than n) go to the selected list at slots handed out
//            by an integer counter -- their place in the list means nothing, the ranking below sorts them; the records EQUAL to T
//            are only counted, per block                                                                     tp_count_kernel
//   scan     the exclusive sum of the per-block tie counts in block order = row-major order                   tp_scan_kernel
//   ties     of the ties, the `need` = n - #above with the smallest row-major index win: a block whose offset is below need reads
//            its columns again and writes its ties in index order (ballot ranks within the wave, wave counts through LDS, e by e)
//            while the running offset is below need                                                          tp_ties_kernel
//   rank     rank of a selected record = the number of selected records that precede it in the total order: n x n comparisons, the
//            list staged 256 records at a time in LDS, one record per thread.  The records are distinct (the index is), so the ranks
//            are a permutation of 0 .. n - 1 and every output row below n is written once; the threads past n write the fill rows
//            (-1, -1, NaN) and one thread the count                                                          tp_rank_kernel
#include "common.h"
#include "top_pairs_key.h"

namespace rnamsm {

constexpr int TP_MAX_L = 32768, TP_MAX_K = 65536, TP_MAX_SEP = 32768;
constexpr int TP_THREADS = 256, TP_PER = 8, TP_SEG = TP_THREADS * TP_PER;

struct TpState {
    unsigned long long prefix;     // the digits of the threshold key fixed so far, the last one in the low byte
    unsigned long long need;       // of the candidates whose top digits equal prefix, how many are wanted (after pass 7: the ties wanted)
    unsigned long long total;      // the number of candidates
    uint32_t n;                    // min(k, total): the rows of the result
    uint32_t above;                // slots of the selected list handed out to records strictly above the threshold
};

__device__ __forceinline__ bool tp_block_empty(int i, int seg, int min_sep) { return (seg + 1) * TP_SEG <= i + min_sep; }

// The block's 8 columns per thread: key[e] of column seg * 2048 + e * 256 + t, bit e of the result set where that column is a
// candidate (inside the band and the map, not NaN).  Columns that are no candidates are not read.
template <class T>
__device__ __forceinline__ unsigned tp_load(const T* __restrict__ x, int L, int64_t ld, int min_sep, int i, int seg, uint64_t (&key)[TP_PER]) {
    const T* row = x + (int64_t)i * ld;
    const int j0 = seg * TP_SEG + (int)threadIdx.x, first = i + min_sep;
    T raw[TP_PER];
    unsigned in = 0;
#pragma unroll
    for (int e = 0; e < TP_PER; ++e) {
        const int j = j0 + e * TP_THREADS;
        const bool v = j >= first && j < L;
        raw[e] = v ? row[j] : (T)0;
        in |= v ? 1u << e : 0u;
    }
    unsigned ok = 0;
#pragma unroll
    for (int e = 0; e < TP_PER; ++e) {
        const double v = (double)raw[e];
        key[e] = tp_key(v);
        ok |= (((in >> e) & 1u) && v == v) ? 1u << e : 0u;
    }
    return ok;
}

__global__ __launch_bounds__(256) void tp_init_kernel(TpState* __restrict__ st, unsigned long long* __restrict__ hist) {
    hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        st->prefix = 0;
        st->need = 0;
        st->total = 0;
        st->n = 0;
        st->above = 0;
    }
}

// grid (nseg, rows)
template <class T>
__global__ __launch_bounds__(TP_THREADS) void tp_hist_kernel(const T* __restrict__ x, int L, int64_t ld, int min_sep, int pass,
                                                             const TpState* __restrict__ st, unsigned long long* __restrict__ hist) {
    const int i = blockIdx.y, seg = blockIdx.x, t = threadIdx.x, lane = t & 63;
    if (tp_block_empty(i, seg, min_sep)) return;
    __shared__ unsigned s_hist[256];
    s_hist[t] = 0;
    __syncthreads();
    uint64_t key[TP_PER];
    const unsigned ok = tp_load(x, L, ld, min_sep, i, seg, key);
    const uint64_t prefix = pass ? st->prefix : 0;
    const int high = pass ? 64 - 8 * pass : 63, low = 56 - 8 * pass;        // (pass 0: every candidate matches)
#pragma unroll
    for (int e = 0; e < TP_PER; ++e) {
        const bool m = ((ok >> e) & 1u) && (pass == 0 || (key[e] >> high) == prefix);
        const int d = (int)((key[e] >> low) & 255u);
        const uint64_t act = __ballot(m);
        if (act) {                                                           // (the same for the whole wave)
            // the digit of the first matching lane is added once for all lanes that share it: the top digits of a map are few
            const int lead = __ffsll((unsigned long long)act) - 1;
            const int d0 = __shfl(d, lead, 64);
            const uint64_t same = __ballot(m && d == d0);
            if (lane == lead) atomicAdd(&s_hist[d0], (unsigned)__popcll(same));
            else if (m && d != d0) atomicAdd(&s_hist[d], 1u);
        }
    }
    __syncthreads();
    if (s_hist[t]) atomicAdd(&hist[t], (unsigned long long)s_hist[t]);
}

// one block: the next digit of the threshold key from the pass's histogram, which is cleared for the next pass
__global__ __launch_bounds__(256) void tp_select_kernel(int pass, int k, TpState* __restrict__ st, unsigned long long* __restrict__ hist) {
    __shared__ unsigned long long s[256];
    const int t = threadIdx.x;
    s[t] = hist[t];
    hist[t] = 0;
    __syncthreads();
    if (t != 0) return;
    unsigned long long need = st->need;
    if (pass == 0) {
        unsigned long long total = 0;
        for (int d = 0; d < 256; ++d) total += s[d];
        need = total < (unsigned long long)k ? total : (unsigned long long)k;
        st->total = total;
        st->n = (uint32_t)need;
    }
    int d = 0;
    if (need > 0) {
        unsigned long long over = 0;                   // the candidates in the bins above d
        for (d = 255; d > 0; --d) {
            if (over + s[d] >= need) break;
            over += s[d];
        }
        need -= over;
    }
    st->prefix = (st->prefix << 8) | (unsigned long long)d;
    st->need = need;
}

// grid (nseg, rows); tie_cnt[block] for EVERY block of the grid
template <class T>
__global__ __launch_bounds__(TP_THREADS) void tp_count_kernel(const T* __restrict__ x, int L, int64_t ld, int min_sep, int k,
                                                              TpState* __restrict__ st, uint64_t* __restrict__ sel_key,
                                                              uint32_t* __restrict__ sel_idx, uint32_t* __restrict__ tie_cnt) {
    const int i = blockIdx.y, seg = blockIdx.x, t = threadIdx.x;
    const int b = i * (int)gridDim.x + seg;
    if (tp_block_empty(i, seg, min_sep) || st->n == 0) {
        if (t == 0) tie_cnt[b] = 0;
        return;
    }
    __shared__ unsigned s_above, s_ties, s_base;
    if (t == 0) s_above = s_ties = 0;
    __syncthreads();
    uint64_t key[TP_PER];
    const unsigned ok = tp_load(x, L, ld, min_sep, i, seg, key);
    const uint64_t thr = st->prefix;
    unsigned am = 0, na = 0, nt = 0;
#pragma unroll
    for (int e = 0; e < TP_PER; ++e) {
        if (!((ok >> e) & 1u)) continue;
        if (key[e] > thr) { am |= 1u << e; ++na; }
        else if (key[e] == thr) ++nt;
    }
    unsigned mine = 0;
    if (na) mine = atomicAdd(&s_above, na);
    if (nt) atomicAdd(&s_ties, nt);
    __syncthreads();
    if (t == 0) {
        tie_cnt[b] = s_ties;
        s_base = s_above ? atomicAdd(&st->above, s_above) : 0u;
    }
    __syncthreads();
    if (!na) return;
    unsigned pos = s_base + mine;
#pragma unroll
    for (int e = 0; e < TP_PER; ++e) {
        if (!((am >> e) & 1u)) continue;
        if (pos < (unsigned)k) {                      // (fewer than n <= k records lie above the threshold: the guard never bites)
            sel_key[pos] = key[e];
            sel_idx[pos] = (uint32_t)i * (uint32_t)L + (uint32_t)(seg * TP_SEG + e * TP_THREADS + t);
        }
        ++pos;
    }
}

// one block: cnt[0 .. nb) -> its exclusive sums in place, cnt[nb] = the total.  At most 5.4e8 candidates: 32 bits hold every sum.
__global__ __launch_bounds__(1024) void tp_scan_kernel(uint32_t* __restrict__ cnt, int nb) {
    __shared__ unsigned s[1024];
    const int t = threadIdx.x;
    const int per = (nb + 1023) / 1024;
    const int lo = t * per, hi = lo + per < nb ? lo + per : nb;
    unsigned sum = 0;
    for (int b = lo; b < hi; ++b) sum += cnt[b];
    s[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {                            // inclusive scan
        const unsigned v = t >= off ? s[t - off] : 0u;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    unsigned run = s[t] - sum;
    for (int b = lo; b < hi; ++b) {
        const unsigned c = cnt[b];
        cnt[b] = run;
        run += c;
    }
    if (t == 1023) cnt[nb] = s[1023];
}

// grid (nseg, rows)
template <class T>
__global__ __launch_bounds__(TP_THREADS) void tp_ties_kernel(const T* __restrict__ x, int L, int64_t ld, int min_sep, int k,
                                                             const TpState* __restrict__ st, uint64_t* __restrict__ sel_key,
                                                             uint32_t* __restrict__ sel_idx, const uint32_t* __restrict__ tie_off) {
    const int i = blockIdx.y, seg = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (tp_block_empty(i, seg, min_sep)) return;
    const unsigned n = st->n;
    if (n == 0) return;
    const int b = i * (int)gridDim.x + seg;
    const unsigned need = (unsigned)st->need, off = tie_off[b], cnt = tie_off[b + 1] - off;
    if (cnt == 0 || off >= need) return;                                   // (the same for the whole block)
    __shared__ unsigned s_w[TP_THREADS / 64];
    uint64_t key[TP_PER];
    const unsigned ok = tp_load(x, L, ld, min_sep, i, seg, key);
    const uint64_t thr = st->prefix;
    const unsigned base = n - need;                                        // the records above the threshold come first
    unsigned run = off;
#pragma unroll
    for (int e = 0; e < TP_PER; ++e) {
        const bool f = ((ok >> e) & 1u) && key[e] == thr;
        const uint64_t m = __ballot(f);
        if (lane == 0) s_w[w] = (unsigned)__popcll(m);
        __syncthreads();
        unsigned before = 0, all = 0;
#pragma unroll
        for (int q = 0; q < TP_THREADS / 64; ++q) {
            const unsigned c = s_w[q];
            before += q < w ? c : 0u;
            all += c;
        }
        const unsigned pos = run + before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (f && pos < need && base + pos < (unsigned)k) {
            sel_key[base + pos] = key[e];
            sel_idx[base + pos] = (uint32_t)i * (uint32_t)L + (uint32_t)(seg * TP_SEG + e * TP_THREADS + t);
        }
        run += all;
        __syncthreads();
    }
}

// grid ceil(k / 256): thread s ranks selected record s (s < n) or writes fill row s (n <= s < k)
__global__ __launch_bounds__(256) void tp_rank_kernel(int L, int k, const TpState* __restrict__ st, const uint64_t* __restrict__ sel_key,
                                                      const uint32_t* __restrict__ sel_idx, int32_t* __restrict__ pairs,
                                                      double* __restrict__ scores, int32_t* __restrict__ count) {
    __shared__ uint64_t s_key[256];
    __shared__ uint32_t s_idx[256];
    const int t = threadIdx.x;
    const unsigned s = blockIdx.x * 256u + (unsigned)t, n = st->n;
    if (s == 0) *count = (int32_t)n;
    const bool mine = s < n;
    unsigned rank = 0;
    uint64_t ka = 0;
    uint32_t ia = 0;
    if (blockIdx.x * 256u < n) {                                           // (the same for the whole block)
        if (mine) { ka = sel_key[s]; ia = sel_idx[s]; }
        for (unsigned b0 = 0; b0 < n; b0 += 256u) {
            __syncthreads();
            // past n: key 0 is the key of no value (it would be a NaN's), so such an entry precedes nothing
            const bool in = b0 + (unsigned)t < n;
            s_key[t] = in ? sel_key[b0 + t] : 0ull;
            s_idx[t] = in ? sel_idx[b0 + t] : 0xffffffffu;
            __syncthreads();
#pragma unroll 8
            for (int q = 0; q < 256; ++q) {
                const uint64_t kb = s_key[q];
                const uint32_t ib = s_idx[q];
                rank += (kb > ka || (kb == ka && ib < ia)) ? 1u : 0u;
            }
        }
    }
    if (mine) {
        if (rank < (unsigned)k) {
            pairs[2 * (size_t)rank] = (int32_t)(ia / (uint32_t)L);
            pairs[2 * (size_t)rank + 1] = (int32_t)(ia % (uint32_t)L);
            scores[rank] = tp_value(ka);
        }
    } else if (s < (unsigned)k) {
        pairs[2 * (size_t)s] = -1;
        pairs[2 * (size_t)s + 1] = -1;
        scores[s] = __builtin_nan("");
    }
}

struct TpWs {
    size_t state, hist, sel_key, sel_idx, ties, total;      // offsets, each a multiple of 256
    int nseg;
};
static size_t tp_round(size_t n) { return (n + 255) & ~(size_t)255; }
static TpWs tp_ws(int L, int k) {
    TpWs w;
    w.nseg = (L + TP_SEG - 1) / TP_SEG;
    w.state = 0;
    w.hist = tp_round(sizeof(TpState));
    w.sel_key = w.hist + 256 * 8;
    w.sel_idx = w.sel_key + tp_round((size_t)k * 8);
    w.ties = w.sel_idx + tp_round((size_t)k * 4);
    w.total = w.ties + tp_round(((size_t)(L - 1) * w.nseg + 1) * 4);         // a slot per block at min_sep = 1, and the total
    return w;
}
static bool tp_shape_ok(int L, int k) { return L >= 2 && L <= TP_MAX_L && k >= 1 && k <= TP_MAX_K; }

template <class T>
static int tp_run(const char* name, const T* x, int L, int64_t ld, int min_sep, int k, int32_t* pairs, double* scores, int32_t* count,
                  void* workspace, size_t workspace_bytes, void* stream) {
    RNAMSM_CHECK_ARG(x && pairs && scores && count && workspace, "%s: null pointer", name);
    RNAMSM_CHECK_ARG(L >= 2 && L <= TP_MAX_L, "%s: L=%d outside [2, %d]", name, L, TP_MAX_L);
    RNAMSM_CHECK_ARG(k >= 1 && k <= TP_MAX_K, "%s: k=%d outside [1, %d]", name, k, TP_MAX_K);
    RNAMSM_CHECK_ARG(min_sep >= 1 && min_sep <= TP_MAX_SEP, "%s: min_sep=%d outside [1, %d]", name, min_sep, TP_MAX_SEP);
    RNAMSM_CHECK_ARG(ld >= L, "%s: ld=%lld is smaller than L=%d", name, (long long)ld, L);
    const TpWs w = tp_ws(L, k);
    RNAMSM_CHECK_ARG(workspace_bytes >= w.total, "%s: workspace of %zu bytes is smaller than the %zu that L=%d, k=%d need", name,
                     workspace_bytes, w.total, L, k);
    RNAMSM_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "%s: workspace misaligned (256 bytes)", name);
    RNAMSM_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & (sizeof(T) - 1)) == 0 && (reinterpret_cast<uintptr_t>(pairs) & 3u) == 0 &&
                         (reinterpret_cast<uintptr_t>(scores) & 7u) == 0 && (reinterpret_cast<uintptr_t>(count) & 3u) == 0,
                     "%s: x / pairs / scores / count misaligned", name);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    TpState* st = reinterpret_cast<TpState*>(ws + w.state);
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(ws + w.hist);
    uint64_t* sel_key = reinterpret_cast<uint64_t*>(ws + w.sel_key);
    uint32_t* sel_idx = reinterpret_cast<uint32_t*>(ws + w.sel_idx);
    uint32_t* ties = reinterpret_cast<uint32_t*>(ws + w.ties);
    const int rows = L - min_sep > 1 ? L - min_sep : 1;                    // rows from L - min_sep on hold no candidate
    const dim3 grid(w.nseg, rows), block(TP_THREADS);
    const int nb = w.nseg * rows;                                          // <= (L - 1) * nseg: the slots tp_ws counted

    hipLaunchKernelGGL(tp_init_kernel, dim3(1), dim3(256), 0, s, st, hist);
    for (int pass = 0; pass < 8; ++pass) {
        hipLaunchKernelGGL(tp_hist_kernel<T>, grid, block, 0, s, x, L, ld, min_sep, pass, st, hist);
        hipLaunchKernelGGL(tp_select_kernel, dim3(1), dim3(256), 0, s, pass, k, st, hist);
    }
    hipLaunchKernelGGL(tp_count_kernel<T>, grid, block, 0, s, x, L, ld, min_sep, k, st, sel_key, sel_idx, ties);
    hipLaunchKernelGGL(tp_scan_kernel, dim3(1), dim3(1024), 0, s, ties, nb);
    hipLaunchKernelGGL(tp_ties_kernel<T>, grid, block, 0, s, x, L, ld, min_sep, k, st, sel_key, sel_idx, ties);
    hipLaunchKernelGGL(tp_rank_kernel, dim3((k + 255) / 256), dim3(256), 0, s, L, k, st, sel_key, sel_idx, pairs, scores, count);
    RNAMSM_CHECK_LAUNCH(name);
    return RNAMSM_OK;
}

}  // namespace rnamsm

using namespace rnamsm;

extern "C" size_t rnamsm_top_pairs_workspace_bytes(int L, int k) {
    if (!tp_shape_ok(L, k)) return 0;
    return tp_ws(L, k).total;
}

extern "C" int rnamsm_top_pairs_f64(const double* x, int L, int64_t ld, int min_sep, int k, int32_t* pairs, double* scores,
                                    int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
    return tp_run<double>("top_pairs_f64", x, L, ld, min_sep, k, pairs, scores, count, workspace, workspace_bytes, stream);
}

extern "C" int rnamsm_top_pairs_f32(const float* x, int L, int64_t ld, int min_sep, int k, int32_t* pairs, double* scores,
                                    int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
    return tp_run<float>("top_pairs_f32", x, L, ld, min_sep, k, pairs, scores, count, workspace, workspace_bytes, stream);
}
