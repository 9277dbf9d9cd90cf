// Jobs of ONE block that several files need (device code): three for a block of 1024 threads, and the wave-shuffle prefix sum of
// the text writers (struct_text.h, rsa_text.hip) for a block of any whole number of waves.
#pragma once
#include <type_traits>

#include "common.h"

namespace rnamsm {

// The sum of v over the threads below the calling one; total: the sum over the whole block, the same in every thread.  V: uint32_t
// or uint64_t (unsigned: several fields may share the word as long as no field's sum overflows into the next).  The block is
// blockDim.x threads, a multiple of 64 and at most 1024; wave_sums: blockDim.x / 64 words of LDS.  One barrier inside, between the
// write and the reads of wave_sums: the caller may write those words again only behind its own next barrier.
template <class V>
__device__ __forceinline__ V block_exclusive_sum(V v, V* wave_sums, V& total) {
    static_assert(sizeof(V) == 4 || sizeof(V) == 8, "a 32-bit or a 64-bit word");
    using Shfl = typename std::conditional<sizeof(V) == 8, unsigned long long, unsigned int>::type;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    V incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const V up = (V)__shfl_up((Shfl)incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    V before = 0;
    total = 0;
    for (int w = 0; w < nw; ++w) {
        const V s = wave_sums[w];
        if (w < wave) before += s;
        total += s;
    }
    return before + incl - v;
}

// the lowest n in [0, N) with pred(n), or -1 when there is none; the same value in every thread.  The caller's block is 1024 threads.
template <class Pred>
__device__ __forceinline__ int block_first_index(int N, Pred pred) {
    __shared__ int first[1024];
    int mine = INT32_MAX;
    for (int n = threadIdx.x; n < N; n += 1024)
        if (pred(n) && n < mine) mine = n;
    first[threadIdx.x] = mine;
    __syncthreads();
    for (int h = 512; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h && first[threadIdx.x + h] < first[threadIdx.x]) first[threadIdx.x] = first[threadIdx.x + h];
        __syncthreads();
    }
    return first[0] == INT32_MAX ? -1 : first[0];
}

// the inclusive sums of one value per thread over the block's 1024 threads (thread t gets v[0] + ... + v[t]); s: 1024 values of LDS
// that are free again when the call returns
template <class V>
__device__ __forceinline__ V block_inclusive_sum(V v, V* s) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const V w = t >= off ? s[t - off] : (V)0;
        __syncthreads();
        s[t] += w;
        __syncthreads();
    }
    const V r = s[t];
    __syncthreads();
    return r;
}

// single block: flags -> the ascending list of the indices whose flag is set, 1024 at a time by an inclusive scan
template <class Flag>
__global__ __launch_bounds__(1024) void compact_flags_kernel(const Flag* __restrict__ flags, int N, int32_t* __restrict__ out) {
    __shared__ int base;
    __shared__ int cnt[1024];
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int start = 0; start < N; start += 1024) {
        const int n = start + threadIdx.x;
        const int f = (n < N && flags[n]) ? 1 : 0;
        cnt[threadIdx.x] = f;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {                        // inclusive scan
            const int v = (int)threadIdx.x >= off ? cnt[threadIdx.x - off] : 0;
            __syncthreads();
            cnt[threadIdx.x] += v;
            __syncthreads();
        }
        if (f) out[base + cnt[threadIdx.x] - 1] = n;
        __syncthreads();
        if (threadIdx.x == 1023) base += cnt[1023];
        __syncthreads();
    }
}

}  // namespace rnamsm
