// Average-product correction of a square float64 map (the reference's apc, utils/tensor.py:103-113):
//   a1 = row sums, a2 = column sums, a12 = the total,   out[i, j] = x[i, j] - (a1[i] * a2[j]) / a12
// in that order: product, division, subtraction (compiled without contraction).  Any square map, symmetric or not.  With
// zero_diagonal the diagonal of x is read as 0 in the sums and in the subtraction, so out[i, i] = 0 - (a1[i] * a2[i]) / a12.  A total
// of 0 gives NaN everywhere, as the reference's 0 / 0 does.
//
// Every sum has one fixed order (no atomics, the same bits on every run):
//   a1[i]   thread t of 256 adds x[i, t], x[i, t + 256], ... ascending from 0.0; the 256 sums are folded in halves
//           (s[t] += s[t + 128], then + 64, ..., + 1)                                                     apc_rowcol_kernel, block i
//   a2[j]   a block owns 64 columns; part g of 4 adds x[g, j], x[g + 4, j], ... ascending from 0.0; a2[j] = (p0 + p2) + (p1 + p3)
//           (the same halving: p[g] += p[g + 2], then + 1)                                 apc_rowcol_kernel, block L + j / 64
//   a12     the row sums: thread t of 256 adds a1[t], a1[t + 256], ... ascending from 0.0, folded in halves     apc_total_kernel
#include "common.h"

namespace rnamsm {

constexpr int APC_MAX_L = 32768;

__device__ __forceinline__ double apc_fold256(double* s, int t) {
    for (int h = 128; h > 0; h >>= 1) {
        __syncthreads();
        if (t < h) s[t] += s[t + h];
    }
    __syncthreads();
    return s[0];
}

// blocks [0, L): the row sums; blocks [L, L + ceil(L / 64)): the column sums of 64 columns each
__global__ __launch_bounds__(256) void apc_rowcol_kernel(const double* __restrict__ x, int L, int64_t ld, int zero_diagonal,
                                                         double* __restrict__ a1, double* __restrict__ a2) {
    __shared__ double s[256];
    const int t = threadIdx.x;
    if ((int)blockIdx.x < L) {
        const int i = blockIdx.x;
        const double* row = x + (int64_t)i * ld;
        double acc = 0.0;
        for (int j = t; j < L; j += 256) acc += (zero_diagonal && j == i) ? 0.0 : row[j];
        s[t] = acc;
        const double total = apc_fold256(s, t);
        if (t == 0) a1[i] = total;
        return;
    }
    const int j = ((int)blockIdx.x - L) * 64 + (t & 63), g = t >> 6;
    double acc = 0.0;
    if (j < L)
        for (int i = g; i < L; i += 4) acc += (zero_diagonal && j == i) ? 0.0 : x[(int64_t)i * ld + j];
    s[t] = acc;
    __syncthreads();
    if (t < 128) s[t] += s[t + 128];
    __syncthreads();
    if (t < 64 && j < L) a2[j] = s[t] + s[t + 64];
}

__global__ __launch_bounds__(256) void apc_total_kernel(const double* __restrict__ a1, int L, double* __restrict__ a12) {
    __shared__ double s[256];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int i = t; i < L; i += 256) acc += a1[i];
    s[t] = acc;
    const double total = apc_fold256(s, t);
    if (t == 0) *a12 = total;
}

// out may be x itself where ld == L: an element is read and written by one thread, after the sums are complete
__global__ __launch_bounds__(256) void apc_apply_kernel(const double* x, int L, int64_t ld, int zero_diagonal,
                                                        const double* __restrict__ a1, const double* __restrict__ a2,
                                                        const double* __restrict__ a12, double* out) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= L) return;
    const double v = (zero_diagonal && j == i) ? 0.0 : x[(int64_t)i * ld + j];
    const double prod = a1[i] * a2[j];
    const double avg = prod / *a12;
    out[(int64_t)i * L + j] = v - avg;
}

}  // namespace rnamsm

using namespace rnamsm;

extern "C" size_t rnamsm_apc_f64_workspace_bytes(int L) {
    if (L < 1 || L > APC_MAX_L) return 0;
    return (((size_t)2 * L + 1) * 8 + 255) & ~(size_t)255;
}

extern "C" int rnamsm_apc_f64(const double* x, int L, int64_t ld, int zero_diagonal, double* out, void* workspace,
                              size_t workspace_bytes, void* stream) {
    RNAMSM_CHECK_ARG(x && out && workspace, "apc_f64: null pointer");
    RNAMSM_CHECK_ARG(L >= 1 && L <= APC_MAX_L, "apc_f64: L=%d outside [1, %d]", L, APC_MAX_L);
    RNAMSM_CHECK_ARG(ld >= L, "apc_f64: ld=%lld is smaller than L=%d", (long long)ld, L);
    RNAMSM_CHECK_ARG(zero_diagonal == 0 || zero_diagonal == 1, "apc_f64: zero_diagonal=%d is not 0 or 1", zero_diagonal);
    RNAMSM_CHECK_ARG(workspace_bytes >= rnamsm_apc_f64_workspace_bytes(L),
                     "apc_f64: workspace of %zu bytes is smaller than the %zu that L=%d needs", workspace_bytes,
                     rnamsm_apc_f64_workspace_bytes(L), L);
    RNAMSM_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(workspace)) & 7u) == 0,
                     "apc_f64: x / out / workspace misaligned (8 bytes)");
    RNAMSM_CHECK_ARG(out != x || ld == L, "apc_f64: out == x needs ld == L (ld=%lld, L=%d)", (long long)ld, L);
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* a1 = static_cast<double*>(workspace);
    double *a2 = a1 + L, *a12 = a2 + L;
    hipLaunchKernelGGL(apc_rowcol_kernel, dim3(L + (L + 63) / 64), dim3(256), 0, s, x, L, ld, zero_diagonal, a1, a2);
    hipLaunchKernelGGL(apc_total_kernel, dim3(1), dim3(256), 0, s, a1, L, a12);
    hipLaunchKernelGGL(apc_apply_kernel, dim3((L + 255) / 256, L), dim3(256), 0, s, x, L, ld, zero_diagonal, a1, a2, a12, out);
    RNAMSM_CHECK_LAUNCH("apc_f64");
    return RNAMSM_OK;
}
