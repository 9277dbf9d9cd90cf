// What the fp32 SS head (ss_head.hip) and the bf16 one (ss_head16.hip) share: the member descriptors of a packed call, the
// LayerNorm + ReLU of one pixel and the output pass (final LN + ReLU + fc1 + sigmoid), all fp32 in both arithmetics.
#pragma once
#include "common.h"

namespace rnamsm {
namespace {

constexpr int SS_CH = 48;                      // trunk channels
constexpr int SS_TILE = 16;                    // output tile: 16 x 16 pixels
constexpr float SS_LN_EPS = 1e-5f;             // nn.LayerNorm default

// relu(LayerNorm(v)) of one pixel's 48 channels, in place (biased variance, two passes)
__device__ __forceinline__ void ln_relu48(f32x4 (&v)[12], const float* __restrict__ gamma, const float* __restrict__ beta) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    const float mean = s * (1.f / SS_CH);
    float s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = v[i][k] - mean;
            s2 = fmaf(d, d, s2);
        }
    const float rstd = 1.f / sqrtf(s2 * (1.f / SS_CH) + SS_LN_EPS);
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + 4 * i), bt = *reinterpret_cast<const f32x4*>(beta + 4 * i);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[i][k] = relu_nan(fmaf((v[i][k] - mean) * rstd, gm[k], bt[k]));
    }
}

// ---- the member of a block ------------------------------------------------------------------------------------------------------
// One kernel per stage serves the lone call (rnamsm_ss_head) and the batched one (rnamsm_ss_head_packed).  The images of a batch lie
// back to back in the two workspace images (member b's first pixel is pixel pix0 of the buffer), and a launch has the SUM of the
// members' tiles as a flat grid.  Batched, mem is the device table of the B members and a block finds its own by a search over the
// tile prefix sums (common.h: member_of); lone, mem is null and the one member is the kernel argument itself (tile0 = 0, pix0 = 0:
// the caller's workspace with no table in front).  Either way the stage's body runs on the member's own (image, L, tile): one
// arithmetic, so a structure's bits depend on nothing else.
// The choice is a template argument, not a test of mem: one definition, two code objects.  With the test inside the kernel the
// compiler reads the descriptor through ONE flat load of a selected address (table or kernel argument) and L, the offsets and the
// pointers land in vector registers: +5 to +14 VGPRs over the lone kernels in every stage.
struct SsMember {            // 64 bytes
    const float* atp;
    int64_t plane_stride;
    const uint8_t* codes;
    float* logits;
    float* probs;
    int64_t pix0;            // pixels of the members before it
    int32_t L, tiles;        // tiles = ceil(L / 16): its launches' share is tiles x tiles blocks, row by row
    int32_t tile0;           // blocks of the members before it
    int32_t pad_;
};
static_assert(sizeof(SsMember) == 64, "SsMember layout");
template <bool PACKED, class K, class F>
__device__ __forceinline__ SsMember ss_member(const SsMember* __restrict__ mem, int B, const SsMember& lone, K key, F SsMember::*field) {
    if (PACKED) return mem[member_of(mem, B, key, field)];
    return lone;
}

// Head: logits = fc1(relu(LN(x))) (fc1: Linear(48, 1)), probs = sigmoid(logits); one thread per pixel.
// pixel: the 48 channels of the pixel; i: its index inside its own [L, L] outputs
__device__ __forceinline__ void ss_out_body(const float* __restrict__ pixel, const float* __restrict__ gamma,
                                            const float* __restrict__ beta, const float* __restrict__ fw,
                                            const float* __restrict__ fb, float* __restrict__ logits, float* __restrict__ probs,
                                            int64_t i) {
    const f32x4* src = reinterpret_cast<const f32x4*>(pixel);
    f32x4 v[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = src[k];
    ln_relu48(v, gamma, beta);
    float z = 0.f;
#pragma unroll
    for (int k = 0; k < 12; ++k)
#pragma unroll
        for (int t = 0; t < 4; ++t) z = fmaf(v[k][t], fw[4 * k + t], z);
    z += fb[0];
    if (logits) logits[i] = z;
    if (probs) probs[i] = 1.f / (1.f + expf(-z));
}
// n pixels of the whole buffer; a thread finds its pixel's member by the pixel prefix sums
template <bool PACKED>
__global__ __launch_bounds__(256) void ss_out_kernel(const SsMember* __restrict__ mem, int B, const SsMember lone,
                                                     const float* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const float* __restrict__ fw,
                                                     const float* __restrict__ fb, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const SsMember m = ss_member<PACKED>(mem, B, lone, i, &SsMember::pix0);
    ss_out_body(x + i * SS_CH, gamma, beta, fw, fb, m.logits, m.probs, i - m.pix0);
}

constexpr size_t ss_members_bytes(int B) { return ((size_t)B * sizeof(SsMember) + 255) & ~(size_t)255; }

template <class K>
int allow_lds(K kernel, size_t bytes, DeviceOnce& once) {
    if (once.pending()) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return fail(RNAMSM_ERR_HIP, "ss_head: hipFuncSetAttribute: %s", hipGetErrorString(e));
        once.mark();
    }
    return RNAMSM_OK;
}

}  // namespace
}  // namespace rnamsm
