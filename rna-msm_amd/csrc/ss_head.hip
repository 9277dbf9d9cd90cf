// RNA-MSM-SS: the secondary-structure head on the attention maps (_downstream_tasks/SS/code/model.py, ResNet._forward_impl
// :223-233 with BasicBlock.forward :67-85; renet_b16 = 16 blocks; input built by pre_processing/data_processing.py):
//   x0      = conv1(in) + b                       3x3, 128 -> 48 channels; in[c, i, j] = onehot(seq[i])[c] (c < 4),
//                                                 onehot(seq[j])[c - 4] (c < 8), atp[c - 8, i, j] (c < 128)
//   x_{k+1} = x_k + conv5x5(relu(LN2(conv3x3(relu(LN1(x_k))))))     48 -> 48, no bias, zero padding of the conv INPUTS
//   logits  = fc1(relu(LN(x_16))),  probs = sigmoid(logits)           [L, L]
// Every convolution is an implicit GEMM on the exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32): one 512-thread block per
// 16 x 16 output pixels (M = 256), N = 48 = 3 MFMA columns, K = taps x input channels.  The block's input window (tile +
// halo) is staged in LDS once, NHWC with a 52-float pixel stride; the LayerNorm + ReLU of the consuming conv is applied
// while staging (per pixel, over its 48 staged channels) and out-of-image pixels are written as zeros AFTER it, as
// nn.Conv2d pads relu(LN(x)).  Wave w owns output rows 2w, 2w+1 of the tile: 2 x 3 accumulators of 16 x 16.
// One ds_read_b128 gives a lane the four k-steps {16q + 4g + j, j = 0..3} of its lane group g = lane >> 4 (A: the
// pixel's channels, B: the weight row's input channels, permuted identically) -- a fixed order, so results are the same
// bits run to run; nothing is reduced across threads, no atomics.  The weights of the next tap are loaded into
// registers while the current tap's 72 MFMAs run (straight from L2: 9 KB per tap, read by every block).
// Activations live in the caller's workspace as two NHWC [L*L][48] fp32 images: the residual stream x and the block's
// middle t.  The 5x5 conv adds x in its epilogue and writes x in place (each output element is read and then written
// by the one lane that owns it).
#include "ss_head_common.h"

namespace rnamsm {
namespace {

constexpr int SS_THREADS = 512;                // 8 waves, 2 output rows each
constexpr int SS_LDC = SS_CH + 4;              // LDS pixel stride (floats) of the trunk's staged window
constexpr int SS_STEM_CK = 32;                 // stem: input channels per staged chunk (4 chunks of the 128)
constexpr int SS_STEM_LDC = SS_STEM_CK + 4;
constexpr int SS_STEM_SW = SS_TILE + 2;

constexpr size_t ss_trunk_lds_bytes(int ks) {
    return (size_t)(SS_TILE + ks - 1) * (SS_TILE + ks - 1) * SS_LDC * sizeof(float);
}
constexpr size_t SS_STEM_LDS_BYTES = (size_t)SS_STEM_SW * SS_STEM_SW * SS_STEM_LDC * sizeof(float);

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// B fragments of one tap: b[q][nt] = W[n = 16 nt + r][c0 + 16 q + 4 g .. +3] of a [48][cin] weight slab
template <int NQ>
__device__ __forceinline__ void load_b(const float* __restrict__ wt, int cin, int c0, f32x4 (&b)[NQ][3]) {
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int nt = 0; nt < 3; ++nt)
            b[q][nt] = *reinterpret_cast<const f32x4*>(wt + (size_t)(16 * nt + r) * cin + c0 + 16 * q + 4 * g);
}

// acc[mt][nt] += window pixel (row 2w + mt + dy, col r + dx), channels [0, 16 NQ) . b
template <int NQ>
__device__ __forceinline__ void tap_mma(const float* S, int sw, int ldc, int dy, int dx, const f32x4 (&b)[NQ][3],
                                        f32x4 (&acc)[2][3]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        f32x4 a[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
            a[mt] = *reinterpret_cast<const f32x4*>(S + ((2 * w + mt + dy) * sw + r + dx) * ldc + 16 * q + 4 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 3; ++nt) acc[mt][nt] = mfma16(a[mt][j], b[q][nt][j], acc[mt][nt]);
    }
}

// The taps of one staged window: weights [taps][48][cin], this window holds input channels [c0, c0 + 16 NQ).
template <int KS, int NQ>
__device__ __forceinline__ void window_mma(const float* S, int sw, int ldc, const float* __restrict__ w, int cin, int c0,
                                           f32x4 (&acc)[2][3]) {
    f32x4 b[NQ][3], bn[NQ][3];
    load_b<NQ>(w, cin, c0, b);
#pragma unroll 1
    for (int tap = 0; tap < KS * KS; ++tap) {
        if (tap + 1 < KS * KS) load_b<NQ>(w + (size_t)(tap + 1) * SS_CH * cin, cin, c0, bn);
        tap_mma<NQ>(S, sw, ldc, tap / KS, tap % KS, b, acc);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int nt = 0; nt < 3; ++nt) b[q][nt] = bn[q][nt];
    }
}

__device__ __forceinline__ void zero_acc16(f32x4 (&acc)[2][3]) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 3; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// Epilogue: lane (r, g) holds D[pixel col 4g + t][channel 16 nt + r] of output row 2w + mt.
// bias: per-channel bias (stem) or null; RESIDUAL: out += (in place: out is the residual stream).
template <bool RESIDUAL>
__device__ __forceinline__ void store_tile(const f32x4 (&acc)[2][3], const float* __restrict__ bias, float* out, int y0,
                                           int x0, int L) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int oy = y0 + 2 * w + mt;
        if (oy >= L) continue;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int ox = x0 + 4 * g + t;
            if (ox >= L) continue;
            float* o = out + ((size_t)oy * L + ox) * SS_CH + r;
#pragma unroll
            for (int nt = 0; nt < 3; ++nt) {
                float v = acc[mt][nt][t];
                if (bias) v += bias[16 * nt + r];
                if (RESIDUAL) v = v + o[16 * nt];
                o[16 * nt] = v;
            }
        }
    }
}

// Stem: 3x3, 128 -> 48 with bias.  The input planes are built while staging: one-hot channels from the base codes
// (0..3 = A, C, G, U; any other value = the all-zero vector of OneHotEncoder(handle_unknown='ignore')), the 120 maps read
// in place from atp (plane c - 8 at c_plane_stride * (c - 8), rows of L floats).  Four chunks of 32 channels.
__device__ __forceinline__ void ss_stem_body(float* S, const float* __restrict__ atp, int64_t plane_stride,
                                             const uint8_t* __restrict__ codes, const float* __restrict__ w,
                                             const float* __restrict__ bias, float* __restrict__ out, int L, int y0, int x0) {
    constexpr int NPIX = SS_STEM_SW * SS_STEM_SW;
    f32x4 acc[2][3];
    zero_acc16(acc);
#pragma unroll 1
    for (int chunk = 0; chunk < 128 / SS_STEM_CK; ++chunk) {
        if (chunk) __syncthreads();                       // every wave is done with the previous chunk's window
        for (int e = threadIdx.x; e < SS_STEM_CK * NPIX; e += SS_THREADS) {
            const int c = e / NPIX, p = e - c * NPIX;
            const int sy = p / SS_STEM_SW, sx = p - sy * SS_STEM_SW;
            const int iy = y0 - 1 + sy, ix = x0 - 1 + sx, ch = chunk * SS_STEM_CK + c;
            float v = 0.f;
            if (iy >= 0 && iy < L && ix >= 0 && ix < L) {
                if (ch < 4) v = codes[iy] == ch ? 1.f : 0.f;
                else if (ch < 8) v = codes[ix] == ch - 4 ? 1.f : 0.f;
                else v = atp[(int64_t)(ch - 8) * plane_stride + (int64_t)iy * L + ix];
            }
            S[p * SS_STEM_LDC + c] = v;
        }
        __syncthreads();
        window_mma<3, SS_STEM_CK / 16>(S, SS_STEM_SW, SS_STEM_LDC, w, 128, chunk * SS_STEM_CK, acc);
    }
    store_tile<false>(acc, bias, out, y0, x0, L);
}
template <bool PACKED>
__global__ __launch_bounds__(SS_THREADS) void ss_stem_kernel(const SsMember* __restrict__ mem, int B, const SsMember lone,
                                                             const float* __restrict__ w, const float* __restrict__ bias,
                                                             float* __restrict__ out) {
    extern __shared__ f32x4 ss_smem[];
    const SsMember m = ss_member<PACKED>(mem, B, lone, (int)blockIdx.x, &SsMember::tile0);
    const int t = (int)blockIdx.x - m.tile0, ty = t / m.tiles, tx = t - ty * m.tiles;
    ss_stem_body(reinterpret_cast<float*>(ss_smem), m.atp, m.plane_stride, m.codes, w, bias, out + (size_t)m.pix0 * SS_CH, m.L,
                 ty * SS_TILE, tx * SS_TILE);
}

// Trunk conv: out (+)= conv_KS(relu(LN(x))), 48 -> 48, no bias.  RESIDUAL: out is the residual stream, updated in place.
// The bounds tests are those of the IMAGE (iy < L), never of the buffer it lies in: in a packed batch the rows before and after
// an image are its neighbours' pixels, and a halo read there must give the zero padding all the same.
template <int KS, bool RESIDUAL>
__device__ __forceinline__ void ss_conv_body(float* S, const float* __restrict__ x, const float* __restrict__ gamma,
                                             const float* __restrict__ beta, const float* __restrict__ w, float* out, int L,
                                             int y0, int x0) {
    constexpr int P = KS / 2, SW = SS_TILE + 2 * P;
    for (int p = threadIdx.x; p < SW * SW; p += SS_THREADS) {
        const int sy = p / SW, sx = p - sy * SW, iy = y0 - P + sy, ix = x0 - P + sx;
        f32x4* dst = reinterpret_cast<f32x4*>(S + p * SS_LDC);
        if (iy >= 0 && iy < L && ix >= 0 && ix < L) {
            const f32x4* src = reinterpret_cast<const f32x4*>(x + ((size_t)iy * L + ix) * SS_CH);
            f32x4 v[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) v[i] = src[i];
            ln_relu48(v, gamma, beta);
#pragma unroll
            for (int i = 0; i < 12; ++i) dst[i] = v[i];
        } else {                                          // zero padding of the conv input relu(LN(x)), not relu(LN(0))
#pragma unroll
            for (int i = 0; i < 12; ++i) dst[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    __syncthreads();
    f32x4 acc[2][3];
    zero_acc16(acc);
    window_mma<KS, 3>(S, SW, SS_LDC, w, SS_CH, 0, acc);
    store_tile<RESIDUAL>(acc, nullptr, out, y0, x0, L);
}
template <int KS, bool RESIDUAL, bool PACKED>
__global__ __launch_bounds__(SS_THREADS) void ss_conv_kernel(const SsMember* __restrict__ mem, int B, const SsMember lone,
                                                             const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ w,
                                                             float* out) {
    extern __shared__ f32x4 ss_smem[];
    const SsMember m = ss_member<PACKED>(mem, B, lone, (int)blockIdx.x, &SsMember::tile0);
    const int t = (int)blockIdx.x - m.tile0, ty = t / m.tiles, tx = t - ty * m.tiles;
    const size_t off = (size_t)m.pix0 * SS_CH;
    ss_conv_body<KS, RESIDUAL>(reinterpret_cast<float*>(ss_smem), x + off, gamma, beta, w, out + off, m.L, ty * SS_TILE,
                               tx * SS_TILE);
}

// The launches over `blocks` tiles and `pixels` pixels (xs, ts: the two [pixels][48] images): PACKED with mem / B the uploaded table
// of a batch, else null / 1 and the lone member.  weights: checked by the caller; conv1.weight, conv1.bias, bn1.weight, bn1.bias,
// then per block conv1.weight, bn1.weight, bn1.bias, conv2.weight, bn2.weight, bn2.bias, then fc1.weight, fc1.bias (include/rnamsm.h)
template <bool PACKED>
int ss_launch(const SsMember* mem, int B, const SsMember& lone, int64_t blocks, int64_t pixels, int num_blocks,
              const float* const* weights, float* xs, hipStream_t s) {
    float* ts = xs + (size_t)pixels * SS_CH;
    const dim3 grid((unsigned)blocks);           // the members' own tiles, nothing for a small member beside a large one
    hipLaunchKernelGGL(ss_stem_kernel<PACKED>, grid, dim3(SS_THREADS), SS_STEM_LDS_BYTES, s, mem, B, lone, weights[0], weights[1], xs);
    RNAMSM_CHECK_LAUNCH(PACKED ? "ss_stem (packed)" : "ss_stem");
    for (int k = 0; k < num_blocks; ++k) {
        const float* const* bw = weights + 4 + RNAMSM_SS_WEIGHTS_PER_BLOCK * k;
        hipLaunchKernelGGL((ss_conv_kernel<3, false, PACKED>), grid, dim3(SS_THREADS), ss_trunk_lds_bytes(3), s, mem, B, lone, xs, bw[1], bw[2],
                           bw[0], ts);
        RNAMSM_CHECK_LAUNCH(PACKED ? "ss_conv3x3 (packed)" : "ss_conv3x3");
        hipLaunchKernelGGL((ss_conv_kernel<5, true, PACKED>), grid, dim3(SS_THREADS), ss_trunk_lds_bytes(5), s, mem, B, lone, ts, bw[4], bw[5],
                           bw[3], xs);
        RNAMSM_CHECK_LAUNCH(PACKED ? "ss_conv5x5 (packed)" : "ss_conv5x5");
    }
    const float* const* hw = weights + 4 + RNAMSM_SS_WEIGHTS_PER_BLOCK * num_blocks;
    hipLaunchKernelGGL(ss_out_kernel<PACKED>, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, mem, B, lone, xs, weights[2], weights[3],
                       hw[0], hw[1], pixels);
    RNAMSM_CHECK_LAUNCH(PACKED ? "ss_out (packed)" : "ss_out");
    return RNAMSM_OK;
}

// the last step before anything is enqueued: the weight table, then the dynamic LDS of the kernels ss_launch<PACKED> runs, once per device
template <bool PACKED>
int ss_check_weights_and_lds(const char* prefix, const float* const* weights, int num_blocks) {
    static DeviceOnce once_stem, once3, once5;
    int rc = check_weight_table(prefix, weights, RNAMSM_SS_GLOBAL_WEIGHTS + RNAMSM_SS_WEIGHTS_PER_BLOCK * num_blocks);
    if (rc == RNAMSM_OK) rc = allow_lds(ss_stem_kernel<PACKED>, SS_STEM_LDS_BYTES, once_stem);
    if (rc == RNAMSM_OK) rc = allow_lds(ss_conv_kernel<3, false, PACKED>, ss_trunk_lds_bytes(3), once3);
    if (rc == RNAMSM_OK) rc = allow_lds(ss_conv_kernel<5, true, PACKED>, ss_trunk_lds_bytes(5), once5);
    return rc;
}

}  // namespace
}  // namespace rnamsm

using namespace rnamsm;

// The lone call under either limit: rnamsm_ss_head (RNAMSM_SS_MAX_L) and rnamsm_ss_head_long (RNAMSM_LONG_MAX_L) run the same
// kernels on the same descriptor, so the same bits where both run.  Beyond 1024: the grid is ceil(L / 16)^2 <= 2^16 blocks; a pixel's
// index y * L + x < 2^24 is widened before it is scaled by 48 (store_tile, ss_conv_body, ss_out_kernel) and the stem reads plane
// p * plane_stride + y * L + x in int64_t -- 120 planes of 2^24 floats are 8 GB.
static size_t ss_head_bytes(int L, int max_L) {
    if (L < 1 || L > max_L) return 0;
    return 2 * (size_t)L * L * SS_CH * sizeof(float);
}
static int ss_head_lone(const char* who, int max_L, const float* atp, int64_t atp_plane_stride, const uint8_t* base_codes, int L,
                        int num_blocks, const float* const* weights, float* logits, float* probs, void* workspace,
                        size_t workspace_bytes, void* stream) {
    RNAMSM_CHECK_ARG(atp && base_codes && weights && workspace, "%s: null pointer", who);
    RNAMSM_CHECK_ARG(logits || probs, "%s: neither logits nor probs given", who);
    RNAMSM_CHECK_ARG(L >= 1 && L <= max_L, "%s: L=%d outside [1, %d]", who, L, max_L);
    RNAMSM_CHECK_ARG(num_blocks >= 1 && num_blocks <= RNAMSM_SS_MAX_BLOCKS, "%s: num_blocks=%d outside [1, %d]", who, num_blocks,
                     RNAMSM_SS_MAX_BLOCKS);
    RNAMSM_CHECK_ARG(atp_plane_stride >= (int64_t)L * L, "%s: atp plane stride %lld < L*L", who, (long long)atp_plane_stride);
    RNAMSM_CHECK_ARG(workspace_bytes >= ss_head_bytes(L, max_L), "%s: workspace too small", who);
    RNAMSM_CHECK_ARG(aligned16(workspace), "%s: 16-byte alignment of the workspace", who);
    if (int rc = ss_check_weights_and_lds<false>(who, weights, num_blocks)) return rc;
    const int tiles = (L + SS_TILE - 1) / SS_TILE;
    const SsMember lone = {atp, atp_plane_stride, base_codes, logits, probs, 0, L, tiles, 0, 0};
    return ss_launch<false>(nullptr, 1, lone, (int64_t)tiles * tiles, (int64_t)L * L, num_blocks, weights, static_cast<float*>(workspace),
                            static_cast<hipStream_t>(stream));
}

extern "C" size_t rnamsm_ss_head_workspace_bytes(int L) { return ss_head_bytes(L, RNAMSM_SS_MAX_L); }

extern "C" int rnamsm_ss_head(const float* atp, int64_t atp_plane_stride, const uint8_t* base_codes, int L, int num_blocks,
                              const float* const* weights, float* logits, float* probs, void* workspace, size_t workspace_bytes,
                              void* stream) {
    return ss_head_lone("ss_head", RNAMSM_SS_MAX_L, atp, atp_plane_stride, base_codes, L, num_blocks, weights, logits, probs, workspace,
                        workspace_bytes, stream);
}

extern "C" size_t rnamsm_ss_head_long_workspace_bytes(int L) { return ss_head_bytes(L, RNAMSM_LONG_MAX_L); }

extern "C" int rnamsm_ss_head_long(const float* atp, int64_t atp_plane_stride, const uint8_t* base_codes, int L, int num_blocks,
                                   const float* const* weights, float* logits, float* probs, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    return ss_head_lone("ss_head_long", RNAMSM_LONG_MAX_L, atp, atp_plane_stride, base_codes, L, num_blocks, weights, logits, probs,
                        workspace, workspace_bytes, stream);
}

extern "C" size_t rnamsm_ss_head_packed_workspace_bytes(int B, const int* Ls) {
    if (B < 1 || B > RNAMSM_SS_MAX_BATCH || !Ls) return 0;
    size_t pixels = 0;
    for (int b = 0; b < B; ++b) {
        if (Ls[b] < 1 || Ls[b] > RNAMSM_SS_MAX_L) return 0;
        pixels += (size_t)Ls[b] * Ls[b];
    }
    return ss_members_bytes(B) + 2 * pixels * SS_CH * sizeof(float);
}

extern "C" int rnamsm_ss_head_packed(const rnamsm_ss_item* items, int B, int num_blocks, const float* const* weights, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    // every refusal comes before the first launch: a refused call leaves the stream and the outputs untouched
    RNAMSM_CHECK_ARG(items && weights && workspace, "ss_head_packed: null pointer");
    RNAMSM_CHECK_ARG(B >= 1 && B <= RNAMSM_SS_MAX_BATCH, "ss_head_packed: B=%d outside [1, %d]", B, RNAMSM_SS_MAX_BATCH);
    RNAMSM_CHECK_ARG(num_blocks >= 1 && num_blocks <= RNAMSM_SS_MAX_BLOCKS, "ss_head_packed: num_blocks=%d outside [1, %d]", num_blocks,
                     RNAMSM_SS_MAX_BLOCKS);
    int64_t pixels = 0, tiles_total = 0;
    for (int b = 0; b < B; ++b) {
        const rnamsm_ss_item& it = items[b];
        RNAMSM_CHECK_ARG(it.L >= 1 && it.L <= RNAMSM_SS_MAX_L, "ss_head_packed: member %d: L=%d outside [1, %d]", b, it.L, RNAMSM_SS_MAX_L);
        RNAMSM_CHECK_ARG(it.atp && it.base_codes, "ss_head_packed: member %d: null pointer", b);
        RNAMSM_CHECK_ARG(it.logits || it.probs, "ss_head_packed: member %d: neither logits nor probs given", b);
        RNAMSM_CHECK_ARG(((uintptr_t)it.atp & 3u) == 0 && ((uintptr_t)it.logits & 3u) == 0 && ((uintptr_t)it.probs & 3u) == 0,
                         "ss_head_packed: member %d: a float pointer is not 4-byte aligned", b);
        RNAMSM_CHECK_ARG(it.atp_plane_stride >= (int64_t)it.L * it.L, "ss_head_packed: member %d: atp plane stride %lld < L*L", b,
                         (long long)it.atp_plane_stride);
        const int64_t t = (it.L + SS_TILE - 1) / SS_TILE;
        pixels += (int64_t)it.L * it.L;
        tiles_total += t * t;
    }
    RNAMSM_CHECK_ARG(aligned16(workspace), "ss_head_packed: 16-byte alignment of the workspace");
    RNAMSM_CHECK_ARG(workspace_bytes >= ss_members_bytes(B) + 2 * (size_t)pixels * SS_CH * sizeof(float),
                     "ss_head_packed: workspace too small");
    if (int rc = ss_check_weights_and_lds<true>("ss_head_packed", weights, num_blocks)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SsMember* mem = static_cast<SsMember*>(workspace);
    int64_t pix0 = 0;
    int32_t tile0 = 0;
    const int rc = upload_members(mem, B, [&](int b) {
        const rnamsm_ss_item& it = items[b];
        const int32_t tiles = (it.L + SS_TILE - 1) / SS_TILE;
        const SsMember m = {it.atp, it.atp_plane_stride, it.base_codes, it.logits, it.probs, pix0, it.L, tiles, tile0, 0};
        pix0 += (int64_t)it.L * it.L;
        tile0 += tiles * tiles;
        return m;
    }, s, "ss_members");
    if (rc != RNAMSM_OK) return rc;
    return ss_launch<true>(mem, B, SsMember{}, tiles_total, pixels, num_blocks, weights,
                           reinterpret_cast<float*>(static_cast<char*>(workspace) + ss_members_bytes(B)), s);
}
