// RNA-MSM-SS head, bf16 matrix-core mode (rnamsm_ss_head16, rnamsm_ss_head16_packed): the network of ss_head.hip with the
// convolutions on v_mfma_f32_16x16x32_bf16.  The arithmetic contract (include/rnamsm.h):
//   bf16, rounded to nearest even (NaN stays NaN, +-inf stays +-inf): the stem's inputs (the 120 maps, the 8 one-hot planes), each
//   block's relu(LN(x)) activations, every conv weight;  fp32: the MFMA accumulation, the residual image x, the middle image t,
//   the LayerNorm statistics and affine, the stem bias, the output pass (ss_head_common.h: the fp32 head's own functions).
// Structure as in ss_head.hip: one implicit GEMM per conv, a block per 16 x 16 output pixels, the input window (tile + halo) staged
// once in LDS, NHWC, with the consumer's LN + ReLU applied while staging and the out-of-image pixels written as zeros after it.
// What differs:
//   K is FLAT over (tap, channel): an MFMA step sums 32 k = four chunks of 8 channels, one per lane group g = lane >> 4 (lane l
//   holds A[row l & 15][k = 8 g + j] and B[k = 8 g + j][col l & 15], j = 0..7: one 16-byte read each).  Chunk q of a window with
//   CW channels is tap q / (CW / 8), channels 8 (q % (CW / 8)) .. +7, so the four lane groups of a step may read four different
//   taps' pixels.  Trunk (CW = 48): 54 chunks = 13.5 steps for the 3x3, 150 = 37.5 for the 5x5; the two missing chunks of the last
//   step are zeros in A AND B (0 x NaN would be NaN).  Stem (two windows of CW = 64): 72 chunks = 18 whole steps each.  Nothing is
//   padded: the matrix cores do 432 / 1200 of 448 / 1216 k per pixel.
//   A block is 256 threads, wave w owns output rows 4w .. 4w+3 of the tile (4 x 3 accumulators): a B fragment, which comes
//   straight from L2 (the bf16 planes of one conv are 41 / 115 KB), feeds four MFMAs instead of two.
//   LDS pixel stride 56 bf16 = 112 B (stem: 72 = 144 B): the 16 lanes of a group read 16 bytes each from 16 consecutive pixels,
//   28 (36) dwords apart -- all 64 banks once.  The windows are 36 KB (3x3), 45 KB (5x5) and 47 KB (stem): under 64 KB.
// The summation order of a pixel is the step order, the same for every pixel, tile and member: no atomics, the same bits run to
// run, and a member of a packed call has the bits of the lone call.
#include "ss_head_common.h"

namespace rnamsm {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int S16_THREADS = 256;               // 4 waves
constexpr int S16_MT = 4;                      // output rows of the tile per wave
constexpr int S16_LDC = SS_CH + 8;             // LDS pixel stride (bf16) of the trunk's staged window
constexpr int S16_STEM_CW = 64;                // stem: input channels per staged window (2 windows of the 128)
constexpr int S16_STEM_LDC = S16_STEM_CW + 8;
constexpr int S16_STEM_SW = SS_TILE + 2;
static_assert(S16_THREADS / WAVE * S16_MT == SS_TILE, "the waves' rows are the tile");

constexpr size_t s16_trunk_lds_bytes(int ks) {
    return (size_t)(SS_TILE + ks - 1) * (SS_TILE + ks - 1) * S16_LDC * sizeof(__bf16);
}
constexpr size_t S16_STEM_LDS_BYTES = (size_t)S16_STEM_SW * S16_STEM_SW * S16_STEM_LDC * sizeof(__bf16);

__device__ __forceinline__ bf16x8 zero8() {
    bf16x8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (__bf16)0.f;
    return z;
}
// round to nearest even; NaN -> NaN, +-inf -> +-inf
__device__ __forceinline__ bf16x8 to_bf16x8(f32x4 lo, f32x4 hi) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[j] = (__bf16)lo[j];
        o[4 + j] = (__bf16)hi[j];
    }
    return o;
}

// One step's operands of this lane: its chunk q = 4 step + g of the window's KS x KS x CW flat K.
//   b[nt] = W[tap][n = 16 nt + r][c0 + 8 cc .. +7] of the [taps][48][cin] bf16 planes, aoff = the LDS offset (bf16) of channels
//   8 cc .. +7 of window pixel (4 w + dy, r + dx); past the last chunk: zeros and aoff < 0 (-1 - a valid offset).
template <int KS, int CW>
__device__ __forceinline__ void load_step16(const __bf16* __restrict__ w, int cin, int c0, int sw, int ldc, int step, bf16x8 (&b)[3],
                                            int& aoff) {
    constexpr int CPT = CW / 8, NCHUNK = KS * KS * CPT;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int q = 4 * step + g;
    const bool live = NCHUNK % 4 == 0 || q < NCHUNK;
    const int qq = live ? q : NCHUNK - 1;                 // a valid address either way
    const int tap = qq / CPT, cc = qq - tap * CPT, dy = tap / KS, dx = tap - dy * KS;
    aoff = ((S16_MT * wv + dy) * sw + r + dx) * ldc + 8 * cc;
    if (!live) aoff = -1 - aoff;
#pragma unroll
    for (int nt = 0; nt < 3; ++nt) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(w + ((size_t)tap * SS_CH + 16 * nt + r) * cin + c0 + 8 * cc);
        b[nt] = live ? v : zero8();
    }
}

// acc[mt][nt] += the window's conv: S the staged window (sw pixels wide, ldc bf16 per pixel, CW channels = input channels
// [c0, c0 + CW) of the planes w).  The next step's weights are loaded while the current step's 12 MFMAs run.
template <int KS, int CW>
__device__ __forceinline__ void window_mma16(const __bf16* S, int sw, int ldc, const __bf16* __restrict__ w, int cin, int c0,
                                             f32x4 (&acc)[S16_MT][3]) {
    constexpr int NSTEP = (KS * KS * (CW / 8) + 3) / 4;
    bf16x8 b[3], bn[3];
    int aoff, aoffn = -1;
    load_step16<KS, CW>(w, cin, c0, sw, ldc, 0, b, aoff);
#pragma unroll 1
    for (int step = 0; step < NSTEP; ++step) {
        if (step + 1 < NSTEP) load_step16<KS, CW>(w, cin, c0, sw, ldc, step + 1, bn, aoffn);
        bf16x8 a[S16_MT];
#pragma unroll
        for (int mt = 0; mt < S16_MT; ++mt) {
            const bf16x8 v = *reinterpret_cast<const bf16x8*>(S + (aoff >= 0 ? aoff : -1 - aoff) + mt * sw * ldc);
            a[mt] = aoff >= 0 ? v : zero8();
        }
#pragma unroll
        for (int mt = 0; mt < S16_MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < 3; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int nt = 0; nt < 3; ++nt) b[nt] = bn[nt];
        aoff = aoffn;
    }
}

// Epilogue: lane (r, g) holds D[pixel col 4g + t][channel 16 nt + r] of output row 4w + mt (the C/D map of ss_head.hip's MFMA).
// bias: per-channel bias (stem) or null; RESIDUAL: out += (in place: out is the fp32 residual stream).
template <bool RESIDUAL>
__device__ __forceinline__ void store_tile16(const f32x4 (&acc)[S16_MT][3], const float* __restrict__ bias, float* out, int y0,
                                             int x0, int L) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int mt = 0; mt < S16_MT; ++mt) {
        const int oy = y0 + S16_MT * wv + mt;
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

__device__ __forceinline__ void zero_acc(f32x4 (&acc)[S16_MT][3]) {
#pragma unroll
    for (int mt = 0; mt < S16_MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 3; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// Stem: 3x3, 128 -> 48 with fp32 bias.  The input planes are built while staging, eight channels of a pixel per thread and step
// (one 16-byte LDS store): one-hot channels from the base codes, the 120 maps read in place from atp and rounded to bf16.
__device__ __forceinline__ void ss16_stem_body(__bf16* S, const float* __restrict__ atp, int64_t plane_stride,
                                               const uint8_t* __restrict__ codes, const __bf16* __restrict__ w,
                                               const float* __restrict__ bias, float* __restrict__ out, int L, int y0, int x0) {
    constexpr int NPIX = S16_STEM_SW * S16_STEM_SW;
    f32x4 acc[S16_MT][3];
    zero_acc(acc);
#pragma unroll 1
    for (int win = 0; win < 128 / S16_STEM_CW; ++win) {
        if (win) __syncthreads();                         // every wave is done with the previous window
        for (int e = threadIdx.x; e < S16_STEM_CW / 8 * NPIX; e += S16_THREADS) {
            const int c8 = e / NPIX, p = e - c8 * NPIX;
            const int sy = p / S16_STEM_SW, sx = p - sy * S16_STEM_SW;
            const int iy = y0 - 1 + sy, ix = x0 - 1 + sx, ch0 = win * S16_STEM_CW + 8 * c8;
            bf16x8 v = zero8();
            if (iy >= 0 && iy < L && ix >= 0 && ix < L) {
                if (ch0 == 0) {
                    const int ci = codes[iy], cj = codes[ix];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        v[j] = (__bf16)(ci == j ? 1.f : 0.f);
                        v[4 + j] = (__bf16)(cj == j ? 1.f : 0.f);
                    }
                } else {
                    const float* src = atp + (int64_t)(ch0 - 8) * plane_stride + (int64_t)iy * L + ix;
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = (__bf16)src[(int64_t)j * plane_stride];
                }
            }
            *reinterpret_cast<bf16x8*>(S + p * S16_STEM_LDC + 8 * c8) = v;
        }
        __syncthreads();
        window_mma16<3, S16_STEM_CW>(S, S16_STEM_SW, S16_STEM_LDC, w, 128, win * S16_STEM_CW, acc);
    }
    store_tile16<false>(acc, bias, out, y0, x0, L);
}
template <bool PACKED>
__global__ __launch_bounds__(S16_THREADS) void ss16_stem_kernel(const SsMember* __restrict__ mem, int B, const SsMember lone,
                                                                const __bf16* __restrict__ w, const float* __restrict__ bias,
                                                                float* __restrict__ out) {
    extern __shared__ f32x4 ss16_smem[];
    const SsMember m = ss_member<PACKED>(mem, B, lone, (int)blockIdx.x, &SsMember::tile0);
    const int t = (int)blockIdx.x - m.tile0, ty = t / m.tiles, tx = t - ty * m.tiles;
    ss16_stem_body(reinterpret_cast<__bf16*>(ss16_smem), m.atp, m.plane_stride, m.codes, w, bias, out + (size_t)m.pix0 * SS_CH, m.L,
                   ty * SS_TILE, tx * SS_TILE);
}

// Trunk conv: out (+)= conv_KS(bf16(relu(LN(x)))), 48 -> 48, no bias; x and out are fp32 images.  The bounds tests are those of
// the IMAGE, never of the buffer it lies in (ss_head.hip).
template <int KS, bool RESIDUAL>
__device__ __forceinline__ void ss16_conv_body(__bf16* S, const float* __restrict__ x, const float* __restrict__ gamma,
                                               const float* __restrict__ beta, const __bf16* __restrict__ w, float* out, int L,
                                               int y0, int x0) {
    constexpr int P = KS / 2, SW = SS_TILE + 2 * P;
    for (int p = threadIdx.x; p < SW * SW; p += S16_THREADS) {
        const int sy = p / SW, sx = p - sy * SW, iy = y0 - P + sy, ix = x0 - P + sx;
        bf16x8* dst = reinterpret_cast<bf16x8*>(S + p * S16_LDC);
        if (iy >= 0 && iy < L && ix >= 0 && ix < L) {
            const f32x4* src = reinterpret_cast<const f32x4*>(x + ((size_t)iy * L + ix) * SS_CH);
            f32x4 v[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) v[i] = src[i];
            ln_relu48(v, gamma, beta);
#pragma unroll
            for (int i = 0; i < 6; ++i) dst[i] = to_bf16x8(v[2 * i], v[2 * i + 1]);
        } else {                                          // zero padding of the conv input relu(LN(x)), not relu(LN(0))
#pragma unroll
            for (int i = 0; i < 6; ++i) dst[i] = zero8();
        }
    }
    __syncthreads();
    f32x4 acc[S16_MT][3];
    zero_acc(acc);
    window_mma16<KS, SS_CH>(S, SW, S16_LDC, w, SS_CH, 0, acc);
    store_tile16<RESIDUAL>(acc, nullptr, out, y0, x0, L);
}
template <int KS, bool RESIDUAL, bool PACKED>
__global__ __launch_bounds__(S16_THREADS) void ss16_conv_kernel(const SsMember* __restrict__ mem, int B, const SsMember lone,
                                                                const float* __restrict__ x, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, const __bf16* __restrict__ w,
                                                                float* out) {
    extern __shared__ f32x4 ss16_smem[];
    const SsMember m = ss_member<PACKED>(mem, B, lone, (int)blockIdx.x, &SsMember::tile0);
    const int t = (int)blockIdx.x - m.tile0, ty = t / m.tiles, tx = t - ty * m.tiles;
    const size_t off = (size_t)m.pix0 * SS_CH;
    ss16_conv_body<KS, RESIDUAL>(reinterpret_cast<__bf16*>(ss16_smem), x + off, gamma, beta, w, out + off, m.L, ty * SS_TILE,
                                 tx * SS_TILE);
}

__global__ __launch_bounds__(256) void ss_pack_conv16_kernel(const float* __restrict__ w, __bf16* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (__bf16)w[i];
}

// The launches of ss_head.hip's ss_launch with the bf16 convs.  weights: the table of rnamsm_ss_head, its conv entries bf16 planes.
template <bool PACKED>
int ss16_launch(const SsMember* mem, int B, const SsMember& lone, int64_t blocks, int64_t pixels, int num_blocks,
                const void* const* weights, float* xs, hipStream_t s) {
    float* ts = xs + (size_t)pixels * SS_CH;
    const dim3 grid((unsigned)blocks);
    auto f32 = [](const void* p) { return static_cast<const float*>(p); };
    auto b16 = [](const void* p) { return static_cast<const __bf16*>(p); };
    hipLaunchKernelGGL(ss16_stem_kernel<PACKED>, grid, dim3(S16_THREADS), S16_STEM_LDS_BYTES, s, mem, B, lone, b16(weights[0]),
                       f32(weights[1]), xs);
    RNAMSM_CHECK_LAUNCH(PACKED ? "ss16_stem (packed)" : "ss16_stem");
    for (int k = 0; k < num_blocks; ++k) {
        const void* const* bw = weights + 4 + RNAMSM_SS_WEIGHTS_PER_BLOCK * k;
        hipLaunchKernelGGL((ss16_conv_kernel<3, false, PACKED>), grid, dim3(S16_THREADS), s16_trunk_lds_bytes(3), s, mem, B, lone, xs,
                           f32(bw[1]), f32(bw[2]), b16(bw[0]), ts);
        RNAMSM_CHECK_LAUNCH(PACKED ? "ss16_conv3x3 (packed)" : "ss16_conv3x3");
        hipLaunchKernelGGL((ss16_conv_kernel<5, true, PACKED>), grid, dim3(S16_THREADS), s16_trunk_lds_bytes(5), s, mem, B, lone, ts,
                           f32(bw[4]), f32(bw[5]), b16(bw[3]), xs);
        RNAMSM_CHECK_LAUNCH(PACKED ? "ss16_conv5x5 (packed)" : "ss16_conv5x5");
    }
    const void* const* hw = weights + 4 + RNAMSM_SS_WEIGHTS_PER_BLOCK * num_blocks;
    hipLaunchKernelGGL(ss_out_kernel<PACKED>, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, mem, B, lone, xs, f32(weights[2]),
                       f32(weights[3]), f32(hw[0]), f32(hw[1]), pixels);
    RNAMSM_CHECK_LAUNCH(PACKED ? "ss16_out (packed)" : "ss16_out");
    return RNAMSM_OK;
}

static_assert(S16_STEM_LDS_BYTES <= 65536 && s16_trunk_lds_bytes(5) <= 65536, "the windows fit the default dynamic LDS limit");

}  // namespace
}  // namespace rnamsm

using namespace rnamsm;

extern "C" int rnamsm_ss_pack_conv16(const float* w, uint16_t* out, int64_t n, void* stream) {
    RNAMSM_CHECK_ARG(w && out, "ss_pack_conv16: null pointer");
    RNAMSM_CHECK_ARG(n >= 1 && n <= ((int64_t)1 << 31), "ss_pack_conv16: n=%lld outside [1, 2^31]", (long long)n);
    RNAMSM_CHECK_ARG(((uintptr_t)w & 3u) == 0 && aligned16(out), "ss_pack_conv16: w not 4-byte or out not 16-byte aligned");
    hipLaunchKernelGGL(ss_pack_conv16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), w,
                       reinterpret_cast<__bf16*>(out), n);
    RNAMSM_CHECK_LAUNCH("ss_pack_conv16");
    return RNAMSM_OK;
}

// the same two fp32 images as the fp32 head: the residual stream and the block's middle
extern "C" size_t rnamsm_ss_head16_workspace_bytes(int L) {
    if (L < 1 || L > RNAMSM_SS_MAX_L) return 0;
    return 2 * (size_t)L * L * SS_CH * sizeof(float);
}

extern "C" int rnamsm_ss_head16(const float* atp, int64_t atp_plane_stride, const uint8_t* base_codes, int L, int num_blocks,
                                const void* const* weights, float* logits, float* probs, void* workspace, size_t workspace_bytes,
                                void* stream) {
    RNAMSM_CHECK_ARG(atp && base_codes && weights && workspace, "ss_head16: null pointer");
    RNAMSM_CHECK_ARG(logits || probs, "ss_head16: neither logits nor probs given");
    RNAMSM_CHECK_ARG(L >= 1 && L <= RNAMSM_SS_MAX_L, "ss_head16: L=%d outside [1, %d]", L, RNAMSM_SS_MAX_L);
    RNAMSM_CHECK_ARG(num_blocks >= 1 && num_blocks <= RNAMSM_SS_MAX_BLOCKS, "ss_head16: num_blocks=%d outside [1, %d]", num_blocks,
                     RNAMSM_SS_MAX_BLOCKS);
    RNAMSM_CHECK_ARG(atp_plane_stride >= (int64_t)L * L, "ss_head16: atp plane stride %lld < L*L", (long long)atp_plane_stride);
    RNAMSM_CHECK_ARG(workspace_bytes >= rnamsm_ss_head16_workspace_bytes(L), "ss_head16: workspace too small");
    RNAMSM_CHECK_ARG(aligned16(workspace), "ss_head16: 16-byte alignment of the workspace");
    if (int rc = check_weight_table("ss_head16", weights, RNAMSM_SS_GLOBAL_WEIGHTS + RNAMSM_SS_WEIGHTS_PER_BLOCK * num_blocks)) return rc;
    const int tiles = (L + SS_TILE - 1) / SS_TILE;
    const SsMember lone = {atp, atp_plane_stride, base_codes, logits, probs, 0, L, tiles, 0, 0};
    return ss16_launch<false>(nullptr, 1, lone, (int64_t)tiles * tiles, (int64_t)L * L, num_blocks, weights, static_cast<float*>(workspace),
                              static_cast<hipStream_t>(stream));
}

extern "C" size_t rnamsm_ss_head16_packed_workspace_bytes(int B, const int* Ls) {
    if (B < 1 || B > RNAMSM_SS_MAX_BATCH || !Ls) return 0;
    size_t pixels = 0;
    for (int b = 0; b < B; ++b) {
        if (Ls[b] < 1 || Ls[b] > RNAMSM_SS_MAX_L) return 0;
        pixels += (size_t)Ls[b] * Ls[b];
    }
    return ss_members_bytes(B) + 2 * pixels * SS_CH * sizeof(float);
}

extern "C" int rnamsm_ss_head16_packed(const rnamsm_ss_item* items, int B, int num_blocks, const void* const* weights, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    // every refusal comes before the first launch: a refused call leaves the stream and the outputs untouched
    RNAMSM_CHECK_ARG(items && weights && workspace, "ss_head16_packed: null pointer");
    RNAMSM_CHECK_ARG(B >= 1 && B <= RNAMSM_SS_MAX_BATCH, "ss_head16_packed: B=%d outside [1, %d]", B, RNAMSM_SS_MAX_BATCH);
    RNAMSM_CHECK_ARG(num_blocks >= 1 && num_blocks <= RNAMSM_SS_MAX_BLOCKS, "ss_head16_packed: num_blocks=%d outside [1, %d]", num_blocks,
                     RNAMSM_SS_MAX_BLOCKS);
    int64_t pixels = 0, tiles_total = 0;
    for (int b = 0; b < B; ++b) {
        const rnamsm_ss_item& it = items[b];
        RNAMSM_CHECK_ARG(it.L >= 1 && it.L <= RNAMSM_SS_MAX_L, "ss_head16_packed: member %d: L=%d outside [1, %d]", b, it.L, RNAMSM_SS_MAX_L);
        RNAMSM_CHECK_ARG(it.atp && it.base_codes, "ss_head16_packed: member %d: null pointer", b);
        RNAMSM_CHECK_ARG(it.logits || it.probs, "ss_head16_packed: member %d: neither logits nor probs given", b);
        RNAMSM_CHECK_ARG(((uintptr_t)it.atp & 3u) == 0 && ((uintptr_t)it.logits & 3u) == 0 && ((uintptr_t)it.probs & 3u) == 0,
                         "ss_head16_packed: member %d: a float pointer is not 4-byte aligned", b);
        RNAMSM_CHECK_ARG(it.atp_plane_stride >= (int64_t)it.L * it.L, "ss_head16_packed: member %d: atp plane stride %lld < L*L", b,
                         (long long)it.atp_plane_stride);
        const int64_t t = (it.L + SS_TILE - 1) / SS_TILE;
        pixels += (int64_t)it.L * it.L;
        tiles_total += t * t;
    }
    RNAMSM_CHECK_ARG(aligned16(workspace), "ss_head16_packed: 16-byte alignment of the workspace");
    RNAMSM_CHECK_ARG(workspace_bytes >= ss_members_bytes(B) + 2 * (size_t)pixels * SS_CH * sizeof(float),
                     "ss_head16_packed: workspace too small");
    if (int rc = check_weight_table("ss_head16_packed", weights, RNAMSM_SS_GLOBAL_WEIGHTS + RNAMSM_SS_WEIGHTS_PER_BLOCK * num_blocks))
        return rc;
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
    }, s, "ss16_members");
    if (rc != RNAMSM_OK) return rc;
    return ss16_launch<true>(mem, B, SsMember{}, tiles_total, pixels, num_blocks, weights,
                             reinterpret_cast<float*>(static_cast<char*>(workspace) + ss_members_bytes(B)), s);
}
