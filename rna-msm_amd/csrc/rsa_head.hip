// RNA-MSM RSA (relative solvent accessibility) predictor: the reference's _downstream_tasks/RSA network -- a squeeze-excite
// BasicBlock(Cin -> 64) over the normalised [one-hot | embedding | mask] columns, one minGPT Block(64, 8 heads), Linear(64 -> 1),
// sigmoid -- for all K ensemble members in FOUR launches (the model is gridDim.y of each), exact fp32, no atomics:
//   rsa_stem   conv1 (k = 3) and the 1x1 shortcut as one implicit GEMM on v_mfma_f32_32x32x2_f32, normalisation / one-hot / mask
//              built while staging, the embedding read in place through its row stride; BN1 + ReLU and BNs in the epilogue
//   rsa_conv2  conv2 (k = 3, 64 -> 64) + BN2 + ReLU, per-tile channel sums for the squeeze
//   rsa_mix    squeeze-excite from the tile sums (fixed order), scale + shortcut + ReLU, LN1, Q / K / V
//   rsa_attn   softmax(Q K^T / sqrt 8) V over all 8 heads of a 32-query tile (K / V streamed through LDS, 64 keys a time),
//              proj + residual, LN2, the MLP (exact-erf GELU), Linear(64 -> 1), sigmoid
// The only whole-sequence dependencies are the squeeze mean (launch 2 -> 3) and the attention keys (3 -> 4).
// Every sum has one fixed order that depends on L and the position alone: same bits on every run, for a member inside any ensemble.
#include "common.h"

namespace rnamsm {
namespace {

constexpr int RSA_CH = 64;             // planes
constexpr int RSA_TILE = 32;           // positions per block, every kernel
constexpr int RSA_EMB = 768;
constexpr int RSA_KC = 32;             // input channels staged per step of the stem
constexpr int RSA_CIN_PAD = 800;       // 773 / 769 input channels padded to whole steps (zero weights, zero inputs)
constexpr int RSA_XP = RSA_TILE + 3;   // pitch of the stem's staged [channel][position + halo] tile (odd: conflict-free transposing writes)
constexpr int RSA_STEM_THREADS = 512;  // 8 waves: 2 output-channel halves x 4 quarters of every 32-channel step
constexpr int RSA_THREADS = 256;
constexpr int RSA_HID = 256;
constexpr int RSA_KEYS = 64;           // keys per streamed K / V chunk
constexpr int RSA_MAX_TILES = RNAMSM_RSA_MAX_L / RSA_TILE;
constexpr int RSA_LONG_TILES = RNAMSM_LONG_MAX_L / RSA_TILE;      // tile-sum rows of the long layout (rnamsm_rsa_head_long)
constexpr int RSA_SUM_GROUP = 32;      // tile sums per chain of the squeeze mean beyond RSA_MAX_TILES tiles
static_assert(RSA_SUM_GROUP == RSA_MAX_TILES, "one group of tile sums is the existing layout's one chain");
constexpr float RSA_LN_EPS = 1e-5f;

// per-model workspace: h1, shortcut, h2, y, q, k, v ([L][64] each) and the tile sums [TR][64] -- TR = 32 rows in the layout of
// rnamsm_rsa_head / _packed, 128 in the one of rnamsm_rsa_head_long.  TR is a template argument of the four bodies: the slab size
// stays a compile-time function of L in every instance, as it was.
template <int TR = RSA_MAX_TILES>
__host__ __device__ inline size_t rsa_model_floats(int L) { return (size_t)7 * L * RSA_CH + (size_t)TR * RSA_CH; }

// The caller's weight table lives on the host (as rnamsm_ss_head's): it travels to every launch by value, in the kernel arguments.
constexpr int RSA_TABLE_MAX = RNAMSM_RSA_GLOBAL_WEIGHTS + RNAMSM_RSA_WEIGHTS_PER_MODEL * RNAMSM_RSA_MAX_MODELS;
struct RsaTable {
    const void* p[RSA_TABLE_MAX];
};
struct RsaModel {          // one member's slice of the table (include/rnamsm.h, RNAMSM_RSA_WEIGHTS_PER_MODEL entries)
    const float* w[RNAMSM_RSA_WEIGHTS_PER_MODEL];
};
__device__ __forceinline__ RsaModel rsa_model(const RsaTable& table, int m) {
    RsaModel r;
#pragma unroll
    for (int i = 0; i < RNAMSM_RSA_WEIGHTS_PER_MODEL; ++i)
        r.w[i] = static_cast<const float*>(table.p[RNAMSM_RSA_GLOBAL_WEIGHTS + m * RNAMSM_RSA_WEIGHTS_PER_MODEL + i]);
    return r;
}
enum {   // indices inside a member's slice
    W_STEM = 0, W_BN1_S, W_BN1_B, W_BNS_S, W_BNS_B, W_CONV2, W_BN2_S, W_BN2_B, W_SE1_W, W_SE1_B, W_SE2_W, W_SE2_B,
    W_LN1_G, W_LN1_B, W_QKV_W, W_QKV_B, W_PROJ_W, W_PROJ_B, W_LN2_G, W_LN2_B, W_FC1_W, W_FC1_B, W_FC2_W, W_FC2_B, W_OUT_W, W_OUT_B
};
static_assert(W_OUT_B + 1 == RNAMSM_RSA_WEIGHTS_PER_MODEL, "weight table layout");

// ---- the member of a block ------------------------------------------------------------------------------------------------------
// One kernel per stage serves the lone call (rnamsm_rsa_head) and the batched one (rnamsm_rsa_head_packed).  A launch has the SUM
// of the members' 32-position tiles as gridDim.x and the model as gridDim.y.  Batched, mem is the device table of the B members
// and a block finds its own by a search over the tile prefix sums (common.h: member_of); lone, mem is null and the one member is
// the kernel argument itself (tile0 = 0, ws_off = 0: the caller's workspace with no table in front).  Either way the stage's body
// runs on the member's own (embedding, L, workspace base, tile): one arithmetic, so a member's bits depend on nothing else.
// The choice is a template argument, not a test of mem: one definition, two code objects.  With the test inside the kernel the
// compiler reads the descriptor through ONE flat load of a selected address (table or kernel argument) and L, the offsets and the
// pointers land in vector registers: +4 to +8 VGPRs over the lone kernels in three of the four stages.
// Every member has its own K model slabs in the workspace (floats [ws_off, ws_off + K * rsa_model_floats(L))): its tile sums, K
// and V live there, so the squeeze mean and the attention keys of a member are its own.
struct RsaMember {           // 64 bytes
    const float* emb;
    int64_t emb_stride;
    const uint8_t* codes;
    float* logits;
    float* probs;
    int64_t ws_off;          // floats of the members' slabs before it
    int32_t L;
    int32_t tile0;           // tiles of the members before it
    int32_t pad_[2];
};
static_assert(sizeof(RsaMember) == 64, "RsaMember layout");
template <bool PACKED>
__device__ __forceinline__ RsaMember rsa_member(const RsaMember* __restrict__ mem, int B, const RsaMember& lone) {
    if (PACKED) return mem[member_of(mem, B, (int)blockIdx.x, &RsaMember::tile0)];
    return lone;
}

// ---------------------------------------------------------------------------------------------------------------- launch 1
// Block (tile of 32 positions, model).  Per 32-channel step the tile [32 channels][34 positions] is staged normalised; wave
// (half, quarter) multiplies its 8 channels of the step into four 32 x 32 accumulators (conv taps 0..2 and the shortcut, which is
// the centre tap of the same staged input against a second weight slab) for output channels half*32 ..+32.  The four quarters are
// then summed in fixed order through LDS.
// In the four bodies ws is the MEMBER's base (its K model slabs); LDS is the calling kernel's.
constexpr int RSA_STEM_XS = RSA_KC * RSA_XP;
constexpr int RSA_STEM_RED = 3 * 2 * 2 * 16 * 64;
template <int TR>
__device__ __forceinline__ void rsa_stem_body(float* Xs, float* Red, const float* __restrict__ emb, int64_t emb_stride,
                                              const uint8_t* __restrict__ codes, int L, int use_onehot, const RsaTable& table,
                                              float* __restrict__ ws, int m, int p0) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int half = wave & 1, quarter = wave >> 1;
    const RsaModel M = rsa_model(table, m);
    const float* mu_emb = static_cast<const float*>(table.p[0]);
    const float* sd_emb = static_cast<const float*>(table.p[1]);
    const double* mu_oh = static_cast<const double*>(table.p[2]);
    const double* sd_oh = static_cast<const double*>(table.p[3]);
    const int noh = use_onehot ? 4 : 0, cin = noh + RSA_EMB + 1;

    f32x16 acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[a][i] = 0.f;

    const int sc = t & 31, spl = t >> 5;       // staging: channel of the step, local position (16 per pass)
    const int r = lane & 31, kk = lane >> 5;
    const float* wbase = M.w[W_STEM] + half * 32 + r;
    for (int c0 = 0; c0 < RSA_CIN_PAD; c0 += RSA_KC) {
        __syncthreads();
        const int c = c0 + sc;
#pragma unroll
        for (int pass = 0; pass < 3; ++pass) {
            const int pl = spl + 16 * pass;
            const int p = p0 - 1 + pl;
            if (pl < RSA_TILE + 2) {
                float v = 0.f;        // the reference's Conv1d zero padding is applied to the NORMALISED input, mask channel included
                if (p >= 0 && p < L && c < cin) {
                    if (c < noh) {          // numpy's arithmetic: float64 statistics for the one-hot columns, float32 for the embedding
                        const double oh = codes[p] == c ? 1.0 : 0.0;
                        v = (float)((oh - mu_oh[c]) / sd_oh[c]);
                    } else if (c == cin - 1) {
                        v = 1.f;
                    } else {
                        const int e = c - noh;
                        v = __fdiv_rn(__fsub_rn(emb[(int64_t)p * emb_stride + e], mu_emb[e]), sd_emb[e]);
                    }
                }
                Xs[sc * RSA_XP + pl] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int cl = quarter * 8 + s * 2 + kk;          // this lane's k row of the step
            const float* wr = wbase + (size_t)(c0 + cl) * RSA_CH;
            const float* xr = Xs + cl * RSA_XP + r;
            const float x0 = xr[0], x1 = xr[1], x2 = xr[2];
            acc[0] = mfma32(x0, wr[0], acc[0]);
            acc[1] = mfma32(x1, wr[(size_t)RSA_CIN_PAD * RSA_CH], acc[1]);
            acc[2] = mfma32(x2, wr[(size_t)2 * RSA_CIN_PAD * RSA_CH], acc[2]);
            acc[3] = mfma32(x1, wr[(size_t)3 * RSA_CIN_PAD * RSA_CH], acc[3]);
        }
    }
    f32x16 conv, shortcut = acc[3];
#pragma unroll
    for (int i = 0; i < 16; ++i) conv[i] = (acc[0][i] + acc[1][i]) + acc[2][i];
    if (quarter > 0) {
        float* dst = Red + ((size_t)((quarter - 1) * 2 + half) * 2) * 16 * 64;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            dst[i * 64 + lane] = conv[i];
            dst[(16 + i) * 64 + lane] = shortcut[i];
        }
    }
    __syncthreads();
    if (quarter == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float* src = Red + ((size_t)(q * 2 + half) * 2) * 16 * 64;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                conv[i] += src[i * 64 + lane];
                shortcut[i] += src[(16 + i) * 64 + lane];
            }
        }
        const int co = half * 32 + r;
        const float s1 = M.w[W_BN1_S][co], b1 = M.w[W_BN1_B][co], ss = M.w[W_BNS_S][co], bs = M.w[W_BNS_B][co];
        float* h1 = ws + (size_t)m * rsa_model_floats<TR>(L);
        float* sh = h1 + (size_t)L * RSA_CH;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int p = p0 + (i & 3) + 8 * (i >> 2) + 4 * kk;      // accumulator layout: common.h mfma32
            if (p < L) {
                h1[(size_t)p * RSA_CH + co] = relu_nan(fmaf(conv[i], s1, b1));
                sh[(size_t)p * RSA_CH + co] = fmaf(shortcut[i], ss, bs);
            }
        }
    }
}
template <bool PACKED, int TR>
__global__ __launch_bounds__(RSA_STEM_THREADS) void rsa_stem_kernel(const RsaMember* __restrict__ mem, int B, const RsaMember lone,
                                                                    int use_onehot, const RsaTable table, float* __restrict__ ws) {
    __shared__ float Xs[RSA_STEM_XS];
    __shared__ float Red[RSA_STEM_RED];
    const RsaMember m = rsa_member<PACKED>(mem, B, lone);
    rsa_stem_body<TR>(Xs, Red, m.emb, m.emb_stride, m.codes, m.L, use_onehot, table, ws + m.ws_off, blockIdx.y,
                      ((int)blockIdx.x - m.tile0) * RSA_TILE);
}

// out[j] += sum_ci Wt[ci][co] * Xs[(pb + j)][ci], ci ascending: thread (co, 8 positions); Xs rows are read as wave-wide broadcasts
template <int NP>
__device__ __forceinline__ void dense_acc(const float* __restrict__ Wt, int ldw, int co, const float* Xs, int ldx, int pb, int K,
                                          float (&acc)[NP]) {
#pragma unroll 2
    for (int ci = 0; ci < K; ci += 4) {
        const float w0 = Wt[(size_t)ci * ldw + co], w1 = Wt[(size_t)(ci + 1) * ldw + co];
        const float w2 = Wt[(size_t)(ci + 2) * ldw + co], w3 = Wt[(size_t)(ci + 3) * ldw + co];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(Xs + (pb + j) * ldx + ci);
            acc[j] = fmaf(w0, x[0], acc[j]);
            acc[j] = fmaf(w1, x[1], acc[j]);
            acc[j] = fmaf(w2, x[2], acc[j]);
            acc[j] = fmaf(w3, x[3], acc[j]);
        }
    }
}

// LayerNorm(64) of the 32 rows of Src into Dst (both [32][64] in LDS): wave w takes rows 8w .. 8w+7, lane = channel
__device__ __forceinline__ void ln_tile(const float* Src, float* Dst, const float* __restrict__ g, const float* __restrict__ b, int t) {
    const int lane = t & 63, wave = t >> 6;
    const float gg = g[lane], bb = b[lane];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int p = wave * 8 + j;
        const float v = Src[p * RSA_CH + lane];
        const float mean = wave_sum(v) * (1.f / RSA_CH);
        const float d = v - mean;
        const float var = wave_sum(d * d) * (1.f / RSA_CH);
        Dst[p * RSA_CH + lane] = fmaf(d * (1.f / sqrtf(var + RSA_LN_EPS)), gg, bb);
    }
}

// ---------------------------------------------------------------------------------------------------------------- launch 2
template <int TR>
__device__ __forceinline__ void rsa_conv2_body(float* Xs, float* Ps, int L, const RsaTable& table, float* __restrict__ ws, int m,
                                               int p0) {
    const int t = threadIdx.x, co = t & 63, pg = t >> 6;
    const RsaModel M = rsa_model(table, m);
    float* base = ws + (size_t)m * rsa_model_floats<TR>(L);
    const float* h1 = base;
    float* h2 = base + (size_t)2 * L * RSA_CH;
    float* part = base + (size_t)7 * L * RSA_CH;
    for (int i = t; i < (RSA_TILE + 2) * RSA_CH; i += RSA_THREADS) {
        const int p = p0 - 1 + i / RSA_CH;
        Xs[i] = (p >= 0 && p < L) ? h1[(size_t)p * RSA_CH + (i % RSA_CH)] : 0.f;
    }
    __syncthreads();
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll 1
    for (int tap = 0; tap < 3; ++tap) dense_acc<8>(M.w[W_CONV2] + (size_t)tap * RSA_CH * RSA_CH, RSA_CH, co, Xs, RSA_CH, pg * 8 + tap, RSA_CH, acc);
    const float s2 = M.w[W_BN2_S][co], b2 = M.w[W_BN2_B][co];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int p = p0 + pg * 8 + j;
        if (p < L) {
            const float v = relu_nan(fmaf(acc[j], s2, b2));
            h2[(size_t)p * RSA_CH + co] = v;
            sum += v;
        }
    }
    Ps[pg * RSA_CH + co] = sum;
    __syncthreads();
    if (t < RSA_CH) part[(size_t)(p0 / RSA_TILE) * RSA_CH + t] = ((Ps[t] + Ps[RSA_CH + t]) + Ps[2 * RSA_CH + t]) + Ps[3 * RSA_CH + t];
}
template <bool PACKED, int TR>
__global__ __launch_bounds__(RSA_THREADS) void rsa_conv2_kernel(const RsaMember* __restrict__ mem, int B, const RsaMember lone,
                                                                const RsaTable table, float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float Xs[(RSA_TILE + 2) * RSA_CH];
    __shared__ float Ps[4 * RSA_CH];
    const RsaMember m = rsa_member<PACKED>(mem, B, lone);
    rsa_conv2_body<TR>(Xs, Ps, m.L, table, ws + m.ws_off, blockIdx.y, ((int)blockIdx.x - m.tile0) * RSA_TILE);
}

// ---------------------------------------------------------------------------------------------------------------- launch 3
// Sc: the squeeze-excite's scratch -- the channel means [64], the hidden units [4], the gate [64]
constexpr int RSA_MIX_SC = 2 * RSA_CH + 4;
template <int TR>
__device__ __forceinline__ void rsa_mix_body(float* Ys, float* Xs, float* Sc, int L, const RsaTable& table, float* __restrict__ ws,
                                             int m, int p0) {
    float* Mean = Sc;
    float* Z = Sc + RSA_CH;
    float* Gate = Sc + RSA_CH + 4;
    const int t = threadIdx.x, co = t & 63, pg = t >> 6;
    const RsaModel M = rsa_model(table, m);
    float* base = ws + (size_t)m * rsa_model_floats<TR>(L);
    const float* sh = base + (size_t)L * RSA_CH;
    const float* h2 = base + (size_t)2 * L * RSA_CH;
    float* y = base + (size_t)3 * L * RSA_CH;
    float* qkv = base + (size_t)4 * L * RSA_CH;
    const float* part = base + (size_t)7 * L * RSA_CH;
    // squeeze-excite: every block repeats the same few hundred operations in the same order
    if (t < RSA_CH) {
        const int tiles = (L + RSA_TILE - 1) / RSA_TILE;
        float s = 0.f;
        if (TR <= RSA_SUM_GROUP) {
            for (int i = 0; i < tiles; ++i) s += part[(size_t)i * RSA_CH + t];
        } else {
            // one ascending chain per group of 32 tiles, the group sums added ascending: the chain above when there is one group
            for (int g0 = 0; g0 < tiles; g0 += RSA_SUM_GROUP) {
                const int gn = min(tiles, g0 + RSA_SUM_GROUP);
                float gs = 0.f;
                for (int i = g0; i < gn; ++i) gs += part[(size_t)i * RSA_CH + t];
                s = g0 ? s + gs : gs;
            }
        }
        Mean[t] = s / (float)L;
    }
    __syncthreads();
    if (t < 4) {
        float z = 0.f;
        for (int c = 0; c < RSA_CH; ++c) z = fmaf(M.w[W_SE1_W][t * RSA_CH + c], Mean[c], z);
        Z[t] = relu_nan(z + M.w[W_SE1_B][t]);
    }
    __syncthreads();
    if (t < RSA_CH) {
        float z = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) z = fmaf(M.w[W_SE2_W][t * 4 + c], Z[c], z);
        z += M.w[W_SE2_B][t];
        Gate[t] = 1.f / (1.f + expf(-z));
    }
    __syncthreads();
    for (int i = t; i < RSA_TILE * RSA_CH; i += RSA_THREADS) {
        const int p = p0 + i / RSA_CH, c = i % RSA_CH;
        float v = 0.f;
        if (p < L) {
            v = relu_nan(fmaf(h2[(size_t)p * RSA_CH + c], Gate[c], sh[(size_t)p * RSA_CH + c]));
            y[(size_t)p * RSA_CH + c] = v;
        }
        Ys[i] = v;
    }
    __syncthreads();
    ln_tile(Ys, Xs, M.w[W_LN1_G], M.w[W_LN1_B], t);
    __syncthreads();
#pragma unroll 1
    for (int which = 0; which < 3; ++which) {        // query, key, value
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        dense_acc<8>(M.w[W_QKV_W] + (size_t)which * RSA_CH * RSA_CH, RSA_CH, co, Xs, RSA_CH, pg * 8, RSA_CH, acc);
        const float b = M.w[W_QKV_B][which * RSA_CH + co];
        float* dst = qkv + (size_t)which * L * RSA_CH;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int p = p0 + pg * 8 + j;
            if (p < L) dst[(size_t)p * RSA_CH + co] = acc[j] + b;
        }
    }
}
template <bool PACKED, int TR>
__global__ __launch_bounds__(RSA_THREADS) void rsa_mix_kernel(const RsaMember* __restrict__ mem, int B, const RsaMember lone,
                                                              const RsaTable table, float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float Ys[RSA_TILE * RSA_CH];
    __shared__ __attribute__((aligned(16))) float Xs[RSA_TILE * RSA_CH];
    __shared__ float Sc[RSA_MIX_SC];
    const RsaMember m = rsa_member<PACKED>(mem, B, lone);
    rsa_mix_body<TR>(Ys, Xs, Sc, m.L, table, ws + m.ws_off, blockIdx.y, ((int)blockIdx.x - m.tile0) * RSA_TILE);
}

// ---------------------------------------------------------------------------------------------------------------- launch 4
// Thread (query ql = t / 8, head h = t % 8) owns one row of one head's attention: sweep 1 finds the row maximum, sweep 2 the
// exponentials, their sum and the weighted values (the softmax of the reference, no running rescale).  Sums over the keys are
// two-level: inside a 64-key chunk, then over the chunks.
// The keys are [0, L) of the member's own K / V and nothing else; logits / probs: the member's [K, L] (either may be null).
template <int TR>
__device__ __forceinline__ void rsa_attn_body(float* KV, float* Ys, float* Xs, int L, const RsaTable& table,
                                              const float* __restrict__ ws, int m, int p0, float* __restrict__ logits,
                                              float* __restrict__ probs) {
    const int t = threadIdx.x, co = t & 63, pg = t >> 6;
    const RsaModel M = rsa_model(table, m);
    const float* base = ws + (size_t)m * rsa_model_floats<TR>(L);
    const float* y = base + (size_t)3 * L * RSA_CH;
    const float* qg = base + (size_t)4 * L * RSA_CH;
    const float* kg = base + (size_t)5 * L * RSA_CH;
    const float* vg = base + (size_t)6 * L * RSA_CH;
    float* Ks = KV;
    float* Vs = KV + RSA_KEYS * RSA_CH;

    const int h = t & 7, ql = t >> 3;
    const int pq = p0 + ql;
    float q[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) q[d] = pq < L ? qg[(size_t)pq * RSA_CH + h * 8 + d] : 0.f;
    const float scale = 0.35355339059327373f;       // 1 / sqrt(8), applied to the logit as the reference does

    float mx = -INFINITY;
    for (int j0 = 0; j0 < L; j0 += RSA_KEYS) {
        __syncthreads();
        for (int i = t; i < RSA_KEYS * RSA_CH / 4; i += RSA_THREADS) {
            const int j = j0 + i / (RSA_CH / 4);
            f32x4 kv = {0.f, 0.f, 0.f, 0.f};
            if (j < L) kv = *reinterpret_cast<const f32x4*>(kg + (size_t)j0 * RSA_CH + (size_t)i * 4);
            *reinterpret_cast<f32x4*>(Ks + i * 4) = kv;
        }
        __syncthreads();
        const int jn = min(RSA_KEYS, L - j0);
        for (int j = 0; j < jn; ++j) {
            const f32x4 k0 = *reinterpret_cast<const f32x4*>(Ks + j * RSA_CH + h * 8);
            const f32x4 k1 = *reinterpret_cast<const f32x4*>(Ks + j * RSA_CH + h * 8 + 4);
            float s = q[0] * k0[0];
            s = fmaf(q[1], k0[1], s); s = fmaf(q[2], k0[2], s); s = fmaf(q[3], k0[3], s);
            s = fmaf(q[4], k1[0], s); s = fmaf(q[5], k1[1], s); s = fmaf(q[6], k1[2], s); s = fmaf(q[7], k1[3], s);
            mx = fmaxf(mx, s * scale);
        }
    }
    float den = 0.f, o[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) o[d] = 0.f;
    for (int j0 = 0; j0 < L; j0 += RSA_KEYS) {
        __syncthreads();
        for (int i = t; i < RSA_KEYS * RSA_CH / 4; i += RSA_THREADS) {
            const int j = j0 + i / (RSA_CH / 4);
            f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
            if (j < L) {
                kv = *reinterpret_cast<const f32x4*>(kg + (size_t)j0 * RSA_CH + (size_t)i * 4);
                vv = *reinterpret_cast<const f32x4*>(vg + (size_t)j0 * RSA_CH + (size_t)i * 4);
            }
            *reinterpret_cast<f32x4*>(Ks + i * 4) = kv;
            *reinterpret_cast<f32x4*>(Vs + i * 4) = vv;
        }
        __syncthreads();
        const int jn = min(RSA_KEYS, L - j0);
        float cden = 0.f, c[8];
#pragma unroll
        for (int d = 0; d < 8; ++d) c[d] = 0.f;
        for (int j = 0; j < jn; ++j) {
            const f32x4 k0 = *reinterpret_cast<const f32x4*>(Ks + j * RSA_CH + h * 8);
            const f32x4 k1 = *reinterpret_cast<const f32x4*>(Ks + j * RSA_CH + h * 8 + 4);
            float s = q[0] * k0[0];
            s = fmaf(q[1], k0[1], s); s = fmaf(q[2], k0[2], s); s = fmaf(q[3], k0[3], s);
            s = fmaf(q[4], k1[0], s); s = fmaf(q[5], k1[1], s); s = fmaf(q[6], k1[2], s); s = fmaf(q[7], k1[3], s);
            const float e = expf(s * scale - mx);
            cden += e;
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(Vs + j * RSA_CH + h * 8);
            const f32x4 v1 = *reinterpret_cast<const f32x4*>(Vs + j * RSA_CH + h * 8 + 4);
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                c[d] = fmaf(e, v0[d], c[d]);
                c[4 + d] = fmaf(e, v1[d], c[4 + d]);
            }
        }
        den += cden;
#pragma unroll
        for (int d = 0; d < 8; ++d) o[d] += c[d];
    }
    // context [32][64] -> Xs; the block's rows of y -> Ys
#pragma unroll
    for (int d = 0; d < 8; ++d) Xs[ql * RSA_CH + h * 8 + d] = pq < L ? o[d] / den : 0.f;
    for (int i = t; i < RSA_TILE * RSA_CH; i += RSA_THREADS) {
        const int p = p0 + i / RSA_CH;
        Ys[i] = p < L ? y[(size_t)p * RSA_CH + (i % RSA_CH)] : 0.f;
    }
    __syncthreads();
    {   // y += proj(context) + bias
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        dense_acc<8>(M.w[W_PROJ_W], RSA_CH, co, Xs, RSA_CH, pg * 8, RSA_CH, acc);
        const float b = M.w[W_PROJ_B][co];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) Ys[(pg * 8 + j) * RSA_CH + co] += acc[j] + b;
    }
    __syncthreads();
    ln_tile(Ys, Xs, M.w[W_LN2_G], M.w[W_LN2_B], t);
    __syncthreads();
    float* Hs = KV;                                   // [32][256]
    {   // hidden = gelu(W1 ln2 + b1): thread = hidden unit, all 32 positions
        const float b = M.w[W_FC1_B][t];
#pragma unroll 1
        for (int g = 0; g < 4; ++g) {
            float acc[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = 0.f;
            dense_acc<8>(M.w[W_FC1_W], RSA_HID, t, Xs, RSA_CH, g * 8, RSA_CH, acc);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = acc[j] + b;
                Hs[(g * 8 + j) * RSA_HID + t] = 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
            }
        }
    }
    __syncthreads();
    {   // y += W2 hidden + b2
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        dense_acc<8>(M.w[W_FC2_W], RSA_CH, co, Hs, RSA_HID, pg * 8, RSA_HID, acc);
        const float b = M.w[W_FC2_B][co];
#pragma unroll
        for (int j = 0; j < 8; ++j) Ys[(pg * 8 + j) * RSA_CH + co] += acc[j] + b;
    }
    __syncthreads();
    {   // Linear(64 -> 1) + sigmoid: wave w takes rows 8w .. 8w+7
        const int lane = t & 63, wave = t >> 6;
        const float wf = M.w[W_OUT_W][lane], bf = M.w[W_OUT_B][0];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int p = p0 + wave * 8 + j;
            const float z = wave_sum(Ys[(wave * 8 + j) * RSA_CH + lane] * wf) + bf;
            if (lane == 0 && p < L) {
                if (logits) logits[(size_t)m * L + p] = z;
                if (probs) probs[(size_t)m * L + p] = 1.f / (1.f + expf(-z));
            }
        }
    }
}
template <bool PACKED, int TR>
__global__ __launch_bounds__(RSA_THREADS) void rsa_attn_kernel(const RsaMember* __restrict__ mem, int B, const RsaMember lone,
                                                               const RsaTable table, const float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float KV[2 * RSA_KEYS * RSA_CH];      // K / V chunk; later the MLP's hidden tile [32][256]
    __shared__ __attribute__((aligned(16))) float Ys[RSA_TILE * RSA_CH];
    __shared__ __attribute__((aligned(16))) float Xs[RSA_TILE * RSA_CH];
    const RsaMember m = rsa_member<PACKED>(mem, B, lone);
    rsa_attn_body<TR>(KV, Ys, Xs, m.L, table, ws + m.ws_off, blockIdx.y, ((int)blockIdx.x - m.tile0) * RSA_TILE, m.logits, m.probs);
}

constexpr size_t rsa_members_bytes(int B) { return ((size_t)B * sizeof(RsaMember) + 255) & ~(size_t)255; }

// The four launches over `tiles` tiles of n_models models each, on the layout with TR tile-sum rows: PACKED with mem / B the
// uploaded table of a batch, else null / 1 and the lone member.  The instances are <false, RSA_MAX_TILES> (rnamsm_rsa_head),
// <true, RSA_MAX_TILES> (_packed) and <false, RSA_LONG_TILES> (_long).  weights: checked by the caller.
template <bool PACKED, int TR>
int rsa_launch(const RsaMember* mem, int B, const RsaMember& lone, int64_t tiles, int n_models, int use_onehot,
               const void* const* weights, float* ws, hipStream_t s) {
    const int nw = RNAMSM_RSA_GLOBAL_WEIGHTS + RNAMSM_RSA_WEIGHTS_PER_MODEL * n_models;
    RsaTable table;
    for (int i = 0; i < RSA_TABLE_MAX; ++i) table.p[i] = i < nw ? weights[i] : nullptr;
    const dim3 grid((unsigned)tiles, (unsigned)n_models);      // the members' own tiles, nothing for a short member beside a long one
    constexpr bool LONG = TR > RSA_MAX_TILES;
    hipLaunchKernelGGL((rsa_stem_kernel<PACKED, TR>), grid, dim3(RSA_STEM_THREADS), 0, s, mem, B, lone, use_onehot ? 1 : 0, table, ws);
    RNAMSM_CHECK_LAUNCH(PACKED ? "rsa_stem (packed)" : LONG ? "rsa_stem (long)" : "rsa_stem");
    hipLaunchKernelGGL((rsa_conv2_kernel<PACKED, TR>), grid, dim3(RSA_THREADS), 0, s, mem, B, lone, table, ws);
    RNAMSM_CHECK_LAUNCH(PACKED ? "rsa_conv2 (packed)" : LONG ? "rsa_conv2 (long)" : "rsa_conv2");
    hipLaunchKernelGGL((rsa_mix_kernel<PACKED, TR>), grid, dim3(RSA_THREADS), 0, s, mem, B, lone, table, ws);
    RNAMSM_CHECK_LAUNCH(PACKED ? "rsa_mix (packed)" : LONG ? "rsa_mix (long)" : "rsa_mix");
    hipLaunchKernelGGL((rsa_attn_kernel<PACKED, TR>), grid, dim3(RSA_THREADS), 0, s, mem, B, lone, table, ws);
    RNAMSM_CHECK_LAUNCH(PACKED ? "rsa_attn (packed)" : LONG ? "rsa_attn (long)" : "rsa_attn");
    return RNAMSM_OK;
}

// the entries of the table that a call reads: all, but for the one-hot statistics (2, 3) of an embedding-only ensemble
int rsa_check_weights(const char* prefix, const void* const* weights, int n_models, int use_onehot) {
    return check_weight_table(prefix, weights, RNAMSM_RSA_GLOBAL_WEIGHTS + RNAMSM_RSA_WEIGHTS_PER_MODEL * n_models,
                              use_onehot ? 0u : 0xCu);
}

}  // namespace
}  // namespace rnamsm

using namespace rnamsm;

extern "C" size_t rnamsm_rsa_head_workspace_bytes(int L, int n_models) {
    if (L < 1 || L > RNAMSM_RSA_MAX_L || n_models < 1 || n_models > RNAMSM_RSA_MAX_MODELS) return 0;
    return (size_t)n_models * rsa_model_floats(L) * sizeof(float);
}

// The lone call, written once for rnamsm_rsa_head (who = "rsa_head", TR = RSA_MAX_TILES, max_L = RNAMSM_RSA_MAX_L) and
// rnamsm_rsa_head_long ("rsa_head_long", RSA_LONG_TILES, RNAMSM_LONG_MAX_L), as ss_head_lone is: one list of refusals under the
// entry's own name and limit, every one before the first launch, then the four launches on the layout with TR tile-sum rows.
template <int TR>
static int rsa_head_lone(const char* who, int max_L, const float* emb, int64_t emb_row_stride, const uint8_t* base_codes, int L,
                         int n_models, int use_onehot, const void* const* weights, float* probs, float* logits, void* workspace,
                         size_t workspace_bytes, void* stream) {
    RNAMSM_CHECK_ARG(emb, "%s: null pointer (emb)", who);
    RNAMSM_CHECK_ARG(base_codes, "%s: null pointer (base_codes)", who);
    RNAMSM_CHECK_ARG(weights, "%s: null pointer (weights)", who);
    RNAMSM_CHECK_ARG(workspace, "%s: null pointer (workspace)", who);
    RNAMSM_CHECK_ARG(logits || probs, "%s: neither probs nor logits given", who);
    RNAMSM_CHECK_ARG(L >= 1 && L <= max_L, "%s: L=%d outside [1, %d]", who, L, max_L);
    RNAMSM_CHECK_ARG(n_models >= 1 && n_models <= RNAMSM_RSA_MAX_MODELS, "%s: n_models=%d outside [1, %d]", who, n_models,
                     RNAMSM_RSA_MAX_MODELS);
    RNAMSM_CHECK_ARG(emb_row_stride >= RSA_EMB, "%s: embedding row stride %lld < %d", who, (long long)emb_row_stride, RSA_EMB);
    const size_t need = (size_t)n_models * rsa_model_floats<TR>(L) * sizeof(float);
    RNAMSM_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    RNAMSM_CHECK_ARG(aligned16(emb), "%s: emb is not 16-byte aligned", who);
    RNAMSM_CHECK_ARG(aligned16(workspace), "%s: workspace is not 16-byte aligned", who);
    RNAMSM_CHECK_ARG((reinterpret_cast<uintptr_t>(probs) & 3u) == 0, "%s: probs is not 4-byte aligned", who);
    RNAMSM_CHECK_ARG((reinterpret_cast<uintptr_t>(logits) & 3u) == 0, "%s: logits is not 4-byte aligned", who);
    if (int rc = rsa_check_weights(who, weights, n_models, use_onehot)) return rc;
    const RsaMember lone = {emb, emb_row_stride, base_codes, logits, probs, 0, L, 0, {0, 0}};
    return rsa_launch<false, TR>(nullptr, 1, lone, (L + RSA_TILE - 1) / RSA_TILE, n_models, use_onehot, weights,
                                 static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int rnamsm_rsa_head(const float* emb, int64_t emb_row_stride, const uint8_t* base_codes, int L, int n_models,
                               int use_onehot, const void* const* weights, float* probs, float* logits, void* workspace,
                               size_t workspace_bytes, void* stream) {
    return rsa_head_lone<RSA_MAX_TILES>("rsa_head", RNAMSM_RSA_MAX_L, emb, emb_row_stride, base_codes, L, n_models, use_onehot, weights,
                                        probs, logits, workspace, workspace_bytes, stream);
}

extern "C" size_t rnamsm_rsa_head_long_workspace_bytes(int L, int n_models) {
    if (L < 1 || L > RNAMSM_LONG_MAX_L || n_models < 1 || n_models > RNAMSM_RSA_MAX_MODELS) return 0;
    return (size_t)n_models * rsa_model_floats<RSA_LONG_TILES>(L) * sizeof(float);
}

extern "C" int rnamsm_rsa_head_long(const float* emb, int64_t emb_row_stride, const uint8_t* base_codes, int L, int n_models,
                                    int use_onehot, const void* const* weights, float* probs, float* logits, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    return rsa_head_lone<RSA_LONG_TILES>("rsa_head_long", RNAMSM_LONG_MAX_L, emb, emb_row_stride, base_codes, L, n_models, use_onehot,
                                         weights, probs, logits, workspace, workspace_bytes, stream);
}

extern "C" size_t rnamsm_rsa_head_packed_workspace_bytes(int B, const int* Ls, int n_models) {
    if (B < 1 || B > RNAMSM_RSA_MAX_BATCH || !Ls || n_models < 1 || n_models > RNAMSM_RSA_MAX_MODELS) return 0;
    size_t floats = 0;
    for (int b = 0; b < B; ++b) {
        if (Ls[b] < 1 || Ls[b] > RNAMSM_RSA_MAX_L) return 0;
        floats += (size_t)n_models * rsa_model_floats(Ls[b]);
    }
    return rsa_members_bytes(B) + floats * sizeof(float);
}

extern "C" int rnamsm_rsa_head_packed(const rnamsm_rsa_item* items, int B, int n_models, int use_onehot, const void* const* weights,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    // every refusal comes before the first launch: a refused call leaves the stream and the outputs untouched
    RNAMSM_CHECK_ARG(items && weights && workspace, "rsa_head_packed: null pointer");
    RNAMSM_CHECK_ARG(B >= 1 && B <= RNAMSM_RSA_MAX_BATCH, "rsa_head_packed: B=%d outside [1, %d]", B, RNAMSM_RSA_MAX_BATCH);
    RNAMSM_CHECK_ARG(n_models >= 1 && n_models <= RNAMSM_RSA_MAX_MODELS, "rsa_head_packed: n_models=%d outside [1, %d]", n_models,
                     RNAMSM_RSA_MAX_MODELS);
    size_t floats = 0;
    int64_t tiles_total = 0;
    for (int b = 0; b < B; ++b) {
        const rnamsm_rsa_item& it = items[b];
        RNAMSM_CHECK_ARG(it.L >= 1 && it.L <= RNAMSM_RSA_MAX_L, "rsa_head_packed: member %d: L=%d outside [1, %d]", b, it.L,
                         RNAMSM_RSA_MAX_L);
        RNAMSM_CHECK_ARG(it.emb && it.base_codes, "rsa_head_packed: member %d: null pointer", b);
        RNAMSM_CHECK_ARG(it.logits || it.probs, "rsa_head_packed: member %d: neither probs nor logits given", b);
        RNAMSM_CHECK_ARG(it.emb_row_stride >= RSA_EMB, "rsa_head_packed: member %d: embedding row stride %lld < %d", b,
                         (long long)it.emb_row_stride, RSA_EMB);
        RNAMSM_CHECK_ARG(aligned16(it.emb), "rsa_head_packed: member %d: the embedding is not 16-byte aligned", b);
        RNAMSM_CHECK_ARG(((uintptr_t)it.logits & 3u) == 0 && ((uintptr_t)it.probs & 3u) == 0,
                         "rsa_head_packed: member %d: an output pointer is not 4-byte aligned", b);
        floats += (size_t)n_models * rsa_model_floats(it.L);
        tiles_total += (it.L + RSA_TILE - 1) / RSA_TILE;
    }
    RNAMSM_CHECK_ARG(aligned16(workspace), "rsa_head_packed: 16-byte alignment of the workspace");
    RNAMSM_CHECK_ARG(workspace_bytes >= rsa_members_bytes(B) + floats * sizeof(float), "rsa_head_packed: workspace too small");
    if (int rc = rsa_check_weights("rsa_head_packed", weights, n_models, use_onehot)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    RsaMember* mem = static_cast<RsaMember*>(workspace);
    int64_t ws_off = 0;
    int32_t tile0 = 0;
    const int rc = upload_members(mem, B, [&](int b) {
        const rnamsm_rsa_item& it = items[b];
        const RsaMember m = {it.emb, it.emb_row_stride, it.base_codes, it.logits, it.probs, ws_off, it.L, tile0, {0, 0}};
        ws_off += (int64_t)n_models * (int64_t)rsa_model_floats(it.L);
        tile0 += (it.L + RSA_TILE - 1) / RSA_TILE;
        return m;
    }, s, "rsa_members");
    if (rc != RNAMSM_OK) return rc;
    return rsa_launch<true, RSA_MAX_TILES>(mem, B, RsaMember{}, tiles_total, n_models, use_onehot, weights,
                                           reinterpret_cast<float*>(static_cast<char*>(workspace) + rsa_members_bytes(B)), s);
}
