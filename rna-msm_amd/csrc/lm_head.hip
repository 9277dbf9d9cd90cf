// f4: the LM head on chosen rows of a feature buffer (RobertaLMHead.forward, modules.py:303-319; the log-softmax and the wild-type
// subtraction of utils/likelihood.py:86-120).  For row i of a member, x_i = x + (rows ? rows[i] : i) * ld:
//   h      = gelu_erf(x_i . Wd^T + bd)
//   y      = LayerNorm(h; gamma, beta, eps)
//   logits = y . Wp^T + bp                  Wp [V, D], the tied embed_tokens rows as they are
//   logp   = (logits - max) - log(sum exp(logits - max))
//   scores = logp - logp[wt_i],  nll = -logp[wt_i]
// Two launches:
//   lm_dense   block = (32-row tile, 64-column tile), two waves, each one 32 x 32 tile of v_mfma_f32_32x32x2_f32 over the whole of
//              k.  The operands come straight from global memory -- lane (li, lh) reads x_i[8kk + 4lh .. + 3] of ITS row and the same
//              four k of ITS row of Wd as one 16-byte load each -- so the gather costs nothing and no row but the selected ones is
//              touched.  n = 1023 at D = 768 is 32 x 12 = 384 blocks; the step is launch- and latency-bound at these sizes (1.2 GFLOP
//              at n = 1023), LDS staging would save L1 hits, not time.
//   lm_rows    one wave per row: LayerNorm of h (common.h's ln_row_stats / ln_value), V dot products, log-softmax, scores, nll.
// The bits of a row: every output element of lm_dense is the same sum whatever tile, lane or block holds it -- k in blocks of 32,
// a block one accumulator chain over k = (8kk + s, 8kk + 4 + s), s = 0..3, kk ascending, the block sums added in ascending order
// -- and an MFMA row reads nothing of another row; lm_rows is a wave to itself with
// fixed butterflies.  So a row's result depends on its D values and the weights only -- not on n, its place, its neighbours or the
// members beside it -- and the packed call has the lone call's bits.  No atomics.
// One kernel per stage serves the lone and the packed call (as contact_head.hip): packed, a block finds its member by member_of over
// the prefix sums of the 32-row tiles; lone, the member is the kernel argument.
#include "common.h"

namespace rnamsm {
namespace {

constexpr int LM_TM = 32;                 // rows of a tile (one MFMA tile)
constexpr int LM_TN = 64;                 // columns of a dense block: two waves x 32
constexpr int LM_ROW_BLOCKS = LM_TM / 4;  // lm_rows blocks per tile: four waves = four rows each

// A member's descriptor is two 64-byte records (upload_members moves 64-byte records): what both kernels read, what lm_rows writes.
struct LmIn {
    const float* x;
    const int32_t* rows;     // or null
    const int32_t* wt;       // or null
    int64_t ld;
    int32_t n;
    int32_t tile0;           // 32-row tiles of the members before it (a member's share: ceil(n / 32))
    int32_t row0;            // rows of the members before it: its slab of h starts at float row0 * D of the workspace
    int32_t pad_[5];
};
struct LmOut {
    float* logits;
    float* logp;
    float* scores;
    float* nll;
    int64_t pad_[4];
};
static_assert(sizeof(LmIn) == 64 && sizeof(LmOut) == 64, "LM head descriptor layout");

// ---------------------------------------------------------------------------------------------------------------- launch 1
// h[i, c] = gelu_erf(sum_k x_i[k] Wd[c, k] + bd[c]).  Block id = tile * (D / 64) + column tile.  A tile's rows past n repeat its
// first row (always a selected one) as operands and are not stored.
template <bool PACKED>
__global__ __launch_bounds__(128) void lm_dense_kernel(const LmIn* __restrict__ mem, int B, const LmIn lone, const float* __restrict__ Wd,
                                                       const float* __restrict__ bd, float* __restrict__ ws, int D) {
    const int nct = D / LM_TN;
    const int tile = (int)(blockIdx.x / (unsigned)nct), ct = (int)(blockIdx.x % (unsigned)nct);
    const LmIn m = PACKED ? mem[member_of(mem, B, tile, &LmIn::tile0)] : lone;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
    const int r0 = (tile - m.tile0) * LM_TM;
    const int col = ct * LM_TN + wave * 32 + li;
    int r = r0 + li;
    if (r >= m.n) r = r0;
    const int64_t src = m.rows ? (int64_t)m.rows[r] : (int64_t)r;
    const float* xa = m.x + src * m.ld + 4 * lh;
    const float* wb = Wd + (int64_t)col * D + 4 * lh;
    f32x16 acc;
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = 0.f;
    // 64 k per step (D % 64 == 0): the sixteen loads of step t + 1 are in flight behind the 32 MFMAs of step t
    f32x4 a[8], b[8], an[8], bn[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        a[j] = *reinterpret_cast<const f32x4*>(xa + 8 * j);
        b[j] = *reinterpret_cast<const f32x4*>(wb + 8 * j);
    }
    for (int k = 0; k < D; k += 64) {
        const int kn = k + 64 < D ? k + 64 : k;                   // the last step reloads itself: no read past the row
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            an[j] = *reinterpret_cast<const f32x4*>(xa + kn + 8 * j);
            bn[j] = *reinterpret_cast<const f32x4*>(wb + kn + 8 * j);
        }
        // two blocks of 32 k, each a chain of its own from zero, then added to the running sum in ascending order: the rounding
        // error of a 768-term sum grows with the length of its chains, and blocks of about sqrt(K) keep it at a quarter of one
        // chain's -- what a blocked host GEMM has, and what the tests' fp32 yardstick is
        f32x16 p0, p1;
#pragma unroll
        for (int t = 0; t < 16; ++t) p0[t] = p1[t] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                p0 = mfma32(a[j][s], b[j][s], p0);
                p1 = mfma32(a[j + 4][s], b[j + 4][s], p1);
            }
        acc = (acc + p0) + p1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            a[j] = an[j];
            b[j] = bn[j];
        }
    }
    const float bias = bd[col];
    float* h = ws + (int64_t)m.row0 * D;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int row = r0 + (t & 3) + 8 * (t >> 2) + 4 * lh;
        if (row < m.n) h[(int64_t)row * D + col] = gelu_erf(acc[t] + bias);
    }
}

// ---------------------------------------------------------------------------------------------------------------- launch 2
// One wave per row; block id = tile * 8 + (four rows of the tile).  Lane v < V ends up with logit v of the row.
template <bool PACKED>
__global__ __launch_bounds__(256) void lm_rows_kernel(const LmIn* __restrict__ mem, const LmOut* __restrict__ outs, int B, const LmIn lone,
                                                      const LmOut lone_out, const float* __restrict__ ws, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float* __restrict__ Wp,
                                                      const float* __restrict__ bp, int D, int V, float eps) {
    const int tile = (int)(blockIdx.x / (unsigned)LM_ROW_BLOCKS);
    const int b = PACKED ? member_of(mem, B, tile, &LmIn::tile0) : 0;
    const LmIn m = PACKED ? mem[b] : lone;
    const LmOut o = PACKED ? outs[b] : lone_out;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = (tile - m.tile0) * LM_TM + (int)(blockIdx.x % (unsigned)LM_ROW_BLOCKS) * 4 + wave;
    if (i >= m.n) return;                                         // wave-uniform
    const int nvec = D >> 2;
    const f32x4* h = reinterpret_cast<const f32x4*>(ws + ((int64_t)m.row0 + i) * D);
    f32x4 y[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (lane + 64 * e < nvec) y[e] = h[lane + 64 * e];
        else y[e] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const LnStats st = ln_row_stats(y, nvec, lane, D, eps);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (lane + 64 * e < nvec) {
            const f32x4 g = reinterpret_cast<const f32x4*>(gamma)[lane + 64 * e];
            const f32x4 bb = reinterpret_cast<const f32x4*>(beta)[lane + 64 * e];
#pragma unroll
            for (int c = 0; c < 4; ++c) y[e][c] = ln_value(y[e][c], st, g[c], bb[c]);
        }
    float mine = 0.f;
    for (int v = 0; v < V; ++v) {
        const f32x4* w = reinterpret_cast<const f32x4*>(Wp + (int64_t)v * D);
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (lane + 64 * e < nvec) {
                const f32x4 ww = w[lane + 64 * e];
#pragma unroll
                for (int c = 0; c < 4; ++c) s = fmaf(y[e][c], ww[c], s);
            }
        s = wave_sum(s) + bp[v];
        if (lane == v) mine = s;
    }
    const bool live = lane < V;
    if (o.logits && live) o.logits[(int64_t)i * V + lane] = mine;
    if (!o.logp && !o.scores && !o.nll) return;
    const float mx = wave_max(live ? mine : -INFINITY);
    const float sum = wave_sum(live ? expf(mine - mx) : 0.f);
    const float lp = (mine - mx) - logf(sum);
    if (o.logp && live) o.logp[(int64_t)i * V + lane] = lp;
    if (!o.scores && !o.nll) return;
    // the wild type: a lane of this wave, never an address.  Outside [0, V) the row's scores and nll are NaN.
    const int w = m.wt[i];
    const bool ok = w >= 0 && w < V;
    float ref = __shfl(lp, ok ? w : 0, 64);
    if (!ok) ref = __builtin_nanf("");
    if (o.scores && live) o.scores[(int64_t)i * V + lane] = lp - ref;
    if (o.nll && lane == 0) o.nll[i] = -ref;
}

constexpr size_t lm_members_bytes(int B) { return ((size_t)B * 64 + 255) & ~(size_t)255; }
inline int lm_tiles(int n) { return (n + LM_TM - 1) / LM_TM; }
inline bool lm_dims_ok(int D, int V) { return D >= 64 && D <= RNAMSM_LM_MAX_D && D % 64 == 0 && V >= 1 && V <= RNAMSM_LM_MAX_V; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// The checks of one member; who = "lm_head" or "lm_head_packed: member 3".
int lm_check_item(const char* who, const rnamsm_lm_item& it, int D) {
    RNAMSM_CHECK_ARG(it.x, "%s: null pointer (x)", who);
    RNAMSM_CHECK_ARG(it.n >= 1, "%s: n=%d < 1", who, it.n);
    RNAMSM_CHECK_ARG(it.n <= RNAMSM_LM_MAX_ROWS, "%s: n=%d above %d rows per call", who, it.n, RNAMSM_LM_MAX_ROWS);
    RNAMSM_CHECK_ARG(it.ld >= D, "%s: ld=%lld < D=%d", who, (long long)it.ld, D);
    RNAMSM_CHECK_ARG(aligned16(it.x) && it.ld % 4 == 0, "%s: x is not 16-byte aligned or ld=%lld is no multiple of 4", who,
                     (long long)it.ld);
    RNAMSM_CHECK_ARG(it.logits || it.logp || it.scores || it.nll, "%s: every output is null", who);
    RNAMSM_CHECK_ARG(it.wt || (!it.scores && !it.nll), "%s: scores / nll asked without wt", who);
    RNAMSM_CHECK_ARG(aligned4(it.rows) && aligned4(it.wt) && aligned4(it.logits) && aligned4(it.logp) && aligned4(it.scores) &&
                         aligned4(it.nll), "%s: a pointer is not 4-byte aligned", who);
    return RNAMSM_OK;
}

template <bool PACKED>
int lm_launch(const LmIn* mem, const LmOut* outs, int B, const LmIn& lone, const LmOut& lone_out, int64_t tiles, int D, int V,
              const float* const* w, float eps, float* ws, hipStream_t s) {
    hipLaunchKernelGGL(lm_dense_kernel<PACKED>, dim3((unsigned)(tiles * (D / LM_TN))), dim3(128), 0, s, mem, B, lone, w[0], w[1], ws, D);
    RNAMSM_CHECK_LAUNCH(PACKED ? "lm_dense (packed)" : "lm_dense");
    hipLaunchKernelGGL(lm_rows_kernel<PACKED>, dim3((unsigned)(tiles * LM_ROW_BLOCKS)), dim3(256), 0, s, mem, outs, B, lone, lone_out,
                       (const float*)ws, w[2], w[3], w[4], w[5], D, V, eps);
    RNAMSM_CHECK_LAUNCH(PACKED ? "lm_rows (packed)" : "lm_rows");
    return RNAMSM_OK;
}

}  // namespace
}  // namespace rnamsm

using namespace rnamsm;

extern "C" size_t rnamsm_lm_head_workspace_bytes(int n, int D) {
    if (n < 1 || n > RNAMSM_LM_MAX_ROWS || !lm_dims_ok(D, 1)) return 0;
    return (size_t)n * D * sizeof(float);
}

extern "C" int rnamsm_lm_head(const rnamsm_lm_item* item, int D, int V, const float* const* weights, float eps, void* workspace,
                              size_t workspace_bytes, void* stream) {
    RNAMSM_CHECK_ARG(item && weights && workspace, "lm_head: null pointer");
    RNAMSM_CHECK_ARG(lm_dims_ok(D, V), "lm_head: D=%d (a multiple of 64 in [64, %d]) V=%d (in [1, %d])", D, RNAMSM_LM_MAX_D, V,
                     RNAMSM_LM_MAX_V);
    int rc = check_weight_table("lm_head", weights, RNAMSM_LM_NUM_WEIGHTS);
    if (rc != RNAMSM_OK) return rc;
    rc = lm_check_item("lm_head", *item, D);
    if (rc != RNAMSM_OK) return rc;
    RNAMSM_CHECK_ARG(aligned16(workspace), "lm_head: 16-byte alignment of the workspace");
    RNAMSM_CHECK_ARG(workspace_bytes >= (size_t)item->n * D * sizeof(float), "lm_head: workspace too small");
    const LmIn lone = {item->x, item->rows, item->wt, item->ld, item->n, 0, 0, {0, 0, 0, 0, 0}};
    const LmOut lone_out = {item->logits, item->logp, item->scores, item->nll, {0, 0, 0, 0}};
    return lm_launch<false>(nullptr, nullptr, 1, lone, lone_out, lm_tiles(item->n), D, V, weights, eps, static_cast<float*>(workspace),
                            static_cast<hipStream_t>(stream));
}

extern "C" size_t rnamsm_lm_head_packed_workspace_bytes(int B, const int* ns, int D) {
    if (B < 1 || B > RNAMSM_LM_MAX_BATCH || !ns || !lm_dims_ok(D, 1)) return 0;
    int64_t rows = 0;
    for (int b = 0; b < B; ++b) {
        if (ns[b] < 1 || ns[b] > RNAMSM_LM_MAX_ROWS) return 0;
        rows += ns[b];
    }
    if (rows > RNAMSM_LM_MAX_ROWS) return 0;
    return 2 * lm_members_bytes(B) + (size_t)rows * D * sizeof(float);
}

extern "C" int rnamsm_lm_head_packed(const rnamsm_lm_item* items, int B, int D, int V, const float* const* weights, float eps,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    // every refusal comes before the first launch: a refused call leaves the stream and the outputs untouched
    RNAMSM_CHECK_ARG(items && weights && workspace, "lm_head_packed: null pointer");
    RNAMSM_CHECK_ARG(B >= 1 && B <= RNAMSM_LM_MAX_BATCH, "lm_head_packed: B=%d outside [1, %d]", B, RNAMSM_LM_MAX_BATCH);
    RNAMSM_CHECK_ARG(lm_dims_ok(D, V), "lm_head_packed: D=%d (a multiple of 64 in [64, %d]) V=%d (in [1, %d])", D, RNAMSM_LM_MAX_D, V,
                     RNAMSM_LM_MAX_V);
    int rc = check_weight_table("lm_head_packed", weights, RNAMSM_LM_NUM_WEIGHTS);
    if (rc != RNAMSM_OK) return rc;
    int64_t rows = 0, tiles = 0;
    for (int b = 0; b < B; ++b) {
        char who[48];
        snprintf(who, sizeof(who), "lm_head_packed: member %d", b);
        rc = lm_check_item(who, items[b], D);
        if (rc != RNAMSM_OK) return rc;
        rows += items[b].n;
        tiles += lm_tiles(items[b].n);
        RNAMSM_CHECK_ARG(rows <= RNAMSM_LM_MAX_ROWS, "lm_head_packed: member %d: the rows of the call exceed %d", b, RNAMSM_LM_MAX_ROWS);
    }
    RNAMSM_CHECK_ARG(aligned16(workspace), "lm_head_packed: 16-byte alignment of the workspace");
    RNAMSM_CHECK_ARG(workspace_bytes >= 2 * lm_members_bytes(B) + (size_t)rows * D * sizeof(float), "lm_head_packed: workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    LmIn* mem = static_cast<LmIn*>(workspace);
    LmOut* outs = reinterpret_cast<LmOut*>(static_cast<char*>(workspace) + lm_members_bytes(B));
    int32_t tile0 = 0, row0 = 0;
    rc = upload_members(mem, B, [&](int b) {
        const rnamsm_lm_item& it = items[b];
        const LmIn m = {it.x, it.rows, it.wt, it.ld, it.n, tile0, row0, {0, 0, 0, 0, 0}};
        tile0 += lm_tiles(it.n);
        row0 += it.n;
        return m;
    }, s, "lm_members");
    if (rc != RNAMSM_OK) return rc;
    rc = upload_members(outs, B, [&](int b) {
        const rnamsm_lm_item& it = items[b];
        return LmOut{it.logits, it.logp, it.scores, it.nll, {0, 0, 0, 0}};
    }, s, "lm_outputs");
    if (rc != RNAMSM_OK) return rc;
    return lm_launch<true>(mem, outs, B, LmIn{}, LmOut{}, tiles, D, V, weights, eps,
                           reinterpret_cast<float*>(static_cast<char*>(workspace) + 2 * lm_members_bytes(B)), s);
}
