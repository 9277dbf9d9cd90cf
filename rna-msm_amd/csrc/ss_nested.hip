// RNA-MSM-SS: the nested structure of greatest summed pair probability on the device (ss_nested.h: the contract, the tile working
// set and the cell logic; include/rnamsm.h: the C ABI).  Nothing of size L^2 reaches the host.
// The fill: one launch per tile-diagonal, ceil(L / 64) in all; block (x, y) = tile (x, x + d) of member y of the chunk, so a packed
// call costs the launches of its largest member.  256 threads:
//   outer phase   k-tiles strictly between I and J: a max-plus 64 x 64 x 64 product per k-tile on the VALU, panels staged in LDS,
//                 thread (ty, tx) holds the 4 x 4 cells (ty + 16 a, tx + 16 b) -- rows a bank apart, columns a bank apart: every LDS
//                 read of the loop is conflict-free -- and folds two k per v_max3_i32
//   inner phase   127 anti-diagonal steps in LDS, four threads per cell sharing its walk over k, one barrier per step
// The traceback: one workgroup of 1024 threads per member, an explicit stack in LDS, at most L + 1 intervals, each resolved by two
// block-wide reductions; then the partner vector and the dot-bracket line, and the tail every decoder shares for the .ct / .bpseq
// bodies (struct_text.h: emit_struct_text, over threads that own ceil(L / 1024) consecutive bases each, their partners in LDS).
// No atomics anywhere: the same bytes on every run.
// The lone entry point and the packed one run the same kernels: the descriptors travel as kernel arguments, 32 per launch
// (common.h: MemberChunk, member_chunk).
#include "common.h"
#include "ss_nested.h"

namespace rnamsm {
namespace {

static_assert(ssnested::MAX_L == RNAMSM_LONG_MAX_L, "one limit");
static_assert(ssnested::MAX_LOOP == RNAMSM_SS_NESTED_MAX_LOOP, "one limit");
using ssnested::TILE;
using ssnested::TileMem;
constexpr int FILL_THREADS = 256, TRACE_THREADS = 1024, TRACE_WAVES = TRACE_THREADS / 64;

struct NestedMember {
    const float* probs;      // [L, L]
    const uint8_t* letters;  // [L]
    int32_t* N;              // [Lp, Lp] inside the workspace; M follows it
    int32_t* partner;        // [L]
    int32_t* counts;         // [5]
    uint8_t* ct;             // [32 L]
    uint8_t* bpseq;          // [12 L]
    uint8_t* dbn;            // [L]
    int32_t L, pad_;
};

__global__ __launch_bounds__(FILL_THREADS) void ss_nested_fill_kernel(const MemberChunk<NestedMember> chunk, int d,
                                                                      ssnested::Params q) {
    __shared__ TileMem mem;
    const NestedMember mb = chunk.m[blockIdx.y];
    const int L = mb.L, T = ssnested::tiles(L), Lp = T * TILE;
    const int I = blockIdx.x, J = I + d;
    if (J >= T) return;                                      // block-uniform: a shorter member of the chunk
    const int32_t* __restrict__ N = mb.N;
    const int32_t* __restrict__ M = mb.N + (size_t)Lp * Lp;
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;

    int32_t acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0;
    // the panels of one k-tile lie where the inner phase will keep X and Mc
    int32_t* const pa = mem.X;                               // pa[r][kk] = A(64 I + r, 64 K + kk) = N(64 I + r, 64 K + kk - 1)
    int32_t* const pb = mem.Mc;                              // pb[kk][c] = M(64 K + kk, 64 J + c)
    for (int K = I + 1; K < J; ++K) {
        for (int e = t; e < TILE * TILE; e += FILL_THREADS) {
            const int r = e >> 6, c = e & 63;
            pa[r * ssnested::LD + c] = N[(size_t)(TILE * I + r) * Lp + TILE * K + c - 1];
            pb[r * ssnested::LD + c] = M[(size_t)(TILE * K + r) * Lp + TILE * J + c];
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < TILE; kk += 2) {
            int32_t a0[4], a1[4], b0[4], b1[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                a0[a] = pa[(ty + 16 * a) * ssnested::LD + kk];
                a1[a] = pa[(ty + 16 * a) * ssnested::LD + kk + 1];
                b0[a] = pb[kk * ssnested::LD + tx + 16 * a];
                b1[a] = pb[(kk + 1) * ssnested::LD + tx + 16 * a];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = max(max(acc[a][b], a0[a] + b0[b]), a1[a] + b1[b]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) ssnested::nh(mem, ty + 16 * a, tx + 16 * b) = acc[a][b];
    for (int e = t; e < (TILE + 1) * (TILE + 1); e += FILL_THREADS) ssnested::stage_inner(mem, mb.probs, L, N, M, Lp, I, J, q, e);
    __syncthreads();

    const bool diag = d == 0;
    const int r = t >> 2, part = t & 3;
    for (int s = diag ? TILE - 1 : 0; s < 2 * TILE - 1; ++s) {
        const int c = s - (TILE - 1) + r;
        const bool on = c >= 0 && c < TILE;                  // the same in the four threads of a cell
        int32_t over_k = ssnested::NEG;
        if (on) over_k = ssnested::cell_part(mem, r, c, diag, q.min_loop, part, 4);      // reads cells of earlier steps only
        over_k = max(over_k, __shfl_xor(over_k, 1, 64));
        over_k = max(over_k, __shfl_xor(over_k, 2, 64));
        // one thread of the four reads the cell's w(i, j) and writes its M and N
        if (on && part == 0) ssnested::cell_store(mem, r, c, ssnested::cell_m(mem, r, c), over_k);
        __syncthreads();
    }

    int32_t* const No = mb.N;
    int32_t* const Mo = mb.N + (size_t)Lp * Lp;
    for (int e = t; e < TILE * TILE; e += FILL_THREADS) {
        const int rr = e >> 6, cc = e & 63;
        const size_t at = (size_t)(TILE * I + rr) * Lp + TILE * J + cc;
        No[at] = ssnested::nh(mem, rr, cc);
        Mo[at] = mem.Mc[rr * ssnested::LD + cc];
    }
}

// the greatest (Max) or the least value of the block; red: TRACE_WAVES words, free again on return
template <bool Max>
__device__ __forceinline__ int block_extreme(int v, int* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(v, off, 64);
        v = Max ? max(v, o) : min(v, o);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = red[0];
#pragma unroll
    for (int w = 1; w < TRACE_WAVES; ++w) r = Max ? max(r, red[w]) : min(r, red[w]);
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(TRACE_THREADS) void ss_nested_trace_kernel(const MemberChunk<NestedMember> chunk, int min_loop) {
    __shared__ int32_t partner[ssnested::MAX_L];
    __shared__ int32_t stack[ssnested::MAX_L + 4];           // (i, j) pairs: never more than L / 2 + 1 intervals wait
    __shared__ int red[TRACE_WAVES];
    __shared__ uint64_t scan[TRACE_WAVES];
    const NestedMember mb = chunk.m[blockIdx.x];
    const int L = mb.L, Lp = ssnested::padded(L);
    const int32_t* __restrict__ N = mb.N;
    const int32_t* __restrict__ M = mb.N + (size_t)Lp * Lp;
    const int t = threadIdx.x;

    for (int b = t; b < L; b += TRACE_THREADS) partner[b] = 0;
    if (t == 0) {
        stack[0] = 0;
        stack[1] = L - 1;
    }
    __syncthreads();
    int sp = L > 1 ? 1 : 0;                                  // block-uniform, as is everything that steers the loop
    bool failed = false;
    for (int step = 0; sp > 0 && step < 2 * L + 2; ++step) {
        --sp;
        const int i = stack[2 * sp], j = stack[2 * sp + 1];
        const int c = block_extreme<true>(ssnested::trace_paired_column(N, Lp, i, j, t, TRACE_THREADS), red);
        if (c < 0) continue;                                 // block_extreme's barriers keep the stack reads above ahead of any push
        const int k = block_extreme<false>(ssnested::trace_partner(N, M, Lp, i, c, min_loop, t, TRACE_THREADS), red);
        if (k == INT32_MAX) {                                // cannot happen on a table the fill wrote: the structure would be partial
            failed = true;
            break;
        }
        if (t == 0) {
            partner[k] = c + 1;
            partner[c] = k + 1;
        }
        int top = sp;
        if (k - 1 > i) {
            if (t == 0) {
                stack[2 * top] = i;
                stack[2 * top + 1] = k - 1;
            }
            ++top;
        }
        if (c - 1 > k + 1) {
            if (t == 0) {
                stack[2 * top] = k + 1;
                stack[2 * top + 1] = c - 1;
            }
            ++top;
        }
        sp = top;
        __syncthreads();
    }
    __syncthreads();

    const int b0 = sspairs::first_base(t, L, TRACE_THREADS), b1 = sspairs::end_base(t, L, TRACE_THREADS);
    for (int b = b0; b < b1; ++b) {
        const int p = partner[b];
        mb.partner[b] = p;
        mb.dbn[b] = ssnested::dbn_char(b, p);
    }
    emit_struct_text(L, b0, b1, [&](int b) { return partner[b]; }, mb.letters, mb.ct, mb.bpseq, mb.counts, scan);
    if (t == 0)
        mb.counts[4] = (failed || sp > 0) ? -1 : N[L - 1];   // -1: the traceback did not end (an inconsistent table); never a valid score
}

size_t tables_bytes(int L) {
    const size_t Lp = (size_t)ssnested::padded(L);
    return 2 * Lp * Lp * sizeof(int32_t);                    // a multiple of 32 KB
}

// Every refusal, then the launches.  who: the entry point's name; lone: the one item is the call's own arguments, not "member 0".
// phases: bit 0 = the fill, bit 1 = the traceback (on tables a fill has written).
int ss_nested_run(const char* who, bool lone, const rnamsm_ss_nested_item* items, int B, float theta, int min_loop, void* workspace,
                  size_t workspace_bytes, hipStream_t s, int phases = 3) {
    RNAMSM_CHECK_ARG(theta >= 0.f && theta < 1.f, "%s: theta=%g outside [0, 1)", who, (double)theta);          // NaN fails both
    RNAMSM_CHECK_ARG(min_loop >= 0 && min_loop <= RNAMSM_SS_NESTED_MAX_LOOP, "%s: min_loop=%d outside [0, %d]", who, min_loop,
                     RNAMSM_SS_NESTED_MAX_LOOP);
    char where[32] = "";
    size_t need = 0;
    for (int b = 0; b < B; ++b) {
        const rnamsm_ss_nested_item& it = items[b];
        if (!lone) snprintf(where, sizeof(where), "member %d: ", b);
        const rnamsm_ss_pairs_item six = {it.probs, it.letters, it.L, it.partner, it.counts, it.ct, it.bpseq};
        if (int rc = check_struct_item(who, where, RNAMSM_LONG_MAX_L, six, &it.dbn)) return rc;
        need += tables_bytes(it.L);
    }
    if (int rc = check_struct_workspace(who, workspace, workspace_bytes, need)) return rc;
    const ssnested::Params q = ssnested::params(theta, min_loop);
    size_t off = 0;
    for (int b0 = 0; b0 < B; b0 += 32) {
        int n, max_T = 1;
        auto fill = [&](int b) {
            const rnamsm_ss_nested_item& it = items[b];
            NestedMember m = {it.probs, it.letters, reinterpret_cast<int32_t*>(static_cast<uint8_t*>(workspace) + off),
                              it.partner, it.counts, it.ct, it.bpseq, it.dbn, it.L, 0};
            off += tables_bytes(it.L);
            if (ssnested::tiles(it.L) > max_T) max_T = ssnested::tiles(it.L);
            return m;
        };
        const MemberChunk<NestedMember> chunk = member_chunk<NestedMember>(b0, B, fill, n);
        for (int d = 0; d < max_T && (phases & 1); ++d) {
            hipLaunchKernelGGL(ss_nested_fill_kernel, dim3((unsigned)(max_T - d), (unsigned)n), dim3(FILL_THREADS), 0, s, chunk, d, q);
            RNAMSM_CHECK_LAUNCH("ss_nested_fill");
        }
        if (phases & 2) {
            hipLaunchKernelGGL(ss_nested_trace_kernel, dim3((unsigned)n), dim3(TRACE_THREADS), 0, s, chunk, min_loop);
            RNAMSM_CHECK_LAUNCH("ss_nested_trace");
        }
    }
    return RNAMSM_OK;
}

}  // namespace
}  // namespace rnamsm

using namespace rnamsm;

extern "C" size_t rnamsm_ss_nested_workspace_bytes(int B, const int* Ls) {
    if (B < 1 || B > RNAMSM_SS_MAX_BATCH || !Ls) return 0;
    size_t n = 0;
    for (int b = 0; b < B; ++b) {
        if (Ls[b] < 1 || Ls[b] > RNAMSM_LONG_MAX_L) return 0;
        n += tables_bytes(Ls[b]);
    }
    return n;
}

extern "C" int rnamsm_ss_nested(const float* probs, const uint8_t* letters, int L, float theta, int min_loop, int32_t* partner,
                                int32_t* counts, uint8_t* ct, uint8_t* bpseq, uint8_t* dbn, void* workspace, size_t workspace_bytes,
                                void* stream) {
    const rnamsm_ss_nested_item item = {probs, letters, L, partner, counts, ct, bpseq, dbn};
    return ss_nested_run("ss_nested", true, &item, 1, theta, min_loop, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int rnamsm_ss_nested_packed(const rnamsm_ss_nested_item* items, int B, float theta, int min_loop, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    // every refusal comes before the first launch: a refused call leaves the stream and the outputs untouched
    RNAMSM_CHECK_ARG(items, "ss_nested_packed: null pointer");
    RNAMSM_CHECK_ARG(B >= 1 && B <= RNAMSM_SS_MAX_BATCH, "ss_nested_packed: B=%d outside [1, %d]", B, RNAMSM_SS_MAX_BATCH);
    return ss_nested_run("ss_nested_packed", false, items, B, theta, min_loop, workspace, workspace_bytes,
                         static_cast<hipStream_t>(stream));
}

extern "C" int rnamsm_ss_nested_phases(const rnamsm_ss_nested_item* items, int B, float theta, int min_loop, void* workspace,
                                       size_t workspace_bytes, int phases, void* stream) {
    RNAMSM_CHECK_ARG(items, "ss_nested_phases: null pointer");
    RNAMSM_CHECK_ARG(B >= 1 && B <= RNAMSM_SS_MAX_BATCH, "ss_nested_phases: B=%d outside [1, %d]", B, RNAMSM_SS_MAX_BATCH);
    RNAMSM_CHECK_ARG(phases >= 1 && phases <= 3, "ss_nested_phases: phases=%d outside [1, 3]", phases);
    return ss_nested_run("ss_nested_phases", false, items, B, theta, min_loop, workspace, workspace_bytes,
                         static_cast<hipStream_t>(stream), phases);
}
