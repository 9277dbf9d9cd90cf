// The two K loops of the 16-bit 256x256 kernels, each written once (the 16-bit counterpart of mma_core.h):
//   swp_kloop16     the software-pipelined two-buffer ring on v_mfma_f32_32x32x16: gemm16_swp_kernel (gemm_bf16.hip) and
//                   row_logits16x_kernel (row_attn16.hip)
//   staged_kloop16  the staged-by-operand loop on v_mfma_f32_16x16x32_bf16: gemm16_q16s_kernel
// row_apply16x_kernel (the ring) and row_logits16q_kernel (the staged loop) run the same loops from their own text: called through
// these functions they took one or two VGPRs more than before (profiles/gemm16_core_code_objects.md).  A change to a loop here
// has to be made there too.
// Both run 8 waves as 2 (M, `wm`) x 4 (N, `wn`) with a 128 x 64 wave tile (128 accumulator VGPRs) over two LDS buffers filled by
// LDS-DMA (dma16, tile16.h).  What a kernel keeps for itself: its DMA map (the `issue` functor), its tile walk, its epilogue.
#pragma once
#include <type_traits>

#include "tile16.h"

namespace rnamsm {

template <class V, int N, int M>
__device__ __forceinline__ void zero_acc16(V (&acc)[N][M]) {
#pragma unroll
    for (int mt = 0; mt < N; ++mt)
#pragma unroll
        for (int nt = 0; nt < M; ++nt) acc[mt][nt] = V(0.f);
}

// Pin "NMF MFMAs with NDS LDS reads between them": one read per MFMA from the start, so the last read has the rest of the run to
// land before the next phase waits for it.  sched_group_barrier acts per basic block: the MFMAs and reads it names must be
// straight-line code between two sched_barriers.
template <int NMF, int NDS>
__device__ __forceinline__ void pin_mfma_ds() {
#pragma unroll
    for (int i = 0; i < (NDS < NMF ? NDS : NMF); ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    if (NMF > NDS) __builtin_amdgcn_sched_group_barrier(0x008, NMF - NDS, 0);
    __builtin_amdgcn_sched_barrier(0);
}

// ---- the software-pipelined ring ------------------------------------------------------------------------------------------
// Geometry of one stage: NPL planes per operand (hi [, lo]) of [256 rows][BK halves], A planes then B planes.  BK = 32 (64-B tile
// rows; the hi/lo modes: four planes per stage) or 64 (128-B rows = whole cache lines per DMA row, twice the bytes in flight,
// half the barriers; one plane per operand only: 2 stages x 64 KB).
template <int SPLIT, int BK>
struct Ring16Cfg {
    static_assert(BK == 32 || (BK == 64 && SPLIT == 1), "64-deep K tiles: two 64 KB stages fit for one plane per operand only");
    static constexpr int NPL = SPLIT == 3 ? 2 : 1;
    static constexpr int ROWB = BK * 2;
    static constexpr int PLANE = 256 * ROWB;
    static constexpr int BUF = 2 * NPL * PLANE;
    static constexpr int RPI = 1024 / ROWB;                 // tile rows per wave DMA instruction
    static constexpr int IPW = 256 / RPI / 8;               // DMA instructions per wave per plane tile
    static constexpr int KS = BK / 16;                      // MFMA k steps per tile
};

// fragments of one k step of a 128 x 64 wave tile: 4 A + 2 B ds_read_b128 per plane
template <int SPLIT, int FMT>
struct Frag16 {
    typename Half16<FMT>::V8 a[SPLIT == 3 ? 2 : 1][4], b[SPLIT == 3 ? 2 : 1][2];
};
// SPLIT 3: small cross terms first, the leading term last
template <int SPLIT, int FMT>
__device__ __forceinline__ void frag16_mma(const Frag16<SPLIT, FMT>& f, f32x16 (&acc)[4][2]) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            if (SPLIT == 3) {
                acc[mt][nt] = Half16<FMT>::mfma(f.a[1][mt], f.b[0][nt], acc[mt][nt]);
                acc[mt][nt] = Half16<FMT>::mfma(f.a[0][mt], f.b[1][nt], acc[mt][nt]);
            }
            acc[mt][nt] = Half16<FMT>::mfma(f.a[0][mt], f.b[0][nt], acc[mt][nt]);
        }
}
// Swizzled 16-B chunk of k step kk for lane (li, lh) of a "k" tile with BK halves per row.  64-B rows: physical chunk = logical ^
// ((row >> 2) & 3); 128-B rows: logical ^ ((row >> 1) & 7) -- either way the 16 rows of a ds_read_b128 lane group hit 16 distinct
// 16-B slots.  Tile rows are multiples of 32 + li, so the row term depends on li alone; the DMA maps apply the same XOR to the source.
template <int BK>
__device__ __forceinline__ int chunk16_k(int kk, int li, int lh) {
    return (BK == 32 ? ((2 * kk + lh) ^ ((li >> 2) & 3)) : ((2 * kk + lh) ^ ((li >> 1) & 7))) * 16;
}
// the same on the DMA side: the logical chunk lane `lane` of wave `wv` fetches (wave instruction = RPI rows, row = RPI g + lane / CPR)
template <int BK>
__device__ __forceinline__ int dma_chunk16_k(int lane, int wv) {
    return BK == 32 ? ((lane & 3) ^ ((lane >> 4) & 3))                      // (row >> 2) & 3
                    : ((lane & 7) ^ ((4 * (wv & 1) + (lane >> 4)) & 7));    // (row >> 1) & 7, row = 8 g + lane / 8
}
template <int SPLIT, int FMT, int BK>
__device__ __forceinline__ void frag16_load_k(const char* buf, int kk, int wm, int wn, int li, int lh, Frag16<SPLIT, FMT>& f) {
    using Cfg = Ring16Cfg<SPLIT, BK>;
    typedef typename Half16<FMT>::V8 V8;
    const int chunk = chunk16_k<BK>(kk, li, lh);
#pragma unroll
    for (int p = 0; p < Cfg::NPL; ++p) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            f.a[p][t] = *reinterpret_cast<const V8*>(buf + p * Cfg::PLANE + (wm * 128 + t * 32 + li) * Cfg::ROWB + chunk);
#pragma unroll
        for (int t = 0; t < 2; ++t)
            f.b[p][t] = *reinterpret_cast<const V8*>(buf + (Cfg::NPL + p) * Cfg::PLANE + (wn * 64 + t * 32 + li) * Cfg::ROWB + chunk);
    }
}

// The ring.  A kernel that reads a k step's fragments and waits for them right before the MFMAs that use them (rounds 1-3:
// gemm16_dma256_kernel, removed in round 4) has its two waves per SIMD barrier-synchronised, so they tend to sit in those waits
// together and the matrix pipe idles (PMC, split 3 QKV: 56% MFMA busy at the actual clock, waves 32% of their time in s_waitcnt).
// Here a k step's fragments are requested while the PREVIOUS step's MFMAs issue (two fragment sets, step kk in f[kk & 1], KS even;
// the interleave pinned: NMF MFMAs, NDS reads per step), also across the tile boundary.
//   THE BARRIER SITS MID-TILE, right after the tile's last fragment read: at that point every wave is done READING buffer `cur`, so
//   the DMA of tile kt+2 can start overwriting it while the last step's MFMAs of tile kt are still issuing, and the first
//   fragments of tile kt+1 (issued one tile ago, landed: the same wait) load under them.
//   THE RELOAD IS CLAMPED, k2 = min(kt + 2, nk - 1): the last reload (and, when nk == 1, the second start-up request) is never
//   read, but keeps the number of requests per tile fixed, so the steady body is branch-free and every wait is a vmcnt(0).  The
//   caller's trailing wait lets it land before LDS is reused or the block exits.
//   DEPHASED ISSUE: a wave is stuck for ~100 cycles per LDS-DMA request it issues (8 per tile); when the two waves of a SIMD issue
//   theirs at the same moment -- right after the barrier -- nobody feeds the matrix pipe meanwhile, so the upper wave group
//   (wm == 1) issues one step later.  (Staging by operand as in staged_kloop16 was built for the GEMM too and measured no better
//   than this delay: f16x3 six GEMMs x1.026 against x1.035, plain bf16 QKV x1.01 and fc1 x0.93; EXPERIMENTS.md R3.3.)
// Measured against the wait-before-use kernel in one process (GEMM, cfg3 shapes): +3..5% for split 3 (QKV 337 -> 356 TF
// algorithmic, matrix pipe 56% -> 60% busy at the ~1.7 GHz the chip sustains here) and +4..10% for split 1.  What remains is not
// fragment latency: a 4-stage DMA pipeline with counted vmcnt (three tiles in flight, BK = 16 for split 3) was also built and
// measured -- split 1 +5..10%, split 3 -7..12% (twice the barriers for the same bytes) -- and dropped.  What-if builds (DESIGN.md
// 3.1b): skipping the B fragment reads gains <= 2% (LDS read bandwidth is not the limiter); skipping the DMA gains 23-45%; a
// DMA-only loop takes 60-75% of the kernel time.  Data movement and MFMA each need most of the time and overlap imperfectly --
// contention of the LDS-DMA path or the power budget, still open.  Split 1 with BK = 64 against BK = 32, one process, cfg3 shapes:
// QKV 775 -> 882 TF, out_proj 515 -> 553, fc1 714 -> 759, fc2 830 -> 996 TF.
// Functors: issue(kt, b) requests K tile kt into buffer b (0 / 1); frag_load(buf, kk, f) reads step kk of the stage at `buf`;
// frag_mma(f, acc, is_last) with is_last = std::true_type for the very last step (no younger fragment reads in flight).
template <class Frag, int BUF, int KS, int NMF, int NDS, class Acc, class IssueFn, class LoadFn, class MmaFn>
__device__ __forceinline__ void swp_kloop16(int nk, const char* lds, int wm, Acc& acc, IssueFn issue, LoadFn frag_load, MmaFn frag_mma) {
    static_assert(KS >= 2 && KS % 2 == 0, "step kk lives in f[kk & 1]");
    issue(0, 0);
    wait_dma_then_barrier<0>();                               // tile 0 landed
    issue(nk > 1 ? 1 : 0, 1);                                 // (a redundant reload when nk == 1: never read)
    Frag f[2];
    frag_load(lds, 0, f[0]);
    for (int kt = 0; kt + 1 < nk; ++kt) {
        const char* cur = lds + (kt & 1) * BUF;
        const char* nxt = lds + ((kt & 1) ^ 1) * BUF;
#pragma unroll
        for (int kk = 0; kk + 1 < KS; ++kk) {                 // step kk on f[kk & 1], step kk+1's fragments arriving
            frag_load(cur, kk + 1, f[(kk + 1) & 1]);
            frag_mma(f[kk & 1], acc, std::false_type());
            pin_mfma_ds<NMF, NDS>();
        }
        wait_dma_then_barrier<0>();
        const int k2 = kt + 2 < nk ? kt + 2 : nk - 1;
        if (wm == 0) issue(k2, kt & 1);
        __builtin_amdgcn_sched_barrier(0);
        frag_load(nxt, 0, f[0]);                              // last step of tile kt, step 0 of tile kt+1 arriving
        frag_mma(f[(KS - 1) & 1], acc, std::false_type());
        pin_mfma_ds<NMF, NDS>();
        if (wm == 1) issue(k2, kt & 1);
        __builtin_amdgcn_sched_barrier(0);
    }
    {   // last tile
        const char* cur = lds + ((nk - 1) & 1) * BUF;
#pragma unroll
        for (int kk = 0; kk + 1 < KS; ++kk) {
            frag_load(cur, kk + 1, f[(kk + 1) & 1]);
            frag_mma(f[kk & 1], acc, std::false_type());
            pin_mfma_ds<NMF, NDS>();
        }
        frag_mma(f[(KS - 1) & 1], acc, std::true_type());
    }
}

// ---- the staged-by-operand loop ---------------------------------------------------------------------------------------------
// The ring's tiles (Ring16Cfg<1, 64>, same swizzle: the 16 lanes of a ds_read_b128 group hold rows distinct mod 16 and two
// k groups, 16 distinct 16-B slots) on v_mfma_f32_16x16x32_bf16: the same flops per cycle on paper, but the chip holds a higher
// clock on the 16x16 shape under sustained matrix load (MI355X_MICROARCH.md, DVFS give-back item 7: ~1.12-1.15x the FLOP/s of the
// 32x32 loop at equal cycles) -- and everything else in the kernel speeds up with the clock.  Wave tile 128 x 64 = 8 x 4 MFMA tiles,
// a k step is 32 deep.  The MFMA operands are swapped, so a tile comes out TRANSPOSED in the registers: lane (fr, fq) holds row fr,
// columns 4 fq .. 4 fq + 3 of a 16x16 tile, and an epilogue can store row pieces straight from the accumulators.
//   STAGING BY OPERAND.  A wave is stuck for ~100 cycles per LDS-DMA request it issues, and while both waves of a SIMD issue
//   theirs at the same moment nobody feeds the matrix pipe.  Here the lower wave group (wm = 0) moves the whole B tile (plane 1:
//   W, k) and the upper one the whole A tile (plane 0) -- 8 requests per wave and K tile either way, issue_mine(kt, b) -- and a
//   tile is consumed in four micro-steps (k step ks, row half h) of 16 MFMAs in the order (0,0) (1,0) (0,1) (1,1): the B tile
//   has been read completely after the FIRST micro-step's fragment reads, the A tile after the third's.  So B of tile kt+2 is
//   requested behind a barrier at the start of micro-step 1 and A of tile kt+2 behind the barrier at the start of micro-step 3:
//   the two bursts lie half a tile apart, each overlapped by the other group's MFMAs, and both have at least a whole tile of
//   flight time.  At the second barrier the A group waits for all of its requests, the B group leaves its newest 8 (B of tile
//   kt+2, requested half a tile ago) in flight.  The reload is clamped as in the ring, which keeps those counts fixed.
//   FRAGMENTS: the A fragments of one half (4 x V8) ping-pong by micro-step, the B fragments of a k step (4 x V8) by k step -- 64
//   fragment registers instead of the 96 of two whole k-step sets, which with 128 accumulators would not fit 256.
// The caller has requested tile 0 (of BOTH groups: issue_mine(0, 0)) before the previous output tile's stores or at kernel
// start: it has landed once at most those STORES store instructions are still outstanding (vector memory operations retire in
// order).  Returns with every wave done with LDS and the clamped reload landed.
// (GEMM, round 3 against the 32x32 ring: QKV +18 %, fc1 +14 %, fc2 +6.6 % (long K), out_proj -14 %.)
template <int STORES, class IssueFn>
__device__ __forceinline__ void staged_kloop16(int nk, const char* lds, int wm, int wn, int lane, bool stores_in_flight,
                                               f32x4 (&acc)[8][4], IssueFn issue_mine) {
    using Cfg = Ring16Cfg<1, 64>;
    constexpr int ROWB = Cfg::ROWB, PLANE = Cfg::PLANE, BUF = Cfg::BUF;
    typedef typename Half16<0>::V8 V8;
    // lane (row fr, k-group fq) of a 16-row tile reads logical chunk 4 ks + fq of its row; (row >> 1) & 7 = (fr >> 1) & 7
    const int fr = lane & 15, fq = lane >> 4;
    V8 ah[2][4], bq[2][4];
    auto load_a = [&](const char* buf, int ks, int h, V8 (&a)[4]) {
        const char* row0 = buf + (wm * 128 + fr) * ROWB + ((4 * ks + fq) ^ ((fr >> 1) & 7)) * 16;
#pragma unroll
        for (int t = 0; t < 4; ++t) a[t] = *reinterpret_cast<const V8*>(row0 + (4 * h + t) * 16 * ROWB);
    };
    auto load_b = [&](const char* buf, int ks, V8 (&b)[4]) {
        const char* row0 = buf + PLANE + (wn * 64 + fr) * ROWB + ((4 * ks + fq) ^ ((fr >> 1) & 7)) * 16;
#pragma unroll
        for (int t = 0; t < 4; ++t) b[t] = *reinterpret_cast<const V8*>(row0 + t * 16 * ROWB);
    };
    zero_acc16(acc);
    auto mma = [&](int h, const V8 (&a)[4], const V8 (&b)[4]) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
                acc[4 * h + mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[nt], a[mt], acc[4 * h + mt][nt], 0, 0, 0);
    };

    if (stores_in_flight) wait_dma_then_barrier<STORES>();
    else wait_dma_then_barrier<0>();
    issue_mine(nk > 1 ? 1 : 0, 1);
    load_a(lds, 0, 0, ah[0]);
    load_b(lds, 0, bq[0]);
    for (int kt = 0; kt + 1 < nk; ++kt) {
        const char* cur = lds + (kt & 1) * BUF;
        const char* nxt = lds + ((kt & 1) ^ 1) * BUF;
        const int k2 = kt + 2 < nk ? kt + 2 : nk - 1;         // clamped: the last reload is never read
        load_a(cur, 1, 0, ah[1]);                             // u0 = (ks 0, h 0) computes; u1 = (ks 1, h 0) arriving: the last reads of B
        load_b(cur, 1, bq[1]);
        mma(0, ah[0], bq[0]);
        pin_mfma_ds<16, 8>();
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // every wave has read the B tile of `cur`
        if (wm == 0) issue_mine(k2, kt & 1);                  // B of tile kt+2 -> the B plane of `cur`
        __builtin_amdgcn_sched_barrier(0);
        load_a(cur, 0, 1, ah[0]);                             // u1 computes; u2 = (ks 0, h 1) arriving
        mma(0, ah[1], bq[1]);
        pin_mfma_ds<16, 4>();
        load_a(cur, 1, 1, ah[1]);                             // u2 computes; u3 = (ks 1, h 1) arriving: the last reads of A
        mma(1, ah[0], bq[0]);
        pin_mfma_ds<16, 4>();
        if (wm == 0) wait_dma_then_barrier<8>();              // every wave has read the A tile of `cur`, and tile kt+1 has landed
        else wait_dma_then_barrier<0>();
        if (wm == 1) issue_mine(k2, kt & 1);                  // A of tile kt+2 -> the A plane of `cur`
        __builtin_amdgcn_sched_barrier(0);
        load_a(nxt, 0, 0, ah[0]);                             // u3 computes; the next tile's u0 operands arriving
        load_b(nxt, 0, bq[0]);
        mma(1, ah[1], bq[1]);
        pin_mfma_ds<16, 8>();
    }
    {   // last tile
        const char* cur = lds + ((nk - 1) & 1) * BUF;
        load_a(cur, 1, 0, ah[1]);
        load_b(cur, 1, bq[1]);
        mma(0, ah[0], bq[0]);
        pin_mfma_ds<16, 8>();
        load_a(cur, 0, 1, ah[0]);
        mma(0, ah[1], bq[1]);
        pin_mfma_ds<16, 4>();
        load_a(cur, 1, 1, ah[1]);
        mma(1, ah[0], bq[0]);
        pin_mfma_ds<16, 4>();
        mma(1, ah[1], bq[1]);
    }
    wait_dma_then_barrier<0>();                               // every wave is done with LDS; the clamped reload has landed
}

}  // namespace rnamsm
