// The blocked "popcount GEMM" of the alignment kernels (device code): msa_pdist.hip's pdist_pair_kernel, seqid_filter.hip's
// seqid_cand_kernel and seqid_resolve_kernel, invcov.hip's invcov_count_kernel -- and the packer that makes the word planes of the
// first two.
//
// The operands are word-major planes P[w][row] of 64-bit words, rows padded to a multiple of 64 and words to a multiple of WK with
// zero words.  A block of 256 threads owns a 64 x 64 tile of pairs, thread (ty, tx) = (threadIdx.x / 16, % 16) the 4 x 4 pairs
// (ty * 4 + x, tx * 4 + y) in registers.  Per step WK words of the 64 + 64 rows are staged in LDS (sA / sB, [WK][64], word-major, so
// the global reads and the LDS reads are contiguous 16-byte vectors) between two barriers.  Every sum is over one thread's words in
// ascending order in integers: no atomics, no scratch, the same bits on every run.
#pragma once
#include "common.h"
#include "msa_words.h"

namespace rnamsm {

constexpr int WT_TILE = 64;        // rows of a pair tile, each way

// acc + the set bits of mask in ONE instruction (v_bcnt_u32_b32 adds its second operand).  Written out because the compiler, left to
// itself, counts into fresh registers and adds afterwards: one more instruction per dword, and 256 live temporaries per step.
__device__ __forceinline__ int count_add(uint32_t mask, int acc) {
    int out;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(out) : "v"(mask), "v"(acc));
    return out;
}

// The per-word operations.  Acc: what a pair accumulates; Side: a staged word as the 16-pair loop wants it, made ONCE per a[x] / b[y]
// by prep; add: one word of one pair.
struct MismatchOp {                // bytes that differ (msa_words.h: pd_mismatches)
    using Acc = int;
    using Side = uint64_t;
    static __device__ __forceinline__ Side prep(uint64_t w) { return w; }
    static __device__ __forceinline__ void add(Side a, Side b, Acc& c) {
        const uint64_t x = a ^ b;
        c = count_add(nonzero_bytes32((uint32_t)(x >> 32)), count_add(nonzero_bytes32((uint32_t)x), c));
    }
};
struct ResiduePairOp {             // both / same under the residue masks (msa_words.h: sq_pair)
    struct Acc { int both, same; };
    struct Side { uint64_t w; uint32_t lo, hi; };
    static __device__ __forceinline__ Side prep(uint64_t w) { return {w, sq_residues_lo(w), sq_residues_hi(w)}; }
    static __device__ __forceinline__ void add(const Side& a, const Side& b, Acc& c) {
        const uint64_t d = a.w ^ b.w;
        const uint32_t ml = a.lo & b.lo, mh = a.hi & b.hi;
        c.both = count_add(mh, count_add(ml, c.both));
        c.same = count_add(mh & ~sq_residues_hi(d), count_add(ml & ~sq_residues_lo(d), c.same));
    }
};
struct AndPopcountOp {             // rows that have both bits
    using Acc = int;
    using Side = uint64_t;
    static __device__ __forceinline__ Side prep(uint64_t w) { return w; }
    static __device__ __forceinline__ void add(Side a, Side b, Acc& c) { c += __popcll(a & b); }
};

// acc = the sums over all Wp words (a multiple of WK) of the tile's pairs, from zero.  Side A is the 64 consecutive rows from `ra`;
// side B is the 64 consecutive rows from `rb`, or with GATHER the rows idxB[0 .. 63] (LDS; -1 = no row: zero words; 8-byte reads, no
// second copy of the rows).  A thread stages rows sp, sp + 1 of the words sw, sw + 8, ...: one 16-byte vector per panel and eight
// words.  Ends with a barrier: the panels are free again.
template <int WK, bool GATHER, class Op>
__device__ __forceinline__ void word_tile_loop(const uint64_t* __restrict__ P, int Wp, int64_t Np, int64_t ra, int64_t rb, const int* idxB,
                                               uint64_t (*sA)[WT_TILE], uint64_t (*sB)[WT_TILE], typename Op::Acc (&acc)[4][4]) {
    static_assert(WK % 8 == 0, "256 threads stage eight words of 64 rows at a time");
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = typename Op::Acc{};
    const int sw = threadIdx.x >> 5, sp = (threadIdx.x & 31) * 2;
    int64_t g0 = 0, g1 = 0;
    if constexpr (GATHER) { g0 = idxB[sp]; g1 = idxB[sp + 1]; }
    for (int w0 = 0; w0 < Wp; w0 += WK) {
#pragma unroll
        for (int w = sw; w < sw + WK; w += 8) {
            const uint64_t* base = P + (int64_t)(w0 + w) * Np;
            *reinterpret_cast<uint4*>(&sA[w][sp]) = *reinterpret_cast<const uint4*>(base + ra + sp);
            if constexpr (GATHER) {
                sB[w][sp] = g0 >= 0 ? base[g0] : 0ull;
                sB[w][sp + 1] = g1 >= 0 ? base[g1] : 0ull;
            } else {
                *reinterpret_cast<uint4*>(&sB[w][sp]) = *reinterpret_cast<const uint4*>(base + rb + sp);
            }
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < WK; ++w) {
            typename Op::Side a[4], b[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) { a[x] = Op::prep(sA[w][ty * 4 + x]); b[x] = Op::prep(sB[w][tx * 4 + x]); }
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) Op::add(a[x], b[y], acc[x][y]);
        }
        __syncthreads();
    }
}

// The packer of such planes from an alignment's bytes, words_pack_kernel (msa_pdist.hip), on stream s.
void words_pack(const uint8_t* msa, int N, int L, int64_t ld, int gap, const int32_t* order, int Wp, int64_t Np, uint64_t* P, hipStream_t s);

}  // namespace rnamsm
