// RNA-MSM-SS: the nested (pseudoknot-free) structure of greatest summed pair probability above a threshold -- the core of
// ss_nested.hip.  Plain C++: g++ compiles it for the host test (tests/native/ss_nested_check.cpp, which runs the tile schedule and the
// traceback serially over the "threads"), hipcc for the kernels.  The contract is stated in include/rnamsm.h; in short
//   allowed  (i, j), i < j, iff j - i > min_loop and P[i, j] > theta in float32 (NaN, -inf: never; +inf and above 1: as 1.0)
//   w(i, j)  max(1, Q(P[i, j]) - Q(theta)), Q(x) = floor(min(x, 1) * 2^18): exact in float32, an int32
//   N(i, j)  = max(N(i, j-1), max over allowed (k, j), i <= k, of N(i, k-1) + w(k, j) + N(k+1, j-1)); 0 for j <= i
// Everything is integer arithmetic: the tables, the score and the canonical traceback are specified bit for bit.
// With M(k, j) = w(k, j) + N(k+1, j-1) (NEG where the pair is not allowed) the row is a max-plus product,
//   N(i, j) = max(N(i, j-1), max_k A(i, k) + M(k, j)),   A(i, k) = N(i, k-1), A(i, i) = 0,
// computed over 64 x 64 cell tiles of two int32 [Lp, Lp] tables (Lp = L rounded up to 64; cells past L are "not allowed"), one
// tile-diagonal after the other.  Tile (I, J):
//   outer phase   the k-tiles strictly between I and J: every operand tile is complete (outer_plain here; a register-tiled loop in
//                 the kernel -- max is exact, so the order does not matter)
//   inner phase   k inside tile I (A from the complete diagonal tile (I, I), M from THIS tile) and inside tile J (A from THIS
//                 tile's row, M from the complete (J, J)): cell (r, c) needs same-row cells to its left, same-column cells below it
//                 and its lower-left neighbour, so the cells of one anti-diagonal d = c - r + 63 are independent: 127 steps from the
//                 bottom-left corner.  A diagonal tile has one k range, inside itself, and starts at d = 63.
#pragma once
#include <stdint.h>

#include "struct_text.h"

namespace ssnested {

#define SSN_HD SSP_HD

constexpr int MAX_L = 4096, MAX_LOOP = 32, TILE = 64;
constexpr int32_t NEG = -(1 << 30);          // "not allowed": NEG + NEG = INT32_MIN and NEG + any sum (< 2^29) stay inside int32
constexpr float DEFAULT_THETA = 0.516f;
static_assert(MAX_L <= sspairs::LONG_MAX_L, "the lines' limit");

SSN_HD inline int tiles(int L) { return (L + TILE - 1) / TILE; }
SSN_HD inline int padded(int L) { return tiles(L) * TILE; }
// x > theta >= 0 here (or +inf): the conversion truncates a non-negative value = floor; x * 2^18 is exact
SSN_HD inline int32_t quant(float x) { return (int32_t)((x < 1.f ? x : 1.f) * 262144.f); }
SSN_HD inline int32_t imax(int32_t a, int32_t b) { return a > b ? a : b; }

struct Params {
    float theta;
    int32_t q_theta, min_loop;
};
SSN_HD inline Params params(float theta, int min_loop) { return Params{theta, quant(theta), min_loop}; }

// w(i, j), or NEG.  Reads the strict upper triangle only; cells past L are not allowed.
SSN_HD inline int32_t weight(const float* P, int L, int i, int j, Params q) {
    if (j >= L || j - i <= q.min_loop) return NEG;          // min_loop >= 0: i < j from here on
    const float p = P[(size_t)i * L + j];
    if (!(p > q.theta)) return NEG;                         // NaN, -inf
    return imax(1, quant(p) - q.q_theta);
}

// N(i, j) of the table, 0 below the diagonal (where nothing is ever stored or read)
SSN_HD inline int32_t table_n(const int32_t* N, int Lp, int i, int j) { return j < i ? 0 : N[(size_t)i * Lp + j]; }

// ---- the working set of one tile (LDS in the kernel): rows of 65 words, so that a column walk touches every bank
constexpr int LD = TILE + 1, NH_LD = TILE + 2;
struct TileMem {
    // off-diagonal tiles only.  a < b: A(64 I + a, 64 I + b) = N(64 I + a, 64 I + b - 1), from tile (I, I);
    // a > b: M(64 J + b, 64 J + a), tile (J, J) transposed, so that a cell's walk over k runs along a row
    int32_t X[TILE * LD];
    // this tile's N with a halo: nh(r, c), r in [0, 64], c in [-1, 63]; column -1 = the tile to the left, row 64 = the tile below.
    // Before its step a cell holds the outer phase's maximum.
    int32_t Nh[(TILE + 1) * NH_LD];
    int32_t Mc[TILE * LD];                                  // this tile's M; before its step a cell holds w(i, j)
};
SSN_HD inline int32_t& nh(TileMem& m, int r, int c) { return m.Nh[r * NH_LD + c + 1]; }

// Element e of the staging work of tile (I, J), e in [0, 65 * 65): call for every e after the outer maxima are in nh(r, c).
SSN_HD inline void stage_inner(TileMem& m, const float* P, int L, const int32_t* N, const int32_t* M, int Lp, int I, int J, Params q,
                               int e) {
    const int a = e / (TILE + 1), b = e % (TILE + 1), i0 = TILE * I, j0 = TILE * J;
    if (a == TILE || b == TILE) {                           // the halo: row 64 at columns -1 .. 62, column -1 at rows 0 .. 63
        if (a == TILE && b < TILE) nh(m, TILE, b - 1) = table_n(N, Lp, i0 + TILE, j0 + b - 1);
        else if (a < TILE) nh(m, a, -1) = table_n(N, Lp, i0 + a, j0 - 1);
        return;
    }
    m.Mc[a * LD + b] = weight(P, L, i0 + a, j0 + b, q);
    if (I == J) return;
    if (a < b) m.X[a * LD + b] = table_n(N, Lp, i0 + a, i0 + b - 1);
    else if (a > b) m.X[a * LD + b] = M[(size_t)(j0 + b) * Lp + j0 + a];
}

// M of cell (r, c) from its weight and its lower-left neighbour
SSN_HD inline int32_t cell_m(TileMem& m, int r, int c) {
    const int32_t w = m.Mc[r * LD + c];
    return w == NEG ? NEG : w + nh(m, r + 1, c - 1);
}

// Share `part` of `nparts` of cell (r, c)'s maximum over k (k = i itself is cell_m: A(i, i) = 0).
SSN_HD inline int32_t cell_part(TileMem& m, int r, int c, bool diag, int min_loop, int part, int nparts) {
    int32_t best = NEG;
    const int last = c - min_loop - 1;                      // k <= j - min_loop - 1 inside the column tile
    if (diag) {
        for (int kk = r + 1 + part; kk <= last; kk += nparts) best = imax(best, nh(m, r, kk - 1) + m.Mc[kk * LD + c]);
        return best;
    }
    for (int kk = r + 1 + part; kk < TILE; kk += nparts) best = imax(best, m.X[r * LD + kk] + m.Mc[kk * LD + c]);
    for (int kk = part; kk <= last; kk += nparts) best = imax(best, nh(m, r, kk - 1) + m.X[c * LD + kk]);
    return best;
}

// cell (r, c) done: over_k = the maximum of its shares
SSN_HD inline void cell_store(TileMem& m, int r, int c, int32_t cm, int32_t over_k) {
    nh(m, r, c) = imax(imax(nh(m, r, c), nh(m, r, c - 1)), imax(cm, over_k));
    m.Mc[r * LD + c] = cm;
}

// The outer phase of cell (r, c) of tile (I, J), stated plainly.
SSN_HD inline int32_t outer_plain(const int32_t* N, const int32_t* M, int Lp, int I, int J, int r, int c) {
    int32_t best = 0;
    const int i = TILE * I + r, j = TILE * J + c;
    for (int k = TILE * (I + 1); k < TILE * J; ++k) best = imax(best, N[(size_t)i * Lp + k - 1] + M[(size_t)k * Lp + j]);
    return best;
}

// ---- the traceback.  An interval (i, j), i < j: the largest j' in (i, j] with N(i, j') != N(i, j'-1) is the first column the
// canonical walk does not leave unpaired; its partner is the smallest k that attains N(i, j').
SSN_HD inline int trace_paired_column(const int32_t* N, int Lp, int i, int j, int first, int stride) {
    int best = -1;
    for (int c = i + 1 + first; c <= j; c += stride)
        if (N[(size_t)i * Lp + c] != N[(size_t)i * Lp + c - 1]) best = c;
    return best;
}
SSN_HD inline int trace_partner(const int32_t* N, const int32_t* M, int Lp, int i, int j, int min_loop, int first, int stride) {
    const int32_t want = N[(size_t)i * Lp + j];
    for (int k = i + first; k <= j - min_loop - 1; k += stride)
        if ((k == i ? 0 : N[(size_t)i * Lp + k - 1]) + M[(size_t)k * Lp + j] == want) return k;
    return INT32_MAX;
}

SSN_HD inline uint8_t dbn_char(int b, int partner) { return partner == 0 ? '.' : partner > b + 1 ? '(' : ')'; }

#if !defined(__HIPCC__)
// ---- the whole decode, serially: the kernels' schedule with one "thread".  N, M: [Lp, Lp] each; stack: [L + 2] pairs of int.
inline void fill_serial(const float* P, int L, Params q, int32_t* N, int32_t* M, TileMem& m) {
    const int T = tiles(L), Lp = padded(L);
    for (int d = 0; d < T; ++d)
        for (int I = 0; I + d < T; ++I) {
            const int J = I + d;
            const bool diag = d == 0;
            for (int r = 0; r < TILE; ++r)
                for (int c = 0; c < TILE; ++c) nh(m, r, c) = d >= 2 ? outer_plain(N, M, Lp, I, J, r, c) : 0;
            for (int e = 0; e < (TILE + 1) * (TILE + 1); ++e) stage_inner(m, P, L, N, M, Lp, I, J, q, e);
            for (int s = diag ? TILE - 1 : 0; s < 2 * TILE - 1; ++s)
                for (int r = 0; r < TILE; ++r) {
                    const int c = s - (TILE - 1) + r;
                    if (c < 0 || c >= TILE) continue;
                    const int32_t cm = cell_m(m, r, c);
                    int32_t over_k = NEG;
                    for (int part = 0; part < 4; ++part) over_k = imax(over_k, cell_part(m, r, c, diag, q.min_loop, part, 4));
                    cell_store(m, r, c, cm, over_k);
                }
            for (int r = 0; r < TILE; ++r)
                for (int c = 0; c < TILE; ++c) {
                    N[(size_t)(TILE * I + r) * Lp + TILE * J + c] = nh(m, r, c);
                    M[(size_t)(TILE * I + r) * Lp + TILE * J + c] = m.Mc[r * LD + c];
                }
        }
}

// partner [L] (zeroed here), counts [5], the bodies within 32 L and 12 L bytes, dbn [L]; returns false if a loop bound was hit
inline bool trace_serial(const int32_t* N, const int32_t* M, int L, int min_loop, const uint8_t* letters, int32_t* stack,
                         int32_t* partner, int32_t* counts, uint8_t* ct, uint8_t* bpseq, uint8_t* dbn) {
    const int Lp = padded(L);
    for (int b = 0; b < L; ++b) partner[b] = 0;
    int sp = 0, steps = 0;
    if (L > 1) {
        stack[0] = 0;
        stack[1] = L - 1;
        sp = 1;
    }
    for (; sp > 0 && steps < 2 * L + 2; ++steps) {
        --sp;
        const int i = stack[2 * sp], j = stack[2 * sp + 1];
        const int c = trace_paired_column(N, Lp, i, j, 0, 1);
        if (c < 0) continue;
        const int k = trace_partner(N, M, Lp, i, c, min_loop, 0, 1);
        if (k == INT32_MAX) return false;
        partner[k] = c + 1;
        partner[c] = k + 1;
        if (k - 1 > i) {
            stack[2 * sp] = i;
            stack[2 * sp + 1] = k - 1;
            ++sp;
        }
        if (c - 1 > k + 1) {
            stack[2 * sp] = k + 1;
            stack[2 * sp + 1] = c - 1;
            ++sp;
        }
    }
    if (sp > 0) return false;
    const auto at = [&](int b) { return partner[b]; };          // the kernel's tail with one "thread" that owns every base
    bool bad = false;
    const uint64_t total = sspairs::measure_lines(0, L, L, at, letters, &bad);
    sspairs::put_lines(0, L, L, at, letters, 0, ct, bpseq);
    sspairs::put_counts(counts, total, bad);
    counts[4] = N[(size_t)Lp * 0 + L - 1];
    for (int b = 0; b < L; ++b) dbn[b] = dbn_char(b, partner[b]);
    return true;
}
#endif

}  // namespace ssnested
