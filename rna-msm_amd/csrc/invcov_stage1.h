// Stage 1 of invcov.hip (the symbols that occur, the bit planes, the integer marginals, the banded integer count launch) as the
// host functions its users call: rnamsm_msa_invcov and rnamsm_msa_mi in invcov.hip, rnamsm_msa_wmi in msa_wmi.hip.  The kernels and
// the definitions live in invcov.hip; the layout of the planes is described at its top.
#pragma once
#include "common.h"

namespace rnamsm {

constexpr int IC_TILE = 64;        // (column, symbol) rows of a count tile, each way
constexpr int IC_WK = 16;          // words staged per step
constexpr int IC_MAX_K = 16;
constexpr int IC_META = 32;        // int32 header: K, then the symbols ascending (the first 16 of them)
constexpr int IC_MAX_N = 1 << 20;
constexpr size_t IC_BAND_BYTES = (size_t)1 << 28;      // counts of one band of columns i

struct InvcovWs {
    size_t present, lut, meta, marg, planes, band, total;
    int W, Wp;
    int64_t Rp;
};
// K: the symbols the layout is made for (the size function knows no K and takes IC_MAX_K; the call lays the planes out for the K
// it found, inside the same bytes)
InvcovWs invcov_ws(int N, int L, int K);

// `who` is the entry point's name in every message.
int stage1_check(const char* who, bool pointers, int N, int L, int64_t ld, int gap);

struct Stage1 {
    InvcovWs w;                  // the layout for the K that was found
    int K, R;
    int32_t *meta, *marg, *band; // the header (K, the symbols), n_a(i) as [L, K], the workspace's band of counts
    uint64_t* P;
};

// One more int32 for the read-back that already fetches K: a verdict some kernel of the caller's, enqueued on the stream before
// the call, left on the device.  The caller reads `host` after stage1_planes returned RNAMSM_OK.
struct Stage1Verdict {
    const int32_t* dev;
    int32_t host;
};

// presence, table (the one wait for the stream: K is read back, and the verdict with it), planes, marginals
int stage1_planes(const char* who, const uint8_t* tokens, int N, int L, int64_t ld, int gap, char* ws, hipStream_t s, Stage1* st,
                  Stage1Verdict* verdict = nullptr);

// columns i per band of counts held in the workspace: all of them, or a multiple of 64 (tile-aligned rows)
int stage1_band(int L, int K);

// the counts of columns [i0, i1) into cnt as [i - i0][j][a][b]; full = 0: tiles wholly below the diagonal are left out
void stage1_count(const Stage1& st, int L, int i0, int i1, int full, int32_t* cnt, hipStream_t s);

}  // namespace rnamsm
