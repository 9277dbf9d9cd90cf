// f1: contact head on the row attentions (ContactPredictionHead.forward, modules.py:344-366; symmetrize / apc,
// utils/tensor.py:98-113; called from model.py:412-414):
//   X_ch = attn[ch, 1:, 1:]            (strip <cls>; the RNA alphabet appends no <eos>)
//   S_ch = X_ch + X_ch^T
//   N_ch = S_ch - rowsum(S_ch) colsum(S_ch) / sum(S_ch)
//   contacts[i,j] = sigmoid(b + sum_ch w[ch] N_ch[i,j])
// HBM-bound: the 120 x C x C maps (126 MB at C = 512) are read twice (once for the sums, once -- plus the transposed
// tile -- for the regression); S is symmetric so colsum == rowsum.
// The maps' layout is a parameter: X(ch, i, j) = maps[ch * plane_stride + (i + off) * ld + (j + off)], T x T per channel.
//   rnamsm_contact_head            the un-stripped [nch, C, C] maps:  off = 1, ld = C, plane_stride = C * C, T = C - 1
//   rnamsm_contact_head_atp        the stripped atp [nch, L, L] of rnamsm_pack_outputs: off = 0, ld = L, the caller's plane_stride
//   rnamsm_contact_head_packed     B members of the second kind in one launch set
// One arithmetic for all three: a [T, T] result depends on the T x T values of each channel and on nothing else.
#include "common.h"

namespace rnamsm {
namespace {

constexpr int CT_ROWS = 256;       // rows of one block of the sums (= the stride of the total's partial sums)
constexpr int CT_TILE = 32;        // output tile of the regression: 32 x 32
constexpr int CT_CHAIN = 64;       // terms of one sequential chain of a row / column sum (as lm_dense's K blocks)

// ---- the member of a block ------------------------------------------------------------------------------------------------------
// One kernel per stage serves the lone calls and the batched one, as in ss_head.hip / rsa_head.hip: batched, mem is the device
// table of the B members and a block finds its own by a search over the prefix sums of the stage's blocks (common.h: member_of);
// lone, the one member is the kernel argument itself (tile0 = chunk0 = 0, ws_off = 0).  The choice is a template argument: one
// definition, two code objects.
// Every member has its own slab in the workspace (floats [ws_off, ws_off + nch * T + nch)): rs [nch, T], then tot [nch] -- the lone
// call's workspace.
struct ContactMember {       // 64 bytes
    const float* maps;
    int64_t plane_stride;
    float* contacts;         // [T, T]
    int64_t ws_off;          // floats of the members' slabs before it
    int32_t ld, off, T;
    int32_t tile0;           // 32 x 32 output tiles of the members before it (a member's share: ceil(T / 32)^2, row by row)
    int32_t chunk0;          // 256-row blocks of the sums of the members before it (a member's share: ceil(T / 256))
    int32_t pad_[3];
};
static_assert(sizeof(ContactMember) == 64, "ContactMember layout");
template <bool PACKED, class F>
__device__ __forceinline__ ContactMember contact_member(const ContactMember* __restrict__ mem, int B, const ContactMember& lone, int key,
                                                        F ContactMember::*field) {
    if (PACKED) return mem[member_of(mem, B, key, field)];
    return lone;
}
__device__ __forceinline__ const float* contact_plane(const ContactMember& m, int ch) {      // &X(ch, 0, 0)
    return m.maps + (int64_t)ch * m.plane_stride + (int64_t)m.off * m.ld + m.off;
}

// The halving tree of the total: red[t] = thread t's partial sum (rows t, t + 256, ... in increasing order) -> red[0]
__device__ __forceinline__ void contact_tree(float* red) {
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- launch 1
// rs[ch, i] = sum_j X[i,j]  +  sum_j X[j,i], each summed in fixed blocks of CT_CHAIN: a chain from zero over j = 64 b .. 64 b + 63,
// the block sums added in ascending b.  One chain over all T terms lost 3.7 x (T = 255) to 7 x (T = 1023) what the library's fp32
// sum loses on rows of unlike elements.  Block (channel, 256 rows): the rows of a channel are spread over ceil(T / 256) blocks, where one block per channel walked them 256 at a time (120 blocks on 256 CUs,
// whatever T).  A member of T <= 256 has one block per channel, which then holds every partial sum of the total and finishes
// it here; a longer member's total is launch 2.
template <bool PACKED>
__global__ __launch_bounds__(CT_ROWS) void contact_sums_kernel(const ContactMember* __restrict__ mem, int B, const ContactMember lone,
                                                               float* __restrict__ ws) {
    __shared__ float red[CT_ROWS];
    const ContactMember m = contact_member<PACKED>(mem, B, lone, (int)blockIdx.y, &ContactMember::chunk0);
    const int ch = blockIdx.x, nch = gridDim.x, T = m.T, ld = m.ld;
    const float* X = contact_plane(m, ch);
    float* rs = ws + m.ws_off;
    const int i = ((int)blockIdx.y - m.chunk0) * CT_ROWS + (int)threadIdx.x;
    float total = 0.f;
    if (i < T) {
        float r = 0.f, c = 0.f;
        int j0 = 0;
        for (; j0 + CT_CHAIN <= T; j0 += CT_CHAIN) {                // the whole chains: a constant trip count
            float rb = 0.f, cb = 0.f;
#pragma unroll 8
            for (int j = j0; j < j0 + CT_CHAIN; ++j) {
                rb += X[(int64_t)i * ld + j];  // row i of X      (lanes stride rows: L2-resident re-reads)
                cb += X[(int64_t)j * ld + i];  // column i of X   (coalesced across lanes)
            }
            r += rb;
            c += cb;
        }
        if (j0 < T) {                                               // the last, shorter chain (T % 64 terms)
            float rb = 0.f, cb = 0.f;
            for (int j = j0; j < T; ++j) {
                rb += X[(int64_t)i * ld + j];
                cb += X[(int64_t)j * ld + i];
            }
            r += rb;
            c += cb;
        }
        const float s = r + c;
        rs[(int64_t)ch * T + i] = s;
        total += s;
    }
    if (T > CT_ROWS) return;                  // block-uniform
    red[threadIdx.x] = total;
    contact_tree(red);
    if (threadIdx.x == 0) rs[(int64_t)nch * T + ch] = red[0];
}

// ---------------------------------------------------------------------------------------------------------------- launch 2
// tot[ch] = sum_i rs[ch, i] of a member of T > 256, in the order one block per channel had: thread t adds rows t, t + 256, ... in
// increasing order, then the tree.  Block (channel, member); a member of T <= 256 has its total already.
template <bool PACKED>
__global__ __launch_bounds__(CT_ROWS) void contact_tot_kernel(const ContactMember* __restrict__ mem, const ContactMember lone,
                                                              float* __restrict__ ws) {
    __shared__ float red[CT_ROWS];
    const ContactMember m = PACKED ? mem[blockIdx.y] : lone;
    const int ch = blockIdx.x, nch = gridDim.x, T = m.T;
    if (T <= CT_ROWS) return;                 // block-uniform
    float* rs = ws + m.ws_off;
    float total = 0.f;
    for (int i = threadIdx.x; i < T; i += CT_ROWS) total += rs[(int64_t)ch * T + i];
    red[threadIdx.x] = total;
    contact_tree(red);
    if (threadIdx.x == 0) rs[(int64_t)nch * T + ch] = red[0];
}

// ---------------------------------------------------------------------------------------------------------------- launch 3
// 32x32 output tile per block; the transposed operand X[J, I] goes through LDS so both global reads are coalesced.
// The channel's term is s - (r_i r_j) / tot with a correctly rounded fp32 division, as the reference divides (tensor.py:107-108): a
// product with a rounded 1 / tot costs a second rounding, which at T = 1, where the quotient is exactly s, left an ulp of s per
// channel in a logit that is the bias alone.  The accumulation acc + w (...) is an explicit fmaf, so that no
// instance's layout can change the contraction.  The head is HBM-bound; the division does not show in its time.
template <bool PACKED>
__global__ __launch_bounds__(256) void contact_regress_kernel(const ContactMember* __restrict__ mem, int B, const ContactMember lone,
                                                              const float* __restrict__ ws, const float* __restrict__ weight,
                                                              const float* __restrict__ bias, int nch) {
    __shared__ float tr[CT_TILE][CT_TILE + 1];
    const ContactMember m = contact_member<PACKED>(mem, B, lone, (int)blockIdx.x, &ContactMember::tile0);
    const int T = m.T, ld = m.ld;
    const int tiles = (T + CT_TILE - 1) / CT_TILE, tile = (int)blockIdx.x - m.tile0;
    const int i0 = (tile / tiles) * CT_TILE, j0 = (tile % tiles) * CT_TILE;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 8 rows of 32 per pass
    const float* rs = ws + m.ws_off;
    const float* tot = rs + (int64_t)nch * T;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < nch; ++ch) {
        const float* X = contact_plane(m, ch);
        const float w = weight[ch], t = tot[ch];
        const float* r = rs + (int64_t)ch * T;
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 4; ++p) {                               // tr[a][b] = X[j0 + a, i0 + b]
            const int a = ty + 8 * p, jj = j0 + a, ii = i0 + tx;
            tr[a][tx] = (jj < T && ii < T) ? X[(int64_t)jj * ld + ii] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int a = ty + 8 * p, i = i0 + a, j = j0 + tx;
            if (i < T && j < T) {
                const float s = X[(int64_t)i * ld + j] + tr[tx][a];
                const float a12 = r[i] * r[j];                      // a1 * a2 / a12, same order as tensor.py:107-108
                acc[p] = fmaf(w, s - a12 / t, acc[p]);
            }
        }
    }
    const float b = bias[0];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int i = i0 + ty + 8 * p, j = j0 + tx;
        if (i < T && j < T) m.contacts[(int64_t)i * T + j] = 1.f / (1.f + expf(-(acc[p] + b)));
    }
}

constexpr size_t contact_members_bytes(int B) { return ((size_t)B * sizeof(ContactMember) + 255) & ~(size_t)255; }
inline size_t contact_slab_floats(int T, int nch) { return (size_t)nch * T + nch; }
inline int contact_tiles(int T) { const int t = (T + CT_TILE - 1) / CT_TILE; return t * t; }
inline int contact_chunks(int T) { return (T + CT_ROWS - 1) / CT_ROWS; }

// The launches over `chunks` blocks of the sums and `tiles` output tiles: PACKED with mem / B the uploaded table of a batch, else
// null / 1 and the lone member.  any_long: a member has T > 256 (launch 2 has work).
template <bool PACKED>
int contact_launch(const ContactMember* mem, int B, const ContactMember& lone, int64_t chunks, int64_t tiles, bool any_long, int nch,
                   const float* weight, const float* bias, float* ws, hipStream_t s) {
    hipLaunchKernelGGL(contact_sums_kernel<PACKED>, dim3((unsigned)nch, (unsigned)chunks), dim3(CT_ROWS), 0, s, mem, B, lone, ws);
    RNAMSM_CHECK_LAUNCH(PACKED ? "contact_sums (packed)" : "contact_sums");
    if (any_long) {
        hipLaunchKernelGGL(contact_tot_kernel<PACKED>, dim3((unsigned)nch, (unsigned)B), dim3(CT_ROWS), 0, s, mem, lone, ws);
        RNAMSM_CHECK_LAUNCH(PACKED ? "contact_tot (packed)" : "contact_tot");
    }
    hipLaunchKernelGGL(contact_regress_kernel<PACKED>, dim3((unsigned)tiles), dim3(256), 0, s, mem, B, lone, ws, weight, bias, nch);
    RNAMSM_CHECK_LAUNCH(PACKED ? "contact_regress (packed)" : "contact_regress");
    return RNAMSM_OK;
}
int contact_lone(const float* maps, int64_t plane_stride, int ld, int off, int T, int nch, const float* weight, const float* bias,
                 float* contacts, void* workspace, hipStream_t s) {
    const ContactMember lone = {maps, plane_stride, contacts, 0, ld, off, T, 0, 0, {0, 0, 0}};
    return contact_launch<false>(nullptr, 1, lone, contact_chunks(T), contact_tiles(T), T > CT_ROWS, nch, weight, bias,
                                 static_cast<float*>(workspace), s);
}

}  // namespace
}  // namespace rnamsm

using namespace rnamsm;

extern "C" size_t rnamsm_contact_head_workspace_bytes(int C, int nch) {
    if (C < 2 || nch <= 0) return 0;
    return contact_slab_floats(C - 1, nch) * sizeof(float);
}

extern "C" int rnamsm_contact_head(const float* row_attn, const float* weight, const float* bias, float* contacts,
                                   void* workspace, size_t workspace_bytes, int C, int nch, void* stream) {
    RNAMSM_CHECK_ARG(row_attn && weight && bias && contacts && workspace, "contact_head: null pointer");
    RNAMSM_CHECK_ARG(C >= 2 && nch > 0, "contact_head: bad shape C=%d nch=%d", C, nch);
    RNAMSM_CHECK_ARG(workspace_bytes >= rnamsm_contact_head_workspace_bytes(C, nch), "contact_head: workspace too small");
    return contact_lone(row_attn, (int64_t)C * C, C, 1, C - 1, nch, weight, bias, contacts, workspace, static_cast<hipStream_t>(stream));
}

// The lone call on stripped maps, written once for rnamsm_contact_head_atp (who = "contact_head_atp", max_L = RNAMSM_CONTACT_MAX_L)
// and rnamsm_contact_head_long ("contact_head_long", RNAMSM_LONG_MAX_L: the stitched atp of a long alignment), as ss_head_lone
// is: one list of refusals under the entry's own name and limit, then the three kernels on the same descriptor, so the same bits
// where both run.  Every refusal comes before the first launch: a refused call leaves the stream and the outputs untouched.
// Beyond 1023: every offset into the maps, the contacts and the slab -- ch * plane_stride, i * ld + j, i * T + j, ch * T + i -- is
// int64_t in the kernels; the grids are nch x ceil(T / 256) <= nch x 16 and ceil(T / 32)^2 <= 2^14 blocks.
static int contact_atp_lone(const char* who, int max_L, const float* atp, int64_t plane_stride, int L, int nch, const float* weight,
                            const float* bias, float* contacts, void* workspace, size_t workspace_bytes, void* stream) {
    RNAMSM_CHECK_ARG(atp, "%s: null pointer (atp)", who);
    RNAMSM_CHECK_ARG(weight, "%s: null pointer (weight)", who);
    RNAMSM_CHECK_ARG(bias, "%s: null pointer (bias)", who);
    RNAMSM_CHECK_ARG(contacts, "%s: null pointer (contacts)", who);
    RNAMSM_CHECK_ARG(workspace, "%s: null pointer (workspace)", who);
    RNAMSM_CHECK_ARG(L >= 1 && L <= max_L, "%s: L=%d outside [1, %d]", who, L, max_L);
    RNAMSM_CHECK_ARG(nch > 0, "%s: nch=%d", who, nch);
    RNAMSM_CHECK_ARG(plane_stride >= (int64_t)L * L, "%s: plane stride %lld < L * L = %lld", who, (long long)plane_stride,
                     (long long)L * L);
    RNAMSM_CHECK_ARG(((uintptr_t)atp & 3u) == 0, "%s: atp is not 4-byte aligned", who);
    RNAMSM_CHECK_ARG(((uintptr_t)contacts & 3u) == 0, "%s: contacts is not 4-byte aligned", who);
    RNAMSM_CHECK_ARG(((uintptr_t)workspace & 3u) == 0, "%s: workspace is not 4-byte aligned", who);
    const size_t need = contact_slab_floats(L, nch) * sizeof(float);
    RNAMSM_CHECK_ARG(workspace_bytes >= need, "%s: workspace too small (workspace of %zu bytes, %zu needed)", who, workspace_bytes, need);
    return contact_lone(atp, plane_stride, L, 0, L, nch, weight, bias, contacts, workspace, static_cast<hipStream_t>(stream));
}

extern "C" int rnamsm_contact_head_atp(const float* atp, int64_t plane_stride, int L, int nch, const float* weight, const float* bias,
                                       float* contacts, void* workspace, size_t workspace_bytes, void* stream) {
    return contact_atp_lone("contact_head_atp", RNAMSM_CONTACT_MAX_L, atp, plane_stride, L, nch, weight, bias, contacts, workspace,
                            workspace_bytes, stream);
}

extern "C" size_t rnamsm_contact_head_long_workspace_bytes(int L, int nch) {
    if (L < 1 || L > RNAMSM_LONG_MAX_L || nch <= 0) return 0;
    return contact_slab_floats(L, nch) * sizeof(float);
}

extern "C" int rnamsm_contact_head_long(const float* atp, int64_t plane_stride, int L, int nch, const float* weight, const float* bias,
                                        float* contacts, void* workspace, size_t workspace_bytes, void* stream) {
    return contact_atp_lone("contact_head_long", RNAMSM_LONG_MAX_L, atp, plane_stride, L, nch, weight, bias, contacts, workspace,
                            workspace_bytes, stream);
}

extern "C" size_t rnamsm_contact_head_packed_workspace_bytes(int B, const int* Ls, int nch) {
    if (B < 1 || B > RNAMSM_CONTACT_MAX_BATCH || !Ls || nch <= 0) return 0;
    size_t floats = 0;
    for (int b = 0; b < B; ++b) {
        if (Ls[b] < 1 || Ls[b] > RNAMSM_CONTACT_MAX_L) return 0;
        floats += contact_slab_floats(Ls[b], nch);
    }
    return contact_members_bytes(B) + floats * sizeof(float);
}

extern "C" int rnamsm_contact_head_packed(const rnamsm_contact_item* items, int B, int nch, const float* weight, const float* bias,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    // every refusal comes before the first launch: a refused call leaves the stream and the outputs untouched
    RNAMSM_CHECK_ARG(items && weight && bias && workspace, "contact_head_packed: null pointer");
    RNAMSM_CHECK_ARG(B >= 1 && B <= RNAMSM_CONTACT_MAX_BATCH, "contact_head_packed: B=%d outside [1, %d]", B, RNAMSM_CONTACT_MAX_BATCH);
    RNAMSM_CHECK_ARG(nch > 0, "contact_head_packed: nch=%d", nch);
    size_t floats = 0;
    int64_t tiles_total = 0, chunks_total = 0;
    bool any_long = false;
    for (int b = 0; b < B; ++b) {
        const rnamsm_contact_item& it = items[b];
        RNAMSM_CHECK_ARG(it.L >= 1 && it.L <= RNAMSM_CONTACT_MAX_L, "contact_head_packed: member %d: L=%d outside [1, %d]", b, it.L,
                         RNAMSM_CONTACT_MAX_L);
        RNAMSM_CHECK_ARG(it.atp && it.contacts, "contact_head_packed: member %d: null pointer", b);
        RNAMSM_CHECK_ARG(it.plane_stride >= (int64_t)it.L * it.L, "contact_head_packed: member %d: plane stride %lld < L * L = %lld", b,
                         (long long)it.plane_stride, (long long)it.L * it.L);
        RNAMSM_CHECK_ARG(((uintptr_t)it.atp & 3u) == 0 && ((uintptr_t)it.contacts & 3u) == 0,
                         "contact_head_packed: member %d: a pointer is not 4-byte aligned", b);
        floats += contact_slab_floats(it.L, nch);
        tiles_total += contact_tiles(it.L);
        chunks_total += contact_chunks(it.L);
        any_long = any_long || it.L > CT_ROWS;
    }
    RNAMSM_CHECK_ARG(aligned16(workspace), "contact_head_packed: 16-byte alignment of the workspace");
    RNAMSM_CHECK_ARG(workspace_bytes >= contact_members_bytes(B) + floats * sizeof(float), "contact_head_packed: workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ContactMember* mem = static_cast<ContactMember*>(workspace);
    int64_t ws_off = 0;
    int32_t tile0 = 0, chunk0 = 0;
    const int rc = upload_members(mem, B, [&](int b) {
        const rnamsm_contact_item& it = items[b];
        const ContactMember m = {it.atp, it.plane_stride, it.contacts, ws_off, it.L, 0, it.L, tile0, chunk0, {0, 0, 0}};
        ws_off += (int64_t)contact_slab_floats(it.L, nch);
        tile0 += contact_tiles(it.L);
        chunk0 += contact_chunks(it.L);
        return m;
    }, s, "contact_members");
    if (rc != RNAMSM_OK) return rc;
    return contact_launch<true>(mem, B, ContactMember{}, chunks_total, tiles_total, any_long, nch, weight, bias,
                                reinterpret_cast<float*>(static_cast<char*>(workspace) + contact_members_bytes(B)), s);
}
