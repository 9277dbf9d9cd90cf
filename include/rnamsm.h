/*
 * rnamsm.h -- C ABI of librnamsm_hip.so: the MI355X (gfx950) implementation of RNA-MSM's
 * axial-attention forward path.
 *
 * The reference (yikunpku/RNA-MSM) has no FFI: the path is reached through nn.Module.forward
 * calls that bottom out in ATen ops.  Each entry point below replaces one
 * group of those ATen call sites; the citation names the reference lines (relative to the
 * reference root) whose result it reproduces.  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, no torch types; every pointer is DEVICE memory owned by the caller;
 *   - one MSA per call (B = 1, as the reference CLI runs it: RNA_MSM_Inference.py:141-148);
 *     a token (r, c) of the [R rows, C columns] alignment is row t = r*C + c of a [T, D] matrix;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing
 *     synchronises, nothing allocates (scratch is caller-provided, sized by *_workspace_bytes);
 *   - return value: RNAMSM_OK or a negative rnamsm_status; rnamsm_last_error() gives the text
 *     for the calling thread;
 *   - dtype: the per-kernel entry points implement RNAMSM_F32 (exact-fp32 MFMA, v_mfma_f32_32x32x2_f32) and return
 *     RNAMSM_ERR_UNSUPPORTED otherwise; rnamsm_gemm_bf16 and rnamsm_forward's dtype select the bf16 matrix-core modes.
 */
#ifndef RNAMSM_H_
#define RNAMSM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RNAMSM_VERSION 600 /* major*10000 + minor*100 + patch; 6.0 (round 6): same 63 entry points and signatures; ten knob names of
                              * rnamsm_set_param are gone (INVALID), rnamsm_forward_packed refuses a table mixing the two LayerNorm-fold classes,
                              * rnamsm_pack_outputs requires D % 4 == 0 and 16-byte-aligned x_final / emb.  5.0: rnamsm_forward_packed takes dtype +
                              * weight_planes, dtype value 2 (bf16x3) answers UNSUPPORTED, + rnamsm_softmax_rows_scaled; 4.0: row_pos_dim, rnamsm_embed_ln_rows.
                              * Entry points added since (the heads, the stitcher, rnamsm_msa_invcov) are additive and left the number where it was. */

typedef enum {
    RNAMSM_OK = 0,
    RNAMSM_ERR_INVALID = -1,     /* bad shape / null pointer / misaligned argument */
    RNAMSM_ERR_UNSUPPORTED = -2, /* valid request this build does not implement */
    RNAMSM_ERR_HIP = -3          /* a HIP runtime call failed (launch, attribute) */
} rnamsm_status;

/* Arithmetic of the Linear GEMMs inside rnamsm_forward (everything else -- attention contractions, softmax,
 * LayerNorm, residual stream, outputs -- is fp32 in every mode):
 *   RNAMSM_F32     exact-fp32 MFMA (default; the parity path)
 *   RNAMSM_BF16    bf16 MFMA on bf16-rounded operands, fp32 accumulate (mixed precision; BASELINE config 4)
 *   (value 2, RNAMSM_BF16X3_REMOVED: hi/lo bf16 pairs, 3 products -- removed in round 5: the same three MFMAs per product as
 *                  F16X3 with 17 instead of 22 operand bits; every entry point answers RNAMSM_ERR_UNSUPPORTED for it)
 *   RNAMSM_F16X3   fp16 MFMA on hi/lo-split operands, 3 products, fp32 accumulate (~2^-22 operand error: fp32-grade
 *                  for the fp16-range operands this model feeds its Linear layers) */
typedef enum { RNAMSM_F32 = 0, RNAMSM_BF16 = 1, RNAMSM_BF16X3_REMOVED = 2, RNAMSM_F16X3 = 3 } rnamsm_dtype;
typedef enum { RNAMSM_ACT_NONE = 0, RNAMSM_ACT_GELU_ERF = 1 } rnamsm_act;

int rnamsm_version(void);
const char* rnamsm_last_error(void);
/* Number of visible HIP devices (0 on a CPU-only box); never initialises a context. */
int rnamsm_device_count(void);

/* K0 -- MSATransformer.forward embedding section (model.py:349-362) with
 * LearnedPositionalEmbedding.forward (modules.py:286-300):
 *   x[r,c,:] = LayerNorm( E_tok[tok[r,c]] + E_pos[pos(r,c)] + row_pos[r] ),
 *   pos(r,c) = (#non-pad tokens in tok[r,0..c]) * (tok[r,c] != pad) + pad_idx.
 * tokens int64 [R,C]; embed_tokens [V,D]; embed_positions [P,D]; row_pos [>=R] (the
 * (1,1024,1,1) msa_position_embedding); out [R*C, D].  Token ids outside [0,V) or positions
 * outside [0,P) set bit 0 of *err_flag (device int, may be NULL; value 1) and are clamped. */
int rnamsm_embed_ln(const int64_t* tokens, const float* embed_tokens, const float* embed_positions,
                    const float* row_pos, const float* gamma, const float* beta, float* out,
                    int R, int C, int D, int vocab, int num_positions, int pad_idx, float eps,
                    int* err_flag, void* stream);
/* The same with the per-channel alignment-row embedding of msm/model.py:289-292: row_pos_dim = D reads row_pos as
 * [>=R, D] (x[r,c,:] += row_pos[r,:]); row_pos_dim = 0 or 1 is rnamsm_embed_ln. */
int rnamsm_embed_ln_rows(const int64_t* tokens, const float* embed_tokens, const float* embed_positions,
                         const float* row_pos, int row_pos_dim, const float* gamma, const float* beta, float* out,
                         int R, int C, int D, int vocab, int num_positions, int pad_idx, float eps,
                         int* err_flag, void* stream);

/* K1 -- nn.LayerNorm over the last dim (modules.py:383,387; model.py:396): y = (x-mean)/sqrt(var+eps)*gamma+beta,
 * biased variance.  x, y [T, D] contiguous (y may alias x). */
int rnamsm_layernorm(const float* x, const float* gamma, const float* beta, float* y,
                     int64_t T, int D, float eps, void* stream);

/* K1 folded into the Linear that consumes it (NormalizedResidualBlock, modules.py:385-401: layer(LayerNorm(x)) with
 * layer's first op a Linear -- q/k/v projections modules.py:760-766, 794, 896-905; fc1 modules.py:424):
 *   LN(x) W^T + b  =  rstd[m] * ( sum_k x[m,k] Wg[n,k]  -  mean[m] * c[n] ) + d[n]
 *   Wg = W * gamma (per input feature k),  c[n] = sum_k Wg[n,k],  d[n] = b[n] + sum_k W[n,k] * beta[k]
 * so the GEMM reads the residual stream itself: no normalised copy of it is written or re-read (806 MB per LayerNorm at
 * M=256 L=512) and LayerNorm is no launch at all.  The statistics come from whoever wrote x: `row_partials`
 * [K/32, M, 2] (slab-major) holds, per row and 32-feature slab, the slab's sum and its sum of squares about the slab's own
 * mean; rnamsm_row_stats_from_partials combines them into (mean, rstd) per row as in Chan et al. (M2 = sum of slab M2 +
 * sum of 32 (slab mean - mean)^2), so the biased variance never comes from a difference of large numbers.  What the fold itself costs is the subtraction of
 * mean * c[n] from the accumulated x.Wg: a row whose |mean| is much larger than its spread loses log2(|mean| / spread)
 * bits there (a residual stream is nowhere near: the synthetic model's rows sit below 1).  `cond_flag` (device int, may be
 * NULL) gets bit 1 (value 2) OR-ed in when a row has mean^2 > 1024 (var + eps) -- by rnamsm_row_stats_from_partials, or by
 * rnamsm_gemm_lnfold when it sums the rows itself; rnamsm_forward passes its err_flag and
 * the Python mirror then redoes that MSA with separate LayerNorm launches.  Results agree with LayerNorm -> Linear to fp32
 * rounding (different association; against an fp64 truth the two are equally far from it:
 * tests/analysis/ln_fold_numerics.py, tests/test_gpu_fullsize.py).
 *   rnamsm_ln_fold_weights     one-time preparation: Wg [N,K], c [N], d [N] from W [N,K], bias [N] (or NULL), gamma, beta [K]
 *                              (c and d are accumulated in double; c sums the ROUNDED Wg the GEMM will multiply)
 *   rnamsm_row_partials        row_partials of x [T, D] as it lies in memory (D % 32 == 0, D <= 1024): for an x that did
 *                              not come out of rnamsm_gemm_residual_stats (the embedding)
 *   rnamsm_gemm_residual_stats Cout = A W^T + bias + residual (K8: out_proj / fc2 + the residual add, modules.py:396) and
 *                              row_partials [N/32, M, 2] of the Cout it stores; requirements of rnamsm_gemm_bias_act_res
 *   rnamsm_row_stats_from_partials  row_stats [M, 2] = (mean, rstd) of the first M rows from row_partials [K/32, partials_ld, 2]
 *   rnamsm_gemm_lnfold         Cout[m,n] = act( (rstd[m] * (sum_k X[m,k] Wg[n,k] - mean[m] c[n]) + d[n]) * (n < scale_cols ? scale : 1) )
 *                              X [M,K] row stride ldx; row_stats [M, 2] or NULL = the block sums the rows it stages itself
 *                              (self-contained, variance as E[x^2] - mean^2, ~2.6 % slower); eps = ln_eps; requirements of
 *                              rnamsm_gemm_bias_act_res, scale_cols % 4 == 0
 * partials_ld = rows per slab of the row_partials buffer (>= M: a GEMM over the first M rows of a longer stream, as the
 * outputs-only forward runs them, addresses the buffer with its own slab stride) */
int rnamsm_ln_fold_weights(const float* W, const float* bias, const float* gamma, const float* beta, float* Wg,
                           float* cvec, float* dvec, int N, int K, void* stream);
int rnamsm_row_partials(const float* x, float* row_partials, int64_t T, int D, void* stream);
int rnamsm_gemm_residual_stats(const float* A, int64_t lda, const float* W, const float* bias, const float* residual,
                               int64_t ldr, float* Cout, int64_t ldc, int64_t M, int N, int K, float* row_partials,
                               int64_t partials_ld, int dtype, void* stream);
int rnamsm_row_stats_from_partials(const float* row_partials, int64_t partials_ld, int64_t M, int K, float eps,
                                   float* row_stats, int* cond_flag, void* stream);
int rnamsm_gemm_lnfold(const float* X, int64_t ldx, const float* Wg, const float* cvec, const float* dvec,
                       float ln_eps, const float* row_stats, int* cond_flag, float* Cout, int64_t ldc, int64_t M,
                       int N, int K, int act, float scale, int scale_cols, int dtype, void* stream);

/* K2/K3/K8 -- nn.Linear with fused epilogue (modules.py:760-766, 794-799, 896-905, 923, 424-426, 396):
 *   Cout[m,n] = act( (sum_k A[m,k]*W[n,k] + bias[n]) * (n < scale_cols ? scale : 1) ) + residual[m,n]
 * A [M,K] row stride lda; W [N,K] contiguous (torch Linear layout); bias [N] or NULL;
 * residual [M,N] row stride ldr or NULL; Cout [M,N] row stride ldc (may alias residual).
 * Requires N % 128 == 0, K % 32 == 0, lda/ldr/ldc % 4 == 0 and 16-byte aligned pointers.
 * zero_rows (uint8 [M], may be NULL): rows flagged 1 get 0 in the scaled columns -- the reference's
 * `q *= 1 - padding_mask` (modules.py:767-772).
 * dtype: RNAMSM_F32 only (RNAMSM_ERR_UNSUPPORTED otherwise); the 16-bit modes of the same Linear are rnamsm_gemm_bf16. */
int rnamsm_gemm_bias_act_res(const float* A, int64_t lda, const float* W, const float* bias,
                             const float* residual, int64_t ldr, float* Cout, int64_t ldc,
                             int64_t M, int N, int K, int act, float scale, int scale_cols,
                             const uint8_t* zero_rows, int dtype, void* stream);

/* K2 with a per-row factor on the scaled columns (the general form of zero_rows):
 *   Cout[m, n] = ((A W^T + bias)[m, n] * scale) * row_factor[m]   for n < scale_cols,   (A W^T + bias)[m, n] elsewhere.
 * The QKV projection of a RAGGED batch (rnamsm_forward_batch with true_rows): a token's q is scaled by dh^-1/2 and by
 * 1/sqrt(the true depth of ITS alignment) (align_scaling, modules.py:713-715) and zeroed at <pad> (q *= 1 - padding_mask,
 * modules.py:767-772) -- row_factor (float [M], device) carries both.  No activation, no residual.  dtype: RNAMSM_F32 only. */
int rnamsm_gemm_row_scaled(const float* A, int64_t lda, const float* W, const float* bias, float* Cout, int64_t ldc, int64_t M,
                           int N, int K, float scale, int scale_cols, const float* row_factor, int dtype, void* stream);

/* Linear on the bf16 matrix cores (fp32 accumulate, fp32 activations in HBM), same epilogue as above.
 *   split = 1: operands rounded to bf16 (mixed-precision mode, BASELINE config 4);
 *   split = 3: both operands as hi + lo pairs, product = hi*hi + hi*lo + lo*hi, fp32 accumulation; opt-in fast mode, the
 *              exact-fp32 kernel stays the default.
 *   fmt   = 0: bf16 halves (split 1 only: split 3 with fmt 0, "bf16x3", was removed -> RNAMSM_ERR_UNSUPPORTED);
 *   fmt   = 1 (split 3 only): fp16 halves, "f16x3": a hi/lo fp16 pair carries ~22 mantissa bits (fp32: 24) for operands
 *              inside fp16 range (|x| < 65504).
 * W_hi / W_lo [N, K] are bf16 planes produced once by rnamsm_split_bf16 (lo = bf16(w - hi); may be NULL there
 * and here when split = 1); A is split while it is staged.  Requires N % 128 == 0, K % 64 == 0. */
int rnamsm_split_bf16(const float* src, uint16_t* hi, uint16_t* lo, int64_t n, int fmt, void* stream);
int rnamsm_gemm_bf16(const float* A, int64_t lda, const uint16_t* W_hi, const uint16_t* W_lo, const float* bias,
                     const float* residual, int64_t ldr, float* Cout, int64_t ldc, int64_t M, int N, int K,
                     int act, float scale, int scale_cols, int split, int fmt,
                     const uint16_t* A_hi, const uint16_t* A_lo, uint16_t* O_hi, uint16_t* O_lo, void* stream);
/* K1 folded in the 16-bit modes (same scheme as rnamsm_gemm_lnfold / rnamsm_gemm_residual_stats above; 256x256-tile kernels:
 * M >= 2048, N % 256 == 0, K % 64 == 0):
 *   rnamsm_gemm16_lnfold          O planes = act( (rstd[m] (sum_k X[m,k] Wg[n,k] - mean[m] c[n]) + d[n]) * colscale ): X planes hold
 *                                 the RAW residual stream, Wg planes = rnamsm_split_bf16(W * gamma), c[n] = the row sums of the
 *                                 Wg planes' values (hi + lo), d = bias + W beta; row_stats [M,2] from
 *                                 rnamsm_row_stats_from_partials.  Output as planes (the QKV / fc1 shapes).
 *   rnamsm_gemm16_residual_stats  x[m,:] += A W^T + bias in place (fp32 residual stream, out_proj / fc2), the new x written
 *                                 once more as 16-bit planes X_hi/X_lo [M, ldp] (the next rnamsm_gemm16_lnfold's operand) and
 *                                 its slab sums left in row_partials [N/32, partials_ld, 2]. */
int rnamsm_gemm16_lnfold(const uint16_t* X_hi, const uint16_t* X_lo, int64_t ldx, const uint16_t* Wg_hi,
                         const uint16_t* Wg_lo, const float* cvec, const float* dvec, const float* row_stats,
                         uint16_t* O_hi, uint16_t* O_lo, int64_t ldo, int64_t M, int N, int K, int act, float scale,
                         int scale_cols, int split, int fmt, void* stream);
int rnamsm_gemm16_residual_stats(const uint16_t* A_hi, const uint16_t* A_lo, int64_t lda, const uint16_t* W_hi,
                                 const uint16_t* W_lo, const float* bias, float* x, int64_t ldx, int64_t M, int N,
                                 int K, int split, int fmt, uint16_t* X_hi, uint16_t* X_lo, int64_t ldp,
                                 float* row_partials, int64_t partials_ld, void* stream);
/* LayerNorm (K1) whose output is written as 16-bit hi/lo planes [T, D] (lo may be NULL), the pre-split A operand of
 * rnamsm_gemm_bf16: with A_hi/A_lo given (row stride lda halves) A is ignored and no conversion runs in the GEMM;
 * with O_hi/O_lo given (fc1: GELU; QKV: no activation; never with a residual) the result is written as planes with row stride ldc for the next
 * GEMM instead of fp32 Cout. */
int rnamsm_layernorm_split(const float* x, const float* gamma, const float* beta, uint16_t* hi, uint16_t* lo,
                           int64_t T, int D, float eps, int fmt, void* stream);

/* K4 -- tied row-attention logits, RowSelfAttention.compute_attention_weights (modules.py:752-786):
 *   S[h,i,j] = sum_{r,d} q[r,i,h,d] * k[r,j,h,d]      (q already scaled by dh^-0.5/sqrt(R), K3)
 * q, k: element (r,i,h,d) at ptr[(r*C+i)*ld + h*64 + d]  (head_dim is 64).
 * The sum over rows is split into `nsplit` contiguous row ranges (rnamsm_row_logits_nsplit);
 * partial [nsplit, H, C, C] holds one slab per range and K5 adds them in range order, so the
 * result does not depend on scheduling.  This replaces the reference's chunk-and-sum
 * _batched_forward (modules.py:717-750): same sum, fixed order. */
int rnamsm_row_logits_nsplit(int R, int C, int H);
size_t rnamsm_row_logits_workspace_bytes(int R, int C, int H);
int rnamsm_row_logits(const float* q, const float* k, int64_t ld, float* partial,
                      int R, int C, int H, int head_dim, int dtype, void* stream);

/* K5 -- softmax over the last axis of the summed logits (modules.py:818 / 739):
 *   probs[h,i,:] = softmax_j( sum_s partial[s,h,i,:] ).  probs [H, C, C] is the layer's
 *   row_attentions slab (model.py:392).  key_mask (uint8 [C], may be NULL): keys flagged 1 have their summed
 *   logit replaced by -10000 first (masked_fill with padding_mask[:, 0], modules.py:781-785). */
int rnamsm_softmax_rows(const float* partial, int nsplit, float* probs, int H, int C,
                        const uint8_t* key_mask, void* stream);
/* The same with the summed logits multiplied by logit_scale (0 < logit_scale <= 1) before the mask fill and the softmax.  This is
 * where the exact path applies align_scaling's 1/sqrt(R) (modules.py:713-715) since round 5: q leaves the QKV epilogue scaled by
 * dh^-1/2 only, in rnamsm_forward, rnamsm_forward_batch and rnamsm_forward_packed alike, so that an alignment's outputs are the
 * same bits whatever batch it is computed in (the reference's loop is list-independent, RNA_MSM_Inference.py:141-166). */
int rnamsm_softmax_rows_scaled(const float* partial, int nsplit, float* probs, int H, int C, const uint8_t* key_mask,
                               float logit_scale, void* stream);

/* K4 / K5 with padding on the reference's CHUNKED path (RowSelfAttention._batched_forward, modules.py:717-750, taken when
 * R*C > max_tokens_per_msa): the rows are processed in chunks of max_rows = max(1, max_tokens_per_msa / C) (:724), every
 * chunk's logits are filled with -10000 where the chunk's OWN first row is <pad> (:727-737 slice the mask per chunk,
 * :781-785 use its row 0) and the filled slabs are added in chunk order (:738).  With padding this differs from the direct
 * path: a pad on a chunk-starting row masks that key column, and an all-padded chunk start shifts every logit by -10000.
 *   rnamsm_row_chunks            number of chunks, 0 when the reference takes the direct path (R*C <= max_tokens_per_msa)
 *   rnamsm_row_logits_chunked    rnamsm_row_logits with one partial slab per chunk: partial [nchunks, H, C, C]
 *   rnamsm_softmax_rows_chunked  probs = softmax_j( sum_c (pad_mask[c*rows_per_chunk, j] ? -10000 : partial[c,h,i,j]) );
 *                                pad_mask uint8 [R, C] (rnamsm_pad_mask). */
int rnamsm_row_chunks(int R, int C, int max_tokens_per_msa);
int rnamsm_row_logits_chunked(const float* q, const float* k, int64_t ld, float* partial, int R, int C, int H,
                              int head_dim, int rows_per_chunk, int dtype, void* stream);
int rnamsm_softmax_rows_chunked(const float* partial, int nchunks, float* probs, int H, int C,
                                const uint8_t* pad_mask, int rows_per_chunk, void* stream);

/* K6 -- RowSelfAttention.compute_attention_update's contraction (modules.py:797-798):
 *   ctx[r,i,h,:] = sum_j probs[h,i,j] * v[r,j,h,:]
 * v addressed like q/k above; ctx element (r,i,h,d) at ctx[(r*C+i)*ldc + h*64 + d].
 * With ctx_hi given the context is written instead as 16-bit hi (+ lo if non-NULL) planes with the same indexing
 * (plane_fmt 0 = bf16, 1 = fp16): the pre-split A operand of rnamsm_gemm_bf16 for the following out_proj.
 * dtype: RNAMSM_F32 only; the 16-bit modes are rnamsm_row_apply16 (and rnamsm_row_logits16 / rnamsm_softmax_rows_planes for
 * K4 / K5, whose fp32 entry points rnamsm_row_logits[_chunked] likewise take RNAMSM_F32 only). */
int rnamsm_row_apply(const float* probs, const float* v, int64_t ld, float* ctx, int64_t ldc,
                     int R, int C, int H, int head_dim, uint16_t* ctx_hi, uint16_t* ctx_lo, int plane_fmt,
                     int dtype, void* stream);

/* K7 -- ColumnSelfAttention.compute_attention_update's attention (modules.py:905-921), fused:
 *   for every column c and head h: ctx[:,c,h,:] = softmax_j( q[:,c,h,:] k[:,c,h,:]^T ) v[:,c,h,:]
 * (q already scaled by dh^-0.5).  The [H,C,R,R] probabilities are never written (the reference
 * computes and discards them).  R == 1 degenerates to ctx = v (modules.py:882-894).
 * pad_mask (uint8 [R, C], may be NULL): scores of keys flagged 1 are replaced by -10000 (modules.py:911-915).
 * ctx_hi / ctx_lo / plane_fmt: optional 16-bit plane output as for rnamsm_row_apply (not with pad_mask).
 * dtype: RNAMSM_F32 only; the 16-bit modes are rnamsm_col_attn16. */
int rnamsm_col_attn_fused(const float* q, const float* k, const float* v, int64_t ld,
                          float* ctx, int64_t ldc, int R, int C, int H, int head_dim,
                          const uint8_t* pad_mask, uint16_t* ctx_hi, uint16_t* ctx_lo, int plane_fmt,
                          int dtype, void* stream);

/* K7 restricted to the query rows [0, q_rows) of every column (keys / values: all R rows): what the LAST layer needs when
 * only alignment row 0 of the final representation is wanted (rnamsm_forward without RNAMSM_OUT_REPR).  Row i of ctx is
 * written for i < q_rows only and equals rnamsm_col_attn_fused's row i bit for bit.
 * dtype: RNAMSM_F32 only. */
int rnamsm_col_attn_fused_queries(const float* q, const float* k, const float* v, int64_t ld, float* ctx, int64_t ldc,
                                  int R, int C, int H, int head_dim, int q_rows, const uint8_t* pad_mask, int dtype,
                                  void* stream);

/* K7 on PRESCALED q (round 4): q already carries dh^-1/2 * log2(e) (the scale / scale_cols of the QKV GEMM's epilogue), so the
 * scores are in log2 units and the kernel's first pass needs no running maximum -- p = exp2(s) on the raw score, no max chain, no
 * rescale of the accumulators (softmax does not depend on the reference point and fp32 keeps its relative precision at any
 * scale); a wave (32 query rows) whose row sums leave [2^-64, 2^100] (a score outside fp32's exponent range) redoes its rows with
 * the online softmax in log2 units (round 5: per wave, not per 128-query block -- a row's arithmetic does not depend on its block mates).  No mask, fp32 context; q_rows as in rnamsm_col_attn_fused_queries (q_rows == R: all rows).  Results
 * equal rnamsm_col_attn_fused on q / log2(e) to fp32 rounding.  What rnamsm_forward / _batch / _packed call on the exact path
 * when the MSA has no padding.  Knob "col_fast" = 0 keeps the online softmax only (A/B). */
int rnamsm_col_attn_fused_prescaled(const float* q, const float* k, const float* v, int64_t ld, float* ctx, int64_t ldc,
                                    int R, int C, int H, int head_dim, int q_rows, void* stream);

/* K7's probabilities, materialised on request -- ColumnSelfAttention's second return value (modules.py:905-917 builds
 * attn_probs [H, C, B, R, R]; :926-945 returns it; AxialTransformerLayer.forward hands it on, :253-267):
 *   probs[((h*C + c)*R + i)*R + j] = softmax_j( scale * q[i,c,h,:] . k[j,c,h,:]   [-10000 where pad_mask[j*C + c]] )
 * i.e. the reference's tensor for B = 1, contiguous.  The fused kernels above never form it (H*C*R*R floats: 1.6 GB per
 * layer at R = 256, C = 512); callers that read it (rnamsm.modules.ColumnSelfAttention(return_probs=True)) pay for it
 * here.  q, k addressed like rnamsm_col_attn_fused's; the fp32 form takes q as the QKV GEMM left it (already scaled by
 * dh^-0.5: pass scale = 1), the plane form takes the 16-bit modes' unscaled q planes (scale = dh^-0.5; *_lo may be NULL
 * together; fmt 0 = bf16, 1 = fp16; ld in halves).  R == 1 gives ones, as modules.py:882-891.
 * dtype: RNAMSM_F32 only. */
int rnamsm_col_attn_probs(const float* q, const float* k, int64_t ld, float* probs, int R, int C, int H, int head_dim,
                          const uint8_t* pad_mask, float scale, int dtype, void* stream);
int rnamsm_col_attn_probs16(const uint16_t* q_hi, const uint16_t* q_lo, const uint16_t* k_hi, const uint16_t* k_lo,
                            int64_t ld, float* probs, int R, int C, int H, int head_dim, const uint8_t* pad_mask, int fmt,
                            float scale, void* stream);

/* K4' / K5' / K6' / K7' -- the attention contractions of the 16-bit modes (same reference lines as K4..K7).  Operands
 * are 16-bit planes in HBM, addressed like their fp32 counterparts (element (r,c,h,d) = plane[(r*C+c)*ld + h*64 + d],
 * ld in halves): q/k/v as written by rnamsm_gemm_bf16's plane epilogue (O_hi/O_lo over the fused [T,3D] QKV output),
 * P as written by rnamsm_softmax_rows_planes.  All *_lo NULL = bf16 operands, one MFMA per product (fmt must be 0);
 * all *_lo given = hi/lo pairs, three MFMAs per product (fmt must be 1 = f16x3, fp32-grade; fmt 0 with lo planes -- bf16x3 -- was removed).
 * Accumulation, softmax and the partial-slab sum stay fp32.  Padding masks (f2): rnamsm_zero_plane_rows on the q
 * planes, key_mask in rnamsm_softmax_rows_planes, pad_mask in rnamsm_col_attn16. */
/* Scaling is applied to fp32 accumulators, never to 16-bit operands (a q scaled by ~1e-2 or a probability ~1e-3 would
 * push its fp16 lo plane into subnormals): q arrives UNSCALED and `scale` multiplies the logits; P planes hold
 * P * plane_scale (a power of two, 4096 in rnamsm_forward) and out_scale = 1 / plane_scale undoes it. */
/* Row split of rnamsm_row_logits16 for split = 1 (hi planes only) or 3 (hi/lo pairs); it may differ from
 * rnamsm_row_logits_nsplit (large C in the hi/lo modes uses a 256x256 tile with its own split), and the size of a
 * partial buffer that fits either tiling. */
int rnamsm_row_logits16_nsplit(int R, int C, int H, int split);
size_t rnamsm_row_logits16_workspace_bytes(int R, int C, int H);
int rnamsm_row_logits16(const uint16_t* q_hi, const uint16_t* q_lo, const uint16_t* k_hi, const uint16_t* k_lo,
                        int64_t ld, float* partial, int R, int C, int H, int head_dim, float scale, int fmt,
                        void* stream);
/* rnamsm_softmax_rows that also writes P * plane_scale as planes [H*C, ldp] (ldp = C rounded up to 64, tail zeroed). */
int rnamsm_softmax_rows_planes(const float* partial, int nsplit, float* probs, uint16_t* p_hi, uint16_t* p_lo,
                               int64_t ldp, float plane_scale, int H, int C, const uint8_t* key_mask, int fmt,
                               void* stream);
/* ctx = out_scale * P v as fp32 (ctx_hi NULL) or as ctx_hi(+ctx_lo) planes in the operands' format. */
int rnamsm_row_apply16(const uint16_t* p_hi, const uint16_t* p_lo, int64_t ldp, const uint16_t* v_hi,
                       const uint16_t* v_lo, int64_t ld, float* ctx, int64_t ldc, int R, int C, int H, int head_dim,
                       float out_scale, uint16_t* ctx_hi, uint16_t* ctx_lo, int fmt, void* stream);
/* ctx = softmax_j(scale * q k^T) v per (column, head); pad_mask (uint8 [R, C], may be NULL): scaled scores of keys
 * flagged 1 are replaced by -10000 (modules.py:911-915). */
int rnamsm_col_attn16(const uint16_t* q_hi, const uint16_t* q_lo, const uint16_t* k_hi, const uint16_t* k_lo,
                      const uint16_t* v_hi, const uint16_t* v_lo, int64_t ld, float* ctx, int64_t ldc, int R, int C,
                      int H, int head_dim, float scale, const uint8_t* pad_mask, uint16_t* ctx_hi, uint16_t* ctx_lo,
                      int fmt, void* stream);
/* The same for bf16 operand formats (plain bf16: lo planes NULL, or bf16 hi/lo pairs) without a padding mask, with q PRESCALED:
 * the q planes hold q * scale * log2(e) (scale = dh^-0.5), multiplied in BEFORE the rounding to 16 bits -- rnamsm_gemm_bf16's
 * epilogue does that for the q columns (scale, scale_cols) -- so the kernel's softmax is p = exp2(q'.k) with no multiply, no
 * reference subtraction and no pre-pass; a row sum outside [2^-96, 2^96] sends the block to the online-softmax loop.  This is
 * what rnamsm_forward runs in the bf16 modes. */
int rnamsm_col_attn16_prescaled(const uint16_t* q_hi, const uint16_t* q_lo, const uint16_t* k_hi, const uint16_t* k_lo,
                                const uint16_t* v_hi, const uint16_t* v_lo, int64_t ld, float* ctx, int64_t ldc, int R,
                                int C, int H, int head_dim, uint16_t* ctx_hi, uint16_t* ctx_lo, void* stream);
/* f2 in the 16-bit modes: zero the first ncols halves of the plane rows flagged in mask (uint8 [T]) -- q *= 1 -
 * padding_mask (modules.py:767-772) applied to the q planes after the QKV GEMM. */
int rnamsm_zero_plane_rows(uint16_t* hi, uint16_t* lo, const uint8_t* mask, int64_t T, int ncols, int64_t ld, void* stream);

/* f2 -- padding_mask = tokens.eq(pad_idx) (model.py:346): mask uint8 [n]. */
int rnamsm_pad_mask(const int64_t* tokens, uint8_t* mask, int64_t n, int pad_idx, void* stream);

/* K10 -- extract_feat's output section (RNA_MSM_Inference.py:151-166):
 *   emb[c-1, :]            = x_final[row 0, c, :]                c = 1..C-1      -> [C-1, D]
 *   atp[l*H+h, i-1, j-1]   = probs_all[l, h, i, j]               i,j = 1..C-1    -> [NL*H, C-1, C-1]
 * x_final [R*C, D] is the output of emb_layer_norm_after; probs_all [NL, H, C, C].
 * The embedding rows move as 16-byte vectors: D % 4 == 0, x_final and emb 16-byte aligned (refused with RNAMSM_ERR_INVALID
 * otherwise); probs_all / atp have no alignment requirement. */
int rnamsm_pack_outputs(const float* x_final, const float* probs_all, float* emb, float* atp,
                        int C, int D, int num_layers, int H, void* stream);

/* f1 -- contact head on the stacked row attentions (ContactPredictionHead.forward, modules.py:344-366 with
 * symmetrize/apc, utils/tensor.py:98-113; model.py:412-414): row_attn [nch = L*H, C, C] (with <cls>) ->
 * contacts [C-1, C-1] = sigmoid(regression(apc(symmetrize(row_attn[:, 1:, 1:])))).  weight [nch], bias [1].
 * The workspace after the call, for this entry, rnamsm_contact_head_atp and rnamsm_contact_head_long alike (T = C - 1 or L): floats
 * rs [nch, T] -- rs[ch, i] = sum_j (X[i, j] + X[j, i]), the row sum of the symmetrised channel -- then tot [nch] = sum_i rs[ch, i],
 * and nothing else; a packed call leaves each member's rs and tot in that member's slab (below).  The tests read the stages there. */
size_t rnamsm_contact_head_workspace_bytes(int C, int nch);
int rnamsm_contact_head(const float* row_attn, const float* weight, const float* bias, float* contacts,
                        void* workspace, size_t workspace_bytes, int C, int nch, void* stream);

/* f1 on the stripped maps -- the same head on atp [nch, L, L], the maps as rnamsm_pack_outputs leaves them (<cls> gone):
 * plane p at atp + p * plane_stride, rows of L floats (stride L*L for the packed [nch, L, L]; a larger stride reads the planes of
 * a wider buffer in place, and nothing between the planes is read).  contacts [L, L].  workspace:
 * rnamsm_contact_head_workspace_bytes(L + 1, nch) bytes -- rs [nch, L], then tot [nch].
 * The kernels are those of rnamsm_contact_head with the layout as a parameter, and every sum keeps its order, so contacts are
 * BIT-IDENTICAL to rnamsm_contact_head on the [nch, L+1, L+1] maps whose [1:, 1:] part holds the same values.
 * Refused (RNAMSM_ERR_INVALID) before anything is enqueued: a null pointer, L outside [1, RNAMSM_CONTACT_MAX_L], nch <= 0,
 * plane_stride < L * L, atp, contacts or workspace not 4-byte aligned (the checks of rnamsm_contact_head_long, in its order: the
 * two entries are one function under two names and limits; a pointer the library or an allocator hands out is always aligned), a
 * short workspace. */
#define RNAMSM_CONTACT_MAX_L 1023
int rnamsm_contact_head_atp(const float* atp, int64_t plane_stride, int L, int nch, const float* weight, const float* bias,
                            float* contacts, void* workspace, size_t workspace_bytes, void* stream);

/* f1, several alignments per launch -- rnamsm_contact_head_atp over B maps of unlike L in ONE launch set: the row sums over
 * sum_b ceil(L_b / 256) x nch blocks, the totals of the members of L > 256 (skipped where there is none), the regression over
 * sum_b ceil(L_b / 32)^2 blocks -- each member's own blocks, never B x the longest member's -- and a block finds its member in a
 * device descriptor table.
 * The contract: a member's [L, L] contacts are BIT-IDENTICAL to rnamsm_contact_head on that alignment's [nch, L+1, L+1] maps
 * alone, whatever its company, its place in the batch and its plane stride.  Each member's workspace slab holds its rs and tot
 * and is its own: a non-finite member never reaches a neighbour.  Nothing is written behind the last slab.
 * items: a HOST array of B entries, read during the call and free to go afterwards (the descriptors travel as kernel arguments
 * on `stream`); the members' maps may be slices of one buffer, their contacts must not overlap.
 * workspace: rnamsm_contact_head_packed_workspace_bytes(B, Ls, nch) bytes, 16-byte aligned, caller-owned (nothing is allocated
 * inside): the descriptor table (64 bytes per member, rounded up to 256), then the members' slabs in order -- member b's is the
 * lone call's workspace at the sum of the slabs before it.  The size is 0 for B outside [1, RNAMSM_CONTACT_MAX_BATCH], a null Ls,
 * an L outside [1, RNAMSM_CONTACT_MAX_L] or nch <= 0.  Its contents on entry do not matter.
 * Refused (RNAMSM_ERR_INVALID) before anything is enqueued, rnamsm_last_error naming the member where one is at fault: B out of
 * range, nch <= 0, a null pointer (items, weight, bias, workspace, a member's atp or contacts), a member's L out of range, its
 * plane_stride < L * L, a member pointer that is not 4-byte aligned, a workspace that is short or not 16-byte aligned.
 * No atomics: the same inputs give the same bits on every run. */
typedef struct {                 /* one alignment of the batch */
    const float* atp;            /* device: plane p at atp + p * plane_stride, [L, L] row-major */
    int64_t      plane_stride;   /* >= L * L */
    int32_t      L;              /* 1 .. RNAMSM_CONTACT_MAX_L */
    float*       contacts;       /* device [L, L] */
} rnamsm_contact_item;
#define RNAMSM_CONTACT_MAX_BATCH 1024
size_t rnamsm_contact_head_packed_workspace_bytes(int B, const int* Ls, int nch);
int rnamsm_contact_head_packed(const rnamsm_contact_item* items, int B, int nch, const float* weight, const float* bias,
                               void* workspace, size_t workspace_bytes, void* stream);

/* f4 -- LM head on CHOSEN ROWS of a feature buffer (RobertaLMHead.forward, modules.py:303-319, plus the log-softmax and the
 * wild-type subtraction of utils/likelihood.py), exact fp32.  For every selected row i of a member:
 *   h      = gelu_erf(x_i . Wd^T + bd)                 Wd [D, D]
 *   y      = LayerNorm(h; gamma, beta, eps)
 *   logits = y . Wp^T + bp                             Wp [V, D]: the tied embed_tokens rows as they are (no padding)
 *   logp   = logits - logsumexp(logits)                max-subtracted
 *   scores = logp - logp[wt_i]                         nll = -logp[wt_i]
 * x_i = x + (rows ? rows[i] : i) * ld, D floats: the gather happens in the kernel, a row that is not selected is never read and
 * nothing is staged through a contiguous copy.  rows[i] is device data and is trusted: it must name a row of the caller's buffer.
 * wt_i outside [0, V) is device data too and cannot be refused: that row's scores and nll are NaN, its logits and logp are what
 * they would have been, and no index is formed from it.
 * Two launches: the dense step on v_mfma_f32_32x32x2_f32 over (32-row tile) x (64-column tile) blocks with k in a fixed order (chains of 32 k,
 * their sums added in ascending order), h into the workspace; then one wave per row for the LayerNorm, the V dot products and the log-softmax.  No atomics.  A
 * row's result depends on that row's D values and the weights and on nothing else -- not on n, its position, its neighbours or
 * the company in a packed call: a member of rnamsm_lm_head_packed has the BITS of rnamsm_lm_head on it alone, and a row selected
 * twice gives the same bits twice.
 * weights: HOST table of RNAMSM_LM_NUM_WEIGHTS device pointers, 16-byte aligned: dense W [D, D], dense b [D], LayerNorm gamma [D],
 * beta [D], projection W [V, D], projection b [V].
 * Each of the four outputs may be NULL; what is NULL is neither computed nor written.
 * workspace: rnamsm_lm_head_workspace_bytes(n, D) = n * D floats (h); packed: two descriptor tables of B entries (each padded to
 * 256 bytes), then the members' slabs back to back -- rnamsm_lm_head_packed_workspace_bytes(B, ns, D).  16-byte aligned,
 * caller-owned, contents on entry do not matter; only a member's own n * D floats are written.  A size is 0 for arguments outside
 * the limits.
 * Refused (RNAMSM_ERR_INVALID) before anything is enqueued, rnamsm_last_error naming the member where one is at fault: a null
 * pointer (item(s), weights, a weight, workspace, a member's x), D not a multiple of 64 in [64, RNAMSM_LM_MAX_D], V outside
 * [1, RNAMSM_LM_MAX_V], B outside [1, RNAMSM_LM_MAX_BATCH], n < 1, the sum of n above RNAMSM_LM_MAX_ROWS, ld < D, x not 16-byte
 * aligned or ld not a multiple of 4 (rows are read as 16-byte vectors), rows / wt / an output not 4-byte aligned, scores or nll
 * asked without wt, every output NULL, a short or misaligned workspace. */
#define RNAMSM_LM_MAX_D 1024
#define RNAMSM_LM_MAX_V 64
#define RNAMSM_LM_MAX_BATCH 1024
#define RNAMSM_LM_MAX_ROWS 16777216
#define RNAMSM_LM_NUM_WEIGHTS 6
typedef struct {                 /* one member: n chosen rows of one feature buffer */
    const float*   x;            /* device: row r at x + r * ld, D floats */
    int64_t        ld;           /* row pitch in floats, >= D, a multiple of 4 */
    const int32_t* rows;         /* device int32 [n], or NULL: rows 0 .. n-1 */
    const int32_t* wt;           /* device int32 [n] (the wild-type token of every row), or NULL */
    int32_t        n;            /* >= 1 */
    float*         logits;       /* device [n, V], or NULL */
    float*         logp;         /* device [n, V], or NULL */
    float*         scores;       /* device [n, V], or NULL; needs wt */
    float*         nll;          /* device [n], or NULL; needs wt */
} rnamsm_lm_item;
size_t rnamsm_lm_head_workspace_bytes(int n, int D);
int rnamsm_lm_head(const rnamsm_lm_item* item, int D, int V, const float* const* weights, float eps, void* workspace,
                   size_t workspace_bytes, void* stream);
size_t rnamsm_lm_head_packed_workspace_bytes(int B, const int* ns, int D);
int rnamsm_lm_head_packed(const rnamsm_lm_item* items, int B, int D, int V, const float* const* weights, float eps, void* workspace,
                          size_t workspace_bytes, void* stream);

/* Long alignments -- the outputs of overlapping windows blended into full-length emb / atp.  An alignment of
 * L > W body columns (W = max_seqlen - 1) runs as n = ceil((L - W) / stride) + 1 forwards over windows of W columns: window k
 * starts at s_k = k * stride, the last one at L - W; stride in [ceil(W / 2), W].  Blend weight of window k at its local column
 * i in [0, W), ramp = W - stride: u = 1 where ramp == 0, else (float)min(left, right, ramp) / (float)ramp, left = ramp in the
 * first window, else i + 1, right = ramp in the last window, else W - i (one IEEE fp32 division; never zero).
 *   rows   out[p, d]    = (sum_k u_k(p) x_k[p - s_k, d]) / (sum_k u_k(p))
 *   pairs  out[h, p, q] = (sum_k (u_k(p) u_k(q)) a_k[h, p - s_k, q - s_k]) / (sum_k u_k(p) u_k(q))
 * over the windows that contain p (pairs: p and q), ascending, starting from the first term; all fp32, every product, sum and
 * quotient rounded on its own (no fused multiply-add, no reciprocal).  A pair no window contains is +0.0.
 * One call applies the windows k0 .. k0 + nb - 1, which lie win_stride floats apart: one window of a one-by-one run (nb = 1), or
 * all windows of a batched forward.  The calls of an alignment come in ascending k0 on one stream and together apply every window
 * once; between them `out` holds running sums.  After the last call every element of `out` is defined, whatever it held before
 * the first, and a NaN / inf of a window has reached exactly the elements that window covers.
 *   rnamsm_stitch_rows   x: window w of the call, local row i at x + w * win_stride + i * ld, D floats (ld >= D: rows inside a
 *                        wider buffer are read in place); out [L, D].
 *   rnamsm_stitch_pairs  a: element (h, i, j) of window w at a + w * win_stride + h * plane_stride + (i + off) * ld + (j + off)
 *                        -- off = 0, ld = W for the stripped atp [H, W, W]; off = 1, ld = W + 1 for maps that still carry <cls>,
 *                        as rnamsm_contact_head reads them; out [H, L, L].
 * One launch per call on the caller's stream, no workspace, no allocation, no atomics: every element of `out` is written by at
 * most one thread, and the same inputs give the same bits on every run.  rnamsm_stitch_num_windows: n, or 0 for an (L, W, stride)
 * the stitcher refuses.
 * Refused (RNAMSM_ERR_INVALID) before anything is enqueued: a null pointer, L <= W, W < 1, L above RNAMSM_STITCH_MAX_L, a stride
 * outside [ceil(W / 2), W] (rnamsm_last_error names the bounds), k0 / nb outside the plan, D < 1, ld < D (pairs: ld < W + off,
 * off < 0), H outside [1, RNAMSM_STITCH_MAX_H], a plane or window stride below the extent of what it steps over, a pointer that
 * is not 4-byte aligned. */
#define RNAMSM_STITCH_MAX_L (1 << 19)
#define RNAMSM_STITCH_MAX_H (1 << 16)
int rnamsm_stitch_num_windows(int L, int W, int stride);
int rnamsm_stitch_rows(const float* x, int64_t win_stride, int64_t ld, int L, int W, int stride, int k0, int nb, int D, float* out,
                       void* stream);
int rnamsm_stitch_pairs(const float* a, int64_t win_stride, int64_t plane_stride, int64_t ld, int off, int L, int W, int stride,
                        int k0, int nb, int H, float* out, void* stream);

/* f4 -- RNA-MSM-SS secondary-structure head (_downstream_tasks/SS: predict.py, code/model.py ResNet._forward_impl with
 * num_blocks BasicBlocks; renet_b16 = 16) on the attention maps of one alignment, exact fp32:
 *   in[c, i, j] = onehot(seq[i])[c] (c < 4), onehot(seq[j])[c-4] (c < 8), atp[c-8, i, j] (c < 128)     i, j < L
 *   x = conv3x3(in) + b;  per block x = x + conv5x5(relu(LN2(conv3x3(relu(LN1(x))))));  logits = fc1(relu(LN(x)))
 *   probs = sigmoid(logits)                                                    logits / probs [L, L] row-major, i = row
 * atp: plane p (= layer * 12 + head) at atp + p * atp_plane_stride, rows of L floats (the [120, L, L] of rnamsm_pack_outputs:
 * stride L*L; a larger stride reads the planes of a wider buffer in place).  base_codes [L]: 0..3 = A, C, G, U; any other
 * value is the all-zero one-hot vector (the reference encoder's handle_unknown='ignore').
 * weights: RNAMSM_SS_GLOBAL_WEIGHTS + RNAMSM_SS_WEIGHTS_PER_BLOCK * num_blocks pointers in the reference's state_dict order:
 *   [0] conv1.weight  [3][3][48 out][128 in]     [1] conv1.bias [48]     [2] bn1.weight [48]     [3] bn1.bias [48]
 *   per block k, at 4 + 6k:  layer1.k.conv1.weight [3][3][48][48], layer1.k.bn1.weight, .bias [48],
 *                            layer1.k.conv2.weight [5][5][48][48], layer1.k.bn2.weight, .bias [48]
 *   last two: fc1.weight [48], fc1.bias [1]
 * (bn1 is the LayerNorm after the blocks; conv weights are the torch [out][in][kh][kw] tensors repacked tap-major
 * [kh][kw][out][in]); every weight pointer 16-byte aligned.  Either of logits / probs may be null, not both.
 * workspace: rnamsm_ss_head_workspace_bytes(L) bytes (two [L*L, 48] fp32 images), 16-byte aligned; 0 for an L outside
 * [1, RNAMSM_SS_MAX_L].  Refused (RNAMSM_ERR_INVALID): L outside [1, RNAMSM_SS_MAX_L], num_blocks outside
 * [1, RNAMSM_SS_MAX_BLOCKS], atp_plane_stride < L*L, a null or misaligned pointer, a short workspace.
 * A NaN or an inf in atp is not refused: it comes out as NaN exactly where the reference network gives NaN (every ReLU carries
 * a NaN on, as nn.ReLU does) -- the pixels within 1 + 3 num_blocks of it -- and every other pixel keeps the bits it has without it.
 * No atomics: the same inputs give the same bits on every run. */
#define RNAMSM_SS_MAX_L 1024
#define RNAMSM_SS_MAX_BLOCKS 64
#define RNAMSM_SS_GLOBAL_WEIGHTS 6
#define RNAMSM_SS_WEIGHTS_PER_BLOCK 6
size_t rnamsm_ss_head_workspace_bytes(int L);
int rnamsm_ss_head(const float* atp, int64_t atp_plane_stride, const uint8_t* base_codes, int L, int num_blocks,
                   const float* const* weights, float* logits, float* probs, void* workspace, size_t workspace_bytes,
                   void* stream);

/* f4, several structures per launch -- rnamsm_ss_head over B structures of unlike length in ONE set of launches (stem,
 * num_blocks x (3x3 + 5x5), output pass).  Every launch covers sum_b ceil(L_b / 16)^2 blocks -- each member's own tiles,
 * never B x the largest member's -- and a block finds its member in a device descriptor table.  A tile's arithmetic is the lone
 * call's (the same device functions on the member's own image and L), so every member's logits / probs are BIT-IDENTICAL to
 * rnamsm_ss_head on that member alone, whatever its company and its place in the batch.
 * items: a HOST array of B entries, read during the call and free to go afterwards (the descriptors travel as kernel
 * arguments on `stream`).  Per member: atp / atp_plane_stride / base_codes / L / logits / probs as for rnamsm_ss_head; the
 * members' maps may be slices of one buffer (the atp of rnamsm_forward_packed), their outputs must not overlap.
 * weights, num_blocks: exactly those of rnamsm_ss_head.
 * workspace: rnamsm_ss_head_packed_workspace_bytes(B, Ls) bytes, 16-byte aligned, caller-owned (nothing is allocated inside):
 * the descriptor table (64 bytes per member, rounded up to 256), then the two NHWC [sum L_b^2, 48] fp32 images; member b's
 * image starts at pixel sum_{a<b} L_a^2.  The size is 0 for B outside [1, RNAMSM_SS_MAX_BATCH], a null Ls or an L outside
 * [1, RNAMSM_SS_MAX_L].
 * Refused (RNAMSM_ERR_INVALID) before anything is enqueued, rnamsm_last_error naming the member where one is at fault: B or
 * num_blocks out of range, a member's L out of range, a null pointer (items, weights, workspace, a member's atp or
 * base_codes, a weight), a member with neither logits nor probs, a float pointer that is not 4-byte aligned, a weight pointer
 * or workspace that is not 16-byte aligned, atp_plane_stride < L*L, a short workspace.
 * A non-finite input comes out as NaN exactly where the reference network gives NaN, as for rnamsm_ss_head, and a member never
 * affects another: the neighbours of a poisoned member stay finite and keep their bits.
 * No atomics: the same inputs give the same bits on every run. */
typedef struct {                 /* one structure of the batch */
    const float*   atp;          /* device: plane p at atp + p * atp_plane_stride, rows of L floats */
    int64_t        atp_plane_stride;   /* >= L*L */
    const uint8_t* base_codes;   /* device, [L] */
    int32_t        L;            /* 1 .. RNAMSM_SS_MAX_L */
    float*         logits;       /* device [L, L] or null */
    float*         probs;        /* device [L, L] or null; not both null */
} rnamsm_ss_item;
#define RNAMSM_SS_MAX_BATCH 1024
size_t rnamsm_ss_head_packed_workspace_bytes(int B, const int* Ls);
int rnamsm_ss_head_packed(const rnamsm_ss_item* items, int B, int num_blocks, const float* const* weights,
                          void* workspace, size_t workspace_bytes, void* stream);

/* f4 in bf16 -- the SS head with its convolutions on the bf16 matrix cores (v_mfma_f32_16x16x32_bf16), opt-in: rnamsm_ss_head and
 * rnamsm_ss_head_packed keep their arithmetic and their bits.  The arithmetic contract:
 *   bf16, rounded to nearest even (NaN stays NaN, +-inf stays +-inf): the conv operands -- the stem's inputs (the 120 maps and the 8
 *     one-hot planes), each block's relu(LN(x)) activations (both convs), every conv weight;
 *   fp32: the accumulation of every conv, the residual image x (and the block's middle image), the LayerNorm statistics and affine,
 *     the stem bias, the output pass (final LN + ReLU + fc1 + sigmoid).
 *   Zero padding is of relu(LN(x)); every ReLU carries a NaN on; no atomics and one summation order per pixel, so the same inputs
 *   give the same bits on every run, and a member of a packed call has the bits of the lone bf16 call on it, whatever its company
 *   and place.  A non-finite input comes out as NaN exactly where the reference network gives NaN, as for rnamsm_ss_head.
 * Arguments, workspace sizes (the same two fp32 images) and refusals are those of rnamsm_ss_head / rnamsm_ss_head_packed, made
 * before anything is enqueued.  weights: the table of rnamsm_ss_head in which the conv entries ([0] and, per block, 4 + 6k and
 * 4 + 6k + 3) point to bf16 planes of the same tap-major shape [kh][kw][48 out][in]; every other entry is fp32 as before.
 * rnamsm_ss_pack_conv16 makes such planes on the device: out[i] = bf16(w[i]), i < n, from the fp32 tap-major weights (w 4-byte,
 * out 16-byte aligned; n in [1, 2^31]). */
int rnamsm_ss_pack_conv16(const float* w, uint16_t* out, int64_t n, void* stream);
size_t rnamsm_ss_head16_workspace_bytes(int L);
int rnamsm_ss_head16(const float* atp, int64_t atp_plane_stride, const uint8_t* base_codes, int L, int num_blocks,
                     const void* const* weights, float* logits, float* probs, void* workspace, size_t workspace_bytes,
                     void* stream);
size_t rnamsm_ss_head16_packed_workspace_bytes(int B, const int* Ls);
int rnamsm_ss_head16_packed(const rnamsm_ss_item* items, int B, int num_blocks, const void* const* weights,
                            void* workspace, size_t workspace_bytes, void* stream);

/* f4, the text of the probabilities -- the bytes np.savetxt(path, probs, delimiter="\t") writes for the [L, L] probabilities of
 * rnamsm_ss_head (the reference's `<name>.prob`), produced on the device: L*L records of 25 bytes, "%.18e" of the element (24
 * characters for every float32 in [0, 1]: d.dddddddddddddddddde-XX, the digits computed exactly in integers) and then '\t', or
 * '\n' behind the last column of a row.  rnamsm_ss_prob_text_bytes(L) = 25 L^2, or 0 for an L outside [1, RNAMSM_SS_MAX_L].
 * probs [L, L] fp32 row-major (device); text: rnamsm_ss_prob_text_bytes(L) bytes, 16-byte aligned (device); fallback: one int32
 * (device).  The call sets *fallback to 0 and then, from every thread that meets an element outside [0, 1] -- a set sign bit
 * (-0.0 included), a value above 1.0, a NaN, an inf -- to 1, with plain stores (no atomics): text is exact when the word reads 0
 * and unspecified when it reads 1 (the caller then formats that matrix on the host, where a NaN-poisoned map comes out as `nan`
 * fields).  Nothing is allocated inside the call and it takes no workspace.
 * Packed: B members in one call, every member's text and word exactly those of the lone call on it, whatever its company.  items:
 * a HOST array, read during the call and free to go afterwards (the descriptors travel as kernel arguments, 32 members per
 * launch).  Members may share a fallback word (it then reads 1 when any of them left the domain); their texts must not overlap.
 * Refused (RNAMSM_ERR_INVALID) before anything is enqueued, rnamsm_last_error naming the member where one is at fault: B outside
 * [1, RNAMSM_SS_MAX_BATCH], an L outside [1, RNAMSM_SS_MAX_L], a null pointer, probs or fallback not 4-byte aligned, text not
 * 16-byte aligned. */
typedef struct {                 /* one matrix of the batch */
    const float* probs;          /* device [L, L] */
    int32_t      L;              /* 1 .. RNAMSM_SS_MAX_L */
    uint8_t*     text;           /* device, 25 L^2 bytes, 16-byte aligned */
    int32_t*     fallback;       /* device, one word */
} rnamsm_ss_text_item;
size_t rnamsm_ss_prob_text_bytes(int L);
int rnamsm_ss_prob_text(const float* probs, int L, uint8_t* text, int32_t* fallback, void* stream);
int rnamsm_ss_prob_text_packed(const rnamsm_ss_text_item* items, int B, void* stream);

/* f4, the predicted structure -- the reference's prob_to_secondary_structure (code/post_processing/processing_output.py: the upper
 * triangle above 0.516, multiplets_free_bp, the .ct and .bpseq tables; without the VARNA plots) on the [L, L] probabilities where they
 * lie on the device.  The decoding as a graph process: {i, j}, i < j, is an edge iff probs[i, j] > float32(0.516) (only the upper
 * triangle is read; NaN is never an edge, +inf is one); in a round every base of degree >= 2 marks its incident edge of lowest
 * probability, on equal values the one to the lowest partner, and all marked edges are removed at once; rounds repeat until no base
 * has two partners (at most L - 2).  Every float pattern has a defined outcome: the decoding has no fallback.
 * probs [L, L] fp32 row-major; letters uint8 [L]: the sequence's characters as the tables print them (all device memory).  Outputs:
 *   partner int32 [L]      0 = unpaired, else the partner's 1-based index: the fifth .ct column, the third .bpseq column
 *   counts  int32 [4]      {pairs, bytes written to ct, bytes written to bpseq, fallback}
 *   ct      the body of `<name>.ct`: L lines "%d\t\t%c\t\t%d\t\t%d\t\t%d\t\t%d\n" of (i, letter, i - 1, i + 1 or 0 on the last line,
 *           partner, i), i = 1 .. L; the caller prepends the header line that carries the name
 *   bpseq   the body of `<name>.bpseq`: L lines "%d %c %d\n" of (i, letter, partner)
 * ct / bpseq hold at least the bounds of rnamsm_ss_struct_text_bytes(L, &ct_bytes, &bpseq_bytes) (32 L and 12 L: the longest lines
 * at L = 1024); bytes behind counts[1] / counts[2] are not written.  A letter of 0 or >= 128 -- nothing the host writer prints as
 * that one byte -- sets counts[3] = 1 (one plain store per structure): its two bodies are then unspecified and the caller writes
 * its tables on the host; partner and counts[0] are valid either way.
 * workspace: rnamsm_ss_pairs_workspace_bytes(B, Ls) bytes (B = 1 and &L for the lone call), 16-byte aligned, caller-owned (nothing
 * is allocated inside): the members' adjacency bit matrices, L x ceil(L / 64) 64-bit words each, rounded up to 256 bytes.  The
 * size is 0 for B outside [1, RNAMSM_SS_MAX_BATCH], a null Ls or an L outside [1, RNAMSM_SS_MAX_L].  Its contents on entry do not
 * matter.
 * Packed: B members of unlike L, one workgroup each, 32 members per launch (the descriptors travel as kernel arguments; items is a
 * HOST array, free to go after the call).  A member's four outputs are byte-identical to the lone call's, whatever its company;
 * the members' outputs must not overlap.
 * Refused (RNAMSM_ERR_INVALID) before anything is enqueued, rnamsm_last_error naming the member where one is at fault: B outside
 * [1, RNAMSM_SS_MAX_BATCH], an L outside [1, RNAMSM_SS_MAX_L], a null pointer, probs / partner / counts not 4-byte aligned, a
 * workspace that is not 16-byte aligned or too short.
 * No atomics: the same inputs give the same bytes on every run. */
typedef struct {                 /* one structure of the batch */
    const float*   probs;        /* device [L, L] */
    const uint8_t* letters;      /* device [L] */
    int32_t        L;            /* 1 .. RNAMSM_SS_MAX_L */
    int32_t*       partner;      /* device [L] */
    int32_t*       counts;       /* device [4] */
    uint8_t*       ct;           /* device, 32 L bytes */
    uint8_t*       bpseq;        /* device, 12 L bytes */
} rnamsm_ss_pairs_item;
size_t rnamsm_ss_pairs_workspace_bytes(int B, const int* Ls);
int rnamsm_ss_struct_text_bytes(int L, size_t* ct_bytes, size_t* bpseq_bytes);
int rnamsm_ss_pairs(const float* probs, const uint8_t* letters, int L, int32_t* partner, int32_t* counts, uint8_t* ct,
                    uint8_t* bpseq, void* workspace, size_t workspace_bytes, void* stream);
int rnamsm_ss_pairs_packed(const rnamsm_ss_pairs_item* items, int B, void* workspace, size_t workspace_bytes, void* stream);

/* f1 / f4 on a LONG alignment -- the pair heads on the stitched atp of rnamsm_stitch_pairs, for L in [1, RNAMSM_LONG_MAX_L].  Lone
 * calls only (a wide alignment never joins a group).  The entry points above keep their limits; each of these gives, for an L both
 * accept, the BITS (bytes) of its namesake above.  4096: four decimal digits in .ct / .bpseq; L^2 and 120 L^2 are int32 element
 * counts; the atp is 8 GB.
 *   rnamsm_contact_head_long    rnamsm_contact_head_atp under another limit: the same function, so the same checks, kernels and
 *                               summation order.  Symmetrise and APC are taken over
 *                               the whole [L, L] map: a pair no window holds (+0.0 in every channel) takes part as 0.  workspace:
 *                               rnamsm_contact_head_long_workspace_bytes(L, nch) = (nch L + nch) floats, 4-byte aligned.
 *   rnamsm_ss_head_long         rnamsm_ss_head under another limit, the same function (exact fp32; there is no bf16 long head).  workspace:
 *                               rnamsm_ss_head_long_workspace_bytes(L) = 2 x 48 L^2 floats (6.4 GB at the limit), 16-byte aligned.
 *   rnamsm_ss_prob_text_long    rnamsm_ss_prob_text's arguments, kernel and fallback word; rnamsm_ss_prob_text_long_bytes(L) = 25 L^2
 *                               (419 MB at the limit).
 *   rnamsm_ss_pairs_long        rnamsm_ss_pairs' arguments and contract -- partner [L], counts [4], the .ct and .bpseq bodies, within
 *                               the bounds of rnamsm_ss_struct_text_long_bytes (32 L and 12 L) -- by a kernel pair of its own: the
 *                               adjacency bits across the grid, then the rounds and the lines in one workgroup of 1024 threads
 *                               that own ceil(L / 1024) consecutive bases each.  The bytes are the host writer's for every L in
 *                               range.  workspace: rnamsm_ss_pairs_long_workspace_bytes(L) = L x ceil(L / 64) 64-bit words rounded
 *                               up to 256 bytes (2 MB at the limit), 16-byte aligned; its contents on entry do not matter.
 * Every size is 0 for an L outside [1, RNAMSM_LONG_MAX_L].  Refused (RNAMSM_ERR_INVALID) before anything is enqueued, with the
 * argument named: L out of range, a null pointer, a misaligned pointer, a plane stride < L * L, a short workspace.
 * No atomics: the same inputs give the same bits on every run. */
#define RNAMSM_LONG_MAX_L 4096
size_t rnamsm_contact_head_long_workspace_bytes(int L, int nch);
int rnamsm_contact_head_long(const float* atp, int64_t plane_stride, int L, int nch, const float* weight, const float* bias,
                             float* contacts, void* workspace, size_t workspace_bytes, void* stream);
size_t rnamsm_ss_head_long_workspace_bytes(int L);
int rnamsm_ss_head_long(const float* atp, int64_t atp_plane_stride, const uint8_t* base_codes, int L, int num_blocks,
                        const float* const* weights, float* logits, float* probs, void* workspace, size_t workspace_bytes,
                        void* stream);
size_t rnamsm_ss_prob_text_long_bytes(int L);
int rnamsm_ss_prob_text_long(const float* probs, int L, uint8_t* text, int32_t* fallback, void* stream);
size_t rnamsm_ss_pairs_long_workspace_bytes(int L);
int rnamsm_ss_struct_text_long_bytes(int L, size_t* ct_bytes, size_t* bpseq_bytes);
int rnamsm_ss_pairs_long(const float* probs, const uint8_t* letters, int L, int32_t* partner, int32_t* counts, uint8_t* ct,
                         uint8_t* bpseq, void* workspace, size_t workspace_bytes, void* stream);

/* f4 nested -- the pseudoknot-free structure of greatest expected accuracy, decoded from the [L, L] probabilities on the device
 * (csrc/ss_nested.h: the arithmetic below in a plain C++ header that g++ and hipcc both compile; csrc/ss_nested.hip: the kernels).
 * rnamsm_ss_pairs keeps every pair above 0.516 and removes multiplets base by base, so two crossing helices both survive; this
 * decoding finds the NESTED matching that maximises the summed pair probability in excess of a threshold (a Nussinov-style
 * max-plus dynamic programme, O(L^3)).  Everything is exact integer arithmetic: the result is specified bit for bit.
 *   inputs    probs [L, L] fp32: only the strict upper triangle is read; theta, fp32 in [0, 1) (the reference's 0.516f by
 *             default); min_loop in [0, RNAMSM_SS_NESTED_MAX_LOOP] (3 by default)
 *   allowed   (i, j), i < j, iff j - i > min_loop and probs[i, j] > theta, compared in fp32.  NaN and -inf are never allowed; +inf
 *             and values above 1 are allowed and count as 1.0
 *   weights   Q(x) = floor(min(x, 1) * 2^18), exact in fp32 (a scaling by a power of two);
 *             w(i, j) = max(1, Q(probs[i, j]) - Q(theta)) for an allowed pair, an int32.  At most L / 2 = 2048 pairs of weight
 *             <= 2^18: every sum is below 2^29; "not allowed" is -2^30, and one such value plus any sum stays inside int32
 *   table     N(i, j) = 0 for j <= i (and N(i, i - 1) = 0); for i < j
 *             N(i, j) = max(N(i, j-1), max over k in [i, j - min_loop - 1] with (k, j) allowed of N(i, k-1) + w(k, j) + N(k+1, j-1));
 *             the score is N(0, L-1)
 *   traceback canonical, so the structure is unique: from (0, L-1) with an explicit stack; at (i, j), j > i: if N(i, j) == N(i, j-1)
 *             go to (i, j-1) (j unpaired is preferred), else take the SMALLEST k that attains N(i, j), record the pair (k, j) and
 *             continue in (i, k-1) and (k+1, j-1)
 * Outputs:
 *   partner int32 [L]      0 = unpaired, else the partner's 1-based index, as rnamsm_ss_pairs writes it
 *   counts  int32 [5]      {pairs, bytes written to ct, bytes written to bpseq, fallback, score}; a score of -1 (no valid score is
 *                          negative) says that the traceback did not end on the tables it was given: the structure is then partial
 *   ct, bpseq              the bodies of `<name>.nested.ct` / `<name>.nested.bpseq`: rnamsm_ss_pairs' lines, bounds (32 L and 12 L
 *                          bytes) and fallback word (a letter of 0 or >= 128 sets counts[3] = 1: the bodies are then unspecified)
 *   dbn     uint8 [L]      '(' at the lower base of a pair, ')' at the upper one, '.' elsewhere
 * workspace: rnamsm_ss_nested_workspace_bytes(B, Ls) bytes (B = 1 and &L for the lone call), 16-byte aligned, caller-owned (nothing
 * is allocated inside): per member the int32 tables N and M(k, j) = w(k, j) + N(k+1, j-1), [Lp, Lp] each with Lp = L rounded up
 * to 64 (8 Lp^2 bytes: 134 MB at the limit).  The size is 0 for B outside [1, RNAMSM_SS_MAX_BATCH], a null Ls or an L outside
 * [1, RNAMSM_LONG_MAX_L].  Its contents on entry do not matter.
 * One entry point with one limit, L in [1, RNAMSM_LONG_MAX_L]: ceil(L / 64) fill launches (one per diagonal of 64 x 64 cell tiles)
 * and one traceback launch of one workgroup per member.  Packed: B members of unlike L, 32 per launch set (the descriptors travel
 * as kernel arguments; items is a HOST array, free to go after the call); the member is a grid dimension, so a set costs the
 * launches of its largest member.  A member's outputs are byte-identical to the lone call's, whatever its company; the members'
 * outputs must not overlap.
 * Refused (RNAMSM_ERR_INVALID) before anything is enqueued, rnamsm_last_error naming the argument or the member at fault: L, B,
 * theta (also NaN) or min_loop out of range, a null pointer, probs / partner / counts not 4-byte aligned, a workspace that is not
 * 16-byte aligned or too short.
 * No atomics: the same inputs give the same bytes on every run.
 * rnamsm_ss_nested_phases is rnamsm_ss_nested_packed with the two stages selectable, for measurement (tools/ss_nested_timing.py):
 * phases = 1 the fill alone (no output is written), 2 the traceback alone, on a workspace that a fill with the same arguments has
 * written, 3 both.  Its refusals are the packed call's, and phases outside [1, 3]. */
#define RNAMSM_SS_NESTED_MAX_LOOP 32
typedef struct {                 /* one structure of the batch */
    const float*   probs;        /* device [L, L] */
    const uint8_t* letters;      /* device [L] */
    int32_t        L;            /* 1 .. RNAMSM_LONG_MAX_L */
    int32_t*       partner;      /* device [L] */
    int32_t*       counts;       /* device [5] */
    uint8_t*       ct;           /* device, 32 L bytes */
    uint8_t*       bpseq;        /* device, 12 L bytes */
    uint8_t*       dbn;          /* device, L bytes */
} rnamsm_ss_nested_item;
size_t rnamsm_ss_nested_workspace_bytes(int B, const int* Ls);
int rnamsm_ss_nested(const float* probs, const uint8_t* letters, int L, float theta, int min_loop, int32_t* partner, int32_t* counts,
                     uint8_t* ct, uint8_t* bpseq, uint8_t* dbn, void* workspace, size_t workspace_bytes, void* stream);
int rnamsm_ss_nested_packed(const rnamsm_ss_nested_item* items, int B, float theta, int min_loop, void* workspace,
                            size_t workspace_bytes, void* stream);
int rnamsm_ss_nested_phases(const rnamsm_ss_nested_item* items, int B, float theta, int min_loop, void* workspace,
                            size_t workspace_bytes, int phases, void* stream);

/* f5 -- RNA-MSM RSA (relative solvent accessibility) predictor (_downstream_tasks/RSA: predict.py, model/_0811/model_entry.py
 * FrameModel(Cin, 1, planes 64, depth 1, BatchNorm1d)) for an ensemble of n_models members in one set of four launches, exact fp32:
 *   x[c, p]  = (onehot(code[p])[c] - mu_oh[c]) / std_oh[c]  (c < 4, only with use_onehot),
 *              (emb[p, e] - mu_emb[e]) / std_emb[e]  (the next 768 channels), 1 (the last channel: the mask)      p < L
 *              and 0 in every channel outside [0, L): the convolutions pad the NORMALISED input, mask channel included
 *   h = relu(BN1(conv1_k3(x)));  h = relu(BN2(conv2_k3(h)));  w = sigmoid(fc2(relu(fc1(mean_p h))))
 *   y = relu(h * w + BNs(shortcut_k1(x)));  y += proj(softmax(Q K^T / sqrt 8) V) on LN1(y), 8 heads of 8;
 *   y += W2 gelu_erf(W1 LN2(y));  logits = final(y);  probs = sigmoid(logits)              probs / logits [n_models, L]
 * emb: row p at emb + p * emb_row_stride, 768 floats (stride 768: the [L, 768] of rnamsm_pack_outputs; a larger stride reads rows
 * of a wider buffer in place, e.g. row 0, columns 1..L of the final representation).  base_codes [L] as for rnamsm_ss_head.
 * Cin = 773 with use_onehot, 769 without.  The normalisation repeats the reference's numpy arithmetic on its shipped statistics:
 * float32 subtraction and division for the embedding, float64 (rounded once) for the one-hot columns.
 * weights: RNAMSM_RSA_GLOBAL_WEIGHTS + RNAMSM_RSA_WEIGHTS_PER_MODEL * n_models pointers (a host array), 16-byte aligned each:
 *   [0] mu_emb  [1] std_emb  (float [768])       [2] mu_oh  [3] std_oh  (double [4]; not read and may be null without use_onehot)
 *   per member k, at 4 + 26k, fp32 (names of the reference's state_dict; BN folded in float64 into scale = weight / sqrt(var + 1e-5),
 *   shift = bias - mean * scale; every matrix transposed to [in][out] so that a wave reads consecutive outputs):
 *    +0 stem [4][800][64]: slabs 0..2 = net.0.0.conv1.weight taps, slab 3 = net.0.0.shortcut.0.weight; rows >= Cin are zero
 *    +1 bn1 scale  +2 bn1 shift  +3 shortcut.1 scale  +4 shortcut.1 shift  [64]
 *    +5 conv2.weight [3 taps][64 in][64 out]   +6 bn2 scale  +7 bn2 shift [64]
 *    +8 fc1.weight [4][64]  +9 fc1.bias [4]  +10 fc2.weight [64][4]  +11 fc2.bias [64]           (squeeze-excite, as stored)
 *    +12 net.1.0.ln1.weight  +13 ln1.bias [64]
 *    +14 attn.{query,key,value}.weight [3][64 in][64 out]   +15 their biases [3][64]
 *    +16 attn.proj.weight [64 in][64 out]  +17 attn.proj.bias [64]   +18 ln2.weight  +19 ln2.bias [64]
 *    +20 mlp.0.weight [64 in][256 out]  +21 mlp.0.bias [256]  +22 mlp.2.weight [256 in][64 out]  +23 mlp.2.bias [64]
 *    +24 final.weight [64]  +25 final.bias [1]
 * Either of probs / logits may be null, not both.  workspace: rnamsm_rsa_head_workspace_bytes(L, n_models) bytes, 16-byte aligned,
 * caller-owned (nothing is allocated inside); 0 for L or n_models outside their limits.
 * Refused (RNAMSM_ERR_INVALID) before anything is launched: L outside [1, RNAMSM_RSA_MAX_L], n_models outside
 * [1, RNAMSM_RSA_MAX_MODELS], emb_row_stride < 768, a null or misaligned pointer, a short workspace.
 * A NaN or an inf in emb is not refused: it comes out as NaN exactly where the reference network gives NaN (every ReLU carries
 * a NaN on, as nn.ReLU does) -- through the squeeze mean and the attention that is every position of every member.
 * No atomics, one fixed summation order: the same bits on every run, and member k's row does not depend on the other members. */
#define RNAMSM_RSA_MAX_L 1024
#define RNAMSM_RSA_MAX_MODELS 8
#define RNAMSM_RSA_GLOBAL_WEIGHTS 4
#define RNAMSM_RSA_WEIGHTS_PER_MODEL 26
size_t rnamsm_rsa_head_workspace_bytes(int L, int n_models);
int rnamsm_rsa_head(const float* emb, int64_t emb_row_stride, const uint8_t* base_codes, int L, int n_models, int use_onehot,
                    const void* const* weights, float* probs, float* logits, void* workspace, size_t workspace_bytes,
                    void* stream);

/* f5, several alignments per launch -- rnamsm_rsa_head over B embeddings of unlike length in ONE set of four launches.  Every
 * launch covers sum_b ceil(L_b / 32) x n_models blocks -- each member's own tiles, never B x the longest member's -- and a block
 * finds its member in a device descriptor table.  A tile's arithmetic is the lone call's (the same device functions on the
 * member's own embedding, L and workspace slab; its squeeze mean and attention keys are its own), so every member's
 * [n_models, L_b] probs / logits are BIT-IDENTICAL to rnamsm_rsa_head on that member alone, whatever its company, its place in
 * the batch and its embedding's row stride.
 * items: a HOST array of B entries, read during the call and free to go afterwards (the descriptors travel as kernel arguments
 * on `stream`).  Per member: emb / emb_row_stride / base_codes / L / probs / logits as for rnamsm_rsa_head; the members'
 * embeddings may be slices of one buffer, their outputs must not overlap.
 * weights, n_models, use_onehot: exactly those of rnamsm_rsa_head.
 * workspace: rnamsm_rsa_head_packed_workspace_bytes(B, Ls, n_models) bytes, 16-byte aligned, caller-owned (nothing is allocated
 * inside): the descriptor table (64 bytes per member, rounded up to 256), then the members' slabs in order -- member b's is the
 * lone call's workspace, rnamsm_rsa_head_workspace_bytes(L_b, n_models) bytes, at the sum of the slabs before it.  The size is 0
 * for B outside [1, RNAMSM_RSA_MAX_BATCH], a null Ls, an L outside [1, RNAMSM_RSA_MAX_L] or n_models outside
 * [1, RNAMSM_RSA_MAX_MODELS].
 * Refused (RNAMSM_ERR_INVALID) before anything is enqueued, rnamsm_last_error naming the member where one is at fault: B or
 * n_models out of range, a member's L out of range, a null pointer (items, weights, workspace, a member's emb or base_codes, a
 * weight), a member with neither probs nor logits, emb_row_stride < 768, an embedding, weight pointer or workspace that is not
 * 16-byte aligned, an output that is not 4-byte aligned, a short workspace.
 * A non-finite input comes out as NaN exactly where the reference network gives NaN, as for rnamsm_rsa_head, and a member never
 * affects another: the neighbours of a poisoned member stay finite and keep their bits.
 * No atomics: the same inputs give the same bits on every run. */
typedef struct {                 /* one alignment of the batch */
    const float*   emb;          /* device: row p at emb + p * emb_row_stride, 768 floats; 16-byte aligned */
    int64_t        emb_row_stride;     /* >= 768 */
    const uint8_t* base_codes;   /* device, [L] */
    int32_t        L;            /* 1 .. RNAMSM_RSA_MAX_L */
    float*         probs;        /* device [n_models, L] or null */
    float*         logits;       /* device [n_models, L] or null; not both null */
} rnamsm_rsa_item;
#define RNAMSM_RSA_MAX_BATCH 1024
size_t rnamsm_rsa_head_packed_workspace_bytes(int B, const int* Ls, int n_models);
int rnamsm_rsa_head_packed(const rnamsm_rsa_item* items, int B, int n_models, int use_onehot, const void* const* weights,
                           void* workspace, size_t workspace_bytes, void* stream);

/* f5, the text of the tables -- the bodies of the reference's `RSA_result/<name>_<k>/<name>.txt` (one per member) and
 * `<name>_ensemble/<name>.txt` (predict.py: doSavePredict_single), written on the device from the [n_models, L] RSA of
 * rnamsm_rsa_head, byte for byte.  Per position p, in float64 (K = n_models):
 *   scale[p] = 400 for the letter A or G, 350 for C, U or T (T scales as U; the letter column prints the letter itself)
 *   member k: asa_k = double(rsa[k][p]) * scale[p], rsa_k = double(rsa[k][p])
 *   ensemble: asa_e = (((asa_0 + asa_1) + ...) + asa_{K-1}) / K in that order, rsa_e = asa_e / scale[p]     (IEEE, nothing fused)
 * A body is L lines "%d\t\t%c\t\t%.2f\t\t%.3f\n" of (p + 1, letter[p], asa, rsa): "%.2f" / "%.3f" are the double's exact binary
 * value rounded half to even at that decimal, computed in integers.  The caller prepends the header, which carries the names.
 * rsa [n_models, L] fp32 row-major, letters uint8 [L]: the sequence's characters (all device memory).  Outputs:
 *   text    rnamsm_rsa_text_bytes(L, n_models) = (n_models + 1) x RNAMSM_RSA_TEXT_LINE_MAX x L bytes, 16-byte aligned: body f (member
 *           f, or the ensemble for f = n_models) starts at f x RNAMSM_RSA_TEXT_LINE_MAX x L -- 23 bytes is the longest line at
 *           L <= 1024; bytes behind a body's count are not written.  The size is 0 for L outside [1, RNAMSM_RSA_MAX_L] or n_models
 *           outside [1, RNAMSM_RSA_MAX_MODELS].
 *   counts  int32 [n_models + 3]: the bytes written to each of the n_models + 1 bodies, then the fallback word, then the zero word
 *   ens     double [2, L] or null: asa_e, then rsa_e
 * The fallback word reads 1 (else 0) when a member value is NaN or inf, has its sign bit set (-0.0 included) or lies above 1.0, or
 * when a letter is none of A C G U T (the host path replaces such a letter by a base drawn from its generator): the bodies and ens
 * are then unspecified (every write still stays inside its bound) and the caller formats that alignment on the host.  The zero word
 * reads 1 (else 0) when a member's ASA or the ensemble's is exactly 0, where the reference exits.  With both words 0 the text is
 * exact.  Each word is one plain store; no atomics, no workspace, nothing allocated: the same inputs give the same bytes on every
 * run.
 * Packed: B members of unlike L in one call, one workgroup per (member, table), 32 members per launch (the descriptors travel as
 * kernel arguments; items is a HOST array, free to go after the call).  A member's bytes, counts and ens are those of the lone call
 * on it, whatever its company and place; the members' outputs must not overlap.
 * Refused (RNAMSM_ERR_INVALID) before anything is enqueued, rnamsm_last_error naming the member where one is at fault: B outside
 * [1, RNAMSM_RSA_MAX_BATCH], n_models or an L out of range, a null pointer other than ens, rsa or counts not 4-byte aligned, ens
 * not 8-byte aligned, text not 16-byte aligned. */
#define RNAMSM_RSA_TEXT_LINE_MAX 23
typedef struct {                 /* one alignment of the batch */
    const float*   rsa;          /* device [n_models, L] */
    const uint8_t* letters;      /* device [L] */
    int32_t        L;            /* 1 .. RNAMSM_RSA_MAX_L */
    uint8_t*       text;         /* device, rnamsm_rsa_text_bytes(L, n_models) bytes, 16-byte aligned */
    int32_t*       counts;       /* device [n_models + 3] */
    double*        ens;          /* device [2, L] or null */
} rnamsm_rsa_text_item;
size_t rnamsm_rsa_text_bytes(int L, int n_models);
int rnamsm_rsa_text(const float* rsa, const uint8_t* letters, int L, int n_models, uint8_t* text, int32_t* counts, double* ens,
                    void* stream);
int rnamsm_rsa_text_packed(const rnamsm_rsa_text_item* items, int B, int n_models, void* stream);

/* f5 on a LONG alignment -- the RSA ensemble and its tables on the stitched embedding of rnamsm_stitch_rows, for L in
 * [1, RNAMSM_LONG_MAX_L].  Lone calls only (a wide alignment never joins a group).  rnamsm_rsa_head and rnamsm_rsa_text keep their
 * limits and their workspace layout; each of these gives, for an L both accept, the BITS (bytes) of its namesake above: logits,
 * probs, text, counts, ens and the two flag words.
 *   rnamsm_rsa_head_long   rnamsm_rsa_head's arguments, weight table and checks (one function under two names and limits), and the
 *                          same kernel template per stage, instantiated for a second workspace layout: per model 7 L 64 floats
 *                          (h1, shortcut, h2, y, q, k, v) and then
 *                          RNAMSM_LONG_MAX_L / 32 = 128 rows of 64 tile sums, of which the first ceil(L / 32) are written --
 *                          rnamsm_rsa_head_long_workspace_bytes(L, n_models) = n_models (7 L 64 + 128 x 64) x 4 bytes (7.4 MB per
 *                          model at the limit), 16-byte aligned.  The squeeze mean adds the tile sums in one ascending chain per
 *                          group of 32 tiles and the group sums ascending (one group: rnamsm_rsa_head's chain), the same order
 *                          in every block; the attention sums 64 keys a chunk and the chunks ascending, as for any L.
 *   rnamsm_rsa_text_long   rnamsm_rsa_text's arguments, kernel, counts, ens, fallback word and zero word; the bytes are the host
 *                          writer's for every L in range.  rnamsm_rsa_text_long_bytes(L, n_models) = (n_models + 1) x
 *                          RNAMSM_RSA_TEXT_LINE_MAX x L: 23 bytes still hold the longest line, "4096\t\tG\t\t400.00\t\t1.000\n".
 * Every size is 0 for an L outside [1, RNAMSM_LONG_MAX_L] or n_models outside [1, RNAMSM_RSA_MAX_MODELS].  Refused
 * (RNAMSM_ERR_INVALID) before anything is launched, with the value or the argument named: L or n_models out of range, a null or
 * misaligned pointer, emb_row_stride < 768, a short workspace.  No atomics: the same inputs give the same bits on every run. */
size_t rnamsm_rsa_head_long_workspace_bytes(int L, int n_models);
int rnamsm_rsa_head_long(const float* emb, int64_t emb_row_stride, const uint8_t* base_codes, int L, int n_models, int use_onehot,
                         const void* const* weights, float* probs, float* logits, void* workspace, size_t workspace_bytes,
                         void* stream);
size_t rnamsm_rsa_text_long_bytes(int L, int n_models);
int rnamsm_rsa_text_long(const float* rsa, const uint8_t* letters, int L, int n_models, uint8_t* text, int32_t* counts, double* ens,
                         void* stream);

/* a7 -- the residual add of NormalizedResidualBlock around a layer that is NOT one of this library's (modules.py:396,
 * `x = residual + x`; around the library's own layers the add is fused into the layer's last GEMM): out[i] = a[i] + b[i], fp32,
 * out may alias a or b. */
int rnamsm_add(const float* a, const float* b, float* out, int64_t n, void* stream);

/* a10 -- head-averaged attention weights of the generic MultiheadAttention (msm/multihead_attention.py:389-397,
 * need_weights=True without need_head_weights): out[i] = mean_h probs[h, i], probs [H, n] fp32, out [n]. */
int rnamsm_head_mean(const float* probs, float* out, int H, int64_t n, void* stream);

/* f3 -- greedy max/min mean-Hamming row sub-sampling (MSA.greedy_select, utils/align.py:128-148, via
 * select_diverse "diversity-max" / "diversity-min", :165-181): msa uint8 [N, L] (any per-character code, e.g. the raw
 * bytes or token ids), keeps row 0, returns the num_seqs selected row indices in ascending order.  Performs the
 * reference's float64 operations in the reference's order (numpy's pairwise summation of every candidate's distance
 * history), so the indices are identical to numpy's.  L < 65536, num_seqs <= 2048. */
size_t rnamsm_greedy_select_workspace_bytes(int N, int L, int num_seqs);
int rnamsm_greedy_select(const uint8_t* msa, int N, int L, int num_seqs, int minimise, int* out_indices,
                         void* workspace, size_t workspace_bytes, void* stream);

/* f3 -- sequence weights for `sample-pretrained` sub-sampling (MSA.weights, utils/align.py:250-253, consumed by
 * MSA.sample_weights, :150-163): weights[i] = 1 / #{ j : hamming(msa[i], msa[j]) / L < seqid_cutoff } as float64 (the row
 * itself counts), msa uint8 [N, L], L <= 32768.  The random draw itself stays on the host (numpy's generator is the
 * contract).  The reference compares raw character bytes; any one-to-one recoding (the tokenizer's ids for A/C/G/U/X/-)
 * gives the same distances. */
int rnamsm_msa_weights(const uint8_t* msa, int N, int L, double seqid_cutoff, double* weights, void* stream);

/* Covariance contacts (MSA.invcov, utils/align.py:183-193): out[i, j] = the spectral norm of the K x K block (column i, column j) of
 * np.cov of the one-hot alignment, float64 [L, L] -- the co-evolution map of the raw alignment, no network involved.  tokens uint8
 * [N, L] with leading dimension ld >= L; the K symbols are the distinct values other than `gap` that occur, ascending; a gap is all
 * zeros in the one-hot.  The reference runs over raw character bytes; any one-to-one recoding (the tokenizer's ids) permutes the
 * rows and columns of every block and leaves its spectral norm unchanged, so token ids give the same map.
 *   stage 1  n_ab(i,j) = #{rows with symbol a in column i and b in column j}: exact int32 from and + popcount over bit planes of the
 *            alignment, no atomics, the same bits on every run;
 *   stage 2  B[a][b] = ((double)n_ab(i,j) - ((double)n_a(i) * (double)n_b(j)) / N) / (N - 1) in exactly this order (n_a(i) =
 *            n_aa(i,i); the product is exact), then the largest singular value of B by one-sided Jacobi in fp64.  A zero block
 *            (a constant column) gives exactly 0; no finite input gives NaN.  B(j,i) is the transpose of B(i,j): the upper triangle
 *            is computed and mirrored, so out is exactly symmetric.
 * counts: NULL, or int32 [32 + L*L*K*K]: a header (K, then the K symbols ascending, then zeros) followed by n_ab as [L, L, K, K];
 * the caller sizes it for the K of its alignment (16 is the upper bound).
 * N in [2, 2^20], L in [1, RNAMSM_LONG_MAX_L], K in [1, 16]: an alignment of gaps only (K = 0) or with more than 16 distinct
 * non-gap values is refused, the message names the count.  workspace: 256-byte aligned, rnamsm_msa_invcov_workspace_bytes(N, L)
 * bytes (0 outside the limits; sized for K = 16: the bit planes, N * L * 2 bytes and padding, and a band of counts of at most
 * 256 MB).  Unlike the rest of this header the call WAITS for the stream once: K is read back before the planes are laid out.  It
 * must not be captured into a graph. */
size_t rnamsm_msa_invcov_workspace_bytes(int N, int L);
int rnamsm_msa_invcov(const uint8_t* tokens, int N, int L, int64_t ld, int gap, double* out, int32_t* counts, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Mutual-information contacts: mi[i, j] = the mutual information of alignment columns i and j, and mip = its average-product
 * corrected form (MIp), float64 [L, L] each; either may be NULL, not both.  tokens, ld, gap, the K symbols, the refusals (K = 0,
 * K > 16) and the limits (N in [2, 2^20], L in [1, RNAMSM_LONG_MAX_L]) are rnamsm_msa_invcov's, and so is stage 1: the exact integer
 * pair counts n_ab(i, j) and marginals n_a(i).  The states of a column pair give an integer table c[a][b]; gap_mode says what a gap is:
 *   RNAMSM_MI_GAPS_PAIRWISE (0)  rows with a gap in column i or j are left out of that pair: c[a][b] = n_ab(i, j) over the K symbols,
 *                                all of it from the pair's own K x K block;
 *   RNAMSM_MI_GAPS_STATE (1)     the gap is a (K+1)-th state, its row and column from the marginals in integers:
 *                                c[a][gap] = n_a(i) - sum_b n_ab, c[gap][b] = n_b(j) - sum_a n_ab, c[gap][gap] = N - the rest; n = N.
 * With n = sum c, r_a = sum_b c[a][b], s_b = sum_a c[a][b], all integers,
 *   mi(i, j) = sum over a, b with c[a][b] > 0 of (c[a][b] / n) * log((c[a][b] * n) / (r_a * s_b))        natural log, float64;
 * a pair with n = 0 gives 0.  Both integer products are below 2^40 and exact in a double, so the argument of the log is one
 * correctly rounded division of exact integers; the sum runs a-major then b, ascending, in one thread, without contraction, no
 * atomics: the same bits on every run.  Hence, exactly: a constant column, and in state mode an all-gap column, has ratio 1.0, log 0,
 * and its whole row and column of mi exactly 0; mi(i, i) is the column's entropy; j >= i is computed and written to both places, so
 * the map is exactly symmetric.
 *   mip = rnamsm_apc_f64 of mi with its diagonal read as 0 (below); a total of 0 (L = 1, or every column constant) gives NaN everywhere.
 * workspace: 256-byte aligned, rnamsm_msa_mi_workspace_bytes(N, L) bytes (0 outside the limits): rnamsm_msa_invcov's, an [L, L]
 * float64 map (used when mi is NULL) and the correction's sums.  Every refusal comes before the first launch and names the value.
 * Like rnamsm_msa_invcov the call WAITS for the stream once (K is read back); it must not be captured into a graph. */
#define RNAMSM_MI_GAPS_PAIRWISE 0
#define RNAMSM_MI_GAPS_STATE 1
size_t rnamsm_msa_mi_workspace_bytes(int N, int L);
int rnamsm_msa_mi(const uint8_t* tokens, int N, int L, int64_t ld, int gap, int gap_mode, double* mi, double* mip, void* workspace,
                  size_t workspace_bytes, void* stream);

/* Sequence-weighted mutual information (rnamsm_msa_mi with row n counted weights[n] times): the pair's table is
 *   c[a][b] = sum over rows n of weights[n] * [x(n, i) = a] * [x(n, j) = b]                                  float64,
 * over S states: the K symbols in RNAMSM_MI_GAPS_PAIRWISE (S = K; a row with a gap in column i or j is in no entry), the K symbols
 * and the gap as state K, counted like any other, in RNAMSM_MI_GAPS_STATE (S = K + 1 <= 17).  tokens, ld, gap, the K symbols, the
 * refusals and the limits (N in [2, 2^20], L in [1, RNAMSM_LONG_MAX_L], K in [1, 16]) are rnamsm_msa_invcov's.  weights: float64
 * [N] on the device, every one finite and > 0 (rnamsm_msa_neff's at a cutoff above 0); they are checked on the device and the
 * verdict is read back with K: a weight that is NaN, +-inf, zero or negative is refused with RNAMSM_ERR_INVALID, the message names
 * the first such row, and no output is touched.  The counts are a contraction of one-hot operands on the fp64 matrix pipe: every
 * product is exact, one thread block adds all N rows of its results in groups of four ascending rows from 0.0 (within a group in
 * the instruction's order), without atomics: the same bits on every run, and c(i,a; j,b) == c(j,b; i,a) bit for bit.  Then
 *   s_b = sum_a c[a][b], r_a = sum_b c[a][b], n = sum_b s_b, each ascending from 0.0,
 *   mi(i, j) = sum over a then b ascending, the entries with c > 0 only, of (c / n) * log((c * n) / (r_a * s_b)); n = 0 gives 0,
 * one operation at a time: with every weight 1.0 the two maps are rnamsm_msa_mi's bit for bit.  mip = rnamsm_apc_f64 of mi with a
 * zero diagonal.  mi, mip: float64 [L, L]; either may be NULL, and both where wcounts is given.  wcounts (optional): float64
 * [L, L, S, S], every table.  wmarg (optional): float64 [L, S], c(i,a; i,a), the weighted column profile.  meta (optional): int32
 * [32], K and the symbols ascending, as rnamsm_msa_invcov's counts header.  workspace, 256-byte aligned: any size from
 * rnamsm_msa_wmi_min_workspace_bytes(N, L) upward, rnamsm_msa_wmi_workspace_bytes(N, L) by default (both 0 outside the limits):
 * stage 1's planes, the state planes, an [L, L] map, the correction's sums and a band of counts, L * S * S * 8 bytes per column i
 * (at most 256 MB by default, one column at S = 17 at least).  Without wcounts the columns are counted band by band; the band
 * count follows from workspace_bytes alone and every accepted size gives the same bits.  Every refusal of an argument comes
 * before the first launch and names the value.  Like its two siblings the call WAITS for the stream once (K and the weights'
 * verdict are read back); it must not be captured into a graph. */
size_t rnamsm_msa_wmi_workspace_bytes(int N, int L);
size_t rnamsm_msa_wmi_min_workspace_bytes(int N, int L);
int rnamsm_msa_wmi(const uint8_t* tokens, int N, int L, int64_t ld, int gap, int gap_mode, const double* weights, double* mi,
                   double* mip, double* wcounts, double* wmarg, int32_t* meta, void* workspace, size_t workspace_bytes, void* stream);

/* Average-product correction of a square float64 map (the reference's apc, utils/tensor.py:103-113), symmetric or not:
 *   a1 = row sums, a2 = column sums, a12 = the total,  out[i, j] = x[i, j] - (a1[i] * a2[j]) / a12     (product, division, subtraction).
 * x [L, L] with leading dimension ld >= L, out [L, L] packed.  zero_diagonal = 1: the diagonal of x is read as 0, in the sums and in
 * the subtraction, so out[i, i] = 0 - (a1[i] * a2[i]) / a12.  A total of 0 gives NaN everywhere, as the reference's 0 / 0 does.
 * Every sum has one fixed order, no atomics: a1[i]: 256 running sums, sum t over x[i, t], x[i, t + 256], ... ascending from 0.0,
 * folded in halves (s[t] += s[t + 128], then + 64, ..., + 1); a2[j]: four running sums, sum g over x[g, j], x[g + 4, j], ...
 * ascending from 0.0, a2[j] = (p0 + p2) + (p1 + p3); a12: the 256-sum-and-fold of a1.  L in [1, 32768].  out == x is allowed where
 * ld == L (an element is read and written by one thread, after the sums) and refused otherwise; other overlaps are the caller's
 * error.  workspace: rnamsm_apc_f64_workspace_bytes(L) bytes (2 L + 1 doubles; 0 outside the limits), 8-byte aligned.  Asynchronous:
 * the call waits for nothing. */
size_t rnamsm_apc_f64_workspace_bytes(int L);
int rnamsm_apc_f64(const double* x, int L, int64_t ld, int zero_diagonal, double* out, void* workspace, size_t workspace_bytes,
                   void* stream);

/* Alignment statistics built on the pairwise Hamming matrix (utils/align.py: MSA.pdist :121-126, MSA.weights / MSA.neff :250-269, the
 * coverage property :242-247).  msa uint8 [N, L] with leading dimension ld >= L: any byte values, any number of distinct ones (raw
 * character bytes or token ids: a one-to-one recoding changes no distance); bytes in [L, ld) are never read as data.  All of it rests
 * on m(i, j) = the number of columns in which rows i and j differ, an exact int32 from xor + a per-byte non-zero mask + popcount over
 * the rows kept eight bytes to a 64-bit word (zero past L), 64 x 64 pairs a block, tiles on or above the diagonal only: no atomics,
 * the same bits on every run.
 *   rnamsm_msa_pdist     counts int32 [N, N] = m and / or dist float64 [N, N] = (double)m / (double)L (scipy's pdist "hamming", one
 *                        IEEE division); either may be NULL, not both.  The diagonal is exactly 0, the lower triangle a copy of the
 *                        upper.  N in [1, 16384] (dist is 2 GB there; every i * N + j is 64-bit), L in [1, 32768].  workspace:
 *                        rnamsm_msa_pdist_workspace_bytes(N, L) bytes (the packed rows; 0 outside the limits), 256-byte aligned.
 *   rnamsm_msa_neff      n_neighbors[i] = #{ j : (double)m(i, j) / (double)L < seqid_cutoff } int32 [N] (the reference's strict
 *                        comparison; the row itself has m = 0 and counts unless the cutoff is 0), weights[i] = 1.0 / n_neighbors[i]
 *                        float64 [N] (rnamsm_msa_weights' values, bit for bit; inf where nothing counts), neff = the weights' sum,
 *                        one float64, added in one fixed order: 1024 running sums, sum t over rows t, t + 1024, ... ascending from
 *                        0.0, then folded in halves (s[t] += s[t + 512], then + 256, ..., + 1).  Each output may be NULL, not all
 *                        three.  The N x N matrix is never formed: every tile's thresholded row and column sums go to int32 partial
 *                        slots, one per (row, block of 64 rows), each written once, and are added per row.  N in [1, 2^20], L in
 *                        [1, 32768], seqid_cutoff in [0, 1].  workspace, 256-byte aligned: any size from
 *                        rnamsm_msa_neff_min_workspace_bytes(N, L) upward; rnamsm_msa_neff_workspace_bytes(N, L) is the default (the
 *                        packed rows, N int32 totals and a partial table of at most 256 MB).  A partial table that does not hold
 *                        every row block is reused band by band of row blocks; the band count follows from workspace_bytes alone,
 *                        and every accepted size gives the same bits (the totals are integer sums).
 *   rnamsm_msa_coverage  coverage[c] = (double)#{rows whose byte in column c != gap} / (double)N, float64 [L]: integer counts, one
 *                        division.  N in [1, 2^20], L in [1, 32768], gap a byte value.
 * Every refusal comes before the first launch, leaves the outputs untouched and names the offending value.  The calls are
 * asynchronous: none waits for the stream. */
size_t rnamsm_msa_pdist_workspace_bytes(int N, int L);
int rnamsm_msa_pdist(const uint8_t* msa, int N, int L, int64_t ld, int32_t* counts, double* dist, void* workspace,
                     size_t workspace_bytes, void* stream);
size_t rnamsm_msa_neff_workspace_bytes(int N, int L);
size_t rnamsm_msa_neff_min_workspace_bytes(int N, int L);
int rnamsm_msa_neff(const uint8_t* msa, int N, int L, int64_t ld, double seqid_cutoff, int32_t* n_neighbors, double* weights,
                    double* neff, void* workspace, size_t workspace_bytes, void* stream);
int rnamsm_msa_coverage(const uint8_t* msa, int N, int L, int64_t ld, int gap, double* coverage, void* stream);

/* The identity redundancy filter: a row sub-sampling rule of this project's own, modelled on what the reference asks of the external
 * hhfilter binary (-id 90 -diff num_seqs, utils/align.py:68-102) and NOT that binary's algorithm -- hhfilter's -diff counts sequences
 * per window of 50 columns and has its own threshold schedule, this rule counts over the whole alignment.  Integers throughout.
 *   msa uint8 [N, L], leading dimension ld >= L, `gap` one byte value; bytes in [L, ld) are never read as data.  Per pair of rows:
 *   both(i, j) = the columns where neither row has the gap, same(i, j) = those of them where the bytes are equal, nres(i) = both(i, i).
 *   Row k is REDUNDANT to row j at threshold t (a percentage) iff both(k, j) > 0 and 100 * same(k, j) >= t * both(k, j)  (int32).
 *   order: int32 [N] on the device, the rows in the order they are walked (a permutation of 0 .. N - 1; the Python layer passes
 *   row 0, then the others by descending nres, ties by ascending index), or NULL = rows as given.  An entry outside [0, N) is found
 *   on the device and refused (RNAMSM_ERR_INVALID, the message names its position; no output is touched); a repeated row is not
 *   looked for -- it is redundant to its first occurrence, and a row that is missing is never kept.
 *   thresholds: num_seqs > 0: min_seqid, min_seqid + step, ... while below max_seqid, then max_seqid; num_seqs == 0, or
 *   min_seqid >= max_seqid: max_seqid alone.  1 <= min_seqid, 1 <= max_seqid <= 100, step >= 1.
 *   a pass at threshold t walks the rows not kept yet, in order: a row is kept iff it is redundant at t to no kept row (of an earlier
 *   pass, or earlier in this one); a row with nres = 0 is never kept unless it is the first of the order, which always is; a row
 *   rejected in one pass is tried again in the next.  The walk stops after the first pass that leaves at least num_seqs rows kept
 *   (num_seqs > 0), and after the last threshold in any case.
 * kept_indices: int32 [N] on the device; its first *n_kept entries are the kept row indices, ascending, the rest is untouched.
 * kept_at: int32 [N] on the device or NULL: per row the threshold of the pass that kept it, -1 for a row never kept.  n_kept: on the
 * HOST.  Cutting to num_seqs rows (the first num_seqs of the ascending list) is the caller's.
 * The rows are kept eight bytes to a 64-bit word, the gap recoded to the zero byte (one-to-one); the pairs are counted 64 x 64 a
 * block like rnamsm_msa_neff's.  The order is walked in chunks of "seqid_filter_chunk" positions (rnamsm_set_param): per chunk one
 * launch rejects what is redundant to the rows kept so far and one block resolves the chunk's own survivors in order; ANY chunk size
 * gives the same indices.  No atomics, the same indices on every run.  N in [1, 2^20], L in [1, 32768].  workspace:
 * rnamsm_seqid_filter_workspace_bytes(N, L) bytes (the packed rows and four int32 per row; 0 outside the limits), 256-byte aligned.
 * Every argument refusal comes before the first launch and names the value.  Unlike the statistics calls above this call WAITS for
 * the stream: the kept count is read back once per pass to decide whether to stop, and the call returns with the outputs complete;
 * it must not be captured into a graph. */
size_t rnamsm_seqid_filter_workspace_bytes(int N, int L);
int rnamsm_seqid_filter(const uint8_t* msa, int N, int L, int64_t ld, int gap, const int32_t* order, int num_seqs, int min_seqid,
                        int max_seqid, int step, int32_t* kept_indices, int32_t* kept_at, int* n_kept, void* workspace,
                        size_t workspace_bytes, void* stream);

/* The top-k ranked pairs of an L x L map (contacts, covariance, mutual information: any pair score), selected and ranked on the
 * device.  x [L, L] with leading dimension ld >= L, float64 (_f64) or float32 (_f32).
 *   Candidates: the pairs (i, j) with 0 <= i < j < L, j - i >= min_sep and x[i * ld + j] not NaN.  ONLY those elements are read: the
 *   diagonal, the lower triangle, the band closer than min_sep and the padding beyond column L are never looked at, and symmetry is
 *   not assumed.
 *   A pair's value is v = (double)x[i, j] (exact for float32).  -0.0 counts as +0.0; +inf and -inf are ordinary values.
 *   The order is total: larger v first, then smaller i, then smaller j.
 * With n = min(k, the number of candidates): pairs[0 .. n) (int32 [k, 2], 0-based i then j) and scores[0 .. n) (float64 [k]) hold the
 * first n candidates in that order, a zero written as +0.0; *count = n, an int32 on the DEVICE; the rows n .. k are -1, -1 and NaN, so
 * every output byte is defined.  L in [2, 32768], k in [1, 65536], min_sep in [1, 32768]; min_sep >= L is legal and gives count = 0.
 * How: values map to unsigned 64-bit keys that are strictly monotone in v (zero canonicalised; negatives with every bit flipped,
 * the others with the sign bit flipped); the k-th largest key is found by a radix select over 8-bit digits with integer histograms;
 * records above it are compacted, and of the records equal to it those with the smallest row-major index win (per-block counts, an
 * exclusive sum in index order); the n selected records are ranked by counting the records that precede each.  Integer atomic adds
 * are used for counts and slots only; no output bit depends on the order in which they land, and every run gives the same bytes.
 * workspace: rnamsm_top_pairs_workspace_bytes(L, k) bytes (0 outside the limits of L and k), 256-byte aligned.  Every refusal -- a
 * limit, ld < L, a null pointer, a workspace that is short or misaligned -- comes before the first launch, names the offending value
 * (rnamsm_last_error) and touches no output.  Asynchronous: the call waits for nothing and reads nothing back. */
size_t rnamsm_top_pairs_workspace_bytes(int L, int k);
int rnamsm_top_pairs_f64(const double* x, int L, int64_t ld, int min_sep, int k, int32_t* pairs, double* scores, int32_t* count,
                         void* workspace, size_t workspace_bytes, void* stream);
int rnamsm_top_pairs_f32(const float* x, int L, int64_t ld, int min_sep, int k, int32_t* pairs, double* scores, int32_t* count,
                         void* workspace, size_t workspace_bytes, void* stream);

/* A pair map against a target structure, counted on the device: the reference's rna_compute_precisions (the threshold sweep) and
 * compute_precisions (precision among the top-ranked pairs), utils/metrics.py, as exact integer counts.  Shared by both calls:
 *   x [L, L] with leading dimension ld >= L, float64 (_f64) or float32 (_f32); target int8 [L, L] with leading dimension ld_t >= L;
 *   L in [2, 32768].  min_sep in [1, 32768] is the least j - i, as in rnamsm_top_pairs_*; min_sep >= L is legal and leaves no
 *   candidate.  The Python wrappers named after the reference translate: the sweep's `minsep` is min_sep - 1 (its mask is
 *   triu(minsep + 1)), compute_precisions' `minsep` is min_sep.
 *   ONLY candidate elements of x and target are read: never the diagonal, the lower triangle, the band closer than min_sep or the
 *   padding beyond column L.  A pair's value is v = (double)x[i, j] (exact for float32).
 * rnamsm_pair_sweep_*: skip uint8 [L] on the device or NULL; a position with a non-zero byte drops its whole row and column (the
 *   reference's missing_nt_index).  thresholds float64 [T] on the device, T in [1, 4096], strictly ascending and finite: that is the
 *   caller's contract (the Python wrapper checks it before the upload; the device does not).
 *   Candidates: the pairs i < j with j - i >= min_sep where neither i nor j is skipped.  A candidate is POSITIVE iff
 *   target[i, j] != 0.  Its bin is the number of thresholds with v >= thresholds[t]: NaN gives 0, as np.greater_equal does; +inf and
 *   -inf are ordinary values.  counts int64 [4, T], the rows tp, fp, tn, fn: tp[t] = the positives with bin > t, fp[t] = the negatives
 *   with bin > t, fn[t] = P - tp[t], tn[t] = N - fp[t] (P, N = all positives, all negatives).  The counts add over a dataset.
 *   How: a block streams row pieces with the thresholds and a histogram of 2 * (T + 1) bins in LDS (a binary search of at most 12
 *   steps per value, equal bins added once per wave), adds one 64-bit integer per used bin into a global table, and one block takes
 *   the suffix sums.  workspace: rnamsm_pair_sweep_workspace_bytes(T) bytes (0 outside the limits of T), 256-byte aligned.
 * rnamsm_pair_precision_*: Candidates: the pairs i < j with j - i >= min_sep, j - i < max_sep when max_sep > 0 (0 = no upper limit),
 *   target[i, j] >= 0 (a negative target is invalid, as in the reference) and x[i, j] not NaN.  They are ranked by the rule of
 *   rnamsm_top_pairs_*: larger v first, then smaller i, then smaller j.  n = min(k, the number of candidates), k in [1, 65536].
 *   cuts int32 [ncuts] on the device, ascending, each in [1, k] (the caller's contract; a cut is read as min(max(cut, 0), n)),
 *   ncuts in [1, 64].  hits int32 [ncuts]: hits[c] = the number of the first min(cuts[c], n) ranked pairs whose target is > 0.
 *   *count = n, an int32 on the DEVICE.  pairs (int32 [k, 2]) and scores (float64 [k]) are optional (NULL = not wanted) and defined as
 *   in rnamsm_top_pairs_*.  With fewer than k candidates the list ends at n and the rest count as misses (the reference ranks its
 *   -inf-filled pairs there and sums their targets).
 *   How: a copy of the candidate band with NaN at the excluded pairs goes through rnamsm_top_pairs_* unchanged; one block gathers the
 *   target at the n listed pairs, scans it and reads the sums at the cuts.  workspace:
 *   rnamsm_pair_precision_workspace_bytes(L, k, elem_bytes) bytes with elem_bytes = 8 (_f64) or 4 (_f32) (0 outside the limits),
 *   256-byte aligned; it holds the L x L copy.
 * Integer atomic adds are used for counts only; no output bit depends on the order in which they land, and every run gives the same
 * bytes.  Every refusal -- a limit, ld < L, ld_t < L, a null pointer, a workspace that is short or misaligned -- comes before the
 * first launch, names the offending value (rnamsm_last_error) and touches no output.  Asynchronous: the calls wait for nothing and
 * read nothing back. */
size_t rnamsm_pair_sweep_workspace_bytes(int T);
int rnamsm_pair_sweep_f64(const double* x, int L, int64_t ld, const int8_t* target, int64_t ld_t, const uint8_t* skip, int min_sep,
                          const double* thresholds, int T, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int rnamsm_pair_sweep_f32(const float* x, int L, int64_t ld, const int8_t* target, int64_t ld_t, const uint8_t* skip, int min_sep,
                          const double* thresholds, int T, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
size_t rnamsm_pair_precision_workspace_bytes(int L, int k, int elem_bytes);
int rnamsm_pair_precision_f64(const double* x, int L, int64_t ld, const int8_t* target, int64_t ld_t, int min_sep, int max_sep, int k,
                              const int32_t* cuts, int ncuts, int32_t* hits, int32_t* count, int32_t* pairs, double* scores,
                              void* workspace, size_t workspace_bytes, void* stream);
int rnamsm_pair_precision_f32(const float* x, int L, int64_t ld, const int8_t* target, int64_t ld_t, int min_sep, int max_sep, int k,
                              const int32_t* cuts, int ncuts, int32_t* hits, int32_t* count, int32_t* pairs, double* scores,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Whole forward, K0..K10 for one MSA, driven from C++ so that one call enqueues every launch
 * (MSATransformer.forward, model.py:338-416, with repr_layers=[num_layers], need_head_weights=True,
 * lm_head / contact head omitted -- their results are unused by the CLI).
 *
 * Weights are passed as a table of device pointers in the order documented for
 * rnamsm_weight_index (fused QKV is packed by the caller: Wqkv [3D, D] = q;k;v rows). */
typedef struct {
    int num_layers, embed_dim, num_heads, ffn_dim, vocab, num_positions, pad_idx;
    float ln_eps;
    /* msa_position_embedding: 0 or 1 = one scalar per alignment row, weights[RNAMSM_W_ROW_POS] = [1024] (the RNA-MSM
     * model, model.py:293-296: shape (1,1024,1,1)); embed_dim = one VECTOR per alignment row, [1024, embed_dim] (the msm/
     * variant of the shell, msm/model.py:289-292: shape (1,1024,1,emb_dim)).  A trailing field: an initialiser written for
     * ABI 3.x leaves it 0. */
    int row_pos_dim;
} rnamsm_model_dims;

enum {
    RNAMSM_W_EMBED_TOKENS = 0, RNAMSM_W_EMBED_POSITIONS, RNAMSM_W_ROW_POS,
    RNAMSM_W_LN_BEFORE_G, RNAMSM_W_LN_BEFORE_B, RNAMSM_W_LN_AFTER_G, RNAMSM_W_LN_AFTER_B,
    RNAMSM_W_GLOBAL_COUNT
};
enum { /* per layer, offset RNAMSM_W_GLOBAL_COUNT + layer * RNAMSM_W_LAYER_COUNT */
    RNAMSM_WL_ROW_LN_G = 0, RNAMSM_WL_ROW_LN_B, RNAMSM_WL_ROW_WQKV, RNAMSM_WL_ROW_BQKV,
    RNAMSM_WL_ROW_WO, RNAMSM_WL_ROW_BO,
    RNAMSM_WL_COL_LN_G, RNAMSM_WL_COL_LN_B, RNAMSM_WL_COL_WQKV, RNAMSM_WL_COL_BQKV,
    RNAMSM_WL_COL_WO, RNAMSM_WL_COL_BO,
    RNAMSM_WL_FFN_LN_G, RNAMSM_WL_FFN_LN_B, RNAMSM_WL_FC1_W, RNAMSM_WL_FC1_B,
    RNAMSM_WL_FC2_W, RNAMSM_WL_FC2_B,
    RNAMSM_W_LAYER_COUNT
};

/* max_tokens_per_msa: the reference's chunking budget (MSATransformer.max_tokens_per_msa_, model.py:418-428).  Without
 * padding chunking only re-orders sums and the value is ignored; with has_padding and R*C > max_tokens_per_msa the row
 * attention reproduces the chunked path's per-chunk mask fill (above; the partial-slab region grows to one slab per
 * chunk and, in the 16-bit modes, that MSA runs on the exact-fp32 kernels).  0 = never chunk. */
size_t rnamsm_forward_workspace_bytes(const rnamsm_model_dims* dims, int R, int C, int has_padding, int max_tokens_per_msa);
/* tokens int64 [R,C]; weights: host array of (RNAMSM_W_GLOBAL_COUNT + L*RNAMSM_W_LAYER_COUNT)
 * device pointers; workspace >= rnamsm_forward_workspace_bytes; row_attn [L,H,C,C] (full, with
 * <cls>), repr [R*C, D] (after emb_layer_norm_after), emb [C-1, D], atp [L*H, C-1, C-1]; all four are
 * required outputs.  has_padding != 0: the MSA contains <pad> tokens; the driver builds the padding mask and applies
 * the reference's mask semantics (§8 f2): zeroed embeddings and q at padded tokens, -10000 on keys whose first-row token
 * is <pad> (row attention; per row chunk when R*C > max_tokens_per_msa) and on padded keys (column attention). */
/* weight_planes (host array, may be NULL when dtype == RNAMSM_F32): for every layer 12 device pointers to bf16 planes
 * from rnamsm_split_bf16, in the order {row_wqkv, row_wo, col_wqkv, col_wo, fc1_w, fc2_w} x {hi, lo} (lo may be
 * NULL for RNAMSM_BF16). */
#define RNAMSM_PLANES_PER_LAYER 12
/* ln_folded (host array, may be NULL = separate LayerNorm launches): for every layer 9 device pointers from
 * rnamsm_ln_fold_weights, {Wg, c, d} for {row QKV [3D,D] with the row LayerNorm, column QKV with the column LayerNorm,
 * fc1 [F,D] with the FFN LayerNorm}.  Used by the exact path on MSAs without padding (knob "ln_fold"). */
#define RNAMSM_FOLDED_PER_LAYER 9
/* ln_folded16 (host array, may be NULL): the same for the 16-bit modes (planes end to end, "attn16" on, no padding): for
 * every layer 12 device pointers {Wg_hi, Wg_lo (NULL for RNAMSM_BF16), c, d} for {row QKV, column QKV, fc1}; Wg planes =
 * rnamsm_split_bf16(W * gamma) in the mode's format, c = row sums of the plane values (rnamsm_gemm16_lnfold). */
#define RNAMSM_FOLDED16_PER_LAYER 12
/* outputs: RNAMSM_OUT_REPR = the whole final representation repr [R*C, D] is wanted (MSATransformer.forward's
 * representations[num_layers]).  Without it only what extract_feat writes is produced -- emb (alignment row 0) and atp
 * (RNA_MSM_Inference.py:151-166) -- and the last layer stops computing the other rows once its tied row attention is done:
 * K and V of the last column attention still cover every row, but its queries, out_proj, the last FFN and the final
 * LayerNorm run on row 0's C tokens only (~5 % of the forward at M=256 L=512).  emb and atp are bit-identical either
 * way; repr then holds valid data in its first C rows only.  (Exact path without padding; otherwise the flag is ignored
 * and everything is computed.) */
#define RNAMSM_OUT_REPR 1
/* err_flag (device int, may be NULL) collects, OR-ed by the kernels: bit 0 a token / position index outside its table (K0,
 * clamped); bit 1 the folded LayerNorm's precondition failed for some row (K1 folded; redo with ln_folded = NULL); bit 2
 * (RNAMSM_ERR_NONFINITE) an emb / atp value is inf or NaN (K10 inspects every value it packs) -- in the 16-bit modes that is
 * how an operand outside fp16 range shows, and the caller should redo the MSA with dtype RNAMSM_F32.  One word, one read. */
#define RNAMSM_ERR_NONFINITE 4
int rnamsm_forward(const rnamsm_model_dims* dims, const float* const* weights, const int64_t* tokens,
                   int R, int C, void* workspace, size_t workspace_bytes,
                   float* row_attn, float* repr, float* emb, float* atp,
                   int* err_flag, int has_padding, int max_tokens_per_msa, int outputs, int dtype,
                   const uint16_t* const* weight_planes, const float* const* ln_folded,
                   const void* const* ln_folded16, void* stream);

/* B same-shape MSAs -- ragged ones padded to one shape with <pad> -- through one set of token-parallel launches:
 * MSATransformer.forward(tokens[B,R,C]) (model.py:338-416), exact path.  Why it exists: below ~4 k tokens a forward costs 5.5-6 ms whatever the
 * alignment holds (each of its ~140 dependent launches lasts one block's serial time on a mostly idle chip); LayerNorm, the
 * Linear GEMMs and the final LayerNorm are per token and run ONCE over the B*R*C tokens of the batch, only the embedding
 * (row positions restart per MSA) and the attention kernels (they couple the tokens of one MSA) are launched per MSA.
 * tokens int64 [B,R,C]; row_attn [B,L,H,C,C]; repr [B,R*C,D]; emb [B,C-1,D]; atp [B,L*H,C-1,C-1]; err_flag as in
 * rnamsm_forward; has_padding != 0: the batch contains <pad> and the reference's direct-path mask semantics apply (as in
 * rnamsm_forward; the chunked path's per-chunk fill is not offered here -- callers keep R*C <= max_tokens_per_msa or use
 * rnamsm_forward per MSA); ln_folded as in rnamsm_forward or NULL (ignored with padding).
 * true_rows (device int32 [B], or NULL = the reference's batch semantics): RAGGED batches -- alignments of different shapes
 * padded into one [R, C] frame (rows and columns appended) that must come out as each would ALONE.  A padded element already
 * equals its unpadded forward in everything (masked keys get probability exactly 0, padded queries are zeroed, padded values
 * never reach a real token) except one number: the reference scales the tied logits by 1/sqrt(R) of the PADDED depth
 * (align_scaling, modules.py:713-715).  With true_rows[b] = the real depth of MSA b that factor is applied per MSA, and
 * emb[b, :C_b-1], atp[b, :, :C_b-1, :C_b-1] equal rnamsm_forward's outputs on the unpadded MSA b to fp32 rounding.  Every MSA's outputs equal rnamsm_forward's on that MSA alone up
 * to fp32 rounding (bit-identical when the two shape-dependent choices agree: fc2 split-K and the folded LayerNorm are
 * decided by the batch's token count).  B*R*C must fit 31 bits.
 * dtype / weight_planes as in rnamsm_forward (round 3): the 16-bit modes run the same plane data flow -- LayerNorm-split, the
 * plane GEMMs, K4'..K7' with the MSA on gridDim.y; in a ragged batch the tied logits are scaled per MSA on the fp32
 * accumulators (q stays unscaled in the planes) -- and need the "attn16" knob on; which GEMM kernel runs depends on the
 * batch's token count, so an element agrees with its lone forward to the mode's rounding, not bit for bit. */
size_t rnamsm_forward_batch_workspace_bytes(const rnamsm_model_dims* dims, int B, int R, int C);
int rnamsm_forward_batch(const rnamsm_model_dims* dims, const float* const* weights, const int64_t* tokens, int B, int R, int C,
                         void* workspace, size_t workspace_bytes, float* row_attn, float* repr, float* emb, float* atp,
                         int* err_flag, int has_padding, const int* true_rows, const float* const* ln_folded, int dtype,
                         const uint16_t* const* weight_planes, void* stream);

/* B alignments of DIFFERENT shapes as one TOKEN-PACKED batch (round 4): no frame, no padding.  The reference
 * feeds short RNAs of unlike length and depth one by one (RNA_MSM_Inference.py:141-148, model.py:338-416 per MSA); a padded
 * frame of such alignments (rnamsm_forward_batch with true_rows) holds 1.4-1.5x their real tokens.  Here the alignments lie
 * back to back on the token axis and every output is the concatenation of what rnamsm_forward returns per alignment:
 *   tokens   int64 [T], T = sum R_b*C_b: alignment 0's [R_0, C_0] row-major, then alignment 1's, ... (device)
 *   shapes   int32 [B][2] = {R_b, C_b} on the HOST (read during the call; 1 <= R_b <= 1024, 2 <= C_b)
 *   row_attn [sum L*H*C_b*C_b]   repr [T, D]   emb [sum (C_b-1)*D]   atp [sum L*H*(C_b-1)^2]   (device, fp32)
 * The per-token launches (LayerNorm, the six GEMMs of a layer) run once over the T real tokens; K0, K4-K7 and K10 take the
 * alignment from gridDim.y and its shape / offsets from a descriptor table the call writes into the workspace.  Every
 * alignment keeps the tied-logit slab split of its own forward; q carries dh^-1/2 and the alignment's 1/sqrt(R_b)
 * (align_scaling, modules.py:713-715) multiplies its summed logits -- the arithmetic of rnamsm_forward itself since round 5 --
 * fc2 is never split and LayerNorm is folded only where every member's own forward folds it (>= 4096 tokens each; with ln_folded given
 * and the by-shape rule in force a table that mixes the two classes is REFUSED with RNAMSM_ERR_INVALID: hand it over as two
 * batches, one per class, as the Python mirror does): with
 * RNAMSM_F32 every alignment's outputs are rnamsm_forward's BIT FOR BIT (tests/test_gpu_forward.py).  A packed batch builds no
 * masks: <pad> inside it sets bit 3 (value 8) of *err_flag and the caller reruns that batch framed.
 * dtype RNAMSM_BF16 / RNAMSM_F16X3 (round 5; weight_planes as in rnamsm_forward, NULL for RNAMSM_F32): every Linear runs on the
 * 16-bit matrix cores over the T packed tokens (LayerNorm and fc1 write operand planes); the attention contractions stay on
 * the exact-fp32 descriptor kernels K4-K7 (a few per cent of a batch of small alignments).  An alignment then equals its own
 * 16-bit forward to the mode's rounding.  ln_folded as in rnamsm_forward or NULL (fp32 only).
 * rnamsm_forward_packed_workspace_bytes returns 0 for a shape outside the limits. */
#define RNAMSM_ERR_PAD_IN_PACKED 8
size_t rnamsm_forward_packed_workspace_bytes(const rnamsm_model_dims* dims, int B, const int* shapes);
int rnamsm_forward_packed(const rnamsm_model_dims* dims, const float* const* weights, const int64_t* tokens, int B,
                          const int* shapes, void* workspace, size_t workspace_bytes, float* row_attn, float* repr, float* emb,
                          float* atp, int* err_flag, const float* const* ln_folded, int dtype,
                          const uint16_t* const* weight_planes, void* stream);

/* Per-kernel timing with HIP events recorded on the launch stream (measurement aid for bench.py's
 * roofline block; adds two event records per launch while enabled, nothing when disabled).
 *   rnamsm_timing_enable(1) ... enqueue work ... (caller synchronises the stream) ... rnamsm_timing_collect()
 * collect folds every completed (start, stop) pair into per-category totals and returns the number of
 * categories; rnamsm_timing_get reads one: name, launches, total milliseconds, total algorithmic flops and bytes
 * (the figures DESIGN.md derives per kernel).  rnamsm_timing_reset clears the totals. */
int rnamsm_timing_enable(int on);
int rnamsm_timing_collect(void);
int rnamsm_timing_get(int category, const char** name, long long* launches, double* ms, double* flops, double* bytes);
/* Roofline terms of the timed launches of a category: bound_ms = sum over launches of max(executed matrix flops / the dense
 * peak of the launch's MFMA family, algorithmic bytes / the achievable HBM rate), plus both terms summed separately
 * (peaks from MI355X_MICROARCH.md: 157.3 TFLOP/s fp32 MFMA, 2.5 PFLOP/s bf16 / f16 MFMA, 6.3 TB/s HBM).  bound_ms / ms is
 * the fraction of its own roofline a kernel family reached (bench.py's `roofline` of the 16-bit modes). */
int rnamsm_timing_get_bound(int category, double* bound_ms, double* mfma_ms, double* hbm_ms);
/* Third roofline term, for the kernels whose softmax can out-weigh their contractions (the fused column attention at head_dim
 * 64): the launches' vector-ALU issue time, (plain instructions + 4 x transcendentals) per score x scores / (1024 SIMDs x
 * 32 lanes x 2.4 GHz).  bound_ms of rnamsm_timing_get_bound is the per-launch max over all three terms. */
int rnamsm_timing_get_valu_bound(int category, double* valu_ms);
void rnamsm_timing_reset(void);

/* Knobs: process-global selectors between SHIPPED kernels / arithmetic rules, for in-process A/B measurements and for the tests that
 * compare two kernels on the same input.  14 names since round 6 (round 5 had 24: the ten whose A/B was closed -- gemm16_persist,
 * gemm16_stagger, gemm16_dephase, gemm16_big_rows, gemm16_big_rows_fwd, row16_q16, row16_bk64, row_narrow_rows, gemm_flat_tiles, row_vt --
 * are constants now, the losing code paths are gone; rnamsm_set_param answers RNAMSM_ERR_INVALID for them).  rnamsm_set_param takes
 * the knob table's lock exclusively and REFUSES (RNAMSM_ERR_INVALID) while a forward driver is enqueuing on another thread.
 *   "gemm16_dma"  staging of the plane-input 16-bit GEMMs: 0 register-staged, 1 (or 2) LDS-DMA 128x128 tile,
 *                 3 (default) = LDS-DMA 256x256 tile when the problem allows, software-pipelined fragment
 *                 reads and a mid-tile barrier (K tile 64 deep for plain bf16, 32 for the hi/lo modes), 4 = 3 with
 *                 32-deep K tiles for every mode.  Speed only.
 *   "gemm16_mfma16"  plain-bf16 256x256 GEMM: 1 (default) = the 16x16x32-MFMA kernel for N > 1024 or K >= 2048, 2 = for every shape,
 *                 0 = the 32x32x16 kernel.  Results agree to fp32 rounding (the k order inside a step differs).
 *   "gemm_group"  GEMM block order (fp32 kernel and the 256x256 16-bit kernel): row panels per XCD group (0 = chosen
 *                 from the shape, default: 8 for N > 1024, else 1 -- and the fp32 kernel deals a GEMM of <= 512 tiles flat,
 *                 tile = block id; 1 = whole panels).  An XCD's panels beyond its full groups form one smaller group: no padding
 *                 groups.  Changes HBM-side traffic and speed, never results.
 *   "gemm_tile"   fp32 GEMM block tile: 0 (default) = 128x128, or 128x64 where that evens out the last round of blocks
 *                 on a small problem, or MIXED (whole rounds of 128x128 tiles, the tile positions of the last,
 *                 partly empty round cut into their two 128x64 halves); 1 = always 128x128; 2 = always 128x64; 3 = mixed
 *                 wherever a launch has both whole rounds and a tail; 4 = by shape among the two uniform tilings only.
 *                 Results are bit-identical under every tiling: each output element sums its K products in the same order.
 *   "gemm_splitk_short"  rnamsm_forward*, the K = 768 GEMMs of a lone small alignment (<= 192 tiles): 0 (default) = off, 2 / 4 = that
 *                 many K ranges with the epilogue applied by the reduction pass (A/B: no gain once the block order was fixed).
 *   "row_narrow"  fp32 rnamsm_row_logits / rnamsm_row_apply at C <= 64: 1 (default) = the LDS-free narrow kernels, 0 = the
 *                 128x128 tile kernels.  Speed only, results bit-identical.
 *   "col_small"   fp32 rnamsm_col_attn_fused at R <= 16: 1 (default) = one wave per (column, head) on v_mfma_f32_16x16x4_f32,
 *                 no LDS; 0 = the 128-query-block kernels.  Results agree to fp32 rounding.  Plane output (ctx_hi) comes from the
 *                 same kernel as the fp32 context under either value: the planes are the split of exactly those fp32 values.
 *   "col_fast"    rnamsm_col_attn_fused_prescaled: 1 (default) = first pass without a running maximum, the online softmax as the
 *                 fallback of a block whose row sums leave [2^-64, 2^100]; 0 = the online softmax only (results agree to rounding).
 *   "col_dma"     fp32 rnamsm_col_attn_fused: 1 = K/V chunks staged by LDS-DMA, 32-key chunks, three blocks per CU;
 *                 0 = register-staged 64-key chunks, two blocks per CU; -1 (default) = chosen from the shape.  Speed only
 *                 (the two kernels run the same arithmetic per 32-key tile; results agree to fp32 rounding).
 *   "row16_max_rows"  hi/lo modes of rnamsm_row_logits16: cap on the rows of one partial slab (default 32, 0 = none).
 *                 Shorter fp32 accumulation chains; changes results at the rounding level (and the slab count).
 *   "greedy_fused"  rnamsm_greedy_select: 1 (default) = one launch per step (one wave per row) for alignments of up to 3072
 *                 rows, three launches per step (one thread per row) above; 2 = always one; 0 = always three.  Same indices.
 *   "ln_fold"     rnamsm_forward with ln_folded given: 1 (default) = LayerNorm folded into the QKV / fc1 GEMMs, row sums
 *                 left by the out_proj / fc2 epilogues, for MSAs of R*C >= 4096 tokens (rnamsm_get_param("ln_fold_min_tokens"); below that the separate launches
 *                 are faster); 3 = for every shape, and in the 16-bit modes too (ln_folded16; measured neutral there, hence
 *                 not the default); 2 = folded, every GEMM sums the rows it stages itself; 0 = separate LayerNorm launches
 *                 (all agree to fp32 rounding, resp. to the 16-bit mode's rounding).
 *   "gemm_splitk" exact path of rnamsm_forward, fc2 (K = ffn_dim >= 2048) of MSAs with at most 64 output tiles (below ~1.4 k
 *                 tokens): 0 (default since round 5) = never; 1 = four K ranges computed side by side into partial tiles of the
 *                 workspace and added in range order with the bias and the residual (bit-identical reruns; results differ
 *                 from the unsplit GEMM at the fp32 rounding level -- and the choice follows the token count of whatever
 *                 batch the alignment is computed in, which is why it is off by default: an alignment's emb / atp are the
 *                 same bits alone, in a same-shape batch and token-packed); 2 / 4 / 8 = that many ranges whenever
 *                 tiles x ranges <= 512 (A/B).
 *   "attn16"      16-bit modes of rnamsm_forward: 1 (default) = the attention contractions also run on the 16-bit
 *                 matrix cores in the mode's operand format (K4'..K7'), 0 = they stay on the exact-fp32 kernels,
 *                 2 = as 1 but the row kernels keep 128x128 tiles for every C (A/B of the 256x256-tile kernels);
 *                 rnamsm_col_attn16 only: 4 = one 32-query block per wave for every R, 5 = the TRACKED (online-softmax) loop for
 *                 every format (A/B, and the reference the FAST loop's fallback is tested against).
 *                 The RNAMSM_F32 path is not affected by either.
 *   "seqid_filter_chunk"  rnamsm_seqid_filter (added after round 6, the fifteenth name): the positions of the order one block
 *                 resolves per step of a pass, a multiple of 64 in [64, 512] (anything else is refused), default 256.  Every value
 *                 gives the same indices; smaller chunks mean more launches, larger ones a longer one-block stage.
 * Threading: the knobs are process-global and are read on the host while a call enqueues its launches.  Change them only between
 * calls; while any thread is inside rnamsm_forward / _forward_batch / _forward_packed, rnamsm_set_param changes nothing and returns
 * RNAMSM_ERR_INVALID (the one per-forward choice that used to be a knob write, the 16-bit GEMM tile threshold, is thread-local). */
int rnamsm_set_param(const char* name, int value);
int rnamsm_get_param(const char* name);

#ifdef __cplusplus
}
#endif
#endif /* RNAMSM_H_ */
