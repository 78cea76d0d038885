/* mi355fa_kvcache_fp8_token.h -- decoding attention over a KV cache of OCP e4m3 bytes with ONE FP32 SCALE PER CACHED TOKEN AND
 * K/V HEAD, computed when the token is appended: padded, paged, and with packed variable-length queries, in libmi355fa.so.
 *
 * A companion to mi355fa_kvcache_fp8.h, mi355fa_paged.h and mi355fa_ragged.h (included below for the decoding conventions:
 * shapes, cache_seqlens, the bottom-right mask, the split workspace, pages and the block table, packed queries and
 * cu_seqlens_q; mi355fa.h, its ABI version and every other header's function list are unchanged).  Inference only.
 *
 * Why: mi355fa_kvcache_fp8.h's k_descale[b, hk] is fixed for the life of a sequence, so its user must know every future key's
 * amax before the first append.  Here a row brings its own scale: no calibration pass, and one outlier token costs the other
 * tokens nothing.  The price is 4 bytes per D-byte row.
 *
 * The format:
 *   Caches        e4m3 bytes exactly as in mi355fa_kvcache_fp8.h (torch.float8_e4m3fn): padded [B, H_kv, S_cache, D], paged pools
 *                 [num_pages, H_kv, page_size, D]; byte strides that are multiples of 16; transposed storage is read in place.
 *   Scales        float32 tensors k_scale, v_scale of their own with the cache's dimension order and no last dimension: padded
 *                 [B, H_kv, S_cache], paged [num_pages, H_kv, page_size], with their own {batch-or-page, head, row} strides
 *                 counted in ELEMENTS.  Any non-negative strides are taken, so [B, S_cache, H_kv] storage is read in place.
 *   Value         K[b, hk, j, :] = float(k_cache[b, hk, j, :]) * k_scale[b, hk, j]; V likewise.  No per-(sequence, head) factor on
 *                 top.  A scale that is not a finite normal number > 0 gives unspecified results, as does an e4m3 NaN byte.
 *                 Rows at or past L_b are never read, in the caches or in the scales.
 *   Exactness     K's bytes become q's dtype without rounding (every e4m3 value is a normal fp16 and bf16 number), and a key's
 *                 scale multiplies its fp32 score: S = (q . bytes) * k_scale * softmax_scale.  V's scale s = 2^e * m, 1 <= m < 2,
 *                 is split: the bytes are converted with the row's scale as the conversion's operand, of which the
 *                 instruction takes 2^e alone (below), so V enters the matrix product as byte * 2^e -- exact wherever q's
 *                 dtype represents it, its subnormals included --, and m multiplies the fp32 probability of the key before
 *                 that is rounded to q's dtype: a factor below 2, so nothing small meets fp16.
 *                 (The full scale on the probabilities would make them fp16 subnormals at v_scale ~ 2^-15.)
 *                 The conversion, v_cvt_scalef32_pk_{f16,bf16}_fp8, was NOT found to be one rounding of byte * scale for an
 *                 arbitrary fp32 scale: it reads the exponent field of its scale operand alone, as an e8m0 byte, and ignores
 *                 the mantissa -- what the MXFP4 conversions do (mi355fa_kvcache_fp4.h).  With a power of two it delivers
 *                 byte * 2^e without rounding, results subnormal in q's dtype included; a product past q's largest finite
 *                 number (fp16: byte * 2^e > 65504, v_scale >= 256 at the largest byte) is unspecified.
 *                 tests/test_gpu_fp8_token_scales.py holds this over every code but the two NaN bytes, per dtype.
 *                 With every scale 1.0 the result has the bits of fa_fwd_kvcache_fp8 without descales at the same split count.
 *
 * The quantiser (the append of k_new / v_new, and quantize_kv_fp8_per_token in fp8_token_kvcache.py), per row of D elements:
 *   1. amax = max |float(x)| over the row.
 *   2. s = amax / 448.0f, an fp32 IEEE division.  If s is not a normal fp32 number (a zero row, a subnormal quotient), s = 1.0f.
 *   3. byte = e4m3_rne(clamp(float(x) / s, -448, 448)): divide, saturate, round to nearest even, -0.0 kept -- the cast
 *      mi355fa_kvcache_fp8.h documents.
 *   4. NaN and Inf inputs are unspecified.
 *   The append writes D bytes and one fp32 scale per (token, K/V head), through the table for pools.  Rows may cross pages.  Rows
 *   past the table, or whose table entry is outside the pool, are dropped, bytes and scale together.
 *
 *   D             : 64 or 128; packed queries (fa_fwd_kvcache_fp8_token_ragged) also 256.  D = 256 on the two rectangular calls
 *                   is refused with MI355FA_ERR_SHAPE, every other head dim with MI355FA_ERR_HEAD_DIM.  A padded cache
 *                   [B, H_kv, S_cache, D] with S_cache % 32 == 0 goes into the packed call as a pool of B pages of S_cache keys
 *                   whose table is {0, 1, .., B - 1} with max_pages_per_seq = 1.
 *   k_cache/v_cache: as in mi355fa_kvcache_fp8.h: 16-byte aligned (MI355FA_ERR_ALIGN); opts->k_strides / v_strides in elements
 *                   (= bytes) {batch-or-page, head, row}, multiples of 16, the row stride at least D (MI355FA_ERR_STRIDE); NULL =
 *                   contiguous.  K and V share their row stride.
 *   k_scale/v_scale: float32, 4-byte aligned (MI355FA_ERR_ALIGN), not NULL (MI355FA_ERR_NULL).  k_scale_strides / v_scale_strides:
 *                   ELEMENT strides {batch-or-page, head, row}, non-negative (MI355FA_ERR_STRIDE); NULL = contiguous.  One
 *                   (batch-or-page, head) slice stays below 2^31 bytes (MI355FA_ERR_STRIDE).
 *   k_new / v_new : [B, H_kv, S_new, D] (packed: [total_q, H_kv, D]) in `dtype`, contiguous, or both NULL.  Quantised as above
 *                   into the rows [cache_seqlens[b], cache_seqlens[b] + S_new) of the caches AND of the scale tensors before
 *                   attention.
 *   sinks         : NULL, or one fp32 DEVICE logit per query head as in mi355fa_sink.h (4-byte aligned).
 *   page_size     : a positive multiple of 32 (MI355FA_ERR_PAGED otherwise); the other paged arguments as in mi355fa_paged.h,
 *                   the packed ones (cu_seqlens_q, total_q, the packed q / o strides, MI355FA_ERR_RAGGED) as in mi355fa_ragged.h.
 *   There is no kv_dtype argument, and no soft-cap or ALiBi form.
 *
 * The host reads none of cache_seqlens, block_table, cu_seqlens_q or the scales, so a captured step replays while all of them
 * change.  The workspace functions return n * rows * (D + 2) * 4 bytes (0 when n = 1) with rows = B * H * S_q, the formula of
 * mi355fa_kvcache.h; the packed one roundup16(16 + 8 * NB_max) + (n > 1 ? n * H * total_q * (D + 2) * 4 : 0), never 0, the
 * formula of mi355fa_ragged.h.  The split count n is the e4m3 path's rule (the D = 256 rule at D = 256).  The masks, rows with no
 * visible key (O = 0, LSE = -inf), determinism and the error codes are those of the parents; every argument error is reported
 * before anything is enqueued.  The paged call has the bits of the padded call on the gathered cache and scales, and the rows
 * of a sequence in the packed call the bits of the paged call on that sequence alone (D = 64, 128).
 */
#ifndef MI355FA_KVCACHE_FP8_TOKEN_H_
#define MI355FA_KVCACHE_FP8_TOKEN_H_
#include "mi355fa_kvcache_fp8.h"
#include "mi355fa_paged.h"
#include "mi355fa_ragged.h"
#ifdef __cplusplus
extern "C" {
#endif
long long fa_fwd_kvcache_fp8_token_workspace_bytes(int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D);
int fa_fwd_kvcache_fp8_token(const void* q, void* k_cache, void* v_cache, float* k_scale, float* v_scale, const void* k_new,
                             const void* v_new, const int* cache_seqlens, const long long* k_scale_strides,
                             const long long* v_scale_strides, const float* sinks, void* o, float* lse, void* workspace,
                             long long workspace_bytes, int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D,
                             int dtype, float scale, int window_left, int window_right, const mi355fa_opts* opts,
                             void* stream);
long long fa_fwd_kvcache_fp8_token_paged_workspace_bytes(int B, int H, int H_kv, int S_q, int max_pages_per_seq, int page_size,
                                                         int S_new, int D);
int fa_fwd_kvcache_fp8_token_paged(const void* q, void* k_pool, void* v_pool, float* k_scale, float* v_scale, const void* k_new,
                                   const void* v_new, const int* cache_seqlens, const int* block_table,
                                   const long long* k_scale_strides, const long long* v_scale_strides, const float* sinks,
                                   void* o, float* lse, void* workspace, long long workspace_bytes, int B, int H, int H_kv,
                                   int S_q, int num_pages, int page_size, int max_pages_per_seq, long long block_table_stride,
                                   int S_new, int D, int dtype, float scale, int window_left, int window_right,
                                   const mi355fa_opts* opts, void* stream);
long long fa_fwd_kvcache_fp8_token_ragged_workspace_bytes(int total_q, int B, int H, int H_kv, int max_pages_per_seq,
                                                          int page_size, int D);
int fa_fwd_kvcache_fp8_token_ragged(const void* q, void* k_pool, void* v_pool, float* k_scale, float* v_scale, const void* k_new,
                                    const void* v_new, const int* cu_seqlens_q, const int* cache_seqlens,
                                    const int* block_table, const long long* k_scale_strides,
                                    const long long* v_scale_strides, const float* sinks, void* o, float* lse, void* workspace,
                                    long long workspace_bytes, int total_q, int B, int H, int H_kv, int num_pages,
                                    int page_size, int max_pages_per_seq, long long block_table_stride, int D, int dtype,
                                    float scale, int window_left, int window_right, const mi355fa_opts* opts, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_KVCACHE_FP8_TOKEN_H_ */
