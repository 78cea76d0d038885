/* mi355fa_kvcache_fp4.h -- decoding attention over a KV cache stored as MXFP4 (OCP Microscaling v1.0: 4-bit e2m1 elements
 * with one shared e8m0 scale per 32 elements), padded or paged, in libmi355fa.so.
 *
 * A companion to mi355fa_kvcache.h and mi355fa_paged.h (included below for the decoding conventions: shapes, cache_seqlens,
 * the bottom-right mask, the split workspace, pages and the block table; mi355fa.h, its ABI version, mi355fa_paged_mods
 * and every other header's function list are unchanged).  Inference only.
 *
 * The format:
 *   Elements      e2m1: bit 3 sign, bits 2-1 exponent (bias 1), bit 0 mantissa; the values +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}.
 *   Packing       two elements per byte, element 2i in the low nibble and 2i + 1 in the high nibble
 *                 (torch.float4_e2m1fn_x2's packing, and the order gfx950's conversion instruction reads).
 *   Cache row     D elements = D / 2 bytes.
 *   Scales        each run of 32 consecutive elements of a row shares one e8m0 byte e, the value 2^(e - 127).  Byte 255 is
 *                 NaN: a block that carries it gives unspecified results.
 *   Scale tensor  a tensor of its own with the cache's dimension order and D / 32 bytes per row:
 *                 padded k_scale, v_scale [B, H_kv, S_cache, D / 32], paged [num_pages, H_kv, page_size, D / 32], with their
 *                 own {batch-or-page, head, row} strides, last dimension contiguous.  A transposed [.., S, H_kv, ..]
 *                 storage is read in place, as the caches are.
 *   Value         K[b, hk, j, d] = e2m1(k_cache nibble) * 2^(k_scale[b, hk, j, d / 32] - 127); V likewise.
 *   No per-tensor factor: there is no per-(sequence, head) fp32 descale in this call.
 *   Exactness     each such product that q's dtype represents is produced without rounding, so O and LSE are
 *                 fa_fwd_kvcache's on the dequantised cache, with the 16-bit kernel's error.  A product q's dtype cannot
 *                 represent gets what v_cvt_scalef32_pk_{f16,bf16}_fp4 gives, which is unspecified here.
 *                 This holds for every scale byte 0..254, byte 0 (2^-127) and products subnormal in q's dtype included:
 *                 all 16 codes for e in [104, 140] with fp16 and [0, 252] with bf16, fewer at the bytes beside them, and in
 *                 fp16 zeros alone below 101 and above 143 (tests/test_gpu_fp4_scales.py).
 *
 * The quantiser (the append of k_new / v_new, and quantize_kv_mxfp4 in fp4_kvcache.py), per 32-element block:
 *   1. amax = max |x| over the block.
 *   2. X = floor(log2(amax)) - 2, e = clamp(X + 127, 0, 254).  A block with amax = 0 gets e = 127 and all nibbles 0.
 *   3. Each element is x / 2^(e - 127) (= x / 2^X wherever the clamp does not bind), rounded to nearest even onto the e2m1
 *      grid, saturating at +-6.  -0.0 stays -0.0.
 *   4. NaN and Inf inputs are unspecified.
 *
 *   kv_dtype      : MI355FA_KV_MXFP4; anything else is refused with MI355FA_ERR_DTYPE.
 *   D             : 64 or 128.  D = 256 and every other head dim are refused with MI355FA_ERR_SHAPE by the two calls here; the
 *                   packed call of mi355fa_ragged_fp4.h takes D = 256, and a padded cache as a pool of B pages.
 *   k_cache/v_cache: [B, H_kv, S_cache, D / 2] bytes (paged: pools [num_pages, H_kv, page_size, D / 2]), 16-byte aligned
 *                   (MI355FA_ERR_ALIGN).  opts->k_strides / v_strides are BYTE strides {batch-or-page, head, row}, multiples
 *                   of 16, the row stride at least D / 2 (MI355FA_ERR_STRIDE); NULL = contiguous.  K and V share their row
 *                   stride.
 *   k_scale/v_scale: bytes as above, aligned to D / 32 bytes (MI355FA_ERR_ALIGN).  k_scale_strides / v_scale_strides are
 *                   byte strides {batch-or-page, head, row}, non-negative multiples of D / 32, the row stride at least
 *                   D / 32 (MI355FA_ERR_STRIDE); NULL = contiguous.  One (batch-or-page, head) slice stays below 2^31 bytes.
 *   k_new / v_new : [B, H_kv, S_new, D] in `dtype`, contiguous, or both NULL.  Quantised as above into the rows
 *                   [cache_seqlens[b], cache_seqlens[b] + S_new) of the caches AND of the scale tensors before attention
 *                   (paged: through the table; rows may cross pages; rows past the table, or whose entry is outside the
 *                   pool, are dropped).
 *   sinks         : NULL, or one fp32 DEVICE logit per query head as in mi355fa_sink.h (4-byte aligned).
 *   page_size     : a positive multiple of 32 (MI355FA_ERR_PAGED otherwise); the other paged arguments as in mi355fa_paged.h.
 *
 * The host reads none of cache_seqlens, block_table or the scales, so a captured step replays.  Rows at or past L_b are
 * never read, in the caches or in the scales.  The workspace functions return n * B * H * S_q * (D + 2) * 4 bytes (0 when
 * n = 1), the formula of mi355fa_kvcache.h / mi355fa_kvcache_fp8.h; the split count n is this path's own (the fp8 path's
 * split length with up to two workgroups per CU at both head dims) and may differ from theirs.  The masks, rows with no visible
 * key (O = 0, LSE = -inf), determinism and the error codes are those of mi355fa_kvcache.h / mi355fa_paged.h; every argument
 * error is reported before anything is enqueued.  Packed variable-length queries over MXFP4 pools are
 * mi355fa_ragged_fp4.h's call; soft-capping and ALiBi have no MXFP4 form.
 */
#ifndef MI355FA_KVCACHE_FP4_H_
#define MI355FA_KVCACHE_FP4_H_
#include "mi355fa_kvcache.h"
#include "mi355fa_paged.h"
#ifdef __cplusplus
extern "C" {
#endif
#define MI355FA_KV_MXFP4 1 /* kv_dtype: OCP MXFP4, e2m1 nibbles (torch.float4_e2m1fn_x2) + e8m0 block scales */
long long fa_fwd_kvcache_fp4_workspace_bytes(int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D);
int fa_fwd_kvcache_fp4(const void* q, void* k_cache, void* v_cache, void* k_scale, void* v_scale, const void* k_new,
                       const void* v_new, const int* cache_seqlens, const long long* k_scale_strides,
                       const long long* v_scale_strides, const float* sinks, void* o, float* lse, void* workspace,
                       long long workspace_bytes, int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D, int dtype,
                       int kv_dtype, float scale, int window_left, int window_right, const mi355fa_opts* opts, void* stream);
long long fa_fwd_kvcache_fp4_paged_workspace_bytes(int B, int H, int H_kv, int S_q, int max_pages_per_seq, int page_size,
                                                   int S_new, int D);
int fa_fwd_kvcache_fp4_paged(const void* q, void* k_pool, void* v_pool, void* k_scale, void* v_scale, const void* k_new,
                             const void* v_new, const int* cache_seqlens, const int* block_table,
                             const long long* k_scale_strides, const long long* v_scale_strides, const float* sinks, void* o,
                             float* lse, void* workspace, long long workspace_bytes, int B, int H, int H_kv, int S_q,
                             int num_pages, int page_size, int max_pages_per_seq, long long block_table_stride, int S_new,
                             int D, int dtype, int kv_dtype, float scale, int window_left, int window_right,
                             const mi355fa_opts* opts, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_KVCACHE_FP4_H_ */
