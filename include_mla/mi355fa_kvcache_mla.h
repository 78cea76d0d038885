/* mi355fa_kvcache_mla.h -- MLA (multi-head latent attention) decoding over a paged latent cache in libmi355fa.so: the absorbed
 * decode form of DeepSeek-V2 / V3 / R1 and Kimi-K2.
 *
 * A companion to mi355fa_paged.h (included below for the decoding conventions and the error codes; mi355fa.h, its ABI version
 * and every other header's function list are unchanged).  The header lives in include_mla/, beside include/ and include_quant/,
 * whose listings are recorded sets.  Inference only: there is no backward.
 *
 * A query head has 576 dims: [0, 512) the absorbed no-RoPE ("latent") part, [512, 576) the RoPE part.  The cache holds ONE row
 * of 576 values per token, shared by all H query heads (one latent head).  The key of a token is its whole row, its value the
 * first 512 values of the same row -- D_qk = 576, D_v = 512 --, and the kernel loads those bytes once for both.
 *
 *   q             : [B, H, S_q, 576] in `dtype`, 16-byte aligned.  q_strides: element strides {batch, head, row} (NULL =
 *                   contiguous), non-negative multiples of 8, the row stride at least 576.
 *   kv_pool       : [num_pages, page_size, 576] in `dtype`, 16-byte aligned, read -- and with kv_new written -- in place.
 *                   kv_strides: element strides {page, row} (NULL = contiguous), multiples of 8 (16-byte rows), the row
 *                   stride at least 576.  One page is addressed with 32-bit offsets; the page number goes into the 64-bit
 *                   base of the page, so num_pages * page stride may exceed 2^32 bytes.
 *   block_table   : int32 DEVICE tensor [B, max_pages_per_seq], 4-byte aligned, rows block_table_stride (>= max_pages_per_seq)
 *                   elements apart.  Key j of sequence b lives in page block_table[b][j / page_size], row j % page_size.
 *                   Entries at index >= ceil(L_b / page_size) are never read.  An entry outside [0, num_pages) below that index
 *                   makes the sequence's result unspecified, but no access leaves the pool: its keys read as an empty page and
 *                   an appended row that would land there is dropped.
 *   page_size     : a positive multiple of 32 (MI355FA_ERR_PAGED otherwise).
 *   cache_seqlens : int32 DEVICE vector [B], 4-byte aligned.  L_b = cache_seqlens[b] + S_new, clamped to
 *                   [0, max_pages_per_seq * page_size].  The host reads neither cache_seqlens nor block_table: a step can be
 *                   captured in a hipGraph and replayed while both change in place.  cache_seqlens is not modified.
 *   kv_new        : [B, S_new, 576] in `dtype`, contiguous, 16-byte aligned, or NULL with S_new = 0.  Written to the rows
 *                   cache_seqlens[b] + j through the table (they may cross page boundaries) before attention.  Rows at or past
 *                   max_pages_per_seq * page_size are dropped.
 *   o             : [B, H, S_q, 512] in `dtype`, 16-byte aligned.  o_strides: element strides {batch, head, row} (NULL =
 *                   contiguous), multiples of 8, the row stride at least 512, no zero batch / head stride.
 *   lse           : NULL or fp32 [B, H, S_q], natural-log units.
 *   causal        : 0 or 1; the only mask.  Query i of sequence b sits at position L_b - S_q + i (bottom-right aligned, as
 *                   every decode call here) and with causal = 1 sees the keys at or below its position.  A row with no visible
 *                   key gets O = 0 and LSE = -inf.
 *   scale         : finite and > 0.  DeepSeek passes (128 + 64) ** -0.5 times its mscale, not 576 ** -0.5.
 *
 * The launch has n splits of the key range, n a function of the arguments of fa_fwd_kvcache_mla_workspace_bytes alone; that
 * function returns n > 1 ? n * B * H * S_q * (512 + 2) * 4 : 0, the bytes of the 16-byte aligned workspace the call needs.
 * Every order of summation is fixed: the result is deterministic.  Every argument error is reported before anything is
 * enqueued, with a text (fa_last_error) that names the argument and carries the offending value.
 */
#ifndef MI355FA_KVCACHE_MLA_H_
#define MI355FA_KVCACHE_MLA_H_
#include "../include/mi355fa_paged.h"
#ifdef __cplusplus
extern "C" {
#endif
#define MI355FA_MLA_D 576   /* a query head and a cached row */
#define MI355FA_MLA_DV 512  /* a value and a row of the result */
long long fa_fwd_kvcache_mla_workspace_bytes(int B, int H, int S_q, int max_pages_per_seq, int page_size, int S_new);
int fa_fwd_kvcache_mla(const void* q, void* kv_pool, const void* kv_new, const int* cache_seqlens, const int* block_table,
                       void* o, float* lse, void* workspace, long long workspace_bytes, int B, int H, int S_q, int num_pages,
                       int page_size, int max_pages_per_seq, long long block_table_stride, int S_new, int dtype, float scale,
                       int causal, const long long* q_strides, const long long* kv_strides, const long long* o_strides,
                       void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_KVCACHE_MLA_H_ */
