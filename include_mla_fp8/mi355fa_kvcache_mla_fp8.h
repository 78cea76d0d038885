/* mi355fa_kvcache_mla_fp8.h -- MLA (multi-head latent attention) decoding over a paged FP8 latent cache in libmi355fa.so: the
 * call of mi355fa_kvcache_mla.h over a cache of 656-byte rows, e4m3 latent bytes with one fp32 scale per 128 latent dims and the
 * RoPE part kept in 16 bits (the row of FlashMLA's FP8 cache and of vLLM's "fp8_ds_mla").
 *
 * A companion to mi355fa_kvcache_mla.h (included below for MI355FA_MLA_D / MI355FA_MLA_DV, the decoding conventions and the
 * error codes; mi355fa.h, its ABI version and every other header's function list are unchanged).  The header lives in
 * include_mla_fp8/, beside the other include directories, whose listings are recorded sets.  Inference only.
 *
 * A cached row, every piece at a multiple of 16 bytes:
 *     bytes [0, 512)    512 OCP e4m3 bytes (S.EEEE.MMM, bias 7, no infinities, 0x7F / 0xFF = NaN): the latent dims
 *     bytes [512, 528)  4 fp32 scales, little endian; scale j belongs to the latent dims [128 j, 128 j + 128)
 *     bytes [528, 656)  the 64 RoPE values in `dtype` (fp16 or bf16), not quantised
 * The key of a token is float(byte) * scale on its 512 latent dims followed by its 64 RoPE values; its value is the latent part
 * alone -- D_qk = 576, D_v = 512.  A scale that is not a finite normal number > 0 and a NaN byte give unspecified results.
 *
 *   q             : [B, H, S_q, 576] in `dtype`, 16-byte aligned.  q_strides: element strides {batch, head, row} (NULL =
 *                   contiguous), non-negative multiples of 8, the row stride at least 576.
 *   kv_pool       : bytes [num_pages, page_size, 656], 16-byte aligned, read -- and with kv_new written -- in place.
 *                   kv_strides: BYTE strides {page, row} (NULL = contiguous), multiples of 16, the row stride at least 656.  One
 *                   page is addressed with 32-bit offsets; the page number goes into the 64-bit base of the page, so
 *                   num_pages * page stride may exceed 2^32 bytes.
 *   block_table, page_size, cache_seqlens, o, lse, causal, scale: as in mi355fa_kvcache_mla.h, word for word.  The host reads
 *                   neither cache_seqlens nor block_table: a step can be captured in a hipGraph and replayed while both
 *                   change in place.
 *   kv_new        : [B, S_new, 576] in `dtype`, contiguous, 16-byte aligned, or NULL with S_new = 0: UNQUANTISED rows, which
 *                   the call quantises on the device into the rows cache_seqlens[b] + j through the table (they may cross page
 *                   boundaries) before attention.  Per 128-dim block: amax = max |float(x)|; s = amax / 448 in fp32 (the
 *                   correctly rounded division), and 1.0 where that is not a normal fp32 number (an all-zero block, a subnormal
 *                   quotient); byte = e4m3_rne(clamp(float(x) / s, -448, 448)), -0.0 kept; s is stored as it is.  The RoPE
 *                   values are copied bit for bit.  Rows at or past max_pages_per_seq * page_size, and rows whose table entry
 *                   is outside the pool, are dropped.  Two rows of one call that land on the same cache row: unspecified.
 *
 * The launch has n splits of the key range, n a function of the arguments of fa_fwd_kvcache_mla_fp8_workspace_bytes alone (the
 * rule of fa_fwd_kvcache_mla); that function returns n > 1 ? n * B * H * S_q * (512 + 2) * 4 : 0, the bytes of the 16-byte
 * aligned workspace the call needs.  Every order of summation is fixed: the result is deterministic.  Every argument error is
 * reported before anything is enqueued, with a text (fa_last_error) that names the argument and carries the offending value.
 */
#ifndef MI355FA_KVCACHE_MLA_FP8_H_
#define MI355FA_KVCACHE_MLA_FP8_H_
#include "../include_mla/mi355fa_kvcache_mla.h"
#ifdef __cplusplus
extern "C" {
#endif
#define MI355FA_MLA_FP8_ROW_BYTES 656   /* a cached row */
#define MI355FA_MLA_FP8_SCALE_OFFSET 512 /* its four fp32 scales */
#define MI355FA_MLA_FP8_ROPE_OFFSET 528  /* its 64 RoPE values */
long long fa_fwd_kvcache_mla_fp8_workspace_bytes(int B, int H, int S_q, int max_pages_per_seq, int page_size, int S_new);
int fa_fwd_kvcache_mla_fp8(const void* q, void* kv_pool, const void* kv_new, const int* cache_seqlens, const int* block_table,
                           void* o, float* lse, void* workspace, long long workspace_bytes, int B, int H, int S_q, int num_pages,
                           int page_size, int max_pages_per_seq, long long block_table_stride, int S_new, int dtype, float scale,
                           int causal, const long long* q_strides, const long long* kv_strides, const long long* o_strides,
                           void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_KVCACHE_MLA_FP8_H_ */
