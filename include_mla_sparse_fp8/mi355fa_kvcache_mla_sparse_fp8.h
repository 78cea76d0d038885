/* mi355fa_kvcache_mla_sparse_fp8.h -- sparse (top-k indexed) MLA decoding over the paged FP8 latent cache in libmi355fa.so: the
 * decode step of DeepSeek-V3.2 as it is released, top-k indexed attention over 656-byte rows (e4m3 latent bytes with one fp32
 * scale per 128 latent dims and the RoPE part kept in 16 bits).
 *
 * A companion to mi355fa_kvcache_mla_fp8.h (included below: the row format, the pool and its BYTE strides, kv_new and its
 * quantisation, the conventions and every argument but the three named here are that header's, word for word; mi355fa.h, its
 * ABI version and every other header's function list are unchanged).  The header lives in include_mla_sparse_fp8/, as the
 * listings of the other include directories are recorded sets.  Inference only.
 *
 *   indices         : int32 DEVICE tensor [B, S_q, topk], 4-byte aligned, the last dim contiguous.  Entry j of (b, i) is a
 *                     LOGICAL position of sequence b, not a pool row: the key lives in page block_table[b][idx / page_size], row
 *                     idx % page_size.  Query i of sequence b attends to exactly the entries with 0 <= idx < L_b and, with
 *                     causal = 1, idx <= L_b - S_q + i.  Every other entry is skipped: -1 padding, garbage, a position behind
 *                     the query.  An entry that appears twice counts twice; the order of the list does not change the
 *                     mathematical result.  A visible idx whose table entry is outside [0, num_pages) reads as skipped and
 *                     makes the sequence's result unspecified.  Whatever indices, block_table or cache_seqlens hold, no access
 *                     leaves the pool.  A row with no visible entry gets O = 0 and LSE = -inf.  The host does not read it: a
 *                     captured step replays while indices change in place.
 *   topk            : the length of a list, in [1, 2^24].
 *   indices_strides : element strides {batch, row} of indices (NULL = contiguous), non-negative.
 *
 * kv_new is quantised and appended before attention, so a list may name the rows being appended.  L_b = cache_seqlens[b] +
 * S_new, clamped as in the dense call.  Only the rows a list names are read: a scale or a byte of a row no visible entry names
 * may hold anything.
 *
 * The launch has n splits of the LIST (not of the cache), n a function of the arguments of
 * fa_fwd_kvcache_mla_sparse_fp8_workspace_bytes alone (the rule of fa_fwd_kvcache_mla_sparse); that function returns
 * n > 1 ? n * B * H * S_q * (512 + 2) * 4 : 0, the bytes of the 16-byte aligned workspace the call needs.  Every order of
 * summation is fixed: the result is deterministic.  Every argument error is reported before anything is enqueued, with a text
 * (fa_last_error) that names the argument and carries the offending value.
 */
#ifndef MI355FA_KVCACHE_MLA_SPARSE_FP8_H_
#define MI355FA_KVCACHE_MLA_SPARSE_FP8_H_
#include "../include_mla_fp8/mi355fa_kvcache_mla_fp8.h"
#ifdef __cplusplus
extern "C" {
#endif
long long fa_fwd_kvcache_mla_sparse_fp8_workspace_bytes(int B, int H, int S_q, int topk, int max_pages_per_seq, int page_size, int S_new);
int fa_fwd_kvcache_mla_sparse_fp8(const void* q, void* kv_pool, const void* kv_new, const int* indices, const int* cache_seqlens,
                                  const int* block_table, void* o, float* lse, void* workspace, long long workspace_bytes, int B,
                                  int H, int S_q, int topk, int num_pages, int page_size, int max_pages_per_seq,
                                  long long block_table_stride, int S_new, int dtype, float scale, int causal,
                                  const long long* q_strides, const long long* kv_strides, const long long* o_strides,
                                  const long long* indices_strides, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_KVCACHE_MLA_SPARSE_FP8_H_ */
