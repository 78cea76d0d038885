/* mi355fa_mla_indexer.h -- the DeepSeek-V3.2 "lightning indexer" logits over a paged FP8 key cache in libmi355fa.so: for every
 * query token a score of every cached token,
 *
 *     logits[b, i, t] = k_scale[t] * sum_h weights[b, i, h] * max(0, sum_d q[b, i, h, d] * k[t, d]),
 *
 * the row torch.topk turns into the `indices` of fa_fwd_kvcache_mla_sparse / fa_fwd_kvcache_mla_sparse_fp8.  A companion to
 * mi355fa_paged.h (included below for the error codes and the words cache_seqlens / block_table; mi355fa.h, its ABI version and
 * every other header's function list are unchanged).  The header lives in include_mla_indexer/, as the listings of the other
 * include directories are recorded sets.  Inference only.
 *
 *   q              : e4m3 bytes [B, S_q, H_i, 128], 16-byte aligned, the 128 dims contiguous.  H_i in {16, 32, 48, 64}.
 *   weights        : fp32 [B, S_q, H_i].  The caller folds q's dequantisation scale, H_i ** -0.5 and the softmax scale into it.
 *                    ReLU comes before the weights, which may have either sign.
 *   k_cache        : e4m3 bytes [num_pages, page_size, 128], 16-byte aligned; page_size a positive multiple of 32.  Read and (with
 *                    k_new) appended to in place.  The pool may exceed 4 GiB.
 *   k_scale        : fp32 [num_pages, page_size], one scale per cached key.
 *   k_new          : fp16 / bf16 (dtype) contiguous [B, S_new, 128] with S_new == S_q, 16-byte aligned, or NULL with S_new == 0.
 *                    Row i of sequence b is quantised -- s = amax / 448, 1.0 where that is not a normal fp32 number, the byte
 *                    e4m3_rne(clamp(x / s, -448, 448)) -- into logical position cache_seqlens[b] + i through block_table, bytes
 *                    and scale, before the logits are formed.  A position outside the table's reach or a table entry outside
 *                    [0, num_pages) drops the row.  cache_seqlens is not modified.
 *   cache_seqlens, block_table : int32 DEVICE arrays as in fa_fwd_kvcache_paged; the host reads neither.  L_b = cache_seqlens[b] +
 *                    S_new, clamped to [0, max_pages_per_seq * page_size].  Table entries at or past ceil(L_b / page_size) and
 *                    rows and scales at or past L_b are never read.  An entry outside [0, num_pages) makes that page's logits
 *                    unspecified; no access leaves the pools.
 *   logits         : fp32 [B, S_q, W], 4-byte aligned.  Column t is VISIBLE when t < L_b and, with causal = 1, t <= L_b - S_q + i.
 *                    Every other column of [0, W) is written as -inf, exactly.
 *   q_strides      : BYTE strides {batch, row, head} of q (NULL = contiguous), non-negative multiples of 16, head stride >= 128.
 *   weights_strides: element strides {batch, row, head} of weights (NULL = contiguous), non-negative.
 *   k_strides      : BYTE strides {page, row} of k_cache (NULL = contiguous), multiples of 16, row stride >= 128.
 *   k_scale_strides: element strides {page, row} of k_scale (NULL = contiguous), non-negative.  Two views of one buffer with a page
 *                    stride of page_size * 132 bytes are the "all bytes of a block, then its scales" layout.
 *   logits_strides : element strides {batch, row} of logits (NULL = contiguous), row stride >= W.
 *
 * No workspace, no split and no combine: one workgroup owns a run of columns of one sequence, so every order of summation is
 * fixed and the result is deterministic.  Every argument error is reported before anything is enqueued, with a text
 * (fa_last_error) that names the argument and carries the offending value.
 */
#ifndef MI355FA_MLA_INDEXER_H_
#define MI355FA_MLA_INDEXER_H_
#include "../include/mi355fa_paged.h"
#ifdef __cplusplus
extern "C" {
#endif
int fa_mla_indexer_logits_fp8(const void* q, const float* weights, void* k_cache, float* k_scale, const void* k_new,
                              const int* cache_seqlens, const int* block_table, float* logits, int B, int S_q, int H_i, int W,
                              int num_pages, int page_size, int max_pages_per_seq, long long block_table_stride, int S_new,
                              int dtype, int causal, const long long* q_strides, const long long* weights_strides,
                              const long long* k_strides, const long long* k_scale_strides, const long long* logits_strides,
                              void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_MLA_INDEXER_H_ */
