/* mi355fa_mla_sparse_prefill.h -- sparse (top-k indexed) MLA attention of a PREFILL step in libmi355fa.so: packed absorbed
 * queries over the rows of ONE contiguous latent array that per-token index lists name,
 *
 *     O[m, h, :] = softmax_j(scale * q[m, h, :] . kv[idx[m, j], :]) @ kv[idx[m, j], :512]     over the visible j of row m,
 *
 * where entry j of row m is visible iff 0 <= indices[m, j] < N.  Every other value -- -1 padding, anything negative, anything
 * at or past N -- is skipped and causes no access at all; a duplicate counts as often as it appears.  There is no causal flag:
 * the indexer's ranges (fa_mla_indexer_logits_fp8_prefill, mi355fa_mla_indexer_prefill.h) already decided what a row may see,
 * and fa_mla_indexer_select (mi355fa_mla_select.h) on its logits returns exactly these lists.  The decode-step form over a paged
 * cache is fa_fwd_kvcache_mla_sparse (mi355fa_kvcache_mla_sparse.h).  mi355fa_paged.h is included below for the error codes;
 * mi355fa.h, its ABI version and every other header's function list are unchanged.  The header lives in
 * include_mla_sparse_prefill/, as the listings of the other include directories are recorded sets.  Inference only.
 *
 *   q        : fp16 / bf16 [M, H, 576], 16-byte aligned: dims [0, 512) the absorbed no-RoPE part, [512, 576) the RoPE part.
 *              M in [1, 2^22], H in [1, 1024].
 *   kv       : the same dtype [N, 576], 16-byte aligned, read in place with 64-bit addresses; it may exceed 4 GiB.  N in
 *              [0, 2^31 - 1]; NULL only with N == 0.
 *   indices  : int32 DEVICE array [M, topk], 4-byte aligned; the host never reads it.  topk in [1, 2^24].
 *   o        : q's dtype [M, H, 512], 16-byte aligned.  A row with no visible entry gets zeros.
 *   lse      : fp32 [M, H] contiguous, natural log, -inf for a row with no visible entry; NULL: not written.
 *   dtype    : MI355FA_FP16 or MI355FA_BF16.  scale: finite and > 0.
 *   q_strides, o_strides : ELEMENT strides {row, head} (NULL = contiguous), non-negative multiples of 8; o's rows and heads are
 *              distinct memory (row stride >= 512, head stride >= 512 unless H == 1).
 *   kv_row_stride      : element stride of a row of kv, a multiple of 8 and at least 576.
 *   indices_row_stride : element stride of a row of indices, non-negative.
 *
 * No workspace, no split and no combine: one workgroup follows one list for 32 heads of its token from start to end, so every
 * order of summation is fixed -- list order -- and the result is deterministic.  Every argument error is reported before
 * anything is enqueued, with a text (fa_last_error) that names the argument and carries the offending value.
 */
#ifndef MI355FA_MLA_SPARSE_PREFILL_H_
#define MI355FA_MLA_SPARSE_PREFILL_H_
#include "../include/mi355fa_paged.h"
#ifdef __cplusplus
extern "C" {
#endif
int fa_fwd_mla_sparse_prefill(const void* q, const void* kv, const int* indices, void* o, float* lse, int M, int H, int N, int topk,
                              int dtype, float scale, const long long* q_strides, long long kv_row_stride, const long long* o_strides,
                              long long indices_row_stride, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_MLA_SPARSE_PREFILL_H_ */
