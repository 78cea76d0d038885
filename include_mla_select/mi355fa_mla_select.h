/* mi355fa_mla_select.h -- top-k selection from the indexer's logits in libmi355fa.so: the step between
 * fa_mla_indexer_logits_fp8 and the `indices` of fa_fwd_kvcache_mla_sparse / fa_fwd_kvcache_mla_sparse_fp8.  Per row (b, i) of
 * logits the best min(topk, #candidates) columns, in ASCENDING column order, then -1 to the end.  A companion to
 * mi355fa_mla_indexer.h (mi355fa_paged.h is included below for the error codes; mi355fa.h, its ABI version and every other
 * header's function list are unchanged).  The header lives in include_mla_select/, as the listings of the other include
 * directories are recorded sets.  Inference only.
 *
 *   logits         : fp32 [B, S_q, W], read in place, 4-byte aligned -- rows need no more: the kernel peels to its 16-byte loads
 *                    itself.  W in [1, 2^30].
 *   lengths        : int32 DEVICE array [B] or NULL.  Columns at or past clamp(lengths[b], 0, W) are not read and count as
 *                    hidden; NULL: every row is W long.  The host never reads it.  Pass the L_b of the logits call.
 *   indices        : int32 [B, S_q, topk], 4-byte aligned.  Every one of a row's topk entries is written.
 *   topk           : in [1, 65536].
 *   logits_strides : element strides {batch, row} of logits (NULL = contiguous), non-negative, row stride >= W.
 *   indices_strides: element strides {batch, row} of indices (NULL = contiguous), non-negative, row stride >= topk.
 *
 * The contract.  A column is a CANDIDATE when it is below the row's length and its value is neither -inf nor NaN.  Candidates are
 * ordered by value descending, -0.0 == +0.0, ties by lower column first; +inf is an ordinary largest value.  The row's result
 * is the first min(topk, #candidates) columns of that order, written in ascending column order, then -1.  The result is exact
 * and unique, and the same input gives the same bits on every launch.
 *
 * No workspace.  One workgroup owns one row and never waits for another.  Rows of W <= 32768 are held in LDS and read from memory
 * once; wider rows are re-read (from L2) once per pass.  Every argument error is reported before anything is enqueued, with a
 * text (fa_last_error) that names the argument and carries the offending value.
 */
#ifndef MI355FA_MLA_SELECT_H_
#define MI355FA_MLA_SELECT_H_
#include "../include/mi355fa_paged.h"
#ifdef __cplusplus
extern "C" {
#endif
int fa_mla_indexer_select(const float* logits, const int* lengths, int* indices, int B, int S_q, int W, int topk,
                          const long long* logits_strides, const long long* indices_strides, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_MLA_SELECT_H_ */
