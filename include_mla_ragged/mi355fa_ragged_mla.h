/* mi355fa_ragged_mla.h -- MLA decoding over a paged latent cache with PACKED VARIABLE-LENGTH QUERIES in libmi355fa.so: one
 * call for a step of continuous batching, in which some sequences decode one token, some verify a draft of a few tokens and
 * some run a chunk of their prefill.
 *
 * A companion to include_mla/mi355fa_kvcache_mla.h (included below: the latent cache, its conventions and the error codes;
 * mi355fa.h, its ABI version and every other header's function list are unchanged).  The header lives in a directory of its
 * own, beside include/, include_quant/ and include_mla/, whose listings are recorded sets.  Inference only.
 *
 *   q             : [total_q, H, 576] in `dtype`, 16-byte aligned: the queries of all sequences packed along the first
 *                   dimension.  q_strides: element strides {row, head} (NULL = contiguous), non-negative multiples of 8, the
 *                   row stride at least 576, both below 2^30.
 *   cu_seqlens_q  : int32 DEVICE vector [B + 1], 4-byte aligned.  Sequence b owns the packed rows [cu[b], cu[b + 1]), S_b of
 *                   them (0 is allowed).  Each end is clamped into [0, total_q] and the second to the first: whatever the
 *                   vector holds, no access leaves q, o, lse, the workspace and the pool; sequences whose rows are not their
 *                   own (a descending, negative or too large entry) get unspecified results.  Rows at or past cu[B] are
 *                   padding -- the tail of a captured step: never read, and their rows of o and lse are never written.
 *   kv_pool, kv_strides, block_table, block_table_stride, page_size, num_pages, max_pages_per_seq
 *                 : as in fa_fwd_kvcache_mla.
 *   cache_seqlens : int32 DEVICE vector [B].  L_b = cache_seqlens[b] + (has_new ? S_b : 0), clamped to
 *                   [0, max_pages_per_seq * page_size].  The host reads none of cu_seqlens_q, cache_seqlens and block_table:
 *                   the launch is sized from total_q and B alone, and a step captured at a fixed total_q and B replays while
 *                   all three change in place.
 *   kv_new        : [total_q, 576] in `dtype`, contiguous, 16-byte aligned, with has_new = 1; NULL with has_new = 0.  Packed
 *                   row cu[b] + i is written to cache row cache_seqlens[b] + i of sequence b through the table before
 *                   attention.  Rows past the table, or whose table entry is outside the pool, are dropped.
 *   o             : [total_q, H, 512] in `dtype`, 16-byte aligned.  o_strides: element strides {row, head} (NULL =
 *                   contiguous), multiples of 8, the row stride at least 512, a non-zero head stride when H > 1.
 *   lse           : NULL or fp32 [H, total_q], natural-log units.
 *   causal, scale : as in fa_fwd_kvcache_mla.  Query i of sequence b sits at position L_b - S_b + i.  A row with no visible
 *                   key gets O = 0 and LSE = -inf.
 *   H * total_q and B are at most 2^24.
 *
 * workspace: 16-byte aligned, fa_fwd_kvcache_mla_ragged_workspace_bytes(...) bytes = the device-built list of the step's
 * 32-row blocks, (16 + 8 * nb_max) rounded up to 16 with nb_max = (H * total_q + 31 * B) / 32, followed by the partials of the
 * launch's n splits, n > 1 ? n * H * total_q * (512 + 2) * 4 : 0; n is a function of that function's arguments alone.  The
 * rows of sequence b have the bits of fa_fwd_kvcache_mla on that sequence alone (B = 1, S_q = S_b) at the same split count.
 * Every argument error is reported before anything is enqueued, with a text (fa_last_error) that names the argument and
 * carries the offending value.
 */
#ifndef MI355FA_RAGGED_MLA_H_
#define MI355FA_RAGGED_MLA_H_
#include "../include_mla/mi355fa_kvcache_mla.h"
#ifdef __cplusplus
extern "C" {
#endif
long long fa_fwd_kvcache_mla_ragged_workspace_bytes(int total_q, int B, int H, int max_pages_per_seq, int page_size);
int fa_fwd_kvcache_mla_ragged(const void* q, void* kv_pool, const void* kv_new, const int* cu_seqlens_q,
                              const int* cache_seqlens, const int* block_table, void* o, float* lse, void* workspace,
                              long long workspace_bytes, int total_q, int B, int H, int num_pages, int page_size,
                              int max_pages_per_seq, long long block_table_stride, int has_new, int dtype, float scale,
                              int causal, const long long* q_strides, const long long* kv_strides, const long long* o_strides,
                              void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_RAGGED_MLA_H_ */
