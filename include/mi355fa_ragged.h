/* mi355fa_ragged.h -- decoding attention over a paged KV cache with PACKED VARIABLE-LENGTH QUERIES in libmi355fa.so: one
 * call for a step of continuous batching, in which some sequences decode one token, some verify a draft of a few and some
 * run a chunk of their prefill (vLLM's flash_attn_varlen_func(..., cu_seqlens_q, seqused_k, block_table), FlashAttention's
 * flash_attn_with_kvcache(cu_seqlens_q=...)).
 *
 * A companion to mi355fa_paged.h (included below: the pools, the table, cache_seqlens, cache_dtype, mi355fa_paged_mods and
 * their refusals are exactly as there; mi355fa.h, its ABI version and every other header's function list are unchanged).
 * Inference only: there is no backward.
 *
 *   q, o          : [total_q, H, D] in `dtype`, 16-byte aligned.  opts->q_strides / o_strides are the element strides
 *                   {ignored, head, row} (NULL = contiguous: {0, D, H * D}); both multiples of 8 elements, row >= D, and
 *                   for o both non-zero.  A slice of a fused QKV projection is read in place.
 *   cu_seqlens_q  : int32 DEVICE tensor [B + 1], 4-byte aligned.  Sequence b owns the packed rows [cu[b], cu[b + 1]),
 *                   S_b of them (0 is allowed).  Rows at or past cu[B] are padding: never read, and never written in o /
 *                   lse.  The host does not read it (nor cache_seqlens nor block_table): a step captured at a fixed
 *                   total_q and B replays while all three change in place.  The kernels clamp both ends of a sequence
 *                   into [0, total_q] and the second to the first, so whatever it holds no access leaves q, o, lse, the
 *                   workspace or the pools; sequences whose rows are not their own (a non-monotone, negative or too
 *                   large entry, lengths beyond total_q) get unspecified results, and so does the append of a step whose
 *                   cu_seqlens_q does not ascend.
 *   positions     : query i of sequence b sits at L_b - S_b + i (bottom-right aligned), L_b = cache_seqlens[b] without
 *                   k_new, cache_seqlens[b] + S_b with it, clamped to [0, max_pages_per_seq * page_size].  A row with no
 *                   visible key (every row of a sequence with L_b < S_b at its negative positions, under a causal mask)
 *                   gets O = 0 and LSE = -inf.
 *   k_new / v_new : [total_q, H_kv, D] in `dtype`, contiguous, or both NULL.  Packed row cu[b] + i goes to cache row
 *                   cache_seqlens[b] + i of sequence b through the table, before attention; an fp8 pool quantises as
 *                   fa_fwd_kvcache_paged does.  Rows past the table are dropped; cache_seqlens is not modified.
 *   lse           : fp32 [H, total_q] (may be NULL).
 *   mods          : mi355fa_paged_mods; with shape (B, .) vectors the batch index is the sequence.
 *
 * The grid does not depend on the longest sequence.  With g = H / H_kv, a step has sum_b ceil(g * S_b / 32) blocks of 32
 * (query, head) rows, at most NB_max = (g * total_q + 31 * B) / 32 whatever the lengths; a one-workgroup kernel lists them
 * on the device, and the attention kernel runs NB_max * H_kv * n workgroups, of which those past the list's end leave at
 * once.  n, the split count, follows the rules of mi355fa_kvcache.h / mi355fa_kvcache_fp8.h with H_kv * NB_max workgroups
 * per split and S_cache = max_pages_per_seq * page_size.  The workspace holds the list and the splits' partials:
 *
 *   fa_fwd_kvcache_ragged_workspace_bytes = roundup16(16 + 8 * NB_max) + (n > 1 ? n * H * total_q * (D + 2) * 4 : 0)
 *
 * and is never 0.  The rows of sequence b have the bits of fa_fwd_kvcache_paged on that sequence alone (B = 1, S_q = S_b)
 * at the same n.  Every argument error is reported before anything is enqueued.
 */
#ifndef MI355FA_RAGGED_H_
#define MI355FA_RAGGED_H_
#include "mi355fa_paged.h"
#ifdef __cplusplus
extern "C" {
#endif
#define MI355FA_ERR_RAGGED (-13) /* total_q, B, or a stride of the packed q / o the kernels cannot address */
/* Head dims: D = 64, 128 or 256, as for the paged decode call, in every variant. */
long long fa_fwd_kvcache_ragged_workspace_bytes(int total_q, int B, int H, int H_kv, int max_pages_per_seq, int page_size,
                                                int D, int cache_dtype);
int fa_fwd_kvcache_ragged(const void* q, void* k_pool, void* v_pool, const void* k_new, const void* v_new,
                          const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table, void* o, float* lse,
                          void* workspace, long long workspace_bytes, int total_q, int B, int H, int H_kv, int num_pages,
                          int page_size, int max_pages_per_seq, long long block_table_stride, int D, int dtype,
                          int cache_dtype, float scale, int window_left, int window_right, const mi355fa_paged_mods* mods,
                          const mi355fa_opts* opts, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_RAGGED_H_ */
