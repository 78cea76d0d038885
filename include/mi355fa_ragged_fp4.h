/* mi355fa_ragged_fp4.h -- decoding attention with PACKED VARIABLE-LENGTH QUERIES over paged MXFP4 pools in libmi355fa.so:
 * the continuous-batching step of mi355fa_ragged.h over the cache format of mi355fa_kvcache_fp4.h.
 *
 * A companion to both (included below; mi355fa.h, its ABI version and every other header's function list are unchanged).
 * The conventions are the union of the two parents', and nothing here restates what they define:
 *
 *   from mi355fa_ragged.h       packed q / o [total_q, H, D] with opts->q_strides / o_strides, cu_seqlens_q, lse [H, total_q],
 *                               k_new / v_new [total_q, H_kv, D], positions (bottom-right aligned per sequence), the padding
 *                               rows at or past cu[B] (never read, never written), the clamping of a malformed
 *                               cu_seqlens_q, the device-built list of row blocks with NB_max = (g * total_q + 31 * B) / 32,
 *                               and MI355FA_ERR_RAGGED.
 *   from mi355fa_kvcache_fp4.h  the format (e2m1 nibbles, e8m0 block scales, no per-tensor factor), the quantiser of the
 *                               append, kv_dtype, the pools [num_pages, H_kv, page_size, D / 2] and scale pools
 *                               [num_pages, H_kv, page_size, D / 32] with their byte strides and alignments, sinks, and
 *                               the paged arguments as in mi355fa_paged.h.
 *
 *   D             : 64, 128 or 256; every other head dim is refused with MI355FA_ERR_SHAPE.  This is the one MXFP4 call
 *                   at D = 256: fa_fwd_kvcache_fp4 and fa_fwd_kvcache_fp4_paged keep refusing it.  A padded MXFP4 cache
 *                   [B, H_kv, S_cache, D / 2] with S_cache % 32 == 0 goes in here as a pool of B pages of S_cache keys whose
 *                   table is {0, 1, .., B - 1} with max_pages_per_seq = 1 (q [B, H, 1, D] is the packed q with
 *                   cu_seqlens_q = {0, 1, .., B}).  At D = 256 a scale row is 8 bytes, and the alignment rule of
 *                   mi355fa_kvcache_fp4.h (scales aligned to D / 32 bytes, strides multiples of it) is what the kernel's
 *                   4-byte loads of half a row rely on.
 *   k_new / v_new : packed row cu[b] + i is quantised into row cache_seqlens[b] + i of sequence b, nibbles and scale bytes,
 *                   through the table before attention; rows past the table, or whose entry is outside the pool, are
 *                   dropped; cache_seqlens is not modified.
 *   workspace     : roundup16(16 + 8 * NB_max) + (n > 1 ? n * H * total_q * (D + 2) * 4 : 0) bytes, never 0 -- the formula of
 *                   mi355fa_ragged.h.  n, the split count, is this path's own: the MXFP4 rule of mi355fa_kvcache_fp4.h (at
 *                   D = 256 with the D = 256 split length) over H_kv * NB_max workgroups per split and S_cache =
 *                   max_pages_per_seq * page_size.
 *
 * The rows of sequence b have the bits of fa_fwd_kvcache_fp4_paged on that sequence alone (B = 1, S_q = S_b) at the same n,
 * where that call exists (D = 64, 128).  The host reads none of cu_seqlens_q, cache_seqlens, block_table or the scales: a
 * step captured at a fixed total_q and B replays while they change in place.  Every argument error is reported before
 * anything is enqueued, with the parents' codes: MI355FA_ERR_RAGGED, _PAGED, _DTYPE, _SHAPE, _ALIGN, _STRIDE, _NULL.
 * There is no soft-cap or ALiBi argument: those stay without an MXFP4 form.
 */
#ifndef MI355FA_RAGGED_FP4_H_
#define MI355FA_RAGGED_FP4_H_
#include "mi355fa_ragged.h"
#include "mi355fa_kvcache_fp4.h"
#ifdef __cplusplus
extern "C" {
#endif
long long fa_fwd_kvcache_fp4_ragged_workspace_bytes(int total_q, int B, int H, int H_kv, int max_pages_per_seq, int page_size,
                                                    int D);
int fa_fwd_kvcache_fp4_ragged(const void* q, void* k_pool, void* v_pool, void* k_scale, void* v_scale, const void* k_new,
                              const void* v_new, const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table,
                              const long long* k_scale_strides, const long long* v_scale_strides, const float* sinks, void* o,
                              float* lse, void* workspace, long long workspace_bytes, int total_q, int B, int H, int H_kv,
                              int num_pages, int page_size, int max_pages_per_seq, long long block_table_stride, int D,
                              int dtype, int kv_dtype, float scale, int window_left, int window_right,
                              const mi355fa_opts* opts, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_RAGGED_FP4_H_ */
