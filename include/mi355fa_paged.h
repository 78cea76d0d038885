/* mi355fa_paged.h -- decoding attention over a PAGED KV cache (a pool of fixed-size pages and a per-sequence table of page
 * numbers: vLLM / SGLang block tables, FlashAttention's flash_attn_with_kvcache(block_table=...)) in libmi355fa.so.
 *
 * A companion to mi355fa_kvcache.h, mi355fa_kvcache_fp8.h, mi355fa_softcap.h, mi355fa_alibi.h and mi355fa_sink.h (included
 * below for the decoding conventions and the score transforms; mi355fa.h, its ABI version and every other header's
 * function list are unchanged).  Inference only: there is no backward.
 *
 *   k_pool / v_pool: [num_pages, H_kv, page_size, D], 16-bit (`dtype`) or OCP e4m3 bytes (cache_dtype), 16-byte aligned.
 *                   opts->k_strides / v_strides are the element strides {page, head, row} (NULL = contiguous); K and V share
 *                   their row stride.  A [num_pages, page_size, H_kv, D] pool is read in place through them.  One
 *                   (page, head) slice is addressed with 32-bit offsets; the page number goes into the 64-bit base of the
 *                   slice, so num_pages * page stride may exceed 2^32 bytes.
 *   block_table   : int32 DEVICE tensor [B, max_pages_per_seq], 4-byte aligned, rows block_table_stride (>= max_pages_per_seq)
 *                   elements apart.  Key j of sequence b lives in page block_table[b][j / page_size], row j % page_size.
 *                   Entries at index >= ceil(L_b / page_size) are never read.  An entry outside [0, num_pages) below that
 *                   index makes the sequence's result unspecified, but no access leaves the pool: its keys read as an
 *                   empty page and an appended row that would land there is dropped.
 *   page_size     : a positive multiple of 32 (MI355FA_ERR_PAGED otherwise).
 *   cache_seqlens : as in mi355fa_kvcache.h.  L_b = cache_seqlens[b] + S_new, clamped to [0, max_pages_per_seq * page_size].
 *                   The host reads neither cache_seqlens nor block_table: a step can be captured in a hipGraph and replayed
 *                   while both change in place.
 *   k_new / v_new : [B, H_kv, S_new, D] in `dtype`, contiguous, or both NULL.  Written to the rows cache_seqlens[b] + j
 *                   through the table (they may cross page boundaries) before attention; an fp8 pool quantises them as
 *                   fa_fwd_kvcache_fp8 does.  Rows at or past max_pages_per_seq * page_size are dropped.
 *   cache_dtype   : MI355FA_PAGED_CACHE_16BIT (the pools hold `dtype`) or MI355FA_PAGED_CACHE_FP8_E4M3.
 *   mods          : NULL or all members zero = plain attention.  At most one of softcap (> 0, finite: mi355fa_softcap.h),
 *                   alibi_slopes (+ slopes_batch_stride: mi355fa_alibi.h) and sinks (mi355fa_sink.h); an fp8 pool takes
 *                   sinks only.  k_descale / v_descale (+ descale_bstride: mi355fa_kvcache_fp8.h) belong to an fp8 pool and
 *                   are refused with a 16-bit one.  A combination outside these is refused with MI355FA_ERR_PAGED; each
 *                   member is otherwise checked as its own header says.
 *
 * The masks (bottom-right aligned), rows with no visible key (O = 0, LSE = -inf), the split count n and the workspace
 * follow mi355fa_kvcache.h / mi355fa_kvcache_fp8.h with S_cache = max_pages_per_seq * page_size:
 * fa_fwd_kvcache_paged_workspace_bytes returns what fa_fwd_kvcache[_fp8]_workspace_bytes returns for that S_cache, and the
 * result has the bits of the padded call on the gathered cache.  Every argument error is reported before anything is
 * enqueued.
 */
#ifndef MI355FA_PAGED_H_
#define MI355FA_PAGED_H_
#include "mi355fa_kvcache.h"
#include "mi355fa_kvcache_fp8.h"
#include "mi355fa_softcap.h"
#include "mi355fa_alibi.h"
#include "mi355fa_sink.h"
#ifdef __cplusplus
extern "C" {
#endif
#define MI355FA_ERR_PAGED (-12) /* page_size, num_pages, max_pages_per_seq, block_table_stride or a mods combination */
#define MI355FA_PAGED_CACHE_16BIT 0    /* cache_dtype: the pools hold `dtype` (fp16 / bf16) */
#define MI355FA_PAGED_CACHE_FP8_E4M3 1 /* cache_dtype: OCP float8 e4m3 bytes (torch.float8_e4m3fn) */
typedef struct mi355fa_paged_mods {
  float softcap;                 /* > 0: the soft cap; 0 = none */
  const float* alibi_slopes;     /* fp32 device slopes; NULL = none */
  long long slopes_batch_stride; /* 0: shape (H,); >= H: shape (B, H) */
  const float* sinks;            /* fp32 device vector (H,); NULL = none */
  const float* k_descale;        /* fp8 pools: fp32 device factors, NULL = 1.0 */
  const float* v_descale;
  long long descale_bstride;     /* 0: shape (H_kv,); >= H_kv: shape (B, H_kv) */
} mi355fa_paged_mods;
/* Head dims: D = 64, 128 or 256, as for the padded decode calls, in every variant. */
long long fa_fwd_kvcache_paged_workspace_bytes(int B, int H, int H_kv, int S_q, int max_pages_per_seq, int page_size,
                                               int S_new, int D, int cache_dtype);
int fa_fwd_kvcache_paged(const void* q, void* k_pool, void* v_pool, const void* k_new, const void* v_new,
                         const int* cache_seqlens, const int* block_table, void* o, float* lse, void* workspace,
                         long long workspace_bytes, int B, int H, int H_kv, int S_q, int num_pages, int page_size,
                         int max_pages_per_seq, long long block_table_stride, int S_new, int D, int dtype, int cache_dtype,
                         float scale, int window_left, int window_right, const mi355fa_paged_mods* mods,
                         const mi355fa_opts* opts, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_PAGED_H_ */
