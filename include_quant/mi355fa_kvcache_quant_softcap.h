/* mi355fa_kvcache_quant_softcap.h -- decoding attention with LOGIT SOFT-CAPPING over the three quantised KV-cache formats:
 * per-tensor e4m3, per-token-scaled e4m3 and MXFP4; padded, paged, and with packed variable-length queries, in libmi355fa.so.
 *
 * A companion to mi355fa_softcap.h (the transform), mi355fa_kvcache_fp8.h, mi355fa_kvcache_fp8_token.h, mi355fa_kvcache_fp4.h and
 * mi355fa_ragged_fp4.h (the formats, their quantisers and their appends), mi355fa_paged.h and mi355fa_ragged.h (the geometries),
 * all included below; mi355fa.h, its ABI version and every other header's function list are unchanged.  Inference only.
 * The header lives in include_quant/, beside include/ -- whose listing is a recorded set -- and includes its parents as
 * "../include/<name>": add no include path for it, or only the repository's root.
 *
 * Why: the models that cap their logits (Gemma 2: cap 50, D = 256, alternating sliding windows; Grok-1) could decode over a
 * 16-bit cache only.  These calls give them the quantised caches: half or a quarter of the bytes per cached key.
 *
 * The transform: every score s = q . dequantised(k) becomes softcap * tanh(scale * s / softcap) before the masks, as in
 * mi355fa_softcap.h.  "Dequantised" per format:
 *   MI355FA_QUANT_E4M3        s = (q . bytes) * k_descale[b, hk]: the descale belongs to the score, so it goes UNDER the tanh
 *                             with the scale, tanh(scale * k_descale * (q . bytes) / softcap).  v_descale multiplies the result
 *                             row as without the cap.  NULL descales are 1.0.
 *   MI355FA_QUANT_E4M3_TOKEN  s = (q . bytes) * k_scale[b, hk, j]: the key's scale multiplies its fp32 score in front of the
 *                             transform.  V's scale is split as in mi355fa_kvcache_fp8_token.h ("Exactness"): its power of two
 *                             through the conversion, its mantissa on the fp32 probability behind the exponential -- the cap
 *                             does not touch it.  With every scale 1.0 the result has the bits of MI355FA_QUANT_E4M3 with NULL
 *                             descales at the same split count.
 *   MI355FA_QUANT_MXFP4       the block scale goes through the conversion: the matrix product is the dequantised score.
 * The quantised bytes reach the matrix product without rounding in all three, so the error of a call is the 16-bit soft-capped
 * call's on the dequantised cache.  At most one transform: there are no sinks and no ALiBi slopes here.
 *
 * The cache of a call is one struct:
 *   format           MI355FA_QUANT_E4M3, _E4M3_TOKEN or _MXFP4; anything else is refused with MI355FA_ERR_DTYPE.
 *   k_descale, v_descale, descale_bstride
 *                    E4M3 only, as in mi355fa_kvcache_fp8.h: fp32 DEVICE factors at [b * descale_bstride + hk], NULL = 1.0,
 *                    4-byte aligned; descale_bstride 0 (shape (H_kv,)) or >= H_kv.  With another format all three must be
 *                    NULL / 0 (MI355FA_ERR_SHAPE).
 *   k_scale, v_scale E4M3_TOKEN: float* row scales [.., H_kv, rows]; MXFP4: e8m0 bytes [.., H_kv, rows, D / 32].  Not NULL for
 *                    these two formats (MI355FA_ERR_NULL); with E4M3 they and the strides must be NULL (MI355FA_ERR_SHAPE).
 *                    The append of k_new / v_new writes them.
 *   k_scale_strides, v_scale_strides
 *                    {batch-or-page, head, row} as in the format's own header (E4M3_TOKEN: ELEMENT strides, any non-negative
 *                    ones; MXFP4: byte strides, multiples of D / 32); NULL = contiguous.
 * The caches themselves (k_cache / v_cache or the pools, opts->k_strides / v_strides), k_new / v_new and their append, q, o,
 * lse, cache_seqlens, block_table, cu_seqlens_q, the windows and the workspace are those of the format's own padded, paged or
 * packed call, checked by the same code and refused with the same codes and texts under this header's function names.
 *
 *   softcap       : finite and > 0 (MI355FA_ERR_SOFTCAP otherwise), after `scale` as in fa_fwd_kvcache_softcap.
 *   D             : E4M3: 64, 128 or 256 in every geometry.  E4M3_TOKEN and MXFP4: 64 or 128, and 256 on the packed call
 *                   alone; D = 256 on their two rectangular calls is refused with MI355FA_ERR_SHAPE, every other head dim
 *                   with MI355FA_ERR_HEAD_DIM -- what the plain calls of each format take.
 *   The order of the checks: the struct (NULL: MI355FA_ERR_NULL), its format, the members of another format, missing scale
 *   tensors, D = 256 on a rectangular call; packed: cu_seqlens_q, total_q and B; softcap; paged: the block table, the page
 *   geometry, the table's stride; then everything the decode calls share, in their order.  Every argument error is reported
 *   before anything is enqueued.
 *
 * The workspace functions return what the plain call of that format and geometry returns: n * B * H * S_q * (D + 2) * 4 bytes
 * (0 when n = 1), packed roundup16(16 + 8 * NB_max) + (n > 1 ? n * H * total_q * (D + 2) * 4 : 0), with the split count n of
 * the format's own rule.  The host reads none of cache_seqlens, block_table, cu_seqlens_q, the descales or the scales, so a
 * captured step replays while all of them change.  The masks, rows with no visible key (O = 0, LSE = -inf) and determinism are
 * the parents'.  The paged call has the bits of the padded call on the gathered cache (and scales), and the rows of a sequence
 * in the packed call the bits of the paged call on that sequence alone (D = 64, 128).
 */
#ifndef MI355FA_KVCACHE_QUANT_SOFTCAP_H_
#define MI355FA_KVCACHE_QUANT_SOFTCAP_H_
#include "../include/mi355fa_softcap.h"
#include "../include/mi355fa_kvcache_fp8.h"
#include "../include/mi355fa_kvcache_fp8_token.h"
#include "../include/mi355fa_kvcache_fp4.h"
#include "../include/mi355fa_ragged_fp4.h"
#include "../include/mi355fa_paged.h"
#include "../include/mi355fa_ragged.h"
#ifdef __cplusplus
extern "C" {
#endif
#define MI355FA_QUANT_E4M3 0       /* mi355fa_kvcache_fp8.h: bytes + k_descale / v_descale */
#define MI355FA_QUANT_E4M3_TOKEN 1 /* mi355fa_kvcache_fp8_token.h: bytes + fp32 row scales */
#define MI355FA_QUANT_MXFP4 2      /* mi355fa_kvcache_fp4.h: nibbles + e8m0 block scales */
typedef struct mi355fa_quant_cache {
  int format;
  const float *k_descale, *v_descale; /* E4M3 only; NULL = 1.0 */
  long long descale_bstride;
  void *k_scale, *v_scale; /* E4M3_TOKEN: float*, MXFP4: bytes; the append writes them */
  const long long *k_scale_strides, *v_scale_strides; /* as in the format's own header; NULL = contiguous */
} mi355fa_quant_cache;
long long fa_fwd_kvcache_quant_softcap_workspace_bytes(int format, int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D);
int fa_fwd_kvcache_quant_softcap(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                                 const int* cache_seqlens, void* o, float* lse, void* workspace, long long workspace_bytes, int B,
                                 int H, int H_kv, int S_q, int S_cache, int S_new, int D, int dtype, float scale, float softcap,
                                 int window_left, int window_right, const mi355fa_quant_cache* cache, const mi355fa_opts* opts,
                                 void* stream);
long long fa_fwd_kvcache_quant_softcap_paged_workspace_bytes(int format, int B, int H, int H_kv, int S_q, int max_pages_per_seq,
                                                             int page_size, int S_new, int D);
int fa_fwd_kvcache_quant_softcap_paged(const void* q, void* k_pool, void* v_pool, const void* k_new, const void* v_new,
                                       const int* cache_seqlens, const int* block_table, void* o, float* lse, void* workspace,
                                       long long workspace_bytes, int B, int H, int H_kv, int S_q, int num_pages, int page_size,
                                       int max_pages_per_seq, long long block_table_stride, int S_new, int D, int dtype,
                                       float scale, float softcap, int window_left, int window_right,
                                       const mi355fa_quant_cache* cache, const mi355fa_opts* opts, void* stream);
long long fa_fwd_kvcache_quant_softcap_ragged_workspace_bytes(int format, int total_q, int B, int H, int H_kv,
                                                              int max_pages_per_seq, int page_size, int D);
int fa_fwd_kvcache_quant_softcap_ragged(const void* q, void* k_pool, void* v_pool, const void* k_new, const void* v_new,
                                        const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table, void* o,
                                        float* lse, void* workspace, long long workspace_bytes, int total_q, int B, int H,
                                        int H_kv, int num_pages, int page_size, int max_pages_per_seq,
                                        long long block_table_stride, int D, int dtype, float scale, float softcap,
                                        int window_left, int window_right, const mi355fa_quant_cache* cache,
                                        const mi355fa_opts* opts, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_KVCACHE_QUANT_SOFTCAP_H_ */
