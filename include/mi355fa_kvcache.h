/* mi355fa_kvcache.h -- decoding attention over a padded KV cache (split-KV, "flash-decoding") in libmi355fa.so.
 *
 * A companion to mi355fa_gqa.h (included below for its error codes and the window convention; mi355fa.h, its ABI version
 * and function list are unchanged).  Inference only: there is no backward.
 *
 *   q             : [B, H, S_q, D]          S_q >= 1 queries per sequence (1 for plain decoding)
 *   k_cache/v_cache: [B, H_kv, S_cache, D]  padded caches; H a positive multiple of H_kv, query head h reads K/V head
 *                                           h / (H / H_kv) as in fa_fwd_gqa
 *   cache_seqlens : int32 DEVICE vector [B]: the valid rows of each sequence's cache (0 allowed).  The host never reads
 *                   it, so a decode step can be captured in a hipGraph and replayed as the vector advances.
 *   k_new / v_new : [B, H_kv, S_new, D] contiguous, or both NULL (S_new = 0).  Written into cache rows
 *                   [cache_seqlens[b], cache_seqlens[b] + S_new) before attention, on the same stream; cache_seqlens
 *                   itself is not modified.
 *   o             : [B, H, S_q, D] in q's dtype;  lse: [B, H, S_q] fp32 contiguous, or NULL.
 *
 * Sequence b attends to L_b = cache_seqlens[b] + S_new keys; the caller guarantees L_b <= S_cache (otherwise that
 * sequence's result is unspecified, but no access leaves the cache tensors).  The mask is BOTTOM-RIGHT aligned: query i
 * sits at position p_i = L_b - S_q + i and key j is visible iff
 *     j < L_b  and  (window_left < 0 or j >= p_i - window_left)  and  (window_right < 0 or j <= p_i + window_right).
 * (-1, -1) is full attention over the cache, (-1, 0) causal; a value below -1 is refused (MI355FA_ERR_WINDOW).  A row with
 * no visible key gets O = 0 and LSE = -inf.  `scale` is the softmax scale (1/sqrt(D) for the usual one); it must be
 * finite and > 0, anything else is refused with MI355FA_ERR_SHAPE.
 *
 * The key range of each sequence is split over n workgroups per (sequence, K/V head); n follows from the shapes
 * (B, H_kv, S_cache, S_q, D), never from cache_seqlens.  With n > 1 the partial results go to `workspace` (device memory
 * the caller allocates, 16-byte aligned; its contents need no initialisation) and a second kernel merges them:
 *     workspace bytes = n * B * H * S_q * (D + 2) * 4   (0 when n = 1; workspace may then be NULL),
 * which fa_fwd_kvcache_workspace_bytes returns for the same shape arguments (a negative value is an argument error code).
 * Results are deterministic: the same inputs give the same bits at any n.
 *
 * `opts` (may be NULL) carries the strides of q, k_cache, v_cache and o as for the _ex functions (k / v: the cache
 * strides, e.g. a [B, S_cache, H_kv, D] cache seen as [B, H_kv, S_cache, D]; K and V share their sequence stride).
 * cu_seqlens, p_drop and q_scaled are refused (MI355FA_ERR_SHAPE).  Every argument error is reported before anything is
 * enqueued; everything else -- pointers, alignment, stream, return codes -- is as in mi355fa.h.
 */
#ifndef MI355FA_KVCACHE_H_
#define MI355FA_KVCACHE_H_
#include "mi355fa_gqa.h"
#ifdef __cplusplus
extern "C" {
#endif
#define MI355FA_ERR_WORKSPACE (-9) /* workspace_bytes below fa_fwd_kvcache_workspace_bytes(...) */
/* Head dims: D = 64, 128 or 256.  256 is taken by the KV-cache decode calls only (this header and its companions); the
 * training calls of mi355fa.h and fa_supported keep to 64 and 128. */
long long fa_fwd_kvcache_workspace_bytes(int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D);
int fa_fwd_kvcache(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                   const int* cache_seqlens, void* o, float* lse, void* workspace, long long workspace_bytes, int B, int H,
                   int H_kv, int S_q, int S_cache, int S_new, int D, int dtype, float scale, int window_left,
                   int window_right, const mi355fa_opts* opts, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_KVCACHE_H_ */
