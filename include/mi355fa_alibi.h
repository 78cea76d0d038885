/* mi355fa_alibi.h -- ALiBi position bias (FlashAttention-2's `alibi_slopes`) in libmi355fa.so.
 *
 * A companion to mi355fa_kvcache.h (included below for the GQA, window and decoding conventions; mi355fa.h, its ABI
 * version and function list are unchanged).  Each function is the corresponding GQA or KV-cache call with two more
 * arguments, `alibi_slopes` and `slopes_batch_stride`, right after `scale`.  For every visible score
 *
 *     s_ij = scale * q_i . k_j  -  slope_h * |pos_q(i) - j|          (natural-log units, ALiBi: Press et al., 2022)
 *     P = softmax over the visible j of s_ij,  O = P V,  LSE_i = logsumexp_j s_ij (natural log, bias included)
 *     dV = P^T dO,  dS_ij = P_ij (dP_ij - delta_i),  dQ = scale dS K,  dK = scale dS^T Q
 *
 * The bias is added before the masks and the softmax.  It depends on neither Q nor K, so dS has no extra factor, and
 * there is no gradient for the slopes.  pos_q(i) is the query position the call's mask already uses:
 *   - the training calls (fa_fwd_alibi, fa_bwd_dq_alibi, fa_bwd_dkv_alibi) are top-left aligned, as every training mask
 *     of this library (mi355fa_local.h): pos_q(i) = i;
 *   - the decoding call (fa_fwd_kvcache_alibi) is bottom-right aligned: pos_q(i) = L_b - S_q + i, L_b the key count
 *     after the append.
 * FlashAttention-2 biases by |i + S_k - S_q - j|.  That is the same whenever the two alignments agree: every decoding
 * call, and every training call with S_q = S_k per sequence.  A training call with S_q != S_k uses |i - j|.
 * FlashAttention-2's causal kernel adds slope * j instead of -slope * |i - j|, which shifts its LSE by a per-row
 * constant; here LSE is the logsumexp of s_ij above.
 *
 * alibi_slopes: fp32 on the device, 4-byte aligned, indexed by QUERY head.  slopes_batch_stride counts elements: 0 means
 * one slope per head, shape (H,), shared by the batch; >= H means shape (B, H) with row b at alibi_slopes +
 * b * slopes_batch_stride (under cu_seqlens, B is the number of sequences).  A NULL pointer is refused with
 * MI355FA_ERR_NULL, a pointer that is not 4-byte aligned with MI355FA_ERR_ALIGN, a negative stride, 0 < stride < H, or a
 * slope index beyond 2^31 - 1 with MI355FA_ERR_ALIBI.  The host never reads the values (a decoding step with ALiBi
 * stays graph-capturable): any finite slope is defined, 0 and negative values included; a NaN or inf slope gives
 * undefined output.
 *
 * The masks act on s as in the unbiased calls: the training calls take the window of mi355fa_local.h ((-1, -1) full
 * attention, (-1, 0) causal), and H_kv K/V heads as in mi355fa_gqa.h (H_kv = H is plain multi-head attention; dK / dV are
 * summed over each group in fp32).  The decoding call is fa_fwd_kvcache with its mask, its split count and its workspace
 * size (fa_fwd_kvcache_workspace_bytes).  A row with no visible key gets O = 0, LSE = -inf and dQ = 0.
 *
 * `scale` must be finite and > 0 (MI355FA_ERR_SHAPE).  Dropout is not supported: opts->p_drop != 0 is refused
 * (MI355FA_ERR_SHAPE), and neither is a combination with mi355fa_softcap.h.  `opts` otherwise composes as for the _gqa
 * functions (strides, cu_seqlens, the bf16 q_scaled workspace: fa_bwd_dq_alibi then stores the Q rows it multiplied and
 * fa_bwd_dkv_alibi reads them) and as for fa_fwd_kvcache (q, k, v, o strides only).  Every argument error is reported
 * before anything is enqueued; fa_last_error names the argument.  Pointers, ownership, stream, return codes and the order
 * fa_bwd_dkv_alibi after fa_bwd_dq_alibi are as in mi355fa.h.
 */
#ifndef MI355FA_ALIBI_H_
#define MI355FA_ALIBI_H_
#include "mi355fa_kvcache.h"
#ifdef __cplusplus
extern "C" {
#endif
#define MI355FA_ERR_ALIBI (-11) /* slopes_batch_stride negative, 0 < slopes_batch_stride < H, or too large */
int fa_fwd_alibi(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int H_kv, int S_q,
                 int S_k, int D, int dtype, float scale, const float* alibi_slopes, long long slopes_batch_stride,
                 int window_left, int window_right, const mi355fa_opts* opts, void* stream);
int fa_bwd_dq_alibi(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                    void* dq, float* delta, int B, int H, int H_kv, int S_q, int S_k, int D, int dtype, float scale,
                    const float* alibi_slopes, long long slopes_batch_stride, int window_left, int window_right,
                    const mi355fa_opts* opts, void* stream);
int fa_bwd_dkv_alibi(const void* q, const void* k, const void* v, const void* dout, const float* lse, const float* delta,
                     void* dk, void* dv, int B, int H, int H_kv, int S_q, int S_k, int D, int dtype, float scale,
                     const float* alibi_slopes, long long slopes_batch_stride, int window_left, int window_right,
                     const mi355fa_opts* opts, void* stream);
/* The decoding call below also takes D = 256 (mi355fa_kvcache.h); the training calls above keep to 64 and 128. */
int fa_fwd_kvcache_alibi(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                         const int* cache_seqlens, void* o, float* lse, void* workspace, long long workspace_bytes, int B,
                         int H, int H_kv, int S_q, int S_cache, int S_new, int D, int dtype, float scale,
                         const float* alibi_slopes, long long slopes_batch_stride, int window_left, int window_right,
                         const mi355fa_opts* opts, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_ALIBI_H_ */
