/* mi355fa_softcap.h -- logit soft-capping (FlashAttention-2's `softcap`) in libmi355fa.so.
 *
 * A companion to mi355fa_kvcache.h (included below for the GQA, window and decoding conventions; mi355fa.h, its ABI
 * version and function list are unchanged).  Each function is the corresponding GQA or KV-cache call with one more
 * argument, `softcap`, right after `scale`.  For every visible score
 *
 *     t_ij = tanh(scale * q_i . k_j / softcap),   u_ij = softcap * t_ij
 *     P = softmax over the visible j of u_ij,  O = P V,  LSE_i = logsumexp_j u_ij (natural log)
 *     dV = P^T dO,  dS_ij = P_ij (dP_ij - delta_i) (1 - t_ij^2),  dQ = scale dS K,  dK = scale dS^T Q
 *
 * (Gemma 2 caps at 50, Grok-1 at 30.)  The masks act on u as they act on the score of the uncapped calls: the training
 * calls take the window of mi355fa_local.h, top-left aligned ((-1, -1) full attention, (-1, 0) causal), and H_kv K/V heads
 * as in mi355fa_gqa.h (H_kv = H is plain multi-head attention; dK / dV are summed over each group in fp32).  The decoding
 * call is fa_fwd_kvcache with its bottom-right aligned mask, its split count and its workspace size
 * (fa_fwd_kvcache_workspace_bytes).  A row with no visible key gets O = 0, LSE = -inf and dQ = 0.
 *
 * softcap must be finite and > 0; 0, -0, a negative value, NaN and +-inf are refused with MI355FA_ERR_SOFTCAP.  `scale`
 * must be finite and > 0 (MI355FA_ERR_SHAPE).  Dropout is not supported: opts->p_drop != 0 is refused (MI355FA_ERR_SHAPE).
 * `opts` otherwise composes as for the _gqa functions (strides, cu_seqlens, the bf16 q_scaled workspace: fa_bwd_dq_softcap
 * then stores the Q rows it multiplied and fa_bwd_dkv_softcap reads them) and as for fa_fwd_kvcache (q, k, v, o strides
 * only).  Every argument error is reported before anything is enqueued; fa_last_error names the argument.  Pointers,
 * ownership, stream, return codes and the order fa_bwd_dkv_softcap after fa_bwd_dq_softcap are as in mi355fa.h.
 */
#ifndef MI355FA_SOFTCAP_H_
#define MI355FA_SOFTCAP_H_
#include "mi355fa_kvcache.h"
#ifdef __cplusplus
extern "C" {
#endif
#define MI355FA_ERR_SOFTCAP (-10) /* softcap not finite and > 0 */
int fa_fwd_softcap(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int H_kv, int S_q,
                   int S_k, int D, int dtype, float scale, float softcap, int window_left, int window_right,
                   const mi355fa_opts* opts, void* stream);
int fa_bwd_dq_softcap(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                      void* dq, float* delta, int B, int H, int H_kv, int S_q, int S_k, int D, int dtype, float scale,
                      float softcap, int window_left, int window_right, const mi355fa_opts* opts, void* stream);
int fa_bwd_dkv_softcap(const void* q, const void* k, const void* v, const void* dout, const float* lse, const float* delta,
                       void* dk, void* dv, int B, int H, int H_kv, int S_q, int S_k, int D, int dtype, float scale,
                       float softcap, int window_left, int window_right, const mi355fa_opts* opts, void* stream);
/* The decoding call below also takes D = 256 (mi355fa_kvcache.h); the training calls above keep to 64 and 128. */
int fa_fwd_kvcache_softcap(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                           const int* cache_seqlens, void* o, float* lse, void* workspace, long long workspace_bytes,
                           int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D, int dtype, float scale,
                           float softcap, int window_left, int window_right, const mi355fa_opts* opts, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_SOFTCAP_H_ */
