/* mi355fa_gqa.h -- grouped-query attention (GQA) entry points of libmi355fa.so.
 *
 * A companion to mi355fa_local.h (included below; mi355fa.h, its ABI version and function list are unchanged).  Each
 * function is the corresponding fa_*_local call with one more argument, H_kv, the number of K/V heads:
 *
 *   Q, O, dO, dQ are [B, H, S_q, D];  K, V, dK, dV are [B, H_kv, S_k, D];  LSE and delta are [B, H, S_q].
 *   H must be a positive multiple of H_kv; g = H / H_kv, and query head h reads K/V head h / g
 *   (torch's repeat_interleave(g, dim=1), as in FlashAttention-2 and SDPA's enable_gqa).  H_kv = 1 is multi-query
 *   attention, H_kv = H plain multi-head attention.  H_kv < 1 or H % H_kv != 0 is refused with MI355FA_ERR_GROUP.
 *
 *   dK[b, j] and dV[b, j] are the sums over the query heads j*g .. (j+1)*g - 1 of their per-head gradients, taken in
 *   fp32 inside the kernel in ascending head order and rounded once to 16 bits: the result is deterministic.
 *
 * The window (window_left, window_right) is that of mi355fa_local.h: (-1, -1) is full attention, (-1, 0) causal.
 *
 * `opts` composes as for the _local functions: strides (those of K, V, dK and dV describe [B, H_kv, S_k, D]),
 * cu_seqlens (K and V then packed as [total_k, H_kv, D], Q as [total_q, H, D]) and the bf16 q_scaled workspace, which
 * is Q-sized ([B, H, S_q, D] or [total_q, H, D]).  Dropout is not supported: opts->p_drop != 0 is refused
 * (MI355FA_ERR_SHAPE).  `scale` is the softmax scale as in mi355fa.h: finite and > 0, else MI355FA_ERR_SHAPE.  Every
 * argument error is reported before anything is enqueued.  Everything else -- pointers,
 * ownership, stream, return codes, fa_bwd_dkv_gqa after fa_bwd_dq_gqa -- is as in mi355fa.h.
 */
#ifndef MI355FA_GQA_H_
#define MI355FA_GQA_H_
#include "mi355fa_local.h"
#ifdef __cplusplus
extern "C" {
#endif
#define MI355FA_ERR_GROUP (-8) /* H_kv < 1, or H not a multiple of H_kv */
int fa_fwd_gqa(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int H_kv, int S_q, int S_k,
               int D, int dtype, float scale, int window_left, int window_right, const mi355fa_opts* opts, void* stream);
int fa_bwd_dq_gqa(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, void* dq,
                  float* delta, int B, int H, int H_kv, int S_q, int S_k, int D, int dtype, float scale, int window_left,
                  int window_right, const mi355fa_opts* opts, void* stream);
int fa_bwd_dkv_gqa(const void* q, const void* k, const void* v, const void* dout, const float* lse, const float* delta,
                   void* dk, void* dv, int B, int H, int H_kv, int S_q, int S_k, int D, int dtype, float scale,
                   int window_left, int window_right, const mi355fa_opts* opts, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_GQA_H_ */
