/* mi355fa_sink.h -- learned attention sinks (gpt-oss; FlashAttention-3's `s_aux`, vLLM's `sinks`) in libmi355fa.so.
 *
 * A companion to mi355fa_kvcache_fp8.h (included below for the GQA, window and decoding conventions; mi355fa.h, its ABI
 * version and function list are unchanged).  A sink is one extra logit z_h per QUERY head that joins the softmax
 * denominator of every row of that head and carries no value.  With the visible scores s_ij = scale * q_i . k_j, masked as
 * the call's mask says, and pos_q as in the sink-less call:
 *
 *     LSE_i = log( exp(z_h) + sum_j exp(s_ij) )        natural log, the sink INCLUDED
 *     P_ij  = exp(s_ij - LSE_i)                         rows sum to less than 1
 *     O_i   = sum_j P_ij v_j                            the sink has no value row
 *     p0_i  = exp(z_h - LSE_i)                          the mass the sink took
 *
 * z_h is in natural-log units and is NOT multiplied by `scale` (the gpt-oss / FlashAttention-3 / vLLM convention).
 *
 * Backward, with delta_i = dO_i . O_i:
 *
 *     dV = P^T dO,  dS_ij = P_ij (dP_ij - delta_i),  dQ = scale dS K,  dK = scale dS^T Q      (the sink-less formulas)
 *     dz_h = - sum over b, i of  p0_i * delta_i                                                (the sink's dP is 0)
 *
 * P is recomputed from the saved LSE and delta from O and dO, so the backward of fa_fwd_sink is
 *     fa_bwd_dq_gqa   on this forward's O and LSE (it writes dQ and delta),
 *     fa_bwd_dkv_gqa  on the same LSE and that delta,
 *     fa_bwd_dsink    on the same LSE and that delta (any time after fa_bwd_dq_gqa, same stream),
 * with the same window, strides, cu_seqlens and bf16 q_scaled workspace as any _gqa backward.
 *
 *   fa_fwd_sink             fa_fwd_gqa with `sinks` after `scale`.
 *   fa_bwd_dsink            dsinks[h] = - sum_{b,i} exp(sinks[h] - lse[b,h,i]) * delta[b,h,i].  lse and delta are the
 *                           [B, H, S_q] fp32 rows (16-byte aligned) the forward and fa_bwd_dq_gqa wrote; with
 *                           opts->cu_seqlens_q they are the packed [H, total_q] rows, B is the number of sequences and S_q
 *                           the longest one (opts->total_q rows per head are summed).  Of `opts` only cu_seqlens_q /
 *                           cu_seqlens_k / total_q / total_k are read.  dsinks is fp32 (H,) on the device, 4-byte aligned,
 *                           OVERWRITTEN, not accumulated.  fp32 throughout, one workgroup per head, a fixed reduction
 *                           order and no atomics: the same inputs give the same bits.
 *   fa_fwd_kvcache_sink     fa_fwd_kvcache with `sinks` after `scale`.
 *   fa_fwd_kvcache_fp8_sink fa_fwd_kvcache_fp8 with `sinks` after `scale`; k_descale scales the scores only, never the
 *                           sink, and v_descale the output only.
 * The decoding calls use the split count and the workspace size of their sink-less forms
 * (fa_fwd_kvcache_workspace_bytes / fa_fwd_kvcache_fp8_workspace_bytes); the sink enters a row's softmax exactly once,
 * whatever the split count.
 *
 * sinks: fp32 on the device, shape (H,), indexed by query head, 4-byte aligned.  NULL is refused with MI355FA_ERR_NULL,
 * a pointer that is not 4-byte aligned with MI355FA_ERR_ALIGN.  The host never reads the values, so a decoding step stays
 * graph-capturable and the sinks may change between replays.
 *
 * Edge cases:
 *   - a row with no visible key (a window that holds none, S_k = 0 of a packed sequence, L_b = 0) gets O = 0 and
 *     LSE = z_h (finite, not -inf), dQ = 0, and contributes -delta = 0 to dz;
 *   - z_h = -inf is defined: O, LSE, dQ, dK and dV are, bit for bit, those of the sink-less call (a row with no visible
 *     key then has O = 0 and LSE = -inf), and dz_h = 0;
 *   - z_h = +inf or NaN gives undefined output.
 *
 * `scale` must be finite and > 0 (MI355FA_ERR_SHAPE).  Dropout is not supported: opts->p_drop != 0 is refused
 * (MI355FA_ERR_SHAPE).  Sinks do not combine with mi355fa_softcap.h or mi355fa_alibi.h (there is no entry point that takes
 * both).  Every argument error is reported before anything is enqueued; fa_last_error names the argument.  Pointers,
 * ownership, stream and return codes are as in mi355fa.h.
 */
#ifndef MI355FA_SINK_H_
#define MI355FA_SINK_H_
#include "mi355fa_kvcache_fp8.h"
#ifdef __cplusplus
extern "C" {
#endif
int fa_fwd_sink(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int H_kv, int S_q, int S_k,
                int D, int dtype, float scale, const float* sinks, int window_left, int window_right,
                const mi355fa_opts* opts, void* stream);
int fa_bwd_dsink(const float* lse, const float* delta, const float* sinks, float* dsinks, int B, int H, int S_q,
                 const mi355fa_opts* opts, void* stream);
/* The two decoding calls below also take D = 256 (mi355fa_kvcache.h); the training calls above keep to 64 and 128. */
int fa_fwd_kvcache_sink(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                        const int* cache_seqlens, void* o, float* lse, void* workspace, long long workspace_bytes, int B,
                        int H, int H_kv, int S_q, int S_cache, int S_new, int D, int dtype, float scale, const float* sinks,
                        int window_left, int window_right, const mi355fa_opts* opts, void* stream);
int fa_fwd_kvcache_fp8_sink(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                            const int* cache_seqlens, const float* k_descale, const float* v_descale,
                            long long descale_bstride, void* o, float* lse, void* workspace, long long workspace_bytes,
                            int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D, int dtype, int kv_dtype,
                            float scale, const float* sinks, int window_left, int window_right, const mi355fa_opts* opts,
                            void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_SINK_H_ */
