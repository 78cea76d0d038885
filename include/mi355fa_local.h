/* mi355fa_local.h -- sliding-window (local) attention entry points of libmi355fa.so.
 *
 * A companion to mi355fa.h (included below; its ABI version and function list are unchanged).  Each function is the
 * corresponding fa_*_ex call of mi355fa.h with the `causal` flag replaced by a window:
 *
 *   key j is visible from query i  iff  j <= i + window_right   (if window_right >= 0)
 *                                   and  j >= i - window_left    (if window_left >= 0)
 *                                   and  j <  S_k.
 *
 * The window is top-left aligned, as `causal` is: (-1, 0) is causal attention and (-1, -1) full attention; -1 means
 * unbounded on that side, a value below -1 is refused with MI355FA_ERR_WINDOW.  This is FlashAttention-2's
 * window_size = (left, right).  A query row that sees no key gets O = 0, LSE = -inf and dQ = 0; a key that no query
 * sees gets dK = dV = 0.
 *
 * `opts` composes as for the _ex functions: strides, cu_seqlens (the window is measured inside each sequence) and the
 * bf16 q_scaled workspace.  Dropout with a window is not supported: opts->p_drop != 0 is refused (MI355FA_ERR_SHAPE).
 * `scale` is the softmax scale as in mi355fa.h: finite and > 0, else MI355FA_ERR_SHAPE.  Everything else -- pointers,
 * ownership, stream, return codes, fa_bwd_dkv_local after fa_bwd_dq_local -- is as in mi355fa.h.  The work of a launch scales with the visible (query, key) pairs, not with S_q * S_k.
 */
#ifndef MI355FA_LOCAL_H_
#define MI355FA_LOCAL_H_
#include "mi355fa.h"
#ifdef __cplusplus
extern "C" {
#endif
#define MI355FA_ERR_WINDOW (-7) /* window_left or window_right below -1 */
int fa_fwd_local(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int S_q, int S_k, int D,
                 int dtype, float scale, int window_left, int window_right, const mi355fa_opts* opts, void* stream);
int fa_bwd_dq_local(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                    void* dq, float* delta, int B, int H, int S_q, int S_k, int D, int dtype, float scale, int window_left,
                    int window_right, const mi355fa_opts* opts, void* stream);
int fa_bwd_dkv_local(const void* q, const void* k, const void* v, const void* dout, const float* lse, const float* delta,
                     void* dk, void* dv, int B, int H, int S_q, int S_k, int D, int dtype, float scale, int window_left,
                     int window_right, const mi355fa_opts* opts, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_LOCAL_H_ */
