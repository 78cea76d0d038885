/* mi355fa_kvcache_fp8.h -- decoding attention over a padded KV cache stored in 8-bit floating point, in libmi355fa.so.
 *
 * A companion to mi355fa_kvcache.h (included below for the decoding conventions: shapes, cache_seqlens, the bottom-right
 * mask, the split workspace; mi355fa.h, its ABI version and function list are unchanged).  Inference only.
 *
 * The caches hold OCP float8 e4m3 ("e4m3fn": bias 7, no infinities, largest value 448, the format gfx950 converts in
 * hardware; NOT the e4m3fnuz of MI300), one byte per element, with one fp32 dequantisation factor per (sequence, K/V head)
 * for K and one for V:
 *
 *     K[b, hk, j, :] = float(k_cache[b, hk, j, :]) * k_descale[b, hk]        V likewise with v_descale
 *     O, LSE         = fa_fwd_kvcache's result on those K and V
 *
 * q, o, k_new and v_new are 16-bit (`dtype`: MI355FA_FP16 / MI355FA_BF16); q is not quantised.  Every e4m3 value is exact
 * in fp16 and in bf16, so the kernel converts the cache bytes without rounding; k_descale is folded into the softmax scale
 * and v_descale into the final normalisation, both in fp32.
 *
 *   kv_dtype      : MI355FA_KV_FP8_E4M3; anything else is refused with MI355FA_ERR_DTYPE.
 *   k_cache/v_cache: [B, H_kv, S_cache, D] bytes, 16-byte aligned (MI355FA_ERR_ALIGN).  opts->k_strides / v_strides are
 *                   element strides, here bytes, and must be multiples of 16 (MI355FA_ERR_STRIDE); K and V share their
 *                   sequence stride.
 *   k_descale / v_descale: fp32 DEVICE vectors, 4-byte aligned, read at [b * descale_bstride + hk]: descale_bstride = H_kv
 *                   (or more) for shape (B, H_kv), 0 for one (H_kv,) vector shared by the batch.  NULL = 1.0.  A stride
 *                   that is neither 0 nor >= H_kv is refused with MI355FA_ERR_SHAPE.  The values are the caller's
 *                   responsibility (finite, > 0); the host never reads them, so a step stays graph-capturable.
 *   k_new / v_new : [B, H_kv, S_new, D] in `dtype`, contiguous, or both NULL.  Quantised into cache rows
 *                   [cache_seqlens[b], cache_seqlens[b] + S_new) before attention:
 *                       byte = e4m3_rne(clamp(float(x) / descale[b, hk], -448, 448))
 *                   (correctly rounded fp32 division, saturating, round to nearest even including e4m3 subnormals,
 *                   -0.0 stays -0.0; NaN inputs are unspecified).
 *
 * fa_fwd_kvcache_fp8_workspace_bytes returns the workspace of the fp8 call for the same shape arguments,
 * n * B * H * S_q * (D + 2) * 4 bytes (0 when n = 1); its split count n is the fp8 path's own and may differ from
 * fa_fwd_kvcache's.  Everything else -- the mask, rows with no visible key (O = 0, LSE = -inf), rows past L_b never read,
 * determinism, error codes, `every argument error is reported before anything is enqueued` -- is as in mi355fa_kvcache.h.
 */
#ifndef MI355FA_KVCACHE_FP8_H_
#define MI355FA_KVCACHE_FP8_H_
#include "mi355fa_kvcache.h"
#ifdef __cplusplus
extern "C" {
#endif
#define MI355FA_KV_FP8_E4M3 0 /* kv_dtype: OCP float8 e4m3 (torch.float8_e4m3fn) */
/* Head dims: D = 64, 128 or 256, as for the 16-bit decode call (a cache row is then 256 bytes). */
long long fa_fwd_kvcache_fp8_workspace_bytes(int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D);
int fa_fwd_kvcache_fp8(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                       const int* cache_seqlens, const float* k_descale, const float* v_descale,
                       long long descale_bstride, void* o, float* lse, void* workspace, long long workspace_bytes, int B,
                       int H, int H_kv, int S_q, int S_cache, int S_new, int D, int dtype, int kv_dtype, float scale,
                       int window_left, int window_right, const mi355fa_opts* opts, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_KVCACHE_FP8_H_ */
