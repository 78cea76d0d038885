/* mi355fa_mla_indexer_prefill.h -- the DeepSeek-V3.2 "lightning indexer" logits of a PREFILL step in libmi355fa.so: one packed
 * query tensor over several sequences, one contiguous FP8 key array, and a visible key range per query row,
 *
 *     logits[m, t] = k_scale[t] * sum_h weights[m, h] * max(0, sum_d q[m, h, d] * k[t, d])      for ks[m] <= t < ke[m]
 *                  = -inf, exactly                                                               for every other t in [0, W).
 *
 * The decode-step form is fa_mla_indexer_logits_fp8 (mi355fa_mla_indexer.h); its result and this one feed
 * fa_mla_indexer_select (mi355fa_mla_select.h) alike: logits as [M, 1, W] with lengths = ke.  mi355fa_paged.h is included below
 * for the error codes; mi355fa.h, its ABI version and every other header's function list are unchanged.  The header lives in
 * include_mla_indexer_prefill/, as the listings of the other include directories are recorded sets.  Inference only.
 *
 *   q              : e4m3 bytes [M, H_i, 128], 16-byte aligned, the 128 dims contiguous.  H_i in {16, 32, 48, 64}.  M in
 *                    [1, 1048560].
 *   weights        : fp32 [M, H_i].  The caller folds q's dequantisation scale, H_i ** -0.5 and the softmax scale into it.  ReLU
 *                    comes before the weights, which may have either sign.
 *   k              : e4m3 bytes [N, 128], 16-byte aligned, read in place; it may exceed 4 GiB.  N in [0, W]; NULL only with N == 0.
 *   k_scale        : fp32 [N], one scale per key.
 *   ks, ke         : int32 DEVICE arrays [M]; the host reads neither.  Both are clamped to [0, N] by the kernel; a row with
 *                    ke <= ks sees nothing.  A block of 16 query rows reads no key row or scale outside [min ks, max ke) of its
 *                    non-empty ranges, so none at or past N; what a row's range excludes never reaches a logit of that row,
 *                    whatever its bytes and its scale are (the mask is a select, not a multiply).
 *   logits         : fp32 [M, W], 4-byte aligned, W in [1, 2^30].  Every column of [0, W) of every row is written.
 *   q_strides      : BYTE strides {row, head} of q (NULL = contiguous), non-negative multiples of 16, head stride >= 128.
 *   weights_strides: element strides {row, head} of weights (NULL = contiguous), non-negative.
 *   k_row_stride   : BYTE stride of a key row, a multiple of 16 and at least 128.
 *   k_scale_stride : element stride of k_scale, non-negative.
 *   logits_row_stride : element stride of a row of logits, at least W.
 *
 * No workspace, no split and no combine: one workgroup owns 16 rows x a run of columns, so every order of summation is fixed
 * and the result is deterministic.  Every argument error is reported before anything is enqueued, with a text (fa_last_error)
 * that names the argument and carries the offending value.
 */
#ifndef MI355FA_MLA_INDEXER_PREFILL_H_
#define MI355FA_MLA_INDEXER_PREFILL_H_
#include "../include/mi355fa_paged.h"
#ifdef __cplusplus
extern "C" {
#endif
int fa_mla_indexer_logits_fp8_prefill(const void* q, const float* weights, const void* k, const float* k_scale, const int* ks,
                                      const int* ke, float* logits, int M, int H_i, int N, int W, const long long* q_strides,
                                      const long long* weights_strides, long long k_row_stride, long long k_scale_stride,
                                      long long logits_row_stride, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MI355FA_MLA_INDEXER_PREFILL_H_ */
