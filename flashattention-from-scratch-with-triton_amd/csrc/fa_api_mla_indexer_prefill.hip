// C ABI of the prefill indexer logits (include_mla_indexer_prefill/mi355fa_mla_indexer_prefill.h): the entry point, its argument
// checks and its refusal texts -- a translation unit of its own, as the other decode calls' are: those files' refusal texts are
// recorded sets.  Every error is reported before anything is enqueued, and every text names the argument and carries the
// offending value (fa_last_error() is fa_api.hip's, through api_fail_value).
#include <stdint.h>

#include "../../include_mla_indexer_prefill/mi355fa_mla_indexer_prefill.h"
#include "fa_mla_indexer_prefill.h"
#include "fa_quant_softcap.h"

namespace {

using fa::api_fail_value;

constexpr long long kMaxStride = 1ll << 40;

}  // namespace

extern "C" {

int fa_mla_indexer_logits_fp8_prefill(const void* q, const float* weights, const void* k, const float* k_scale, const int* ks,
                                      const int* ke, float* logits, int M, int H_i, int N, int W, const long long* q_strides,
                                      const long long* weights_strides, long long k_row_stride, long long k_scale_stride,
                                      long long logits_row_stride, void* stream) {
  const char* fn = "fa_mla_indexer_logits_fp8_prefill";
  if (!q) return api_fail_value(MI355FA_ERR_NULL, "%s: q is NULL (argument %lld)", fn, 1);
  if (!weights) return api_fail_value(MI355FA_ERR_NULL, "%s: weights is NULL (argument %lld)", fn, 2);
  if (!ks) return api_fail_value(MI355FA_ERR_NULL, "%s: ks is NULL (argument %lld)", fn, 5);
  if (!ke) return api_fail_value(MI355FA_ERR_NULL, "%s: ke is NULL (argument %lld)", fn, 6);
  if (!logits) return api_fail_value(MI355FA_ERR_NULL, "%s: logits is NULL (argument %lld)", fn, 7);
  if (M < 1 || M > fa::kPreMaxM) return api_fail_value(MI355FA_ERR_SHAPE, "%s: M must be in [1, 1048560] (got %lld)", fn, M);
  if (H_i < 16 || H_i > 64 || H_i % 16 != 0)
    return api_fail_value(MI355FA_ERR_SHAPE, "%s: H_i must be 16, 32, 48 or 64 (got %lld)", fn, H_i);
  if (W < 1 || W > (1 << 30)) return api_fail_value(MI355FA_ERR_SHAPE, "%s: W must be in [1, 2^30] (got %lld)", fn, W);
  if (N < 0 || N > W) return api_fail_value(MI355FA_ERR_SHAPE, "%s: N must be in [0, W] (got %lld)", fn, N);
  if (N > 0 && !k) return api_fail_value(MI355FA_ERR_NULL, "%s: k is NULL (argument %lld)", fn, 3);
  if (N > 0 && !k_scale) return api_fail_value(MI355FA_ERR_NULL, "%s: k_scale is NULL (argument %lld)", fn, 4);
  fa::IdxPrefillParams p{};
  p.q_sm = (long long)H_i * 128, p.q_sh = 128;
  if (q_strides) {
    for (int i = 0; i < 2; ++i)
      if (q_strides[i] < 0 || q_strides[i] % 16 != 0 || q_strides[i] > kMaxStride)
        return api_fail_value(MI355FA_ERR_STRIDE, "%s: q_strides must be non-negative multiples of 16 bytes (got %lld)", fn, q_strides[i]);
    if (q_strides[1] < 128)
      return api_fail_value(MI355FA_ERR_STRIDE, "%s: the head stride of q must be at least 128 bytes (got %lld)", fn, q_strides[1]);
    p.q_sm = q_strides[0], p.q_sh = q_strides[1];
  }
  p.w_sm = H_i, p.w_sh = 1;
  if (weights_strides) {
    for (int i = 0; i < 2; ++i)
      if (weights_strides[i] < 0 || weights_strides[i] > kMaxStride)
        return api_fail_value(MI355FA_ERR_STRIDE, "%s: weights_strides must be non-negative and at most 2^40 elements (got %lld)", fn,
                              weights_strides[i]);
    p.w_sm = weights_strides[0], p.w_sh = weights_strides[1];
  }
  if (k_row_stride < 128 || k_row_stride % 16 != 0 || k_row_stride > (1 << 24))
    return api_fail_value(MI355FA_ERR_STRIDE, "%s: k_row_stride must be a multiple of 16 in [128, 2^24] bytes (got %lld)", fn, k_row_stride);
  if (k_scale_stride < 0 || k_scale_stride > kMaxStride)
    return api_fail_value(MI355FA_ERR_STRIDE, "%s: k_scale_stride must be non-negative and at most 2^40 elements (got %lld)", fn, k_scale_stride);
  if (logits_row_stride < W || logits_row_stride > kMaxStride)
    return api_fail_value(MI355FA_ERR_STRIDE, "%s: the rows of logits must not overlap: logits_row_stride must be at least W (got %lld)", fn,
                          logits_row_stride);
  if ((uintptr_t)q & 15) return api_fail_value(MI355FA_ERR_ALIGN, "%s: q must be 16-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)q & 15));
  if ((uintptr_t)k & 15) return api_fail_value(MI355FA_ERR_ALIGN, "%s: k must be 16-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)k & 15));
  for (const void* ptr : {(const void*)weights, (const void*)k_scale, (const void*)ks, (const void*)ke, (const void*)logits})
    if ((uintptr_t)ptr & 3)
      return api_fail_value(MI355FA_ERR_ALIGN, "%s: weights, k_scale, ks, ke and logits must be 4-byte aligned (one ends in %lld)", fn,
                            (long long)((uintptr_t)ptr & 3));
  p.q = q, p.w = weights, p.k = k, p.ks = k_scale, p.lo = ks, p.hi = ke, p.out = logits;
  p.k_rs = k_row_stride, p.s_rs = k_scale_stride, p.o_sm = logits_row_stride;
  p.M = M, p.Hi = H_i, p.N = N, p.W = W;
  if (hipError_t e = fa::launch_mla_indexer_prefill(p, (hipStream_t)stream))
    return api_fail_value((int)e, "%s: the launch failed (HIP error %lld)", fn, (long long)e);
  return 0;
}

}  // extern "C"
