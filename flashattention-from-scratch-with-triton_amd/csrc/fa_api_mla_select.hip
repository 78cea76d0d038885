// C ABI of the top-k selection from indexer logits (include_mla_select/mi355fa_mla_select.h): the entry point, its argument
// checks and its refusal texts -- a translation unit of its own, as the other decode calls' are: those files' refusal texts are
// recorded sets.  Every error is reported before anything is enqueued, and every text names the argument and carries the
// offending value (fa_last_error() is fa_api.hip's, through api_fail_value).
#include <stdint.h>

#include "../../include_mla_select/mi355fa_mla_select.h"
#include "fa_mla_select.h"
#include "fa_quant_softcap.h"

namespace {

using fa::api_fail_value;

// the {batch, row} strides of `what` [B, S_q, width]: each in [0, 2^40], rows that do not overlap
int check_rows(const char* fn, const char* range_fmt, const char* overlap_fmt, const long long* st, int B, int S_q, int width) {
  for (int i = 0; i < 2; ++i)
    if (st[i] < 0 || st[i] > (1ll << 40)) return api_fail_value(MI355FA_ERR_STRIDE, range_fmt, fn, st[i]);
  if ((S_q > 1 && st[1] < width) || (B > 1 && st[0] == 0)) return api_fail_value(MI355FA_ERR_STRIDE, overlap_fmt, fn, st[1]);
  return 0;
}

}  // namespace

extern "C" {

int fa_mla_indexer_select(const float* logits, const int* lengths, int* indices, int B, int S_q, int W, int topk,
                          const long long* logits_strides, const long long* indices_strides, void* stream) {
  const char* fn = "fa_mla_indexer_select";
  if (!logits) return api_fail_value(MI355FA_ERR_NULL, "%s: logits is NULL (argument %lld)", fn, 1);
  if (!indices) return api_fail_value(MI355FA_ERR_NULL, "%s: indices is NULL (argument %lld)", fn, 3);
  if (B < 1 || B > 65535) return api_fail_value(MI355FA_ERR_SHAPE, "%s: B must be in [1, 65535] (got %lld)", fn, B);
  if (S_q < 1 || S_q > (1 << 20)) return api_fail_value(MI355FA_ERR_SHAPE, "%s: S_q must be in [1, 2^20] (got %lld)", fn, S_q);
  if (W < 1 || W > (1 << 30)) return api_fail_value(MI355FA_ERR_SHAPE, "%s: W must be in [1, 2^30] (got %lld)", fn, W);
  if (topk < 1 || topk > fa::kSelMaxTopk) return api_fail_value(MI355FA_ERR_SHAPE, "%s: topk must be in [1, 65536] (got %lld)", fn, topk);
  fa::SelectParams p{};
  p.l_sb = (long long)S_q * W, p.l_ss = W;
  if (logits_strides) {
    if (int rc = check_rows(fn, "%s: logits_strides must be non-negative and at most 2^40 elements (got %lld)",
                            "%s: the rows of logits must not overlap: a row stride of at least W, a non-zero batch stride (row stride %lld)",
                            logits_strides, B, S_q, W))
      return rc;
    p.l_sb = logits_strides[0], p.l_ss = logits_strides[1];
  }
  p.o_sb = (long long)S_q * topk, p.o_ss = topk;
  if (indices_strides) {
    if (int rc = check_rows(fn, "%s: indices_strides must be non-negative and at most 2^40 elements (got %lld)",
                            "%s: the rows of indices must not overlap: a row stride of at least topk, a non-zero batch stride (row stride %lld)",
                            indices_strides, B, S_q, topk))
      return rc;
    p.o_sb = indices_strides[0], p.o_ss = indices_strides[1];
  }
  for (const void* ptr : {(const void*)logits, (const void*)lengths, (const void*)indices})
    if ((uintptr_t)ptr & 3)
      return api_fail_value(MI355FA_ERR_ALIGN, "%s: logits, lengths and indices must be 4-byte aligned (one ends in %lld)", fn,
                            (long long)((uintptr_t)ptr & 3));
  p.logits = logits, p.lengths = lengths, p.out = indices;
  p.B = B, p.Sq = S_q, p.W = W, p.topk = topk;
  if (hipError_t e = fa::launch_mla_select(p, (hipStream_t)stream))
    return api_fail_value((int)e, "%s: the launch failed (HIP error %lld)", fn, (long long)e);
  return 0;
}

}  // extern "C"
