// C ABI of the sparse MLA prefill call (include_mla_sparse_prefill/mi355fa_mla_sparse_prefill.h): the entry point, its argument
// checks and its refusal texts -- a translation unit of its own, as fa_api_mla.hip's refusal texts are a recorded set.  Every
// error is reported before anything is enqueued, and every text names the argument and carries the offending value
// (fa_last_error() is fa_api.hip's, through api_fail_value).
#include <stdint.h>
#include <string.h>

#include "../../include_mla_sparse_prefill/mi355fa_mla_sparse_prefill.h"
#include "fa_decode_mla.h"
#include "fa_mla_sparse_prefill.h"
#include "fa_quant_softcap.h"

namespace {

using fa::api_fail_value;

// Element strides {row, head} of q or o (NULL = contiguous rows of `width`) -> bytes.
int row_head_strides(const char* fn, bool q, const long long* st, int H, int width, long long* sm, long long* sh) {
  *sm = (long long)H * width * 2, *sh = (long long)width * 2;
  if (!st) return 0;
  for (int i = 0; i < 2; ++i)
    if (st[i] < 0 || (st[i] & 7) != 0 || st[i] > (1ll << 40))
      return api_fail_value(MI355FA_ERR_STRIDE,
                            q ? "%s: q_strides must be non-negative multiples of 8 elements (got %lld)"
                              : "%s: o_strides must be non-negative multiples of 8 elements (got %lld)", fn, st[i]);
  if (!q && H > 1 && st[1] < width)
    return api_fail_value(MI355FA_ERR_STRIDE, "%s: the head stride of o must be at least 512 elements (got %lld)", fn, st[1]);
  if (!q && st[0] < width)
    return api_fail_value(MI355FA_ERR_STRIDE, "%s: the row stride of o must be at least 512 elements (got %lld)", fn, st[0]);
  *sm = st[0] * 2, *sh = st[1] * 2;
  return 0;
}

}  // namespace

extern "C" {

int fa_fwd_mla_sparse_prefill(const void* q, const void* kv, const int* indices, void* o, float* lse, int M, int H, int N, int topk,
                              int dtype, float scale, const long long* q_strides, long long kv_row_stride, const long long* o_strides,
                              long long indices_row_stride, void* stream) {
  const char* fn = "fa_fwd_mla_sparse_prefill";
  if (!q) return api_fail_value(MI355FA_ERR_NULL, "%s: q is NULL (argument %lld)", fn, 1);
  if (!indices) return api_fail_value(MI355FA_ERR_NULL, "%s: indices is NULL (argument %lld)", fn, 3);
  if (!o) return api_fail_value(MI355FA_ERR_NULL, "%s: o is NULL (argument %lld)", fn, 4);
  if (dtype != MI355FA_FP16 && dtype != MI355FA_BF16)
    return api_fail_value(MI355FA_ERR_DTYPE, "%s: dtype must be 0 (fp16) or 1 (bf16) (got %lld)", fn, dtype);
  {   // finite and > 0, tested on the bits (this file is built with -fno-honor-nans)
    uint32_t u;
    memcpy(&u, &scale, sizeof(u));
    if ((u >> 31) != 0 || (u & 0x7fffffffu) == 0 || ((u >> 23) & 0xffu) == 0xffu)
      return api_fail_value(MI355FA_ERR_SHAPE, "%s: scale must be finite and > 0 (its bits are %lld)", fn, (long long)u);
  }
  if (M < 1 || M > fa::kRowListMaxM) return api_fail_value(MI355FA_ERR_SHAPE, "%s: M must be in [1, 2^22] (got %lld)", fn, M);
  if (H < 1 || H > fa::kRowListMaxH) return api_fail_value(MI355FA_ERR_SHAPE, "%s: H must be in [1, 1024] (got %lld)", fn, H);
  if (N < 0) return api_fail_value(MI355FA_ERR_SHAPE, "%s: N must be >= 0 (got %lld)", fn, N);
  if (topk < 1 || topk > (1 << 24)) return api_fail_value(MI355FA_ERR_SHAPE, "%s: topk must be in [1, 2^24] (got %lld)", fn, topk);
  if (N > 0 && !kv) return api_fail_value(MI355FA_ERR_NULL, "%s: kv is NULL (argument %lld)", fn, 2);
  fa::RowListParams p{};
  if (int rc = row_head_strides(fn, true, q_strides, H, fa::kMlaD, &p.q_sm, &p.q_sh)) return rc;
  if (int rc = row_head_strides(fn, false, o_strides, H, fa::kMlaDv, &p.o_sm, &p.o_sh)) return rc;
  if (kv_row_stride < fa::kMlaD || (kv_row_stride & 7) != 0 || kv_row_stride > (1 << 24))
    return api_fail_value(MI355FA_ERR_STRIDE, "%s: kv_row_stride must be a multiple of 8 in [576, 2^24] elements (got %lld)", fn, kv_row_stride);
  if (indices_row_stride < 0 || indices_row_stride > (1ll << 40))
    return api_fail_value(MI355FA_ERR_STRIDE, "%s: indices_row_stride must be non-negative and at most 2^40 elements (got %lld)", fn,
                          indices_row_stride);
  const struct {
    const char* text;
    const void* ptr;
    unsigned a;
  } rows[] = {{"%s: q must be 16-byte aligned (ends in %lld)", q, 16},
              {"%s: kv must be 16-byte aligned (ends in %lld)", kv, 16},
              {"%s: o must be 16-byte aligned (ends in %lld)", o, 16},
              {"%s: lse must be 4-byte aligned (ends in %lld)", lse, 4},
              {"%s: indices must be 4-byte aligned (ends in %lld)", indices, 4}};
  for (const auto& r : rows)
    if ((uintptr_t)r.ptr & (r.a - 1)) return api_fail_value(MI355FA_ERR_ALIGN, r.text, fn, (long long)((uintptr_t)r.ptr & (r.a - 1)));
  p.q = q, p.kv = kv, p.indices = indices, p.o = o, p.lse = lse;
  p.kv_rs = kv_row_stride * 2, p.idx_rs = indices_row_stride;
  p.M = M, p.H = H, p.N = N, p.topk = topk, p.scale = scale;
  if (hipError_t e = fa::launch_mla_sparse_prefill(p, dtype, (hipStream_t)stream))
    return api_fail_value((int)e, "%s: the launch failed (HIP error %lld)", fn, (long long)e);
  return 0;
}

}  // extern "C"
