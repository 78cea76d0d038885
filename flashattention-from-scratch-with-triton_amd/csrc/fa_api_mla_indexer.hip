// C ABI of the DeepSeek-V3.2 indexer logits over a paged FP8 key cache (include_mla_indexer/mi355fa_mla_indexer.h): the entry
// point, its argument checks and its refusal texts -- a translation unit of its own, as the other decode calls' are: those files'
// refusal texts are recorded sets.  Every error is reported before anything is enqueued, and every text names the argument and
// carries the offending value (fa_last_error() is fa_api.hip's, through api_fail_value).
#include <stdint.h>

#include "../../include_mla_indexer/mi355fa_mla_indexer.h"
#include "fa_mla_indexer.h"
#include "fa_quant_softcap.h"

namespace {

using fa::api_fail_value;

bool misaligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// `n` strides of `what`, each in [0, 2^40] and a multiple of `gran`
int check_strides(const char* fn, const char* fmt, const long long* st, int n, long long gran) {
  for (int i = 0; i < n; ++i)
    if (st[i] < 0 || st[i] % gran != 0 || st[i] > (1ll << 40)) return api_fail_value(MI355FA_ERR_STRIDE, fmt, fn, st[i]);
  return 0;
}

}  // namespace

extern "C" {

int fa_mla_indexer_logits_fp8(const void* q, const float* weights, void* k_cache, float* k_scale, const void* k_new,
                              const int* cache_seqlens, const int* block_table, float* logits, int B, int S_q, int H_i, int W,
                              int num_pages, int page_size, int max_pages_per_seq, long long block_table_stride, int S_new,
                              int dtype, int causal, const long long* q_strides, const long long* weights_strides,
                              const long long* k_strides, const long long* k_scale_strides, const long long* logits_strides,
                              void* stream) {
  const char* fn = "fa_mla_indexer_logits_fp8";
  if (!q) return api_fail_value(MI355FA_ERR_NULL, "%s: q is NULL (argument %lld)", fn, 1);
  if (!weights) return api_fail_value(MI355FA_ERR_NULL, "%s: weights is NULL (argument %lld)", fn, 2);
  if (!k_cache) return api_fail_value(MI355FA_ERR_NULL, "%s: k_cache is NULL (argument %lld)", fn, 3);
  if (!k_scale) return api_fail_value(MI355FA_ERR_NULL, "%s: k_scale is NULL (argument %lld)", fn, 4);
  if (!cache_seqlens) return api_fail_value(MI355FA_ERR_NULL, "%s: cache_seqlens is NULL (argument %lld)", fn, 6);
  if (!block_table) return api_fail_value(MI355FA_ERR_NULL, "%s: block_table is NULL (argument %lld)", fn, 7);
  if (!logits) return api_fail_value(MI355FA_ERR_NULL, "%s: logits is NULL (argument %lld)", fn, 8);
  if (!k_new && S_new != 0) return api_fail_value(MI355FA_ERR_NULL, "%s: S_new != 0 needs k_new (S_new %lld)", fn, S_new);
  if (B < 1 || B > 65535) return api_fail_value(MI355FA_ERR_SHAPE, "%s: B must be in [1, 65535] (got %lld)", fn, B);
  if (S_q < 1 || S_q > (1 << 20)) return api_fail_value(MI355FA_ERR_SHAPE, "%s: S_q must be in [1, 2^20] (got %lld)", fn, S_q);
  if (H_i < 16 || H_i > 64 || H_i % 16 != 0)
    return api_fail_value(MI355FA_ERR_SHAPE, "%s: H_i must be 16, 32, 48 or 64 (got %lld)", fn, H_i);
  if (W < 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: W must be >= 1 (got %lld)", fn, W);
  if (k_new && S_new != S_q)
    return api_fail_value(MI355FA_ERR_SHAPE, "%s: k_new holds one row per query row: S_new must be S_q (S_new %lld)", fn, S_new);
  if (dtype != MI355FA_FP16 && dtype != MI355FA_BF16)
    return api_fail_value(MI355FA_ERR_DTYPE, "%s: dtype must be 0 (fp16) or 1 (bf16), the type of k_new (got %lld)", fn, dtype);
  if (causal != 0 && causal != 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: causal must be 0 or 1 (got %lld)", fn, causal);
  if (page_size < 32 || page_size % 32 != 0)
    return api_fail_value(MI355FA_ERR_PAGED, "%s: page_size must be a positive multiple of 32 (got %lld)", fn, page_size);
  if (num_pages < 1) return api_fail_value(MI355FA_ERR_PAGED, "%s: num_pages must be >= 1 (got %lld)", fn, num_pages);
  if (max_pages_per_seq < 1) return api_fail_value(MI355FA_ERR_PAGED, "%s: max_pages_per_seq must be >= 1 (got %lld)", fn, max_pages_per_seq);
  if ((long long)max_pages_per_seq * page_size > 0x7fffffffLL)
    return api_fail_value(MI355FA_ERR_PAGED, "%s: max_pages_per_seq * page_size must stay below 2^31 (got %lld)", fn,
                          (long long)max_pages_per_seq * page_size);
  if (block_table_stride < (long long)max_pages_per_seq || block_table_stride > 0x7fffffffLL)
    return api_fail_value(MI355FA_ERR_PAGED, "%s: block_table_stride must be at least max_pages_per_seq and below 2^31 (got %lld)", fn,
                          block_table_stride);
  fa::IndexerParams p{};
  p.q_sb = (long long)S_q * H_i * fa::kIdxD, p.q_ss = (long long)H_i * fa::kIdxD, p.q_sh = fa::kIdxD;
  if (q_strides) {
    if (int rc = check_strides(fn, "%s: q_strides must be non-negative multiples of 16 bytes (got %lld)", q_strides, 3, 16)) return rc;
    if (q_strides[2] < fa::kIdxD)
      return api_fail_value(MI355FA_ERR_STRIDE, "%s: the head stride of q must be at least 128 bytes (got %lld)", fn, q_strides[2]);
    p.q_sb = q_strides[0], p.q_ss = q_strides[1], p.q_sh = q_strides[2];
  }
  p.w_sb = (long long)S_q * H_i, p.w_ss = H_i, p.w_sh = 1;
  if (weights_strides) {
    if (int rc = check_strides(fn, "%s: weights_strides must be non-negative and at most 2^40 elements (got %lld)", weights_strides, 3, 1))
      return rc;
    p.w_sb = weights_strides[0], p.w_ss = weights_strides[1], p.w_sh = weights_strides[2];
  }
  long long k_rs = fa::kIdxD;
  p.k_ps = (long long)page_size * fa::kIdxD;
  if (k_strides) {
    if (int rc = check_strides(fn, "%s: k_strides must be non-negative multiples of 16 bytes (got %lld)", k_strides, 2, 16)) return rc;
    if (k_strides[1] < fa::kIdxD || k_strides[1] > (1 << 24))
      return api_fail_value(MI355FA_ERR_STRIDE, "%s: the row stride of k_cache must be in [128, 2^24] bytes (got %lld)", fn, k_strides[1]);
    p.k_ps = k_strides[0], k_rs = k_strides[1];
  }
  p.ks_ps = page_size, p.ks_rs = 1;
  if (k_scale_strides) {
    if (int rc = check_strides(fn, "%s: k_scale_strides must be non-negative and at most 2^40 elements (got %lld)", k_scale_strides, 2, 1))
      return rc;
    p.ks_ps = k_scale_strides[0], p.ks_rs = k_scale_strides[1];
  }
  p.o_sb = (long long)S_q * W, p.o_ss = W;
  if (logits_strides) {
    if (int rc = check_strides(fn, "%s: logits_strides must be non-negative and at most 2^40 elements (got %lld)", logits_strides, 2, 1))
      return rc;
    if ((S_q > 1 && logits_strides[1] < W) || (B > 1 && logits_strides[0] == 0))
      return api_fail_value(MI355FA_ERR_STRIDE, "%s: the rows of logits must not overlap: a row stride of at least W, a non-zero batch stride (row stride %lld)",
                            fn, logits_strides[1]);
    p.o_sb = logits_strides[0], p.o_ss = logits_strides[1];
  }
  if (misaligned(q, 16)) return api_fail_value(MI355FA_ERR_ALIGN, "%s: q must be 16-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)q & 15));
  if (misaligned(k_cache, 16))
    return api_fail_value(MI355FA_ERR_ALIGN, "%s: k_cache must be 16-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)k_cache & 15));
  if (misaligned(k_new, 16))
    return api_fail_value(MI355FA_ERR_ALIGN, "%s: k_new must be 16-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)k_new & 15));
  for (const void* ptr : {(const void*)weights, (const void*)k_scale, (const void*)logits, (const void*)cache_seqlens, (const void*)block_table})
    if (misaligned(ptr, 4))
      return api_fail_value(MI355FA_ERR_ALIGN, "%s: weights, k_scale, logits, cache_seqlens and block_table must be 4-byte aligned (one ends in %lld)",
                            fn, (long long)((uintptr_t)ptr & 3));
  p.q = q;
  p.w = weights;
  p.k = k_cache;
  p.ks = k_scale;
  p.k_new = k_new;
  p.seqlens = cache_seqlens;
  p.table = block_table;
  p.out = logits;
  p.k_rs = (int)k_rs;
  p.B = B, p.Sq = S_q, p.Hi = H_i, p.W = W, p.Snew = S_new, p.causal = causal;
  p.num_pages = num_pages, p.page_size = page_size, p.max_pages = max_pages_per_seq, p.bt_stride = (int)block_table_stride;
  p.tpp = fa::make_fastdiv(page_size / fa::kIdxTile);
  p.pdiv = fa::make_fastdiv(page_size);
  if (hipError_t e = fa::launch_mla_indexer(p, dtype, (hipStream_t)stream))
    return api_fail_value((int)e, "%s: the launch failed (HIP error %lld)", fn, (long long)e);
  return 0;
}

}  // extern "C"
