// C ABI of sparse (top-k indexed) MLA decoding over the paged FP8 latent cache
// (include_mla_sparse_fp8/mi355fa_kvcache_mla_sparse_fp8.h): the two entry points, their argument checks and their refusal
// texts -- a translation unit of its own, as fa_api_mla_fp8.hip and fa_api_mla_sparse.hip are: those files' refusal texts are
// recorded sets, and their helpers are local to them.  The pool's checks are the former's (byte strides), the list's the
// latter's.  Every error is reported before anything is enqueued, and every text names the argument and carries the offending
// value (fa_last_error() is fa_api.hip's, through api_fail_value).
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include_mla_sparse_fp8/mi355fa_kvcache_mla_sparse_fp8.h"
#include "fa_decode_mla_sparse.h"
#include "fa_decode_mla_sparse_fp8.h"
#include "fa_quant_softcap.h"

namespace fa {
extern std::atomic<int> g_force_kvsplits;   // fa_api.hip: fa_debug_kvcache_splits(), 0 = the formula
}

namespace {

using fa::api_fail_value;

// What the call and its workspace function share: the shape, the list length, the page geometry and the launch's split count.
int gather_shape(const char* fn, int B, int H, int S_q, int topk, int max_pages, int page_size, int S_new, int* S_cache, int* nsplit) {
  if (B < 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: B must be >= 1 (got %lld)", fn, B);
  if (H < 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: H must be >= 1 (got %lld)", fn, H);
  if (S_q < 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: S_q must be >= 1 (got %lld)", fn, S_q);
  if (S_new < 0) return api_fail_value(MI355FA_ERR_SHAPE, "%s: S_new must be >= 0 (got %lld)", fn, S_new);
  if (topk < 1 || topk > (1 << 24)) return api_fail_value(MI355FA_ERR_SHAPE, "%s: topk must be in [1, 2^24] (got %lld)", fn, topk);
  if ((long long)H * S_q > (1 << 24))
    return api_fail_value(MI355FA_ERR_SHAPE, "%s: too many query rows for one launch: H * S_q is at most 2^24 (got %lld)", fn,
                          (long long)H * S_q);
  if (page_size < 32 || page_size % 32 != 0)
    return api_fail_value(MI355FA_ERR_PAGED, "%s: page_size must be a positive multiple of 32 (got %lld)", fn, page_size);
  if (max_pages < 1) return api_fail_value(MI355FA_ERR_PAGED, "%s: max_pages_per_seq must be >= 1 (got %lld)", fn, max_pages);
  if ((long long)max_pages * page_size > 0x7fffffffLL)
    return api_fail_value(MI355FA_ERR_PAGED, "%s: max_pages_per_seq * page_size must stay below 2^31 (got %lld)", fn,
                          (long long)max_pages * page_size);
  *S_cache = max_pages * page_size;
  const long long wgs = (long long)B * S_q * ((H + 31) / 32);
  *nsplit = fa::mla_sparse_splits(wgs, topk, fa::g_force_kvsplits.load(std::memory_order_relaxed));
  if (wgs * *nsplit > (1ll << 31) - 1 || (long long)B * H * S_q * fa::kMlaDv > (1ll << 40))
    return api_fail_value(MI355FA_ERR_SHAPE, "%s: too many workgroups or rows for one launch (B * S_q * head blocks * splits = %lld)",
                          fn, wgs * *nsplit);
  return 0;
}

// Element strides {batch, head, row} of q or o (NULL = contiguous rows of `width`) -> the byte layout.
int gather_layout(const char* fn, bool q, const long long* st, int B, int H, int S, int width, fa::TensorLayout* out) {
  if (!st) {
    *out = fa::TensorLayout{(long long)H * S * width * 2, (long long)S * width * 2, width * 2};
    return 0;
  }
  for (int i = 0; i < 3; ++i)
    if (st[i] < 0 || (st[i] & 7) != 0 || st[i] > (1ll << 40))
      return api_fail_value(MI355FA_ERR_STRIDE,
                            q ? "%s: q_strides must be non-negative multiples of 8 elements (got %lld)"
                              : "%s: o_strides must be non-negative multiples of 8 elements (got %lld)", fn, st[i]);
  if (st[2] < width || ((long long)S - 1) * st[2] * 2 + 2ll * width > (1ll << 31) - 1)
    return api_fail_value(MI355FA_ERR_STRIDE,
                          q ? "%s: the row stride of q must be at least 576 elements, one (batch, head) slice below 2^31 bytes (got %lld)"
                            : "%s: the row stride of o must be at least 512 elements, one (batch, head) slice below 2^31 bytes (got %lld)",
                          fn, st[2]);
  if (!q && ((B > 1 && st[0] == 0) || (H > 1 && st[1] == 0)))
    return api_fail_value(MI355FA_ERR_STRIDE, "%s: o_strides: an output cannot have a zero batch / head stride (head stride %lld)", fn, st[1]);
  *out = fa::TensorLayout{st[0] * 2, st[1] * 2, (int)(st[2] * 2)};
  return 0;
}

bool misaligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace

extern "C" {

long long fa_fwd_kvcache_mla_sparse_fp8_workspace_bytes(int B, int H, int S_q, int topk, int max_pages_per_seq, int page_size, int S_new) {
  int S_cache = 0, nsplit = 1;
  if (int rc = gather_shape("fa_fwd_kvcache_mla_sparse_fp8_workspace_bytes", B, H, S_q, topk, max_pages_per_seq, page_size, S_new,
                            &S_cache, &nsplit))
    return rc;
  return fa::kvcache_ws_bytes(nsplit, B, H, S_q, fa::kMlaDv);
}

int fa_fwd_kvcache_mla_sparse_fp8(const void* q, void* kv_pool, const void* kv_new, const int* indices, const int* cache_seqlens,
                                  const int* block_table, void* o, float* lse, void* workspace, long long workspace_bytes, int B,
                                  int H, int S_q, int topk, int num_pages, int page_size, int max_pages_per_seq,
                                  long long block_table_stride, int S_new, int dtype, float scale, int causal,
                                  const long long* q_strides, const long long* kv_strides, const long long* o_strides,
                                  const long long* indices_strides, void* stream) {
  const char* fn = "fa_fwd_kvcache_mla_sparse_fp8";
  if (!q) return api_fail_value(MI355FA_ERR_NULL, "%s: q is NULL (argument %lld)", fn, 1);
  if (!kv_pool) return api_fail_value(MI355FA_ERR_NULL, "%s: kv_pool is NULL (argument %lld)", fn, 2);
  if (!indices) return api_fail_value(MI355FA_ERR_NULL, "%s: indices is NULL (argument %lld)", fn, 4);
  if (!cache_seqlens) return api_fail_value(MI355FA_ERR_NULL, "%s: cache_seqlens is NULL (argument %lld)", fn, 5);
  if (!block_table) return api_fail_value(MI355FA_ERR_NULL, "%s: block_table is NULL (argument %lld)", fn, 6);
  if (!o) return api_fail_value(MI355FA_ERR_NULL, "%s: o is NULL (argument %lld)", fn, 7);
  if (!kv_new && S_new > 0) return api_fail_value(MI355FA_ERR_NULL, "%s: S_new > 0 needs kv_new (S_new %lld)", fn, S_new);
  if (kv_new && S_new < 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: kv_new given with S_new < 1 (S_new %lld)", fn, S_new);
  if (dtype != MI355FA_FP16 && dtype != MI355FA_BF16)
    return api_fail_value(MI355FA_ERR_DTYPE, "%s: dtype must be 0 (fp16) or 1 (bf16), the type of q, o, kv_new and the RoPE values (got %lld)",
                          fn, dtype);
  if (causal != 0 && causal != 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: causal must be 0 or 1 (got %lld)", fn, causal);
  // the scale: finite and > 0, tested on the bits (this file is built with -fno-honor-nans)
  uint32_t u;
  memcpy(&u, &scale, sizeof(u));
  if ((u >> 31) != 0 || (u & 0x7fffffffu) == 0 || ((u >> 23) & 0xffu) == 0xffu)
    return api_fail_value(MI355FA_ERR_SHAPE, "%s: scale must be finite and > 0 (its bits are %lld)", fn, (long long)u);
  int S_cache = 0, nsplit = 1;
  if (int rc = gather_shape(fn, B, H, S_q, topk, max_pages_per_seq, page_size, S_new, &S_cache, &nsplit)) return rc;
  if (num_pages < 1) return api_fail_value(MI355FA_ERR_PAGED, "%s: num_pages must be >= 1 (got %lld)", fn, num_pages);
  if (block_table_stride < (long long)max_pages_per_seq || block_table_stride > 0x7fffffffLL)
    return api_fail_value(MI355FA_ERR_PAGED, "%s: block_table_stride must be at least max_pages_per_seq and below 2^31 (got %lld)", fn,
                          block_table_stride);
  fa::GatherF8Params gp{};
  fa::Fp8RowParams& p = gp.f;
  if (int rc = gather_layout(fn, true, q_strides, B, H, S_q, fa::kMlaD, &p.lq)) return rc;
  if (int rc = gather_layout(fn, false, o_strides, B, H, S_q, fa::kMlaDv, &p.lo)) return rc;
  long long kv_ps = (long long)page_size * fa::kFp8RowB, kv_rs = fa::kFp8RowB;   // bytes
  if (kv_strides) {
    kv_ps = kv_strides[0], kv_rs = kv_strides[1];
    if (kv_ps < 0 || (kv_ps & 15) != 0 || kv_ps > (1ll << 41))
      return api_fail_value(MI355FA_ERR_STRIDE, "%s: the page stride of kv_pool must be a non-negative multiple of 16 bytes (got %lld)", fn,
                            kv_ps);
    if (kv_rs < fa::kFp8RowB || (kv_rs & 15) != 0)
      return api_fail_value(MI355FA_ERR_STRIDE, "%s: the row stride of kv_pool must be a multiple of 16 bytes and at least 656 (got %lld)", fn,
                            kv_rs);
  }
  if (((long long)page_size - 1) * kv_rs + fa::kFp8RowB > (1ll << 31) - 1)
    return api_fail_value(MI355FA_ERR_STRIDE, "%s: one page of kv_pool exceeds 2^31 bytes (row stride %lld bytes)", fn, kv_rs);
  long long idx_sb = (long long)S_q * topk, idx_ss = topk;   // elements
  if (indices_strides) {
    idx_sb = indices_strides[0], idx_ss = indices_strides[1];
    for (long long v : {idx_sb, idx_ss})
      if (v < 0 || v > (1ll << 40))
        return api_fail_value(MI355FA_ERR_STRIDE, "%s: indices_strides must be non-negative and at most 2^40 elements (got %lld)", fn, v);
  }
  if (misaligned(q, 16)) return api_fail_value(MI355FA_ERR_ALIGN, "%s: q must be 16-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)q & 15));
  if (misaligned(kv_pool, 16))
    return api_fail_value(MI355FA_ERR_ALIGN, "%s: kv_pool must be 16-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)kv_pool & 15));
  if (misaligned(kv_new, 16))
    return api_fail_value(MI355FA_ERR_ALIGN, "%s: kv_new must be 16-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)kv_new & 15));
  if (misaligned(o, 16)) return api_fail_value(MI355FA_ERR_ALIGN, "%s: o must be 16-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)o & 15));
  if (misaligned(workspace, 16))
    return api_fail_value(MI355FA_ERR_ALIGN, "%s: workspace must be 16-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)workspace & 15));
  if (misaligned(lse, 4)) return api_fail_value(MI355FA_ERR_ALIGN, "%s: lse must be 4-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)lse & 3));
  if (misaligned(indices, 4))
    return api_fail_value(MI355FA_ERR_ALIGN, "%s: indices must be 4-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)indices & 3));
  if (misaligned(cache_seqlens, 4))
    return api_fail_value(MI355FA_ERR_ALIGN, "%s: cache_seqlens must be 4-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)cache_seqlens & 3));
  if (misaligned(block_table, 4))
    return api_fail_value(MI355FA_ERR_ALIGN, "%s: block_table must be 4-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)block_table & 3));
  const long long need = fa::kvcache_ws_bytes(nsplit, B, H, S_q, fa::kMlaDv);
  if (need > 0 && (!workspace || workspace_bytes < need))
    return api_fail_value(MI355FA_ERR_WORKSPACE, "%s: workspace smaller than fa_fwd_kvcache_mla_sparse_fp8_workspace_bytes() (%lld bytes)", fn,
                          need);
  p.q = q;
  p.kv = kv_pool;
  p.kv_new = kv_new;
  p.seqlens = cache_seqlens;
  p.table = block_table;
  p.o = o;
  p.lse = lse;
  p.ws = (float*)workspace;
  p.kv_ps = kv_ps;
  p.kv_rs = (int)kv_rs;
  p.B = B;
  p.H = H;
  p.Sq = S_q;
  p.Scache = S_cache;
  p.Snew = S_new;
  p.bt_stride = (int)block_table_stride;
  p.page_size = page_size;
  p.num_pages = num_pages;
  p.tpp = fa::make_fastdiv(page_size / 32);
  p.scale = scale;
  p.causal = causal;
  p.nsplit = nsplit;
  gp.indices = indices;
  gp.idx_sb = idx_sb;
  gp.idx_ss = idx_ss;
  gp.topk = topk;
  gp.pdiv = fa::make_fastdiv(page_size);
  if (hipError_t e = fa::launch_decode_mla_sparse_fp8(gp, dtype, (hipStream_t)stream))
    return api_fail_value((int)e, "%s: the launch failed (HIP error %lld)", fn, (long long)e);
  return 0;
}

}  // extern "C"
