// C ABI of MLA decoding over a paged latent cache with packed variable-length queries (include_mla_ragged/mi355fa_ragged_mla.h):
// the two entry points, their argument checks and their refusal texts -- a translation unit of its own beside fa_api_mla.hip,
// whose texts are a recorded set, and in its style: every text names the argument and carries the offending value
// (fa_last_error() is fa_api.hip's, through api_fail_value).
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include_mla_ragged/mi355fa_ragged_mla.h"
#include "fa_decode_mla.h"
#include "fa_quant_softcap.h"

namespace fa {
extern std::atomic<int> g_force_kvsplits;   // fa_api.hip: fa_debug_kvcache_splits(), 0 = the formula
}

namespace {

using fa::api_fail_value;

// What the call and its workspace function share: the shape, the page geometry, the bound on the step's 32-row blocks and the
// launch's split count -- from total_q, B and H alone, never from the lengths.
int packed_shape(const char* fn, int total_q, int B, int H, int max_pages, int page_size, int* S_cache, long long* nb_max,
                 int* nsplit) {
  if (total_q < 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: total_q must be >= 1 (got %lld)", fn, total_q);
  if (B < 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: B must be >= 1 (got %lld)", fn, B);
  if (H < 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: H must be >= 1 (got %lld)", fn, H);
  if ((long long)H * total_q > (1 << 24))
    return api_fail_value(MI355FA_ERR_SHAPE, "%s: too many query rows for one launch: H * total_q is at most 2^24 (got %lld)", fn,
                          (long long)H * total_q);
  if (B > (1 << 24)) return api_fail_value(MI355FA_ERR_SHAPE, "%s: too many sequences for one launch: B is at most 2^24 (got %lld)", fn, B);
  if (page_size < 32 || page_size % 32 != 0)
    return api_fail_value(MI355FA_ERR_PAGED, "%s: page_size must be a positive multiple of 32 (got %lld)", fn, page_size);
  if (max_pages < 1) return api_fail_value(MI355FA_ERR_PAGED, "%s: max_pages_per_seq must be >= 1 (got %lld)", fn, max_pages);
  if ((long long)max_pages * page_size > 0x7fffffffLL)
    return api_fail_value(MI355FA_ERR_PAGED, "%s: max_pages_per_seq * page_size must stay below 2^31 (got %lld)", fn,
                          (long long)max_pages * page_size);
  *S_cache = max_pages * page_size;
  *nb_max = fa::ragged_nb_max(H, total_q, B);
  *nsplit = fa::mla_splits(*nb_max, *S_cache, fa::g_force_kvsplits.load(std::memory_order_relaxed));
  if (*nb_max * *nsplit > (1ll << 31) - 1)
    return api_fail_value(MI355FA_ERR_SHAPE, "%s: too many workgroups for one launch (row blocks * splits = %lld)", fn,
                          *nb_max * *nsplit);
  return 0;
}

// the workspace: the plan at the head, the partials of H * total_q rows behind it (fa_fwd_kvcache_ragged's layout)
long long packed_ws_bytes(long long nb_max, int nsplit, int H, int total_q) {
  return fa::ragged_plan_bytes(nb_max) + fa::kvcache_ws_bytes(nsplit, 1, H, total_q, fa::kMlaDv);
}

// Element strides {row, head} of packed q or o (NULL = contiguous rows of `width`) -> the byte layout.
int packed_layout(const char* fn, bool q, const long long* st, int H, int width, fa::TensorLayout* out) {
  if (!st) {
    *out = fa::TensorLayout{0, (long long)width * 2, H * width * 2};
    return 0;
  }
  for (int i = 0; i < 2; ++i)
    if (st[i] < 0 || (st[i] & 7) != 0 || st[i] >= (1ll << 30))
      return api_fail_value(MI355FA_ERR_STRIDE,
                            q ? "%s: q_strides must be non-negative multiples of 8 elements below 2^30 (got %lld)"
                              : "%s: o_strides must be non-negative multiples of 8 elements below 2^30 (got %lld)", fn, st[i]);
  if (st[0] < width)
    return api_fail_value(MI355FA_ERR_STRIDE,
                          q ? "%s: the row stride of q must be at least 576 elements (got %lld)"
                            : "%s: the row stride of o must be at least 512 elements (got %lld)", fn, st[0]);
  if (!q && H > 1 && st[1] == 0)
    return api_fail_value(MI355FA_ERR_STRIDE, "%s: o_strides: an output cannot have a zero head stride (head stride %lld)", fn, st[1]);
  *out = fa::TensorLayout{0, st[1] * 2, (int)(st[0] * 2)};
  return 0;
}

bool misaligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace

extern "C" {

long long fa_fwd_kvcache_mla_ragged_workspace_bytes(int total_q, int B, int H, int max_pages_per_seq, int page_size) {
  int S_cache = 0, nsplit = 1;
  long long nb_max = 0;
  if (int rc = packed_shape("fa_fwd_kvcache_mla_ragged_workspace_bytes", total_q, B, H, max_pages_per_seq, page_size, &S_cache,
                            &nb_max, &nsplit))
    return rc;
  return packed_ws_bytes(nb_max, nsplit, H, total_q);
}

int fa_fwd_kvcache_mla_ragged(const void* q, void* kv_pool, const void* kv_new, const int* cu_seqlens_q,
                              const int* cache_seqlens, const int* block_table, void* o, float* lse, void* workspace,
                              long long workspace_bytes, int total_q, int B, int H, int num_pages, int page_size,
                              int max_pages_per_seq, long long block_table_stride, int has_new, int dtype, float scale,
                              int causal, const long long* q_strides, const long long* kv_strides, const long long* o_strides,
                              void* stream) {
  const char* fn = "fa_fwd_kvcache_mla_ragged";
  if (!q) return api_fail_value(MI355FA_ERR_NULL, "%s: q is NULL (argument %lld)", fn, 1);
  if (!kv_pool) return api_fail_value(MI355FA_ERR_NULL, "%s: kv_pool is NULL (argument %lld)", fn, 2);
  if (!cu_seqlens_q) return api_fail_value(MI355FA_ERR_NULL, "%s: cu_seqlens_q is NULL (argument %lld)", fn, 4);
  if (!cache_seqlens) return api_fail_value(MI355FA_ERR_NULL, "%s: cache_seqlens is NULL (argument %lld)", fn, 5);
  if (!block_table) return api_fail_value(MI355FA_ERR_NULL, "%s: block_table is NULL (argument %lld)", fn, 6);
  if (!o) return api_fail_value(MI355FA_ERR_NULL, "%s: o is NULL (argument %lld)", fn, 7);
  if (has_new != 0 && has_new != 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: has_new must be 0 or 1 (got %lld)", fn, has_new);
  if (!kv_new && has_new) return api_fail_value(MI355FA_ERR_NULL, "%s: has_new = 1 needs kv_new (has_new %lld)", fn, has_new);
  if (kv_new && !has_new) return api_fail_value(MI355FA_ERR_SHAPE, "%s: kv_new given with has_new = 0 (has_new %lld)", fn, has_new);
  if (dtype != MI355FA_FP16 && dtype != MI355FA_BF16)
    return api_fail_value(MI355FA_ERR_DTYPE, "%s: dtype must be 0 (fp16) or 1 (bf16) (got %lld)", fn, dtype);
  if (causal != 0 && causal != 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: causal must be 0 or 1 (got %lld)", fn, causal);
  // the scale: finite and > 0, tested on the bits (this file is built with -fno-honor-nans)
  uint32_t u;
  memcpy(&u, &scale, sizeof(u));
  if ((u >> 31) != 0 || (u & 0x7fffffffu) == 0 || ((u >> 23) & 0xffu) == 0xffu)
    return api_fail_value(MI355FA_ERR_SHAPE, "%s: scale must be finite and > 0 (its bits are %lld)", fn, (long long)u);
  int S_cache = 0, nsplit = 1;
  long long nb_max = 0;
  if (int rc = packed_shape(fn, total_q, B, H, max_pages_per_seq, page_size, &S_cache, &nb_max, &nsplit)) return rc;
  if (num_pages < 1) return api_fail_value(MI355FA_ERR_PAGED, "%s: num_pages must be >= 1 (got %lld)", fn, num_pages);
  if (block_table_stride < (long long)max_pages_per_seq || block_table_stride > 0x7fffffffLL)
    return api_fail_value(MI355FA_ERR_PAGED, "%s: block_table_stride must be at least max_pages_per_seq and below 2^31 (got %lld)", fn,
                          block_table_stride);
  fa::LatentRaggedParams p{};
  if (int rc = packed_layout(fn, true, q_strides, H, fa::kMlaD, &p.lq)) return rc;
  if (int rc = packed_layout(fn, false, o_strides, H, fa::kMlaDv, &p.lo)) return rc;
  long long kv_ps = (long long)page_size * fa::kMlaD, kv_rs = fa::kMlaD;   // elements
  if (kv_strides) {
    kv_ps = kv_strides[0], kv_rs = kv_strides[1];
    if (kv_ps < 0 || (kv_ps & 7) != 0 || kv_ps > (1ll << 40))
      return api_fail_value(MI355FA_ERR_STRIDE, "%s: the page stride of kv_pool must be a non-negative multiple of 8 elements (got %lld)",
                            fn, kv_ps);
    if (kv_rs < fa::kMlaD || (kv_rs & 7) != 0)
      return api_fail_value(MI355FA_ERR_STRIDE,
                            "%s: the row stride of kv_pool must be a multiple of 8 elements (16-byte rows) and at least 576 (got %lld)", fn,
                            kv_rs);
  }
  if (((long long)page_size - 1) * kv_rs * 2 + fa::kMlaRowB > (1ll << 31) - 1)
    return api_fail_value(MI355FA_ERR_STRIDE, "%s: one page of kv_pool exceeds 2^31 bytes (row stride %lld elements)", fn, kv_rs);
  if (misaligned(q, 16)) return api_fail_value(MI355FA_ERR_ALIGN, "%s: q must be 16-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)q & 15));
  if (misaligned(kv_pool, 16))
    return api_fail_value(MI355FA_ERR_ALIGN, "%s: kv_pool must be 16-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)kv_pool & 15));
  if (misaligned(kv_new, 16))
    return api_fail_value(MI355FA_ERR_ALIGN, "%s: kv_new must be 16-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)kv_new & 15));
  if (misaligned(o, 16)) return api_fail_value(MI355FA_ERR_ALIGN, "%s: o must be 16-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)o & 15));
  if (misaligned(workspace, 16))
    return api_fail_value(MI355FA_ERR_ALIGN, "%s: workspace must be 16-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)workspace & 15));
  if (misaligned(lse, 4)) return api_fail_value(MI355FA_ERR_ALIGN, "%s: lse must be 4-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)lse & 3));
  if (misaligned(cu_seqlens_q, 4))
    return api_fail_value(MI355FA_ERR_ALIGN, "%s: cu_seqlens_q must be 4-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)cu_seqlens_q & 3));
  if (misaligned(cache_seqlens, 4))
    return api_fail_value(MI355FA_ERR_ALIGN, "%s: cache_seqlens must be 4-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)cache_seqlens & 3));
  if (misaligned(block_table, 4))
    return api_fail_value(MI355FA_ERR_ALIGN, "%s: block_table must be 4-byte aligned (ends in %lld)", fn, (long long)((uintptr_t)block_table & 3));
  const long long need = packed_ws_bytes(nb_max, nsplit, H, total_q);   // never 0: the plan
  if (!workspace || workspace_bytes < need)
    return api_fail_value(MI355FA_ERR_WORKSPACE, "%s: workspace smaller than fa_fwd_kvcache_mla_ragged_workspace_bytes() (%lld bytes)", fn, need);
  p.q = q;
  p.kv = kv_pool;
  p.kv_new = kv_new;
  p.seqlens = cache_seqlens;
  p.table = block_table;
  p.o = o;
  p.lse = lse;
  p.plan = (int*)workspace;
  p.ws = (float*)((char*)workspace + fa::ragged_plan_bytes(nb_max));
  p.kv_ps = kv_ps * 2;
  p.kv_rs = (int)(kv_rs * 2);
  p.B = B;
  p.H = H;
  p.Sq = 0;
  p.Scache = S_cache;
  p.Snew = has_new;
  p.bt_stride = (int)block_table_stride;
  p.page_size = page_size;
  p.num_pages = num_pages;
  p.tpp = fa::make_fastdiv(page_size / 32);
  p.scale = scale;
  p.causal = causal;
  p.nsplit = nsplit;
  p.cu_q = cu_seqlens_q;
  p.total_q = total_q;
  p.nb_max = (int)nb_max;
  if (hipError_t e = fa::launch_decode_mla_ragged(p, dtype, (hipStream_t)stream))
    return api_fail_value((int)e, "%s: the launch failed (HIP error %lld)", fn, (long long)e);
  return 0;
}

}  // extern "C"
