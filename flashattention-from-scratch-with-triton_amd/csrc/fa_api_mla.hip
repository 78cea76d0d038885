// C ABI of the MLA decode family over a paged latent cache: the ten entry points fa_fwd_kvcache_mla{,_ragged,_fp8,_sparse,
// _sparse_fp8} and their _workspace_bytes functions (include_mla*/), their argument checks and their refusal texts, in ONE
// translation unit.  What the five calls check alike stands once, as the file-local functions below; each entry point keeps
// its own sequence of calls, so the order of its checks -- a recorded surface, tests/golden/mla_errors.json -- is its own, and
// where two calls' texts differ by a word both texts stay.  Every error is reported before anything is enqueued, and every text
// names the argument and carries the offending value (fa_last_error() is fa_api.hip's, through api_fail_value).
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include_mla/mi355fa_kvcache_mla.h"
#include "../../include_mla_fp8/mi355fa_kvcache_mla_fp8.h"
#include "../../include_mla_ragged/mi355fa_ragged_mla.h"
#include "../../include_mla_sparse/mi355fa_kvcache_mla_sparse.h"
#include "../../include_mla_sparse_fp8/mi355fa_kvcache_mla_sparse_fp8.h"
#include "fa_decode_mla.h"
#include "fa_decode_mla_fp8.h"
#include "fa_decode_mla_sparse.h"
#include "fa_decode_mla_sparse_fp8.h"
#include "fa_quant_softcap.h"

namespace fa {
extern std::atomic<int> g_force_kvsplits;   // fa_api.hip: fa_debug_kvcache_splits(), 0 = the formula
}

namespace {

using fa::api_fail_value;

int forced_splits() { return fa::g_force_kvsplits.load(std::memory_order_relaxed); }

// The page geometry every form checks alike, behind its own shape bounds.
int page_geometry(const char* fn, int max_pages, int page_size, int* S_cache) {
  if (page_size < 32 || page_size % 32 != 0)
    return api_fail_value(MI355FA_ERR_PAGED, "%s: page_size must be a positive multiple of 32 (got %lld)", fn, page_size);
  if (max_pages < 1) return api_fail_value(MI355FA_ERR_PAGED, "%s: max_pages_per_seq must be >= 1 (got %lld)", fn, max_pages);
  if ((long long)max_pages * page_size > 0x7fffffffLL)
    return api_fail_value(MI355FA_ERR_PAGED, "%s: max_pages_per_seq * page_size must stay below 2^31 (got %lld)", fn,
                          (long long)max_pages * page_size);
  *S_cache = max_pages * page_size;
  return 0;
}

// What a call and its workspace function share: the shape, the page geometry and the launch's split count.  topk 0: the dense
// form, (sequence, 32-row block) workgroups split by the cache's reach; topk >= 1: the top-k form, (sequence, row, 32-head
// block) workgroups split by the list length.
int mla_shape(const char* fn, bool sparse, int B, int H, int S_q, int topk, int max_pages, int page_size, int S_new, int* S_cache,
              int* nsplit) {
  if (B < 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: B must be >= 1 (got %lld)", fn, B);
  if (H < 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: H must be >= 1 (got %lld)", fn, H);
  if (S_q < 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: S_q must be >= 1 (got %lld)", fn, S_q);
  if (S_new < 0) return api_fail_value(MI355FA_ERR_SHAPE, "%s: S_new must be >= 0 (got %lld)", fn, S_new);
  if (sparse && (topk < 1 || topk > (1 << 24)))
    return api_fail_value(MI355FA_ERR_SHAPE, "%s: topk must be in [1, 2^24] (got %lld)", fn, topk);
  if ((long long)H * S_q > (1 << 24))
    return api_fail_value(MI355FA_ERR_SHAPE, "%s: too many query rows for one launch: H * S_q is at most 2^24 (got %lld)", fn,
                          (long long)H * S_q);
  if (int rc = page_geometry(fn, max_pages, page_size, S_cache)) return rc;
  const long long wgs = sparse ? (long long)B * S_q * ((H + 31) / 32) : (long long)B * fa::decode_row_blocks(H, S_q);
  *nsplit = sparse ? fa::mla_sparse_splits(wgs, topk, forced_splits()) : fa::mla_splits(wgs, *S_cache, forced_splits());
  if (wgs * *nsplit > (1ll << 31) - 1 || (long long)B * H * S_q * fa::kMlaDv > (1ll << 40))
    return api_fail_value(MI355FA_ERR_SHAPE,
                          sparse ? "%s: too many workgroups or rows for one launch (B * S_q * head blocks * splits = %lld)"
                                 : "%s: too many workgroups or rows for one launch (B * row blocks * splits = %lld)", fn, wgs * *nsplit);
  return 0;
}

// The packed form: the bound on the step's 32-row blocks as well -- from total_q, B and H alone, never from the lengths.
int packed_shape(const char* fn, int total_q, int B, int H, int max_pages, int page_size, int* S_cache, long long* nb_max,
                 int* nsplit) {
  if (total_q < 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: total_q must be >= 1 (got %lld)", fn, total_q);
  if (B < 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: B must be >= 1 (got %lld)", fn, B);
  if (H < 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: H must be >= 1 (got %lld)", fn, H);
  if ((long long)H * total_q > (1 << 24))
    return api_fail_value(MI355FA_ERR_SHAPE, "%s: too many query rows for one launch: H * total_q is at most 2^24 (got %lld)", fn,
                          (long long)H * total_q);
  if (B > (1 << 24)) return api_fail_value(MI355FA_ERR_SHAPE, "%s: too many sequences for one launch: B is at most 2^24 (got %lld)", fn, B);
  if (int rc = page_geometry(fn, max_pages, page_size, S_cache)) return rc;
  *nb_max = fa::ragged_nb_max(H, total_q, B);
  *nsplit = fa::mla_splits(*nb_max, *S_cache, forced_splits());
  if (*nb_max * *nsplit > (1ll << 31) - 1)
    return api_fail_value(MI355FA_ERR_SHAPE, "%s: too many workgroups for one launch (row blocks * splits = %lld)", fn,
                          *nb_max * *nsplit);
  return 0;
}

// the packed workspace: the plan at the head, the partials of H * total_q rows behind it (fa_fwd_kvcache_ragged's layout)
long long packed_ws_bytes(long long nb_max, int nsplit, int H, int total_q) {
  return fa::ragged_plan_bytes(nb_max) + fa::kvcache_ws_bytes(nsplit, 1, H, total_q, fa::kMlaDv);
}

// Element strides {batch, head, row} of q or o (NULL = contiguous rows of `width`) -> the byte layout.
int mla_layout(const char* fn, bool q, const long long* st, int B, int H, int S, int width, fa::TensorLayout* out) {
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

// the scale: finite and > 0, tested on the bits (this file is built with -fno-honor-nans)
int check_scale(const char* fn, float scale) {
  uint32_t u;
  memcpy(&u, &scale, sizeof(u));
  if ((u >> 31) != 0 || (u & 0x7fffffffu) == 0 || ((u >> 23) & 0xffu) == 0xffu)
    return api_fail_value(MI355FA_ERR_SHAPE, "%s: scale must be finite and > 0 (its bits are %lld)", fn, (long long)u);
  return 0;
}

int check_causal(const char* fn, int causal) {
  if (causal != 0 && causal != 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: causal must be 0 or 1 (got %lld)", fn, causal);
  return 0;
}

// the dtype of q, o and kv_new; over an FP8 pool the text says so
int check_dtype(const char* fn, bool fp8_pool, int dtype) {
  if (dtype != MI355FA_FP16 && dtype != MI355FA_BF16)
    return api_fail_value(MI355FA_ERR_DTYPE,
                          fp8_pool ? "%s: dtype must be 0 (fp16) or 1 (bf16), the type of q, o, kv_new and the RoPE values (got %lld)"
                                   : "%s: dtype must be 0 (fp16) or 1 (bf16) (got %lld)", fn, dtype);
  return 0;
}

int check_new_rows(const char* fn, const void* kv_new, int S_new) {
  if (!kv_new && S_new > 0) return api_fail_value(MI355FA_ERR_NULL, "%s: S_new > 0 needs kv_new (S_new %lld)", fn, S_new);
  if (kv_new && S_new < 1) return api_fail_value(MI355FA_ERR_SHAPE, "%s: kv_new given with S_new < 1 (S_new %lld)", fn, S_new);
  return 0;
}

int check_pool_and_table(const char* fn, int num_pages, int max_pages, long long block_table_stride) {
  if (num_pages < 1) return api_fail_value(MI355FA_ERR_PAGED, "%s: num_pages must be >= 1 (got %lld)", fn, num_pages);
  if (block_table_stride < (long long)max_pages || block_table_stride > 0x7fffffffLL)
    return api_fail_value(MI355FA_ERR_PAGED, "%s: block_table_stride must be at least max_pages_per_seq and below 2^31 (got %lld)", fn,
                          block_table_stride);
  return 0;
}

// {page, row} strides of the pool (NULL = contiguous rows) -> bytes.  The 16-bit pool gives them in elements of 2 bytes, rows of
// at least 576 in multiples of 8; the FP8 pool in bytes, rows of at least 656 in multiples of 16.
int pool_strides(const char* fn, bool fp8_pool, const long long* st, int page_size, long long* ps_bytes, int* rs_bytes) {
  const int unit = fp8_pool ? 1 : 2, row = fp8_pool ? fa::kFp8RowB : fa::kMlaD, mask = 16 / unit - 1;
  long long ps = (long long)page_size * row, rs = row;
  if (st) {
    ps = st[0], rs = st[1];
    if (ps < 0 || (ps & mask) != 0 || ps > (1ll << 41) / unit)
      return api_fail_value(MI355FA_ERR_STRIDE,
                            fp8_pool ? "%s: the page stride of kv_pool must be a non-negative multiple of 16 bytes (got %lld)"
                                     : "%s: the page stride of kv_pool must be a non-negative multiple of 8 elements (got %lld)", fn, ps);
    if (rs < row || (rs & mask) != 0)
      return api_fail_value(MI355FA_ERR_STRIDE,
                            fp8_pool ? "%s: the row stride of kv_pool must be a multiple of 16 bytes and at least 656 (got %lld)"
                                     : "%s: the row stride of kv_pool must be a multiple of 8 elements (16-byte rows) and at least 576 (got %lld)",
                            fn, rs);
  }
  if (((long long)page_size - 1) * rs * unit + row * unit > (1ll << 31) - 1)
    return api_fail_value(MI355FA_ERR_STRIDE,
                          fp8_pool ? "%s: one page of kv_pool exceeds 2^31 bytes (row stride %lld bytes)"
                                   : "%s: one page of kv_pool exceeds 2^31 bytes (row stride %lld elements)", fn, rs);
  *ps_bytes = ps * unit;
  *rs_bytes = (int)(rs * unit);
  return 0;
}

// {batch, row} element strides of the index lists (NULL = contiguous)
int index_strides(const char* fn, const long long* st, int S_q, int topk, long long* sb, long long* ss) {
  *sb = (long long)S_q * topk, *ss = topk;
  if (st) {
    *sb = st[0], *ss = st[1];
    for (long long v : {*sb, *ss})
      if (v < 0 || v > (1ll << 40))
        return api_fail_value(MI355FA_ERR_STRIDE, "%s: indices_strides must be non-negative and at most 2^40 elements (got %lld)", fn, v);
  }
  return 0;
}

bool misaligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// the base addresses: the 16-byte ones, lse, then the int vectors; list_text: the line of cu_seqlens_q or indices (NULL: the
// call has neither)
int check_alignment(const char* fn, const void* q, const void* kv_pool, const void* kv_new, const void* o, const void* workspace,
                    const void* lse, const char* list_text, const void* list, const void* cache_seqlens, const void* block_table) {
  const struct {
    const char* text;
    const void* p;
    unsigned a;
  } rows[] = {{"%s: q must be 16-byte aligned (ends in %lld)", q, 16},
              {"%s: kv_pool must be 16-byte aligned (ends in %lld)", kv_pool, 16},
              {"%s: kv_new must be 16-byte aligned (ends in %lld)", kv_new, 16},
              {"%s: o must be 16-byte aligned (ends in %lld)", o, 16},
              {"%s: workspace must be 16-byte aligned (ends in %lld)", workspace, 16},
              {"%s: lse must be 4-byte aligned (ends in %lld)", lse, 4},
              {list_text, list_text ? list : nullptr, 4},
              {"%s: cache_seqlens must be 4-byte aligned (ends in %lld)", cache_seqlens, 4},
              {"%s: block_table must be 4-byte aligned (ends in %lld)", block_table, 4}};
  for (const auto& r : rows)
    if (misaligned(r.p, r.a)) return api_fail_value(MI355FA_ERR_ALIGN, r.text, fn, (long long)((uintptr_t)r.p & (r.a - 1)));
  return 0;
}

// `need` bytes (0: none) against what the caller brought; text: the call's own, which names its workspace function
int check_workspace(const char* fn, const char* text, long long need, const void* workspace, long long workspace_bytes) {
  return need > 0 && (!workspace || workspace_bytes < need) ? api_fail_value(MI355FA_ERR_WORKSPACE, text, fn, need) : 0;
}

// The fields MlaParams, Fp8RowParams and LatentRaggedParams name alike (TopkParams::m and GatherF8Params::f hold one of them).
template <class P>
void fill(P& p, const void* q, void* kv_pool, const void* kv_new, const int* cache_seqlens, const int* block_table, void* o,
          float* lse, float* ws, long long kv_ps, int kv_rs, int B, int H, int S_q, int S_cache, int S_new,
          long long block_table_stride, int page_size, int num_pages, float scale, int causal, int nsplit) {
  p.q = q;
  p.kv = kv_pool;
  p.kv_new = kv_new;
  p.seqlens = cache_seqlens;
  p.table = block_table;
  p.o = o;
  p.lse = lse;
  p.ws = ws;
  p.kv_ps = kv_ps;
  p.kv_rs = kv_rs;
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
}

int launch_failed(const char* fn, hipError_t e) {
  return e ? api_fail_value((int)e, "%s: the launch failed (HIP error %lld)", fn, (long long)e) : 0;
}

// The dense call over either pool: fa_fwd_kvcache_mla (MlaParams) and fa_fwd_kvcache_mla_fp8 (Fp8RowParams).
template <class P, class Launch>
int dense_call(const char* fn, const char* ws_text, bool fp8_pool, Launch launch, const void* q, void* kv_pool, const void* kv_new,
               const int* cache_seqlens, const int* block_table, void* o, float* lse, void* workspace, long long workspace_bytes,
               int B, int H, int S_q, int num_pages, int page_size, int max_pages_per_seq, long long block_table_stride, int S_new,
               int dtype, float scale, int causal, const long long* q_strides, const long long* kv_strides,
               const long long* o_strides, void* stream) {
  if (!q) return api_fail_value(MI355FA_ERR_NULL, "%s: q is NULL (argument %lld)", fn, 1);
  if (!kv_pool) return api_fail_value(MI355FA_ERR_NULL, "%s: kv_pool is NULL (argument %lld)", fn, 2);
  if (!cache_seqlens) return api_fail_value(MI355FA_ERR_NULL, "%s: cache_seqlens is NULL (argument %lld)", fn, 4);
  if (!block_table) return api_fail_value(MI355FA_ERR_NULL, "%s: block_table is NULL (argument %lld)", fn, 5);
  if (!o) return api_fail_value(MI355FA_ERR_NULL, "%s: o is NULL (argument %lld)", fn, 6);
  if (int rc = check_new_rows(fn, kv_new, S_new)) return rc;
  if (int rc = check_dtype(fn, fp8_pool, dtype)) return rc;
  if (int rc = check_causal(fn, causal)) return rc;
  if (int rc = check_scale(fn, scale)) return rc;
  int S_cache = 0, nsplit = 1, kv_rs = 0;
  long long kv_ps = 0;
  if (int rc = mla_shape(fn, false, B, H, S_q, 0, max_pages_per_seq, page_size, S_new, &S_cache, &nsplit)) return rc;
  if (int rc = check_pool_and_table(fn, num_pages, max_pages_per_seq, block_table_stride)) return rc;
  P p{};
  if (int rc = mla_layout(fn, true, q_strides, B, H, S_q, fa::kMlaD, &p.lq)) return rc;
  if (int rc = mla_layout(fn, false, o_strides, B, H, S_q, fa::kMlaDv, &p.lo)) return rc;
  if (int rc = pool_strides(fn, fp8_pool, kv_strides, page_size, &kv_ps, &kv_rs)) return rc;
  if (int rc = check_alignment(fn, q, kv_pool, kv_new, o, workspace, lse, nullptr, nullptr, cache_seqlens, block_table)) return rc;
  if (int rc = check_workspace(fn, ws_text, fa::kvcache_ws_bytes(nsplit, B, H, S_q, fa::kMlaDv), workspace, workspace_bytes)) return rc;
  fill(p, q, kv_pool, kv_new, cache_seqlens, block_table, o, lse, (float*)workspace, kv_ps, kv_rs, B, H, S_q, S_cache, S_new,
       block_table_stride, page_size, num_pages, scale, causal, nsplit);
  return launch_failed(fn, launch(p, dtype, (hipStream_t)stream));
}

// The top-k call over either pool: fa_fwd_kvcache_mla_sparse (TopkParams, its MlaParams m) and fa_fwd_kvcache_mla_sparse_fp8
// (GatherF8Params, its Fp8RowParams f).
template <class T, class P, class Launch>
int sparse_call(const char* fn, const char* ws_text, bool fp8_pool, T& tp, P& p, Launch launch, const void* q, void* kv_pool,
                const void* kv_new, const int* indices, const int* cache_seqlens, const int* block_table, void* o, float* lse,
                void* workspace, long long workspace_bytes, int B, int H, int S_q, int topk, int num_pages, int page_size,
                int max_pages_per_seq, long long block_table_stride, int S_new, int dtype, float scale, int causal,
                const long long* q_strides, const long long* kv_strides, const long long* o_strides,
                const long long* indices_strides, void* stream) {
  if (!q) return api_fail_value(MI355FA_ERR_NULL, "%s: q is NULL (argument %lld)", fn, 1);
  if (!kv_pool) return api_fail_value(MI355FA_ERR_NULL, "%s: kv_pool is NULL (argument %lld)", fn, 2);
  if (!indices) return api_fail_value(MI355FA_ERR_NULL, "%s: indices is NULL (argument %lld)", fn, 4);
  if (!cache_seqlens) return api_fail_value(MI355FA_ERR_NULL, "%s: cache_seqlens is NULL (argument %lld)", fn, 5);
  if (!block_table) return api_fail_value(MI355FA_ERR_NULL, "%s: block_table is NULL (argument %lld)", fn, 6);
  if (!o) return api_fail_value(MI355FA_ERR_NULL, "%s: o is NULL (argument %lld)", fn, 7);
  if (int rc = check_new_rows(fn, kv_new, S_new)) return rc;
  if (int rc = check_dtype(fn, fp8_pool, dtype)) return rc;
  if (int rc = check_causal(fn, causal)) return rc;
  if (int rc = check_scale(fn, scale)) return rc;
  int S_cache = 0, nsplit = 1, kv_rs = 0;
  long long kv_ps = 0;
  if (int rc = mla_shape(fn, true, B, H, S_q, topk, max_pages_per_seq, page_size, S_new, &S_cache, &nsplit)) return rc;
  if (int rc = check_pool_and_table(fn, num_pages, max_pages_per_seq, block_table_stride)) return rc;
  if (int rc = mla_layout(fn, true, q_strides, B, H, S_q, fa::kMlaD, &p.lq)) return rc;
  if (int rc = mla_layout(fn, false, o_strides, B, H, S_q, fa::kMlaDv, &p.lo)) return rc;
  if (int rc = pool_strides(fn, fp8_pool, kv_strides, page_size, &kv_ps, &kv_rs)) return rc;
  if (int rc = index_strides(fn, indices_strides, S_q, topk, &tp.idx_sb, &tp.idx_ss)) return rc;
  if (int rc = check_alignment(fn, q, kv_pool, kv_new, o, workspace, lse, "%s: indices must be 4-byte aligned (ends in %lld)", indices, cache_seqlens, block_table)) return rc;
  if (int rc = check_workspace(fn, ws_text, fa::kvcache_ws_bytes(nsplit, B, H, S_q, fa::kMlaDv), workspace, workspace_bytes)) return rc;
  fill(p, q, kv_pool, kv_new, cache_seqlens, block_table, o, lse, (float*)workspace, kv_ps, kv_rs, B, H, S_q, S_cache, S_new,
       block_table_stride, page_size, num_pages, scale, causal, nsplit);
  tp.indices = indices;
  tp.topk = topk;
  tp.pdiv = fa::make_fastdiv(page_size);
  return launch_failed(fn, launch(tp, dtype, (hipStream_t)stream));
}

}  // namespace

extern "C" {

// ---- include_mla/mi355fa_kvcache_mla.h ------------------------------------------------------------------------------------------
long long fa_fwd_kvcache_mla_workspace_bytes(int B, int H, int S_q, int max_pages_per_seq, int page_size, int S_new) {
  int S_cache = 0, nsplit = 1;
  if (int rc = mla_shape("fa_fwd_kvcache_mla_workspace_bytes", false, B, H, S_q, 0, max_pages_per_seq, page_size, S_new, &S_cache, &nsplit))
    return rc;
  return fa::kvcache_ws_bytes(nsplit, B, H, S_q, fa::kMlaDv);
}

int fa_fwd_kvcache_mla(const void* q, void* kv_pool, const void* kv_new, const int* cache_seqlens, const int* block_table,
                       void* o, float* lse, void* workspace, long long workspace_bytes, int B, int H, int S_q, int num_pages,
                       int page_size, int max_pages_per_seq, long long block_table_stride, int S_new, int dtype, float scale,
                       int causal, const long long* q_strides, const long long* kv_strides, const long long* o_strides,
                       void* stream) {
  return dense_call<fa::MlaParams>("fa_fwd_kvcache_mla", "%s: workspace smaller than fa_fwd_kvcache_mla_workspace_bytes() (%lld bytes)", false, fa::launch_decode_mla, q, kv_pool,
                                   kv_new, cache_seqlens, block_table, o, lse, workspace, workspace_bytes, B, H, S_q, num_pages,
                                   page_size, max_pages_per_seq, block_table_stride, S_new, dtype, scale, causal, q_strides, kv_strides,
                                   o_strides, stream);
}

// ---- include_mla_fp8/mi355fa_kvcache_mla_fp8.h: the pool holds 656-byte rows, kv_strides are byte strides ----------------------------
long long fa_fwd_kvcache_mla_fp8_workspace_bytes(int B, int H, int S_q, int max_pages_per_seq, int page_size, int S_new) {
  int S_cache = 0, nsplit = 1;
  if (int rc = mla_shape("fa_fwd_kvcache_mla_fp8_workspace_bytes", false, B, H, S_q, 0, max_pages_per_seq, page_size, S_new, &S_cache,
                         &nsplit))
    return rc;
  return fa::kvcache_ws_bytes(nsplit, B, H, S_q, fa::kMlaDv);
}

int fa_fwd_kvcache_mla_fp8(const void* q, void* kv_pool, const void* kv_new, const int* cache_seqlens, const int* block_table,
                           void* o, float* lse, void* workspace, long long workspace_bytes, int B, int H, int S_q, int num_pages,
                           int page_size, int max_pages_per_seq, long long block_table_stride, int S_new, int dtype, float scale,
                           int causal, const long long* q_strides, const long long* kv_strides, const long long* o_strides,
                           void* stream) {
  return dense_call<fa::Fp8RowParams>("fa_fwd_kvcache_mla_fp8", "%s: workspace smaller than fa_fwd_kvcache_mla_fp8_workspace_bytes() (%lld bytes)", true, fa::launch_decode_mla_fp8,
                                      q, kv_pool, kv_new, cache_seqlens, block_table, o, lse, workspace, workspace_bytes, B, H, S_q,
                                      num_pages, page_size, max_pages_per_seq, block_table_stride, S_new, dtype, scale, causal, q_strides,
                                      kv_strides, o_strides, stream);
}

// ---- include_mla_sparse/mi355fa_kvcache_mla_sparse.h: top-k index lists beside the table ----------------------------------------------
long long fa_fwd_kvcache_mla_sparse_workspace_bytes(int B, int H, int S_q, int topk, int max_pages_per_seq, int page_size, int S_new) {
  int S_cache = 0, nsplit = 1;
  if (int rc = mla_shape("fa_fwd_kvcache_mla_sparse_workspace_bytes", true, B, H, S_q, topk, max_pages_per_seq, page_size, S_new, &S_cache,
                         &nsplit))
    return rc;
  return fa::kvcache_ws_bytes(nsplit, B, H, S_q, fa::kMlaDv);
}

int fa_fwd_kvcache_mla_sparse(const void* q, void* kv_pool, const void* kv_new, const int* indices, const int* cache_seqlens,
                              const int* block_table, void* o, float* lse, void* workspace, long long workspace_bytes, int B, int H,
                              int S_q, int topk, int num_pages, int page_size, int max_pages_per_seq, long long block_table_stride,
                              int S_new, int dtype, float scale, int causal, const long long* q_strides,
                              const long long* kv_strides, const long long* o_strides, const long long* indices_strides,
                              void* stream) {
  fa::TopkParams tp{};
  return sparse_call("fa_fwd_kvcache_mla_sparse", "%s: workspace smaller than fa_fwd_kvcache_mla_sparse_workspace_bytes() (%lld bytes)", false, tp, tp.m, fa::launch_decode_mla_sparse,
                     q, kv_pool, kv_new, indices, cache_seqlens, block_table, o, lse, workspace, workspace_bytes, B, H, S_q, topk,
                     num_pages, page_size, max_pages_per_seq, block_table_stride, S_new, dtype, scale, causal, q_strides, kv_strides,
                     o_strides, indices_strides, stream);
}

// ---- include_mla_sparse_fp8/mi355fa_kvcache_mla_sparse_fp8.h: the same over the FP8 pool ----------------------------------------------
long long fa_fwd_kvcache_mla_sparse_fp8_workspace_bytes(int B, int H, int S_q, int topk, int max_pages_per_seq, int page_size, int S_new) {
  int S_cache = 0, nsplit = 1;
  if (int rc = mla_shape("fa_fwd_kvcache_mla_sparse_fp8_workspace_bytes", true, B, H, S_q, topk, max_pages_per_seq, page_size, S_new,
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
  fa::GatherF8Params gp{};
  return sparse_call("fa_fwd_kvcache_mla_sparse_fp8", "%s: workspace smaller than fa_fwd_kvcache_mla_sparse_fp8_workspace_bytes() (%lld bytes)", true, gp, gp.f,
                     fa::launch_decode_mla_sparse_fp8, q, kv_pool, kv_new, indices, cache_seqlens, block_table, o, lse, workspace,
                     workspace_bytes, B, H, S_q, topk, num_pages, page_size, max_pages_per_seq, block_table_stride, S_new, dtype, scale,
                     causal, q_strides, kv_strides, o_strides, indices_strides, stream);
}

// ---- include_mla_ragged/mi355fa_ragged_mla.h: packed variable-length queries, its own shape, layout and workspace ------------------
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
  if (int rc = check_dtype(fn, false, dtype)) return rc;
  if (int rc = check_causal(fn, causal)) return rc;
  if (int rc = check_scale(fn, scale)) return rc;
  int S_cache = 0, nsplit = 1, kv_rs = 0;
  long long nb_max = 0, kv_ps = 0;
  if (int rc = packed_shape(fn, total_q, B, H, max_pages_per_seq, page_size, &S_cache, &nb_max, &nsplit)) return rc;
  if (int rc = check_pool_and_table(fn, num_pages, max_pages_per_seq, block_table_stride)) return rc;
  fa::LatentRaggedParams p{};
  if (int rc = packed_layout(fn, true, q_strides, H, fa::kMlaD, &p.lq)) return rc;
  if (int rc = packed_layout(fn, false, o_strides, H, fa::kMlaDv, &p.lo)) return rc;
  if (int rc = pool_strides(fn, false, kv_strides, page_size, &kv_ps, &kv_rs)) return rc;
  if (int rc = check_alignment(fn, q, kv_pool, kv_new, o, workspace, lse, "%s: cu_seqlens_q must be 4-byte aligned (ends in %lld)",
                               cu_seqlens_q, cache_seqlens, block_table))
    return rc;
  // never 0 bytes: the plan
  if (int rc = check_workspace(fn, "%s: workspace smaller than fa_fwd_kvcache_mla_ragged_workspace_bytes() (%lld bytes)", packed_ws_bytes(nb_max, nsplit, H, total_q), workspace,
                               workspace_bytes))
    return rc;
  fill(p, q, kv_pool, kv_new, cache_seqlens, block_table, o, lse, (float*)((char*)workspace + fa::ragged_plan_bytes(nb_max)), kv_ps,
       kv_rs, B, H, 0, S_cache, has_new, block_table_stride, page_size, num_pages, scale, causal, nsplit);
  p.plan = (int*)workspace;
  p.cu_q = cu_seqlens_q;
  p.total_q = total_q;
  p.nb_max = (int)nb_max;
  return launch_failed(fn, fa::launch_decode_mla_ragged(p, dtype, (hipStream_t)stream));
}

}  // extern "C"
