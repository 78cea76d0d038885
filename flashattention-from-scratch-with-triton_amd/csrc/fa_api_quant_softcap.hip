// C ABI of soft-capped decoding over the quantised KV caches (include_quant/mi355fa_kvcache_quant_softcap.h): the six entry points and
// the refusals that are theirs alone -- the cache struct, its format, the members of another format, the head dims of a format's
// geometry.  Every such text carries the offending value.  Everything else is checked by the decode calls' shared code and
// launched through their one path (fa_api.hip, behind fa_quant_softcap.h), so a bad stride or pointer is refused here with the
// code and the text it has under the format's own call.
#include "../../include_quant/mi355fa_kvcache_quant_softcap.h"
#include "fa_quant_softcap.h"

namespace {

// The struct of a call -> the launch path's description of it, or the refusal.  `rect`: a padded or paged call.
int read_cache(const char* fn, const mi355fa_quant_cache* c, int D, bool rect, fa::QuantSoftcapCall* out) {
  if (!c) return fa::api_fail_value(MI355FA_ERR_NULL, "%s: the mi355fa_quant_cache struct is NULL (argument %lld from the end)", fn, 3);
  if (c->format != MI355FA_QUANT_E4M3 && c->format != MI355FA_QUANT_E4M3_TOKEN && c->format != MI355FA_QUANT_MXFP4)
    return fa::api_fail_value(MI355FA_ERR_DTYPE,
                              "%s: format must be MI355FA_QUANT_E4M3 (0), MI355FA_QUANT_E4M3_TOKEN (1) or MI355FA_QUANT_MXFP4 (2) (got %lld)",
                              fn, c->format);
  const bool descales = c->k_descale || c->v_descale || c->descale_bstride != 0;
  const bool scales = c->k_scale || c->v_scale || c->k_scale_strides || c->v_scale_strides;
  if (c->format == MI355FA_QUANT_E4M3 && scales)
    return fa::api_fail_value(MI355FA_ERR_SHAPE,
                              "%s: k_scale / v_scale and their strides belong to MI355FA_QUANT_E4M3_TOKEN and MI355FA_QUANT_MXFP4 (format %lld)",
                              fn, c->format);
  if (c->format != MI355FA_QUANT_E4M3 && descales)
    return fa::api_fail_value(MI355FA_ERR_SHAPE,
                              "%s: k_descale / v_descale / descale_bstride belong to MI355FA_QUANT_E4M3 (format %lld)", fn, c->format);
  if (c->format != MI355FA_QUANT_E4M3 && (!c->k_scale || !c->v_scale))
    return fa::api_fail_value(MI355FA_ERR_NULL, "%s: format %lld needs k_scale and v_scale", fn, c->format);
  if (c->format != MI355FA_QUANT_E4M3 && D == 256 && rect)
    return fa::api_fail_value(MI355FA_ERR_SHAPE,
                              c->format == MI355FA_QUANT_MXFP4
                                  ? "%s: an MXFP4 cache takes head dim %lld with packed queries only (fa_fwd_kvcache_quant_softcap_ragged)"
                                  : "%s: a per-token-scaled cache takes head dim %lld with packed queries only (fa_fwd_kvcache_quant_softcap_ragged)",
                              fn, D);
  *out = fa::QuantSoftcapCall{};
  out->fmt = c->format == MI355FA_QUANT_MXFP4        ? fa::KvFormat::kMXFP4
             : c->format == MI355FA_QUANT_E4M3_TOKEN ? fa::KvFormat::kE4M3Token
                                                     : fa::KvFormat::kE4M3;
  out->k_descale = c->k_descale;
  out->v_descale = c->v_descale;
  out->descale_bstride = c->descale_bstride;
  out->k_scale = c->k_scale;
  out->v_scale = c->v_scale;
  out->k_scale_strides = c->k_scale_strides;
  out->v_scale_strides = c->v_scale_strides;
  return 0;
}

// the same for a workspace function, which has the format alone
int read_format(const char* fn, int format, int D, bool rect, fa::KvFormat* fmt) {
  mi355fa_quant_cache c{};
  c.format = format;
  c.k_scale = c.v_scale = &c;   // (present: the workspace of a call does not depend on them)
  if (format == MI355FA_QUANT_E4M3) c.k_scale = c.v_scale = nullptr;
  fa::QuantSoftcapCall q;
  if (int rc = read_cache(fn, &c, D, rect, &q)) return rc;
  *fmt = q.fmt;
  return 0;
}

}  // namespace

extern "C" {

long long fa_fwd_kvcache_quant_softcap_workspace_bytes(int format, int B, int H, int H_kv, int S_q, int S_cache, int S_new, int D) {
  const char* fn = "fa_fwd_kvcache_quant_softcap_workspace_bytes";
  fa::KvFormat fmt;
  if (int rc = read_format(fn, format, D, true, &fmt)) return rc;
  return fa::kvcache_quant_softcap_workspace(fn, fmt, false, false, 0, B, H, H_kv, S_q, S_cache, 0, 0, S_new, D);
}
int fa_fwd_kvcache_quant_softcap(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                                 const int* cache_seqlens, void* o, float* lse, void* workspace, long long workspace_bytes, int B,
                                 int H, int H_kv, int S_q, int S_cache, int S_new, int D, int dtype, float scale, float softcap,
                                 int window_left, int window_right, const mi355fa_quant_cache* cache, const mi355fa_opts* opts,
                                 void* stream) {
  const char* fn = "fa_fwd_kvcache_quant_softcap";
  fa::QuantSoftcapCall c;
  if (int rc = read_cache(fn, cache, D, true, &c)) return rc;
  c.softcap = softcap;
  return fa::kvcache_quant_softcap(fn, q, k_cache, v_cache, k_new, v_new, cache_seqlens, o, lse, workspace, workspace_bytes, B, H,
                                   H_kv, S_q, S_cache, S_new, D, dtype, scale, window_left, window_right, opts, stream, c);
}

long long fa_fwd_kvcache_quant_softcap_paged_workspace_bytes(int format, int B, int H, int H_kv, int S_q, int max_pages_per_seq,
                                                             int page_size, int S_new, int D) {
  const char* fn = "fa_fwd_kvcache_quant_softcap_paged_workspace_bytes";
  fa::KvFormat fmt;
  if (int rc = read_format(fn, format, D, true, &fmt)) return rc;
  return fa::kvcache_quant_softcap_workspace(fn, fmt, true, false, 0, B, H, H_kv, S_q, 0, max_pages_per_seq, page_size, S_new, D);
}
int fa_fwd_kvcache_quant_softcap_paged(const void* q, void* k_pool, void* v_pool, const void* k_new, const void* v_new,
                                       const int* cache_seqlens, const int* block_table, void* o, float* lse, void* workspace,
                                       long long workspace_bytes, int B, int H, int H_kv, int S_q, int num_pages, int page_size,
                                       int max_pages_per_seq, long long block_table_stride, int S_new, int D, int dtype,
                                       float scale, float softcap, int window_left, int window_right,
                                       const mi355fa_quant_cache* cache, const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_fwd_kvcache_quant_softcap_paged";
  fa::QuantSoftcapCall c;
  if (int rc = read_cache(fn, cache, D, true, &c)) return rc;
  c.softcap = softcap;
  c.paged = true;
  c.block_table = block_table;
  c.num_pages = num_pages;
  c.page_size = page_size;
  c.max_pages = max_pages_per_seq;
  c.block_table_stride = block_table_stride;
  return fa::kvcache_quant_softcap(fn, q, k_pool, v_pool, k_new, v_new, cache_seqlens, o, lse, workspace, workspace_bytes, B, H,
                                   H_kv, S_q, 0, S_new, D, dtype, scale, window_left, window_right, opts, stream, c);
}

long long fa_fwd_kvcache_quant_softcap_ragged_workspace_bytes(int format, int total_q, int B, int H, int H_kv,
                                                              int max_pages_per_seq, int page_size, int D) {
  const char* fn = "fa_fwd_kvcache_quant_softcap_ragged_workspace_bytes";
  fa::KvFormat fmt;
  if (int rc = read_format(fn, format, D, false, &fmt)) return rc;
  return fa::kvcache_quant_softcap_workspace(fn, fmt, true, true, total_q, B, H, H_kv, 0, 0, max_pages_per_seq, page_size, 0, D);
}
int fa_fwd_kvcache_quant_softcap_ragged(const void* q, void* k_pool, void* v_pool, const void* k_new, const void* v_new,
                                        const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table, void* o,
                                        float* lse, void* workspace, long long workspace_bytes, int total_q, int B, int H,
                                        int H_kv, int num_pages, int page_size, int max_pages_per_seq,
                                        long long block_table_stride, int D, int dtype, float scale, float softcap,
                                        int window_left, int window_right, const mi355fa_quant_cache* cache,
                                        const mi355fa_opts* opts, void* stream) {
  const char* fn = "fa_fwd_kvcache_quant_softcap_ragged";
  fa::QuantSoftcapCall c;
  if (int rc = read_cache(fn, cache, D, false, &c)) return rc;
  c.softcap = softcap;
  c.paged = c.packed = true;
  c.block_table = block_table;
  c.num_pages = num_pages;
  c.page_size = page_size;
  c.max_pages = max_pages_per_seq;
  c.block_table_stride = block_table_stride;
  c.cu = cu_seqlens_q;
  c.total_q = total_q;
  return fa::kvcache_quant_softcap(fn, q, k_pool, v_pool, k_new, v_new, cache_seqlens, o, lse, workspace, workspace_bytes, B, H,
                                   H_kv, 0, 0, 0, D, dtype, scale, window_left, window_right, opts, stream, c);
}

}  // extern "C"
