// Soft-capped decoding over the quantised KV caches (include_quant/mi355fa_kvcache_quant_softcap.h): what fa_api_quant_softcap.hip, the
// translation unit of those entry points and of their own refusal texts, takes from fa_api.hip -- the decode calls' shared
// checks and launch path behind one function per kind, so that every argument is checked by the code, and refused with the text,
// of the format's own call.  Internal to libmi355fa.so.
#pragma once
#include "../../include/mi355fa.h"
#include "fa_decode.h"

namespace fa {

// One soft-capped call over a quantised cache, its format and the members of that format already checked (the caller): the cache
// format with its descales (kE4M3) or scale tensors (kE4M3Token: fp32, element strides; kMXFP4: bytes), the cap, and the geometry:
// padded (no table), paged (block_table != NULL or `paged`), packed (`packed`: cu / total_q beside the table).
struct QuantSoftcapCall {
  KvFormat fmt;
  float softcap;
  const float *k_descale, *v_descale;
  long long descale_bstride;
  void *k_scale, *v_scale;
  const long long *k_scale_strides, *v_scale_strides;
  bool paged, packed;
  const int* block_table;
  int num_pages, page_size, max_pages;
  long long block_table_stride;
  const int* cu;
  int total_q;
};
// The checks of the format's own call in its order -- packed: cu_seqlens_q, total_q and B; the cap (MI355FA_ERR_SOFTCAP); paged:
// the block table, the page geometry and the table's stride; then everything the decode calls share -- and the launch.
// S_q is ignored by a packed call, S_cache by a paged one (max_pages * page_size), S_new of a packed call is 1 with k_new.
int kvcache_quant_softcap(const char* fn, const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                          const int* cache_seqlens, void* o, float* lse, void* workspace, long long workspace_bytes, int B, int H,
                          int H_kv, int S_q, int S_cache, int S_new, int D, int dtype, float scale, int window_left,
                          int window_right, const mi355fa_opts* opts, void* stream, const QuantSoftcapCall& c);
// The workspace of such a call: what the plain call of the format and the geometry returns (the same checks, the same split rule).
long long kvcache_quant_softcap_workspace(const char* fn, KvFormat fmt, bool paged, bool packed, int total_q, int B, int H,
                                          int H_kv, int S_q, int S_cache, int max_pages, int page_size, int S_new, int D);
// a refusal with a text of the caller's own, which carries the offending value (fa_last_error() is fa_api.hip's)
int api_fail_value(int code, const char* fmt, const char* fn, long long value);

}  // namespace fa
