// Split-KV decoding attention over a padded or paged KV cache (fa_decode.hip; C ABI in include/mi355fa_kvcache.h and
// include/mi355fa_paged.h): the parameter
// block the three decode kernels share and the host-side launcher.  Internal to libmi355fa.so.
#pragma once
#include <hip/hip_runtime.h>

#include "fa_kernels.h"

namespace fa {

// Q / O: [B, H, S_q, D] (lq / lo); the caches: [B, H_kv, S_cache, D] (lk / lv, one row stride); k_new / v_new:
// contiguous [B, H_kv, S_new, D]; seqlens: device int32 [B].  Sequence b attends to L_b = seqlens[b] + S_new keys, the
// query i of it sits at position L_b - S_q + i (bottom-right aligned), wl / wr >= 0 (unbounded = kWindowUnbounded).
// nsplit > 1: the attention kernel leaves per-split partials in `ws` (layout: kvcache_ws_bytes below) for the combine
// kernel; nsplit == 1: it writes O and LSE itself.  lse may be null.
struct DecodeParams {
  const void* q;
  void* kc;
  void* vc;
  const void* k_new;
  const void* v_new;
  const int* seqlens;
  void* o;
  float* lse;
  float* ws;
  TensorLayout lq, lk, lv, lo;
  int B, H, Hkv, group, Sq, Scache, Snew, D;
  float scale;
  int wl, wr;
  int nsplit;
};

// The split count of a launch (0 = the formula) and the workspace it needs: nsplit * B * H * S_q * (D + 2) * 4 bytes
// when nsplit > 1 (partial O in fp32, then (m, l) pairs), 0 otherwise.
int kvcache_splits(int B, int H_kv, int group, int S_q, int S_cache, int D, int forced);
inline long long kvcache_ws_bytes(int nsplit, int B, int H, int S_q, int D) {
  return nsplit > 1 ? (long long)nsplit * B * H * S_q * (D + 2) * 4 : 0;
}
// A paged cache (include/mi355fa_paged.h): p.kc / p.vc are pools [num_pages, H_kv, page_size, D] (lk / lv: page, head and row
// strides), key j of sequence b is row j % page_size of page table[b * stride + j / page_size], and p.Scache =
// max_pages_per_seq * page_size.  page_size is a multiple of the kernels' 32-key tile, so a tile lies in one page; `tpp`
// divides a tile index by the tiles per page.
struct DecodePaging {
  const int* table;   // device int32 [B, stride]
  int stride;
  int page_size;
  int num_pages;
  FastDiv tpp;
};

// Enqueue the append (when S_new > 0), the attention kernel and (nsplit > 1) the combine kernel on `s`.  softcap > 0:
// the soft-capped attention kernel (include/mi355fa_softcap.h); slopes != NULL: the ALiBi kernel (include/mi355fa_alibi.h,
// slope of query head h of sequence b at slopes[b * sbs + h]); sinks != NULL: the sink kernel (include/mi355fa_sink.h, one
// fp32 logit per query head); none of them: the plain one.  pg != NULL: the paged forms of the append and of the attention
// kernel.
hipError_t launch_decode(const DecodeParams& p, int dtype, hipStream_t s, float softcap = 0.f, const float* slopes = nullptr,
                         int sbs = 0, const float* sinks = nullptr, const DecodePaging* pg = nullptr);

// FP8 (OCP e4m3) caches, include/mi355fa_kvcache_fp8.h: p.kc / p.vc hold bytes (lk / lv strides in bytes, rows of D
// bytes), q / o / k_new / v_new are `dtype`.  kds / vds: the dequantisation factor of K / V head hk of sequence b at
// [b * dbs + hk], NULL = 1.  The append quantises; the combine kernel is the 16-bit one.
int kvcache_fp8_splits(int B, int H_kv, int group, int S_q, int S_cache, int D, int forced);
hipError_t launch_decode_fp8(const DecodeParams& p, int dtype, hipStream_t s, const float* kds, const float* vds, int dbs,
                             const float* sinks = nullptr, const DecodePaging* pg = nullptr);   // sinks, pg: as for launch_decode

}  // namespace fa
