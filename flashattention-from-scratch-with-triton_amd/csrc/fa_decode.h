// Split-KV decoding attention over a padded or paged KV cache (fa_decode.hip; C ABI in include/mi355fa_kvcache.h,
// include/mi355fa_paged.h and, for packed variable-length queries, include/mi355fa_ragged.h): the parameter
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

// Packed variable-length queries over a paged cache (include/mi355fa_ragged.h): Q / O are [total_q, H, D] (lq / lo: head
// and row strides, no batch stride), sequence b owns the packed rows [cu_q[b], cu_q[b + 1]) -- S_b of them, each end
// clamped into [0, total_q] and the second to the first --, LSE is [H, total_q], the partials are those of H * total_q
// rows, k_new / v_new are [total_q, H_kv, D] (p.Snew != 0: every query row brings its key, L_b = seqlens[b] + S_b) and
// p.Sq is unused.  `plan` is the device-built work list (fa_decode_ragged_plan_kernel): ints {count, rows_end, 0, 0},
// then nb_max pairs (b, rb), one per 32-row block of the step, (-1, 0) from `count` on.  nb_max =
// (group * total_q + 31 * B) / 32 bounds sum_b ceil(group * S_b / 32) whatever the lengths, so the host sizes the grid
// without reading cu_q.
struct DecodeRagged {
  const int* cu_q;   // device int32 [B + 1]
  int total_q;
  int* plan;         // ragged_plan_bytes(nb_max) bytes, 16-byte aligned
  int nb_max;
};
inline long long ragged_nb_max(int group, int total_q, int B) { return ((long long)group * total_q + 31ll * B) / 32; }
inline long long ragged_plan_bytes(long long nb_max) { return (16 + 8 * nb_max + 15) / 16 * 16; }
// the split rules below with B * H_kv * (row blocks) = H_kv * nb_max workgroups per split
int kvcache_ragged_splits(long long nb_max, int H_kv, int S_cache, int D, bool fp8, int forced);
// the plan kernel alone, as launch_decode enqueues it first (tools/ragged_bench.py times it)
hipError_t launch_ragged_plan(const int* cu_q, int B, int group, const DecodeRagged& g, hipStream_t s);

// Enqueue the append (when S_new > 0), the attention kernel and (nsplit > 1) the combine kernel on `s`.  softcap > 0:
// the soft-capped attention kernel (include/mi355fa_softcap.h); slopes != NULL: the ALiBi kernel (include/mi355fa_alibi.h,
// slope of query head h of sequence b at slopes[b * sbs + h]); sinks != NULL: the sink kernel (include/mi355fa_sink.h, one
// fp32 logit per query head); none of them: the plain one.  pg != NULL: the paged forms of the append and of the attention
// kernel.  rg != NULL (with pg): the plan kernel first, then the packed forms of all three.
hipError_t launch_decode(const DecodeParams& p, int dtype, hipStream_t s, float softcap = 0.f, const float* slopes = nullptr,
                         int sbs = 0, const float* sinks = nullptr, const DecodePaging* pg = nullptr,
                         const DecodeRagged* rg = nullptr);

// FP8 (OCP e4m3) caches, include/mi355fa_kvcache_fp8.h: p.kc / p.vc hold bytes (lk / lv strides in bytes, rows of D
// bytes), q / o / k_new / v_new are `dtype`.  kds / vds: the dequantisation factor of K / V head hk of sequence b at
// [b * dbs + hk], NULL = 1.  The append quantises; the combine kernel is the 16-bit one.
int kvcache_fp8_splits(int B, int H_kv, int group, int S_q, int S_cache, int D, int forced);
hipError_t launch_decode_fp8(const DecodeParams& p, int dtype, hipStream_t s, const float* kds, const float* vds, int dbs,
                             const float* sinks = nullptr, const DecodePaging* pg = nullptr,
                             const DecodeRagged* rg = nullptr);   // sinks, pg, rg: as for launch_decode

}  // namespace fa
