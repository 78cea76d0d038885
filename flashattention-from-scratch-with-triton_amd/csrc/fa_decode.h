// Split-KV decoding attention over a padded or paged KV cache (fa_decode.hip; C ABI in include/mi355fa_kvcache.h,
// include/mi355fa_paged.h and, for packed variable-length queries, include/mi355fa_ragged.h): the parameter
// block the three decode kernels share, the description of a launch (DecodeMod) and the host-side launcher.  Internal to
// libmi355fa.so.
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

// The workspace of a launch with nsplit splits: nsplit * B * H * S_q * (D + 2) * 4 bytes when nsplit > 1 (partial O in fp32,
// then (m, l) pairs), 0 otherwise.
inline long long kvcache_ws_bytes(int nsplit, int B, int H, int S_q, int D) {
  return nsplit > 1 ? (long long)nsplit * B * H * S_q * (D + 2) * 4 : 0;
}
// the 32-row blocks the group * S_q rows of one K/V head take: a workgroup each, per split
inline long long decode_row_blocks(int group, int S_q) { return ((long long)group * S_q + 31) / 32; }
// What the caches hold: 16-bit values of the call's dtype, OCP e4m3 bytes (include/mi355fa_kvcache_fp8.h), MXFP4
// (include/mi355fa_kvcache_fp4.h: e2m1 nibbles, their e8m0 scales in DecodeFp4 below) or e4m3 bytes with one fp32 scale per
// cached token and K/V head (include/mi355fa_kvcache_fp8_token.h: the scales in DecodeFp8Token below).
enum class KvFormat { k16, kE4M3, kMXFP4, kE4M3Token };
// The split count of a launch with `wgs` workgroups per split (forced > 0: that count): fa_decode.hip has the rule for
// each cache format.
int kvcache_splits(long long wgs, int S_cache, int D, KvFormat fmt, int forced);
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
// the plan kernel alone, as launch_decode enqueues it first (tools/ragged_bench.py times it)
hipError_t launch_ragged_plan(const int* cu_q, int B, int group, const DecodeRagged& g, hipStream_t s);

// MXFP4 caches (include/mi355fa_kvcache_fp4.h): p.kc / p.vc hold e2m1 nibbles (lk / lv strides in bytes, rows of D / 2 bytes),
// ks / vs the e8m0 scale bytes of K / V, [.., H_kv, rows, D / 32] with the byte layouts lks / lvs; q / o / k_new / v_new are
// `dtype`.  The append quantises and writes nibbles and scales, the combine kernel is the 16-bit one.  D = 64 / 128, and with
// packed queries (include/mi355fa_ragged_fp4.h) also 256.
struct DecodeFp4 {
  unsigned char *ks, *vs;
  TensorLayout lks, lvs;
};

// Per-token-scaled e4m3 caches (include/mi355fa_kvcache_fp8_token.h): p.kc / p.vc hold e4m3 bytes exactly as with kE4M3 (lk /
// lv strides in bytes, rows of D bytes), ks / vs one fp32 scale per cache row, [.., H_kv, rows] with the BYTE layouts lks / lvs (a
// "row" of scales is one float); q / o / k_new / v_new are `dtype`.  The append computes each new row's scale and writes bytes and
// scale, the combine kernel is the 16-bit one.  D = 64 / 128, and with packed queries also 256.
struct DecodeFp8Token {
  float *ks, *vs;
  TensorLayout lks, lvs;
};

// One decode launch beside its DecodeParams: the score transform (at most one of softcap, slopes and sinks; a byte cache
// takes sinks or a soft-cap, no slopes), the cache format and the cache / query geometry.  The soft-capped kernels of the byte
// caches take softcap, the descales and the scale tensors in one list (fa_decode.hip).  The other attention kernels take softcap .. sinks as their
// arguments in this order (without `fmt`), the paged ones pg's members after them, the ragged ones cu_q, plan and total_q last;
// the MXFP4 ones take sinks, then fp4's members, then pg's, then (packed) cu_q, plan and total_q, and the kE4M3Token ones the
// same with tok's members for fp4's.
// fmt == kE4M3: p.kc / p.vc hold bytes (lk / lv strides in bytes, rows of D bytes), q / o / k_new / v_new are `dtype`; the append
// quantises, the combine kernel is the 16-bit one.  Both descales may be NULL.  fmt == kMXFP4: `fp4` holds the scale tensors.
// launch_decode refuses the combinations that have no kernel (fa_decode.hip).
struct DecodeMod {
  float softcap = 0.f;                // > 0, finite: the soft-capped kernel (include/mi355fa_softcap.h)
  const float* slopes = nullptr;      // the ALiBi kernel (include/mi355fa_alibi.h): the slope of query head h of sequence b
  int slopes_bstride = 0;             //   at slopes[b * slopes_bstride + h]
  KvFormat fmt = KvFormat::k16;
  const float *kds = nullptr, *vds = nullptr;   // kE4M3: the dequantisation factor of K / V head hk of sequence b at
  int ds_bstride = 0;                           //   [b * ds_bstride + hk], NULL = 1
  const float* sinks = nullptr;       // the sink kernel (include/mi355fa_sink.h): one fp32 logit per query head
  const DecodePaging* pg = nullptr;   // a paged cache: the paged forms of the append and of the attention kernel
  const DecodeRagged* rg = nullptr;   // packed queries (with pg): the plan kernel first, then the packed forms of all three
  const DecodeFp4* fp4 = nullptr;     // kMXFP4: the scale tensors (sinks or softcap, pg and rg only beside it)
  const DecodeFp8Token* tok = nullptr;   // kE4M3Token: the row scales (sinks or softcap, pg and rg only beside it)
};

// Enqueue the append (when S_new > 0), the attention kernel and (nsplit > 1) the combine kernel on `s`.
hipError_t launch_decode(const DecodeParams& p, int dtype, hipStream_t s, const DecodeMod& m);

}  // namespace fa
