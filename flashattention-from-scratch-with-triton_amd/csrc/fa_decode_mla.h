// MLA (multi-head latent attention) decoding over a paged latent cache (fa_decode_mla.hip; C ABI in
// include_mla/mi355fa_kvcache_mla.h, argument checks in fa_api_mla.hip): the parameter block of its kernels and the host-side
// launcher.  Internal to libmi355fa.so.
#pragma once
#include <hip/hip_runtime.h>

#include "fa_decode.h"

namespace fa {

constexpr int kMlaD = 576;     // a query head / a cached row: 512 latent dims, then 64 RoPE dims
constexpr int kMlaDv = 512;    // the value of a key: the latent dims of its row
constexpr int kMlaRowB = kMlaD * 2;

// q [B, H, S_q, 576] (lq), o [B, H, S_q, 512] (lo); kv: the pool [num_pages, page_size, 576] of ONE latent head, page and row
// strides in bytes (the page number goes into a 64-bit base, a row offset inside a page stays below 2^31); kv_new: contiguous
// [B, S_new, 576]; seqlens / table: device int32 [B] / [B, bt_stride].  Sequence b attends to L_b = seqlens[b] + S_new keys
// (clamped to [0, Scache = max_pages * page_size]), query i of it at position L_b - S_q + i; `causal` hides the keys behind it.
// nsplit > 1: per-split partials in `ws` (kvcache_ws_bytes with D = 512) for the combine kernel; lse may be null.
struct MlaParams {
  const void* q;
  void* kv;
  const void* kv_new;
  const int* seqlens;
  const int* table;
  void* o;
  float* lse;
  float* ws;
  TensorLayout lq, lo;
  long long kv_ps;
  int kv_rs;
  int B, H, Sq, Scache, Snew;
  int bt_stride, page_size, num_pages;
  FastDiv tpp;   // a tile index / the 32-key tiles of a page
  float scale;
  int causal;
  int nsplit;
};

// Tells the MLA overloads of fa_decode_paged_kernel and fa_kvcache_append_paged_kernel, <MLA, T>, from every other one.
struct MLA {};

// The split count of a launch with `wgs` workgroups per split (B * row blocks); forced > 0: that count.
int mla_splits(long long wgs, int S_cache, int forced);

// Enqueue the append (S_new > 0), the attention kernel and (nsplit > 1) the combine kernel on `s`.
hipError_t launch_decode_mla(const MlaParams& p, int dtype, hipStream_t s);

// Packed variable-length queries over the same pool (include_mla_ragged/mi355fa_ragged_mla.h): q [total_q, H, 576] / o
// [total_q, H, 512] (lq / lo: head and row strides, no batch stride), sequence b owns the packed rows [cu_q[b], cu_q[b + 1]) --
// S_b of them, each end clamped into [0, total_q] and the second to the first --, LSE is [H, total_q], the partials are those of
// H * total_q rows (kvcache_ws_bytes(nsplit, 1, H, total_q, 512)), kv_new is [total_q, 576] (Snew != 0: every query row brings
// its cached row, L_b = seqlens[b] + S_b) and Sq is unused (0).  `plan` is the work list fa_decode_ragged_plan_kernel builds
// with group = H (fa_decode.h DecodeRagged): nb_max = ragged_nb_max(H, total_q, B) entries, one workgroup each per split.
// A block of its own with the members of MlaParams first: the packed kernels' names are a set apart from the rectangular ones'
// (tests/test_host_mla.py, tests/test_host_mla_ragged.py), and a kernel's name carries the type of its parameter block.
// Latent tells the packed MLA overloads of fa_decode_ragged_kernel, fa_kvcache_append_ragged_kernel and
// fa_decode_combine_ragged_kernel, <Latent, T>, from every other one.
struct Latent {};
struct LatentRaggedParams {
  const void* q;
  void* kv;
  const void* kv_new;
  const int* seqlens;
  const int* table;
  void* o;
  float* lse;
  float* ws;
  TensorLayout lq, lo;
  long long kv_ps;
  int kv_rs;
  int B, H, Sq, Scache, Snew;
  int bt_stride, page_size, num_pages;
  FastDiv tpp;
  float scale;
  int causal;
  int nsplit;
  const int* cu_q;   // device int32 [B + 1]
  int* plan;         // ragged_plan_bytes(nb_max) bytes, 16-byte aligned
  int total_q;
  int nb_max;
};

// Enqueue the plan kernel, the packed append (Snew != 0), the packed attention kernel over nb_max * nsplit workgroups and
// (nsplit > 1) the combine by packed row on `s`.  The host reads none of cu_q, seqlens and table.
hipError_t launch_decode_mla_ragged(const LatentRaggedParams& p, int dtype, hipStream_t s);

}  // namespace fa
