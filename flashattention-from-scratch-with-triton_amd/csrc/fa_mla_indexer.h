// The DeepSeek-V3.2 indexer logits over a paged FP8 key cache (fa_mla_indexer.hip; C ABI in
// include_mla_indexer/mi355fa_mla_indexer.h, argument checks in fa_api_mla_indexer.hip): the parameter block of its two kernels
// and the host-side launcher.  Internal to libmi355fa.so.
#pragma once
#include <hip/hip_runtime.h>

#include "fa_kernels.h"

namespace fa {

constexpr int kIdxD = 128;        // dims of an index head = bytes of a cached key
constexpr int kIdxTile = 32;      // keys a wave takes at a time: two MFMA column blocks of 16
constexpr int kIdxWaves = 4;      // waves of a workgroup, each on its own tiles

// A tag and a block of their own for the overloads <IdxLogits, H_i / 16, QG> of fa_decode_paged_kernel and <IdxLogits, T> of
// fa_kvcache_append_paged_kernel: the other decode kernels' names are recorded sets, and the race tables claim these stems.
struct IdxLogits {};
struct IndexerParams {
  const void* q;          // e4m3 [B, S_q, H_i, 128] through q_sb / q_ss / q_sh (bytes)
  const float* w;         // fp32 [B, S_q, H_i] through w_sb / w_ss / w_sh (elements)
  void* k;                // e4m3 pool [num_pages, page_size, 128] through k_ps / k_rs (bytes)
  float* ks;              // fp32 [num_pages, page_size] through ks_ps / ks_rs (elements)
  const void* k_new;      // T [B, Snew, 128] contiguous, or nullptr
  const int* seqlens;
  const int* table;
  float* out;             // fp32 [B, S_q, W] through o_sb / o_ss (elements)
  long long q_sb, q_ss, q_sh, w_sb, w_ss, w_sh, k_ps, ks_ps, ks_rs, o_sb, o_ss;
  int k_rs;
  int B, Sq, Hi, W, Snew, causal;
  int num_pages, page_size, max_pages, bt_stride;
  int chunk_tiles;        // filled by the launcher: 32-key tiles of one workgroup, a multiple of kIdxWaves
  FastDiv tpp, pdiv;      // a tile index / (page_size / 32), a logical position / page_size
};

// Enqueue the quantising append (Snew > 0) and the logits kernel on `s`.
hipError_t launch_mla_indexer(IndexerParams p, int dtype, hipStream_t s);

}  // namespace fa
