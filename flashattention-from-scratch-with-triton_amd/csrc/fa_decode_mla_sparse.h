// Sparse (top-k indexed) MLA decoding over the paged latent cache (fa_decode_mla_sparse.hip; C ABI in
// include_mla_sparse/mi355fa_kvcache_mla_sparse.h, argument checks in fa_api_mla_sparse.hip): the parameter block of its attention
// kernel and the host-side launcher.  Internal to libmi355fa.so.
#pragma once
#include <hip/hip_runtime.h>

#include "fa_decode_mla.h"

namespace fa {

// The dense call's block (fa_decode_mla.h: the append and the combine are launched from `m` as it stands) and the index lists:
// indices is int32 [B, S_q, topk], the last dim contiguous, batch and row strides in elements.  Entry j of (b, i) is a logical
// position of sequence b: the key in page table[b][idx / page_size], row idx % page_size.  Query i of sequence b attends to the
// entries with 0 <= idx < L_b (and idx <= L_b - S_q + i under m.causal), duplicates counted as often as they appear; every
// other entry is skipped.  m.nsplit splits the topk entries, not the cache.
// A tag and a block of their own for the overload <Topk, T> of fa_decode_paged_kernel: the dense kernels' names are recorded
// sets (tests/test_host_mla.py, _ragged.py, _fp8.py), and a kernel's name carries its template arguments and the type of its
// parameter block.
struct Topk {};
struct TopkParams {
  MlaParams m;
  const int* indices;
  long long idx_sb, idx_ss;
  int topk;
  FastDiv pdiv;   // a logical position / page_size
};

// The split count of a launch with `wgs` workgroups per split (B * S_q * ceil(H / 32)) over lists of topk entries; forced > 0:
// that count.
int mla_sparse_splits(long long wgs, int topk, int forced);

// Enqueue the append (m.Snew > 0), the sparse attention kernel and (m.nsplit > 1) the combine kernel on `s`.
hipError_t launch_decode_mla_sparse(const TopkParams& p, int dtype, hipStream_t s);

}  // namespace fa
