// Sparse (top-k indexed) MLA decoding over the paged FP8 latent cache (fa_decode_mla_sparse_fp8.hip; C ABI in
// include_mla_sparse_fp8/mi355fa_kvcache_mla_sparse_fp8.h, argument checks in fa_api_mla_sparse_fp8.hip): the parameter block of
// its attention kernel and the host-side launcher.  Internal to libmi355fa.so.
#pragma once
#include <hip/hip_runtime.h>

#include "fa_decode_mla_fp8.h"

namespace fa {

// The dense FP8 call's block (fa_decode_mla_fp8.h: the quantising append and the combine are launched from `f` as it stands)
// and the index lists of fa_decode_mla_sparse.h: indices is int32 [B, S_q, topk], the last dim contiguous, batch and row strides
// in elements; entry j of (b, i) is a logical position of sequence b, the 656-byte row idx % page_size of page
// table[b][idx / page_size].  Query i of sequence b attends to the entries with 0 <= idx < L_b (and idx <= L_b - S_q + i under
// f.causal), duplicates counted as often as they appear; every other entry is skipped.  f.nsplit splits the topk entries, not
// the cache.
// A tag and a block of their own for the overload <GatherF8, T> of fa_decode_paged_kernel: the other decode kernels' names are
// recorded sets (tests/test_host_mla.py, _ragged.py, _fp8.py, _sparse.py), and a kernel's name carries its template arguments
// and the type of its parameter block -- not the types of that block's members.
struct GatherF8 {};
struct GatherF8Params {
  Fp8RowParams f;
  const int* indices;
  long long idx_sb, idx_ss;
  int topk;
  FastDiv pdiv;   // a logical position / page_size
};

// Enqueue the quantising append (f.Snew > 0), the gathering attention kernel and (f.nsplit > 1) the combine kernel on `s`.  The
// split count is mla_sparse_splits' (fa_decode_mla_sparse.h).
hipError_t launch_decode_mla_sparse_fp8(const GatherF8Params& p, int dtype, hipStream_t s);

}  // namespace fa
