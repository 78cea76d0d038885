// Sparse (top-k indexed) MLA prefill over one contiguous latent array (fa_mla_sparse_prefill.hip; C ABI in
// include_mla_sparse_prefill/mi355fa_mla_sparse_prefill.h, argument checks in fa_api_mla_sparse_prefill.hip): the parameter
// block of its kernel and the host-side launcher.  Internal to libmi355fa.so.
#pragma once
#include <hip/hip_runtime.h>

namespace fa {

constexpr int kRowListHeads = 32;     // heads of one query token per workgroup: the MFMA's 32 columns
constexpr int kRowListTile = 32;      // list entries per step
constexpr int kRowListMaxM = 1 << 22;
constexpr int kRowListMaxH = 1 << 10;

// A tag and a block of their own for the overloads <RowList, T> of fa_decode_paged_kernel: the other decode kernels' names are
// recorded sets, and the race tables claim this stem.  A kernel's name carries its template arguments and the type of its
// parameter block.
struct RowList {};
struct RowListParams {
  const void* q;          // 16-bit [M, H, 576] through q_sm / q_sh (bytes)
  const void* kv;         // 16-bit [N, 576] through kv_rs (bytes): the latent rows of every key of the step
  const int* indices;     // int32 [M, topk] through idx_rs (elements): rows of kv; visible iff 0 <= idx < N
  void* o;                // 16-bit [M, H, 512] through o_sm / o_sh (bytes)
  float* lse;             // fp32 [M, H], natural log; may be NULL
  long long q_sm, q_sh, kv_rs, o_sm, o_sh, idx_rs;
  int M, H, N, topk;
  float scale;
};

// Enqueue the kernel on `s`: 8 * ceil(H / 32) * ceil(M / 8) workgroups, no workspace.
hipError_t launch_mla_sparse_prefill(const RowListParams& p, int dtype, hipStream_t s);

}  // namespace fa
