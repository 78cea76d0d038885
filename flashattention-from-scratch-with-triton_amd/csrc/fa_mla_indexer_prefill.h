// The DeepSeek-V3.2 indexer logits of a prefill step: packed FP8 queries over one contiguous FP8 key array, a key range per
// query row (fa_mla_indexer_prefill.hip; C ABI in include_mla_indexer_prefill/mi355fa_mla_indexer_prefill.h, argument checks in
// fa_api_mla_indexer_prefill.hip): the parameter block of its kernel and the host-side launcher.  Internal to libmi355fa.so.
#pragma once
#include <hip/hip_runtime.h>

namespace fa {

constexpr int kPreRows = 16;          // query rows of a workgroup: four per wave, resident as the MFMA's A operand
constexpr int kPreTile = 32;          // keys of a tile: two MFMA column blocks of 16
constexpr int kPreRowBytes = 144;     // a 128-byte key row in LDS, padded by 16 bytes (the bank layout: fa_mla_indexer_prefill.hip)
constexpr int kPreMaxM = kPreRows * 65535;   // row blocks are the grid's y dimension

// A tag and a block of their own for the overloads <IdxPrefill, H_i / 16> of fa_decode_paged_kernel: the other decode kernels'
// names are recorded sets, and the race tables claim this stem.
struct IdxPrefill {};
struct IdxPrefillParams {
  const void* q;          // e4m3 [M, H_i, 128] through q_sm / q_sh (bytes)
  const float* w;         // fp32 [M, H_i] through w_sm / w_sh (elements)
  const void* k;          // e4m3 [N, 128] through k_rs (bytes)
  const float* ks;        // fp32 [N] through s_rs (elements)
  const int* lo;          // int32 [M]: the first visible key of a row ...
  const int* hi;          // ... and the one past its last; both clamped to [0, N] by the kernel
  float* out;             // fp32 [M, W] through o_sm (elements)
  long long q_sm, q_sh, w_sm, w_sh, k_rs, s_rs, o_sm;
  int M, Hi, N, W;
  int chunk_tiles;        // filled by the launcher: 32-key tiles of one workgroup
};

// Enqueue the kernel on `s`.
hipError_t launch_mla_indexer_prefill(IdxPrefillParams p, hipStream_t s);

}  // namespace fa
