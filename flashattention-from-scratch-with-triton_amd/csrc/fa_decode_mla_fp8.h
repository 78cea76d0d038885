// MLA decoding over a paged FP8 latent cache (fa_decode_mla_fp8.hip; C ABI in include_mla_fp8/mi355fa_kvcache_mla_fp8.h, argument
// checks in fa_api_mla_fp8.hip): the parameter block of its kernels and the host-side launcher.  Internal to libmi355fa.so.
#pragma once
#include <hip/hip_runtime.h>

#include "fa_decode_mla.h"

namespace fa {

// A cached row: 512 e4m3 bytes (the latent dims), four fp32 scales (scale j: dims [128 j, 128 j + 128)), then the 64 RoPE
// values in the call's 16-bit type, not quantised.  Every piece starts at a multiple of 16 bytes.
constexpr int kFp8RowScaleOff = kMlaDv;                                  // 512
constexpr int kFp8RowRopeOff = kFp8RowScaleOff + 4 * 4;                  // 528
constexpr int kFp8RowB = kFp8RowRopeOff + (kMlaD - kMlaDv) * 2;          // 656

// MlaParams with the pool in bytes: kv is the uint8 pool [num_pages, page_size, 656], kv_ps / kv_rs its page and row strides in
// bytes, kv_new the 16-bit rows [B, S_new, 576] the append quantises.  Everything else is as fa_decode_mla.h says.  A block of
// its own, and a tag of its own for the overloads <Fp8Row, T> of fa_decode_paged_kernel, fa_kvcache_append_paged_kernel and
// fa_decode_combine_kernel: the 16-bit kernels' names are recorded sets (tests/test_host_mla.py, tests/test_host_mla_ragged.py),
// and a kernel's name carries its template arguments and the type of its parameter block.
struct Fp8Row {};
struct Fp8RowParams {
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

// Enqueue the quantising append (S_new > 0), the attention kernel and (nsplit > 1) the combine kernel on `s`.  The split count
// is mla_splits' (fa_decode_mla.h).
hipError_t launch_decode_mla_fp8(const Fp8RowParams& p, int dtype, hipStream_t s);
// Its first and last launch alone, for a call that brings an attention kernel of its own (fa_decode_mla_sparse_fp8.hip): the
// quantising append (S_new > 0: fa_kvcache_append_paged_kernel<Fp8Row, T>) and the combine of the nsplit partials in p.ws
// (fa_decode_combine_kernel<Fp8Row, T>).
hipError_t launch_mla_fp8_append(const Fp8RowParams& p, int dtype, hipStream_t s);
hipError_t launch_mla_fp8_combine(const Fp8RowParams& p, int dtype, hipStream_t s);

}  // namespace fa
