// FlashAttention backward, query-tile-stationary half: dQ and delta = rowsum(dO * O).
//
// Replaces the reference's flash_attention_dQ_kernel
// (code/_flash_attention_kernel_optimized.py:165-258).  Semantics kept: delta from the
// ROUNDED 16-bit O in fp32 (K:210-211) and stored for the dK/dV kernel (K:258);
// P recomputed from the forward's LSE (K:244); dS rounded to the input dtype before
// dS @ K (K:253); dQ cast on store (K:256).  (scale is applied once to the fp32
// accumulator instead of to every partial product.)
//
// Decomposition: workgroup = 4 waves = 128 query rows, wave = 32 rows; K and V stream
// through LDS in 64-key tiles exactly as in the forward.  Both score-shaped products are
// computed transposed with the query on the lane,
//     S^T  = K Q^T          (A = K rows from LDS,  B = Q^T  resident in registers)
//     dP^T = V dO^T - delta (A = V rows from LDS,  B = dO^T resident; -delta[q] is the
//                            accumulator's initial value: q is the lane, so it is one
//                            broadcast register tuple and costs no VALU per tile)
// so LSE / delta are per-lane scalars and dS^T = P^T o dP^T, rounded, is directly the
// B operand of dQ^T += K^T dS^T (K^T fetched from the same LDS image by
// ds_read_b64_tr_b16).
#include <stdlib.h>

#include <type_traits>

#include "fa_common.h"
#include "fa_kernels.h"

namespace fa {

template <int D>
struct DqCfg {
  static constexpr int BM = 128, BN = 64, NT = 256;
  static constexpr int ROWB = D * 2, CPR = D / 8, KS = D / 16, DB = D / 32;
  static constexpr int TILE_BYTES = BN * ROWB;
  static constexpr int DMA_PER_MAT = TILE_BYTES / (4 * 1024);  // 1-KiB LDS-DMA instructions per wave per matrix
  static constexpr int LDS_BYTES = 4 * TILE_BYTES;
};

// OCC = workgroups per CU the register allocation is held to (2: 256 VGPRs, 3: 168).
// DROP: attention dropout (fa_common.h `Dropout`): dP = mask / (1 - p) o (dO V^T), so the dP chain starts from zero and
// the mask, the rescale and -delta are applied per element before dS = P o (dP - delta).
// LOCAL: sliding-window attention (fa_local_bwd_dq_kernel below; CAUSAL and DROP false), the forward's band and tile
// ranges (fa_fwd.hip, fa_common.h local_tiles).  A row with LSE = -inf (no visible key) gets P = 0, so dQ = 0.
template <int D, typename T, bool CAUSAL, int OCC, bool DROP = false>
__global__ __launch_bounds__(256, OCC) void fa_bwd_dq_kernel(BwdParams p) {
  constexpr bool LOCAL = false, GQA = false, SOFTCAP = false, ALIBI = false;
  constexpr int wl = 0, wr = 0, group = 1;
  constexpr float softcap = 0.f;
  constexpr const float* slopes = nullptr;
  constexpr int slopes_bstride = 0;
#include "fa_bwd_dq_body.inc"
}

// Sliding-window dQ + delta (LOCAL, above): one 128-row query tile per workgroup, ascending, unpaired; two workgroups
// per CU.  wl, wr >= 0 (an unbounded side comes in as kWindowUnbounded).
template <int D, typename T>
__global__ __launch_bounds__(256, 2) void fa_local_bwd_dq_kernel(BwdParams p, int wl, int wr) {
  constexpr bool CAUSAL = false, DROP = false, LOCAL = true, GQA = false, SOFTCAP = false, ALIBI = false;
  constexpr int group = 1;
  constexpr float softcap = 0.f;
  constexpr const float* slopes = nullptr;
  constexpr int slopes_bstride = 0;
#include "fa_bwd_dq_body.inc"
}

// GQA dQ + delta over the sliding window: the local kernel with K/V head h / group for query head h.
template <int D, typename T>
__global__ __launch_bounds__(256, 2) void fa_gqa_bwd_dq_kernel(BwdParams p, int wl, int wr, int group) {
  constexpr bool CAUSAL = false, DROP = false, LOCAL = true, GQA = true, SOFTCAP = false, ALIBI = false;
  constexpr float softcap = 0.f;
  constexpr const float* slopes = nullptr;
  constexpr int slopes_bstride = 0;
#include "fa_bwd_dq_body.inc"
}

// Soft-capped GQA dQ + delta (include/mi355fa_softcap.h): the GQA kernel with u = softcap * tanh(s * scale / softcap)
// in place of the score and the factor (1 - tanh^2) in dS.  With the bf16 q_scaled workspace it stores the Q it multiplied.
template <int D, typename T>
__global__ __launch_bounds__(256, 2) void fa_softcap_bwd_dq_kernel(BwdParams p, int wl, int wr, int group, float softcap) {
  constexpr bool CAUSAL = false, DROP = false, LOCAL = true, GQA = true, SOFTCAP = true, ALIBI = false;
  constexpr const float* slopes = nullptr;
  constexpr int slopes_bstride = 0;
#include "fa_bwd_dq_body.inc"
}

// ALiBi GQA dQ + delta (include/mi355fa_alibi.h): the GQA kernel with -slope_h |i - j| added to every recomputed score;
// dS needs no other change.  With the bf16 q_scaled workspace it stores the Q it multiplied.
template <int D, typename T>
__global__ __launch_bounds__(256, 2) void fa_alibi_bwd_dq_kernel(BwdParams p, int wl, int wr, int group, const float* slopes,
                                                                 int slopes_bstride) {
  constexpr bool CAUSAL = false, DROP = false, LOCAL = true, GQA = true, SOFTCAP = false, ALIBI = true;
  constexpr float softcap = 0.f;
#include "fa_bwd_dq_body.inc"
}

template <int D, typename T, bool CAUSAL, int OCC = 2, bool DROP = false>
static hipError_t launch(const BwdParams& p, hipStream_t s) {
  using C = DqCfg<D>;
  const int grid = (CAUSAL && p.pair ? (p.n_tiles + 1) / 2 : p.n_tiles) * p.B * p.H;
  // Three workgroups per CU pay off for the bf16 kernel (no fma/sub in its hot loop, fa_common.h kFoldScale) once
  // the grid fills them: +3 % causal, +7 % non-causal at B4 H32 N4096.  The tighter register budget spills in
  // the prologue only, which costs small grids more than the occupancy gives (B4 H8 S1024: -16 %); fp16: no gain.
  if constexpr (OCC == 2 && D == 64 && T::kFoldScale && !DROP) {
    if (grid >= 3 * 256) return launch<D, T, CAUSAL, 3>(p, s);
  }
  auto kern = fa_bwd_dq_kernel<D, T, CAUSAL, OCC, DROP>;
  if (C::LDS_BYTES > 48 * 1024) {
    static std::atomic<unsigned long long> opted_in{0};   // per template instance: devices already opted in
    if (hipError_t e = opt_in_lds((const void*)kern, C::LDS_BYTES, opted_in)) return e;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(C::NT), C::LDS_BYTES, s, p);
  return hipGetLastError();
}

hipError_t launch_bwd_dq_v2(BwdParams p, int dtype, int causal, hipStream_t s);  // fa_bwd_dq_v2.hip
hipError_t launch_bwd_dq_v3(BwdParams p, int dtype, int causal, hipStream_t s);  // fa_bwd_dq_v3.hip
hipError_t launch_bwd_dq_v4(BwdParams p, int dtype, int causal, hipStream_t s);  // fa_bwd_dq_v4.hip

hipError_t launch_bwd_dq(BwdParams p, int D, int dtype, int causal, hipStream_t s) {
  const int impl = dq_family(D, dtype, p.B, p.H, p.Sq, p.Sk, causal != 0, p.vl.cu_q != nullptr, p.all_contiguous(D),
                             p.drop.thresh != 0);
  if (impl == 4) return launch_bwd_dq_v4(p, dtype, causal, s);
  if (impl == 3) return launch_bwd_dq_v3(p, dtype, causal, s);
  if (impl == 2) return launch_bwd_dq_v2(p, dtype, causal, s);
  p.n_tiles = (p.Sq + 127) / 128;
  p.pair = want_pairs(causal != 0, p.n_tiles, (long)p.B * p.H);
#define FA_GO(DD, TT)                                                                                 \
  (p.drop.thresh ? (causal ? launch<DD, TT, true, 2, true>(p, s) : launch<DD, TT, false, 2, true>(p, s)) \
                 : (causal ? launch<DD, TT, true>(p, s) : launch<DD, TT, false>(p, s)))
  if (D == 64) return dtype == 1 ? FA_GO(64, BF16) : FA_GO(64, FP16);
  if (D == 128) return dtype == 1 ? FA_GO(128, BF16) : FA_GO(128, FP16);
#undef FA_GO
  return hipErrorInvalidValue;
}

template <int D, typename T>
static hipError_t launch_local(const BwdParams& p, int wl, int wr, hipStream_t s) {
  using C = DqCfg<D>;
  auto kern = fa_local_bwd_dq_kernel<D, T>;
  if (C::LDS_BYTES > 48 * 1024) {
    static std::atomic<unsigned long long> opted_in{0};
    if (hipError_t e = opt_in_lds((const void*)kern, C::LDS_BYTES, opted_in)) return e;
  }
  hipLaunchKernelGGL(kern, dim3(p.n_tiles * p.B * p.H), dim3(C::NT), C::LDS_BYTES, s, p, wl, wr);
  return hipGetLastError();
}

// Sliding-window dQ: always family 1 (fa_table.h is not consulted), no dropout (refused by the C ABI).
hipError_t launch_bwd_dq_local(BwdParams p, int D, int dtype, int wl, int wr, hipStream_t s) {
  p.n_tiles = (p.Sq + 127) / 128;
  p.pair = 0;
  if (D == 64) return dtype == 1 ? launch_local<64, BF16>(p, wl, wr, s) : launch_local<64, FP16>(p, wl, wr, s);
  if (D == 128) return dtype == 1 ? launch_local<128, BF16>(p, wl, wr, s) : launch_local<128, FP16>(p, wl, wr, s);
  return hipErrorInvalidValue;
}

template <int D, typename T>
static hipError_t launch_gqa(const BwdParams& p, int wl, int wr, int group, hipStream_t s) {
  using C = DqCfg<D>;
  auto kern = fa_gqa_bwd_dq_kernel<D, T>;
  if (C::LDS_BYTES > 48 * 1024) {
    static std::atomic<unsigned long long> opted_in{0};
    if (hipError_t e = opt_in_lds((const void*)kern, C::LDS_BYTES, opted_in)) return e;
  }
  hipLaunchKernelGGL(kern, dim3(p.n_tiles * p.B * p.H), dim3(C::NT), C::LDS_BYTES, s, p, wl, wr, group);
  return hipGetLastError();
}

// GQA dQ: family 1, one workgroup per (batch, query head, 128-row tile), as launch_bwd_dq_local.
hipError_t launch_bwd_dq_gqa(BwdParams p, int D, int dtype, int wl, int wr, int group, hipStream_t s) {
  p.n_tiles = (p.Sq + 127) / 128;
  p.pair = 0;
  if (D == 64) return dtype == 1 ? launch_gqa<64, BF16>(p, wl, wr, group, s) : launch_gqa<64, FP16>(p, wl, wr, group, s);
  if (D == 128) return dtype == 1 ? launch_gqa<128, BF16>(p, wl, wr, group, s) : launch_gqa<128, FP16>(p, wl, wr, group, s);
  return hipErrorInvalidValue;
}

template <int D, typename T>
static hipError_t launch_softcap(const BwdParams& p, int wl, int wr, int group, float softcap, hipStream_t s) {
  using C = DqCfg<D>;
  auto kern = fa_softcap_bwd_dq_kernel<D, T>;
  if (C::LDS_BYTES > 48 * 1024) {
    static std::atomic<unsigned long long> opted_in{0};
    if (hipError_t e = opt_in_lds((const void*)kern, C::LDS_BYTES, opted_in)) return e;
  }
  hipLaunchKernelGGL(kern, dim3(p.n_tiles * p.B * p.H), dim3(C::NT), C::LDS_BYTES, s, p, wl, wr, group, softcap);
  return hipGetLastError();
}

// Soft-capped dQ: the GQA grid (launch_bwd_dq_gqa).
hipError_t launch_bwd_dq_softcap(BwdParams p, int D, int dtype, int wl, int wr, int group, float softcap, hipStream_t s) {
  p.n_tiles = (p.Sq + 127) / 128;
  p.pair = 0;
  if (D == 64)
    return dtype == 1 ? launch_softcap<64, BF16>(p, wl, wr, group, softcap, s) : launch_softcap<64, FP16>(p, wl, wr, group, softcap, s);
  if (D == 128)
    return dtype == 1 ? launch_softcap<128, BF16>(p, wl, wr, group, softcap, s) : launch_softcap<128, FP16>(p, wl, wr, group, softcap, s);
  return hipErrorInvalidValue;
}

template <int D, typename T>
static hipError_t launch_alibi(const BwdParams& p, int wl, int wr, int group, const float* slopes, int sbs, hipStream_t s) {
  using C = DqCfg<D>;
  auto kern = fa_alibi_bwd_dq_kernel<D, T>;
  if (C::LDS_BYTES > 48 * 1024) {
    static std::atomic<unsigned long long> opted_in{0};
    if (hipError_t e = opt_in_lds((const void*)kern, C::LDS_BYTES, opted_in)) return e;
  }
  hipLaunchKernelGGL(kern, dim3(p.n_tiles * p.B * p.H), dim3(C::NT), C::LDS_BYTES, s, p, wl, wr, group, slopes, sbs);
  return hipGetLastError();
}

// ALiBi dQ: the GQA grid (launch_bwd_dq_gqa).
hipError_t launch_bwd_dq_alibi(BwdParams p, int D, int dtype, int wl, int wr, int group, const float* slopes, int sbs,
                                hipStream_t s) {
  p.n_tiles = (p.Sq + 127) / 128;
  p.pair = 0;
  if (D == 64)
    return dtype == 1 ? launch_alibi<64, BF16>(p, wl, wr, group, slopes, sbs, s) : launch_alibi<64, FP16>(p, wl, wr, group, slopes, sbs, s);
  if (D == 128)
    return dtype == 1 ? launch_alibi<128, BF16>(p, wl, wr, group, slopes, sbs, s) : launch_alibi<128, FP16>(p, wl, wr, group, slopes, sbs, s);
  return hipErrorInvalidValue;
}

}  // namespace fa
