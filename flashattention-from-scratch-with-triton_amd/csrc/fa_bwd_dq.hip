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
// LOCAL: sliding-window attention (fa_bwd_dq_mod_kernel below; CAUSAL and DROP false), the forward's band and tile
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

// The score-transform variants of dQ + delta (fa_kernels.h ScoreMod; the forward's flags, fa_fwd.hip fa_fwd_mod_kernel), all on
// the sliding-window tile loop (LOCAL, above): one 128-row query tile per workgroup, ascending, unpaired; two workgroups per CU.
//   GQA      K/V head h / group for query head h
//   SOFTCAP  u = softcap * tanh(s * scale / softcap) in place of the score and the factor (1 - tanh^2) in dS
//   ALIBI    -slope_h |i - j| added to every recomputed score; dS needs no other change
// With the bf16 q_scaled workspace every variant stores the Q it multiplied.  Attention sinks change no score: their backward
// is the GQA instance on the sink forward's O and LSE.
template <int D, typename T, bool GQA, bool SOFTCAP, bool ALIBI>
__global__ __launch_bounds__(256, 2)
    void fa_bwd_dq_mod_kernel(BwdParams p, int wl, int wr, int group_, float softcap, const float* slopes, int slopes_bstride) {
  constexpr bool CAUSAL = false, DROP = false, LOCAL = true;
  const int group = GQA ? group_ : 1;
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
  return launch_kernel<fa_bwd_dq_kernel<D, T, CAUSAL, OCC, DROP>>(grid, C::NT, C::LDS_BYTES, s, p);
}

hipError_t launch_bwd_dq_v3(BwdParams p, int dtype, int causal, hipStream_t s);  // fa_bwd_dq_v3.hip
hipError_t launch_bwd_dq_v4(BwdParams p, int dtype, int causal, hipStream_t s);  // fa_bwd_dq_v4.hip

hipError_t launch_bwd_dq(BwdParams p, int D, int dtype, int causal, hipStream_t s) {
  const int impl = dq_family(D, dtype, p.B, p.H, p.Sq, p.Sk, causal != 0, p.vl.cu_q != nullptr, p.drop.thresh != 0);
  if (impl == 4) return launch_bwd_dq_v4(p, dtype, causal, s);
  if (impl == 3) return launch_bwd_dq_v3(p, dtype, causal, s);
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

template <int D, typename T, bool GQA, bool SOFTCAP, bool ALIBI>
static hipError_t launch_mod(const BwdParams& p, const ScoreMod& sm, hipStream_t s) {
  using C = DqCfg<D>;
  return launch_kernel<fa_bwd_dq_mod_kernel<D, T, GQA, SOFTCAP, ALIBI>>(p.n_tiles * p.B * p.H, C::NT, C::LDS_BYTES, s, p,
                                                                        sm.wl, sm.wr, sm.group, sm.softcap, sm.slopes, sm.slopes_bstride);
}

// Variant dQ (fa_kernels.h ScoreMod): one workgroup per (batch, query head, 128-row tile).
hipError_t launch_bwd_dq_mod(BwdParams p, int D, int dtype, const ScoreMod& sm, hipStream_t s) {
  p.n_tiles = (p.Sq + 127) / 128;
  p.pair = 0;
#define FA_GO(DD, TT)                                                   \
  (sm.slopes          ? launch_mod<DD, TT, true, false, true>(p, sm, s)  \
   : sm.softcap > 0.f ? launch_mod<DD, TT, true, true, false>(p, sm, s)  \
   : sm.group         ? launch_mod<DD, TT, true, false, false>(p, sm, s) \
                      : launch_mod<DD, TT, false, false, false>(p, sm, s))
  if (D == 64) return dtype == 1 ? FA_GO(64, BF16) : FA_GO(64, FP16);
  if (D == 128) return dtype == 1 ? FA_GO(128, BF16) : FA_GO(128, FP16);
#undef FA_GO
  return hipErrorInvalidValue;
}

}  // namespace fa
