// FlashAttention backward, key-tile-stationary half: dK and dV.
//
// Replaces the reference's flash_attention_dKV_kernel
// (code/_flash_attention_kernel_optimized.py:292-386).  Semantics kept: runs AFTER the dQ
// kernel and loads the delta it stored (K:376, launch order M:111-126); P recomputed from
// LSE (K:367); P^T and dS^T rounded to the input dtype before their matmuls (K:370, K:382);
// padded query rows contribute nothing (K:355-356); causal loop starts at the key tile
// (K:341); dK, dV cast on store (K:385-386).  (scale applied once to the fp32 dK.)
//
// Decomposition: workgroup = 4 waves = 128 keys of one (batch, head); wave = 32 keys whose
// K and V fragments stay in registers as MFMA B operands, and whose dK^T / dV^T tiles
// ([d][key], key on the lane) stay in fp32 accumulators for the whole kernel -- no
// cross-workgroup reduction.  Q and dO stream through LDS in 64-row tiles (one swizzled
// image each, read by rows for S / dP and transposed for dV^T / dK^T), with
// -LSE*log2(e) and -delta staged beside them.  With the key on the lane,
//     S  = Q K^T             (A = Q rows,  B = K^T resident)
//     dP = dO V^T - delta    (A = dO rows, B = V^T resident; -delta[q] preloaded as C)
// have the query index in the accumulator REGISTER, so P and dS = P o dP are, after
// rounding, directly the B operands of dV^T += dO^T P and dK^T += Q^T dS.
#include <stdlib.h>

#include <type_traits>

#include "fa_common.h"
#include "fa_kernels.h"

namespace fa {

template <int D>
struct DkvCfg {
  static constexpr int BK = 128;  // keys per workgroup
  static constexpr int BQ = 64;   // query rows per LDS tile
  static constexpr int NT = 256;
  static constexpr int ROWB = D * 2, CPR = D / 8, KS = D / 16, DB = D / 32;
  static constexpr int TILE_BYTES = BQ * ROWB;
  static constexpr int DMA_PER_MAT = TILE_BYTES / (4 * 1024);  // 1-KiB LDS-DMA instructions per wave per matrix
  static constexpr int ROWC_OFF = 4 * TILE_BYTES;           // row constants after Q[2], dO[2]
  static constexpr int ROWC_BYTES = 2 * BQ * 4;             // nl[64], nd[64] per buffer
  static constexpr int LDS_BYTES = 4 * TILE_BYTES + 2 * ROWC_BYTES;
};

// DROP: attention dropout (fa_common.h `Dropout`): dV uses the masked, rescaled P; dP = mask / (1 - p) o (dO V^T), so the
// dP chain starts from zero and -delta is added per element.
// LOCAL: sliding-window attention (fa_bwd_dkv_mod_kernel below; CAUSAL and DROP false).  Key j is seen by the queries
// j - wr <= i <= j + wl (i < S_q): the workgroup visits only the query tiles that meet its keys' band; per wave the tiles
// fully inside it are unmasked, the edge tiles masked.  A key no query sees gets dK = dV = 0.
template <int D, typename T, bool CAUSAL, bool DROP = false>
__global__ __launch_bounds__(256, (D == 64 ? 2 : 1)) void fa_bwd_dkv_kernel(BwdParams p) {
  constexpr bool LOCAL = false, GQA = false, SOFTCAP = false, ALIBI = false;
  constexpr int wl = 0, wr = 0, group = 1;
  constexpr float softcap = 0.f;
  constexpr const float* slopes = nullptr;
  constexpr int slopes_bstride = 0;
#include "fa_bwd_dkv_body.inc"
}

// The score-transform variants of dK / dV (fa_kernels.h ScoreMod; the forward's flags, fa_fwd.hip fa_fwd_mod_kernel), all on the
// sliding-window tile loop (LOCAL, above): one 128-key tile per workgroup, ascending, unpaired.
//   GQA      one workgroup per (batch, K/V head, 128-key tile).  K, V and their fragments are loaded once; the `group`
//            query heads that read them stream through the tile band one after the other and add into the same fp32
//            accumulators, so dK / dV of the K/V head are the sum over its group, in head order, rounded once on store
//   SOFTCAP  the capped score in P and (1 - tanh^2) in dS
//   ALIBI    -slope_h |i - j| in the recomputed P; the slope is reloaded at every query head of the group
// Attention sinks change no score: their backward is the GQA instance on the sink forward's LSE.
template <int D, typename T, bool GQA, bool SOFTCAP, bool ALIBI>
__global__ __launch_bounds__(256, (D == 64 ? 2 : 1))
    void fa_bwd_dkv_mod_kernel(BwdParams p, int wl, int wr, int group_, float softcap, const float* slopes, int slopes_bstride) {
  constexpr bool CAUSAL = false, DROP = false, LOCAL = true;
  const int group = GQA ? group_ : 1;
  // The body's loop over the group's query heads is in its text only under FA_DKV_HEAD_LOOP (a one-trip loop changes the
  // register allocation of the kernels without GQA), and a macro cannot follow a template parameter: both texts, one compiled.
  if constexpr (GQA) {
#define FA_DKV_HEAD_LOOP
#include "fa_bwd_dkv_body.inc"
#undef FA_DKV_HEAD_LOOP
  } else {
#include "fa_bwd_dkv_body.inc"
  }
}

template <int D, typename T, bool CAUSAL, bool DROP = false>
static hipError_t launch(const BwdParams& p, hipStream_t s) {
  using C = DkvCfg<D>;
  const int grid = (CAUSAL && p.pair ? (p.n_tiles + 1) / 2 : p.n_tiles) * p.B * p.H;
  return launch_kernel<fa_bwd_dkv_kernel<D, T, CAUSAL, DROP>>(grid, C::NT, C::LDS_BYTES, s, p);
}

hipError_t launch_bwd_dkv_v2(BwdParams p, int D, int dtype, int causal, hipStream_t s);  // fa_bwd_dkv_v2.hip
hipError_t launch_bwd_dkv_v3(BwdParams p, int dtype, int causal, hipStream_t s);         // fa_bwd_dkv_v3.hip
hipError_t launch_bwd_dkv_v4(BwdParams p, int dtype, int causal, hipStream_t s);         // fa_bwd_dkv_v4.hip

hipError_t launch_bwd_dkv(BwdParams p, int D, int dtype, int causal, hipStream_t s) {
  const int impl = dkv_family(D, dtype, p.B, p.H, p.Sq, p.Sk, causal != 0, p.vl.cu_q != nullptr, p.drop.thresh != 0);
  if (impl == 4) return launch_bwd_dkv_v4(p, dtype, causal, s);
  if (impl == 2) return launch_bwd_dkv_v2(p, D, dtype, causal, s);
  if (impl == 3) return launch_bwd_dkv_v3(p, dtype, causal, s);
  p.n_tiles = (p.Sk + 127) / 128;
  p.pair = want_pairs(causal != 0, p.n_tiles, (long)p.B * p.H);
#define FA_GO(DD, TT)                                                                           \
  (p.drop.thresh ? (causal ? launch<DD, TT, true, true>(p, s) : launch<DD, TT, false, true>(p, s)) \
                 : (causal ? launch<DD, TT, true>(p, s) : launch<DD, TT, false>(p, s)))
  if (D == 64) return dtype == 1 ? FA_GO(64, BF16) : FA_GO(64, FP16);
  if (D == 128) return dtype == 1 ? FA_GO(128, BF16) : FA_GO(128, FP16);
#undef FA_GO
  return hipErrorInvalidValue;
}

template <int D, typename T, bool GQA, bool SOFTCAP, bool ALIBI>
static hipError_t launch_mod(const BwdParams& p, const ScoreMod& sm, hipStream_t s) {
  using C = DkvCfg<D>;
  const int heads = GQA ? p.H / sm.group : p.H;  // GQA: B * H_kv * key tiles workgroups (p.H is the number of QUERY heads)
  return launch_kernel<fa_bwd_dkv_mod_kernel<D, T, GQA, SOFTCAP, ALIBI>>(p.n_tiles * p.B * heads, C::NT, C::LDS_BYTES, s, p,
                                                                         sm.wl, sm.wr, sm.group, sm.softcap, sm.slopes, sm.slopes_bstride);
}

// Variant dK / dV (fa_kernels.h ScoreMod): one workgroup per (batch, K/V head, 128-key tile).
hipError_t launch_bwd_dkv_mod(BwdParams p, int D, int dtype, const ScoreMod& sm, hipStream_t s) {
  p.n_tiles = (p.Sk + 127) / 128;
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
