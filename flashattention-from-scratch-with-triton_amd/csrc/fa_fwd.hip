// FlashAttention forward for gfx950: O = softmax(Q K^T / sqrt(D) [+causal]) V, LSE = logsumexp.
//
// Replaces the reference's flash_attention_forward_kernel
// (code/_flash_attention_kernel_optimized.py:35-129); semantics kept: fp32 scores and
// softmax state, l sums the un-rounded p (K:111), P is rounded to the input dtype for
// P@V (K:115), O = o / l cast on store (K:120-123), LSE = m + ln(l) (K:126),
// top-left aligned causal mask (K:102), keys >= S_k masked (K:94).
// Deviations inside the stated tolerance: the scale multiplies the fp32 accumulator once (fp16) or is folded into the
// resident Q fragments (bf16, fa_common.h kFoldScale); the rescale is deferred / lazy (tile(), tile_lazy()).
//
// Work decomposition (CDNA4-first, not the reference's 64x64 Triton tiles):
//   workgroup = 4 waves = 128 query rows of one (batch, head); wave = 32 query rows.
//   K/V stream through LDS in 64-key tiles (double buffered, swizzled image, one
//   barrier per tile).  Scores are computed TRANSPOSED, S^T = K Q^T, so the query
//   index sits on the MFMA lane: the online-softmax row max / row sum are in-lane
//   reductions plus one lane<->lane+32 exchange, the rescale is a per-lane scalar,
//   and the fp32 P^T accumulator is, after rounding, directly the B operand of
//   O^T += V^T P^T (V^T fetched with ds_read_b64_tr_b16) -- P never touches LDS.
#include <stdlib.h>

#include <type_traits>

#include "fa_common.h"
#include "fa_kernels.h"

namespace fa {

template <int D>
struct FwdCfg {
  static constexpr int BM = 128;           // query rows per workgroup
  static constexpr int BN = 64;            // keys per LDS tile
  static constexpr int NT = 256;           // threads
  static constexpr int ROWB = D * 2;       // bytes per row
  static constexpr int CPR = D / 8;        // 16-byte chunks per row
  static constexpr int KS = D / 16;        // k-steps of S^T = K Q^T
  static constexpr int DB = D / 32;        // 32-wide d blocks of O^T
  static constexpr int TILE_BYTES = BN * ROWB;
  static constexpr int DMA_PER_MAT = TILE_BYTES / (4 * 1024);  // 1-KiB LDS-DMA instructions per wave per matrix
  static constexpr int LDS_BYTES = 4 * TILE_BYTES;  // K[2], V[2]
  static constexpr int OCC = D == 64 ? 3 : 2;       // workgroups per CU the register allocation is held to (D = 64: two measured the same)
};

// Online-softmax rescale is deferred until a row max grows by more than 2^kDeferLog2 (see tile()).
constexpr float kDeferLog2 = 6.0f;
// Lazy running max: largest partial row sum accepted without recomputing the true max (see tile_lazy).
constexpr float kLazySumMax = 8192.0f;

// DROP: attention dropout (fa_common.h `Dropout`): P is masked before P @ V (exact and lazy tiles alike), l keeps summing
// the undropped p (the softmax normalisation is not affected by dropout), 1 / (1 - p) joins the normalisation of O.
//
// LOCAL: sliding-window (local) attention, fa_fwd_mod_kernel below (CAUSAL and DROP false).  Key j is visible from
// query i iff i - wl <= j <= i + wr (and j < S_k); the launcher passes an unbounded side as kWindowUnbounded.  The workgroup visits
// only the key tiles that meet its band; per wave, the tiles fully inside the band take the unmasked (lazy) path and the
// edge tiles on either side the masked one.  A row can meet its first visible key after masked tiles in which it saw
// none, so the exact tile keeps m = -inf for such a row without forming exp(-inf - -inf).
template <int D, typename T, bool CAUSAL, bool DROP = false>
__global__ __launch_bounds__(256, FwdCfg<D>::OCC) void fa_fwd_kernel(FwdParams p) {
  constexpr bool LOCAL = false, GQA = false, SOFTCAP = false, ALIBI = false, SINK = false;
  constexpr int wl = 0, wr = 0, group = 1;
  constexpr float softcap = 0.f;
  constexpr const float* slopes = nullptr;
  constexpr int slopes_bstride = 0;
  constexpr const float* sinks = nullptr;
#include "fa_fwd_body.inc"
}

// The score-transform variants (fa_kernels.h ScoreMod), all on the sliding-window tile loop (LOCAL, above): one 128-row
// query tile per workgroup, ascending, no causal pairing (a band costs about the same on every tile).  A flag that is
// false compiles its transform out; launch_fwd_mod below instantiates the combinations that exist.
//   GQA      query head h reads K/V head h / group (K and V have H / group heads, their layouts say so); (-1, -1) /
//            (-1, 0) windows cover full and causal attention
//   SOFTCAP  (include/mi355fa_softcap.h) every score s becomes u = softcap * tanh(s * scale / softcap) before the masks
//            and the softmax; softcap is finite and > 0 (the C ABI checks)
//   ALIBI    (include/mi355fa_alibi.h) every score s becomes s * scale - slope_h |i - j| before the masks and the softmax,
//            slope_h = slopes[b * slopes_bstride + h] (query head h; slopes_bstride 0 or >= H)
//   SINK     (include/mi355fa_sink.h) one more logit per query head, sinks[h] in natural-log units, joins every row's
//            softmax denominator and carries no value: only the epilogue (row sum, normalisation, LSE) sees it
template <int D, typename T, bool GQA, bool SOFTCAP, bool ALIBI, bool SINK>
__global__ __launch_bounds__(256, FwdCfg<D>::OCC)
    void fa_fwd_mod_kernel(FwdParams p, int wl, int wr, int group_, float softcap, const float* slopes, int slopes_bstride,
                           const float* sinks) {
  constexpr bool CAUSAL = false, DROP = false, LOCAL = true;
  const int group = GQA ? group_ : 1;
#include "fa_fwd_body.inc"
}

// ---- host launcher ----------------------------------------------------------
template <int D, typename T, bool CAUSAL, bool DROP = false>
static hipError_t launch(const FwdParams& p, hipStream_t s) {
  using C = FwdCfg<D>;
  const int grid = (CAUSAL && p.pair ? (p.nq_tiles + 1) / 2 : p.nq_tiles) * p.B * p.H;
  return launch_kernel<fa_fwd_kernel<D, T, CAUSAL, DROP>>(grid, C::NT, C::LDS_BYTES, s, p);
}

hipError_t launch_fwd_v2(FwdParams p, int dtype, int causal, hipStream_t s);  // fa_fwd_v2.hip
hipError_t launch_fwd_v3(FwdParams p, int dtype, int causal, hipStream_t s);  // fa_fwd_v3.hip
hipError_t launch_fwd_v4(FwdParams p, int D, int dtype, int causal, hipStream_t s);  // fa_fwd_v4.hip

hipError_t launch_fwd(FwdParams p, int D, int dtype, int causal, hipStream_t s) {
  const int impl = fwd_family(D, dtype, p.B, p.H, p.Sq, p.Sk, causal != 0, p.vl.cu_q != nullptr, p.drop.thresh != 0);
  if (impl == 2) return launch_fwd_v2(p, dtype, causal, s);
  if (impl == 3) return launch_fwd_v3(p, dtype, causal, s);
  if (impl == 4) return launch_fwd_v4(p, D, dtype, causal, s);
  p.nq_tiles = (p.Sq + 127) / 128;
  p.pair = want_pairs(causal != 0, p.nq_tiles, (long)p.B * p.H);
#define FA_GO(DD, TT)                                                                           \
  (p.drop.thresh ? (causal ? launch<DD, TT, true, true>(p, s) : launch<DD, TT, false, true>(p, s)) \
                 : (causal ? launch<DD, TT, true>(p, s) : launch<DD, TT, false>(p, s)))
  if (D == 64) return dtype == 1 ? FA_GO(64, BF16) : FA_GO(64, FP16);
  if (D == 128) return dtype == 1 ? FA_GO(128, BF16) : FA_GO(128, FP16);
#undef FA_GO
  return hipErrorInvalidValue;
}

template <int D, typename T, bool GQA, bool SOFTCAP, bool ALIBI, bool SINK>
static hipError_t launch_mod(const FwdParams& p, const ScoreMod& sm, hipStream_t s) {
  using C = FwdCfg<D>;
  return launch_kernel<fa_fwd_mod_kernel<D, T, GQA, SOFTCAP, ALIBI, SINK>>(p.nq_tiles * p.B * p.H, C::NT, C::LDS_BYTES, s, p,
                                                                           sm.wl, sm.wr, sm.group, sm.softcap, sm.slopes, sm.slopes_bstride, sm.sinks);
}

// Variant forward (fa_kernels.h ScoreMod): one workgroup per (batch, query head, 128-row tile).
hipError_t launch_fwd_mod(FwdParams p, int D, int dtype, const ScoreMod& sm, hipStream_t s) {
  p.nq_tiles = (p.Sq + 127) / 128;
  p.pair = 0;
#define FA_GO(DD, TT)                                                          \
  (sm.sinks           ? launch_mod<DD, TT, true, false, false, true>(p, sm, s)  \
   : sm.slopes        ? launch_mod<DD, TT, true, false, true, false>(p, sm, s)  \
   : sm.softcap > 0.f ? launch_mod<DD, TT, true, true, false, false>(p, sm, s)  \
   : sm.group         ? launch_mod<DD, TT, true, false, false, false>(p, sm, s) \
                      : launch_mod<DD, TT, false, false, false, false>(p, sm, s))
  if (D == 64) return dtype == 1 ? FA_GO(64, BF16) : FA_GO(64, FP16);
  if (D == 128) return dtype == 1 ? FA_GO(128, BF16) : FA_GO(128, FP16);
#undef FA_GO
  return hipErrorInvalidValue;
}

}  // namespace fa
