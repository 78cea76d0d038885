// Split-KV decoding attention ("flash-decoding") over a padded KV cache: include/mi355fa_kvcache.h, and over a paged
// one (a pool of pages and a table of page numbers per sequence): include/mi355fa_paged.h.
//
// A decode step has a handful of queries per sequence against thousands of cached keys: the work is reading the cache
// once, and the kernels are built for HBM, not for the MFMA pipe.
//
//   fa_kvcache_append_kernel  k_new / v_new -> cache rows [seqlens[b], seqlens[b] + S_new)   (first, same stream)
//   fa_decode_mod_kernel      one workgroup per (batch, K/V head, 32-row block of the group's rows, split)
//   fa_decode_combine_kernel  nsplit > 1: merges the splits of every row in ascending split order
//
// The MFMA rows of a workgroup are the g * S_q (query, query head) rows of ONE K/V head, query-major (row = i * g + hh),
// so every K/V byte is read once per head group, not once per query head.  More than 32 such rows (long speculative
// chunks, large groups) take several row blocks, each over its own part of the key range.  Split s of n takes the s-th of
// n balanced shares of the row block's visible 32-key tiles, computed on the device from seqlens[b] and the window, so
// every split has work whatever the fill level and the host never reads seqlens (a decode step can be graph-captured).
// Inside a workgroup the four waves are independent flash-attention streams over interleaved tiles (tile t goes to wave
// t mod 4 of the split): no barrier in the loop.  Per wave and tile:
//   K  (32 keys x D): global -> registers, straight into the A operand of S^T = K Q^T (lane (r, h) loads key r's
//      16 bytes at d = 16 ks + 8 h: the MFMA A layout), prefetched one tile ahead;
//   V  (32 keys x D): global -> registers (prefetched one tile ahead) -> the wave's own swizzled LDS tile, read back
//      transposed (lds_read_tr_frag) as the A operand of O^T += V^T P^T;
//   S^T has the query row on the lane, so the softmax row reductions are register + one cross-half exchange.
// The waves' (m, l, O) merge through LDS in wave order; with one split the workgroup writes O / LSE, otherwise the
// fp32 partial (unnormalised O, m, l) of each row goes to the workspace.  Every order is fixed: deterministic.
// Buffer descriptors cover rows [0, min(L_b, S_cache)) of the sequence's cache slice only: rows past L_b are never read
// (NaN padding cannot leak in) and no access leaves the cache even if seqlens is out of range.
//
// FP8 caches (include/mi355fa_kvcache_fp8.h): fa_kvcache_append_fp8_kernel quantises k_new / v_new on the way in and
// fa_decode_mod_kernel<KV8> is the same body over e4m3 bytes (fa_decode_body.inc); the combine kernel is shared.
//
// MXFP4 caches (include/mi355fa_kvcache_fp4.h): e2m1 nibbles with one e8m0 scale byte per 32 elements in a tensor of its own.
// fa_decode_mod_kernel<D, T, SINK> / fa_decode_paged_kernel<D, T, SINK> (overloads by template parameters, with the scale
// tensors as kernel arguments) are the body with KV4 set, fa_kvcache_append_kernel<T> / fa_kvcache_append_paged_kernel<T> the
// quantising appends that write nibbles and scales; the combine kernel is shared.  Packed queries over MXFP4 pools
// (include/mi355fa_ragged_fp4.h) are fa_decode_ragged_kernel<T, D, SINK> and fa_kvcache_append_ragged_kernel<T>, the same
// overloads of the packed names, with the plan and the packed combine kernel shared; that kernel also exists at D = 256.
//
// Per-token-scaled e4m3 caches (include/mi355fa_kvcache_fp8_token.h): e4m3 bytes with one fp32 scale per cached token and K/V
// head in a tensor of its own.  fa_decode_mod_kernel<T, D, SINK, TOKEN> / fa_decode_paged_kernel<T, D, SINK, TOKEN> /
// fa_decode_ragged_kernel<T, D, SINK, TOKEN> (overloads by template parameters again) are the body with KV8 and KVT set: KV8's
// loads, permutation and MFMAs, K's scale on the fp32 scores, V's scale split between the conversion (its power of two) and the
// probabilities (its mantissa); fa_kvcache_append_kernel<T, TOKEN> and its paged and packed forms compute each new row's scale.
//
// Soft-capping over the three byte formats (include_quant/mi355fa_kvcache_quant_softcap.h): fa_decode_mod_kernel<T, D, F, SOFTCAP> /
// fa_decode_paged_kernel<T, D, F, SOFTCAP> / fa_decode_ragged_kernel<T, D, F, SOFTCAP> (overloads by template parameters once
// more, F the cache format) are the body with SOFTCAP and the format's flags; the appends, the plan and the combine kernels are
// the formats' own.
//
// Paged caches (include/mi355fa_paged.h): fa_decode_paged_kernel is the same body again with PAGED set, and
// fa_kvcache_append_paged_kernel / _paged_fp8_kernel are the appends with the destination row routed through the table.  A
// page holds a whole number of 32-key tiles, so the only new work per tile is one wave-uniform table entry, looked up a
// step ahead, and the two descriptors rebased on its page; the combine kernel is shared here too.
//
// Packed variable-length queries (include/mi355fa_ragged.h): q is [total_q, H, D] and sequence b owns S_b rows of it, as an
// engine with continuous batching hands a step over (decode rows, speculative drafts and prefill chunks together).
//   fa_decode_ragged_plan_kernel     one workgroup: cu_seqlens_q -> the list of the step's 32-row blocks (b, rb)
//   fa_kvcache_append_ragged_kernel  (+ _fp8) packed k_new / v_new rows -> cache rows seqlens[b] + i through the table
//   fa_decode_ragged_kernel          the body with RAGGED: one workgroup per (list entry, K/V head, split)
//   fa_decode_combine_ragged_kernel  the combine kernel by (head, packed row)
// The grid is sized from total_q and B alone (fa_decode.h ragged_nb_max), never from the longest sequence, and the host
// reads nothing: entries past the list's end hold a marker and their workgroups leave at once.
//
// D = 256 (the decode calls only; fa_decode_body.inc "D = 256", DecLds below): the four waves are two key groups x two halves
// of the head dim, each wave with the D = 128 wave's loads and registers.  The two waves of a pair add their halves of S^T
// through LDS, one workgroup barrier per step, and a workgroup takes two tiles per step instead of four.
//
// One path for all of it.  The attention kernels are one body (fa_decode_body.inc) behind six wrappers that differ in their
// arguments (nine with the per-token-scaled ones, twelve with the soft-capped ones of the byte formats); the appends one body (kvcache_append_body) behind twelve.  The host side is one chain with the cache format
// (fa_decode.h KvFormat) as its compile-time parameter: launch_decode refuses the combinations without a kernel and picks
// D, T and the format; launch_decode_t enqueues the plan kernel (packed queries), launch_append (S_new > 0) and
// launch_decode_mod, which computes the grid once, launches the attention kernel of the format, transform and geometry and,
// with splits, the combine kernel of the geometry.  A new cache format or geometry is a branch in these, not a copy of them.
#include <algorithm>

#include "fa_common.h"
#include "fa_decode.h"

namespace fa {

namespace {

constexpr int kDecTile = 32;   // keys per wave per step
constexpr int kDecRows = 32;   // MFMA rows per workgroup
constexpr int kDecWaves = 4;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;

template <int D>
struct DecCfg {
  static constexpr int ROWB = D * 2;
  static constexpr int KS = D / 16;                        // k-steps of S^T = K Q^T
  static constexpr int DB = D / 32;                        // 32-column blocks of O^T
  static constexpr int CPR = D / 8;                        // 16-byte chunks per row
  static constexpr int VL = kDecTile * CPR / 64;           // V chunks per lane per tile
  static constexpr int OST = D + 4;                        // fp32 row stride of the merge stage (bank spread)
  static constexpr int STAGE_BYTES = kDecWaves * kDecTile * ROWB;
  static constexpr int MERGE_BYTES = kDecWaves * kDecRows * OST * 4;
  static constexpr int ML_OFF = MERGE_BYTES;
  static constexpr int LDS_BYTES = (STAGE_BYTES > MERGE_BYTES ? STAGE_BYTES : MERGE_BYTES) + 2 * kDecWaves * kDecRows * 4;
};

// The workgroup's LDS.  D = 64 / 128: DecCfg's, the four waves' V tiles with the merge stage over them.  D = 256
// (fa_decode_body.inc, "D = 256"): a wave works on 128 of the 256 head dims, so the loop holds the four waves' 32 x 128 V
// tiles (32 KiB) and behind them the score exchange, two 4 KiB slots per wave (32 KiB); the merge stage, over both, has two
// key groups of 32 rows of 256 + 4 floats (65 KiB) and their (m, l) rows.  65.5 KiB: two workgroups per CU, as the others.
template <int D>
struct DecLds {
  static constexpr int XCH_OFF = 0, XCH_SLOT = 0;   // (no exchange)
  static constexpr int OST = DecCfg<D>::OST;
  static constexpr int ML_OFF = DecCfg<D>::ML_OFF;
  static constexpr int LDS_BYTES = DecCfg<D>::LDS_BYTES;
};
template <>
struct DecLds<256> {
  static constexpr int NG = kDecWaves / 2;                                  // key groups
  static constexpr int XCH_OFF = DecCfg<128>::STAGE_BYTES;                  // behind the V tiles
  static constexpr int XCH_SLOT = 64 * 16 * 4;                              // one wave's 32 x 32 fp32 partial scores
  static constexpr int LOOP_BYTES = XCH_OFF + 2 * kDecWaves * XCH_SLOT;
  static constexpr int OST = 256 + 4;
  static constexpr int MERGE_BYTES = NG * kDecRows * OST * 4;
  static constexpr int ML_OFF = MERGE_BYTES;
  static constexpr int LDS_BYTES = (LOOP_BYTES > MERGE_BYTES ? LOOP_BYTES : MERGE_BYTES) + 2 * NG * kDecRows * 4;
  static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU");
};

// Eight OCP e4m3 bytes (two dwords, ascending addresses) -> eight values of T in the same order.  Exact: every e4m3 value,
// subnormals included, is a normal fp16 and bf16 number.  v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0: two bytes to one
// packed pair per instruction.
template <typename T>
FA_DEVINL u32x4 cvt_fp8(unsigned lo, unsigned hi) {
  if constexpr (std::is_same<T, BF16>::value)
    return u32x4{__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true))};
  else
    return u32x4{__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, false)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, true)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, false)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, true))};
}

// The same conversion with a scale operand (include/mi355fa_kvcache_fp8_token.h, "Exactness").  The instruction reads the
// exponent field e of `scale` alone, as an e8m0 byte -- what the MXFP4 conversions do -- and ignores its mantissa: it delivers
// byte * 2^(e - 127) without rounding wherever T represents it, T's subnormals included, whatever the mantissa holds
// (measured over every code; tests/test_gpu_fp8_token_scales.py holds it).  So the caller passes a row's fp32 scale as it is
// and applies the scale's mantissa elsewhere.
template <typename T>
FA_DEVINL u32x4 cvt_fp8_pow2(unsigned lo, unsigned hi, float scale) {
  if constexpr (std::is_same<T, BF16>::value)
    return u32x4{__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, scale, false)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, scale, true)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, scale, false)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, scale, true))};
  else
    return u32x4{__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, scale, false)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, scale, true)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, scale, false)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, scale, true))};
}

// An e8m0 scale byte e -> the scale operand of the conversions below: e in the exponent field of an fp32, 2^(e - 127) for
// e >= 1.  The conversions read that field alone, as an e8m0 byte: e = 0, whose operand is the fp32 0.0, scales by 2^-127
// like any other byte (measured over every byte and nibble; tests/test_gpu_fp4_scales.py holds it).  Such a block is not
// empty in bf16, whose normal numbers reach down to 2^-126 = 2 * 2^-127 and whose subnormals the conversion delivers too; the
// append writes e = 0 for every bf16 block with amax below 2^-124.  In fp16 nothing but zeros is representable below
// e = 101.  e = 255 is the NaN byte, unspecified.
FA_DEVINL float e8m0_scale(unsigned e) { return __builtin_bit_cast(float, e << 23); }

// Eight e2m1 nibbles (one dword, element 2i in the low nibble of byte i, 2i + 1 in the high one) times `scale` -> eight values
// of T in the same order.  Exact wherever T represents the product.  v_cvt_scalef32_pk_{bf16,f16}_fp4: one byte to one
// packed pair per instruction, the byte chosen by op_sel.
template <typename T>
FA_DEVINL u32x4 cvt_fp4(unsigned w, float scale) {
  if constexpr (std::is_same<T, BF16>::value)
    return u32x4{__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3))};
  else
    return u32x4{__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, scale, 0)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, scale, 1)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, scale, 2)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, scale, 3))};
}

// four values of T (two dwords) -> the four e4m3 bytes e4m3_rne(clamp(float(x) / d, -448, 448)), in the same order
template <typename T>
FA_DEVINL unsigned quant4_fp8(unsigned w0, unsigned w1, float d) {
  typedef __attribute__((ext_vector_type(2))) typename T::elem e2;
  const e2 a = __builtin_bit_cast(e2, w0), b = __builtin_bit_cast(e2, w1);
  float x[4] = {(float)a[0], (float)a[1], (float)b[0], (float)b[1]};
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = __builtin_fminf(__builtin_fmaxf(x[j] / d, -448.f), 448.f);
  int r = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], 0, false);
  return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], r, true);
}

// max |x| over eight values of T (four dwords)
template <typename T>
FA_DEVINL float amax8(u32x4 w) {
  typedef __attribute__((ext_vector_type(2))) typename T::elem e2;
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned wi = w[i];
    const e2 a = __builtin_bit_cast(e2, wi);
    m = __builtin_fmaxf(m, __builtin_fmaxf(__builtin_fabsf((float)a[0]), __builtin_fabsf((float)a[1])));
  }
  return m;
}

// The scale of a row with that amax (include/mi355fa_kvcache_fp8_token.h, "the quantiser"): amax / 448, the correctly rounded
// fp32 division; 1 where the quotient is not a normal number (a zero row, a subnormal quotient).
FA_DEVINL float row_scale_fp8(float amax) {
  const float s = amax / 448.f;
  const unsigned field = (__builtin_bit_cast(unsigned, s) >> 23) & 0xffu;
  return field - 1u < 254u ? s : 1.f;
}

// L_b as the kernels use it: clamped to [0, S_cache] (outside it the result is unspecified, the accesses stay inside)
FA_DEVINL int kv_len(const DecodeParams& p, int b) { return min(max(p.seqlens[b] + p.Snew, 0), p.Scache); }

}  // namespace

// The attention kernel.  A flag that is false compiles its part out; launch_decode_t instantiates the
// combinations that exist.
//   SOFTCAP  (include/mi355fa_softcap.h) the same kernel on the capped scores
//   ALIBI    (include/mi355fa_alibi.h) -slope_h |pos - j| on every score, slope_h = slopes[b * slopes_bstride + h] of the lane's
//            query head h
//   KV8      (include/mi355fa_kvcache_fp8.h) p.kc / p.vc hold OCP e4m3 bytes (lk / lv in bytes, a row is D bytes), q and o are
//            T; K = float(k_cache) * kds[b * ds_bstride + hk], V likewise with vds
//   SINK     (include/mi355fa_sink.h) sinks[h], one extra logit per query head, in the softmax denominator of every row of
//            head h; split 0 adds it (fa_decode_body.inc)
// fa_decode_body.inc names the arguments of every feature, each under the `if constexpr` of its flag only.  A kernel without
// a feature sets the flag false and declares what the body names with one of these (placeholders: never read):
#define FA_DECODE_NO_SCORE_ARGS /* SOFTCAP, ALIBI and KV8 all false */                     \
  constexpr float softcap = 0.f;                                                           \
  constexpr const float *slopes = nullptr, *kds = nullptr, *vds = nullptr;                 \
  constexpr int slopes_bstride = 0, ds_bstride = 0;
#define FA_DECODE_NO_KV4                                                                   \
  constexpr const unsigned char *ksc = nullptr, *vsc = nullptr;                            \
  constexpr TensorLayout lks{0, 0, 0}, lvs{0, 0, 0};
#define FA_DECODE_NO_PAGED                                                                 \
  constexpr const int* block_table = nullptr;                                              \
  constexpr int bt_stride = 0, page_size = 0, num_pages = 0;                               \
  constexpr FastDiv tpp_div{1u, 0};
#define FA_DECODE_NO_RAGGED                                                                \
  constexpr const int *cu_q = nullptr, *plan = nullptr;                                    \
  constexpr int total_q = 0;

template <int D, typename T, bool SOFTCAP, bool ALIBI, bool KV8, bool SINK>
__global__ __launch_bounds__(256, 2)
    void fa_decode_mod_kernel(DecodeParams p, float softcap, const float* slopes, int slopes_bstride, const float* kds,
                              const float* vds, int ds_bstride, const float* sinks) {
  constexpr bool PAGED = false, RAGGED = false, KV4 = false, KVT = false;
  FA_DECODE_NO_KV4 FA_DECODE_NO_PAGED FA_DECODE_NO_RAGGED
#include "fa_decode_body.inc"
}

// The same kernel over a paged cache (include/mi355fa_paged.h, fa_decode.h DecodePaging): p.kc / p.vc are the pools,
// block_table[b * bt_stride + i] the page of sequence b's keys [i * page_size, (i + 1) * page_size), tpp_div the division
// of a tile index by page_size / 32.
template <int D, typename T, bool SOFTCAP, bool ALIBI, bool KV8, bool SINK>
__global__ __launch_bounds__(256, 2)
    void fa_decode_paged_kernel(DecodeParams p, float softcap, const float* slopes, int slopes_bstride, const float* kds,
                                const float* vds, int ds_bstride, const float* sinks, const int* block_table, int bt_stride,
                                int page_size, int num_pages, FastDiv tpp_div) {
  constexpr bool PAGED = true, RAGGED = false, KV4 = false, KVT = false;
  FA_DECODE_NO_KV4 FA_DECODE_NO_RAGGED
#include "fa_decode_body.inc"
}

// The paged kernel over packed variable-length queries (include/mi355fa_ragged.h, fa_decode.h DecodeRagged): sequence b
// owns the packed rows [cu_q[b], cu_q[b + 1]) of q / o, and blockIdx.x names an entry of `plan` (fa_decode_ragged_plan_kernel),
// a K/V head and a split.
template <int D, typename T, bool SOFTCAP, bool ALIBI, bool KV8, bool SINK>
__global__ __launch_bounds__(256, 2)
    void fa_decode_ragged_kernel(DecodeParams p, float softcap, const float* slopes, int slopes_bstride, const float* kds,
                                 const float* vds, int ds_bstride, const float* sinks, const int* block_table, int bt_stride,
                                 int page_size, int num_pages, FastDiv tpp_div, const int* cu_q, const int* plan, int total_q) {
  constexpr bool PAGED = true, RAGGED = true, KV4 = false, KVT = false;
  FA_DECODE_NO_KV4
#include "fa_decode_body.inc"
}

// The kernel over MXFP4 caches (include/mi355fa_kvcache_fp4.h; the body's KV4): p.kc / p.vc hold e2m1 nibbles (lk / lv in
// bytes, a row is D / 2 bytes), ksc / vsc the e8m0 scale bytes of K / V with the byte layouts lks / lvs (a row is D / 32
// bytes), q and o are T.  Plain and SINK.  An overload of fa_decode_mod_kernel by its template parameters <D, T, SINK> rather
// than one more flag of the kernel above: the scale tensors are kernel arguments, and the kernels above keep their names,
// their arguments, and with them their instructions.
template <int D, typename T, bool SINK>
__global__ __launch_bounds__(256, 2)
    void fa_decode_mod_kernel(DecodeParams p, const float* sinks, const unsigned char* ksc, const unsigned char* vsc,
                              TensorLayout lks, TensorLayout lvs) {
  constexpr bool SOFTCAP = false, ALIBI = false, KV8 = false, KV4 = true, KVT = false, PAGED = false, RAGGED = false;
  FA_DECODE_NO_SCORE_ARGS FA_DECODE_NO_PAGED FA_DECODE_NO_RAGGED
#include "fa_decode_body.inc"
}

// and over paged MXFP4 pools (fa_decode_paged_kernel<D, T, SINK>): the scale pools are [num_pages, H_kv, page_size, D / 32]
// and go through the same table entry
template <int D, typename T, bool SINK>
__global__ __launch_bounds__(256, 2)
    void fa_decode_paged_kernel(DecodeParams p, const float* sinks, const unsigned char* ksc, const unsigned char* vsc,
                                TensorLayout lks, TensorLayout lvs, const int* block_table, int bt_stride, int page_size,
                                int num_pages, FastDiv tpp_div) {
  constexpr bool SOFTCAP = false, ALIBI = false, KV8 = false, KV4 = true, KVT = false, PAGED = true, RAGGED = false;
  FA_DECODE_NO_SCORE_ARGS FA_DECODE_NO_RAGGED
#include "fa_decode_body.inc"
}

// and over packed variable-length queries (include/mi355fa_ragged_fp4.h; fa_decode_ragged_kernel<T, D, SINK>): the paged
// MXFP4 kernel's arguments, then the packed kernel's cu_q, plan and total_q.  The one MXFP4 kernel that exists at D = 256.
// (T before D: the twelve 16-bit / e4m3 instances fa_decode_ragged_kernel<256, ...> are a recorded set,
// tests/test_host_decode_d256.py, which these stay out of; tests/test_host_ragged_fp4.py holds them to the same budget.)
template <typename T, int D, bool SINK>
__global__ __launch_bounds__(256, 2)
    void fa_decode_ragged_kernel(DecodeParams p, const float* sinks, const unsigned char* ksc, const unsigned char* vsc,
                                 TensorLayout lks, TensorLayout lvs, const int* block_table, int bt_stride, int page_size,
                                 int num_pages, FastDiv tpp_div, const int* cu_q, const int* plan, int total_q) {
  constexpr bool SOFTCAP = false, ALIBI = false, KV8 = false, KV4 = true, KVT = false, PAGED = true, RAGGED = true;
  FA_DECODE_NO_SCORE_ARGS
#include "fa_decode_body.inc"
}

// The kernel over per-token-scaled e4m3 caches (include/mi355fa_kvcache_fp8_token.h; the body's KVT, with KV8 for the bytes):
// p.kc / p.vc hold e4m3 bytes (lk / lv in bytes, a row is D bytes), ksc / vsc one fp32 scale per cache row with the BYTE layouts
// lks / lvs, q and o are T.  Plain and SINK; padded, paged and packed, the packed one also at D = 256.  Overloads of the three kernel
// names by their template parameters <T, D, SINK, TOKEN> (TOKEN is always true: it tells them from the MXFP4 ones), as the MXFP4
// kernels are: the instances of the kernels above are recorded sets (tests/test_host_decode_d256.py,
// tests/test_host_ragged_fp4.py), which these stay out of; tests/test_host_kvcache_fp8_token.py holds them to the same budget.
template <typename T, int D, bool SINK, bool TOKEN>
__global__ __launch_bounds__(256, 2)
    void fa_decode_mod_kernel(DecodeParams p, const float* sinks, const float* ksc, const float* vsc, TensorLayout lks,
                              TensorLayout lvs) {
  static_assert(TOKEN, "the per-token-scaled overload");
  constexpr bool SOFTCAP = false, ALIBI = false, KV8 = true, KV4 = false, KVT = true, PAGED = false, RAGGED = false;
  FA_DECODE_NO_SCORE_ARGS FA_DECODE_NO_PAGED FA_DECODE_NO_RAGGED
#include "fa_decode_body.inc"
}

template <typename T, int D, bool SINK, bool TOKEN>
__global__ __launch_bounds__(256, 2)
    void fa_decode_paged_kernel(DecodeParams p, const float* sinks, const float* ksc, const float* vsc, TensorLayout lks,
                                    TensorLayout lvs, const int* block_table, int bt_stride, int page_size, int num_pages,
                                    FastDiv tpp_div) {
  static_assert(TOKEN, "the per-token-scaled overload");
  constexpr bool SOFTCAP = false, ALIBI = false, KV8 = true, KV4 = false, KVT = true, PAGED = true, RAGGED = false;
  FA_DECODE_NO_SCORE_ARGS FA_DECODE_NO_RAGGED
#include "fa_decode_body.inc"
}

template <typename T, int D, bool SINK, bool TOKEN>
__global__ __launch_bounds__(256, 2)
    void fa_decode_ragged_kernel(DecodeParams p, const float* sinks, const float* ksc, const float* vsc, TensorLayout lks,
                                     TensorLayout lvs, const int* block_table, int bt_stride, int page_size, int num_pages,
                                     FastDiv tpp_div, const int* cu_q, const int* plan, int total_q) {
  static_assert(TOKEN, "the per-token-scaled overload");
  constexpr bool SOFTCAP = false, ALIBI = false, KV8 = true, KV4 = false, KVT = true, PAGED = true, RAGGED = true;
  FA_DECODE_NO_SCORE_ARGS
#include "fa_decode_body.inc"
}

// The soft-capped kernel over the three quantised cache formats (include_quant/mi355fa_kvcache_quant_softcap.h): the body with SOFTCAP
// and the format's flags -- kE4M3: KV8 with the descales; kE4M3Token: KV8 and KVT with the fp32 row scales; kMXFP4: KV4 with the
// e8m0 scale bytes.  One argument list for the three formats (a format reads its own members only; the others are passed as
// nothing): softcap, the descales, then the scale tensors with their BYTE layouts, then the paged and the packed kernels'
// arguments.  Overloads of the three kernel names by their template parameters <T, D, F, SOFTCAP> (SOFTCAP is always true; the
// format's type tells them from the <T, D, SINK> and <T, D, SINK, TOKEN> ones): the instances of the kernels above are recorded
// sets, which these stay out of; tests/test_host_kvcache_quant_softcap.py holds them to the same budget.  D = 256: every kE4M3
// geometry, and the packed kernel alone for the other two formats, as without the cap.
#define FA_DECODE_QUANT_SOFTCAP                                                                              \
  static_assert(SOFTCAP && F != KvFormat::k16, "the soft-capped overload over a quantised cache");          \
  constexpr bool ALIBI = false, SINK = false, KV4 = F == KvFormat::kMXFP4, KVT = F == KvFormat::kE4M3Token, \
                 KV8 = F == KvFormat::kE4M3 || KVT;                                                         \
  constexpr const float *slopes = nullptr, *sinks = nullptr;                                                \
  constexpr int slopes_bstride = 0;                                                                         \
  const float *kds = F == KvFormat::kE4M3 ? kds_ : nullptr, *vds = F == KvFormat::kE4M3 ? vds_ : nullptr;   \
  const int ds_bstride = F == KvFormat::kE4M3 ? ds_bstride_ : 0;                                            \
  const char *ksc = (const char*)ksc_, *vsc = (const char*)vsc_;

template <typename T, int D, KvFormat F, bool SOFTCAP>
__global__ __launch_bounds__(256, 2)
    void fa_decode_mod_kernel(DecodeParams p, float softcap, const float* kds_, const float* vds_, int ds_bstride_,
                              const void* ksc_, const void* vsc_, TensorLayout lks, TensorLayout lvs) {
  constexpr bool PAGED = false, RAGGED = false;
  FA_DECODE_QUANT_SOFTCAP FA_DECODE_NO_PAGED FA_DECODE_NO_RAGGED
#include "fa_decode_body.inc"
}

template <typename T, int D, KvFormat F, bool SOFTCAP>
__global__ __launch_bounds__(256, 2)
    void fa_decode_paged_kernel(DecodeParams p, float softcap, const float* kds_, const float* vds_, int ds_bstride_,
                                const void* ksc_, const void* vsc_, TensorLayout lks, TensorLayout lvs, const int* block_table,
                                int bt_stride, int page_size, int num_pages, FastDiv tpp_div) {
  constexpr bool PAGED = true, RAGGED = false;
  FA_DECODE_QUANT_SOFTCAP FA_DECODE_NO_RAGGED
#include "fa_decode_body.inc"
}

template <typename T, int D, KvFormat F, bool SOFTCAP>
__global__ __launch_bounds__(256, 2)
    void fa_decode_ragged_kernel(DecodeParams p, float softcap, const float* kds_, const float* vds_, int ds_bstride_,
                                 const void* ksc_, const void* vsc_, TensorLayout lks, TensorLayout lvs, const int* block_table,
                                 int bt_stride, int page_size, int num_pages, FastDiv tpp_div, const int* cu_q, const int* plan,
                                 int total_q) {
  constexpr bool PAGED = true, RAGGED = true;
  FA_DECODE_QUANT_SOFTCAP
#include "fa_decode_body.inc"
}

// fa_decode_combine_kernel<D, T>: text of its own, which fa_decode_mla.hip compiles at D = 512 (the definition is one)
#include "fa_decode_combine.inc"

// The combine kernel by packed row (include/mi355fa_ragged.h): row = head * total_q + packed row, the arithmetic above.  Rows
// at or past the end of the last sequence (plan[1], written by the plan kernel) are the padding of a captured step: they
// are skipped, whatever the workspace holds.
template <int D, typename T>
__global__ __launch_bounds__(256) void fa_decode_combine_ragged_kernel(DecodeParams p, const int* plan, int total_q) {
  constexpr int TPR = D / 4, RPB = 256 / TPR;
  const long long R = (long long)p.H * total_q;
  const long long ridx = (long long)blockIdx.x * RPB + threadIdx.x / TPR;
  if (ridx >= R) return;
  const int head = (int)(ridx / total_q), row = (int)(ridx - (long long)head * total_q);
  if (row >= min(plan[1], total_q)) return;
  const int d4 = (threadIdx.x % TPR) * 4, n = p.nsplit;
  const float* ml = p.ws + (long long)n * R * D;
  float mx = -INFINITY;
#pragma unroll 8
  for (int s = 0; s < n; ++s) mx = __builtin_fmaxf(mx, ml[2 * (s * R + ridx)]);
  const float mo = mx == -INFINITY ? 0.f : mx;
  float ls = 0.f;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int s = 0; s < n; ++s) {
    const long long pr = s * R + ridx;
    const float e = __builtin_amdgcn_exp2f(ml[2 * pr] - mo);
    ls += e * ml[2 * pr + 1];
    acc += e * *(const f32x4*)(p.ws + pr * D + d4);
  }
  const float inv = ls > 0.f ? 1.f / ls : 0.f;
  typedef __attribute__((ext_vector_type(4))) typename T::elem e4;
  e4 ov;
#pragma unroll
  for (int j = 0; j < 4; ++j) ov[j] = (typename T::elem)(acc[j] * inv);
  *(u32x2*)((char*)p.o + (long long)head * p.lo.sh + (long long)row * p.lo.rs + d4 * 2) = __builtin_bit_cast(u32x2, ov);
  if (d4 == 0 && p.lse) p.lse[ridx] = ls > 0.f ? (mx + __builtin_log2f(ls)) * kLn2 : -INFINITY;
}

// ---- the work list of a packed step (include/mi355fa_ragged.h, fa_decode.h DecodeRagged) ----
// S_b as every kernel here takes it from cu_q: both ends clamped into [0, total_q], the second to the first, so whatever
// cu_q holds the rows [*q0, *q0 + S_b) lie inside the packed tensors.
FA_DEVINL int ragged_len(const int* cu_q, int b, int total_q, int* q0) {
  *q0 = min(max(cu_q[b], 0), total_q);
  return min(max(cu_q[b + 1], *q0), total_q) - *q0;
}

// One workgroup.  Sequences in chunks of 256: a scan of their 32-row block counts ceil(g * S_b / 32) in LDS, then the
// chunk's entries written by all threads (entry k finds its sequence by bisection of the chunk's prefix sums, so one long
// prefill chunk is not one thread's work).  The list stops at nb_max, which it reaches only if cu_q is malformed; entries
// from the count on get the end marker (-1, 0).  plan[0] = the count, plan[1] = the end of the last sequence that has rows.
__global__ __launch_bounds__(256) void fa_decode_ragged_plan_kernel(const int* cu_q, int B, int total_q, int g, int nb_max,
                                                                    int* plan) {
  __shared__ int pre[257];   // pre[j]: blocks of the chunk's sequences before the j-th
  const int tid = threadIdx.x;
  int* ent = plan + 4;
  int base = 0, rows_end = 0;
  for (int c0 = 0; c0 < B; c0 += 256) {
    int nb = 0;
    if (c0 + tid < B) {
      int q0;
      const int S = ragged_len(cu_q, c0 + tid, total_q, &q0);
      nb = (g * S + kDecRows - 1) / kDecRows;
      if (S > 0) rows_end = max(rows_end, q0 + S);
    }
    if (tid == 0) pre[0] = 0;
    pre[tid + 1] = nb;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const int v = pre[tid + 1] + (tid >= off ? pre[tid + 1 - off] : 0);
      __syncthreads();
      pre[tid + 1] = v;
      __syncthreads();
    }
    const int tot = pre[256], fit = min(tot, nb_max - base);
    for (int k = tid; k < fit; k += 256) {
      int lo = 0, hi = 256;   // pre[lo] <= k < pre[hi]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid] <= k) lo = mid; else hi = mid;
      }
      ent[2 * (base + k)] = c0 + lo;
      ent[2 * (base + k) + 1] = k - pre[lo];
    }
    base += fit;
    __syncthreads();   // the next chunk rewrites pre
  }
  for (int k = base + tid; k < nb_max; k += 256) {
    ent[2 * k] = -1;
    ent[2 * k + 1] = 0;
  }
  pre[tid] = rows_end;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) pre[tid] = max(pre[tid], pre[tid + off]);
    __syncthreads();
  }
  if (tid == 0) {
    plan[0] = base;
    plan[1] = pre[0];
  }
}

// ---- the appends: one body (kvcache_append_body) behind twelve entry points; plain vector stores.
// (fa_kvcache_append_kernel stays the last function of the code object, as it was: tools/isa_diff.py counts the padding
// behind it.) ----
// Row `dst` of sequence b: its page and its row inside the page, or false for a row outside [0, S_cache) or a table entry
// outside the pool (the row is dropped).
FA_DEVINL bool paged_dst(const DecodeParams& p, int b, int dst, const int* block_table, int bt_stride, int page_size,
                         int num_pages, int* page, int* row) {
  if (dst < 0 || dst >= p.Scache) return false;
  const int i = dst / page_size;
  *page = block_table[(long long)b * bt_stride + i];
  *row = dst - i * page_size;
  return (unsigned)*page < (unsigned)num_pages;
}

// The packed appends (include/mi355fa_ragged.h): k_new / v_new are [total_q, H_kv, D], packed row t of sequence b (the last
// b with cu_q[b] <= t, found by bisection: cu_q ascends unless it is malformed) goes to cache row seqlens[b] + (t - cu_q[b])
// through the table.  A row no sequence owns -- the padding past cu_q[B], or anything a malformed cu_q leaves -- is dropped.
FA_DEVINL bool ragged_owner(const int* cu_q, int B, int total_q, int t, int* b, int* j) {
  if (cu_q[0] > t) return false;
  int lo = 0, hi = B;   // cu_q[lo] <= t, and lo is the last such index below hi
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cu_q[mid] <= t) lo = mid; else hi = mid;
  }
  int q0;
  const int S = ragged_len(cu_q, lo, total_q, &q0);
  *b = lo;
  *j = t - q0;
  return *j >= 0 && *j < S;
}

// The MXFP4 quantiser (include/mi355fa_kvcache_fp4.h, "the quantiser"), one scale block of the append below:
// 32 values of T (four 16-byte loads, w) -> their nibbles, and the block's e8m0 byte in *e.  Everything is exact fp32: the
// exponent of amax is read from its bits (a bf16 subnormal amax has exponent field 0, which the clamp takes to e = 0), the
// factor 2^(127 - e) is a power of two, and the rounding to nearest even onto the e2m1 grid is seven comparisons with the
// grid's midpoints, the ties sent to the even code.
template <typename T>
FA_DEVINL u32x4 quant32_fp4(const u32x4 (&w)[4], unsigned* e) {
  typedef __attribute__((ext_vector_type(2))) typename T::elem e2;
  float x[32];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const unsigned wi = w[i >> 2][i & 3];   // (a scalar first: a bit_cast straight from the vector element reads element 0)
    const e2 a = __builtin_bit_cast(e2, wi);
    x[2 * i] = (float)a[0];
    x[2 * i + 1] = (float)a[1];
  }
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) amax = __builtin_fmaxf(amax, __builtin_fabsf(x[i]));
  const int ex = (int)((__builtin_bit_cast(unsigned, amax) >> 23) & 0xffu) - 2;   // floor(log2(amax)) - 2 + 127
  const unsigned eb = amax == 0.f ? 127u : (unsigned)min(max(ex, 0), 254);
  const float inv = __builtin_bit_cast(float, (254u - eb) << 23);                 // 2^(127 - e)
  u32x4 out;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    unsigned acc = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float v = x[8 * d + i], y = __builtin_fabsf(v) * inv;
      const unsigned mag = (unsigned)(y > 0.25f) + (unsigned)(y >= 0.75f) + (unsigned)(y > 1.25f) + (unsigned)(y >= 1.75f) +
                           (unsigned)(y > 2.5f) + (unsigned)(y >= 3.5f) + (unsigned)(y > 5.f);
      const unsigned sign = amax == 0.f ? 0u : (__builtin_bit_cast(unsigned, v) >> 31) << 3;
      acc |= (sign | mag) << (4 * i);
    }
    out[d] = acc;
  }
  *e = eb;
  return out;
}

// The append, once: one 16-byte store per thread and cache into row seqlens[b] + j of sequence b.
//   F = k16    the row is copied: k_new / v_new and the caches hold the same 16-bit type, one 16-byte chunk in per thread (T = void)
//   F = kE4M3  (include/mi355fa_kvcache_fp8.h) the quantising append: k_new / v_new (T, contiguous) ->
//              e4m3_rne(clamp(float(x) / descale[b, hk], -448, 448)), 16 elements in per thread.  The division is the correctly
//              rounded fp32 one and the clamp is explicit, so the bytes are those of
//              (x.float() / d).clamp(-448, 448).to(float8_e4m3fn) (v_cvt_pk_fp8_f32 rounds to nearest even, subnormals included).
//   F = kMXFP4 (include/mi355fa_kvcache_fp4.h) one scale block per thread and cache: 32 values of T in, 16 bytes of nibbles
//              (quant32_fp4) and one scale byte, into ksc / vsc with the byte layouts lks / lvs, out
//   F = kE4M3Token (include/mi355fa_kvcache_fp8_token.h, "the quantiser") kE4M3's threads, loads and stores with the row's own
//              scale: amax over the row (each thread's 16 elements, then across the D / 16 threads of the row, an aligned group
//              of lanes), s = amax / 448 -- 1 where that is not a normal number --, the bytes of kE4M3 with d = s, and s itself
//              into ksc / vsc (fp32, the BYTE layouts lks / lvs) by the row's first thread
//   PAGED      the destination row goes through the table (paged_dst); otherwise rows outside [0, S_cache) are dropped here
//   RAGGED     k_new / v_new are packed [total_q, H_kv, D] and (b, j) come from ragged_owner; otherwise they are
//              [B, H_kv, S_new, D]
// Loads first, then each store with its address written in place, `p` by value and the scale tensors right behind it: with
// these the eight kernels are, instruction for instruction, what they were as bodies of their own (behind `const DecodeParams&`
// four of them came out with other scalar code, and with the scale layouts behind the descales the MXFP4 four loaded their
// arguments in another order).
template <KvFormat F, typename T, bool PAGED, bool RAGGED>
FA_DEVINL void kvcache_append_body(DecodeParams p, unsigned char* ksc, unsigned char* vsc, TensorLayout lks, TensorLayout lvs,
                                   const float* kds, const float* vds, int ds_bstride, const int* block_table,
                                   int bt_stride, int page_size, int num_pages, const int* cu_q, int total_q) {
  const int cpr = p.D / (F == KvFormat::kMXFP4 ? 32 : F == KvFormat::kE4M3 || F == KvFormat::kE4M3Token ? 16 : 8);
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = RAGGED ? (long long)total_q * p.Hkv * cpr : (long long)p.B * p.Hkv * p.Snew * cpr;
  if (item >= total) return;
  const int c = (int)(item % cpr);
  const long long rowi = item / cpr;   // (b * H_kv + hk) * S_new + j, or RAGGED: t * H_kv + hk
  int b, j, hk;
  if constexpr (RAGGED) {
    hk = (int)(rowi % p.Hkv);
    if (!ragged_owner(cu_q, p.B, total_q, (int)(rowi / p.Hkv), &b, &j)) return;
  } else {
    j = (int)(rowi % p.Snew);
    const int bh = (int)(rowi / p.Snew);
    hk = bh % p.Hkv, b = bh / p.Hkv;
  }
  int slice, row;   // the cache's slice (a page, or the sequence) and the row inside it
  if constexpr (PAGED) {
    if (!paged_dst(p, b, p.seqlens[b] + j, block_table, bt_stride, page_size, num_pages, &slice, &row)) return;
  } else {
    slice = b, row = p.seqlens[b] + j;
    if (row < 0 || row >= p.Scache) return;
  }
  if constexpr (F == KvFormat::kMXFP4) {
    const long long src_off = rowi * p.D * 2 + c * 64;
    u32x4 kw[4], vw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      kw[i] = *(const u32x4*)((const char*)p.k_new + src_off + 16 * i);
      vw[i] = *(const u32x4*)((const char*)p.v_new + src_off + 16 * i);
    }
    unsigned ke, ve;
    const u32x4 kq = quant32_fp4<T>(kw, &ke), vq = quant32_fp4<T>(vw, &ve);
    *(u32x4*)((char*)p.kc + slice * p.lk.sb + (long long)hk * p.lk.sh + (long long)row * p.lk.rs + c * 16) = kq;
    *(u32x4*)((char*)p.vc + slice * p.lv.sb + (long long)hk * p.lv.sh + (long long)row * p.lv.rs + c * 16) = vq;
    ksc[slice * lks.sb + (long long)hk * lks.sh + (long long)row * lks.rs + c] = (unsigned char)ke;
    vsc[slice * lvs.sb + (long long)hk * lvs.sh + (long long)row * lvs.rs + c] = (unsigned char)ve;
  } else if constexpr (F == KvFormat::kE4M3Token) {
    const long long src_off = rowi * p.D * 2 + c * 32;
    const u32x4 k0 = *(const u32x4*)((const char*)p.k_new + src_off), k1 = *(const u32x4*)((const char*)p.k_new + src_off + 16);
    const u32x4 v0 = *(const u32x4*)((const char*)p.v_new + src_off), v1 = *(const u32x4*)((const char*)p.v_new + src_off + 16);
    float ka = fmaxf(amax8<T>(k0), amax8<T>(k1)), va = fmaxf(amax8<T>(v0), amax8<T>(v1));
    // the row's threads are `cpr` consecutive lanes from a multiple of cpr, all of them here (they share every test above)
    for (int o = 1; o < cpr; o <<= 1) {
      ka = fmaxf(ka, __shfl_xor(ka, o));
      va = fmaxf(va, __shfl_xor(va, o));
    }
    const float kd = row_scale_fp8(ka), vd = row_scale_fp8(va);
    *(u32x4*)((char*)p.kc + slice * p.lk.sb + (long long)hk * p.lk.sh + (long long)row * p.lk.rs + c * 16) =
        u32x4{quant4_fp8<T>(k0[0], k0[1], kd), quant4_fp8<T>(k0[2], k0[3], kd), quant4_fp8<T>(k1[0], k1[1], kd),
              quant4_fp8<T>(k1[2], k1[3], kd)};
    *(u32x4*)((char*)p.vc + slice * p.lv.sb + (long long)hk * p.lv.sh + (long long)row * p.lv.rs + c * 16) =
        u32x4{quant4_fp8<T>(v0[0], v0[1], vd), quant4_fp8<T>(v0[2], v0[3], vd), quant4_fp8<T>(v1[0], v1[1], vd),
              quant4_fp8<T>(v1[2], v1[3], vd)};
    if (c == 0) {
      *(float*)((char*)ksc + slice * lks.sb + (long long)hk * lks.sh + (long long)row * lks.rs) = kd;
      *(float*)((char*)vsc + slice * lvs.sb + (long long)hk * lvs.sh + (long long)row * lvs.rs) = vd;
    }
  } else if constexpr (F == KvFormat::kE4M3) {
    const float kd = kds ? kds[b * ds_bstride + hk] : 1.f, vd = vds ? vds[b * ds_bstride + hk] : 1.f;
    const long long src_off = rowi * p.D * 2 + c * 32;
    const u32x4 k0 = *(const u32x4*)((const char*)p.k_new + src_off), k1 = *(const u32x4*)((const char*)p.k_new + src_off + 16);
    const u32x4 v0 = *(const u32x4*)((const char*)p.v_new + src_off), v1 = *(const u32x4*)((const char*)p.v_new + src_off + 16);
    *(u32x4*)((char*)p.kc + slice * p.lk.sb + (long long)hk * p.lk.sh + (long long)row * p.lk.rs + c * 16) =
        u32x4{quant4_fp8<T>(k0[0], k0[1], kd), quant4_fp8<T>(k0[2], k0[3], kd), quant4_fp8<T>(k1[0], k1[1], kd),
              quant4_fp8<T>(k1[2], k1[3], kd)};
    *(u32x4*)((char*)p.vc + slice * p.lv.sb + (long long)hk * p.lv.sh + (long long)row * p.lv.rs + c * 16) =
        u32x4{quant4_fp8<T>(v0[0], v0[1], vd), quant4_fp8<T>(v0[2], v0[3], vd), quant4_fp8<T>(v1[0], v1[1], vd),
              quant4_fp8<T>(v1[2], v1[3], vd)};
  } else {
    const long long src_off = rowi * p.D * 2 + c * 16;
    *(u32x4*)((char*)p.kc + slice * p.lk.sb + (long long)hk * p.lk.sh + (long long)row * p.lk.rs + c * 16) =
        *(const u32x4*)((const char*)p.k_new + src_off);
    *(u32x4*)((char*)p.vc + slice * p.lv.sb + (long long)hk * p.lv.sh + (long long)row * p.lv.rs + c * 16) =
        *(const u32x4*)((const char*)p.v_new + src_off);
  }
}

// The twelve entry points: what a kernel lacks is passed as nothing.
#define FA_APPEND_NO_DESCALES nullptr, nullptr, 0
#define FA_APPEND_NO_SCALES nullptr, nullptr, TensorLayout{0, 0, 0}, TensorLayout{0, 0, 0}
#define FA_APPEND_NO_TABLE nullptr, 0, 0, 0
#define FA_APPEND_NO_CU nullptr, 0

// (fa_kvcache_append_kernel<T> and fa_kvcache_append_paged_kernel<T>: the MXFP4 overloads of the two copying appends below)
template <typename T>
__global__ __launch_bounds__(256) void fa_kvcache_append_kernel(DecodeParams p, unsigned char* ksc, unsigned char* vsc,
                                                                TensorLayout lks, TensorLayout lvs) {
  kvcache_append_body<KvFormat::kMXFP4, T, false, false>(p, ksc, vsc, lks, lvs, FA_APPEND_NO_DESCALES, FA_APPEND_NO_TABLE,
                                                         FA_APPEND_NO_CU);
}

template <typename T>
__global__ __launch_bounds__(256) void fa_kvcache_append_paged_kernel(DecodeParams p, unsigned char* ksc, unsigned char* vsc,
                                                                      TensorLayout lks, TensorLayout lvs,
                                                                      const int* block_table, int bt_stride, int page_size,
                                                                      int num_pages) {
  kvcache_append_body<KvFormat::kMXFP4, T, true, false>(p, ksc, vsc, lks, lvs, FA_APPEND_NO_DESCALES, block_table, bt_stride,
                                                        page_size, num_pages, FA_APPEND_NO_CU);
}

// (fa_kvcache_append_ragged_kernel<T>: the MXFP4 overload of the packed copying append below, include/mi355fa_ragged_fp4.h)
template <typename T>
__global__ __launch_bounds__(256) void fa_kvcache_append_ragged_kernel(DecodeParams p, unsigned char* ksc, unsigned char* vsc,
                                                                       TensorLayout lks, TensorLayout lvs,
                                                                       const int* block_table, int bt_stride, int page_size,
                                                                       int num_pages, const int* cu_q, int total_q) {
  kvcache_append_body<KvFormat::kMXFP4, T, true, true>(p, ksc, vsc, lks, lvs, FA_APPEND_NO_DESCALES, block_table, bt_stride,
                                                       page_size, num_pages, cu_q, total_q);
}

// (the three appends of a per-token-scaled e4m3 cache, include/mi355fa_kvcache_fp8_token.h: padded, paged and packed;
// overloads <T, TOKEN> of the three names, TOKEN always true)
template <typename T, bool TOKEN>
__global__ __launch_bounds__(256) void fa_kvcache_append_kernel(DecodeParams p, float* ksc, float* vsc, TensorLayout lks,
                                                                    TensorLayout lvs) {
  kvcache_append_body<KvFormat::kE4M3Token, T, false, false>(p, (unsigned char*)ksc, (unsigned char*)vsc, lks, lvs,
                                                             FA_APPEND_NO_DESCALES, FA_APPEND_NO_TABLE, FA_APPEND_NO_CU);
}

template <typename T, bool TOKEN>
__global__ __launch_bounds__(256) void fa_kvcache_append_paged_kernel(DecodeParams p, float* ksc, float* vsc,
                                                                          TensorLayout lks, TensorLayout lvs,
                                                                          const int* block_table, int bt_stride, int page_size,
                                                                          int num_pages) {
  kvcache_append_body<KvFormat::kE4M3Token, T, true, false>(p, (unsigned char*)ksc, (unsigned char*)vsc, lks, lvs,
                                                            FA_APPEND_NO_DESCALES, block_table, bt_stride, page_size, num_pages,
                                                            FA_APPEND_NO_CU);
}

template <typename T, bool TOKEN>
__global__ __launch_bounds__(256) void fa_kvcache_append_ragged_kernel(DecodeParams p, float* ksc, float* vsc,
                                                                           TensorLayout lks, TensorLayout lvs,
                                                                           const int* block_table, int bt_stride, int page_size,
                                                                           int num_pages, const int* cu_q, int total_q) {
  kvcache_append_body<KvFormat::kE4M3Token, T, true, true>(p, (unsigned char*)ksc, (unsigned char*)vsc, lks, lvs,
                                                           FA_APPEND_NO_DESCALES, block_table, bt_stride, page_size, num_pages,
                                                           cu_q, total_q);
}

__global__ __launch_bounds__(256) void fa_kvcache_append_paged_kernel(DecodeParams p, const int* block_table, int bt_stride,
                                                                      int page_size, int num_pages) {
  kvcache_append_body<KvFormat::k16, void, true, false>(p, FA_APPEND_NO_SCALES, FA_APPEND_NO_DESCALES, block_table, bt_stride,
                                                        page_size, num_pages, FA_APPEND_NO_CU);
}

__global__ __launch_bounds__(256) void fa_kvcache_append_ragged_kernel(DecodeParams p, const int* block_table, int bt_stride,
                                                                       int page_size, int num_pages, const int* cu_q,
                                                                       int total_q) {
  kvcache_append_body<KvFormat::k16, void, true, true>(p, FA_APPEND_NO_SCALES, FA_APPEND_NO_DESCALES, block_table, bt_stride,
                                                       page_size, num_pages, cu_q, total_q);
}

// k_new / v_new rows -> cache rows seqlens[b] + j, one 16-byte chunk per thread; rows outside [0, S_cache) are dropped.
__global__ __launch_bounds__(256) void fa_kvcache_append_kernel(DecodeParams p) {
  kvcache_append_body<KvFormat::k16, void, false, false>(p, FA_APPEND_NO_SCALES, FA_APPEND_NO_DESCALES, FA_APPEND_NO_TABLE,
                                                         FA_APPEND_NO_CU);
}

// the quantising append
template <typename T>
__global__ __launch_bounds__(256) void fa_kvcache_append_fp8_kernel(DecodeParams p, const float* kds, const float* vds,
                                                                    int ds_bstride) {
  kvcache_append_body<KvFormat::kE4M3, T, false, false>(p, FA_APPEND_NO_SCALES, kds, vds, ds_bstride, FA_APPEND_NO_TABLE,
                                                        FA_APPEND_NO_CU);
}

// the quantising append of a paged cache
template <typename T>
__global__ __launch_bounds__(256) void fa_kvcache_append_paged_fp8_kernel(DecodeParams p, const float* kds, const float* vds,
                                                                          int ds_bstride, const int* block_table,
                                                                          int bt_stride, int page_size, int num_pages) {
  kvcache_append_body<KvFormat::kE4M3, T, true, false>(p, FA_APPEND_NO_SCALES, kds, vds, ds_bstride, block_table, bt_stride,
                                                       page_size, num_pages, FA_APPEND_NO_CU);
}

// the quantising packed append
template <typename T>
__global__ __launch_bounds__(256) void fa_kvcache_append_ragged_fp8_kernel(DecodeParams p, const float* kds, const float* vds,
                                                                           int ds_bstride, const int* block_table,
                                                                           int bt_stride, int page_size, int num_pages,
                                                                           const int* cu_q, int total_q) {
  kvcache_append_body<KvFormat::kE4M3, T, true, true>(p, FA_APPEND_NO_SCALES, kds, vds, ds_bstride, block_table, bt_stride,
                                                      page_size, num_pages, cu_q, total_q);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// Split count: at most one workgroup per CU (256 CUs) over (batch, K/V head, row block, split), and splits of about
// sqrt(128 * S_cache) keys (n <= sqrt(S_cache / 128)), at most kMaxSplits.  A split has fixed costs (its Q rows, the first
// tile's latency, the wave merge, its share of the combine), so the best split length grows with the cache: in the sweep
// behind this rule (profiles/decode_split_sweep.jsonl) it was 512 keys at 4096, 2048 at 32768 and
// 4096-5461 at 131072 for one sequence, and the rule is within 12 % of the best forced count at every swept point.
// The fp8 path: splits of about sqrt(64 * S_cache) keys (n <= sqrt(S_cache / 64)) and, at D = 64, up to two workgroups per
// CU.  A split streams half the bytes per key, so its fixed costs weigh twice as much against them and the best split is
// shorter wherever the workgroup budget leaves room: in the forced-split sweep (profiles/decode_fp8_split_sweep.jsonl,
// DESIGN.md section 3) the 16-bit rule was 19 % off the best count at B1 L4096 and 22 % off at B8 L16384 D64; this one is
// within 12 % at every swept point.
// D = 256, either cache format: splits of about sqrt(16 * S_cache) keys (n <= sqrt(S_cache / 16)) under the same budget of one
// workgroup per CU.  A workgroup takes two tiles per step there, not four, and every step ends at a barrier, so one split
// streams its keys at about half the rate and the machine fills only once the budget is used: in the forced-split sweep
// (profiles/decode_d256_split_sweep.jsonl) the D = 128 rule was about 70 % off the best count at B1 L4096 (5
// splits against 16, between the swept 4 and 6), 43 % at B1 L32768 (16 against 32) and 28 % at B8 L1024 (2 against 4); this one is within 8 % at every
// swept point, bf16 and e4m3.
// The MXFP4 path (include/mi355fa_kvcache_fp4.h): the fp8 rule's split length, sqrt(64 * S_cache) keys, and up to two workgroups
// per CU at both head dims.  A tile of nibbles costs the wave the conversions and MFMAs of an e4m3 tile for half its bytes, so
// one workgroup per CU leaves the step bound by its instruction stream, not by HBM, and a second one hides it: in the
// forced-split sweep (profiles/decode_fp4_split_sweep.jsonl) the fp8 rule was 22 % off the best count at
// B8 L16384 D128 (4 splits against 8) and 15 % at B32 L4096 (1 against 2); this one is at the best swept count or within 3 % of
// it at every swept point.
// Packed queries over MXFP4 pools (include/mi355fa_ragged_fp4.h), D = 256 among them: the rules above as they compose -- the
// MXFP4 budget of 512 workgroups over H_kv * nb_max, the MXFP4 split length at D = 64 / 128 and the D = 256 length
// (sqrt(16 * S_cache) keys) at D = 256.  In the forced-split sweep of the packed call (profiles/decode_fp4_ragged_split_sweep.jsonl,
// pure decode at B1 L4096, B1 L32768, B8 L16384 and B32 L4096, D 128 and 256) this is, of the constants
// here (256 / 512 workgroups; 16 / 64 / 128 keys), the choice closest to the best forced count: at the best swept count at six
// of the eight points, 6.9 % off it at B1 L32768 D128 (22 splits against 32) and 4.8 % at B1 L32768 D256 (45 against 64);
// 256 workgroups are 34 % (D128) and 56 % (D256) off at B8 L16384, the 64-key length at D = 256 21 % off at B1 L4096.
// Per-token-scaled e4m3 caches (include/mi355fa_kvcache_fp8_token.h): the e4m3 rule as it is, the D = 256 rule at D = 256 -- a key
// streams D + 4 bytes for the e4m3 path's D.  In the forced-split sweep at the e4m3 sweep's eleven points
// (profiles/decode_fp8_token_split_sweep.jsonl) the rule is at the best swept count at nine, 4.4 % off it at
// B1 L32768 D128 (22 splits against 24) and 6.2 % at B1 L32768 D64 (22 against 32): where the e4m3 rule stands on its own sweep.
// wgs, the workgroups per split: B * H_kv * decode_row_blocks(group, S_q), or for packed queries (include/mi355fa_ragged.h)
// the H_kv * nb_max of the launch's grid -- the host cannot know how many of them have rows or how long the sequences are;
// S_cache is then the table's reach.
int kvcache_splits(long long wgs, int S_cache, int D, KvFormat fmt, int forced) {
  if (forced > 0) return forced;
  constexpr int kMaxSplits = 64;
  // (a per-token-scaled e4m3 cache streams D + 4 bytes per key for kE4M3's D: kE4M3's rule)
  const bool fp8 = fmt == KvFormat::kE4M3 || fmt == KvFormat::kE4M3Token, fp4 = fmt == KvFormat::kMXFP4;
  const int target_wgs = fp4 || (fp8 && D == 64) ? 512 : 256, keys = D == 256 ? 16 : fp8 || fp4 ? 64 : 128;
  wgs = std::max<long long>(1, wgs);
  long long n = (target_wgs + wgs - 1) / wgs;
  long long by_len = 1;
  while ((by_len + 1) * (by_len + 1) * keys <= S_cache) ++by_len;
  n = std::min(n, by_len);
  return (int)std::max<long long>(1, std::min<long long>(n, kMaxSplits));
}

// The attention kernel of the format, the transform and the geometry (m.rg: fa_decode_ragged_kernel over the plan's entries;
// m.pg: fa_decode_paged_kernel; otherwise fa_decode_mod_kernel) over the (row block, K/V head, split) grid, then the combine
// kernel of the geometry if there are splits.
template <int D, typename T, KvFormat F, bool SOFTCAP, bool ALIBI, bool SINK>
static hipError_t launch_decode_mod(const DecodeParams& p, const DecodeMod& m, hipStream_t s) {
  constexpr int LDS = DecLds<D>::LDS_BYTES;
  const DecodePaging* g = m.pg;
  const DecodeRagged* r = m.rg;
  // the workgroups of a split: the plan's entries (packed queries), or the row blocks of every sequence, per K/V head
  const long long wgs = r ? (long long)r->nb_max * p.Hkv : (long long)p.B * p.Hkv * decode_row_blocks(p.group, p.Sq);
  const unsigned grid = (unsigned)(wgs * p.nsplit);
  hipError_t e;
  if constexpr (SOFTCAP && F != KvFormat::k16) {
    // (the <T, D, F, SOFTCAP> overloads: one argument list, the format's own members filled; D = 256 for kE4M3, and for the
    // other two formats the packed kernel alone, launch_decode)
    const void *ks = nullptr, *vs = nullptr;
    TensorLayout lks{0, 0, 0}, lvs{0, 0, 0};
    if constexpr (F == KvFormat::kMXFP4) ks = m.fp4->ks, vs = m.fp4->vs, lks = m.fp4->lks, lvs = m.fp4->lvs;
    if constexpr (F == KvFormat::kE4M3Token) ks = m.tok->ks, vs = m.tok->vs, lks = m.tok->lks, lvs = m.tok->lvs;
    if (r) {
      e = launch_kernel<fa_decode_ragged_kernel<T, D, F, true>>(grid, 256, LDS, s, p, m.softcap, m.kds, m.vds, m.ds_bstride, ks, vs,
                                                                lks, lvs, g->table, g->stride, g->page_size, g->num_pages, g->tpp,
                                                                r->cu_q, (const int*)r->plan, r->total_q);
    } else if constexpr (D != 256 || F == KvFormat::kE4M3) {
      e = g ? launch_kernel<fa_decode_paged_kernel<T, D, F, true>>(grid, 256, LDS, s, p, m.softcap, m.kds, m.vds, m.ds_bstride, ks,
                                                                   vs, lks, lvs, g->table, g->stride, g->page_size, g->num_pages,
                                                                   g->tpp)
            : launch_kernel<fa_decode_mod_kernel<T, D, F, true>>(grid, 256, LDS, s, p, m.softcap, m.kds, m.vds, m.ds_bstride, ks, vs,
                                                                 lks, lvs);
    } else {
      return hipErrorInvalidValue;
    }
  } else if constexpr (F == KvFormat::kMXFP4) {
    // (the <D, T, SINK> overloads of the three kernel names, picked by their argument lists; D = 256: the packed one alone,
    // launch_decode)
    typedef const unsigned char* scales_t;
    constexpr auto packed =
        static_cast<void (*)(DecodeParams, const float*, scales_t, scales_t, TensorLayout, TensorLayout, const int*, int, int,
                             int, FastDiv, const int*, const int*, int)>(fa_decode_ragged_kernel<T, D, SINK>);
    const DecodeFp4& f = *m.fp4;
    if (r) {
      e = launch_kernel<packed>(grid, 256, LDS, s, p, m.sinks, (scales_t)f.ks, (scales_t)f.vs, f.lks, f.lvs, g->table, g->stride,
                                g->page_size, g->num_pages, g->tpp, r->cu_q, (const int*)r->plan, r->total_q);
    } else if constexpr (D != 256) {
      constexpr auto padded = static_cast<void (*)(DecodeParams, const float*, scales_t, scales_t, TensorLayout, TensorLayout)>(
          fa_decode_mod_kernel<D, T, SINK>);
      constexpr auto paged = static_cast<void (*)(DecodeParams, const float*, scales_t, scales_t, TensorLayout, TensorLayout,
                                                  const int*, int, int, int, FastDiv)>(fa_decode_paged_kernel<D, T, SINK>);
      e = g ? launch_kernel<paged>(grid, 256, LDS, s, p, m.sinks, (scales_t)f.ks, (scales_t)f.vs, f.lks, f.lvs, g->table,
                                   g->stride, g->page_size, g->num_pages, g->tpp)
            : launch_kernel<padded>(grid, 256, LDS, s, p, m.sinks, (scales_t)f.ks, (scales_t)f.vs, f.lks, f.lvs);
    } else {
      return hipErrorInvalidValue;
    }
  } else if constexpr (F == KvFormat::kE4M3Token) {   // (D = 256: the packed kernel alone, launch_decode)
    const DecodeFp8Token& f = *m.tok;
    if (r) {
      e = launch_kernel<fa_decode_ragged_kernel<T, D, SINK, true>>(grid, 256, LDS, s, p, m.sinks, (const float*)f.ks,
                                                                 (const float*)f.vs, f.lks, f.lvs, g->table, g->stride,
                                                                 g->page_size, g->num_pages, g->tpp, r->cu_q,
                                                                 (const int*)r->plan, r->total_q);
    } else if constexpr (D != 256) {
      e = g ? launch_kernel<fa_decode_paged_kernel<T, D, SINK, true>>(grid, 256, LDS, s, p, m.sinks, (const float*)f.ks,
                                                                    (const float*)f.vs, f.lks, f.lvs, g->table, g->stride,
                                                                    g->page_size, g->num_pages, g->tpp)
            : launch_kernel<fa_decode_mod_kernel<T, D, SINK, true>>(grid, 256, LDS, s, p, m.sinks, (const float*)f.ks,
                                                              (const float*)f.vs, f.lks, f.lvs);
    } else {
      return hipErrorInvalidValue;
    }
  } else {
    constexpr bool KV8 = F == KvFormat::kE4M3;
    e = r   ? launch_kernel<fa_decode_ragged_kernel<D, T, SOFTCAP, ALIBI, KV8, SINK>>(
                  grid, 256, LDS, s, p, m.softcap, m.slopes, m.slopes_bstride, m.kds, m.vds, m.ds_bstride, m.sinks, g->table,
                  g->stride, g->page_size, g->num_pages, g->tpp, r->cu_q, (const int*)r->plan, r->total_q)
        : g ? launch_kernel<fa_decode_paged_kernel<D, T, SOFTCAP, ALIBI, KV8, SINK>>(
                  grid, 256, LDS, s, p, m.softcap, m.slopes, m.slopes_bstride, m.kds, m.vds, m.ds_bstride, m.sinks, g->table,
                  g->stride, g->page_size, g->num_pages, g->tpp)
            : launch_kernel<fa_decode_mod_kernel<D, T, SOFTCAP, ALIBI, KV8, SINK>>(
                  grid, 256, LDS, s, p, m.softcap, m.slopes, m.slopes_bstride, m.kds, m.vds, m.ds_bstride, m.sinks);
  }
  if (e != hipSuccess || p.nsplit <= 1) return e;
  // one row per D / 4 threads: the B * H * S_q rows, or the H * total_q packed ones
  const long long rows = r ? (long long)p.H * r->total_q : (long long)p.B * p.H * p.Sq, rpb = 256 / (D / 4);
  const dim3 cgrid((unsigned)((rows + rpb - 1) / rpb)), block(256);
  if (r)
    hipLaunchKernelGGL((fa_decode_combine_ragged_kernel<D, T>), cgrid, block, 0, s, p, (const int*)r->plan, r->total_q);
  else
    hipLaunchKernelGGL((fa_decode_combine_kernel<D, T>), cgrid, block, 0, s, p);
  return hipGetLastError();
}

// the work list of a packed step, first on the stream: everything after it reads the plan
hipError_t launch_ragged_plan(const int* cu_q, int B, int group, const DecodeRagged& g, hipStream_t s) {
  hipLaunchKernelGGL(fa_decode_ragged_plan_kernel, dim3(1), dim3(256), 0, s, cu_q, B, g.total_q, group, g.nb_max, g.plan);
  return hipGetLastError();
}

// The append of the call's cache format and geometry.  A thread stores 16 bytes into each cache, so a cache row of D 16-bit
// values, D e4m3 bytes or D / 2 bytes of nibbles takes D / 8, D / 16 or D / 32 threads.
template <int D, typename T, KvFormat F>
static hipError_t launch_append(const DecodeParams& p, const DecodeMod& m, hipStream_t s) {
  constexpr int tpr = F == KvFormat::kMXFP4 ? D / 32 : F == KvFormat::kE4M3 || F == KvFormat::kE4M3Token ? D / 16 : D / 8;
  const long long rows = m.rg ? (long long)m.rg->total_q * p.Hkv : (long long)p.B * p.Hkv * p.Snew;
  const dim3 grid((unsigned)((rows * tpr + 255) / 256)), block(256);
  const DecodePaging* g = m.pg;
  if constexpr (F == KvFormat::kMXFP4) {   // (the <T> overloads of the three names; a padded or paged D = 256 call: launch_decode)
    const DecodeFp4& f = *m.fp4;
    if (m.rg)
      hipLaunchKernelGGL(fa_kvcache_append_ragged_kernel<T>, grid, block, 0, s, p, f.ks, f.vs, f.lks, f.lvs, g->table, g->stride,
                         g->page_size, g->num_pages, m.rg->cu_q, m.rg->total_q);
    else if (g)
      hipLaunchKernelGGL(fa_kvcache_append_paged_kernel<T>, grid, block, 0, s, p, f.ks, f.vs, f.lks, f.lvs, g->table, g->stride,
                         g->page_size, g->num_pages);
    else
      hipLaunchKernelGGL(fa_kvcache_append_kernel<T>, grid, block, 0, s, p, f.ks, f.vs, f.lks, f.lvs);
  } else if constexpr (F == KvFormat::kE4M3Token) {
    const DecodeFp8Token& f = *m.tok;
    if (m.rg)
      hipLaunchKernelGGL((fa_kvcache_append_ragged_kernel<T, true>), grid, block, 0, s, p, f.ks, f.vs, f.lks, f.lvs, g->table,
                         g->stride, g->page_size, g->num_pages, m.rg->cu_q, m.rg->total_q);
    else if (g)
      hipLaunchKernelGGL((fa_kvcache_append_paged_kernel<T, true>), grid, block, 0, s, p, f.ks, f.vs, f.lks, f.lvs, g->table,
                         g->stride, g->page_size, g->num_pages);
    else
      hipLaunchKernelGGL((fa_kvcache_append_kernel<T, true>), grid, block, 0, s, p, f.ks, f.vs, f.lks, f.lvs);
  } else if constexpr (F == KvFormat::kE4M3) {
    if (m.rg)
      hipLaunchKernelGGL(fa_kvcache_append_ragged_fp8_kernel<T>, grid, block, 0, s, p, m.kds, m.vds, m.ds_bstride, g->table,
                         g->stride, g->page_size, g->num_pages, m.rg->cu_q, m.rg->total_q);
    else if (g)
      hipLaunchKernelGGL(fa_kvcache_append_paged_fp8_kernel<T>, grid, block, 0, s, p, m.kds, m.vds, m.ds_bstride, g->table,
                         g->stride, g->page_size, g->num_pages);
    else
      hipLaunchKernelGGL(fa_kvcache_append_fp8_kernel<T>, grid, block, 0, s, p, m.kds, m.vds, m.ds_bstride);
  } else {
    if (m.rg)
      hipLaunchKernelGGL(fa_kvcache_append_ragged_kernel, grid, block, 0, s, p, g->table, g->stride, g->page_size, g->num_pages,
                         m.rg->cu_q, m.rg->total_q);
    else if (g)
      hipLaunchKernelGGL(fa_kvcache_append_paged_kernel, grid, block, 0, s, p, g->table, g->stride, g->page_size, g->num_pages);
    else
      hipLaunchKernelGGL(fa_kvcache_append_kernel, grid, block, 0, s, p);
  }
  return hipGetLastError();
}

// The plan kernel (packed queries), the append (S_new > 0), then the attention kernel of the call's one score transform: a
// 16-bit cache has the plain, soft-capped, ALiBi and sink kernels, a quantised cache the plain, the sink and the soft-capped one.
template <int D, typename T, KvFormat F>
static hipError_t launch_decode_t(const DecodeParams& p, const DecodeMod& m, hipStream_t s) {
  if (m.rg)
    if (hipError_t e = launch_ragged_plan(m.rg->cu_q, p.B, p.group, *m.rg, s)) return e;
  if (p.Snew > 0)
    if (hipError_t e = launch_append<D, T, F>(p, m, s)) return e;
  if constexpr (F != KvFormat::k16)
    return m.softcap > 0.f ? launch_decode_mod<D, T, F, true, false, false>(p, m, s)
           : m.sinks       ? launch_decode_mod<D, T, F, false, false, true>(p, m, s)
                           : launch_decode_mod<D, T, F, false, false, false>(p, m, s);
  else
    return m.sinks            ? launch_decode_mod<D, T, F, false, false, true>(p, m, s)
           : m.slopes         ? launch_decode_mod<D, T, F, false, true, false>(p, m, s)
           : m.softcap > 0.f  ? launch_decode_mod<D, T, F, true, false, false>(p, m, s)
                              : launch_decode_mod<D, T, F, false, false, false>(p, m, s);
}

template <int D, KvFormat F>
static hipError_t launch_decode_f(const DecodeParams& p, int dtype, hipStream_t s, const DecodeMod& m) {
  return dtype == 1 ? launch_decode_t<D, BF16, F>(p, m, s) : launch_decode_t<D, FP16, F>(p, m, s);
}
template <int D>
static hipError_t launch_decode_d(const DecodeParams& p, int dtype, hipStream_t s, const DecodeMod& m) {
  if (m.fmt == KvFormat::kMXFP4) return launch_decode_f<D, KvFormat::kMXFP4>(p, dtype, s, m);
  if (m.fmt == KvFormat::kE4M3Token) return launch_decode_f<D, KvFormat::kE4M3Token>(p, dtype, s, m);
  return m.fmt == KvFormat::kE4M3 ? launch_decode_f<D, KvFormat::kE4M3>(p, dtype, s, m)
                                  : launch_decode_f<D, KvFormat::k16>(p, dtype, s, m);
}

hipError_t launch_decode(const DecodeParams& p, int dtype, hipStream_t s, const DecodeMod& m) {
  // The combinations no kernel is instantiated for.  Packed queries go over paged pools only.  An MXFP4 cache comes with its
  // scale tensors, plain, with sinks or soft-capped, padded, paged or packed: no ALiBi, and D = 256 with packed queries only.
  if (m.rg && !m.pg) return hipErrorInvalidValue;
  if (m.fmt == KvFormat::kMXFP4 && (!m.fp4 || m.slopes || (p.D == 256 && !m.rg))) return hipErrorInvalidValue;
  // A per-token-scaled e4m3 cache likewise: its scale tensors, sinks or a soft-cap at most, D = 256 with packed queries only.
  if (m.fmt == KvFormat::kE4M3Token && (!m.tok || m.slopes || (p.D == 256 && !m.rg))) return hipErrorInvalidValue;
  // A quantised cache takes at most one transform, sinks or a soft-cap (include_quant/mi355fa_kvcache_quant_softcap.h), and no ALiBi.
  if (m.fmt != KvFormat::k16 && (m.slopes || (m.softcap > 0.f && m.sinks))) return hipErrorInvalidValue;
  if (p.D == 64) return launch_decode_d<64>(p, dtype, s, m);
  if (p.D == 128) return launch_decode_d<128>(p, dtype, s, m);
  if (p.D == 256) return launch_decode_d<256>(p, dtype, s, m);
  return hipErrorInvalidValue;
}

}  // namespace fa
