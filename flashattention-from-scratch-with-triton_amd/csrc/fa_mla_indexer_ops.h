// What the two indexer logits kernels (fa_mla_indexer.hip, fa_mla_indexer_prefill.hip) share: the FP8 matrix instruction over
// operands of 32 bytes per lane, and the first of the two cross-lane steps of the head sum.  Include after fa_common.h.
#pragma once

namespace fa {
namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;

// The instruction: true = one v_mfma_f32_16x16x128_f8f6f4 per (16 heads, 16 keys), false = four v_mfma_f32_16x16x32_fp8_fp8 over
// the same registers, which compiles and has not been measured.
constexpr bool kIdxK128 = true;

FA_DEVINL i32x8 idx_operand(u32x4 lo, u32x4 hi) {
  return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// D[head 4 g + r][key c] = sum over the 128 dims of a (16 heads) and b (16 keys)
FA_DEVINL f32x4 idx_mfma(const i32x8& a, const i32x8& b) {
  const f32x4 zero{0.f, 0.f, 0.f, 0.f};
  if constexpr (kIdxK128) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, zero, 0, 0, 0, 0, 0, 0);   // e4m3 x e4m3, no block scales
  } else {
    f32x4 d = zero;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long aj = (long)(((unsigned long)(unsigned)a[2 * j + 1] << 32) | (unsigned)a[2 * j]);
      const long bj = (long)(((unsigned long)(unsigned)b[2 * j + 1] << 32) | (unsigned)b[2 * j]);
      d = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(aj, bj, d, 0, 0, 0);
    }
    return d;
  }
}

// v + the value of lane ^ 16 (ds_swizzle, bit mode: and 0x1f, or 0, xor 0x10)
FA_DEVINL float idx_sum_xor16(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), (0x10 << 10) | 0x1f));
}

}  // namespace
}  // namespace fa
