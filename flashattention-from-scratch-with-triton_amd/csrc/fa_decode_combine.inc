// The combine kernel of the split-KV decode calls, included inside namespace fa behind fa_common.h and fa_decode.h: joins the
// per-split partials the attention kernel left in the workspace (fa_decode.h kvcache_ws_bytes: unnormalised O in fp32, then the
// (m, l) pairs) into O and LSE.  Text of its own so that fa_decode.hip (D = 64, 128, 256) and fa_decode_mla.hip (D = 512: the latent
// width of an MLA result) compile the one definition.
// One row (b, h, i) per D / 4 threads: the n partials merged in ascending split order.
template <int D, typename T>
__global__ __launch_bounds__(256) void fa_decode_combine_kernel(DecodeParams p) {
  constexpr int TPR = D / 4, RPB = 256 / TPR;
  const long long R = (long long)p.B * p.H * p.Sq;
  const long long ridx = (long long)blockIdx.x * RPB + threadIdx.x / TPR;
  if (ridx >= R) return;
  const int d4 = (threadIdx.x % TPR) * 4, n = p.nsplit;
  const float* ml = p.ws + (long long)n * R * D;
  // (unrolled: the partials' loads of several splits in flight at once; a rolled loop paid one L2 round trip per split)
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
  const int i = (int)(ridx % p.Sq), head = (int)((ridx / p.Sq) % p.H), b = (int)(ridx / ((long long)p.Sq * p.H));
  const float inv = ls > 0.f ? 1.f / ls : 0.f;
  typedef __attribute__((ext_vector_type(4))) typename T::elem e4;
  e4 ov;
#pragma unroll
  for (int j = 0; j < 4; ++j) ov[j] = (typename T::elem)(acc[j] * inv);
  *(u32x2*)((char*)p.o + b * p.lo.sb + (long long)head * p.lo.sh + (long long)i * p.lo.rs + d4 * 2) =
      __builtin_bit_cast(u32x2, ov);
  if (d4 == 0 && p.lse) p.lse[ridx] = ls > 0.f ? (mx + __builtin_log2f(ls)) * kLn2 : -INFINITY;
}
