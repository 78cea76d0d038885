// Gradient of the attention sinks (include/mi355fa_sink.h):
//
//     dsinks[h] = - sum over b, i of  exp(sinks[h] - LSE[b, h, i]) * delta[b, h, i]
//
// with the LSE rows the sink forward wrote and the delta rows (dO . O) the dQ kernel wrote.  The sink has no value row, so
// its dP is 0 and dS = p0 * (0 - delta): nothing else of the backward knows about it.
//
// A streaming reduction of 8 bytes per query row, far below the cost of the dQ / dK/dV kernels it follows.  One workgroup
// per head, so the whole sum of a head has ONE fixed order and needs neither a workspace nor atomics: thread t adds its
// rows (t, t + 256, ... of each sequence, sequences ascending) in fp32, the 64 lanes of a wave combine in a butterfly,
// and thread 0 adds the 4 wave sums in wave order.  The same inputs give the same bits.
#include "fa_common.h"
#include "fa_kernels.h"

namespace fa {

namespace {
constexpr int kDsinkThreads = 256;   // every kernel of the library is a 256-thread workgroup
}

// Head h's rows are `nseg` runs of `len` floats, run b at h * sh + b * sb ([B, H, S_q]: nseg = B, len = S_q, sb = H * S_q,
// sh = S_q; packed [H, total_q]: nseg = 1, len = total_q, sh = total_q).
__global__ __launch_bounds__(kDsinkThreads) void fa_bwd_dsink_kernel(const float* __restrict__ lse, const float* __restrict__ delta,
                                                                   const float* __restrict__ sinks, float* __restrict__ dsinks,
                                                                   int nseg, int len, long long sb, long long sh) {
  __shared__ float wsum[kDsinkThreads / 64];
  const int h = blockIdx.x, tid = threadIdx.x;
  const float z = sinks[h];
  const float z2 = z * kLog2e;
  float acc = 0.f;
  if (z != -INFINITY) {   // z = -inf: p0 = 0 on every row, also where LSE = -inf (exp(-inf - -inf) is not formed)
    for (int b = 0; b < nseg; ++b) {
      const float* l = lse + h * sh + b * sb;
      const float* d = delta + h * sh + b * sb;
#pragma unroll 8
      for (int i = tid; i < len; i += kDsinkThreads) acc = __builtin_fmaf(__builtin_amdgcn_exp2f(__builtin_fmaf(-l[i], kLog2e, z2)), d[i], acc);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((tid & 63) == 0) wsum[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kDsinkThreads / 64; ++w) t += wsum[w];
    dsinks[h] = -t;
  }
}

hipError_t launch_bwd_dsink(const float* lse, const float* delta, const float* sinks, float* dsinks, int H, int nseg, int len,
                            long long sb, long long sh, hipStream_t s) {
  hipLaunchKernelGGL(fa_bwd_dsink_kernel, dim3(H), dim3(kDsinkThreads), 0, s, lse, delta, sinks, dsinks, nseg, len, sb, sh);
  return hipGetLastError();
}

}  // namespace fa
