// The DeepSeek-V3.2 indexer logits over a paged FP8 key cache (include_mla_indexer/mi355fa_mla_indexer.h):
//
//     logits[b, i, t] = k_scale[t] * sum_h w[b, i, h] * max(0, sum_d q[b, i, h, d] * k[t, d])      (-inf where t is hidden)
//
// The first kernel here on the FP8 matrix instructions: q and K stay bytes, one v_mfma_f32_16x16x128_f8f6f4 is 16 heads x 16 keys
// x all 128 dims, its products exact and its sum fp32.
//
// Who does what (fa_decode_paged_kernel<IdxLogits, H_i / 16, QG>).  grid = (key chunks, sequences), 4 waves per workgroup, no split and no combine.  A chunk is chunk_tiles tiles of
// 32 keys, dealt to the waves round-robin (waves of a workgroup read neighbouring 4-KiB pieces at the same time).  Every K byte is
// used by exactly one wave, for all heads and all query tokens, so K never sees LDS: it goes global -> VGPR straight in the MFMA's
// B layout.  q is the resident A operand, loaded once per workgroup: 8 VGPRs per (query token, block of 16 heads), 32 per token
// at H_i = 64.  Query tokens go in groups of QG (1, 2 or 4): S_q <= 4 reads K from HBM once, a larger S_q re-reads it from L2 once
// per further group.
//
// Layouts (lane l: c = l & 15, g = l >> 4).
//   A (q)   lane holds head 16 hb + c, bytes [32 g, 32 g + 32) of its 128: two 16-byte loads.
//   B (K)   lane holds key 16 sub + c of the tile, the same bytes [32 g, 32 g + 32): two 16-byte loads.  q and K share the byte
//           order, which is all a dot product needs; the 4 lane groups of a key cover its 128-byte row.
//   D       lane holds heads 16 hb + 4 g + {0..3} of ONE key c: ReLU, the weights (one 16-byte LDS read of 4 consecutive heads) and
//           the sum over its heads are in-lane, the sum over g is a ds_swizzle (lanes ^ 16) and a v_permlane32_swap (lanes ^ 32),
//           in an order that is the same in all four groups.  Lane group idx & 3 stores the 16 consecutive logits of result idx.
//
// The ring.  Two tiles of registers (cur, nxt: 2 x (16 + 2) VGPRs): tile t + 4 is requested before tile t is multiplied, and its
// table entry was looked up one step before that (ent1 / ent2), so neither the scalar load of the table nor the 16-byte loads
// stand in front of an MFMA.  The waits are hipcc's own counted vmcnt (the loads are plain C++).  A third tile has not been
// measured.
//
// What is never read: a table entry at or past ceil(L_b / page_size) (lookup), a row or a scale at or past L_b (the per-lane
// `key < L` in load_tile), a page whose entry is outside [0, num_pages).  What is always written: every column of [0, W) of every
// query row, -inf where hidden -- a workgroup past L_b's end owes exactly that.
//
// The append (fa_kvcache_append_paged_kernel<IdxLogits, T>): one wave per new row, lanes 0..31 with four values each: amax over the row, s = amax /
// 448 (1.0 where not normal), x / s saturated and rounded to nearest even by v_cvt_pk_fp8_f32 -- the rule and the bits of
// fp8_token_kvcache.quantize_kv_fp8_per_token --, 32 dword stores and one fp32 through the table.  Vector stores only.
#include "fa_common.h"
#include "fa_mla_indexer.h"
#include "fa_mla_indexer_ops.h"

namespace fa {
namespace {

// L_b as the kernels use it: clamped to the table's reach
FA_DEVINL int idx_len(const IndexerParams& p, int b) { return min(max(p.seqlens[b] + p.Snew, 0), p.max_pages * p.page_size); }

// One tile of a wave: per column block the lane's 32 bytes of its key and the key's scale
struct KTile {
  u32x4 k[2][2];
  float s[2];
};

// The table entry of tile `t` of sequence b, -1 where the tile is past the wave's run or past L (no entry is read there)
FA_DEVINL int idx_lookup(const IndexerParams& p, int b, int t, int t_end, int L) {
  if (t >= t_end || t * kIdxTile >= L) return -1;
  return __builtin_amdgcn_readfirstlane(p.table[(long long)b * p.bt_stride + p.tpp.div(t)]);
}

// Request tile t (its table entry: ent).  A lane whose key is at or past L, and every lane of a tile with no page, loads nothing.
FA_DEVINL KTile idx_load_tile(const IndexerParams& p, int t, int ent, int L, int g, int c) {
  KTile r;
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
    r.k[sub][0] = r.k[sub][1] = u32x4{0u, 0u, 0u, 0u};
    r.s[sub] = 0.f;
  }
  if ((unsigned)ent >= (unsigned)p.num_pages) return r;
  const int row0 = (t - p.tpp.div(t) * (p.page_size / kIdxTile)) * kIdxTile;
  const char* page = (const char*)p.k + (long long)ent * p.k_ps;
  const float* spage = p.ks + (long long)ent * p.ks_ps;
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
    const int row = row0 + 16 * sub + c;
    if (t * kIdxTile + 16 * sub + c < L) {
      const u32x4* src = (const u32x4*)(page + (long long)row * p.k_rs + 32 * g);
      r.k[sub][0] = src[0];
      r.k[sub][1] = src[1];
      r.s[sub] = spage[(long long)row * p.ks_rs];
    }
  }
  return r;
}

}  // namespace

template <typename Tag, int HB, int QG>
__global__ __launch_bounds__(256) void fa_decode_paged_kernel(const IndexerParams p) {
  constexpr int HI = 16 * HB;
  __shared__ __attribute__((aligned(16))) float w_lds[QG * HI];
  const int b = blockIdx.y;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int L = idx_len(p, b);
  const int ntiles = (p.W + kIdxTile - 1) / kIdxTile;
  const int t_begin = blockIdx.x * p.chunk_tiles + wave;
  const int t_end = min((int)(blockIdx.x + 1) * p.chunk_tiles, ntiles);
  const float ninf = -__builtin_inff();

  for (int q0 = 0; q0 < p.Sq; q0 += QG) {
    if (q0) __syncthreads();   // every wave is done with the last group's weights
    // a row past S_q in the last group repeats the last row and is not stored
    for (int e = threadIdx.x; e < QG * HI; e += 256) {
      const int j = e / HI, h = e - j * HI, i = min(q0 + j, p.Sq - 1);
      w_lds[e] = p.w[(long long)b * p.w_sb + (long long)i * p.w_ss + (long long)h * p.w_sh];
    }
    i32x8 qa[QG][HB];
#pragma unroll
    for (int j = 0; j < QG; ++j) {
      const int i = min(q0 + j, p.Sq - 1);
#pragma unroll
      for (int hb = 0; hb < HB; ++hb) {
        const u32x4* src = (const u32x4*)((const char*)p.q + (long long)b * p.q_sb + (long long)i * p.q_ss +
                                          (long long)(16 * hb + c) * p.q_sh + 32 * g);
        qa[j][hb] = idx_operand(src[0], src[1]);
      }
    }
    __syncthreads();

    int ent1 = idx_lookup(p, b, t_begin + kIdxWaves, t_end, L);
    KTile cur = idx_load_tile(p, t_begin, idx_lookup(p, b, t_begin, t_end, L), L, g, c);
    for (int t = t_begin; t < t_end; t += kIdxWaves) {
      const int ent2 = idx_lookup(p, b, t + 2 * kIdxWaves, t_end, L);
      const KTile nxt = idx_load_tile(p, t + kIdxWaves, ent1, L, g, c);
      ent1 = ent2;
      float res[2 * QG];
      if (t * kIdxTile < L) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          const i32x8 kb = idx_operand(cur.k[sub][0], cur.k[sub][1]);
          const int col = t * kIdxTile + 16 * sub + c;
#pragma unroll
          for (int j = 0; j < QG; ++j) {
            float s = 0.f;
#pragma unroll
            for (int hb = 0; hb < HB; ++hb) {
              const f32x4 d = idx_mfma(qa[j][hb], kb);
              const f32x4 wv = *(const f32x4*)&w_lds[j * HI + 16 * hb + 4 * g];
#pragma unroll
              for (int r = 0; r < 4; ++r) s = __builtin_fmaf(wv[r], __builtin_fmaxf(d[r], 0.f), s);
            }
            s = half_sum(idx_sum_xor16(s)) * cur.s[sub];
            const bool visible = col < L && (!p.causal || col <= L - p.Sq + q0 + j);
            res[sub * QG + j] = visible ? s : ninf;
          }
        }
      } else {
#pragma unroll
        for (int x = 0; x < 2 * QG; ++x) res[x] = ninf;
      }
#pragma unroll
      for (int x = 0; x < 2 * QG; ++x) {
        const int sub = x / QG, j = x - sub * QG, col = t * kIdxTile + 16 * sub + c;
        if (g == (x & 3) && q0 + j < p.Sq && col < p.W) p.out[(long long)b * p.o_sb + (long long)(q0 + j) * p.o_ss + col] = res[x];
      }
      cur = nxt;
    }
  }
}

namespace {

// max |x| over four values of T (two dwords)
template <typename T>
FA_DEVINL float idx_amax4(u32x2 w) {
  typedef __attribute__((ext_vector_type(2))) typename T::elem e2;
  const unsigned w0 = w[0], w1 = w[1];
  const e2 a = __builtin_bit_cast(e2, w0), b = __builtin_bit_cast(e2, w1);
  return __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf((float)a[0]), __builtin_fabsf((float)a[1])),
                         __builtin_fmaxf(__builtin_fabsf((float)b[0]), __builtin_fabsf((float)b[1])));
}
// the four e4m3 bytes e4m3_rne(clamp(float(x) / d, -448, 448)), in the same order
template <typename T>
FA_DEVINL unsigned idx_quant4(u32x2 w, float d) {
  typedef __attribute__((ext_vector_type(2))) typename T::elem e2;
  const unsigned w0 = w[0], w1 = w[1];
  const e2 a = __builtin_bit_cast(e2, w0), b = __builtin_bit_cast(e2, w1);
  float x[4] = {(float)a[0], (float)a[1], (float)b[0], (float)b[1]};
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = __builtin_fminf(__builtin_fmaxf(x[j] / d, -448.f), 448.f);
  const int r = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], 0, false);
  return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], r, true);
}

}  // namespace

template <typename Tag, typename T>
__global__ __launch_bounds__(256) void fa_kvcache_append_paged_kernel(const IndexerParams p) {
  const int row = blockIdx.x * kIdxWaves + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= p.B * p.Snew) return;
  const int b = row / p.Snew, i = row - b * p.Snew;
  u32x2 w{0u, 0u};
  if (lane < 32) w = ((const u32x2*)p.k_new)[(long long)row * 32 + lane];
  float amax = idx_amax4<T>(w);
#pragma unroll
  for (int m = 1; m < 32; m <<= 1) amax = __builtin_fmaxf(amax, __shfl_xor(amax, m));   // lanes 32..63 hold zeros
  // amax / 448, the correctly rounded fp32 division; 1 where the quotient is not a normal number (a zero row, a subnormal quotient)
  float s = amax / 448.f;
  const unsigned field = (__builtin_bit_cast(unsigned, s) >> 23) & 0xffu;
  s = field - 1u < 254u ? s : 1.f;
  const int pos = p.seqlens[b] + i;
  if (pos < 0 || pos >= p.max_pages * p.page_size) return;
  const int pg = p.pdiv.div(pos);
  const int ent = p.table[(long long)b * p.bt_stride + pg];
  if ((unsigned)ent >= (unsigned)p.num_pages) return;
  const int r = pos - pg * p.page_size;
  if (lane < 32) ((unsigned*)((char*)p.k + (long long)ent * p.k_ps + (long long)r * p.k_rs))[lane] = idx_quant4<T>(w, s);
  if (lane == 0) p.ks[(long long)ent * p.ks_ps + (long long)r * p.ks_rs] = s;
}

namespace {

template <int HB>
hipError_t launch_logits(const IndexerParams& p, dim3 grid, hipStream_t s) {
  if (p.Sq == 1)
    hipLaunchKernelGGL((fa_decode_paged_kernel<IdxLogits, HB, 1>), grid, dim3(256), 0, s, p);
  else if (p.Sq == 2)
    hipLaunchKernelGGL((fa_decode_paged_kernel<IdxLogits, HB, 2>), grid, dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL((fa_decode_paged_kernel<IdxLogits, HB, 4>), grid, dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace

// Workgroups the chunk size aims at: two per CU of a 256-CU device, each wave with a run of tiles longer than its ring.
constexpr long long kIdxTargetWgs = 512;

hipError_t launch_mla_indexer(IndexerParams p, int dtype, hipStream_t s) {
  if (p.Snew > 0) {
    const unsigned grid = (unsigned)(((long long)p.B * p.Snew + kIdxWaves - 1) / kIdxWaves);
    if (dtype == 1)
      hipLaunchKernelGGL((fa_kvcache_append_paged_kernel<IdxLogits, BF16>), dim3(grid), dim3(256), 0, s, p);
    else
      hipLaunchKernelGGL((fa_kvcache_append_paged_kernel<IdxLogits, FP16>), dim3(grid), dim3(256), 0, s, p);
    if (hipError_t e = hipGetLastError()) return e;
  }
  const long long ntiles = ((long long)p.W + kIdxTile - 1) / kIdxTile;
  long long ct = (p.B * ntiles + kIdxTargetWgs - 1) / kIdxTargetWgs;
  ct = (ct + kIdxWaves - 1) / kIdxWaves * kIdxWaves;
  ct = ct < 4 * kIdxWaves ? 4 * kIdxWaves : (ct > 64 * kIdxWaves ? 64 * kIdxWaves : ct);
  p.chunk_tiles = (int)ct;
  const dim3 grid((unsigned)((ntiles + ct - 1) / ct), (unsigned)p.B);
  switch (p.Hi / 16) {
    case 1: return launch_logits<1>(p, grid, s);
    case 2: return launch_logits<2>(p, grid, s);
    case 3: return launch_logits<3>(p, grid, s);
    default: return launch_logits<4>(p, grid, s);
  }
}

}  // namespace fa
