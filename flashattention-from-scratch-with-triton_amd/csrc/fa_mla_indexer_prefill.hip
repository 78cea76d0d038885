// The DeepSeek-V3.2 indexer logits of a prefill step (include_mla_indexer_prefill/mi355fa_mla_indexer_prefill.h):
//
//     logits[m, t] = k_scale[t] * sum_h w[m, h] * max(0, sum_d q[m, h, d] * k[t, d])      for ks[m] <= t < ke[m], -inf elsewhere
//
// over ONE packed query tensor [M, H_i, 128] and ONE contiguous key array [N, 128], every row with a key range of its own.  The
// decode kernel (fa_mla_indexer.hip) keeps all query tokens in every wave and streams K privately; at a prompt's M that is one pass
// over K per four tokens.  This kernel is split the other way round.
//
// Who does what (fa_decode_paged_kernel<IdxPrefill, H_i / 16>).  grid = (key chunks, row blocks), 4 waves per workgroup.  A
// workgroup owns 16 query rows x a run of chunk_tiles tiles of 32 keys.  Wave v keeps rows 4 v .. 4 v + 3 resident as the A operand
// of v_mfma_f32_16x16x128_f8f6f4 (8 VGPRs per (row, block of 16 heads): 128 at H_i = 64) and those rows' weights in LDS; a q byte
// is loaded once per workgroup.  A K tile and its 32 scales come from global ONCE per workgroup -- lane e of 256 loads bytes
// [16 (e & 7), +16) of key e >> 3, so each wave fetches a quarter -- go to LDS, and all four waves read them back in the B layout:
// a K byte serves 16 rows x H_i heads per fetch.
//
// The LDS tile.  Two buffers of 32 rows, each row its 128 bytes + 16 bytes of padding (kPreRowBytes = 144).  A B-operand read is
// two ds_read_b128 per lane: lane (c, g) takes bytes [32 g, 32 g + 32) of key c, i.e. the 16-byte slots 9 c + 2 g and 9 c + 2 g + 1.
// 9 is odd, so the 16 lanes of a column block fall on 16 different slots of the 16 (64 banks x 4 bytes) -- unpadded they would
// all start in one.  The write (slots 9 r + p, p < 8, two rows per 16 lanes) meets itself once per 16 lanes.  A swizzle would
// save the 512 bytes of padding and cost an xor per address on both sides; nothing here is short of LDS (13.4 KiB at H_i = 64).
//
// The pipeline.  Iteration t: request tile t + 1 (global -> 5 VGPRs), read tile t from LDS, 2 x 4 x HB MFMAs with their epilogues,
// store, then write tile t + 1 into the other buffer and meet at ONE barrier: the buffer written in iteration t was last read in
// iteration t - 1, which every wave left through that iteration's barrier.  The global loads and the LDS reads sit under the MFMAs;
// the waits are hipcc's own.
//
// Layouts (lane l: c = l & 15, g = l >> 4): A, B and D are the decode kernel's.  D: a lane holds heads 16 hb + 4 g + {0..3} of ONE
// key c: ReLU, the weights (one 16-byte LDS read) and the sum over its heads are in-lane, the sum over g is a ds_swizzle and a
// v_permlane32_swap, the same order in all four groups.  Lane group g then keeps row 4 v + g of the wave's four: one select chain,
// the key's scale, the range mask -- a select on the column, never a multiply -- and ONE store per column block, 4 rows x 16
// consecutive columns.  Nothing is staged through LDS on the way out (not tried: DESIGN.md).
//
// Skipping.  The workgroup takes the union [min ks, max ke) of its rows' clamped, non-empty ranges.  Tiles of its run that do not
// meet the union are filled with -inf, 256 bytes per wave and store, with no K load and before q is touched; a workgroup with
// nothing else to do ends there.  Inside the union a key row outside it is not read either (zero bytes, zero scale).  Rows past M
// in the last block repeat row M - 1 and are not stored.
//
// What is never read: a key row or scale outside the union of the workgroup's ranges, so none at or past N.  What is always
// written: every column of [0, W) of every row.
#include "fa_common.h"
#include "fa_mla_indexer_ops.h"
#include "fa_mla_indexer_prefill.h"

namespace fa {

template <typename Tag, int HB>
__global__ __launch_bounds__(256) void fa_decode_paged_kernel(const IdxPrefillParams p) {
  constexpr int HI = 16 * HB;
  __shared__ __attribute__((aligned(16))) float w_lds[kPreRows * HI];
  __shared__ __attribute__((aligned(16))) unsigned char k_lds[2][kPreTile * kPreRowBytes];
  __shared__ float s_lds[2][kPreTile];
  __shared__ int r_lds[2][kPreRows];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int row0 = blockIdx.y * kPreRows;
  const float ninf = -__builtin_inff();

  // the row this lane masks and stores, and its range
  const int m_st = row0 + 4 * wave + g;
  const int m_ld = min(m_st, p.M - 1);
  const int lo = min(max(p.lo[m_ld], 0), p.N), hi = min(max(p.hi[m_ld], 0), p.N);
  if (c == 0) {
    r_lds[0][4 * wave + g] = hi > lo ? lo : 0x7fffffff;
    r_lds[1][4 * wave + g] = hi > lo ? hi : 0;
  }
  __syncthreads();
  int ulo = 0x7fffffff, uhi = 0;
#pragma unroll
  for (int i = 0; i < kPreRows; ++i) {
    ulo = min(ulo, r_lds[0][i]);
    uhi = max(uhi, r_lds[1][i]);
  }
  ulo = __builtin_amdgcn_readfirstlane(min(ulo, uhi));   // (no row sees anything: [0, 0))
  uhi = __builtin_amdgcn_readfirstlane(uhi);

  // the run, and the part of it that meets the union: tiles [ta, tb)
  const int ntiles = (p.W + kPreTile - 1) / kPreTile;
  const int t0 = blockIdx.x * p.chunk_tiles, t1 = min(t0 + p.chunk_tiles, ntiles);
  const int ta = min(max(ulo / kPreTile, t0), t1), tb = min(max((uhi + kPreTile - 1) / kPreTile, ta), t1);

  // the rest of the run is -inf: columns [32 t0, 32 ta) and [32 tb, 32 t1), a wave on its own four rows
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const int c0 = (side ? tb : t0) * kPreTile, c1 = min((side ? t1 : ta) * kPreTile, p.W);
    for (int j = 0; j < 4; ++j) {
      const int m = row0 + 4 * wave + j;
      if (m >= p.M) break;
      float* dst = p.out + (long long)m * p.o_sm;
      for (int col = c0 + lane; col < c1; col += 64) dst[col] = ninf;
    }
  }
  if (ta >= tb) return;

  // this lane's 16 bytes of tile t and, in the lanes of a row's first piece, the row's scale
  const int krow = tid >> 3, kpiece = tid & 7;
  auto fetch = [&](int t, u32x4& kv, float& sv) {
    const int key = t * kPreTile + krow;
    kv = u32x4{0u, 0u, 0u, 0u};
    sv = 0.f;
    if (key >= ulo && key < uhi) {
      kv = *(const u32x4*)((const char*)p.k + (long long)key * p.k_rs + 16 * kpiece);
      if (kpiece == 0) sv = p.ks[(long long)key * p.s_rs];
    }
  };
  auto commit = [&](int buf, const u32x4& kv, float sv) {
    *(u32x4*)&k_lds[buf][krow * kPreRowBytes + 16 * kpiece] = kv;
    if (kpiece == 0) s_lds[buf][krow] = sv;
  };

  u32x4 kv;
  float sv;
  fetch(ta, kv, sv);
  for (int e = tid; e < kPreRows * HI; e += 256) {
    const int j = e / HI, h = e - j * HI, m = min(row0 + j, p.M - 1);
    w_lds[e] = p.w[(long long)m * p.w_sm + (long long)h * p.w_sh];
  }
  i32x8 qa[4][HB];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = min(row0 + 4 * wave + j, p.M - 1);
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) {
      const u32x4* src = (const u32x4*)((const char*)p.q + (long long)m * p.q_sm + (long long)(16 * hb + c) * p.q_sh + 32 * g);
      qa[j][hb] = idx_operand(src[0], src[1]);
    }
  }
  commit(0, kv, sv);
  __syncthreads();

  const float* wrow = &w_lds[4 * wave * HI + 4 * g];
  float* dst = p.out + (long long)m_st * p.o_sm;
  for (int t = ta; t < tb; ++t) {
    const int buf = (t - ta) & 1;
    if (t + 1 < tb) fetch(t + 1, kv, sv);
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const u32x4* src = (const u32x4*)&k_lds[buf][(16 * sub + c) * kPreRowBytes + 32 * g];
      const i32x8 kb = idx_operand(src[0], src[1]);
      const float sc = s_lds[buf][16 * sub + c];
      float res[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float s = 0.f;
#pragma unroll
        for (int hb = 0; hb < HB; ++hb) {
          const f32x4 d = idx_mfma(qa[j][hb], kb);
          const f32x4 wv = *(const f32x4*)&wrow[j * HI + 16 * hb];
#pragma unroll
          for (int r = 0; r < 4; ++r) s = __builtin_fmaf(wv[r], __builtin_fmaxf(d[r], 0.f), s);
        }
        res[j] = half_sum(idx_sum_xor16(s));
      }
      const float mine = (g == 0 ? res[0] : g == 1 ? res[1] : g == 2 ? res[2] : res[3]) * sc;
      const int col = t * kPreTile + 16 * sub + c;
      if (m_st < p.M && col < p.W) dst[col] = col >= lo && col < hi ? mine : ninf;
    }
    if (t + 1 < tb) commit(buf ^ 1, kv, sv);
    __syncthreads();
  }
}

// The chunk: the workgroups it aims at are four per CU of a 256-CU device (two are resident at 256 VGPRs; the rest evens out the
// rows whose ranges end early), and a run is at least 16 tiles -- eight times the LDS ring, and the 128 KiB of q a workgroup loads
// at H_i = 64 are then no more than twice the K bytes it streams.  Not tuned (README).
constexpr long long kPreTargetWgs = 1024;

hipError_t launch_mla_indexer_prefill(IdxPrefillParams p, hipStream_t s) {
  const long long ntiles = ((long long)p.W + kPreTile - 1) / kPreTile, blocks = ((long long)p.M + kPreRows - 1) / kPreRows;
  long long ct = (blocks * ntiles + kPreTargetWgs - 1) / kPreTargetWgs;
  ct = ct < 16 ? 16 : (ct > 1024 ? 1024 : ct);
  p.chunk_tiles = (int)ct;
  const dim3 grid((unsigned)((ntiles + ct - 1) / ct), (unsigned)blocks);
  switch (p.Hi / 16) {
    case 1: hipLaunchKernelGGL((fa_decode_paged_kernel<IdxPrefill, 1>), grid, dim3(256), 0, s, p); break;
    case 2: hipLaunchKernelGGL((fa_decode_paged_kernel<IdxPrefill, 2>), grid, dim3(256), 0, s, p); break;
    case 3: hipLaunchKernelGGL((fa_decode_paged_kernel<IdxPrefill, 3>), grid, dim3(256), 0, s, p); break;
    default: hipLaunchKernelGGL((fa_decode_paged_kernel<IdxPrefill, 4>), grid, dim3(256), 0, s, p); break;
  }
  return hipGetLastError();
}

}  // namespace fa
