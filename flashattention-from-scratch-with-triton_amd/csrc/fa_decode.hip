// Split-KV decoding attention ("flash-decoding") over a padded KV cache: include/mi355fa_kvcache.h.
//
// A decode step has a handful of queries per sequence against thousands of cached keys: the work is reading the cache
// once, and the kernels are built for HBM, not for the MFMA pipe.
//
//   fa_kvcache_append_kernel  k_new / v_new -> cache rows [seqlens[b], seqlens[b] + S_new)   (first, same stream)
//   fa_decode_kernel          one workgroup per (batch, K/V head, 32-row block of the group's rows, split)
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

// L_b as the kernels use it: clamped to [0, S_cache] (outside it the result is unspecified, the accesses stay inside)
FA_DEVINL int kv_len(const DecodeParams& p, int b) { return min(max(p.seqlens[b] + p.Snew, 0), p.Scache); }

}  // namespace

template <int D, typename T>
__global__ __launch_bounds__(256, 2) void fa_decode_kernel(DecodeParams p) {
  using C = DecCfg<D>;
  using vec8 = typename T::vec8;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  FA_LDS char* smem = (FA_LDS char*)smem_raw;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- work item: ((b * H_kv + hk) * RB + rb) * nsplit + split ----
  const int g = p.group, M = g * p.Sq, RB = (M + kDecRows - 1) / kDecRows;
  int w = blockIdx.x;
  const int split = w % p.nsplit;
  w /= p.nsplit;
  const int rb = w % RB;
  w /= RB;
  const int hk = w % p.Hkv, b = w / p.Hkv;
  const int L = kv_len(p, b);

  // ---- this row block's visible key tiles, and this split's share of them ----
  const int r0 = rb * kDecRows, rlast = min(M, r0 + kDecRows) - 1;
  const int pos0 = L - p.Sq + r0 / g, pos1 = L - p.Sq + rlast / g;   // positions of the block's first / last query
  const int lo = max(0, pos0 - p.wl), hi = min(L, pos1 + p.wr + 1);
  const int tb = lo / kDecTile, te = hi > lo ? (hi + kDecTile - 1) / kDecTile : tb;
  const int nt = te - tb;
  const int s_beg = tb + (int)((long long)nt * split / p.nsplit);
  const int s_end = tb + (int)((long long)nt * (split + 1) / p.nsplit);

  // ---- this lane's query row: Q^T fragments (B operand), position ----
  const int qrow = r0 + r, qi = qrow / g, qh = hk * g + (qrow - qi * g);
  const int pos = L - p.Sq + qi;
  vec8 qf[C::KS];
  {
    const bool valid = qrow < M;
    const char* qp = (const char*)p.q + b * p.lq.sb + (long long)qh * p.lq.sh + (long long)qi * p.lq.rs + 16 * h;
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks)
      qf[ks] = as_vec8<T>(valid ? *(const u32x4*)(qp + 32 * ks) : u32x4{0u, 0u, 0u, 0u});
  }

  // ---- K / V of (b, hk): rows [0, L) only ----
  const int rs = p.lk.rs;
  const __amdgpu_buffer_rsrc_t rk = make_rsrc((const char*)p.kc + b * p.lk.sb + hk * p.lk.sh, view_bytes(L, rs, C::ROWB));
  const __amdgpu_buffer_rsrc_t rv = make_rsrc((const char*)p.vc + b * p.lv.sb + hk * p.lv.sh, view_bytes(L, rs, C::ROWB));

  FA_LDS char* vt = smem + wave * kDecTile * C::ROWB;
  int v_off[2][C::DB];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int db = 0; db < C::DB; ++db) v_off[e][db] = tr_lane_off<D>(lane, 8 * e, db);

  u32x4 kr[C::KS], vr[C::VL];
  auto load = [&](int t) __attribute__((always_inline)) {
    const int base = t * kDecTile * rs;
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) kr[ks] = buf_load16(rk, base + r * rs + 32 * ks + 16 * h);
#pragma unroll
    for (int u = 0; u < C::VL; ++u) {
      const int id = lane + 64 * u, row = id / C::CPR, c = id % C::CPR;
      vr[u] = buf_load16(rv, base + row * rs + c * 16);
    }
  };

  const float c2 = p.scale * kLog2e;   // scores in log2 units
  float m = -INFINITY, l = 0.f;
  f32x16 oacc[C::DB];
#pragma unroll
  for (int db = 0; db < C::DB; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[db][i] = 0.f;

  int t = s_beg + wave;
  if (t < s_end) load(t);
  for (; t < s_end; t += kDecWaves) {
    // V of tile t into the wave's LDS tile (the previous tile's transposed reads precede these writes in LDS order)
#pragma unroll
    for (int u = 0; u < C::VL; ++u) {
      const int id = lane + 64 * u, row = id / C::CPR, c = id % C::CPR;
      lds_write16(vt + lds_off<D>(row, c), vr[u]);
    }
    u32x4 kc[C::KS];
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) kc[ks] = kr[ks];
    if (t + kDecWaves < s_end) load(t + kDecWaves);   // next tile in flight while this one is computed

    // ---- S^T = K Q^T: reg i of lane (r, h) = score of query row r, key t*32 + (i&3) + 8(i>>2) + 4h ----
    f32x16 s;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) s = T::mfma(as_vec8<T>(kc[ks]), qf[ks], s);
    float tm = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int key = t * kDecTile + (i & 3) + 8 * (i >> 2) + 4 * h;
      const bool dead = key >= L || key < pos - p.wl || key > pos + p.wr;
      s[i] = dead ? -INFINITY : s[i] * c2;
      tm = __builtin_fmaxf(tm, s[i]);
    }
    // ---- online softmax; a row that has seen no visible key keeps m = -inf (offset 0: p = 0, not NaN) ----
    const float mn = __builtin_fmaxf(m, half_max(tm));
    const float mu = mn == -INFINITY ? 0.f : mn;
    const float corr = __builtin_amdgcn_exp2f(m - mu);
    m = mn;
    l *= corr;
#pragma unroll
    for (int db = 0; db < C::DB; ++db)
#pragma unroll
      for (int i = 0; i < 16; ++i) oacc[db][i] *= corr;
    float ls[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      s[i] = __builtin_amdgcn_exp2f(s[i] - mu);
      ls[i & 3] += s[i];
    }
    l += (ls[0] + ls[1]) + (ls[2] + ls[3]);
    // ---- O^T += V^T P^T ----
    const vec8 pf0 = pack8<T, 0>(s), pf1 = pack8<T, 1>(s);
    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): this wave's V writes have landed
#pragma unroll
    for (int db = 0; db < C::DB; ++db) {
      const vec8 a0 = lds_read_tr_frag<T>(vt + v_off[0][db], vt + v_off[1][db]);
      oacc[db] = T::mfma(a0, pf0, oacc[db]);
      const vec8 a1 = lds_read_tr_frag<T>(vt + 16 * C::ROWB + v_off[0][db], vt + 16 * C::ROWB + v_off[1][db]);
      oacc[db] = T::mfma(a1, pf1, oacc[db]);
    }
  }
  const float lt = half_sum(l);

  // ---- merge the four waves (wave order), then O / LSE or the split's partial ----
  __syncthreads();   // every wave is done with its V tile: the LDS is the merge stage now
  float* stage = (float*)smem_raw;
  float* sm = (float*)(smem_raw + C::ML_OFF);
  float* sl = sm + kDecWaves * kDecRows;
  if (h == 0) {
    sm[wave * kDecRows + r] = m;
    sl[wave * kDecRows + r] = lt;
  }
#pragma unroll
  for (int db = 0; db < C::DB; ++db)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      *(f32x4*)(stage + (wave * kDecRows + r) * C::OST + db * 32 + 8 * c + 4 * h) =
          f32x4{oacc[db][4 * c], oacc[db][4 * c + 1], oacc[db][4 * c + 2], oacc[db][4 * c + 3]};
  __syncthreads();
  const long long R = (long long)p.B * p.H * p.Sq;
  for (int it = tid; it < kDecRows * (D / 4); it += 256) {
    const int row = it / (D / 4), d4 = (it % (D / 4)) * 4;
    const int qr = r0 + row;
    if (qr >= M) break;   // rows ascend with `it`
    float mx = -INFINITY;
#pragma unroll
    for (int v = 0; v < kDecWaves; ++v) mx = __builtin_fmaxf(mx, sm[v * kDecRows + row]);
    const float mo = mx == -INFINITY ? 0.f : mx;
    float ls = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int v = 0; v < kDecWaves; ++v) {
      const float e = __builtin_amdgcn_exp2f(sm[v * kDecRows + row] - mo);
      ls += e * sl[v * kDecRows + row];
      acc += e * *(const f32x4*)(stage + (v * kDecRows + row) * C::OST + d4);
    }
    const int i = qr / g, head = hk * g + (qr - i * g);
    const long long ridx = ((long long)b * p.H + head) * p.Sq + i;
    if (p.nsplit == 1) {
      const float inv = ls > 0.f ? 1.f / ls : 0.f;
      typedef __attribute__((ext_vector_type(4))) typename T::elem e4;
      e4 ov;
#pragma unroll
      for (int j = 0; j < 4; ++j) ov[j] = (typename T::elem)(acc[j] * inv);
      *(u32x2*)((char*)p.o + b * p.lo.sb + (long long)head * p.lo.sh + (long long)i * p.lo.rs + d4 * 2) =
          __builtin_bit_cast(u32x2, ov);
      if (d4 == 0 && p.lse) p.lse[ridx] = ls > 0.f ? (mx + __builtin_log2f(ls)) * kLn2 : -INFINITY;
    } else {
      const long long pr = split * R + ridx;
      *(f32x4*)(p.ws + pr * D + d4) = acc;
      if (d4 == 0) *(f32x2_t*)(p.ws + (long long)p.nsplit * R * D + 2 * pr) = f32x2_t{mx, ls};
    }
  }
}

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

// k_new / v_new rows -> cache rows seqlens[b] + j, one 16-byte chunk per thread; rows outside [0, S_cache) are dropped.
__global__ __launch_bounds__(256) void fa_kvcache_append_kernel(DecodeParams p) {
  const int cpr = p.D / 8;
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)p.B * p.Hkv * p.Snew * cpr;
  if (item >= total) return;
  const int c = (int)(item % cpr);
  const long long rowi = item / cpr;   // (b * H_kv + hk) * S_new + j
  const int j = (int)(rowi % p.Snew), bh = (int)(rowi / p.Snew), hk = bh % p.Hkv, b = bh / p.Hkv;
  const int dst = p.seqlens[b] + j;
  if (dst < 0 || dst >= p.Scache) return;
  const long long src_off = rowi * p.D * 2 + c * 16;
  *(u32x4*)((char*)p.kc + b * p.lk.sb + (long long)hk * p.lk.sh + (long long)dst * p.lk.rs + c * 16) =
      *(const u32x4*)((const char*)p.k_new + src_off);
  *(u32x4*)((char*)p.vc + b * p.lv.sb + (long long)hk * p.lv.sh + (long long)dst * p.lv.rs + c * 16) =
      *(const u32x4*)((const char*)p.v_new + src_off);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// Split count: at most one workgroup per CU (256 CUs) over (batch, K/V head, row block, split), and splits of about
// sqrt(128 * S_cache) keys (n <= sqrt(S_cache / 128)), at most kMaxSplits.  A split has fixed costs (its Q rows, the first
// tile's latency, the wave merge, its share of the combine), so the best split length grows with the cache: in the sweep
// behind this rule (profiles/decode_split_sweep.jsonl) it was 512 keys at 4096, 2048 at 32768 and
// 4096-5461 at 131072 for one sequence, and the rule is within 12 % of the best forced count at every swept point.
int kvcache_splits(int B, int H_kv, int group, int S_q, int S_cache, int D, int forced) {
  (void)D;
  if (forced > 0) return forced;
  constexpr int kTargetWgs = 256, kMaxSplits = 64;
  const long long rb = ((long long)group * S_q + kDecRows - 1) / kDecRows;
  const long long wgs = (long long)B * H_kv * rb;
  long long n = (kTargetWgs + wgs - 1) / wgs;
  long long by_len = 1;
  while ((by_len + 1) * (by_len + 1) * 128 <= S_cache) ++by_len;
  n = std::min(n, by_len);
  return (int)std::max<long long>(1, std::min<long long>(n, kMaxSplits));
}

template <int D, typename T>
static hipError_t launch_decode_t(const DecodeParams& p, hipStream_t s) {
  using C = DecCfg<D>;
  if (p.Snew > 0) {
    const long long items = (long long)p.B * p.Hkv * p.Snew * (D / 8);
    hipLaunchKernelGGL(fa_kvcache_append_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, p);
    if (hipError_t e = hipGetLastError()) return e;
  }
  auto kern = fa_decode_kernel<D, T>;
  if (C::LDS_BYTES > 48 * 1024) {
    static std::atomic<unsigned long long> opted_in{0};
    if (hipError_t e = opt_in_lds((const void*)kern, C::LDS_BYTES, opted_in)) return e;
  }
  const long long rb = ((long long)p.group * p.Sq + kDecRows - 1) / kDecRows;
  const long long grid = (long long)p.B * p.Hkv * rb * p.nsplit;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), C::LDS_BYTES, s, p);
  if (hipError_t e = hipGetLastError()) return e;
  if (p.nsplit > 1) {
    const long long rows = (long long)p.B * p.H * p.Sq, rpb = 256 / (D / 4);
    hipLaunchKernelGGL((fa_decode_combine_kernel<D, T>), dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(256), 0, s, p);
    return hipGetLastError();
  }
  return hipSuccess;
}

hipError_t launch_decode(const DecodeParams& p, int dtype, hipStream_t s) {
  if (p.D == 64) return dtype == 1 ? launch_decode_t<64, BF16>(p, s) : launch_decode_t<64, FP16>(p, s);
  if (p.D == 128) return dtype == 1 ? launch_decode_t<128, BF16>(p, s) : launch_decode_t<128, FP16>(p, s);
  return hipErrorInvalidValue;
}

}  // namespace fa
