// MLA (multi-head latent attention) decoding over a paged latent cache: include_mla/mi355fa_kvcache_mla.h.
//
// DeepSeek-V2 / V3 / R1 and Kimi-K2 cache ONE row of 576 values per token -- 512 latent dims and 64 RoPE dims -- that all H
// query heads share.  In the absorbed decode form a query head has those 576 dims, the key of a token is its whole row and
// its value is the first 512 values of the same row: D_qk = 576, D_v = 512, H_kv = 1, and K and V are the same bytes.
//
//   fa_kvcache_append_paged_kernel<MLA, T>  kv_new rows -> cache rows seqlens[b] + j through the table  (first, same stream)
//   fa_decode_paged_kernel<MLA, T>          one workgroup per (sequence, 32-row block of the H * S_q rows, split)
//   fa_decode_combine_kernel<512, T>        nsplit > 1: the shared combine kernel (fa_decode_combine.inc) at the latent width
// (overloads of the decode kernels' names by their template parameters: the MLA tag is a type, which no other overload takes
// first.)
//
// The attention kernel is built from what fa_decode_body.inc has and has measured.  The MFMA rows are the H * S_q (query, head)
// rows, query-major (row = i * H + head: the body's mapping with g = H and one K/V head), so a latent byte is read once per 32
// rows.  All four waves work on the SAME 32-key tile and wave w owns a quarter of the head dim: latent columns
// [128 w, 128 w + 128) and RoPE columns [512 + 16 w, 512 + 16 w + 16).  Per wave and tile:
//   K = V  lane (r, h) loads key r's nine 16-byte pieces straight into the MFMA A layout -- eight of the latent quarter, one of
//          the RoPE slice --, prefetched one tile ahead.  The eight latent pieces go from the same registers into the wave's
//          swizzled 32 x 128 LDS tile (lds_off<128>, chunk 2 ks + h): there is no second global load for V.
//   S^T    the wave's partial = 9 MFMA k-steps against the Q fragments gathered once at the same columns.
//   exchange  each wave writes its partial to an LDS slot chosen by step parity, and behind ONE workgroup barrier all four
//          waves add the four partials as (p0 + p1) + (p2 + p3): the same bits in every wave, so one m, l and P per row.  It is
//          the D = 256 exchange (two slots per wave) widened from pairs to four, and its ordering argument carries over: the
//          write of step k + 2 into the slot of step k follows the barrier of step k + 1, which a wave joins only once its
//          reads of step k have returned (xch_sync waits for lgkmcnt(0) in front of the barrier).
//   softmax, O^T += V^T P^T on the wave's 128 latent columns: the D = 128 wave's code (lds_read_tr_frag, tr_lane_off<128>).
// The paged lookup is the body's PAGED pipeline: a scalar table entry looked up a step ahead through the constant address
// space and a descriptor rebased on the page that covers the page's rows below L only; an entry outside the pool gives an
// empty descriptor.  No access leaves the pool whatever the table or cache_seqlens hold, and rows at or past L are never read.
// There is one key group, so the merge only lays the four waves' 128 columns side by side (fp32 rows of 512 + 4) and writes
// O / LSE (one split) or the fp32 partial (O, m, l) in the decode calls' workspace layout with D = 512.  Every order is fixed:
// the result is deterministic.
// LDS: 32 KiB of V tiles + 32 KiB of exchange slots in the loop, the 64.5 KiB merge stage over them: 64.75 KiB, two workgroups
// per CU.
#include <algorithm>

#include "fa_common.h"
#include "fa_decode_mla.h"

namespace fa {

#include "fa_decode_combine.inc"

namespace {

constexpr int kMlaTile = 32;    // keys per step
constexpr int kMlaRows = 32;    // MFMA rows per workgroup
constexpr int kMlaWaves = 4;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;

struct MlaCfg {
  static constexpr int HD = kMlaDv / kMlaWaves;             // the latent columns of one wave: the D = 128 wave's tile
  static constexpr int RD = (kMlaD - kMlaDv) / kMlaWaves;   // its RoPE columns: one k-step
  static constexpr int KS = HD / 16;                        // latent k-steps of S^T = K Q^T
  static constexpr int DB = HD / 32;                        // 32-column blocks of the wave's O^T
  static constexpr int ROWB = HD * 2;                       // a row of the wave's V tile
  static constexpr int VT_BYTES = kMlaWaves * kMlaTile * ROWB;
  static constexpr int XCH_OFF = VT_BYTES;                  // behind the V tiles
  static constexpr int XCH_SLOT = 64 * 16 * 4;              // one wave's 32 x 32 fp32 partial scores
  static constexpr int LOOP_BYTES = XCH_OFF + 2 * kMlaWaves * XCH_SLOT;
  static constexpr int OST = kMlaDv + 4;                    // fp32 row stride of the merge stage (bank spread)
  static constexpr int MERGE_BYTES = kMlaRows * OST * 4;
  static constexpr int ML_OFF = MERGE_BYTES;
  static constexpr int LDS_BYTES = (LOOP_BYTES > MERGE_BYTES ? LOOP_BYTES : MERGE_BYTES) + 2 * kMlaRows * 4;
  static_assert(RD == 16, "the RoPE slice of a wave is one MFMA k-step");
  static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU");
};

}  // namespace

template <typename TAG, typename T>
__global__ __launch_bounds__(256, 2) void fa_decode_paged_kernel(MlaParams p) {
  static_assert(std::is_same<TAG, MLA>::value, "the MLA overload");
  using C = MlaCfg;
  using vec8 = typename T::vec8;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  FA_LDS char* smem = (FA_LDS char*)smem_raw;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- work item: (b * RB + rb) * nsplit + split ----
  const int g = p.H, M = g * p.Sq, RB = (M + kMlaRows - 1) / kMlaRows;
  int w = blockIdx.x;
  const int split = w % p.nsplit;
  w /= p.nsplit;
  const int rb = w % RB, b = w / RB;
  const int L = min(max(p.seqlens[b] + p.Snew, 0), p.Scache);

  // ---- this row block's visible key tiles (from tile 0: `causal` is the only mask), and this split's share of them ----
  const int r0 = rb * kMlaRows, rlast = min(M, r0 + kMlaRows) - 1;
  const int pos1 = L - p.Sq + rlast / g;   // position of the block's last query
  const int hi = p.causal ? min(L, pos1 + 1) : L;
  const int nt = hi > 0 ? (hi + kMlaTile - 1) / kMlaTile : 0;
  const int s_beg = (int)((long long)nt * split / p.nsplit);
  const int s_end = (int)((long long)nt * (split + 1) / p.nsplit);

  // ---- this lane's query row: the Q^T fragments (B operand) of the wave's columns, its position ----
  const int qrow = r0 + r, qi = qrow / g, qh = qrow - qi * g;
  const int pos = L - p.Sq + qi;
  vec8 qf[C::KS + 1];
  {
    const bool valid = qrow < M;
    const char* qp = (const char*)p.q + b * p.lq.sb + (long long)qh * p.lq.sh + (long long)qi * p.lq.rs + 16 * h;
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks)
      qf[ks] = as_vec8<T>(valid ? *(const u32x4*)(qp + 2 * C::HD * wave + 32 * ks) : u32x4{0u, 0u, 0u, 0u});
    qf[C::KS] = as_vec8<T>(valid ? *(const u32x4*)(qp + 2 * kMlaDv + 2 * C::RD * wave) : u32x4{0u, 0u, 0u, 0u});
  }

  FA_LDS char* vt = smem + wave * kMlaTile * C::ROWB;
  int v_off[2][C::DB];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int db = 0; db < C::DB; ++db) v_off[e][db] = tr_lane_off<C::HD>(lane, 8 * e, db);

  // ---- the paged lookup (fa_decode_body.inc, PAGED): tile t lies in page page_of(t) of the pool, and its descriptor covers
  // that page's rows below L only, based on the page (a 64-bit base: the pool may exceed 2^32 bytes).  The entry is
  // wave-uniform, read through the constant address space (nothing writes the table while the kernel runs) so that it is a
  // scalar load the loop's own lgkmcnt(0) retires.  An entry outside the pool gives an empty descriptor at the pool's base.
  const int rs = p.kv_rs;
  typedef const __attribute__((address_space(4))) int* const_table_t;
  const const_table_t table = (const_table_t)p.table + (long long)b * p.bt_stride;
  auto page_of = [&](int t) __attribute__((always_inline)) {
    return __builtin_amdgcn_readfirstlane(table[p.tpp.div(t)]);
  };
  __amdgpu_buffer_rsrc_t rkp = make_rsrc(p.kv, 0u);
  int basep = 0;
  auto page_desc = [&](int t, int pg) __attribute__((always_inline)) {
    const int first = p.tpp.div(t) * p.page_size;                         // the page's first key
    const int ok = (unsigned)pg < (unsigned)p.num_pages ? 1 : 0;
    rkp = make_rsrc((const char*)p.kv + (long long)(pg * ok) * p.kv_ps, view_bytes(min(L - first, p.page_size) * ok, rs, kMlaRowB));
    basep = (t * kMlaTile - first) * rs;
  };
  // key r's pieces: the latent quarter's 16 bytes at d = 128 w + 16 ks + 8 h, the RoPE slice's at d = 512 + 16 w + 8 h
  const int klat = r * rs + 2 * C::HD * wave + 16 * h, krope = r * rs + 2 * kMlaDv + 2 * C::RD * wave + 16 * h;
  u32x4 kr[C::KS + 1];
  auto load_paged = [&]() __attribute__((always_inline)) {   // the tile (rkp, basep) describe
    const int base = basep;
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) kr[ks] = buf_load16(rkp, base + klat + 32 * ks);
    kr[C::KS] = buf_load16(rkp, base + krope);
  };

  const float c2 = p.scale * kLog2e;   // scores in log2 units
  float m = -INFINITY, l = 0.f;
  f32x16 oacc[C::DB];
#pragma unroll
  for (int db = 0; db < C::DB; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[db][i] = 0.f;

  // At the top of step t the loads of tile t are in flight, (rkp, basep) describe tile t + 1 and pgn is the table entry of
  // tile t + 2.  Only tiles below s_end are looked up: entries at or past ceil(L / page_size) are never read.
  int t = s_beg;
  int pgn = 0;
  if (t < s_end) {
    page_desc(t, page_of(t));
    load_paged();
    if (t + 1 < s_end) page_desc(t + 1, page_of(t + 1));
    if (t + 2 < s_end) pgn = page_of(t + 2);
  }
  // Every wave runs every step (s_beg / s_end are workgroup-uniform), so every wave joins every barrier.
  FA_LDS char* xch = smem + C::XCH_OFF;
  auto xch_sync = [&]() __attribute__((always_inline)) {   // this wave's LDS writes have landed and its reads returned
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(waitcnt_imm(kNoWait, 0));
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  for (; t < s_end; ++t) {
    // V of tile t = the latent pieces of K, into the wave's LDS tile (the previous tile's transposed reads precede these
    // writes in LDS order)
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) lds_write16(vt + lds_off<C::HD>(r, 2 * ks + h), kr[ks]);
    u32x4 kc[C::KS + 1];
#pragma unroll
    for (int ks = 0; ks <= C::KS; ++ks) kc[ks] = kr[ks];
    if (t + 1 < s_end) load_paged();   // next tile in flight while this one is computed

    // ---- the wave's partial S^T = K Q^T over its columns: reg i of lane (r, h) = query row r, key t*32 + (i&3) + 8(i>>2) + 4h
    f32x16 s;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks <= C::KS; ++ks) s = T::mfma(as_vec8<T>(kc[ks]), qf[ks], s);
    {
      // The four partials cross the workgroup through two slots per wave, taken by step parity, behind ONE barrier per step:
      // the write of step k + 2 follows the barrier of step k + 1, which every other wave joins only once its reads of step k
      // have returned.  Every wave then adds the same four values in the same association, (p0 + p1) + (p2 + p3) -- the same
      // bits, so the workgroup holds one m, l and P for the four quarters of a row.
      // (a slot: 16 registers of 64 lanes, as four wave-contiguous 16-byte rows)
      const int par = (t - s_beg) & 1;
      FA_LDS char* slots = xch + par * kMlaWaves * C::XCH_SLOT + lane * 16;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        *(FA_LDS f32x4*)(slots + wave * C::XCH_SLOT + c * (C::XCH_SLOT / 4)) = f32x4{s[4 * c], s[4 * c + 1], s[4 * c + 2], s[4 * c + 3]};
      xch_sync();
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        f32x4 pw[kMlaWaves];
#pragma unroll
        for (int v = 0; v < kMlaWaves; ++v) pw[v] = *(const FA_LDS f32x4*)(slots + v * C::XCH_SLOT + c * (C::XCH_SLOT / 4));
#pragma unroll
        for (int j = 0; j < 4; ++j) s[4 * c + j] = (pw[0][j] + pw[1][j]) + (pw[2][j] + pw[3][j]);
      }
    }
    float tm = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int key = t * kMlaTile + (i & 3) + 8 * (i >> 2) + 4 * h;
      const bool dead = key >= L || (p.causal && key > pos);
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
    // ---- O^T += V^T P^T on the wave's latent columns ----
    const vec8 pf0 = pack8<T, 0>(s), pf1 = pack8<T, 1>(s);
    __builtin_amdgcn_s_waitcnt(waitcnt_imm(kNoWait, 0));   // this wave's V writes have landed
    // the descriptor two tiles ahead from the entry looked up a step ago; the next lookup
    if (t + 2 < s_end) page_desc(t + 2, pgn);
    if (t + 3 < s_end) pgn = page_of(t + 3);
#pragma unroll
    for (int db = 0; db < C::DB; ++db) {
      const vec8 a0 = lds_read_tr_frag<T>(vt + v_off[0][db], vt + v_off[1][db]);
      oacc[db] = T::mfma(a0, pf0, oacc[db]);
      const vec8 a1 = lds_read_tr_frag<T>(vt + 16 * C::ROWB + v_off[0][db], vt + 16 * C::ROWB + v_off[1][db]);
      oacc[db] = T::mfma(a1, pf1, oacc[db]);
    }
  }
  const float lt = half_sum(l);

  // ---- merge: one key group, so the four waves' quarters side by side (every wave holds the same m and l: wave 0 writes
  // them), then O / LSE or the split's partial ----
  __syncthreads();   // every wave is done with its V tile and the exchange slots: the LDS is the merge stage now
  float* stage = (float*)smem_raw;
  float* sm = (float*)(smem_raw + C::ML_OFF);
  float* sl = sm + kMlaRows;
  if (h == 0 && wave == 0) {
    sm[r] = m;
    sl[r] = lt;
  }
#pragma unroll
  for (int db = 0; db < C::DB; ++db)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      *(f32x4*)(stage + r * C::OST + C::HD * wave + db * 32 + 8 * c + 4 * h) =
          f32x4{oacc[db][4 * c], oacc[db][4 * c + 1], oacc[db][4 * c + 2], oacc[db][4 * c + 3]};
  __syncthreads();
  const long long R = (long long)p.B * p.H * p.Sq;   // rows of O / LSE / a split's partials
  for (int it = tid; it < kMlaRows * (kMlaDv / 4); it += 256) {
    const int row = it / (kMlaDv / 4), d4 = (it % (kMlaDv / 4)) * 4;
    const int qr = r0 + row;
    if (qr >= M) break;   // rows ascend with `it`
    const float mx = sm[row], lsum = sl[row];
    const f32x4 acc = *(const f32x4*)(stage + row * C::OST + d4);
    const int i = qr / g, head = qr - i * g;
    const long long ridx = ((long long)b * p.H + head) * p.Sq + i;
    if (p.nsplit == 1) {
      const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
      typedef __attribute__((ext_vector_type(4))) typename T::elem e4;
      e4 ov;
#pragma unroll
      for (int j = 0; j < 4; ++j) ov[j] = (typename T::elem)(acc[j] * inv);
      *(u32x2*)((char*)p.o + b * p.lo.sb + (long long)head * p.lo.sh + (long long)i * p.lo.rs + d4 * 2) =
          __builtin_bit_cast(u32x2, ov);
      if (d4 == 0 && p.lse) p.lse[ridx] = lsum > 0.f ? (mx + __builtin_log2f(lsum)) * kLn2 : -INFINITY;
    } else {
      const long long pr = split * R + ridx;
      *(f32x4*)(p.ws + pr * kMlaDv + d4) = acc;
      if (d4 == 0) *(f32x2_t*)(p.ws + (long long)p.nsplit * R * kMlaDv + 2 * pr) = f32x2_t{mx, lsum};
    }
  }
}

// The append: kv_new [B, S_new, 576] -> cache rows seqlens[b] + j through the table, one 16-byte chunk per thread, as
// fa_kvcache_append_paged_kernel does.  A row outside [0, Scache), or whose table entry is outside the pool, is dropped.
// (T: the rows are copied, whatever 16-bit type they hold; the instances follow the attention kernel's.)
template <typename TAG, typename T>
__global__ __launch_bounds__(256) void fa_kvcache_append_paged_kernel(MlaParams p) {
  static_assert(std::is_same<TAG, MLA>::value, "the MLA overload");
  constexpr int cpr = kMlaRowB / 16;
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)p.B * p.Snew * cpr) return;
  const int c = (int)(item % cpr);
  const long long rowi = item / cpr;   // b * S_new + j
  const int j = (int)(rowi % p.Snew), b = (int)(rowi / p.Snew);
  const int dst = p.seqlens[b] + j;
  if (dst < 0 || dst >= p.Scache) return;
  const int pi = dst / p.page_size;
  const int page = p.table[(long long)b * p.bt_stride + pi];
  if ((unsigned)page >= (unsigned)p.num_pages) return;
  *(u32x4*)((char*)p.kv + page * p.kv_ps + (long long)(dst - pi * p.page_size) * p.kv_rs + c * 16) =
      *(const u32x4*)((const char*)p.kv_new + rowi * kMlaRowB + c * 16);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// Split count: up to two workgroups per CU (512 over (sequence, row block, split)) and splits of at least sqrt(16 * S_cache)
// keys (n <= sqrt(S_cache / 16)), at most 64.  A rule of its own, not the D = 128 one: as at D = 256 every step ends at a
// workgroup barrier and a workgroup takes ONE tile per step here, so a split streams its keys at a quarter of the D = 128
// rate and the machine fills only once the budget is used.  DESIGN.md section 3 has the forced-split sweep behind it
// (profiles/mla_split_sweep.jsonl) and how far the rule lies from the best swept count at each point.
int mla_splits(long long wgs, int S_cache, int forced) {
  if (forced > 0) return forced;
  constexpr int kMaxSplits = 64, kTargetWgs = 512, kKeys = 16;
  wgs = std::max<long long>(1, wgs);
  long long n = (kTargetWgs + wgs - 1) / wgs;
  long long by_len = 1;
  while ((by_len + 1) * (by_len + 1) * kKeys <= S_cache) ++by_len;
  n = std::min(n, by_len);
  return (int)std::max<long long>(1, std::min<long long>(n, kMaxSplits));
}

template <typename T>
static hipError_t launch_decode_mla_t(const MlaParams& p, hipStream_t s) {
  if (p.Snew > 0) {
    const long long items = (long long)p.B * p.Snew * (kMlaRowB / 16);
    hipLaunchKernelGGL((fa_kvcache_append_paged_kernel<MLA, T>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, p);
    if (hipError_t e = hipGetLastError()) return e;
  }
  const long long wgs = (long long)p.B * decode_row_blocks(p.H, p.Sq);
  if (hipError_t e = launch_kernel<fa_decode_paged_kernel<MLA, T>>((unsigned)(wgs * p.nsplit), 256, MlaCfg::LDS_BYTES, s, p)) return e;
  if (p.nsplit <= 1) return hipSuccess;
  // the shared combine kernel reads the workspace, the split count and O / LSE from the decode calls' parameter block
  DecodeParams d{};
  d.o = p.o;
  d.lse = p.lse;
  d.ws = p.ws;
  d.lo = p.lo;
  d.B = p.B;
  d.H = p.H;
  d.Sq = p.Sq;
  d.D = kMlaDv;
  d.nsplit = p.nsplit;
  const long long rows = (long long)p.B * p.H * p.Sq, rpb = 256 / (kMlaDv / 4);
  hipLaunchKernelGGL((fa_decode_combine_kernel<kMlaDv, T>), dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(256), 0, s, d);
  return hipGetLastError();
}

hipError_t launch_decode_mla(const MlaParams& p, int dtype, hipStream_t s) {
  return dtype == 1 ? launch_decode_mla_t<BF16>(p, s) : launch_decode_mla_t<FP16>(p, s);
}

}  // namespace fa
