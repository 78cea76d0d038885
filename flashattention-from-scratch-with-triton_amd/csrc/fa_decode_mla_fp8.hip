// MLA decoding over a paged FP8 latent cache: include_mla_fp8/mi355fa_kvcache_mla_fp8.h.
//
// The cache of fa_decode_mla.hip at about half the bytes: a token's row is 656 bytes -- 512 OCP e4m3 bytes for the latent dims,
// four fp32 scales (scale j belongs to dims [128 j, 128 j + 128)) and the 64 RoPE values in the call's 16-bit type.  The key of
// a token is byte * scale on the latent dims followed by the RoPE dims, its value the latent part alone.
//
//   fa_kvcache_append_paged_kernel<Fp8Row, T>  kv_new rows (16-bit) -> quantised rows seqlens[b] + j through the table
//   fa_decode_paged_kernel<Fp8Row, T>          one workgroup per (sequence, 32-row block of the H * S_q rows, split)
//   fa_decode_combine_kernel<Fp8Row, T>        nsplit > 1: the partials of the decode calls' workspace layout at D = 512 -> O, LSE
// (overloads of the decode kernels' names by their template parameters: the Fp8Row tag is a type, which no other overload takes
// first.)
//
// The work split is the 16-bit kernel's (fa_decode_mla.hip says why): the MFMA rows are the H * S_q (query, head) rows, all four
// waves work on the SAME 32-key tile and wave w owns latent columns [128 w, 128 w + 128) and RoPE columns [512 + 16 w, + 16),
// the four partial scores cross LDS behind one barrier per step and are added as (p0 + p1) + (p2 + p3) in every wave, the table
// entry is looked up a step ahead through the constant address space, and a page's descriptor covers its rows below L only.
// The scale block of the format IS the wave's quarter, so a wave needs ONE scale per key.  The byte path, per wave and tile:
//   loads    lane (r, h) loads key r's latent bytes as four 16-byte pieces -- piece j holds columns 32 j + 16 h + [0, 16) of the
//            quarter: two MFMA k-steps of eight columns each -- where the 16-bit kernel loads eight, the RoPE slice as one
//            16-byte piece of 16-bit values, and the scale of key r as one dword; all prefetched one tile ahead.  The Q fragments
//            are gathered once with the same permutation of the contraction index (k-step ks = 2 j + e reads the columns
//            32 j + 16 h + 8 e + [0, 8)), as fa_decode_body.inc does for its e4m3 caches.
//   convert  v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0: the bytes become T's values without rounding, UNSCALED.
//   scores   eight latent k-steps on the unscaled values; then register i of the partial is multiplied by the scale of its key
//            in fp32 -- the scale enters the score exactly, no dequantised key is ever rounded --; only then the RoPE k-step
//            accumulates on top (RoPE is not scaled).  The 32 scales of the tile go through 128 bytes of wave-private LDS: lane
//            r writes key r's, lane half h reads back four 16-byte rows, the 16 scales of its keys (i & 3) + 8 (i >> 2) + 4 h.
//   values   the V tile in LDS holds the same converted, unscaled values, at the 16-bit kernel's swizzled positions (chunk
//            4 j + 2 h + e), so the transposed reads are the 16-bit kernel's.  The wave folds its own scale into its own copy
//            of P before packing it to 16 bits (p[i] * scale[i]: the same 16 scale registers the scores used); m and l use the
//            unscaled p.  The weights p * scale are packed in units of the row's largest weight so far and the accumulator is
//            kept in those units (the loop says why): the largest weight is exactly 1, as the largest p is in the 16-bit
//            kernel, and no fp16 range limit is left.
//            (A byte tile in LDS would save 16 KiB that nothing here is short of -- LDS allows two workgroups per CU either
//            way -- and would need a byte-transposed read plus the conversions on the PV side a second time.)
// No access leaves the pool whatever the table or cache_seqlens hold, and rows at or past L are never read.  Every order is
// fixed: the result is deterministic.
// LDS: 32 KiB of V tiles + 32 KiB of exchange slots + 512 bytes of scales in the loop, the 64.5 KiB merge stage over them:
// 64.75 KiB with the (m, l) rows, two workgroups per CU.
#include <algorithm>

#include "fa_common.h"
#include "fa_decode_mla_fp8.h"

namespace fa {

namespace {

constexpr int kTile = 32;    // keys per step
constexpr int kRows = 32;    // MFMA rows per workgroup
constexpr int kWaves = 4;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;

struct Fp8RowCfg {
  static constexpr int HD = kMlaDv / kWaves;             // the latent columns of one wave = one scale block of the format
  static constexpr int RD = (kMlaD - kMlaDv) / kWaves;   // its RoPE columns: one k-step
  static constexpr int KS = HD / 16;                     // latent k-steps of S^T = K Q^T
  static constexpr int KL = HD / 32;                     // 16-byte loads of latent bytes per lane and tile: two k-steps each
  static constexpr int DB = HD / 32;                     // 32-column blocks of the wave's O^T
  static constexpr int ROWB = HD * 2;                    // a row of the wave's V tile (converted to 16 bits)
  static constexpr int VT_BYTES = kWaves * kTile * ROWB;
  static constexpr int XCH_OFF = VT_BYTES;               // behind the V tiles
  static constexpr int XCH_SLOT = 64 * 16 * 4;           // one wave's 32 x 32 fp32 partial scores
  static constexpr int SCL_OFF = XCH_OFF + 2 * kWaves * XCH_SLOT;   // behind the exchange slots: the waves' scale slots
  static constexpr int SCL_SLOT = kTile * 4;             // per wave: the tile's 32 scales
  static constexpr int LOOP_BYTES = SCL_OFF + kWaves * SCL_SLOT;
  static constexpr int OST = kMlaDv + 4;                 // fp32 row stride of the merge stage (bank spread)
  static constexpr int MERGE_BYTES = kRows * OST * 4;
  static constexpr int ML_OFF = LOOP_BYTES > MERGE_BYTES ? LOOP_BYTES : MERGE_BYTES;
  static constexpr int LDS_BYTES = ML_OFF + 2 * kRows * 4;
  static_assert(HD == 128, "a wave's quarter is one 128-dim scale block");
  static_assert(RD == 16, "the RoPE slice of a wave is one MFMA k-step");
  static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU");
};

// Eight OCP e4m3 bytes (two dwords, ascending addresses) -> eight values of T in the same order.  Exact: every e4m3 value,
// subnormals included, is a normal fp16 and bf16 number.  (fa_decode.hip's cvt_fp8, static to that unit.)
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

// four values of T (two dwords) -> the four e4m3 bytes e4m3_rne(clamp(float(x) / d, -448, 448)), in the same order: the
// correctly rounded fp32 division, an explicit clamp, v_cvt_pk_fp8_f32's round to nearest even (fa_decode.hip's quant4_fp8)
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

// The scale of a block with that amax: amax / 448, the correctly rounded fp32 division; 1 where the quotient is not a normal
// number (a zero block, a subnormal quotient).
FA_DEVINL float block_scale_fp8(float amax) {
  const float s = amax / 448.f;
  const unsigned field = (__builtin_bit_cast(unsigned, s) >> 23) & 0xffu;
  return field - 1u < 254u ? s : 1.f;
}

}  // namespace

template <typename TAG, typename T>
__global__ __launch_bounds__(256, 2) void fa_decode_paged_kernel(Fp8RowParams p) {
  static_assert(std::is_same<TAG, Fp8Row>::value, "the FP8 latent cache overload");
  using C = Fp8RowCfg;
  using vec8 = typename T::vec8;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  FA_LDS char* smem = (FA_LDS char*)smem_raw;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- work item: (b * RB + rb) * nsplit + split ----
  const int Sq = p.Sq;
  const int g = p.H, M = g * Sq, RB = (M + kRows - 1) / kRows;
  int w = blockIdx.x;
  const int split = w % p.nsplit;
  w /= p.nsplit;
  const int rb = w % RB, b = w / RB;
  const int L = min(max(p.seqlens[b] + p.Snew, 0), p.Scache);

  // ---- this row block's visible key tiles (from tile 0: `causal` is the only mask), and this split's share of them ----
  const int r0 = rb * kRows, rlast = min(M, r0 + kRows) - 1;
  const int pos1 = L - Sq + rlast / g;   // position of the block's last query
  const int hi = p.causal ? min(L, pos1 + 1) : L;
  const int nt = hi > 0 ? (hi + kTile - 1) / kTile : 0;
  const int s_beg = (int)((long long)nt * split / p.nsplit);
  const int s_end = (int)((long long)nt * (split + 1) / p.nsplit);

  // ---- this lane's query row: the Q^T fragments (B operand) of the wave's columns in the byte loads' order, its position ----
  const int qrow = r0 + r, qi = qrow / g, qh = qrow - qi * g;
  const int pos = L - Sq + qi;
  vec8 qf[C::KS + 1];
  {
    const bool valid = qrow < M;
    const char* qp = (const char*)p.q + b * p.lq.sb + (long long)qh * p.lq.sh + (long long)qi * p.lq.rs;
    // k-step ks = 2 j + e: columns 128 w + 32 j + 16 h + 8 e + [0, 8), what bytes [8 e, 8 e + 8) of the lane's piece j hold
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks)
      qf[ks] = as_vec8<T>(valid ? *(const u32x4*)(qp + 2 * C::HD * wave + 64 * (ks >> 1) + 32 * h + 16 * (ks & 1))
                                : u32x4{0u, 0u, 0u, 0u});
    qf[C::KS] = as_vec8<T>(valid ? *(const u32x4*)(qp + 2 * kMlaDv + 2 * C::RD * wave + 16 * h) : u32x4{0u, 0u, 0u, 0u});
  }

  FA_LDS char* vt = smem + wave * kTile * C::ROWB;
  FA_LDS char* scl = smem + C::SCL_OFF + wave * C::SCL_SLOT;   // the tile's 32 scales of this wave's quarter
  int v_off[2][C::DB];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int db = 0; db < C::DB; ++db) v_off[e][db] = tr_lane_off<C::HD>(lane, 8 * e, db);

  // ---- the paged lookup (fa_decode_mla_body.inc's): tile t lies in page page_of(t) of the pool, and its descriptor covers that
  // page's rows below L only, based on the page (a 64-bit base: the pool may exceed 2^32 bytes).  The entry is wave-uniform,
  // read through the constant address space (nothing writes the table while the kernel runs).  An entry outside the pool
  // gives an empty descriptor at the pool's base: its bytes, scales and RoPE values read as 0.
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
    rkp = make_rsrc((const char*)p.kv + (long long)(pg * ok) * p.kv_ps, view_bytes(min(L - first, p.page_size) * ok, rs, kFp8RowB));
    basep = (t * kTile - first) * rs;
  };
  // key r's pieces: latent piece j at byte 128 w + 32 j + 16 h, the scale of the quarter at 512 + 4 w, the RoPE slice's 16 bytes
  // at 528 + 32 w + 16 h
  const int klat = r * rs + C::HD * wave + 16 * h, kscl = r * rs + kFp8RowScaleOff + 4 * wave,
            krope = r * rs + kFp8RowRopeOff + 2 * C::RD * wave + 16 * h;
  u32x4 kr[C::KL + 1];
  float ksc = 0.f;
  auto load_paged = [&]() __attribute__((always_inline)) {   // the tile (rkp, basep) describe
    const int base = basep;
#pragma unroll
    for (int j = 0; j < C::KL; ++j) kr[j] = buf_load16(rkp, base + klat + 32 * j);
    kr[C::KL] = buf_load16(rkp, base + krope);
    ksc = buf_load_f32(rkp, base + kscl);
  };

  const float c2 = p.scale * kLog2e;   // scores in log2 units
  float m = -INFINITY, l = 0.f;
  float unit = 0.f;   // oacc holds this wave's quarter in units of `unit`: the row's largest weight p * scale so far (below)
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
    u32x4 kc[C::KL + 1];
#pragma unroll
    for (int j = 0; j <= C::KL; ++j) kc[j] = kr[j];
    // the tile's scales: lane r brings key r's (both halves write the same value), the wave reads them back below.  The slot
    // is this wave's own and LDS serves a wave's requests in order: the previous tile's reads precede this write.
    *(FA_LDS float*)(scl + 4 * r) = ksc;
    if (t + 1 < s_end) load_paged();   // next tile in flight while this one is computed

    // ---- the wave's partial S^T = K Q^T over its latent columns, on the unscaled values: reg i of lane (r, h) = query row r,
    // key t*32 + (i&3) + 8(i>>2) + 4h.  The same values are V of tile t: into the wave's LDS tile at the columns they hold
    // (chunk 4 j + 2 h + e = columns 32 j + 16 h + 8 e; the previous tile's transposed reads precede these writes in LDS order)
    f32x16 s;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
    for (int j = 0; j < C::KL; ++j)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const u32x4 kv16 = cvt_fp8<T>(kc[j][2 * e], kc[j][2 * e + 1]);
        lds_write16(vt + lds_off<C::HD>(r, 4 * j + 2 * h + e), kv16);
        s = T::mfma(as_vec8<T>(kv16), qf[2 * j + e], s);
      }
    // ---- the scales of this half's 16 keys, one per score register; then the RoPE k-step on top, unscaled ----
    asm volatile("" ::: "memory");
    f32x4 sv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) sv[c] = *(const FA_LDS f32x4*)(scl + 16 * (2 * c + h));
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] *= sv[i >> 2][i & 3];
    s = T::mfma(as_vec8<T>(kc[C::KL]), qf[C::KS], s);
    {
      // The four partials cross the workgroup through two slots per wave, taken by step parity, behind ONE barrier per step:
      // the write of step k + 2 follows the barrier of step k + 1, which every other wave joins only once its reads of step k
      // have returned.  Every wave then adds the same four values in the same association, (p0 + p1) + (p2 + p3) -- the same
      // bits, so the workgroup holds one m, l and P for the four quarters of a row.
      // (a slot: 16 registers of 64 lanes, as four wave-contiguous 16-byte rows)
      const int par = (t - s_beg) & 1;
      FA_LDS char* slots = xch + par * kWaves * C::XCH_SLOT + lane * 16;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        *(FA_LDS f32x4*)(slots + wave * C::XCH_SLOT + c * (C::XCH_SLOT / 4)) = f32x4{s[4 * c], s[4 * c + 1], s[4 * c + 2], s[4 * c + 3]};
      xch_sync();
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        f32x4 pw[kWaves];
#pragma unroll
        for (int v = 0; v < kWaves; ++v) pw[v] = *(const FA_LDS f32x4*)(slots + v * C::XCH_SLOT + c * (C::XCH_SLOT / 4));
#pragma unroll
        for (int j = 0; j < 4; ++j) s[4 * c + j] = (pw[0][j] + pw[1][j]) + (pw[2][j] + pw[3][j]);
      }
    }
    float tm = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int key = t * kTile + (i & 3) + 8 * (i >> 2) + 4 * h;
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
    float ls[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      s[i] = __builtin_amdgcn_exp2f(s[i] - mu);
      ls[i & 3] += s[i];
    }
    l += (ls[0] + ls[1]) + (ls[2] + ls[3]);
    // ---- O^T += V^T P^T on the wave's latent columns: V is unscaled, so this wave's copy of P takes the scales of its quarter
    // (a key at or past L has p = 0 and reads as byte 0 and scale 0).  The weights w = p * scale are packed to 16 bits in units
    // of the row's largest weight so far, `unit`, and the accumulator is kept in those units: the largest weight packs to
    // exactly 1, as the largest p of a row does in the 16-bit kernel, so a row whose softmax is one-hot gets its key's value
    // back without a rounding of P -- packed as it is, p * scale would fall anywhere in a binade and cost up to half an ulp of
    // T there -- and no weight that matters can leave T's normal range.  unit only grows in the current maximum's terms:
    // the accumulator is rescaled by corr * unit_old / unit_new <= 1 where the 16-bit kernel rescales by corr.
    float tw = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      s[i] *= sv[i >> 2][i & 3];
      tw = __builtin_fmaxf(tw, s[i]);
    }
    const float un = __builtin_fmaxf(unit * corr, half_max(tw));
    const float iu = un > 0.f ? 1.f / un : 0.f;   // (no weight yet: the accumulator is 0 and stays 0)
    const float resc = unit * corr * iu;
    unit = un;
#pragma unroll
    for (int db = 0; db < C::DB; ++db)
#pragma unroll
      for (int i = 0; i < 16; ++i) oacc[db][i] *= resc;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] *= iu;
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
  // this wave's quarter out of its units
#pragma unroll
  for (int db = 0; db < C::DB; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[db][i] *= unit;

  // ---- merge: one key group, so the four waves' quarters side by side (every wave holds the same m and l: wave 0 writes
  // them), then O / LSE or the split's partial ----
  __syncthreads();   // every wave is done with its V tile, its scales and the exchange slots: the LDS is the merge stage now
  float* stage = (float*)smem_raw;
  float* sm = (float*)(smem_raw + C::ML_OFF);
  float* sl = sm + kRows;
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
  const long long R = (long long)p.B * p.H * Sq;   // rows of O / LSE / a split's partials
  for (int it = tid; it < kRows * (kMlaDv / 4); it += 256) {
    const int row = it / (kMlaDv / 4), d4 = (it % (kMlaDv / 4)) * 4;
    const int qr = r0 + row;
    if (qr >= M) break;   // rows ascend with `it`
    const float mx = sm[row], lsum = sl[row];
    const f32x4 acc = *(const f32x4*)(stage + row * C::OST + d4);
    const int i = qr / g, head = qr - i * g;
    const long long ridx = ((long long)b * p.H + head) * Sq + i;
    if (p.nsplit == 1) {
      const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
      typedef __attribute__((ext_vector_type(4))) typename T::elem e4;
      e4 ov;
#pragma unroll
      for (int j = 0; j < 4; ++j) ov[j] = (typename T::elem)(acc[j] * inv);
      *(u32x2*)((char*)p.o + b * p.lo.sb + (long long)head * p.lo.sh + (long long)i * p.lo.rs + d4 * 2) = __builtin_bit_cast(u32x2, ov);
      if (d4 == 0 && p.lse) p.lse[ridx] = lsum > 0.f ? (mx + __builtin_log2f(lsum)) * kLn2 : -INFINITY;
    } else {
      const long long pr = split * R + ridx;
      *(f32x4*)(p.ws + pr * kMlaDv + d4) = acc;
      if (d4 == 0) *(f32x2_t*)(p.ws + (long long)p.nsplit * R * kMlaDv + 2 * pr) = f32x2_t{mx, lsum};
    }
  }
}

// The quantising append: kv_new [B, S_new, 576] (T) -> cache rows seqlens[b] + j through the table.  A row takes 40 threads in
// five aligned groups of eight lanes.  Groups 0 .. 3 take one 128-dim block each, 16 values per thread: amax over the thread's
// values and then across the group (three xor steps), s = amax / 448 -- 1 where that is not a normal number --, the thread's 16
// bytes e4m3_rne(clamp(float(x) / s, -448, 448)) as one 16-byte store, and s itself by the group's first thread.  Group 4 copies
// the RoPE values, 16 bytes per thread.  A row outside [0, Scache), or whose table entry is outside the pool, is dropped; the
// lanes of a group share the row, so they take every branch together.
template <typename TAG, typename T>
__global__ __launch_bounds__(256) void fa_kvcache_append_paged_kernel(Fp8RowParams p) {
  static_assert(std::is_same<TAG, Fp8Row>::value, "the FP8 latent cache overload");
  constexpr int ipr = 40;
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)p.B * p.Snew * ipr) return;
  const int c = (int)(item % ipr);
  const long long rowi = item / ipr;   // b * S_new + j
  const int j = (int)(rowi % p.Snew), b = (int)(rowi / p.Snew);
  const int dst = p.seqlens[b] + j;
  if (dst < 0 || dst >= p.Scache) return;
  const int pi = dst / p.page_size;
  const int page = p.table[(long long)b * p.bt_stride + pi];
  if ((unsigned)page >= (unsigned)p.num_pages) return;
  char* row = (char*)p.kv + page * p.kv_ps + (long long)(dst - pi * p.page_size) * p.kv_rs;
  const char* src = (const char*)p.kv_new + rowi * kMlaRowB;
  const int blk = c >> 3, u = c & 7;
  if (blk == 4) {
    *(u32x4*)(row + kFp8RowRopeOff + 16 * u) = *(const u32x4*)(src + 2 * kMlaDv + 16 * u);
    return;
  }
  const u32x4 x0 = *(const u32x4*)(src + 256 * blk + 32 * u), x1 = *(const u32x4*)(src + 256 * blk + 32 * u + 16);
  float a = fmaxf(amax8<T>(x0), amax8<T>(x1));
  for (int o = 1; o < 8; o <<= 1) a = fmaxf(a, __shfl_xor(a, o));
  const float d = block_scale_fp8(a);
  *(u32x4*)(row + 128 * blk + 16 * u) =
      u32x4{quant4_fp8<T>(x0[0], x0[1], d), quant4_fp8<T>(x0[2], x0[3], d), quant4_fp8<T>(x1[0], x1[1], d), quant4_fp8<T>(x1[2], x1[3], d)};
  if (u == 0) *(float*)(row + kFp8RowScaleOff + 4 * blk) = d;
}

// The combine at the latent width: fa_decode_combine.inc's arithmetic -- the n partials of a row merged in ascending split
// order, one row (b, h, i) per 128 threads -- over this call's parameter block.  (An overload by tag, not a second <512, T>
// instance of the shared kernel: those two are a recorded set.)
template <typename TAG, typename T>
__global__ __launch_bounds__(256) void fa_decode_combine_kernel(Fp8RowParams p) {
  static_assert(std::is_same<TAG, Fp8Row>::value, "the FP8 latent cache overload");
  constexpr int D = kMlaDv, TPR = D / 4, RPB = 256 / TPR;
  const long long R = (long long)p.B * p.H * p.Sq;
  const long long ridx = (long long)blockIdx.x * RPB + threadIdx.x / TPR;
  if (ridx >= R) return;
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
  const int i = (int)(ridx % p.Sq), head = (int)((ridx / p.Sq) % p.H), b = (int)(ridx / ((long long)p.Sq * p.H));
  const float inv = ls > 0.f ? 1.f / ls : 0.f;
  typedef __attribute__((ext_vector_type(4))) typename T::elem e4;
  e4 ov;
#pragma unroll
  for (int j = 0; j < 4; ++j) ov[j] = (typename T::elem)(acc[j] * inv);
  *(u32x2*)((char*)p.o + b * p.lo.sb + (long long)head * p.lo.sh + (long long)i * p.lo.rs + d4 * 2) = __builtin_bit_cast(u32x2, ov);
  if (d4 == 0 && p.lse) p.lse[ridx] = ls > 0.f ? (mx + __builtin_log2f(ls)) * kLn2 : -INFINITY;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
template <typename T>
static hipError_t launch_append_t(const Fp8RowParams& p, hipStream_t s) {
  if (p.Snew <= 0) return hipSuccess;
  const long long items = (long long)p.B * p.Snew * 40;
  hipLaunchKernelGGL((fa_kvcache_append_paged_kernel<Fp8Row, T>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, p);
  return hipGetLastError();
}

template <typename T>
static hipError_t launch_combine_t(const Fp8RowParams& p, hipStream_t s) {
  const long long rows = (long long)p.B * p.H * p.Sq, rpb = 256 / (kMlaDv / 4);
  hipLaunchKernelGGL((fa_decode_combine_kernel<Fp8Row, T>), dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(256), 0, s, p);
  return hipGetLastError();
}

template <typename T>
static hipError_t launch_attention_t(const Fp8RowParams& p, hipStream_t s) {
  const long long wgs = (long long)p.B * decode_row_blocks(p.H, p.Sq);
  return launch_kernel<fa_decode_paged_kernel<Fp8Row, T>>((unsigned)(wgs * p.nsplit), 256, Fp8RowCfg::LDS_BYTES, s, p);
}

hipError_t launch_mla_fp8_append(const Fp8RowParams& p, int dtype, hipStream_t s) {
  return dtype == 1 ? launch_append_t<BF16>(p, s) : launch_append_t<FP16>(p, s);
}

hipError_t launch_mla_fp8_combine(const Fp8RowParams& p, int dtype, hipStream_t s) {
  return dtype == 1 ? launch_combine_t<BF16>(p, s) : launch_combine_t<FP16>(p, s);
}

hipError_t launch_decode_mla_fp8(const Fp8RowParams& p, int dtype, hipStream_t s) {
  if (hipError_t e = launch_mla_fp8_append(p, dtype, s)) return e;
  if (hipError_t e = dtype == 1 ? launch_attention_t<BF16>(p, s) : launch_attention_t<FP16>(p, s)) return e;
  return p.nsplit <= 1 ? hipSuccess : launch_mla_fp8_combine(p, dtype, s);
}

}  // namespace fa
