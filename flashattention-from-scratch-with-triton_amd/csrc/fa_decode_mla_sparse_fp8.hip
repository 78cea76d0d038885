// Sparse (top-k indexed) MLA decoding over the paged FP8 latent cache: include_mla_sparse_fp8/mi355fa_kvcache_mla_sparse_fp8.h.
//
// The decode step of DeepSeek-V3.2 as it is released: an indexer picks topk cached tokens per query token, the same for all H
// heads of that token, and attention runs over those alone -- over the 656-byte rows of fa_decode_mla_fp8.hip (512 e4m3 bytes,
// four fp32 scales, one per 128 latent dims, and 64 RoPE values in 16 bits).  The list of query (b, i) holds LOGICAL positions
// of sequence b; the key of position idx is row idx % page_size of page table[b][idx / page_size] of the byte pool.
//
//   fa_kvcache_append_paged_kernel<Fp8Row, T>  fa_decode_mla_fp8.hip's, launched from the dense block  (first, same stream)
//   fa_decode_paged_kernel<GatherF8, T>        one workgroup per (sequence, query token, block of 32 heads, split of the list)
//   fa_decode_combine_kernel<Fp8Row, T>        nsplit > 1: fa_decode_mla_fp8.hip's, from the same block
// (an overload of the decode kernels' name by its template parameters: the GatherF8 tag is a type, which no other overload
// takes first.)
//
// Neither parent can serve a gathered byte row with per-key scales: the dense FP8 kernel addresses keys by tile through one
// wave-uniform page descriptor, the 16-bit sparse kernel gathers 16-bit rows.  This kernel joins them.
//
// Work item and wave split: fa_decode_mla_sparse.hip's.  The 32 MFMA rows are 32 HEADS OF ONE QUERY TOKEN, a workgroup follows
// one list, rows at or past H are zero queries that store nothing, a split is a range of the list's 32-entry tiles.  All four
// waves work on the same 32 entries; wave w owns latent columns [128 w, + 128) -- ONE scale block of the row format, so a wave
// needs one scale per gathered key -- and RoPE columns [512 + 16 w, + 16).
//
// The gather pipeline: fa_decode_mla_sparse.hip's three stages per tile and lane (r, h) for entry 32 t + r,
//   index    one 4-byte load of the entry (-1 at or past topk or the split's end)
//   entry    the decision 0 <= idx < lim -- lim = L_b, or min(L_b, position + 1) under causal --, and for a visible index the
//            4-byte table entry at idx / page_size; idx < L_b <= max_pages * page_size keeps that load inside the table's row
//   rows     the entry checked against num_pages, the 64-bit address pool + page * page_stride + (idx % page_size) * row_stride
//            (both strides in bytes; the pool may exceed 2^32 bytes), and SIX per-lane global loads where the 16-bit gather
//            issues nine: the four 16-byte latent pieces at byte 128 w + 32 j + 16 h, the RoPE slice's 16 bytes at
//            528 + 32 w + 16 h, and the quarter's scale as one dword at 512 + 4 w.  A skipped lane issues no load at all: its
//            bytes are 0 and its scale is 0, so its score is -inf, its p is 0 and p * scale is 0 -- no 0 * NaN, no stray read.
// each a whole step ahead of its consumer: step t issues rows(t + 1), entries(t + 2), indices(t + 3).  The visible lanes of a
// tile are a 32-bit ballot that travels with its rows: it masks the scores, and a tile with none is passed over without LDS
// writes, MFMAs or barrier.  The four waves load the same indices and table entries, so they hold the same ballot and every
// wave joins every barrier that is taken.  The exchange slots alternate by the count of steps TAKEN, not by t.
//
// The byte path: fa_decode_mla_fp8.hip's.  The Q fragments are gathered once with the byte loads' permutation of the
// contraction index (k-step 2 j + e reads columns 32 j + 16 h + 8 e + [0, 8)); the bytes are converted exactly, at scale 1.0, to
// T; eight latent k-steps run on the unscaled values; register i of the partial is multiplied by its key's scale in fp32; the
// RoPE k-step goes on top, unscaled; the four partials cross two slots behind one barrier and are added as (p0 + p1) + (p2 + p3)
// in every wave.  V is the converted, unscaled tile in the wave's swizzled LDS; the wave's own copy of P takes its quarter's
// scales, packed in units of the row's largest weight so far, and the accumulator is kept in those units.
//
// The scale slot.  The 32 scales of a tile cross the wave through its own 128 bytes of LDS: lane r writes key r's (both halves
// the same value), half h reads back the 16 scales of its score registers.  The write sits BEHIND the tile skip, in the taken
// step itself.  That is safe because (1) the slot is wave-private and the skip is wave-uniform: a taken step's write is issued by
// all 64 lanes and covers all 32 entries, so the slot is never half-written; (2) every taken step writes the whole slot before
// its own two reads of it (scores, then P) and LDS serves one wave's requests in order, so a step never reads what an earlier
// step left -- whatever number of skipped tiles lies between, they touch no LDS at all; (3) for the same reason the write of a
// taken step follows the reads of the previous taken step.  A write in front of the skip would be as correct and cost an LDS
// request per dead tile.
//
// No access leaves the pool or the table's row whatever indices, block_table or cache_seqlens hold, and rows at or past L are
// never read.  Every order of summation is fixed -- list order within a split, ascending splits in the combine --, so the
// result is deterministic.
// LDS: 32 KiB of V tiles + 32 KiB of exchange slots + 512 bytes of scales in the loop, the 64.5 KiB merge stage over them:
// 64.75 KiB with the (m, l) rows, two workgroups per CU.
#include <algorithm>

#include "fa_common.h"
#include "fa_decode_mla_sparse.h"
#include "fa_decode_mla_sparse_fp8.h"

namespace fa {

namespace {

constexpr int kTile = 32;    // list entries per step
constexpr int kRows = 32;    // MFMA rows per workgroup: heads of one query token
constexpr int kWaves = 4;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;

struct GatherF8Cfg {
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
// subnormals included, is a normal fp16 and bf16 number.  (fa_decode_mla_fp8.hip's cvt_fp8, static to that unit.)
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

}  // namespace

template <typename TAG, typename T>
__global__ __launch_bounds__(256, 2) void fa_decode_paged_kernel(GatherF8Params gp) {
  static_assert(std::is_same<TAG, GatherF8>::value, "the sparse FP8 overload");
  using C = GatherF8Cfg;
  using vec8 = typename T::vec8;
  const Fp8RowParams& p = gp.f;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  FA_LDS char* smem = (FA_LDS char*)smem_raw;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- work item: (((b * S_q + i) * HB + hb) * nsplit + split ----
  const int HB = (p.H + kRows - 1) / kRows;
  int w = blockIdx.x;
  const int split = w % p.nsplit;
  w /= p.nsplit;
  const int hb = w % HB;
  w /= HB;
  const int qi = w % p.Sq, b = w / p.Sq;
  const int L = min(max(p.seqlens[b] + p.Snew, 0), p.Scache);
  const int pos = L - p.Sq + qi;                                // the query's position
  const int lim = max(p.causal ? min(L, pos + 1) : L, 0);       // an entry is visible iff 0 <= idx < lim
  const int nt = (gp.topk + kTile - 1) / kTile;
  const int s_beg = (int)((long long)nt * split / p.nsplit);
  const int s_end = (int)((long long)nt * (split + 1) / p.nsplit);

  // ---- this lane's query row = head r0 + r of query i: the Q^T fragments (B operand) of the wave's columns in the byte loads'
  // order -- k-step ks = 2 j + e: columns 128 w + 32 j + 16 h + 8 e + [0, 8), what bytes [8 e, 8 e + 8) of the lane's piece j hold
  const int r0 = hb * kRows, head = r0 + r;
  vec8 qf[C::KS + 1];
  {
    const bool valid = head < p.H;
    const char* qp = (const char*)p.q + b * p.lq.sb + (long long)head * p.lq.sh + (long long)qi * p.lq.rs;
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

  // ---- the gather pipeline (the file's head says what each stage may touch) ----
  const int* ind = gp.indices + b * gp.idx_sb + qi * gp.idx_ss;
  const int* table = p.table + (long long)b * p.bt_stride;
  // entry 32 t + r of the list; -1 past the list or the split
  auto load_index = [&](int t) __attribute__((always_inline)) {
    const int e = t * kTile + r;
    return (t < s_end && e < gp.topk) ? ind[e] : -1;
  };
  // the table entry of a visible index; -1 (no page) for a skipped one, which loads nothing
  auto load_entry = [&](int idx) __attribute__((always_inline)) {
    return (unsigned)idx < (unsigned)lim ? table[gp.pdiv.div(idx)] : -1;
  };
  // key idx's pieces out of page pg: latent piece j at byte 128 w + 32 j + 16 h, the RoPE slice's 16 bytes at 528 + 32 w + 16 h,
  // the scale of the quarter at 512 + 4 w; zeros for a skipped lane.  Returns the tile's visible lanes, bit r (both halves agree).
  u32x4 kr[C::KL + 1];
  float ksc = 0.f;
  auto load_rows = [&](int idx, int pg) __attribute__((always_inline)) {
    const bool ok = (unsigned)idx < (unsigned)lim && (unsigned)pg < (unsigned)p.num_pages;
    if (ok) {
      const int pi = gp.pdiv.div(idx);
      const char* row = (const char*)p.kv + pg * p.kv_ps + (long long)(idx - pi * p.page_size) * p.kv_rs;
#pragma unroll
      for (int j = 0; j < C::KL; ++j) kr[j] = *(const u32x4*)(row + C::HD * wave + 32 * j + 16 * h);
      kr[C::KL] = *(const u32x4*)(row + kFp8RowRopeOff + 2 * C::RD * wave + 16 * h);
      ksc = *(const float*)(row + kFp8RowScaleOff + 4 * wave);
    } else {
#pragma unroll
      for (int j = 0; j <= C::KL; ++j) kr[j] = u32x4{0u, 0u, 0u, 0u};
      ksc = 0.f;
    }
    return (unsigned)__builtin_amdgcn_ballot_w64(ok);
  };

  const float c2 = p.scale * kLog2e;   // scores in log2 units
  float m = -INFINITY, l = 0.f;
  float unit = 0.f;   // oacc holds this wave's quarter in units of `unit`: the row's largest weight p * scale so far (below)
  f32x16 oacc[C::DB];
#pragma unroll
  for (int db = 0; db < C::DB; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[db][i] = 0.f;

  // At the top of step t: kr / ksc / vis = the rows of tile t (in flight) and its visible lanes, (idx1, pg1) the indices of
  // tile t + 1 and their table entries (in flight), idx2 the indices of tile t + 2 (in flight).
  int t = s_beg;
  int idx1 = -1, pg1 = -1, idx2 = -1;
  unsigned vis = 0;
  if (t < s_end) {
    const int idx0 = load_index(t);
    idx1 = load_index(t + 1);
    idx2 = load_index(t + 2);
    vis = load_rows(idx0, load_entry(idx0));
    pg1 = load_entry(idx1);
  }
  FA_LDS char* xch = smem + C::XCH_OFF;
  auto xch_sync = [&]() __attribute__((always_inline)) {   // this wave's LDS writes have landed and its reads returned
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(waitcnt_imm(kNoWait, 0));
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  int step = 0;   // steps taken: the parity of the exchange slots
  for (; t < s_end; ++t) {
    const unsigned live = vis;
    const float kscale = ksc;
    u32x4 kc[C::KL + 1];
#pragma unroll
    for (int j = 0; j <= C::KL; ++j) kc[j] = kr[j];
    // the three stages, one tile further each, in flight while this tile is computed
    vis = load_rows(idx1, pg1);
    pg1 = load_entry(idx2);
    idx1 = idx2;
    idx2 = load_index(t + 3);
    // Nothing visible in this tile: pass it over.  `live` is the same in all four waves (the same indices, the same table
    // entries), so they skip the same steps and every wave joins every barrier below.
    if (live == 0u) continue;

    // the tile's scales, behind the skip (the file's head says why that is safe): lane r brings key r's, 0 for a skipped key
    *(FA_LDS float*)(scl + 4 * r) = kscale;

    // ---- the wave's partial S^T = K Q^T over its latent columns, on the unscaled values: reg i of lane (r, h) = head r0 + r,
    // entry t*32 + (i&3) + 8(i>>2) + 4h.  The same values are V of tile t: into the wave's LDS tile at the columns they hold
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
      // The four partials cross the workgroup through two slots per wave, taken by the parity of the steps taken, behind ONE
      // barrier per step: the write of step k + 2 follows the barrier of step k + 1, which every other wave joins only once its
      // reads of step k have returned.  Every wave then adds the same four values in the same association,
      // (p0 + p1) + (p2 + p3) -- the same bits, so the workgroup holds one m, l and P for the four quarters of a row.
      const int par = step & 1;
      ++step;
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
    // the mask: entry (i&3) + 8(i>>2) + 4h of the tile is visible iff its lane loaded its rows
    const unsigned lv = live >> (4 * h);
    float tm = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const bool dead = ((lv >> ((i & 3) + 8 * (i >> 2))) & 1u) == 0u;
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
    // (a skipped entry has p = 0 and scale 0).  The weights w = p * scale are packed to 16 bits in units of the row's largest
    // weight so far, `unit`, and the accumulator is kept in those units (fa_decode_mla_fp8.hip says why): the largest weight
    // packs to exactly 1 and no weight that matters can leave T's normal range.  unit only grows in the current maximum's
    // terms: the accumulator is rescaled by corr * unit_old / unit_new <= 1.
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
  // them), then O / LSE or the split's partial, rows (b, head, i) in the dense call's layout ----
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
  const long long R = (long long)p.B * p.H * p.Sq;   // rows of O / LSE / a split's partials
  for (int it = tid; it < kRows * (kMlaDv / 4); it += 256) {
    const int row = it / (kMlaDv / 4), d4 = (it % (kMlaDv / 4)) * 4;
    const int hd = r0 + row;
    if (hd >= p.H) break;   // rows ascend with `it`
    const float mx = sm[row], lsum = sl[row];
    const f32x4 acc = *(const f32x4*)(stage + row * C::OST + d4);
    const long long ridx = ((long long)b * p.H + hd) * p.Sq + qi;
    if (p.nsplit == 1) {
      const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
      typedef __attribute__((ext_vector_type(4))) typename T::elem e4;
      e4 ov;
#pragma unroll
      for (int j = 0; j < 4; ++j) ov[j] = (typename T::elem)(acc[j] * inv);
      *(u32x2*)((char*)p.o + b * p.lo.sb + (long long)hd * p.lo.sh + (long long)qi * p.lo.rs + d4 * 2) = __builtin_bit_cast(u32x2, ov);
      if (d4 == 0 && p.lse) p.lse[ridx] = lsum > 0.f ? (mx + __builtin_log2f(lsum)) * kLn2 : -INFINITY;
    } else {
      const long long pr = split * R + ridx;
      *(f32x4*)(p.ws + pr * kMlaDv + d4) = acc;
      if (d4 == 0) *(f32x2_t*)(p.ws + (long long)p.nsplit * R * kMlaDv + 2 * pr) = f32x2_t{mx, lsum};
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// The split count is mla_sparse_splits (fa_decode_mla_sparse.hip): the list in the place of the cache.
template <typename T>
static hipError_t launch_gather_f8_t(const GatherF8Params& p, hipStream_t s) {
  const long long wgs = (long long)p.f.B * p.f.Sq * ((p.f.H + kRows - 1) / kRows);
  return launch_kernel<fa_decode_paged_kernel<GatherF8, T>>((unsigned)(wgs * p.f.nsplit), 256, GatherF8Cfg::LDS_BYTES, s, p);
}

hipError_t launch_decode_mla_sparse_fp8(const GatherF8Params& p, int dtype, hipStream_t s) {
  if (hipError_t e = launch_mla_fp8_append(p.f, dtype, s)) return e;
  if (hipError_t e = dtype == 1 ? launch_gather_f8_t<BF16>(p, s) : launch_gather_f8_t<FP16>(p, s)) return e;
  return p.f.nsplit <= 1 ? hipSuccess : launch_mla_fp8_combine(p.f, dtype, s);
}

}  // namespace fa
