// Sparse (top-k indexed) MLA decoding over the paged latent cache: include_mla_sparse/mi355fa_kvcache_mla_sparse.h.
//
// DeepSeek-V3.2 and its successors run an indexer in front of attention: per query token it picks topk cached tokens, the same
// for all H heads of that token, and attention runs over those alone.  The list of query (b, i) holds LOGICAL positions of
// sequence b; the key of position idx is row idx % page_size of page table[b][idx / page_size] of the pool fa_decode_mla.hip
// reads densely.
//
//   fa_kvcache_append_paged_kernel<MLA, T>  fa_decode_mla.hip's, launched from the dense block  (first, same stream)
//   fa_decode_paged_kernel<Topk, T>         one workgroup per (sequence, query token, block of 32 heads, split of the list)
//   fa_decode_combine_kernel<512, T>        nsplit > 1: fa_decode_mla.hip's instance of the shared combine kernel
// (an overload of the decode kernels' name by its template parameters: the Topk tag is a type, which no other overload takes
// first.)
//
// Work item.  The dense kernel's 32 MFMA rows are (query, head) rows that may span several query tokens; here every query token
// has a key list of its own, so the 32 rows are 32 HEADS OF ONE QUERY TOKEN and a workgroup follows one list.  Rows at or past H
// are zero queries that store nothing.  A split is a range of 32-entry tiles of the list; entries of the last tile at or past
// topk are skipped like bad indices.
//
// Wave split, exchange, softmax, O^T += V^T P^T, merge and epilogue are fa_decode_mla_body.inc's, written out here (that text
// addresses keys by tile and rows by (query, head); shared pieces would have to be cut out of it, and the dense kernels are held
// to their instructions): four waves on the same 32 keys, wave w on latent columns [128 w, 128 w + 128) and RoPE columns
// [512 + 16 w, + 16), K = V loaded once and written to the wave's swizzled LDS tile, the four partial scores through two slots
// by step parity behind one barrier per step, added as (p0 + p1) + (p2 + p3) in every wave.
//
// The gather pipeline.  Lane (r, h) owns entry 32 t + r of tile t (both halves h resolve the same entry; each loads its own 16
// bytes of every piece).  Three dependent stages per tile and lane:
//   index    one 4-byte load of the entry (-1 at or past topk or the split's end)
//   entry    the bounds and mask decision 0 <= idx < lim -- lim = L_b, or min(L_b, position + 1) under causal --, and for a visible
//            index the 4-byte table entry at idx / page_size (FastDiv); idx < L_b <= max_pages * page_size keeps that load inside
//            the table's row
//   rows     the entry checked against num_pages, the 64-bit address pool + page * page_stride + (idx % page_size) * row_stride,
//            and the nine 16-byte pieces by per-lane global loads: the pool may exceed 2^32 bytes and the 32 keys of a tile share
//            no descriptor.  A skipped lane issues no load at all and its key registers are zero: neither 0 * NaN nor a stray
//            read can occur, and its score is -inf.
// At the top of step t the rows of tile t are in flight, the table entries of tile t + 1 are in flight or back, and so are the
// indices of tile t + 2; step t issues rows(t + 1), entries(t + 2), indices(t + 3) in that order, so each stage has a whole step
// of MFMA and softmax work to land in -- the dense kernel's descriptor one tile ahead and table entry two ahead, per lane.
// The visible lanes of a tile are a 32-bit ballot that travels with its rows: it masks the scores, and a tile with none is
// passed over without its LDS writes, MFMAs and barrier.  That decision is workgroup-uniform: the four waves load the same
// indices and the same table entries, so they hold the same ballot, and every wave joins every barrier that is taken.  The
// exchange slots alternate by the count of steps taken, not by t, so the ordering argument of the dense kernel carries over.
//
// No access leaves the pool or the table's row whatever indices, block_table or cache_seqlens hold.  Every order of summation is
// fixed -- list order within a split, ascending splits in the combine --, so the result is deterministic.
// LDS: as the dense kernel, 32 KiB of V tiles + 32 KiB of exchange slots in the loop, the 64.5 KiB merge stage over them:
// 64.75 KiB, two workgroups per CU.
#include <algorithm>

#include "fa_common.h"
#include "fa_decode_mla_sparse.h"

namespace fa {

namespace {

constexpr int kTile = 32;    // list entries per step
constexpr int kRows = 32;    // MFMA rows per workgroup: heads of one query token
constexpr int kWaves = 4;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;

struct TopkCfg {
  static constexpr int HD = kMlaDv / kWaves;             // the latent columns of one wave
  static constexpr int RD = (kMlaD - kMlaDv) / kWaves;   // its RoPE columns: one k-step
  static constexpr int KS = HD / 16;                     // latent k-steps of S^T = K Q^T
  static constexpr int DB = HD / 32;                     // 32-column blocks of the wave's O^T
  static constexpr int ROWB = HD * 2;                    // a row of the wave's V tile
  static constexpr int VT_BYTES = kWaves * kTile * ROWB;
  static constexpr int XCH_OFF = VT_BYTES;               // behind the V tiles
  static constexpr int XCH_SLOT = 64 * 16 * 4;           // one wave's 32 x 32 fp32 partial scores
  static constexpr int LOOP_BYTES = XCH_OFF + 2 * kWaves * XCH_SLOT;
  static constexpr int OST = kMlaDv + 4;                 // fp32 row stride of the merge stage (bank spread)
  static constexpr int MERGE_BYTES = kRows * OST * 4;
  static constexpr int ML_OFF = MERGE_BYTES;
  static constexpr int LDS_BYTES = (LOOP_BYTES > MERGE_BYTES ? LOOP_BYTES : MERGE_BYTES) + 2 * kRows * 4;
  static_assert(RD == 16, "the RoPE slice of a wave is one MFMA k-step");
  static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU");
};

}  // namespace

template <typename TAG, typename T>
__global__ __launch_bounds__(256, 2) void fa_decode_paged_kernel(TopkParams tp) {
  static_assert(std::is_same<TAG, Topk>::value, "the sparse overload");
  using C = TopkCfg;
  using vec8 = typename T::vec8;
  const MlaParams& p = tp.m;
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
  const int nt = (tp.topk + kTile - 1) / kTile;
  const int s_beg = (int)((long long)nt * split / p.nsplit);
  const int s_end = (int)((long long)nt * (split + 1) / p.nsplit);

  // ---- this lane's query row = head r0 + r of query i: the Q^T fragments (B operand) of the wave's columns ----
  const int r0 = hb * kRows, head = r0 + r;
  vec8 qf[C::KS + 1];
  {
    const bool valid = head < p.H;
    const char* qp = (const char*)p.q + b * p.lq.sb + (long long)head * p.lq.sh + (long long)qi * p.lq.rs + 16 * h;
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks)
      qf[ks] = as_vec8<T>(valid ? *(const u32x4*)(qp + 2 * C::HD * wave + 32 * ks) : u32x4{0u, 0u, 0u, 0u});
    qf[C::KS] = as_vec8<T>(valid ? *(const u32x4*)(qp + 2 * kMlaDv + 2 * C::RD * wave) : u32x4{0u, 0u, 0u, 0u});
  }

  FA_LDS char* vt = smem + wave * kTile * C::ROWB;
  int v_off[2][C::DB];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int db = 0; db < C::DB; ++db) v_off[e][db] = tr_lane_off<C::HD>(lane, 8 * e, db);

  // ---- the gather pipeline (the file's head says what each stage may touch) ----
  const int* ind = tp.indices + b * tp.idx_sb + qi * tp.idx_ss;
  const int* table = p.table + (long long)b * p.bt_stride;
  // entry 32 t + r of the list; -1 past the list or the split
  auto load_index = [&](int t) __attribute__((always_inline)) {
    const int e = t * kTile + r;
    return (t < s_end && e < tp.topk) ? ind[e] : -1;
  };
  // the table entry of a visible index; -1 (no page) for a skipped one, which loads nothing
  auto load_entry = [&](int idx) __attribute__((always_inline)) {
    return (unsigned)idx < (unsigned)lim ? table[tp.pdiv.div(idx)] : -1;
  };
  // key idx's pieces out of page pg: the latent quarter's 16 bytes at d = 128 w + 16 ks + 8 h, the RoPE slice's at
  // d = 512 + 16 w + 8 h; zeros for a skipped lane.  Returns the tile's visible lanes, bit r (both halves agree).
  u32x4 kr[C::KS + 1];
  auto load_rows = [&](int idx, int pg) __attribute__((always_inline)) {
    const bool ok = (unsigned)idx < (unsigned)lim && (unsigned)pg < (unsigned)p.num_pages;
    if (ok) {
      const int pi = tp.pdiv.div(idx);
      const char* row = (const char*)p.kv + pg * p.kv_ps + (long long)(idx - pi * p.page_size) * p.kv_rs + 16 * h;
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) kr[ks] = *(const u32x4*)(row + 2 * C::HD * wave + 32 * ks);
      kr[C::KS] = *(const u32x4*)(row + 2 * kMlaDv + 2 * C::RD * wave);
    } else {
#pragma unroll
      for (int ks = 0; ks <= C::KS; ++ks) kr[ks] = u32x4{0u, 0u, 0u, 0u};
    }
    return (unsigned)__builtin_amdgcn_ballot_w64(ok);
  };

  const float c2 = p.scale * kLog2e;   // scores in log2 units
  float m = -INFINITY, l = 0.f;
  f32x16 oacc[C::DB];
#pragma unroll
  for (int db = 0; db < C::DB; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[db][i] = 0.f;

  // At the top of step t: kr / vis = the rows of tile t (in flight) and its visible lanes, (idx1, pg1) the indices of tile
  // t + 1 and their table entries (in flight), idx2 the indices of tile t + 2 (in flight).
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
    u32x4 kc[C::KS + 1];
#pragma unroll
    for (int ks = 0; ks <= C::KS; ++ks) kc[ks] = kr[ks];
    // the three stages, one tile further each, in flight while this tile is computed
    vis = load_rows(idx1, pg1);
    pg1 = load_entry(idx2);
    idx1 = idx2;
    idx2 = load_index(t + 3);
    // Nothing visible in this tile: pass it over.  `live` is the same in all four waves (the same indices, the same table
    // entries), so they skip the same steps and every wave joins every barrier below.
    if (live == 0u) continue;

    // V of tile t = the latent pieces of K, into the wave's LDS tile (the previous tile's transposed reads precede these
    // writes in LDS order)
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) lds_write16(vt + lds_off<C::HD>(r, 2 * ks + h), kc[ks]);

    // ---- the wave's partial S^T = K Q^T over its columns: reg i of lane (r, h) = head r0 + r, entry t*32 + (i&3) + 8(i>>2) + 4h
    f32x16 s;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks <= C::KS; ++ks) s = T::mfma(as_vec8<T>(kc[ks]), qf[ks], s);
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
  // them), then O / LSE or the split's partial, rows (b, head, i) in the dense call's layout ----
  __syncthreads();   // every wave is done with its V tile and the exchange slots: the LDS is the merge stage now
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
// Split count: mla_splits (fa_decode_mla.hip) with the list in the place of the cache -- up to two workgroups per CU over
// (sequence, query token, head block, split), splits of at least sqrt(16 * topk) entries, at most 64.  DESIGN.md has the
// forced-split sweep (profiles/mla_sparse_split_sweep.jsonl) and how far the rule lies from the best swept count.
int mla_sparse_splits(long long wgs, int topk, int forced) { return mla_splits(wgs, topk, forced); }

template <typename T>
static hipError_t launch_sparse_t(const TopkParams& p, hipStream_t s) {
  const long long wgs = (long long)p.m.B * p.m.Sq * ((p.m.H + kRows - 1) / kRows);
  return launch_kernel<fa_decode_paged_kernel<Topk, T>>((unsigned)(wgs * p.m.nsplit), 256, TopkCfg::LDS_BYTES, s, p);
}

hipError_t launch_decode_mla_sparse(const TopkParams& p, int dtype, hipStream_t s) {
  if (hipError_t e = launch_mla_append(p.m, dtype, s)) return e;
  if (hipError_t e = dtype == 1 ? launch_sparse_t<BF16>(p, s) : launch_sparse_t<FP16>(p, s)) return e;
  return p.m.nsplit <= 1 ? hipSuccess : launch_mla_combine(p.m, dtype, s);
}

}  // namespace fa
