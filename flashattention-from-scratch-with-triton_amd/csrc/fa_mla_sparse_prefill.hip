// Sparse (top-k indexed) MLA prefill over one contiguous latent array: include_mla_sparse_prefill/mi355fa_mla_sparse_prefill.h.
//
// The prefill step of DeepSeek-V3.2: the indexer (fa_mla_indexer_prefill.hip, fa_mla_select.hip) leaves per packed query token a
// list of rows of the step's packed key array, the same for all H heads of that token, and attention runs over those rows alone.
// No pages, no table, no lengths: entry idx of a list is row idx of kv, visible iff 0 <= idx < N.
//
//   fa_decode_paged_kernel<RowList, T>      one workgroup per (query token, block of 32 heads), one list from start to end
// (an overload of the decode kernels' name by its template parameters and its parameter block.)  No split, no workspace, no
// combine: the epilogue writes O and LSE.
//
// Placement.  Workgroup id = 8 j + x is head block j % HB of token 8 (j / HB) + x, HB = ceil(H / 32): the HB head blocks of a
// token have ids 8 apart, adjacent in launch order.  If ids go round-robin over the 8 XCDs -- a supposition about the
// dispatcher --, the HB gathers of a token's rows run on one XCD at about the same time and the later ones hit its L2.  The grid
// is rounded up to whole groups of 8 tokens; an item whose token is at or past M exits before it touches memory or a barrier.
//
// Kept from fa_decode_mla_sparse.hip: 256 lanes, four waves on the same 32 list entries, wave w on latent columns
// [128 w, 128 w + 128) and RoPE columns [512 + 16 w, + 16); the 32 MFMA columns are 32 heads of the token (rows at or past H are
// zero queries that store nothing); K goes from the gather registers straight into the A operand of S^T = K Q^T, the latent
// pieces (V) through the wave's private swizzled LDS tile, O^T += V^T P^T.
//
// The gather, two stages per tile and lane.  Lane (r, h) owns entry 32 t + r of tile t (both halves h resolve the same entry;
// each loads its own 16 bytes of every piece).
//   index    one 4-byte load of the entry (-1 at or past topk)
//   rows     0 <= idx < N decided, the 64-bit address kv + idx * row_stride, nine 16-byte pieces by per-lane global loads.  A
//            skipped lane issues no load at all and its key registers are zero: neither 0 * NaN nor a stray read can occur.
// At the top of step t the rows of tile t and the indices of tile t + 1 are in flight; step t issues rows(t + 1), then
// indices(t + 2).  The visible lanes of a tile are a 32-bit ballot that travels with its rows: it masks the scores, and a tile
// with none is passed over without LDS writes, MFMAs or barriers.  That decision is workgroup-uniform -- the four waves load the
// same indices --, so every wave joins every barrier that is taken.
//
// Softmax once per row.  The decode kernel lets every wave add the four partial scores and redo the whole 32 x 32 softmax: free
// when bytes bound the call, four times the exp2 and VALU work when they do not.  Here wave w OWNS heads [8 w, 8 w + 8) of the
// block.  Per step:
//   W1  every wave writes its 32 x 32 fp32 partial, grouped by owner: the 1 KiB of owner o holds lane-ordered f32x4 pieces
//   B1  barrier
//   R1  owner w reads its 1 KiB of each of the four partials (one f32x4 per lane and partial) and adds them as
//       (p0 + p1) + (p2 + p3); lane L holds head 8 w + (L & 7), entries 8 (L >> 4) + 4 ((L >> 3) & 1) + {0..3}.  Mask, tile
//       maximum over the head's 8 lanes (lane ^ 8, ^ 16, ^ 32), running m, exp2, per-lane running l: for its 8 heads alone.
//   W2  the owner writes the 16-bit P of its heads into the shared 2 KiB P^T tile, in the B-operand order of the O MFMAs
//       (head r at 64 r, half h at + 32 h), and its 8 rescale factors
//   B2  barrier
//   R2  every wave reads its lanes' two B fragments of P^T and the rescale factor of its lanes' head
// then O^T += V^T P^T from registers and the wave's own V tile.  m and l of a head live in its owner alone; the epilogue takes
// l from there through LDS and writes LSE from the owner's registers.
//
// Ordering, and why no buffer is doubled.  Every barrier is preceded by s_waitcnt lgkmcnt(0): a wave arrives only when its LDS
// writes have landed and its LDS reads have returned.  The partials: W1 of step k + 1 follows B2 of step k in program order,
// and every wave joins B2(k) after its R1(k) returned, so no partial is overwritten before it is read.  The P^T tile and the
// factors: W2(k + 1) follows B1(k + 1), which every wave joins after its R2(k) returned.  Two barriers per step thus order both
// exchanges with single buffers; slots by step parity would save neither barrier.  The V tile is private to its wave.
//
// Rescale.  O is multiplied only when some factor among the wave's 32 heads differs from 1 -- a wave-uniform branch on a
// ballot, with no barrier inside.
//
// No access leaves q, kv, indices, o or lse whatever the lists hold.  Every order of summation is fixed -- list order within
// a row --, so the result is deterministic.
// LDS: 32 KiB of V tiles + 16 KiB of partials + 2 KiB P^T + 256 B of factors and row sums: 50.25 KiB, two workgroups per CU
// (the register budget allows no third).
#include <algorithm>

#include "fa_common.h"
#include "fa_decode_mla.h"
#include "fa_mla_sparse_prefill.h"

namespace fa {

namespace {

constexpr int kWaves = 4;

struct RowListCfg {
  static constexpr int HD = kMlaDv / kWaves;             // the latent columns of one wave
  static constexpr int RD = (kMlaD - kMlaDv) / kWaves;   // its RoPE columns: one k-step
  static constexpr int KS = HD / 16;                     // latent k-steps of S^T = K Q^T
  static constexpr int DB = HD / 32;                     // 32-column blocks of the wave's O^T
  static constexpr int ROWB = HD * 2;                    // a row of the wave's V tile
  static constexpr int VT_BYTES = kWaves * kRowListTile * ROWB;
  static constexpr int XCH_OFF = VT_BYTES;               // behind the V tiles: the four partials
  static constexpr int XCH_SLOT = 64 * 16 * 4;           // one wave's 32 x 32 fp32 partial scores
  static constexpr int OWN_BYTES = XCH_SLOT / kWaves;    // ... of which one owner reads this much
  static constexpr int PT_OFF = XCH_OFF + kWaves * XCH_SLOT;
  static constexpr int PT_BYTES = kRowListHeads * kRowListTile * 2;   // the 16-bit P^T of a step
  static constexpr int SCL_OFF = PT_OFF + PT_BYTES;      // the 32 rescale factors of a step
  static constexpr int SL_OFF = SCL_OFF + kRowListHeads * 4;   // the 32 row sums of the epilogue
  static constexpr int LDS_BYTES = SL_OFF + kRowListHeads * 4;
  static_assert(RD == 16, "the RoPE slice of a wave is one MFMA k-step");
  static_assert(kRowListHeads == 8 * kWaves && kRowListTile == 32, "an owner wave holds 8 heads x 32 entries, four values per lane");
  static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU");
};

// lane ^ 8 (DPP row_ror:8 within a row of 16) and lane ^ 16 (ds_swizzle bit mode: and 0x1f, xor 0x10); lane ^ 32 is
// fa_common.h's swap_halves
FA_DEVINL float lane_xor8(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, true));
}
FA_DEVINL float lane_xor16(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F)); }

}  // namespace

template <typename TAG, typename T>
__global__ __launch_bounds__(256, 2) void fa_decode_paged_kernel(RowListParams p) {
  static_assert(std::is_same<TAG, RowList>::value, "the sparse prefill overload");
  using C = RowListCfg;
  using vec8 = typename T::vec8;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  FA_LDS char* smem = (FA_LDS char*)smem_raw;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- work item: id = 8 j + x -> head block j % HB of token 8 (j / HB) + x (the file's head: placement) ----
  const int HB = (p.H + kRowListHeads - 1) / kRowListHeads;
  const int id = blockIdx.x, j = id >> 3;
  const int hb = j % HB, tok = 8 * (j / HB) + (id & 7);
  if (tok >= p.M) return;   // the rounded-up grid: the whole workgroup leaves, before any access or barrier

  // ---- this lane's query row = head r0 + r of the token: the Q^T fragments (B operand) of the wave's columns ----
  const int r0 = hb * kRowListHeads, head = r0 + r;
  vec8 qf[C::KS + 1];
  {
    const bool valid = head < p.H;
    const char* qp = (const char*)p.q + (long long)tok * p.q_sm + (long long)head * p.q_sh + 16 * h;
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks)
      qf[ks] = as_vec8<T>(valid ? *(const u32x4*)(qp + 2 * C::HD * wave + 32 * ks) : u32x4{0u, 0u, 0u, 0u});
    qf[C::KS] = as_vec8<T>(valid ? *(const u32x4*)(qp + 2 * kMlaDv + 2 * C::RD * wave) : u32x4{0u, 0u, 0u, 0u});
  }

  FA_LDS char* vt = smem + wave * kRowListTile * C::ROWB;
  int v_off[2][C::DB];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int db = 0; db < C::DB; ++db) v_off[e][db] = tr_lane_off<C::HD>(lane, 8 * e, db);

  // ---- the gather pipeline (the file's head says what each stage may touch) ----
  const int* ind = p.indices + (long long)tok * p.idx_rs;
  const int nt = (p.topk + kRowListTile - 1) / kRowListTile;
  // entry 32 t + r of the list; -1 past the list
  auto load_index = [&](int t) __attribute__((always_inline)) {
    const int e = t * kRowListTile + r;
    return e < p.topk ? ind[e] : -1;
  };
  // row idx's pieces: the latent quarter's 16 bytes at d = 128 w + 16 ks + 8 h, the RoPE slice's at d = 512 + 16 w + 8 h; zeros
  // for a skipped lane.  Returns the tile's visible lanes, bit r (both halves agree).
  u32x4 kr[C::KS + 1];
  auto load_rows = [&](int idx) __attribute__((always_inline)) {
    const bool ok = (unsigned)idx < (unsigned)p.N;
    if (ok) {
      const char* row = (const char*)p.kv + (long long)idx * p.kv_rs + 16 * h;
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
  // the softmax owner's view of this lane: head 8 wave + hl of the block, entries eb + {0..3} of a tile
  const int hl = lane & 7, eb = 8 * (lane >> 4) + 4 * ((lane >> 3) & 1);
  float m = -INFINITY, l = 0.f;        // of head 8 wave + hl; l is this lane's share of the row sum
  f32x16 oacc[C::DB];
#pragma unroll
  for (int db = 0; db < C::DB; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[db][i] = 0.f;

  FA_LDS char* xch = smem + C::XCH_OFF;
  FA_LDS char* w1 = xch + wave * C::XCH_SLOT + (r >> 3) * C::OWN_BYTES + ((r & 7) + 8 * h) * 16;   // + 256 c: piece c, to owner r >> 3
  const FA_LDS char* r1 = xch + wave * C::OWN_BYTES + lane * 16;                                    // + XCH_SLOT v: partial v
  // entries eb + {0..3} of the owner's head in B-operand order: value i of half h of a head is entry (i & 3) + 8 (i >> 2) + 4 h
  FA_LDS char* w2 = smem + C::PT_OFF + (8 * wave + hl) * 64 + ((lane >> 3) & 1) * 32 + (lane >> 4) * 8;
  const FA_LDS char* r2 = smem + C::PT_OFF + r * 64 + h * 32;
  FA_LDS float* scl = (FA_LDS float*)(smem + C::SCL_OFF);
  auto xch_sync = [&]() __attribute__((always_inline)) {   // this wave's LDS writes have landed and its reads returned
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(waitcnt_imm(kNoWait, 0));
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  // At the top of step t: kr / vis = the rows of tile t (in flight) and its visible lanes, idx1 the indices of tile t + 1 (in
  // flight).
  unsigned vis = load_rows(load_index(0));
  int idx1 = load_index(1);
  for (int t = 0; t < nt; ++t) {
    const unsigned live = vis;
    u32x4 kc[C::KS + 1];
#pragma unroll
    for (int ks = 0; ks <= C::KS; ++ks) kc[ks] = kr[ks];
    // the two stages, one tile further each, in flight while this tile is computed
    vis = load_rows(idx1);
    idx1 = load_index(t + 2);
    // Nothing visible in this tile: pass it over.  `live` is the same in all four waves (the same indices), so they skip the
    // same steps and every wave joins every barrier below.
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

    // ---- W1 / B1 / R1: the partials to their owners, added in one fixed association ----
#pragma unroll
    for (int c = 0; c < 4; ++c) *(FA_LDS f32x4*)(w1 + 256 * c) = f32x4{s[4 * c], s[4 * c + 1], s[4 * c + 2], s[4 * c + 3]};
    xch_sync();
    f32x4 pw[kWaves];
#pragma unroll
    for (int v = 0; v < kWaves; ++v) pw[v] = *(const FA_LDS f32x4*)(r1 + v * C::XCH_SLOT);
    // the mask: entry eb + i of the tile is visible iff its lane loaded its rows
    const unsigned lv = live >> eb;
    float sv[4], tm = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float x = (pw[0][i] + pw[1][i]) + (pw[2][i] + pw[3][i]);
      sv[i] = ((lv >> i) & 1u) == 0u ? -INFINITY : x * c2;
      tm = __builtin_fmaxf(tm, sv[i]);
    }
    tm = __builtin_fmaxf(tm, lane_xor8(tm));
    tm = __builtin_fmaxf(tm, lane_xor16(tm));
    tm = half_max(tm);
    // ---- online softmax of the owner's heads; a row that has seen no visible key keeps m = -inf (offset 0: p = 0, not NaN) ----
    const float mn = __builtin_fmaxf(m, tm);
    const float mu = mn == -INFINITY ? 0.f : mn;
    const float corr = __builtin_amdgcn_exp2f(m - mu);
    m = mn;
#pragma unroll
    for (int i = 0; i < 4; ++i) sv[i] = __builtin_amdgcn_exp2f(sv[i] - mu);
    l = l * corr + ((sv[0] + sv[1]) + (sv[2] + sv[3]));
    // ---- W2 / B2 / R2: P^T and the rescale factors to every wave ----
    *(FA_LDS u32x2*)w2 = u32x2{pack2<T>(sv[0], sv[1]), pack2<T>(sv[2], sv[3])};
    if (lane < 8) scl[8 * wave + lane] = corr;
    xch_sync();
    const vec8 pf0 = as_vec8<T>(*(const FA_LDS u32x4*)r2), pf1 = as_vec8<T>(*(const FA_LDS u32x4*)(r2 + 16));
    const float f = scl[r];
    // O is rescaled only when a factor among this wave's heads moved: wave-uniform, no barrier inside
    if (__builtin_amdgcn_ballot_w64(f != 1.f) != 0ull) {
#pragma unroll
      for (int db = 0; db < C::DB; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[db][i] *= f;
    }
    // ---- O^T += V^T P^T on the wave's latent columns ----
    __builtin_amdgcn_s_waitcnt(waitcnt_imm(kNoWait, 0));   // this wave's V writes have landed
#pragma unroll
    for (int db = 0; db < C::DB; ++db) {
      const vec8 a0 = lds_read_tr_frag<T>(vt + v_off[0][db], vt + v_off[1][db]);
      oacc[db] = T::mfma(a0, pf0, oacc[db]);
      const vec8 a1 = lds_read_tr_frag<T>(vt + 16 * C::ROWB + v_off[0][db], vt + 16 * C::ROWB + v_off[1][db]);
      oacc[db] = T::mfma(a1, pf1, oacc[db]);
    }
  }

  // ---- epilogue: the owner's row sums over the head's 8 lanes in one fixed association, LSE from the owner's registers, the
  // sums through LDS (a region no step touches) to the lanes that hold the head's O^T column ----
  float lt = l + lane_xor8(l);
  lt += lane_xor16(lt);
  lt = half_sum(lt);
  FA_LDS float* sl = (FA_LDS float*)(smem + C::SL_OFF);
  if (lane < 8) {
    sl[8 * wave + lane] = lt;
    const int hd = r0 + 8 * wave + lane;
    if (hd < p.H && p.lse) p.lse[(long long)tok * p.H + hd] = lt > 0.f ? (m + __builtin_log2f(lt)) * kLn2 : -INFINITY;
  }
  __syncthreads();
  if (head >= p.H) return;
  const float lsum = sl[r];
  const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
  // reg 4 c + i of block db = latent column 128 w + 32 db + 8 c + 4 h + i of head r0 + r: 8 bytes a store
  char* op = (char*)p.o + (long long)tok * p.o_sm + (long long)head * p.o_sh + (C::HD * wave + 4 * h) * 2;
#pragma unroll
  for (int db = 0; db < C::DB; ++db)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      *(u32x2*)(op + (32 * db + 8 * c) * 2) = u32x2{pack2<T>(oacc[db][4 * c] * inv, oacc[db][4 * c + 1] * inv),
                                                    pack2<T>(oacc[db][4 * c + 2] * inv, oacc[db][4 * c + 3] * inv)};
}

// ---- host ----------------------------------------------------------------------------------------------------------------
template <typename T>
static hipError_t launch_row_list_t(const RowListParams& p, hipStream_t s) {
  const long long HB = (p.H + kRowListHeads - 1) / kRowListHeads, groups = (p.M + 7) / 8;
  return launch_kernel<fa_decode_paged_kernel<RowList, T>>((unsigned)(8 * HB * groups), 256, RowListCfg::LDS_BYTES, s, p);
}

hipError_t launch_mla_sparse_prefill(const RowListParams& p, int dtype, hipStream_t s) {
  return dtype == 1 ? launch_row_list_t<BF16>(p, s) : launch_row_list_t<FP16>(p, s);
}

}  // namespace fa
