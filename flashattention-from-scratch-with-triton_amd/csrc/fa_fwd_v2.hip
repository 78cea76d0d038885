// FlashAttention forward, head dim 64, second-generation schedule for gfx950.
//
// Same maths and rounding points as fa_fwd.hip (reference kernel
// code/_flash_attention_kernel_optimized.py:35-129); what changes is the mapping:
//
//   * workgroup = 4 waves = 256 query rows; every wave owns TWO 32-row query blocks.  Per K/V tile
//     a wave therefore does twice the MFMA work for the same staging / barrier cost, K/V cross
//     the L2 -> LDS path half as often, and the two query blocks give the wave two independent
//     dependency chains: the S^T MFMAs of block 1 run under the softmax VALU of block 0, the
//     P V MFMAs of block 0 under the softmax of block 1.
//   * K/V tiles (64 keys) go HBM/L2 -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds) into a
//     3-deep ring, two tiles ahead: no staging VGPRs, no ds_write pass, and the wait that
//     retires tile t+1 (a counted vmcnt) never has to wait -- the loads are a full tile old.
//     The image swizzle is applied to the per-lane SOURCE address (the DMA destination is
//     wave-linear), reads use the same XOR (fa_common.h, lds_off).
//   * one raw s_barrier per tile (no vmcnt(0) drain: the next tile's DMA stays in flight).
#include <type_traits>

#include "fa_common.h"
#include "fa_kernels.h"
#include "fa_stamps.h"

namespace fa {

constexpr float kDeferLog2V2 = 6.0f;  // see fa_fwd.hip: deferred online-softmax rescale
constexpr float kLazySumMaxV2 = 8192.0f;  // see fa_fwd.hip: largest partial row sum a lazy tile accepts

struct Fwd2Cfg {
  static constexpr int D = 64;
  static constexpr int BM = 256, BN = 64, NT = 256, NW = 4;
  static constexpr int ROWB = D * 2, CPR = D / 8, KS = D / 16, DB = D / 32;
  static constexpr int TILE_BYTES = BN * ROWB;        // 8 KiB per matrix
  static constexpr int RING = 3;
  static constexpr int V_BASE = RING * TILE_BYTES;    // K ring, then V ring
  static constexpr int LDS_BYTES = 2 * RING * TILE_BYTES;  // 48 KiB
  static constexpr int DMA_PER_MAT = TILE_BYTES / (NW * 1024);  // 1-KiB DMA instructions per wave per matrix
};


// vmcnt(n) AND lgkmcnt(0): LDS reads issued on the current tile must have returned before the barrier (fa_common.h tile_sync)
#define FA_WAIT_VMCNT(n) __builtin_amdgcn_s_waitcnt(waitcnt_imm((n), 0))

template <typename T, bool CAUSAL>
__global__ __launch_bounds__(256, 2) void fa_fwd2_kernel(FwdParams p) {
  using C = Fwd2Cfg;
  using vec8 = typename T::vec8;
  constexpr int D = C::D;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  FA_LDS char* smem = (FA_LDS char*)smem_raw;

  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);

  // Work list: non-causal -> one 256-row query tile per workgroup.  Causal -> query tile i costs i+1
  // K/V steps, so each workgroup takes the PAIR (nq-1-i, i): every workgroup then streams nq+1 steps
  // and the grid is perfectly balanced (heavy tile first).
  const TileIndex<CAUSAL> ti = tile_index<CAUSAL>(p, p.nq_tiles);   // (fa_kernels.h)
  const bool paired = CAUSAL && p.pair;
  const int bh = ti.bh, idx = ti.idx;
  const int npass = (paired && idx != p.nq_tiles - 1 - idx) ? 2 : 1;
  for (int pass = 0; pass < npass; ++pass) {
  // lane coordinates re-derived per pass (fa_common.h lane_id_now): nothing lane-dependent stays live across passes
  const int lane = lane_id_now(), tid = wave * 64 + lane, r = lane & 31, h = lane >> 5;
  const int qt = paired ? (pass == 0 ? p.nq_tiles - 1 - idx : idx) : (CAUSAL ? p.nq_tiles - 1 - idx : idx);  // heavy first
  const int q0_wg = qt * C::BM;
  // The wave's two 32-row query blocks.  Causal: blocks w and w + 4 of the workgroup's eight (rows 32w.. and 128 + 32w..),
  // so that every wave has one early and one late diagonal -- with two adjacent blocks (rows 64w..) wave 0 is done three
  // tiles before wave 3 and each of the last four steps of a pass waits for one wave's two-block diagonal tile.
  // Non-causal: the mapping is irrelevant (every block sees every key); adjacent blocks keep the O stores contiguous.
  const int qrow0 = q0_wg + (CAUSAL ? 32 * wave : 64 * wave);
  const int qrow1 = qrow0 + (CAUSAL ? 128 : 32);
  auto qrow = [&](int j) __attribute__((always_inline)) { return j == 0 ? qrow0 : qrow1; };
  if (pass) __syncthreads();  // the previous pass staged its O tile in the ring

  // Q, K, V, O may be strided views with a contiguous head dim (fa_fwd.hip): per-tensor batch / head byte strides, one
  // row stride for Q, one shared by K and V, one for O.  (No variable-length launches here: the launcher sends those to
  // family 1.)
  const int b_ = bh / p.H, h_ = bh - b_ * p.H;
  const int q_rs = p.lq.rs, kv_rs = p.lk.rs, o_rs = p.lo.rs;
  const char* qb = (const char*)p.q + b_ * p.lq.sb + h_ * p.lq.sh;
  const char* kb = (const char*)p.k + b_ * p.lk.sb + h_ * p.lk.sh;
  const char* vb = (const char*)p.v + b_ * p.lv.sb + h_ * p.lv.sh;
  char* ob = (char*)p.o + b_ * p.lo.sb + h_ * p.lo.sh;
  const __amdgpu_buffer_rsrc_t rq = make_rsrc(qb, (unsigned)(p.Sq - 1) * q_rs + C::ROWB);
  const __amdgpu_buffer_rsrc_t rk = make_rsrc(kb, (unsigned)(p.Sk - 1) * kv_rs + C::ROWB);
  const __amdgpu_buffer_rsrc_t rv = make_rsrc(vb, (unsigned)(p.Sk - 1) * kv_rs + C::ROWB);
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(ob, (unsigned)(p.Sq - 1) * o_rs + C::ROWB);
  const __amdgpu_buffer_rsrc_t rl = make_rsrc(p.lse + b_ * p.lse_sb + h_ * p.lse_sh, (unsigned)p.Sq * 4);

  // ---- tile schedule (wave-uniform) ----
  const int kv_end = CAUSAL ? min(p.Sk, q0_wg + C::BM) : p.Sk;
  const int ntiles = (kv_end + C::BN - 1) / C::BN;                    // tiles the workgroup streams
  int n_mine = CAUSAL ? min(ntiles, qrow1 / C::BN + 1) : ntiles;      // tiles this wave computes (its later block)
  if (qrow0 >= p.Sq) n_mine = 0;                                      // wave entirely past the last row
  // tiles BOTH blocks see unmasked: the two-block fast path; from there to n_mine each block runs on its own
  const int nfull = min(n_mine, CAUSAL ? min(p.Sk / C::BN, qrow0 / C::BN) : p.Sk / C::BN);

  // A DMA whose source is out of range may leave its LDS bytes untouched; a ragged last tile must
  // not expose uninitialised LDS (0 * NaN in P V), so clear the ring once.  Later rounds only ever
  // leave finite stale K/V there.
  if (p.Sk % C::BN != 0) {
    lds_zero_fill(smem, C::LDS_BYTES, C::NT, tid);
    __syncthreads();
  }

  // ---- LDS-DMA: wave w fills rows [16w, 16w+16) of the K and V tile, 8 rows (1 KiB) per instruction.
  // lane p of instruction i lands on LDS row 16w + 8i + p/8, physical chunk p%8; it must therefore
  // FETCH the logical chunk (p%8) ^ f(row) of that row.  (fa_common.h dma_src_off with shifts in place of its divisions.)
  int dma_src[C::DMA_PER_MAT];
#pragma unroll
  for (int i = 0; i < C::DMA_PER_MAT; ++i) {
    const int row = 16 * wave + 8 * i + (lane >> 3);
    // dma_pieces (fa_common.h): piece i carries the immediate offset 1024*i, which also moves the global address
    dma_src[i] = row * kv_rs + swz_chunk<D>(row, lane & 7) * 16 - 1024 * i;
  }
  auto dma_tile = [&](int t, int buf) __attribute__((always_inline)) {
    const int soff = t * C::BN * kv_rs;
    const int dst0 = buf * C::TILE_BYTES + 16 * wave * C::ROWB;  // this wave's 16 rows = DMA_PER_MAT consecutive KiB
    dma_pieces<C::DMA_PER_MAT>(rk, lds_addr_of(smem + dst0), dma_src, soff);
    dma_pieces<C::DMA_PER_MAT>(rv, lds_addr_of(smem + C::V_BASE + dst0), dma_src, soff);
  };
  constexpr int DMA_PER_TILE = 2 * C::DMA_PER_MAT;  // vmcnt units per tile per wave

  // prologue: tiles 0 and 1 in flight, then the Q fragments
  dma_tile(0, 0);
  if (ntiles > 1) dma_tile(1, 1);

  // ---- Q^T fragments (B operand) of both query blocks, resident ----
  vec8 qf[2][C::KS];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks)
      qf[j][ks] = as_vec8<T>(buf_load16(rq, (qrow(j) + r) * q_rs + (2 * ks + h) * 16));

  int k_off[C::KS];
#pragma unroll
  for (int ks = 0; ks < C::KS; ++ks) k_off[ks] = lds_off<D>(r, 2 * ks + h);
  int v_off[2][C::DB];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int db = 0; db < C::DB; ++db) v_off[e][db] = tr_lane_off<D>(lane, 8 * e, db);

  const float c2 = p.scale * kLog2e;
  // FOLD (bf16, fa_common.h / fa_fwd.hip): Q carries c2, the MFMA delivers scores in log2 units (cs = 1) and a lazy
  // tile's score chains start from -m, so the exponent argument needs no VALU op at all
  constexpr bool FOLD = T::kFoldScale;
  const float cs = FOLD ? 1.0f : c2;  // accumulator units -> log2 units
  if constexpr (FOLD) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) qf[j][ks] = scale_frag<T>(qf[j][ks], c2);
  }
  const float defer_raw = kDeferLog2V2 / cs;
  float m[2] = {-INFINITY, -INFINITY};  // running row max in accumulator units (raw scores, or log2 units if FOLD)
  float l[2] = {0.f, 0.f};
  f32x16 oacc[2][C::DB];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int db = 0; db < C::DB; ++db)
#pragma unroll
      for (int i = 0; i < 16; ++i) oacc[j][db][i] = 0.f;

#ifdef FA_STAMPS
  unsigned long long seg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long last_ = 0, begin_ = 0;
#endif
  using J0 = std::integral_constant<int, 0>;
  using J1 = std::integral_constant<int, 1>;
  // S^T of query block j against the 64 keys of the tile (two 32-key blocks)
  auto scores = [&](const FA_LDS char* kt, auto jt, f32x16 (&s)[2]) __attribute__((always_inline)) {
    constexpr int j = decltype(jt)::value;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
      for (int i = 0; i < 16; ++i) s[b][i] = 0.f;
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        vec8 a = as_vec8<T>(lds_read16(kt + k_off[ks] + b * 32 * C::ROWB));
        s[b] = T::mfma(a, qf[j][ks], s[b]);
      }
    }
  };
  // running max update of block j (deferred rescale); returns nothing, O/l/m updated in place
  auto row_max = [&](auto jt, const f32x16 (&s)[2]) __attribute__((always_inline)) {
    constexpr int j = decltype(jt)::value;
    float t0 = s[0][0], t1 = s[1][0];
#pragma unroll
    for (int i = 1; i < 16; ++i) {
      t0 = __builtin_fmaxf(t0, s[0][i]);
      t1 = __builtin_fmaxf(t1, s[1][i]);
    }
    const float tm = half_max(__builtin_fmaxf(t0, t1));
    if (__builtin_amdgcn_ballot_w64(tm > m[j] + defer_raw) != 0) {
      const float mn = __builtin_fmaxf(m[j], tm);
      const float corr = __builtin_amdgcn_exp2f((m[j] - mn) * cs);
      l[j] *= corr;
#pragma unroll
      for (int db = 0; db < C::DB; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[j][db][i] *= corr;
      m[j] = mn;
    }
  };
  // p = exp2(s*c2 - m*c2), row-sum into l, round to the 16-bit B fragments
  auto probs = [&](auto jt, f32x16 (&s)[2], vec8 (&pf)[2][2]) __attribute__((always_inline)) {
    constexpr int j = decltype(jt)::value;
    const float mc = m[j] * cs;
    float ls[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float pe = __builtin_amdgcn_exp2f(FOLD ? s[b][i] - mc : __builtin_fmaf(s[b][i], c2, -mc));
        s[b][i] = pe;
        ls[i & 3] += pe;
      }
    l[j] += (ls[0] + ls[1]) + (ls[2] + ls[3]);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      pf[b][0] = pack8<T, 0>(s[b]);
      pf[b][1] = pack8<T, 1>(s[b]);
    }
  };
  // O^T[j] += V^T P^T
  auto pv = [&](const FA_LDS char* vt, auto jt, const vec8 (&pf)[2][2], bool use0, bool use1) __attribute__((always_inline)) {
    constexpr int j = decltype(jt)::value;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (!(b == 0 ? use0 : use1)) continue;
      const FA_LDS char* base = vt + b * 32 * C::ROWB;
#pragma unroll
      for (int db = 0; db < C::DB; ++db) {
        vec8 a0 = lds_read_tr_frag<T>(base + v_off[0][db], base + v_off[1][db]);
        oacc[j][db] = T::mfma(a0, pf[b][0], oacc[j][db]);
        vec8 a1 = lds_read_tr_frag<T>(base + 16 * C::ROWB + v_off[0][db], base + 16 * C::ROWB + v_off[1][db]);
        oacc[j][db] = T::mfma(a1, pf[b][1], oacc[j][db]);
      }
    }
  };

  // unmasked tile: every key of the tile visible to all 64 rows of the wave.
  // Both query blocks consume each K / V fragment as soon as it is read (one LDS read, two MFMAs):
  // per tile 8 ds_read_b128 + 16 transposed reads feed 32 MFMAs.  The MFMA phases of this wave run
  // under the softmax phase of the other wave on the SIMD (different workgroup, not barrier-locked).
  auto tile_full = [&](int buf) __attribute__((always_inline)) {
    const FA_LDS char* kt = smem + buf * C::TILE_BYTES;
    const FA_LDS char* vt = smem + C::V_BASE + buf * C::TILE_BYTES;
    f32x16 s0[2], s1[2];
    vec8 p0[2][2], p1[2][2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        s0[b][i] = 0.f;
        s1[b][i] = 0.f;
      }
    // K fragments two reads ahead of their MFMA pair, order pinned: left alone, hipcc issues each
    // ds_read right before its consumers and exposes the LDS latency eight times per tile.
    {
      constexpr int NF = 2 * C::KS;  // fragment f: key block f / KS, k-step f % KS
      vec8 kfr[NF];
      auto kread = [&](int f) __attribute__((always_inline)) {
        kfr[f] = as_vec8<T>(lds_read16(kt + k_off[f % C::KS] + (f / C::KS) * 32 * C::ROWB));
      };
      kread(0);
      kread(1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        if (f + 2 < NF) kread(f + 2);
        s0[f / C::KS] = T::mfma(kfr[f], qf[0][f % C::KS], s0[f / C::KS]);
        s1[f / C::KS] = T::mfma(kfr[f], qf[1][f % C::KS], s1[f / C::KS]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    FA_STAMP(1);  // S^T MFMAs
    row_max(J0{}, s0);
    row_max(J1{}, s1);
    FA_STAMP(2);  // row max (+ rare rescale)
    probs(J0{}, s0, p0);
    probs(J1{}, s1, p1);
    FA_STAMP(3);  // exp / sum / pack
    // V^T fragments: same two-ahead pipeline (fragment f: key block f/4, d block (f/2)%2, k-step f%2)
    {
      constexpr int NF = 2 * C::DB * 2;
      vec8 vfr[NF];
      auto vread = [&](int f) __attribute__((always_inline)) {
        const FA_LDS char* base = vt + (f / (2 * C::DB)) * 32 * C::ROWB + (f % 2) * 16 * C::ROWB;
        const int db = (f / 2) % C::DB;
        vfr[f] = lds_read_tr_frag<T>(base + v_off[0][db], base + v_off[1][db]);
      };
      vread(0);
      vread(1);
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        if (f + 2 < NF) vread(f + 2);
        const int b = f / (2 * C::DB), db = (f / 2) % C::DB, ks = f % 2;
        oacc[0][db] = T::mfma(vfr[f], p0[b][ks], oacc[0][db]);
        oacc[1][db] = T::mfma(vfr[f], p1[b][ks], oacc[1][db]);
      }
    }
  };
  // unmasked tile with a LAZY running max (fa_fwd.hip tile_lazy): both query blocks are exponentiated against their
  // stale row max -- no max reduction, no lane exchange, no rescale test; FOLD: the chains start from -m, so the MFMA
  // output IS the exponent argument.  A lane's partial row sums bound every p it holds: if none exceeds kLazySumMaxV2
  // nothing can overflow and the stale max is as good as the true one; otherwise (always the first tile) nothing has been
  // committed and the caller redoes the tile on the exact path.
  auto tile_lazy = [&](int buf) __attribute__((always_inline)) -> bool {
    const FA_LDS char* kt = smem + buf * C::TILE_BYTES;
    const FA_LDS char* vt = smem + C::V_BASE + buf * C::TILE_BYTES;
    f32x16 s0[2], s1[2];
    const float i0 = FOLD ? -m[0] : 0.f, i1 = FOLD ? -m[1] : 0.f;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        s0[b][i] = i0;
        s1[b][i] = i1;
      }
    {
      constexpr int NF = 2 * C::KS;
      vec8 kfr[NF];
      auto kread = [&](int f) __attribute__((always_inline)) {
        kfr[f] = as_vec8<T>(lds_read16(kt + k_off[f % C::KS] + (f / C::KS) * 32 * C::ROWB));
      };
      kread(0);
      kread(1);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        if (f + 2 < NF) kread(f + 2);
        s0[f / C::KS] = T::mfma(kfr[f], qf[0][f % C::KS], s0[f / C::KS]);
        s1[f / C::KS] = T::mfma(kfr[f], qf[1][f % C::KS], s1[f / C::KS]);
        __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_s_setprio(0);
    }
    const float mc0 = m[0] * c2, mc1 = m[1] * c2;
    float la[4] = {0.f, 0.f, 0.f, 0.f}, lb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p0e = __builtin_amdgcn_exp2f(FOLD ? s0[b][i] : __builtin_fmaf(s0[b][i], c2, -mc0));
        s0[b][i] = p0e;
        la[i & 3] += p0e;
        const float p1e = __builtin_amdgcn_exp2f(FOLD ? s1[b][i] : __builtin_fmaf(s1[b][i], c2, -mc1));
        s1[b][i] = p1e;
        lb[i & 3] += p1e;
      }
    const float ls0 = (la[0] + la[1]) + (la[2] + la[3]), ls1 = (lb[0] + lb[1]) + (lb[2] + lb[3]);
    if (__builtin_amdgcn_ballot_w64(!(ls0 <= kLazySumMaxV2) || !(ls1 <= kLazySumMaxV2)) != 0) return false;
    l[0] += ls0;
    l[1] += ls1;
    vec8 p0[2][2], p1[2][2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      p0[b][0] = pack8<T, 0>(s0[b]);
      p0[b][1] = pack8<T, 1>(s0[b]);
      p1[b][0] = pack8<T, 0>(s1[b]);
      p1[b][1] = pack8<T, 1>(s1[b]);
    }
    {
      constexpr int NF = 2 * C::DB * 2;
      vec8 vfr[NF];
      auto vread = [&](int f) __attribute__((always_inline)) {
        const FA_LDS char* base = vt + (f / (2 * C::DB)) * 32 * C::ROWB + (f % 2) * 16 * C::ROWB;
        const int db = (f / 2) % C::DB;
        vfr[f] = lds_read_tr_frag<T>(base + v_off[0][db], base + v_off[1][db]);
      };
      vread(0);
      vread(1);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        if (f + 2 < NF) vread(f + 2);
        const int b = f / (2 * C::DB), db = (f / 2) % C::DB, ks = f % 2;
        oacc[0][db] = T::mfma(vfr[f], p0[b][ks], oacc[0][db]);
        oacc[1][db] = T::mfma(vfr[f], p1[b][ks], oacc[1][db]);
      }
      __builtin_amdgcn_s_setprio(0);
    }
    return true;
  };
  // masked tile (causal diagonal and/or ragged key tail) on the exact path.  (Trying the lazy path first, per query
  // block, measured -0.9 % with adjacent blocks and -3 % with the interleaved ones: the extra body and its control-flow
  // joins cost more than the four single-block tiles per wave and pass save.)
  auto tile_masked = [&](int t, int buf) __attribute__((always_inline)) {
    const FA_LDS char* kt = smem + buf * C::TILE_BYTES;
    const FA_LDS char* vt = smem + C::V_BASE + buf * C::TILE_BYTES;
    const int s0k = t * C::BN;
    auto one = [&](auto jt) __attribute__((always_inline)) {
      constexpr int j = decltype(jt)::value;
      const int qb0 = qrow(j);
      bool use[2];
#pragma unroll
      for (int b = 0; b < 2; ++b) use[b] = (s0k + 32 * b < p.Sk) && (!CAUSAL || s0k + 32 * b <= qb0);
      if (!use[0] && !use[1]) return;
      f32x16 s[2];
      vec8 pf[2][2];
      scores(kt, jt, s);
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = s0k + 32 * b + (i & 3) + 8 * (i >> 2) + 4 * h;
          const bool dead = !use[b] || (CAUSAL && key > qb0 + r) || key >= p.Sk;
          s[b][i] = dead ? -INFINITY : s[b][i];
        }
      row_max(jt, s);
      probs(jt, s, pf);
      pv(vt, jt, pf, use[0], use[1]);
    };
    one(J0{});
    one(J1{});
  };

  // retire tile t+1 (everything but the DMA just issued), then let every wave leave tile t
  auto ring_sync = [&](bool fetched) __attribute__((always_inline)) {
    asm volatile("" ::: "memory");  // keep LDS reads / DMA issue on their side of the barrier
    if (fetched) FA_WAIT_VMCNT(DMA_PER_TILE); else FA_WAIT_VMCNT(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  // the remaining steps of the workgroup: this wave's masked tile(s), then tiles it only helps stream
  auto step_tail = [&](int t, bool prefetched) __attribute__((always_inline)) {
    const int buf = t % 3;
    const bool fetch = t + 2 < ntiles;
    if (fetch && !prefetched) dma_tile(t + 2, (t + 2) % 3);
    if (t < n_mine) tile_masked(t, buf);
    ring_sync(fetch);
  };

  // tile 0 landed (Q fragments too: they were issued after tile 1's DMA, so wait for everything)
  asm volatile("" ::: "memory");
  FA_WAIT_VMCNT(0);
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  // Unmasked tiles: one exact tile (the first one, or the one a lazy tile bailed out of -- its prefetch is then already
  // issued), followed by lazy tiles until one bails out.  Separate loops on purpose: bodies that merge control flow get
  // their accumulators copied at every join.  `buf` = t % 3, carried along (tile t + 2 goes to slot (buf + 2) % 3).
#ifdef FA_STAMPS
  last_ = stamp_clock();
  begin_ = last_;
#endif
  int t = 0, buf = 0;
  bool prefetched = false;
  auto next_slot = [](int b) __attribute__((always_inline)) { return b == 2 ? 0 : b + 1; };
  while (t < nfull) {
    const bool fetch = t + 2 < ntiles;
    if (fetch && !prefetched) dma_tile(t + 2, next_slot(next_slot(buf)));
    FA_STAMP(0);  // DMA issue
    tile_full(buf);
    FA_STAMP(4);  // P V MFMAs
    ring_sync(fetch);
    FA_STAMP(5);  // vmcnt + barrier
    ++t;
    buf = next_slot(buf);
    prefetched = false;
    for (; t < nfull; ++t, buf = next_slot(buf)) {
      const bool fetch2 = t + 2 < ntiles;
      if (fetch2) dma_tile(t + 2, next_slot(next_slot(buf)));
      if (!tile_lazy(buf)) {
        prefetched = true;
        break;
      }
      ring_sync(fetch2);
    }
  }
  for (; t < ntiles; ++t) {
    step_tail(t, prefetched);
    prefetched = false;
  }

#ifdef FA_STAMPS
  const unsigned long long loop_end_ = stamp_clock();
#endif
  // ---- epilogue: all waves are past the last barrier, the ring is free for staging O ----
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float lt = half_sum(l[j]);
    const float inv = 1.0f / lt;
    store_tile_rows<D, T>(oacc[j], inv, smem + (wave * 2 + j) * 32 * C::ROWB, ro, qrow(j) * o_rs, lane, o_rs);
    if (h == 0) buf_store_f32(rl, (qrow(j) + r) * 4, m[j] * (FOLD ? kLn2 : p.scale) + __builtin_logf(lt));
  }
#ifdef FA_STAMPS
  if (p.dbg && lane == 0) {
    const unsigned long long end_ = stamp_clock_after_stores();
    unsigned long long* d = stamp_record(p.dbg, wave, 12);
    for (int i = 0; i < 6; ++i) d[i] = seg[i];
    d[6] = loop_end_ - begin_;
    d[7] = end_ - loop_end_;
    d[8] = nfull;   // stamped (unmasked) tiles only
    d[9] = ntiles;
    d[10] = begin_;
    d[11] = end_;
  }
#endif
  }  // pass
}

template <typename T, bool CAUSAL>
static hipError_t launch2(const FwdParams& p, hipStream_t s) {
  using C = Fwd2Cfg;
  const int grid = (CAUSAL && p.pair ? (p.nq_tiles + 1) / 2 : p.nq_tiles) * p.B * p.H;
  return launch_kernel<fa_fwd2_kernel<T, CAUSAL>>(grid, C::NT, C::LDS_BYTES, s, p);
}

hipError_t launch_fwd_v2(FwdParams p, int dtype, int causal, hipStream_t s) {
  p.nq_tiles = (p.Sq + Fwd2Cfg::BM - 1) / Fwd2Cfg::BM;
  p.pair = causal != 0;
  if (dtype == 1) return causal ? launch2<BF16, true>(p, s) : launch2<BF16, false>(p, s);
  return causal ? launch2<FP16, true>(p, s) : launch2<FP16, false>(p, s);
}

}  // namespace fa
