// Body of the split-KV decoding attention kernel (fa_decode.hip), included inside fa_decode_mod_kernel: the including
// kernel defines D, T, SOFTCAP with the cap `softcap`,
// ALIBI with the slopes (`slopes`, `slopes_bstride`) and the parameter block p.  Kept as text rather than as a
// device function so that the kernels compile exactly as they did before the transforms existed.  SOFTCAP: every score s
// becomes softcap * tanh(s * scale / softcap) before the masks and the log2 scaling (fa_common.h softcap_tanh).  ALIBI:
// every score gets -slope |pos - j| (pos = L - S_q + i, the mask's position), added in log2 units after the scaling.
// KV8 (include/mi355fa_kvcache_fp8.h): the caches hold OCP e4m3 bytes, a row is D bytes, and the
// kernel also defines `kds` / `vds` / `ds_bstride` (the dequantisation factors, NULL = 1).  A lane's 16-byte K load then
// holds the A fragments of TWO k-steps, d = 32 kp + 16 h + 8 e + j for k-step 2 kp + e, and the Q fragments are gathered
// with the same permutation of the contraction index; the bytes become T's 16-bit values without rounding (cvt_fp8 below)
// right in front of the MFMAs (K) and of the LDS write (V), so the LDS tile and everything after it are the 16-bit
// kernel's.  k_descale folds into the score scale and v_descale into the epilogue.
// KV4 (include/mi355fa_kvcache_fp4.h, include/mi355fa_ragged_fp4.h; the <D, T, SINK> overloads of fa_decode_mod_kernel /
// fa_decode_paged_kernel and fa_decode_ragged_kernel<T, D, SINK> define it true with the scale tensors
// `ksc` / `vsc` and their byte layouts `lks` / `lvs`, the other kernels false with placeholders): the caches hold MXFP4, a
// row is D / 2 bytes of e2m1 nibbles with one e8m0 scale byte per 32 elements in a tensor of its own.  A lane's 16-byte K
// load holds one whole scale block, the A fragments of FOUR k-steps: d = 64 kp + 32 h + 8 e + j for k-step 4 kp + e, the Q
// fragments gathered to match; a 16-byte V chunk is one scale block of one row.  A tile's scales come with its loads (the
// lane's row of K scales in one load, one byte per V chunk) through descriptors that end at row L as the caches' do, and
// cvt_fp4 turns nibbles and scale into T's 16-bit values where KV8 has cvt_fp8.  Everything after is the 16-bit kernel's.
// KV4 composes with PAGED and RAGGED (the flags touch disjoint code) and with D = 256 below (the packed call only), where a
// wave's half of a row is 64 bytes of nibbles and 4 of the row's 8 scale bytes: the D = 128 wave's loads at the offsets of its
// half (`coff`, load_scales).
// KVT (include/mi355fa_kvcache_fp8_token.h; fa_decode_tok_kernel / _tok_paged_kernel / _tok_ragged_kernel define it true, with
// KV8 true and no descales, and the row scales `ksc` / `vsc` as fp32 with the byte layouts `lks` / `lvs`): KV8's bytes, loads,
// permutation, LDS tile and MFMAs, with one fp32 scale per cache row instead of one per (sequence, head).  A tile's scales come
// with its loads through descriptors that end at row L (rebased on the page with the cache's): the lane's key row of K scales,
// the same row of V scales, and the V scale of each chunk the lane converts.  K's scale multiplies the fp32 score of its key.
// V's scale s = 2^e m (m in [1, 2)) is split: 2^e is the conversion's scale operand in front of the LDS write, so V enters the
// MFMA as the exact byte * 2^e, and m multiplies the fp32 probability of its key -- a factor below 2, so nothing small meets fp16.
// A score register belongs to a key, not to the lane's row, so the 32 K scales and V mantissas of a tile cross the wave through
// a 256-byte LDS slot of its own behind the loop's LDS (four 16-byte reads each per lane).  With every scale 1.0 the arithmetic
// is KV8's without descales, bit for bit.  Composes with PAGED, RAGGED, SINK and D = 256 (packed only; both waves of a pair
// read the same row scales).
// SINK (include/mi355fa_sink.h): `sinks` holds one logit per query head
// (natural-log units, not scaled by scale or k_descale).  Split 0 treats it as one more key of its merged (m, l) -- no
// value row -- so it enters each row's softmax exactly once whatever the split count, the partials keep their layout and
// the combine kernel is shared.  sinks[h] = -inf leaves (m, l, O) untouched, bit for bit.
// PAGED (include/mi355fa_paged.h; fa_decode_paged_kernel defines it true with `block_table`, `bt_stride`, `page_size`,
// `num_pages` and `tpp_div`, fa_decode_mod_kernel false with placeholders): p.kc / p.vc are pools of pages and load()
// takes each tile from its page.  Tiles, split shares, arithmetic and merge order are the padded kernel's, so the result
// has the bits of the padded kernel on the gathered cache.
// RAGGED (include/mi355fa_ragged.h; fa_decode_ragged_kernel defines it true with `cu_q`, `plan` and `total_q`, the other two
// kernels false with placeholders; paged pools only): packed queries [total_q, H, D] with a length S_b per sequence.  The
// work item's (b, rb) comes from the device-built plan instead of from the grid, S_q of the item is S_b, and Q / O / LSE /
// the partials are addressed by packed row.  From there it is the same work item: the result has the bits of the paged
// kernel on sequence b alone.
// D = 256 (SPLITD; the decode calls only): a wave that held a whole 32 x 256 tile of K, of V and the 8 blocks of O^T would need
// twice the D = 128 registers.  The four waves are instead 2 key groups x 2 halves of the head dim (kt = wave >> 1,
// dh = wave & 1): wave (kt, dh) loads columns [128 dh, 128 dh + 128) of its group's K and V tiles -- the D = 128 wave's loads at
// a column offset -- contracts its half of S^T, and after the pair has exchanged halves through LDS (at the loop) both
// waves run masks, transforms and the online softmax on the full score, then O^T += V^T P^T on the wave's own half of V.
// The merge joins two key groups instead of four waves.  Every other D compiles as if none of this were here.
  constexpr bool SPLITD = D == 256;                            // the head dim split over wave pairs (header, "D = 256")
  constexpr int HD = SPLITD ? D / 2 : D;                       // the head dims one wave contracts over and accumulates
  constexpr int NG = SPLITD ? kDecWaves / 2 : kDecWaves;       // key groups: the streams over interleaved tiles
  using C = DecCfg<HD>;                                        // the wave's tile
  using CL = DecLds<D>;                                        // the workgroup's LDS
  using vec8 = typename T::vec8;
  constexpr int KROWB = KV4 ? D / 2 : KV8 ? D : 2 * D;                       // bytes of a cache row
  constexpr int KL = KV4 ? C::KS / 4 : KV8 ? C::KS / 2 : C::KS;              // K loads (16 bytes) per lane per tile
  constexpr int VL = KV4 ? C::VL / 4 : KV8 ? C::VL / 2 : C::VL;              // V loads per lane per tile
  constexpr int VCPR = KV4 ? C::CPR / 4 : KV8 ? C::CPR / 2 : C::CPR;         // 16-byte chunks per cache row
  constexpr int SROWB = KVT ? 4 : D / 32;                                    // KV4 / KVT: bytes of a row of scales
  constexpr bool SCALED = KV4 || KVT;                                        // scale tensors beside the caches
  static_assert(!(KV4 && (KV8 || ALIBI)), "MXFP4 caches: plain, SINK and SOFTCAP");
  static_assert(!(KV4 && SPLITD && !RAGGED), "MXFP4 caches at D = 256: the packed call only");
  static_assert(!(KVT && (!KV8 || ALIBI)), "per-token-scaled e4m3 caches: KV8's bytes; plain, SINK and SOFTCAP");
  static_assert(!(KVT && SPLITD && !RAGGED), "per-token-scaled e4m3 caches at D = 256: the packed call only");
  // KVT: a wave's 32 K scales and 32 V mantissas of the tile in hand, behind everything the loop keeps in LDS (the V tiles and,
  // SPLITD, the score exchange) and inside the merge stage, which starts only after the loop
  // (words written one by one and read four at a time: types that may alias, so that the reads stay behind the writes)
  typedef float __attribute__((may_alias)) tsc_f32;
  typedef float __attribute__((ext_vector_type(4), may_alias)) tsc_f32x4;
  constexpr int TSC_OFF = C::STAGE_BYTES + 2 * kDecWaves * CL::XCH_SLOT, TSC_SLOT = 2 * kDecTile * 4;
  static_assert(!KVT || TSC_OFF + kDecWaves * TSC_SLOT <= CL::LDS_BYTES, "the scale slots fit under the merge stage");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  FA_LDS char* smem = (FA_LDS char*)smem_raw;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kt = SPLITD ? wave >> 1 : wave, dh = SPLITD ? wave & 1 : 0;   // the wave's key group and its half of the head dim
  const int coff = (KV4 ? HD / 2 : KV8 ? HD : 2 * HD) * dh;               // that half's first byte in a cache row

  // ---- work item: ((b * H_kv + hk) * RB + rb) * nsplit + split; RAGGED: (k * H_kv + hk) * nsplit + split, (b, rb) =
  // entry k of the plan, whose end marker (b outside [0, B)) leaves before any barrier ----
  int Sq = p.Sq, q0 = 0;      // RAGGED: S_b and the first packed row of sequence b,
  int pb = 0, prb = 0, phk = 0;   // and the work item
  if constexpr (RAGGED) {
    const int k = blockIdx.x / p.nsplit;
    phk = k % p.Hkv;
    // one wave-uniform 8-byte load; the plan kernel finished before this one started (constant address space, as the table)
    typedef const __attribute__((address_space(4))) int* const_plan_t;
    const const_plan_t e = (const_plan_t)plan + 4 + 2 * (long long)(k / p.Hkv);
    pb = __builtin_amdgcn_readfirstlane(e[0]);
    prb = __builtin_amdgcn_readfirstlane(e[1]);
    if ((unsigned)pb >= (unsigned)p.B) return;
    q0 = min(max(cu_q[pb], 0), total_q);
    Sq = min(max(cu_q[pb + 1], q0), total_q) - q0;
    // (cannot happen with the plan of this launch; with it the rows below stay inside S_b whatever the plan holds)
    if (prb < 0 || prb * kDecRows >= p.group * Sq) return;
  }
  const int g = p.group, M = g * Sq, RB = (M + kDecRows - 1) / kDecRows;
  int w = blockIdx.x;
  const int split = w % p.nsplit;
  w /= p.nsplit;
  const int rb = RAGGED ? prb : w % RB;
  if constexpr (!RAGGED) w /= RB;
  const int hk = RAGGED ? phk : w % p.Hkv, b = RAGGED ? pb : w / p.Hkv;
  const int L = RAGGED ? min(max(p.seqlens[b] + (p.Snew ? Sq : 0), 0), p.Scache) : kv_len(p, b);

  // ---- this row block's visible key tiles, and this split's share of them ----
  const int r0 = rb * kDecRows, rlast = min(M, r0 + kDecRows) - 1;
  const int pos0 = L - Sq + r0 / g, pos1 = L - Sq + rlast / g;   // positions of the block's first / last query
  const int lo = max(0, pos0 - p.wl), hi = min(L, pos1 + p.wr + 1);
  const int tb = lo / kDecTile, te = hi > lo ? (hi + kDecTile - 1) / kDecTile : tb;
  const int nt = te - tb;
  const int s_beg = tb + (int)((long long)nt * split / p.nsplit);
  const int s_end = tb + (int)((long long)nt * (split + 1) / p.nsplit);

  // ---- this lane's query row: Q^T fragments (B operand), position ----
  const int qrow = r0 + r, qi = qrow / g, qh = hk * g + (qrow - qi * g);
  const int pos = L - Sq + qi;
  vec8 qf[C::KS];
  {
    const bool valid = qrow < M;
    const char* qp;
    if constexpr (RAGGED)   // packed row q0 + qi (qi < S_b where valid: inside [0, total_q))
      qp = (const char*)p.q + (long long)qh * p.lq.sh + (long long)(q0 + qi) * p.lq.rs + (KV4 ? 64 : KV8 ? 32 : 16) * h + 2 * HD * dh;
    else
      qp = (const char*)p.q + b * p.lq.sb + (long long)qh * p.lq.sh + (long long)qi * p.lq.rs + (KV4 ? 64 : KV8 ? 32 : 16) * h + 2 * HD * dh;
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks)
      qf[ks] = as_vec8<T>(valid ? *(const u32x4*)(qp + (KV4   ? 128 * (ks >> 2) + 16 * (ks & 3)
                                                        : KV8 ? 64 * (ks >> 1) + 16 * (ks & 1)
                                                              : 32 * ks))
                                : u32x4{0u, 0u, 0u, 0u});
  }

  // ---- K / V of (b, hk): rows [0, L) only ----
  const int rs = p.lk.rs;
  const __amdgpu_buffer_rsrc_t rk = make_rsrc((const char*)p.kc + b * p.lk.sb + hk * p.lk.sh, view_bytes(L, rs, KROWB));
  const __amdgpu_buffer_rsrc_t rv = make_rsrc((const char*)p.vc + b * p.lv.sb + hk * p.lv.sh, view_bytes(L, rs, KROWB));
  // KV4 / KVT: the scales of (b, hk), rows [0, L) only as well
  const int srk = lks.rs, srv = lvs.rs;
  __amdgpu_buffer_rsrc_t rks = rk, rvs = rv;
  if constexpr (SCALED && !PAGED) {
    rks = make_rsrc((const char*)ksc + b * lks.sb + hk * lks.sh, view_bytes(L, srk, SROWB));
    rvs = make_rsrc((const char*)vsc + b * lvs.sb + hk * lvs.sh, view_bytes(L, srv, SROWB));
  }

  FA_LDS char* vt = smem + wave * kDecTile * C::ROWB;
  int v_off[2][C::DB];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int db = 0; db < C::DB; ++db) v_off[e][db] = tr_lane_off<HD>(lane, 8 * e, db);

  // PAGED: tile t lies in page page_of(t) of the pool, and its descriptors cover that page's rows below L only, based on
  // the page (a 64-bit base: the pool may exceed 2^32 bytes), with the offsets of the tile inside the page.  The entry is
  // wave-uniform (b and t are); readfirstlane says so to the compiler, which otherwise wraps every buffer load in a
  // waterfall loop.  The table is read through the constant address space (nothing writes it while the kernel runs):
  // inside the loop, behind the LDS writes, hipcc otherwise makes the lookup a vector load, and the vmcnt(0) in front of
  // its readfirstlane waits for the tile loads just issued.  As a scalar load it is retired by the loop's own
  // lgkmcnt(0).  An entry outside the pool gives an empty descriptor at the pool's base.
  typedef const __attribute__((address_space(4))) int* const_table_t;
  const const_table_t table = (const_table_t)block_table + (long long)b * bt_stride;
  auto page_of = [&](int t) __attribute__((always_inline)) {
    return __builtin_amdgcn_readfirstlane(table[tpp_div.div(t)]);
  };
  u32x4 kr[KL], vr[VL];
  unsigned ksr = 0, vsr[SCALED ? VL : 1];   // KV4: the lane's row of K scales (SROWB bytes) and the scale byte of each V chunk
  unsigned vrr = 0;                         // KVT: ksr / vrr = the K / V scale of key row r, vsr[u] = the V scale of chunk u's row
  // the scale loads of a tile, issued with its K / V loads: K scales of row r, V scale of chunk c of each of the lane's rows
  // (SPLITD: the wave's HD / 32 = 4 of the row's 8 scale bytes, at byte 4 dh -- the D = 128 wave's one b32 load, aligned as the
  // scale rows are to D / 32 bytes; chunk c of the wave's half is chunk c + VCPR dh of the row)
  auto load_scales = [&](__amdgpu_buffer_rsrc_t dk, __amdgpu_buffer_rsrc_t dv, int bk, int bv) __attribute__((always_inline)) {
    if constexpr (KVT) {
      ksr = __builtin_amdgcn_raw_buffer_load_b32(dk, bk + r * srk, 0, 0);
      vrr = __builtin_amdgcn_raw_buffer_load_b32(dv, bv + r * srv, 0, 0);
#pragma unroll
      for (int u = 0; u < VL; ++u) vsr[u] = __builtin_amdgcn_raw_buffer_load_b32(dv, bv + ((lane + 64 * u) / VCPR) * srv, 0, 0);
      return;
    }
    if constexpr (SPLITD)
      ksr = __builtin_amdgcn_raw_buffer_load_b32(dk, bk + r * srk + (HD / 32) * dh, 0, 0);
    else if constexpr (SROWB == 4)
      ksr = __builtin_amdgcn_raw_buffer_load_b32(dk, bk + r * srk, 0, 0);
    else
      ksr = __builtin_amdgcn_raw_buffer_load_b16(dk, bk + r * srk, 0, 0);
#pragma unroll
    for (int u = 0; u < VL; ++u) {
      const int id = lane + 64 * u, row = id / VCPR, c = id % VCPR;
      if constexpr (SPLITD)
        vsr[u] = __builtin_amdgcn_raw_buffer_load_b8(dv, bv + row * srv + c + VCPR * dh, 0, 0);
      else
        vsr[u] = __builtin_amdgcn_raw_buffer_load_b8(dv, bv + row * srv + c, 0, 0);
    }
  };
  auto load = [&](int t) __attribute__((always_inline)) {
    const int base = t * kDecTile * rs + coff;
#pragma unroll
    for (int ks = 0; ks < KL; ++ks) kr[ks] = buf_load16(rk, base + r * rs + 32 * ks + 16 * h);
#pragma unroll
    for (int u = 0; u < VL; ++u) {
      const int id = lane + 64 * u, row = id / VCPR, c = id % VCPR;
      vr[u] = buf_load16(rv, base + row * rs + c * 16);
    }
    if constexpr (SCALED) load_scales(rks, rvs, t * kDecTile * srk, t * kDecTile * srv);
  };
  // The descriptors and the first offset of the tile the next load_paged() takes: built by page_desc(t, page_of(t)) a
  // step before those loads are issued, during the previous tile's MFMAs, and carried over the loop's back edge.  Built at
  // the loads themselves, the ~40 dependent scalar instructions sat between the arrival of one tile and the issue of the
  // next, where the wave has no load in flight.
  // KV4: the scale pools go through the same entry, as two more descriptors of the page's rows below L (DESIGN.md section 3 has
  // the register counts of this form).
  __amdgpu_buffer_rsrc_t rkp = rk, rvp = rv, rksp = rk, rvsp = rv;
  int basep = 0, sbkp = 0, sbvp = 0;
  auto page_desc = [&](int t, int pg) __attribute__((always_inline)) {
    const int first = tpp_div.div(t) * page_size;                         // the page's first key
    const int ok = (unsigned)pg < (unsigned)num_pages ? 1 : 0;
    const unsigned bytes = view_bytes(min(L - first, page_size) * ok, rs, KROWB);
    rkp = make_rsrc((const char*)p.kc + (long long)(pg * ok) * p.lk.sb + hk * p.lk.sh, bytes);
    rvp = make_rsrc((const char*)p.vc + (long long)(pg * ok) * p.lv.sb + hk * p.lv.sh, bytes);
    basep = (t * kDecTile - first) * rs + coff;
    if constexpr (SCALED) {
      const int rows = min(L - first, page_size) * ok;
      rksp = make_rsrc((const char*)ksc + (long long)(pg * ok) * lks.sb + hk * lks.sh, view_bytes(rows, srk, SROWB));
      rvsp = make_rsrc((const char*)vsc + (long long)(pg * ok) * lvs.sb + hk * lvs.sh, view_bytes(rows, srv, SROWB));
      sbkp = (t * kDecTile - first) * srk;
      sbvp = (t * kDecTile - first) * srv;
    }
  };
  auto load_paged = [&]() __attribute__((always_inline)) {   // load()'s loads through (rkp, rvp, basep)
    const int base = basep;
#pragma unroll
    for (int ks = 0; ks < KL; ++ks) kr[ks] = buf_load16(rkp, base + r * rs + 32 * ks + 16 * h);
#pragma unroll
    for (int u = 0; u < VL; ++u) {
      const int id = lane + 64 * u, row = id / VCPR, c = id % VCPR;
      vr[u] = buf_load16(rvp, base + row * rs + c * 16);
    }
    if constexpr (SCALED) load_scales(rksp, rvsp, sbkp, sbvp);
  };

  float kd = 1.f, vd = 1.f;   // KV8: the (sequence, K/V head)'s dequantisation factors
  if constexpr (KV8) {
    kd = kds ? kds[b * ds_bstride + hk] : 1.f;
    vd = vds ? vds[b * ds_bstride + hk] : 1.f;
  }
  const float c2 = KV8 ? p.scale * kd * kLog2e : p.scale * kLog2e;   // scores in log2 units
  // (KV8: k_descale belongs to the score, so it goes under the tanh with the scale -- tanh(scale * kd * s / softcap))
  const SoftCap sc = SOFTCAP ? make_softcap(softcap, (KV8 ? p.scale * kd : p.scale) / softcap) : SoftCap{0.f, 0.f};
  // ALIBI: the rows of a block belong to different query heads (qh), so the slope is per lane (qh < H for every lane)
  const float alibi_k = ALIBI ? slopes[b * slopes_bstride + qh] * kLog2e : 0.f;
  float m = -INFINITY, l = 0.f;
  f32x16 oacc[C::DB];
#pragma unroll
  for (int db = 0; db < C::DB; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[db][i] = 0.f;

  // PAGED: at the top of step t the loads of tile t are in flight, (rkp, rvp, basep) describe tile t + NG and pgn is the
  // table entry of tile t + 2 NG, so neither a table round trip nor the descriptor arithmetic sits in front of a tile's loads
  // (the first two tiles' apart).  Only tiles below s_end are looked up: entries at or past ceil(L / page_size) are never
  // read.
  int t = s_beg + kt;
  int pgn = 0;
  if constexpr (PAGED) {
    if (t < s_end) {
      page_desc(t, page_of(t));
      load_paged();
      if (t + NG < s_end) page_desc(t + NG, page_of(t + NG));
      if (t + 2 * NG < s_end) pgn = page_of(t + 2 * NG);
    }
  } else {
    if (t < s_end) load(t);
  }
  // SPLITD: the two waves of a pair hand each other their halves of S^T through LDS behind a workgroup barrier, so every
  // wave runs the same number of steps, from the workgroup-uniform s_beg / s_end alone: a pair whose tile lies past s_end
  // (the last step of an odd share, every step of an empty one) only joins the barrier.  `t` is uniform over the pair.
  FA_LDS char* xch = smem + CL::XCH_OFF;
  auto xch_sync = [&]() __attribute__((always_inline)) {   // this wave's LDS writes have landed and its reads returned
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(waitcnt_imm(kNoWait, 0));
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  // (the loop runs while the step's first tile, t - kt = s_beg + 2 * step, lies below s_end)
  for (; (SPLITD ? t - kt : t) < s_end; t += NG) {
    if constexpr (SPLITD) {
      if (t >= s_end) {
        xch_sync();
        continue;
      }
    }
    // V of tile t into the wave's LDS tile (the previous tile's transposed reads precede these writes in LDS order)
#pragma unroll
    for (int u = 0; u < VL; ++u) {
      const int id = lane + 64 * u, row = id / VCPR, c = id % VCPR;
      if constexpr (KV4) {   // the chunk is one scale block: 32 elements, four 16-byte pieces of the LDS row
        const float sv = e8m0_scale(vsr[u]);
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_write16(vt + lds_off<HD>(row, 4 * c + i), cvt_fp4<T>(vr[u][i], sv));
      } else if constexpr (KVT) {   // the power of two of the row's scale: the conversion reads the exponent field alone
        const float sv = __builtin_bit_cast(float, vsr[u]);
        lds_write16(vt + lds_off<HD>(row, 2 * c), cvt_fp8_pow2<T>(vr[u][0], vr[u][1], sv));
        lds_write16(vt + lds_off<HD>(row, 2 * c + 1), cvt_fp8_pow2<T>(vr[u][2], vr[u][3], sv));
      } else if constexpr (KV8) {
        lds_write16(vt + lds_off<HD>(row, 2 * c), cvt_fp8<T>(vr[u][0], vr[u][1]));
        lds_write16(vt + lds_off<HD>(row, 2 * c + 1), cvt_fp8<T>(vr[u][2], vr[u][3]));
      } else {
        lds_write16(vt + lds_off<HD>(row, c), vr[u]);
      }
    }
    u32x4 kc[KL];
#pragma unroll
    for (int ks = 0; ks < KL; ++ks) kc[ks] = kr[ks];
    float ksf[KL];   // KV4: the scale of the block load ks holds, block 2 ks + h of the row
#pragma unroll
    for (int ks = 0; ks < KL; ++ks) ksf[ks] = KV4 ? e8m0_scale((ksr >> (16 * ks + 8 * h)) & 0xffu) : 1.f;
    // KVT: key row r's K scale and V mantissa into the wave's slot (both halves write the same words), read back by key below
    FA_LDS char* tsc = smem + TSC_OFF + wave * TSC_SLOT;
    if constexpr (KVT) {
      *(FA_LDS tsc_f32*)(tsc + 4 * r) = __builtin_bit_cast(float, ksr);
      *(FA_LDS tsc_f32*)(tsc + 4 * kDecTile + 4 * r) = __builtin_bit_cast(float, (vrr & 0x007fffffu) | 0x3f800000u);
    }
    if constexpr (PAGED) {
      if (t + NG < s_end) {
        load_paged();
      }
    } else {
      if (t + NG < s_end) load(t + NG);   // next tile in flight while this one is computed
    }

    // ---- S^T = K Q^T: reg i of lane (r, h) = score of query row r, key t*32 + (i&3) + 8(i>>2) + 4h ----
    f32x16 s;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
      if constexpr (KV4)
        s = T::mfma(as_vec8<T>(cvt_fp4<T>(kc[ks >> 2][ks & 3], ksf[ks >> 2])), qf[ks], s);
      else if constexpr (KV8)
        s = T::mfma(as_vec8<T>(cvt_fp8<T>(kc[ks >> 1][2 * (ks & 1)], kc[ks >> 1][2 * (ks & 1) + 1])), qf[ks], s);
      else
        s = T::mfma(as_vec8<T>(kc[ks]), qf[ks], s);
    }
    if constexpr (SPLITD) {
      // s is this wave's half of the contraction: the pair swaps halves through two slots per wave, taken by step parity,
      // behind ONE barrier per step (the write of step k + 2 follows the barrier of step k + 1, which the partner joins
      // only once its read of step k has returned).  The sum is half 0 + half 1 in both waves -- the same bits, so the
      // pair holds one m, l and P for the two halves of a row.  Everything below runs on the full score, in both waves.
      // (a slot: 16 registers of 64 lanes, as four wave-contiguous 16-byte rows)
      const int par = ((t - s_beg) >> 1) & 1;   // the step's parity (t - kt = s_beg + 2 * step)
      FA_LDS char* mine = xch + (par * kDecWaves + wave) * CL::XCH_SLOT + lane * 16;
      FA_LDS char* theirs = xch + (par * kDecWaves + (wave ^ 1)) * CL::XCH_SLOT + lane * 16;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        *(FA_LDS f32x4*)(mine + c * (CL::XCH_SLOT / 4)) = f32x4{s[4 * c], s[4 * c + 1], s[4 * c + 2], s[4 * c + 3]};
      xch_sync();
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f32x4 o = *(const FA_LDS f32x4*)(theirs + c * (CL::XCH_SLOT / 4));
#pragma unroll
        for (int j = 0; j < 4; ++j) s[4 * c + j] = dh == 0 ? s[4 * c + j] + o[j] : o[j] + s[4 * c + j];
      }
    }
    if constexpr (KVT) {   // register i is key (i & 3) + 8 (i >> 2) + 4 h of the tile: its K scale on the fp32 score
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f32x4 kq = *(const FA_LDS tsc_f32x4*)(tsc + 16 * h + 32 * c);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[4 * c + j] *= kq[j];
      }
    }
    float tm = -INFINITY;
    const float qk = ALIBI ? (float)(pos - t * kDecTile - 4 * h) : 0.f;   // (position - key) of register 0
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int key = t * kDecTile + (i & 3) + 8 * (i >> 2) + 4 * h;
      const bool dead = key >= L || key < pos - p.wl || key > pos + p.wr;
      s[i] = dead ? -INFINITY
                  : (SOFTCAP ? sc.k2 * softcap_tanh(sc, s[i])
                             : (ALIBI ? alibi_add(alibi_k, qk - (float)((i & 3) + 8 * (i >> 2)), s[i] * c2) : s[i] * c2));
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
    if constexpr (KVT) {   // the mantissa of each key's V scale on its probability (l keeps the plain sum)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f32x4 vm = *(const FA_LDS tsc_f32x4*)(tsc + 4 * kDecTile + 16 * h + 32 * c);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[4 * c + j] *= vm[j];
      }
    }
    // ---- O^T += V^T P^T ----
    const vec8 pf0 = pack8<T, 0>(s), pf1 = pack8<T, 1>(s);
    __builtin_amdgcn_s_waitcnt(waitcnt_imm(kNoWait, 0));   // this wave's V writes have landed
    if constexpr (PAGED) {   // the descriptors two tiles ahead from the entry looked up a step ago; the next lookup
      if (t + 2 * NG < s_end) page_desc(t + 2 * NG, pgn);
      if (t + 3 * NG < s_end) pgn = page_of(t + 3 * NG);
    }
#pragma unroll
    for (int db = 0; db < C::DB; ++db) {
      const vec8 a0 = lds_read_tr_frag<T>(vt + v_off[0][db], vt + v_off[1][db]);
      oacc[db] = T::mfma(a0, pf0, oacc[db]);
      const vec8 a1 = lds_read_tr_frag<T>(vt + 16 * C::ROWB + v_off[0][db], vt + 16 * C::ROWB + v_off[1][db]);
      oacc[db] = T::mfma(a1, pf1, oacc[db]);
    }
  }
  const float lt = half_sum(l);

  // ---- merge the four waves (wave order; SPLITD: the two key groups, (m, l) from the waves of half 0 and each wave's O at
  // its half's columns), then O / LSE or the split's partial ----
  __syncthreads();   // every wave is done with its V tile: the LDS is the merge stage now
  float* stage = (float*)smem_raw;
  float* sm = (float*)(smem_raw + CL::ML_OFF);
  float* sl = sm + NG * kDecRows;
  if (h == 0 && dh == 0) {
    sm[kt * kDecRows + r] = m;
    sl[kt * kDecRows + r] = lt;
  }
#pragma unroll
  for (int db = 0; db < C::DB; ++db)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      *(f32x4*)(stage + (kt * kDecRows + r) * CL::OST + HD * dh + db * 32 + 8 * c + 4 * h) =
          f32x4{oacc[db][4 * c], oacc[db][4 * c + 1], oacc[db][4 * c + 2], oacc[db][4 * c + 3]};
  __syncthreads();
  const long long R = RAGGED ? (long long)p.H * total_q : (long long)p.B * p.H * p.Sq;   // rows of O / LSE / a split's partials
  for (int it = tid; it < kDecRows * (D / 4); it += 256) {
    const int row = it / (D / 4), d4 = (it % (D / 4)) * 4;
    const int qr = r0 + row;
    if (qr >= M) break;   // rows ascend with `it`
    float mx = -INFINITY;
#pragma unroll
    for (int v = 0; v < NG; ++v) mx = __builtin_fmaxf(mx, sm[v * kDecRows + row]);
    const float mo = mx == -INFINITY ? 0.f : mx;
    float ls = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int v = 0; v < NG; ++v) {
      const float e = __builtin_amdgcn_exp2f(sm[v * kDecRows + row] - mo);
      ls += e * sl[v * kDecRows + row];
      acc += e * *(const f32x4*)(stage + (v * kDecRows + row) * CL::OST + d4);
    }
    if constexpr (KV8) acc *= vd;   // before the partial is written: the combine kernel is the 16-bit one
    const int i = qr / g, head = hk * g + (qr - i * g);
    if constexpr (SINK) {
      if (split == 0) {   // the sink as the last key of split 0: the usual max update (z = -inf: factors 1 and 0)
        const float z2 = sinks[head] * kLog2e;
        const float mz = __builtin_fmaxf(mx, z2);
        if (mz != -INFINITY) {   // (a keyless row with z = -inf stays m = -inf, l = 0)
          const float a = __builtin_amdgcn_exp2f(mx - mz);
          ls = __builtin_fmaf(ls, a, __builtin_amdgcn_exp2f(z2 - mz));
          acc *= a;
          mx = mz;
        }
      }
    }
    const long long ridx = RAGGED ? (long long)head * total_q + (q0 + i) : ((long long)b * p.H + head) * p.Sq + i;
    if (p.nsplit == 1) {
      const float inv = ls > 0.f ? 1.f / ls : 0.f;
      typedef __attribute__((ext_vector_type(4))) typename T::elem e4;
      e4 ov;
#pragma unroll
      for (int j = 0; j < 4; ++j) ov[j] = (typename T::elem)(acc[j] * inv);
      if constexpr (RAGGED)
        *(u32x2*)((char*)p.o + (long long)head * p.lo.sh + (long long)(q0 + i) * p.lo.rs + d4 * 2) = __builtin_bit_cast(u32x2, ov);
      else
        *(u32x2*)((char*)p.o + b * p.lo.sb + (long long)head * p.lo.sh + (long long)i * p.lo.rs + d4 * 2) =
            __builtin_bit_cast(u32x2, ov);
      if (d4 == 0 && p.lse) p.lse[ridx] = ls > 0.f ? (mx + __builtin_log2f(ls)) * kLn2 : -INFINITY;
    } else {
      const long long pr = split * R + ridx;
      *(f32x4*)(p.ws + pr * D + d4) = acc;
      if (d4 == 0) *(f32x2_t*)(p.ws + (long long)p.nsplit * R * D + 2 * pr) = f32x2_t{mx, ls};
    }
  }
