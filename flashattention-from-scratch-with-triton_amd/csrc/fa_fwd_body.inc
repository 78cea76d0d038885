// Body of the family-1 forward kernels (fa_fwd.hip), included inside fa_fwd_kernel and fa_fwd_mod_kernel (the window, GQA,
// soft-cap, ALiBi and sink variants): the including kernel defines D, T,
// CAUSAL, DROP, LOCAL, the window (wl, wr), GQA, the head group size `group`, SOFTCAP with the cap `softcap`, ALIBI with
// the slopes (`slopes`, `slopes_bstride`), SINK with the per-head sink logits `sinks` and the parameter block p.  Shared as text rather than through a device function so that fa_fwd_kernel
// compiles exactly as it did before the window and the head groups existed.
  using C = FwdCfg<D>;
  using vec8 = typename T::vec8;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  FA_LDS char* smem = (FA_LDS char*)smem_raw;

  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);

  // ---- which (batch*head, q tile) ----
  // Work list: non-causal -> one 128-row query tile per workgroup.  Causal -> query tile i streams i+1
  // K/V tiles, so a workgroup takes the PAIR (nq-1-i, i): every workgroup then does the same work and the
  // grid is balanced whatever the number of CUs (heavy tile first).
  // (fa_kernels.h tile_index; variable-length launch: this sequence's rows and lengths come from cu_seqlens, and the grid
  // was sized for the longest sequence, so workgroups past this one's own tile count have nothing to do)
  const TileIndex<CAUSAL> tw = tile_index<CAUSAL>(p, p.nq_tiles);
  const BatchHead ix = batch_head(tw.bh, p.B, p.H, p.vl.cu_q != nullptr);
  const int b_ = ix.b, h_ = ix.h;
  const int hk_ = GQA ? h_ / group : h_;  // GQA: query head h reads K/V head h / group
  const SeqInfo si = seq_info(p.vl, b_, p.Sq, p.Sk);
  const int Sq = si.Sq, Sk = si.Sk;
  const int nq = (Sq + C::BM - 1) / C::BM;
  if (tw.surplus(nq)) return;
  const int npass = tw.npass(nq);
  for (int pass = 0; pass < npass; ++pass) {
  // lane coordinates re-derived per pass (fa_common.h lane_id_now): nothing lane-dependent stays live across passes
  const int lane = lane_id_now(), tid = wave * 64 + lane, r = lane & 31, h = lane >> 5;
  const int qt = tw.qtile(nq, pass);  // heavy first
  const int q0_wg = qt * C::BM;
  const int qw0 = q0_wg + wave * 32;
  if (pass) __syncthreads();  // the previous pass staged its O tile in the K/V buffers

  // inputs may be strided views with a contiguous head dim (e.g. a [B,S,H,D] buffer seen as [B,H,S,D]): per-tensor
  // batch / head byte strides, one row stride for Q and one shared by K and V; O has its own layout (contiguous for the
  // reference's launch, packed rows for varlen), LSE rows of one (batch, head) are contiguous
  const int q_rs = p.lq.rs, kv_rs = p.lk.rs, o_rs = p.lo.rs;
  const char* qb = (const char*)p.q + b_ * p.lq.sb + h_ * p.lq.sh + (long long)si.q0 * q_rs;
  const char* kb = (const char*)p.k + b_ * p.lk.sb + hk_ * p.lk.sh + (long long)si.k0 * kv_rs;
  const char* vb = (const char*)p.v + b_ * p.lv.sb + hk_ * p.lv.sh + (long long)si.k0 * kv_rs;
  char* ob = (char*)p.o + b_ * p.lo.sb + h_ * p.lo.sh + (long long)si.q0 * o_rs;
  const __amdgpu_buffer_rsrc_t rq = make_rsrc(qb, (unsigned)(Sq - 1) * q_rs + C::ROWB);
  const __amdgpu_buffer_rsrc_t rk = make_rsrc(kb, view_bytes(Sk, kv_rs, C::ROWB));
  const __amdgpu_buffer_rsrc_t rv = make_rsrc(vb, view_bytes(Sk, kv_rs, C::ROWB));
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(ob, (unsigned)(Sq - 1) * o_rs + C::ROWB);
  const __amdgpu_buffer_rsrc_t rl = make_rsrc(p.lse + b_ * p.lse_sb + h_ * p.lse_sh + si.q0, (unsigned)Sq * 4);


  // ---- Q^T fragments (B operand), resident for the whole kernel ----
  vec8 qf[C::KS];
#pragma unroll
  for (int ks = 0; ks < C::KS; ++ks)
    qf[ks] = as_vec8<T>(buf_load16(rq, (qw0 + r) * q_rs + (2 * ks + h) * 16));

  // ---- tile schedule ----
  const int kv_end = CAUSAL ? min(Sk, q0_wg + C::BM) : Sk;
  // LOCAL: tiles [t_begin, ntiles) meet the workgroup's band, [tf0, nfull) need no mask for this wave
  const LocalTiles lt_ = LOCAL ? local_tiles<C::BN>(q0_wg, min(q0_wg + C::BM, Sq) - 1, qw0, Sk, wl, wr) : LocalTiles{};
  const int t_begin = LOCAL ? lt_.begin : 0, tf0 = LOCAL ? lt_.full0 : 0;
  const int ntiles = LOCAL ? lt_.end : (kv_end + C::BN - 1) / C::BN;
  // tiles [0, nfull) need no mask for this wave
  const int nfull = LOCAL ? lt_.full1 : (CAUSAL ? min(Sk / C::BN, qw0 / C::BN) : Sk / C::BN);

  // ---- staging addresses ----
  // ---- LDS-DMA: wave w fills rows [16w, 16w+16) of each K / V tile, 1 KiB (1024 / ROWB rows) per instruction
  constexpr int RPI = 1024 / C::ROWB;  // rows per piece; dma_pieces: the immediate offset 1024 i of piece i is taken out
  int dma_src[C::DMA_PER_MAT];
#pragma unroll
  for (int i = 0; i < C::DMA_PER_MAT; ++i) dma_src[i] = dma_src_off<D>(16 * wave + RPI * i, lane, kv_rs) - 1024 * i;
  // ---- fragment read addresses (loop invariant) ----
  int k_off[C::KS];
#pragma unroll
  for (int ks = 0; ks < C::KS; ++ks) k_off[ks] = lds_off<D>(r, 2 * ks + h);
  int v_off[2][C::DB];  // [e][dblk]; key-block kb and k-step s add (32*kb + 16*s) rows
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int db = 0; db < C::DB; ++db) v_off[e][db] = tr_lane_off<D>(lane, 8 * e, db);

  const float c2 = p.scale * kLog2e;  // exp(x*scale) = exp2(x*c2)
  // FOLD (bf16, fa_common.h): Q carries c2, the MFMA delivers scores in log2 units (cs = 1) and a lazy tile's
  // score chain starts from a block holding -m, so its exponent argument needs no VALU op at all.
  constexpr bool FOLD = T::kFoldScale;
  // SOFTCAP: every score is capped right after its MFMA chain, u*log2e = cap*log2e * tanh(y) (fa_common.h softcap_tanh),
  // so from there on the scores are in log2 units whatever FOLD is (y = x / (cap*log2e) with FOLD, x*scale/cap without)
  constexpr bool LOG2 = FOLD || SOFTCAP;
  const SoftCap sc = SOFTCAP ? make_softcap(softcap, FOLD ? 1.0f / (softcap * kLog2e) : p.scale / softcap) : SoftCap{0.f, 0.f};
  const float cs = LOG2 ? 1.0f : c2;  // accumulator units -> log2 units
  // ALIBI: the bias -slope |q - k| is one fma per score with a factor in the units of the score it is added to: log2 units
  // with FOLD (slope * log2e), accumulator units without (slope / scale), so the running max and LSE include it
  const float alibi_k = ALIBI ? alibi_slope(slopes, b_ * slopes_bstride + h_, FOLD ? kLog2e : 1.0f / p.scale) : 0.f;
  // SINK (include/mi355fa_sink.h): the head's sink logit in the units of the running max m (log2 units: z * log2e,
  // accumulator units: z / scale), loaded here, used once in the epilogue.  -inf stays -inf.
  const float sink_m = SINK ? alibi_slope(sinks, h_, LOG2 ? kLog2e : 1.0f / p.scale) : 0.f;
  if constexpr (FOLD) {
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) qf[ks] = scale_frag<T>(qf[ks], c2);
  }
  const float defer_raw = kDeferLog2 / cs;  // rescale threshold in accumulator units
  float m = -INFINITY;                // running row max in accumulator units (raw scores, or log2 units if FOLD)
  f32x16 negm;                        // FOLD: -m in every register (this lane's query row)
#pragma unroll
  for (int i = 0; i < 16; ++i) negm[i] = INFINITY;
  float l = 0.f;                      // this lane's partial row sum (its 16 of every 32 keys)
  f32x16 oacc[C::DB];
#pragma unroll
  for (int db = 0; db < C::DB; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[db][i] = 0.f;

  auto dma_tile = [&](int t, int buf) __attribute__((always_inline)) {
    const int soff = t * C::BN * kv_rs;
    const int dst0 = buf * C::TILE_BYTES + 16 * wave * C::ROWB;  // this wave's 16 rows = DMA_PER_MAT consecutive KiB
    dma_pieces<C::DMA_PER_MAT>(rk, lds_addr_of(smem + dst0), dma_src, soff);
    dma_pieces<C::DMA_PER_MAT>(rv, lds_addr_of(smem + 2 * C::TILE_BYTES + dst0), dma_src, soff);
  };

  // One 64-key tile for this wave.  MASKED = false: every key visible to every row.
  // BUF = 0/1: LDS buffer known at compile time (offsets fold into the ds_read immediates);
  // BUF = -1: taken from t at run time (the few masked tiles).
  // DROP: zero the dropped weights of one 32 x 32 block.  Registers 4g..4g+3 of a lane are four consecutive keys of its row =
  // the four bytes of word (row & 3) of patch g, which lane g of the quad generated (fa_common.h quad_bcast).  The factor
  // 1 / (1 - p) of the kept weights is linear in O and applied once, with the normalisation in the epilogue.
  auto drop_weights = [&](f32x16& w16, const u32x4& mine) __attribute__((always_inline)) {
    const unsigned thresh = p.drop.thresh;
    const int qsel = (qw0 + r) & 3;
    auto apply = [&](auto g_tag) __attribute__((always_inline)) {
      constexpr int g = decltype(g_tag)::value;
      const unsigned w = select_word(quad_bcast4<g>(mine), qsel);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool keep = ((w >> (8 * j)) & 255u) >= thresh;
        w16[4 * g + j] = keep ? w16[4 * g + j] : 0.f;
      }
    };
    apply(std::integral_constant<int, 0>{});
    apply(std::integral_constant<int, 1>{});
    apply(std::integral_constant<int, 2>{});
    apply(std::integral_constant<int, 3>{});
  };

  auto tile = [&](int t, auto buf_tag, auto masked_tag) {
    constexpr bool MASKED = decltype(masked_tag)::value;
    constexpr int BUF = decltype(buf_tag)::value;
    const int buf = BUF >= 0 ? BUF : (t & 1);
    const FA_LDS char* kt = smem + buf * C::TILE_BYTES;
    const FA_LDS char* vt = smem + (2 + buf) * C::TILE_BYTES;
    const int s0 = t * C::BN;
    bool use[2] = {true, true};
    if constexpr (MASKED) {
      if (CAUSAL) {
        use[0] = s0 <= qw0;        // key block start <= first row of the wave
        use[1] = s0 + 32 <= qw0;
      }
      if (LOCAL) {  // the key block meets the band of some row of the wave
        use[0] = s0 <= qw0 + 31 + wr && s0 + 31 >= qw0 - wl;
        use[1] = s0 + 32 <= qw0 + 31 + wr && s0 + 63 >= qw0 - wl;
      }
      use[0] = use[0] && s0 < Sk;
      use[1] = use[1] && s0 + 32 < Sk;
      if (!use[0] && !use[1]) return;
    }
    f32x16 sacc[2];
    // DROP: one Philox call per lane and key block -- registers 4g..4g+3 are keys s0 + 32b + 8g + 4h + 0..3 of row qw0 + r,
    // i.e. word (row & 3) of patch g, and the quad's four lanes (four consecutive rows) need the same four patches: lane j
    // generates patch g = j (fa_common.h quad_bcast).  Issued here so that its integer ops run beside the MFMA chains.
    u32x4 mine[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    if constexpr (DROP) {
      const Dropout dr{p.drop.thresh, p.drop.seed_lo, p.drop.seed_hi, p.drop.offset, p.drop.rp};
#pragma unroll
      for (int b = 0; b < 2; ++b)
        if (!(MASKED && !use[b])) mine[b] = dropout_patch(dr, (qw0 + r) >> 2, ((s0 + 32 * b + 4 * h) >> 2) + 2 * (r & 3), b_ * p.H + h_);
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (MASKED && !use[b]) {
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[b][i] = -INFINITY;
        continue;
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[b][i] = 0.f;
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        vec8 a = as_vec8<T>(lds_read16(kt + k_off[ks] + b * 32 * C::ROWB));
        sacc[b] = T::mfma(a, qf[ks], sacc[b]);
      }
      if constexpr (SOFTCAP) {  // the cap comes first: masks and the running max act on the capped score
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[b][i] = sc.k2 * softcap_tanh(sc, sacc[b][i]);
      }
      if constexpr (ALIBI) {  // the bias comes before the masks and the running max; register i is key (i&3) + 8(i>>2) on
        const float qk = (float)(qw0 + r - s0 - 32 * b - 4 * h);  // from this lane's (query - key) of register 0
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[b][i] = alibi_add(alibi_k, qk - (float)((i & 3) + 8 * (i >> 2)), sacc[b][i]);
      }
      if constexpr (MASKED) {
        const int qrow = qw0 + r;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = s0 + 32 * b + (i & 3) + 8 * (i >> 2) + 4 * h;
          // (LOCAL: the left bound applies to the sequence's rows only -- local_tiles)
          const bool dead = (CAUSAL && key > qrow) || (LOCAL && (key > qrow + wr || (key < qrow - wl && qrow < Sq))) || key >= Sk;
          sacc[b][i] = dead ? -INFINITY : sacc[b][i];
        }
      }
    }
    // ---- online softmax (query on the lane) ----
    float tm0 = sacc[0][0], tm1 = sacc[1][0];
#pragma unroll
    for (int i = 1; i < 16; ++i) {
      tm0 = __builtin_fmaxf(tm0, sacc[0][i]);
      tm1 = __builtin_fmaxf(tm1, sacc[1][i]);
    }
    const float tm = half_max(__builtin_fmaxf(tm0, tm1));
    // Deferred rescale: the running max is only raised when some row's tile max exceeds it by
    // more than kDefer (in log2 units), so P stays <= 2^kDefer (exact in fp32, same RELATIVE
    // rounding in 16 bit) and the O-wide multiply is rare.  m = -inf (first tile) always fires.
    if (__builtin_amdgcn_ballot_w64(tm > m + defer_raw) != 0) {
      const float mn = __builtin_fmaxf(m, tm);
      // m = -inf -> 0; LOCAL: a row that has seen no key yet keeps m = mn = -inf (corr 0 on l = 0, O = 0, not NaN)
      const float corr = (LOCAL && mn == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((m - mn) * cs);
      l *= corr;
#pragma unroll
      for (int db = 0; db < C::DB; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[db][i] *= corr;
      m = mn;
      if constexpr (FOLD && !SOFTCAP) {
#pragma unroll
        for (int i = 0; i < 16; ++i) negm[i] = -mn;
      }
    }
    // LOCAL: a row with m = -inf has only dead (-inf) scores in this tile: offset 0 gives p = 0 instead of NaN
    const float mc = (LOCAL && m == -INFINITY) ? 0.f : m * cs;
    float ls[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float pe = __builtin_amdgcn_exp2f(LOG2 ? sacc[b][i] - mc : __builtin_fmaf(sacc[b][i], c2, -mc));
        sacc[b][i] = pe;
        ls[i & 3] += pe;
      }
    l += (ls[0] + ls[1]) + (ls[2] + ls[3]);
    if constexpr (DROP) {  // keep / drop each weight (the row sum above is the undropped one)
#pragma unroll
      for (int b = 0; b < 2; ++b)
        if (!(MASKED && !use[b])) drop_weights(sacc[b], mine[b]);
    }
    // ---- O^T += V^T P^T ----
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (MASKED && !use[b]) continue;
      const vec8 pf0 = pack8<T, 0>(sacc[b]);
      const vec8 pf1 = pack8<T, 1>(sacc[b]);
#pragma unroll
      for (int db = 0; db < C::DB; ++db) {
        const FA_LDS char* base = vt + b * 32 * C::ROWB;
        vec8 a0 = lds_read_tr_frag<T>(base + v_off[0][db], base + v_off[1][db]);
        oacc[db] = T::mfma(a0, pf0, oacc[db]);
        vec8 a1 = lds_read_tr_frag<T>(base + 16 * C::ROWB + v_off[0][db], base + 16 * C::ROWB + v_off[1][db]);
        oacc[db] = T::mfma(a1, pf1, oacc[db]);
      }
    }
  };

  // Unmasked tile with a LAZY running max: exponentiate against the stale row max -- no max reduction, no
  // cross-half exchange, no rescale test.  All p >= 0, so a lane's partial row sum bounds every p it holds: if
  // no partial sum exceeds kLazySumMax nothing can overflow (fp32 sums, 16-bit P fragments) and the stale max
  // is exactly as good as the true one (softmax is shift invariant).  Otherwise (always the first tile: m = -inf
  // gives p = +inf; afterwards only if scores jump by more than ~2^8) NOTHING has been committed: return false
  // and the caller redoes the tile on the exact path.
  // MASKED = true: the same for a tile on the causal diagonal or the ragged tail -- dead scores become -inf (p = 0),
  // key blocks no row of the wave can see are skipped.  A wave whose first visible tile is masked arrives here with
  // m = -inf, overflows by construction and takes the exact path once.
  // SOFTCAP: the same lazy path, reformulated for the capped score.  tanh has to act on the raw score, so the chain cannot
  // start from -m (FOLD's free subtraction): it starts at 0, and the exponent argument is cap*log2e * t - m, one fma
  // after the tanh.  The bail-out test is unchanged (it bounds p whatever the score).
  // ALIBI: the bias is one fma per score, last on the exponent argument with FOLD (the chain from -m is in log2 units),
  // on the raw score before the c2 fma without.  The bail-out test bounds p whatever the sign of the bias.
  auto tile_lazy = [&](int t, auto masked_tag) __attribute__((always_inline)) -> bool {
    constexpr bool MASKED = decltype(masked_tag)::value;
    const FA_LDS char* kt = smem + (t & 1) * C::TILE_BYTES;
    const FA_LDS char* vt = smem + (2 + (t & 1)) * C::TILE_BYTES;
    const int s0 = t * C::BN;
    bool use[2] = {true, true};
    if constexpr (MASKED) {
      if (CAUSAL) {
        use[0] = s0 <= qw0;
        use[1] = s0 + 32 <= qw0;
      }
      if (LOCAL) {  // the key block meets the band of some row of the wave
        use[0] = s0 <= qw0 + 31 + wr && s0 + 31 >= qw0 - wl;
        use[1] = s0 + 32 <= qw0 + 31 + wr && s0 + 63 >= qw0 - wl;
      }
      use[0] = use[0] && s0 < Sk;
      use[1] = use[1] && s0 + 32 < Sk;
      if (!use[0] && !use[1]) return true;  // nothing of this tile is visible to the wave
    }
    f32x16 sacc[2];
    u32x4 mine[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    if constexpr (DROP) {  // as in tile(): one Philox call per lane and key block, issued ahead of the MFMA chains
      const Dropout dr{p.drop.thresh, p.drop.seed_lo, p.drop.seed_hi, p.drop.offset, p.drop.rp};
#pragma unroll
      for (int b = 0; b < 2; ++b)
        if (!(MASKED && !use[b])) mine[b] = dropout_patch(dr, (qw0 + r) >> 2, ((s0 + 32 * b + 4 * h) >> 2) + 2 * (r & 3), b_ * p.H + h_);
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (MASKED && !use[b]) continue;
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[b][i] = (FOLD && !SOFTCAP) ? negm[i] : 0.f;
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        vec8 a = as_vec8<T>(lds_read16(kt + k_off[ks] + b * 32 * C::ROWB));
        sacc[b] = T::mfma(a, qf[ks], sacc[b]);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    const float mc = m * c2;
    float ls[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (MASKED && !use[b]) continue;
      const float qk = ALIBI ? (float)(qw0 + r - s0 - 32 * b - 4 * h) : 0.f;  // as in tile()
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if constexpr (ALIBI && !FOLD) sacc[b][i] = alibi_add(alibi_k, qk - (float)((i & 3) + 8 * (i >> 2)), sacc[b][i]);
        float x = SOFTCAP ? __builtin_fmaf(sc.k2, softcap_tanh(sc, sacc[b][i]), -m)
                          : (FOLD ? sacc[b][i] : __builtin_fmaf(sacc[b][i], c2, -mc));
        if constexpr (ALIBI && FOLD) x = alibi_add(alibi_k, qk - (float)((i & 3) + 8 * (i >> 2)), x);
        if constexpr (MASKED) {
          const int key = s0 + 32 * b + (i & 3) + 8 * (i >> 2) + 4 * h;
          const bool dead = (CAUSAL && key > qw0 + r) ||
                            (LOCAL && (key > qw0 + r + wr || (key < qw0 + r - wl && qw0 + r < Sq))) || key >= Sk;
          x = dead ? -INFINITY : x;
        }
        const float pe = __builtin_amdgcn_exp2f(x);
        sacc[b][i] = pe;
        ls[i & 3] += pe;
      }
    }
    const float lsum = (ls[0] + ls[1]) + (ls[2] + ls[3]);
    if (__builtin_amdgcn_ballot_w64(!(lsum <= kLazySumMax)) != 0) return false;
    l += lsum;
    if constexpr (DROP) {  // the row sum above is the undropped one; drop before P @ V
#pragma unroll
      for (int b = 0; b < 2; ++b)
        if (!(MASKED && !use[b])) drop_weights(sacc[b], mine[b]);
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (MASKED && !use[b]) continue;
      const vec8 pf0 = pack8<T, 0>(sacc[b]);
      const vec8 pf1 = pack8<T, 1>(sacc[b]);
#pragma unroll
      for (int db = 0; db < C::DB; ++db) {
        const FA_LDS char* base = vt + b * 32 * C::ROWB;
        vec8 a0 = lds_read_tr_frag<T>(base + v_off[0][db], base + v_off[1][db]);
        oacc[db] = T::mfma(a0, pf0, oacc[db]);
        vec8 a1 = lds_read_tr_frag<T>(base + 16 * C::ROWB + v_off[0][db], base + 16 * C::ROWB + v_off[1][db]);
        oacc[db] = T::mfma(a1, pf1, oacc[db]);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    return true;
  };

  using BR = std::integral_constant<int, -1>;

  // ---- main loop: one barrier per tile; every wave runs exactly ntiles iterations ----
  if (Sk % C::BN != 0) {  // a ragged last tile must not expose uninitialised LDS (out-of-range DMA may not write)
    lds_zero_fill(smem, C::LDS_BYTES, C::NT, tid);
    __syncthreads();
  }
  int t = t_begin;
  bool prefetched = false;
  if (!LOCAL || t < ntiles) {  // LOCAL: a workgroup whose band holds no key visits no tile (O = 0, LSE = -inf)
  if constexpr (LOCAL) {
    dma_tile(t, t & 1);
    tile_sync();
    // masked tiles on the band's left edge (LOCAL): lazy first, the exact path only if the stale max cannot be used
    for (; t < tf0; ++t) {
      if (t + 1 < ntiles) dma_tile(t + 1, (t + 1) & 1);
      if (!tile_lazy(t, std::true_type{})) tile(t, BR{}, std::true_type{});
      tile_sync();
    }
  } else {
    dma_tile(0, 0);
    tile_sync();  // tile 0 and the Q fragments landed
  }
  // Unmasked tiles: one exact tile (the first one, or the one a lazy tile bailed out of -- its prefetch is
  // then already issued), followed by lazy tiles until one bails out.  Separate loops on purpose: bodies that
  // merge control flow get their accumulators copied at every join.
  while (t < nfull) {
    if (!prefetched && t + 1 < ntiles) dma_tile(t + 1, (t + 1) & 1);
    tile(t, BR{}, std::false_type{});
    tile_sync();
    ++t;
    prefetched = false;
    for (; t < nfull; ++t) {
      if (t + 1 < ntiles) dma_tile(t + 1, (t + 1) & 1);
      if (!tile_lazy(t, std::false_type{})) {
        prefetched = true;
        break;
      }
      tile_sync();
    }
  }
  // masked tiles (causal diagonal, ragged tail): lazy first, the exact path only if the stale max cannot be used
  for (; t < ntiles; ++t) {
    if (!prefetched && t + 1 < ntiles) dma_tile(t + 1, (t + 1) & 1);
    prefetched = false;
    if (!tile_lazy(t, std::true_type{})) tile(t, BR{}, std::true_type{});
    tile_sync();
  }
  }  // tiles

  // ---- epilogue ----
  float lt = half_sum(l);
  // SINK: the sink is one more score of the row, met last: the usual max update folds exp(z - m) into the row sum and
  // rescales O through `onum`; it has no value row, so O gets nothing else.  z = -inf: mz = m, onum = exp2(0) = 1 and the
  // term is exp2(-inf) = 0, so lt, inv and the LSE below are the sink-less kernel's, bit for bit.  m = z = -inf (a row
  // with no visible key and no sink) is left alone: lt = 0, O = 0, LSE = -inf.  m = -inf with a finite z: lt = 1, O = 0,
  // LSE = z.
  float onum = DROP ? p.drop.rp : 1.0f;
  if constexpr (SINK) {
    const float mz = __builtin_fmaxf(m, sink_m);
    if (mz != -INFINITY) {
      onum = __builtin_amdgcn_exp2f((m - mz) * cs);
      lt = __builtin_fmaf(lt, onum, __builtin_amdgcn_exp2f((sink_m - mz) * cs));
      m = mz;
    }
  }
  // lt = 0 only for a variable-length sequence with queries but no keys (S_k = 0: no tile was visited): O = 0, LSE = -inf
  // DROP: O = (1 / (1 - p)) * sum(mask o P) V / l -- the rescale is linear, so it joins the normalisation here
  const float inv = lt > 0.f ? onum / lt : 0.f;
  // all waves are past the last barrier: the K/V buffers are free; wave w stages in its own 32*ROWB bytes
  store_tile_rows<D, T>(oacc, inv, smem + wave * 32 * C::ROWB, ro, qw0 * o_rs, lane, o_rs);
  if (h == 0) buf_store_f32(rl, (qw0 + r) * 4, m * (LOG2 ? kLn2 : p.scale) + __builtin_logf(lt));
  }  // pass
