// Body of the family-1 dQ kernels (fa_bwd_dq.hip), included inside fa_bwd_dq_kernel and fa_bwd_dq_mod_kernel (the window,
// GQA, soft-cap and ALiBi variants): the including kernel defines the template parameters, LOCAL, the window (wl, wr), GQA, the head
// group size `group`, SOFTCAP with the cap `softcap`, ALIBI with the slopes (`slopes`, `slopes_bstride`) and the
// parameter block p.  Shared as text rather than
// through a device function so that the plain kernels compile exactly as they did before the window existed.
  using C = DqCfg<D>;
  using vec8 = typename T::vec8;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  FA_LDS char* smem = (FA_LDS char*)smem_raw;

  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);

  // work list (fa_kernels.h tile_index): causal workgroups take the query-tile pair (nq-1-i, i) -> equal work everywhere
  const TileIndex<CAUSAL> tw = tile_index<CAUSAL>(p, p.n_tiles);
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
  if (pass) __syncthreads();  // the previous pass staged its dQ tile in the K/V buffers

  // Q, K, V, dO may be strided views with a contiguous head dim (fa_fwd.hip); O and dQ carry their own layouts
  // (contiguous for the reference's launch, packed rows for varlen); LSE / delta rows of one (batch, head) are contiguous
  const int q_rs = p.lq.rs, do_rs = p.ldo.rs, kv_rs = p.lk.rs, o_rs = p.lo.rs, dq_rs = p.ldq.rs;
  const __amdgpu_buffer_rsrc_t rq = make_rsrc(
      (const char*)p.q + b_ * p.lq.sb + h_ * p.lq.sh + (long long)si.q0 * q_rs, (unsigned)(Sq - 1) * q_rs + C::ROWB);
  const __amdgpu_buffer_rsrc_t rdo = make_rsrc(
      (const char*)p.dout + b_ * p.ldo.sb + h_ * p.ldo.sh + (long long)si.q0 * do_rs, (unsigned)(Sq - 1) * do_rs + C::ROWB);
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(
      (const char*)p.o + b_ * p.lo.sb + h_ * p.lo.sh + (long long)si.q0 * o_rs, (unsigned)(Sq - 1) * o_rs + C::ROWB);
  const __amdgpu_buffer_rsrc_t rdq = make_rsrc(
      (char*)p.dq + b_ * p.ldq.sb + h_ * p.ldq.sh + (long long)si.q0 * dq_rs, (unsigned)(Sq - 1) * dq_rs + C::ROWB);
  const __amdgpu_buffer_rsrc_t rk = make_rsrc(
      (const char*)p.k + b_ * p.lk.sb + hk_ * p.lk.sh + (long long)si.k0 * kv_rs, view_bytes(Sk, kv_rs, C::ROWB));
  const __amdgpu_buffer_rsrc_t rv = make_rsrc(
      (const char*)p.v + b_ * p.lv.sb + hk_ * p.lv.sh + (long long)si.k0 * kv_rs, view_bytes(Sk, kv_rs, C::ROWB));
  const long long rowc_off = b_ * p.lse_sb + h_ * p.lse_sh + si.q0;
  const __amdgpu_buffer_rsrc_t rl = make_rsrc(p.lse + rowc_off, (unsigned)Sq * 4);
  const __amdgpu_buffer_rsrc_t rd = make_rsrc(p.delta + rowc_off, (unsigned)Sq * 4);


  // ---- resident B operands: Q^T and dO^T of this wave's 32 rows; delta ----
  vec8 qf[C::KS], dof[C::KS];
  float dsum = 0.f;
#pragma unroll
  for (int ks = 0; ks < C::KS; ++ks) {
    const int col = (2 * ks + h) * 16;
    qf[ks] = as_vec8<T>(buf_load16(rq, (qw0 + r) * q_rs + col));
    dof[ks] = as_vec8<T>(buf_load16(rdo, (qw0 + r) * do_rs + col));
    const vec8 of = as_vec8<T>(buf_load16(ro, (qw0 + r) * o_rs + col));
#pragma unroll
    for (int j = 0; j < 8; ++j) dsum = __builtin_fmaf((float)dof[ks][j], (float)of[j], dsum);
  }
  const float delta = half_sum(dsum);
  float nl = -buf_load_f32(rl, (qw0 + r) * 4) * kLog2e;
  if (LOCAL && nl == INFINITY) nl = -INFINITY;  // LSE = -inf: every P of the row is exp2(-inf) = 0
  if (h == 0) buf_store_f32(rd, (qw0 + r) * 4, delta);
  // Both MFMA chains START from a block holding this lane's (= query row's) constant: with Q pre-scaled by
  // softmax_scale*log2(e) the first delivers the exponent argument s*c2 - LSE*log2e, the second dP - delta,
  // and no per-element fma / subtract is left in the hot loop.
  f32x16 ndelta, nlse;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    ndelta[i] = -delta;
    nlse[i] = (T::kFoldScale && !SOFTCAP) ? nl : 0.f;
  }
  const float c2 = p.scale * kLog2e;
  constexpr bool FOLD = T::kFoldScale;  // fa_common.h
  // SOFTCAP (fa_fwd_body.inc): tanh acts on the raw score, so the score chain starts at 0 instead of -LSE*log2e; per
  // element t = tanh(y), P = exp2(cap*log2e * t - LSE*log2e) and dS = P o (dP - delta) o (1 - t^2) before the rounding
  const SoftCap sc = SOFTCAP ? make_softcap(softcap, FOLD ? 1.0f / (softcap * kLog2e) : p.scale / softcap) : SoftCap{0.f, 0.f};
  // ALIBI (fa_fwd_body.inc): P is recomputed with the bias in log2 units (slope * log2e), last on the exponent argument
  // (fp16) or in the block the score chain starts from (FOLD, below); dS = P o (dP - delta) needs nothing else, the bias
  // does not depend on Q or K
  const float alibi_k = ALIBI ? alibi_slope(slopes, b_ * slopes_bstride + h_, kLog2e) : 0.f;
  if constexpr (FOLD) {
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) qf[ks] = scale_frag<T>(qf[ks], c2);
  }

  const int kv_end = CAUSAL ? min(Sk, q0_wg + C::BM) : Sk;
  // LOCAL (fa_fwd.hip): tiles [t_begin, ntiles) meet the workgroup's band, [tf0, nfull) need no mask for this wave
  const LocalTiles lt_ = LOCAL ? local_tiles<C::BN>(q0_wg, min(q0_wg + C::BM, Sq) - 1, qw0, Sk, wl, wr) : LocalTiles{};
  const int t_begin = LOCAL ? lt_.begin : 0, tf0 = LOCAL ? lt_.full0 : 0;
  const int ntiles = LOCAL ? lt_.end : (kv_end + C::BN - 1) / C::BN;
  const int nfull = LOCAL ? lt_.full1 : (CAUSAL ? min(Sk / C::BN, qw0 / C::BN) : Sk / C::BN);

  // LDS-DMA source offsets (fa_common.h): wave w fills rows [16w, 16w+16) of each tile
  constexpr int RPI = 1024 / C::ROWB;  // rows per piece; dma_pieces: the immediate offset 1024 i of piece i is taken out
  int dma_src[C::DMA_PER_MAT];
#pragma unroll
  for (int i = 0; i < C::DMA_PER_MAT; ++i) dma_src[i] = dma_src_off<D>(16 * wave + RPI * i, lane, kv_rs) - 1024 * i;
  int row_off[C::KS];  // A-operand row reads (K rows and V rows)
#pragma unroll
  for (int ks = 0; ks < C::KS; ++ks) row_off[ks] = lds_off<D>(r, 2 * ks + h);
  int tr_off[2][C::DB];  // transposed reads of K
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int db = 0; db < C::DB; ++db) tr_off[e][db] = tr_lane_off<D>(lane, 8 * e, db);

  f32x16 dqacc[C::DB];
#pragma unroll
  for (int db = 0; db < C::DB; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) dqacc[db][i] = 0.f;

  auto dma_tile = [&](int t, int buf) __attribute__((always_inline)) {
    const int soff = t * C::BN * kv_rs;
    const int dst0 = buf * C::TILE_BYTES + 16 * wave * C::ROWB;  // this wave's 16 rows = DMA_PER_MAT consecutive KiB
    dma_pieces<C::DMA_PER_MAT>(rk, lds_addr_of(smem + dst0), dma_src, soff);
    dma_pieces<C::DMA_PER_MAT>(rv, lds_addr_of(smem + 2 * C::TILE_BYTES + dst0), dma_src, soff);
  };

  // BUF: the tile's ring buffer as a compile-time constant (0 / 1), or -1 = t & 1 at run time.  With a constant buffer every
  // LDS address of the tile is `per-lane offset + immediate`; with t & 1 hipcc rebuilds them with vector adds per read
  // (D = 128: 3.6 vector instructions per MFMA where the maths needs 1.7, profiles/r04_pmc_summary_d128.txt).
  auto tile = [&](int t, auto masked_tag, auto buf_tag) __attribute__((always_inline)) {
    constexpr bool MASKED = decltype(masked_tag)::value;
    constexpr int BUF = decltype(buf_tag)::value;
    const int bsel = BUF >= 0 ? BUF : (t & 1);
    const FA_LDS char* kt = smem + bsel * C::TILE_BYTES;
    const FA_LDS char* vt = smem + (2 + bsel) * C::TILE_BYTES;
    const int s0 = t * C::BN;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if constexpr (MASKED) {
        bool use = s0 + 32 * b < Sk;
        if (CAUSAL) use = use && (s0 + 32 * b <= qw0);
        if (LOCAL) use = use && s0 + 32 * b <= qw0 + 31 + wr && s0 + 32 * b + 31 >= qw0 - wl;
        if (!use) continue;
      }
      const FA_LDS char* kbp = kt + b * 32 * C::ROWB;
      const FA_LDS char* vbp = vt + b * 32 * C::ROWB;
      f32x16 sacc = nlse, pacc = ndelta;
      // ALIBI: (query - key) of register 0, from a fresh lane id (fa_common.h lane_id_now), as r and h are not kept live
      // across the tile loop.  With FOLD the bias joins the block the score chain starts from, fma(k, -|d|, -LSE*log2e):
      // added last on the exponent argument instead, it needs the 16-register block nlse live across the loop as well,
      // and the D = 128 kernel spills 7 VGPRs.  k = 0 still gives the unbiased chain bit for bit.
      int ln = 0;
      if constexpr (ALIBI) ln = lane_id_now();
      const float qk = ALIBI ? (float)(qw0 + (ln & 31) - s0 - 32 * b - 4 * (ln >> 5)) : 0.f;
      if constexpr (ALIBI && FOLD) {
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[i] = alibi_add(alibi_k, qk - (float)((i & 3) + 8 * (i >> 2)), nl);
      }
      if constexpr (DROP) {
#pragma unroll
        for (int i = 0; i < 16; ++i) pacc[i] = 0.f;
      }
      // DROP: one Philox call per lane and block -- lane j of a quad generates patch g = j for the quad's four rows
      // (fa_common.h quad_bcast); issued here so that its ~100 integer ops run beside the MFMA chains below
      u32x4 mine = {0, 0, 0, 0};
      if constexpr (DROP) {
        const Dropout dr{p.drop.thresh, p.drop.seed_lo, p.drop.seed_hi, p.drop.offset, p.drop.rp};
        mine = dropout_patch(dr, (qw0 + r) >> 2, ((s0 + 32 * b + 4 * h) >> 2) + 2 * (r & 3), b_ * p.H + h_);
      }
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        vec8 a = as_vec8<T>(lds_read16(kbp + row_off[ks]));
        sacc = T::mfma(a, qf[ks], sacc);
      }
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        vec8 a = as_vec8<T>(lds_read16(vbp + row_off[ks]));
        pacc = T::mfma(a, dof[ks], pacc);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float tc = SOFTCAP ? softcap_tanh(sc, sacc[i]) : 0.f;
        float x = SOFTCAP ? __builtin_fmaf(sc.k2, tc, nl) : (FOLD ? sacc[i] : __builtin_fmaf(sacc[i], c2, nl));
        if constexpr (ALIBI && !FOLD) x = alibi_add(alibi_k, qk - (float)((i & 3) + 8 * (i >> 2)), x);
        if constexpr (MASKED) {
          const int key = s0 + 32 * b + (i & 3) + 8 * (i >> 2) + 4 * h;
          const bool dead = (CAUSAL && key > qw0 + r) || (LOCAL && (key > qw0 + r + wr || key < qw0 + r - wl)) || key >= Sk;
          x = dead ? -INFINITY : x;
        }
        if constexpr (SOFTCAP) sacc[i] = __builtin_amdgcn_exp2f(x) * (pacc[i] * __builtin_fmaf(-tc, tc, 1.0f));
        else if constexpr (!DROP) sacc[i] = __builtin_amdgcn_exp2f(x) * pacc[i];  // dS^T = P^T o (dP^T - delta)
        else sacc[i] = __builtin_amdgcn_exp2f(x);                             // P^T; the mask comes next
      }
      if constexpr (DROP) {
        const Dropout dr{p.drop.thresh, p.drop.seed_lo, p.drop.seed_hi, p.drop.offset, p.drop.rp};
        const int qrow = qw0 + r;
        auto apply = [&](auto g_tag) __attribute__((always_inline)) {
          constexpr int g = decltype(g_tag)::value;
          const unsigned w = select_word(quad_bcast4<g>(mine), qrow & 3);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int i = 4 * g + j;
            const bool keep = ((w >> (8 * j)) & 255u) >= dr.thresh;
            // dS = P o (dP - delta) with dP = mask / (1 - p) o (dO V^T): one fma, one select, one multiply
            const float t = __builtin_fmaf(pacc[i], dr.rp, -delta);
            sacc[i] = sacc[i] * (keep ? t : -delta);
          }
        };
        apply(std::integral_constant<int, 0>{});
        apply(std::integral_constant<int, 1>{});
        apply(std::integral_constant<int, 2>{});
        apply(std::integral_constant<int, 3>{});
      }
      const vec8 d0 = pack8<T, 0>(sacc);
      const vec8 d1 = pack8<T, 1>(sacc);
#pragma unroll
      for (int db = 0; db < C::DB; ++db) {
        vec8 a0 = lds_read_tr_frag<T>(kbp + tr_off[0][db], kbp + tr_off[1][db]);
        dqacc[db] = T::mfma(a0, d0, dqacc[db]);
        vec8 a1 = lds_read_tr_frag<T>(kbp + 16 * C::ROWB + tr_off[0][db], kbp + 16 * C::ROWB + tr_off[1][db]);
        dqacc[db] = T::mfma(a1, d1, dqacc[db]);
      }
    }
  };

  if (Sk % C::BN != 0) {  // a ragged last tile must not expose uninitialised LDS
    lds_zero_fill(smem, C::LDS_BYTES, C::NT, tid);
    __syncthreads();
  }
  using BR = std::integral_constant<int, -1>;
  int t = t_begin;
  if (!LOCAL || t < ntiles) {  // LOCAL: a workgroup whose band holds no key visits no tile (dQ = 0)
  if constexpr (LOCAL) {
    dma_tile(t, t & 1);
    tile_sync();
    for (; t < tf0; ++t) {  // masked tiles on the band's left edge
      if (t + 1 < ntiles) dma_tile(t + 1, (t + 1) & 1);
      tile(t, std::true_type{}, BR{});
      tile_sync();
    }
    if (D == 128 && (t & 1) && t < nfull) {  // the constant-buffer pairs below start on an even tile
      if (t + 1 < ntiles) dma_tile(t + 1, (t + 1) & 1);
      tile(t, std::false_type{}, BR{});
      tile_sync();
      ++t;
    }
  } else {
    dma_tile(0, 0);
    tile_sync();
  }
  if constexpr (D == 128 && !DROP) {   // two tiles per trip, constant buffers (the first tile of a pass is tile 0: buffer 0)
    for (; t + 2 <= nfull; t += 2) {
      dma_tile(t + 1, 1);
      tile(t, std::false_type{}, std::integral_constant<int, 0>{});
      tile_sync();
      if (t + 2 < ntiles) dma_tile(t + 2, 0);
      tile(t + 1, std::false_type{}, std::integral_constant<int, 1>{});
      tile_sync();
    }
  }
  for (; t < nfull; ++t) {
    if (t + 1 < ntiles) dma_tile(t + 1, (t + 1) & 1);
    tile(t, std::false_type{}, BR{});
    tile_sync();
  }
  for (; t < ntiles; ++t) {
    if (t + 1 < ntiles) dma_tile(t + 1, (t + 1) & 1);
    tile(t, std::true_type{}, BR{});
    tile_sync();
  }
  }  // tiles

  if constexpr (FOLD) {
    if (p.qs) {  // workspace for the dK/dV launch: the scaled rows exactly as this kernel (and the forward) multiplied
                 // them; stored here, not in the prologue, where the first tile's vmcnt(0) would wait for them
      const __amdgpu_buffer_rsrc_t rqs = make_rsrc(
          (char*)p.qs + b_ * p.lqs.sb + h_ * p.lqs.sh + (long long)si.q0 * p.lqs.rs, (unsigned)(Sq - 1) * p.lqs.rs + C::ROWB);
      const int ln = lane_id_now();  // re-derived: nothing lane-dependent is kept live across the tile loop for this
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks)
        buf_store16(rqs, (qw0 + (ln & 31)) * p.lqs.rs + (2 * ks + (ln >> 5)) * 16, __builtin_bit_cast(u32x4, qf[ks]));
    }
  }
  store_tile_rows<D, T>(dqacc, p.scale, smem + wave * 32 * C::ROWB, rdq, qw0 * dq_rs, lane, dq_rs);
  }  // pass
