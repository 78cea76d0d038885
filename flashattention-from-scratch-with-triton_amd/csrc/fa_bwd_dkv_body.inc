// Body of the family-1 dK/dV kernels (fa_bwd_dkv.hip), included inside fa_bwd_dkv_kernel and fa_bwd_dkv_mod_kernel (the
// window, GQA, soft-cap and ALiBi variants): the including kernel defines the template parameters, LOCAL, the window (wl, wr),
// GQA, the head group size `group`, SOFTCAP with the cap `softcap`, ALIBI with the slopes (`slopes`, `slopes_bstride`)
// and the parameter block p.  Shared as text rather than
// through a device function so that the plain kernels compile exactly as they did before the window existed.
  using C = DkvCfg<D>;
  using vec8 = typename T::vec8;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  FA_LDS char* smem = (FA_LDS char*)smem_raw;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;

  // work list (fa_kernels.h tile_index): causal workgroups take the key-tile pair (i, nk-1-i)
  // GQA: the slices are (batch, K/V head); h_ is the K/V head and the workgroup visits query heads h_ * group + [0, group)
  const TileIndex<CAUSAL> tw = tile_index<CAUSAL>(p, p.n_tiles);
  const BatchHead ix = batch_head(tw.bh, p.B, GQA ? p.H / group : p.H, p.vl.cu_q != nullptr);
  const int b_ = ix.b, h_ = ix.h;
  const SeqInfo si = seq_info(p.vl, b_, p.Sq, p.Sk);
  const int Sq = si.Sq, Sk = si.Sk;
  const int nk = (Sk + C::BK - 1) / C::BK;
  const bool paired_ = tw.paired();
  const int idx = tw.idx;
  if (idx >= (paired_ ? (nk + 1) / 2 : nk)) return;
  const int npass = (paired_ && idx != nk - 1 - idx) ? 2 : 1;
  for (int pass = 0; pass < npass; ++pass) {
  const int kt_idx = (paired_ ? (pass == 0 ? idx : nk - 1 - idx) : idx);  // low key tiles are the heavy ones
  const int k0_wg = kt_idx * C::BK;
  const int kw0 = k0_wg + wave * 32;
  if (pass) __syncthreads();  // the previous pass staged dK / dV in the tile buffers

  // Q, K, V, dO may be strided views with a contiguous head dim (fa_fwd.hip); dK and dV carry their own layouts
  // (contiguous for the reference's launch, packed rows for varlen); LSE / delta rows of one (batch, head) are contiguous
  const int q_rs = p.lq.rs, do_rs = p.ldo.rs, kv_rs = p.lk.rs, dk_rs = p.ldk.rs, dv_rs = p.ldv.rs;
  // Q, dO and the LSE / delta rows belong to a query head: GQA rebuilds them at each head of the group (hq0 + gi)
  const int hq0 = GQA ? h_ * group : h_;
  __amdgpu_buffer_rsrc_t rq = make_rsrc(
      (const char*)p.q + b_ * p.lq.sb + hq0 * p.lq.sh + (long long)si.q0 * q_rs, (unsigned)(Sq - 1) * q_rs + C::ROWB);
  __amdgpu_buffer_rsrc_t rdo = make_rsrc(
      (const char*)p.dout + b_ * p.ldo.sb + hq0 * p.ldo.sh + (long long)si.q0 * do_rs, (unsigned)(Sq - 1) * do_rs + C::ROWB);
  const __amdgpu_buffer_rsrc_t rk = make_rsrc(
      (const char*)p.k + b_ * p.lk.sb + h_ * p.lk.sh + (long long)si.k0 * kv_rs, (unsigned)(Sk - 1) * kv_rs + C::ROWB);
  const __amdgpu_buffer_rsrc_t rv = make_rsrc(
      (const char*)p.v + b_ * p.lv.sb + h_ * p.lv.sh + (long long)si.k0 * kv_rs, (unsigned)(Sk - 1) * kv_rs + C::ROWB);
  const __amdgpu_buffer_rsrc_t rdk = make_rsrc(
      (char*)p.dk + b_ * p.ldk.sb + h_ * p.ldk.sh + (long long)si.k0 * dk_rs, (unsigned)(Sk - 1) * dk_rs + C::ROWB);
  const __amdgpu_buffer_rsrc_t rdv = make_rsrc(
      (char*)p.dv + b_ * p.ldv.sb + h_ * p.ldv.sh + (long long)si.k0 * dv_rs, (unsigned)(Sk - 1) * dv_rs + C::ROWB);
  // Row constants of a query tile: wave 0 loads its LSE rows, wave 1 its delta rows, through ONE wave-uniform
  // descriptor and an unconditional load (a divergent `if` around the load makes hipcc wait vmcnt(0) at the merge,
  // which also waits for the tile DMA issued just before: the double buffer then hides nothing).
  const long long rowc_off = b_ * p.lse_sb + hq0 * p.lse_sh + si.q0;
  __amdgpu_buffer_rsrc_t rrc = make_rsrc((wave == 0 ? p.lse : p.delta) + rowc_off, wave < 2 ? (unsigned)Sq * 4 : 0u);

  const float c2 = p.scale * kLog2e;
  constexpr bool FOLD = T::kFoldScale;  // fa_common.h: the score chain starts from -LSE*log2e and K carries c2
  // SOFTCAP (fa_bwd_dq_body.inc): the score chain starts at 0 and the row constant is added after the tanh; the scores
  // are in log2 units with FOLD (K * c2, or the dQ launch's Q * c2 with q_prescaled), raw without
  const SoftCap sc = SOFTCAP ? make_softcap(softcap, FOLD ? 1.0f / (softcap * kLog2e) : p.scale / softcap) : SoftCap{0.f, 0.f};
  // ALIBI (fa_bwd_dq_body.inc): slope * log2e of the query head being visited (hq0 + gi in the GQA head loop)
  float alibi_k = ALIBI ? alibi_slope(slopes, b_ * slopes_bstride + hq0, kLog2e) : 0.f;
  // ---- resident B operands: K^T and V^T of this wave's 32 keys ----
  vec8 kf[C::KS], vf[C::KS];
#pragma unroll
  for (int ks = 0; ks < C::KS; ++ks) {
    const int off = (kw0 + r) * kv_rs + (2 * ks + h) * 16;
    kf[ks] = as_vec8<T>(buf_load16(rk, off));
    if (FOLD && !p.q_prescaled) kf[ks] = scale_frag<T>(kf[ks], c2);  // K * softmax_scale * log2(e)
    vf[ks] = as_vec8<T>(buf_load16(rv, off));
  }

  // LOCAL: the keys' band is queries [k0_wg - wr, k_last + wl] (local_tiles with the two sides swapped): tiles
  // [t_start, ntiles) meet it, [t_full, t_full_end) need no mask -- every row of the tile sees every key of this wave
  const LocalTiles lt_ = LOCAL ? local_tiles<C::BQ>(k0_wg, min(k0_wg + C::BK, Sk) - 1, kw0, Sq, wr, wl) : LocalTiles{};
  const int ntiles = LOCAL ? lt_.end : (Sq + C::BQ - 1) / C::BQ;
  const int t_start = LOCAL ? lt_.begin : (CAUSAL ? k0_wg / C::BQ : 0);
  // tiles t >= t_full are entirely below the diagonal for this wave's keys
  const int t_full = LOCAL ? lt_.full0 : (CAUSAL ? kw0 / C::BQ + 1 : 0);
  const int t_full_end = LOCAL ? lt_.full1 : 0;

  // LDS-DMA source offsets (fa_common.h): wave w fills rows [16w, 16w+16) of each tile, one dma16 per piece
  constexpr int RPI = 1024 / C::ROWB;
  int dma_src[C::DMA_PER_MAT];
#pragma unroll
  for (int i = 0; i < C::DMA_PER_MAT; ++i) dma_src[i] = dma_src_off<D>(16 * wave + RPI * i, lane, q_rs);
  // the dO tile has the same lane -> (row, chunk) map; only its row stride may differ (the difference can be
  // negative: it is added in the VGPR offset, whose sum row*do_rs + chunk is not; the scalar offset is unsigned)
  const int do_delta = (16 * wave + lane / C::CPR) * (do_rs - q_rs);
  int row_off[C::KS];
#pragma unroll
  for (int ks = 0; ks < C::KS; ++ks) row_off[ks] = lds_off<D>(r, 2 * ks + h);
  int tr_off[2][C::DB];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int db = 0; db < C::DB; ++db) tr_off[e][db] = tr_lane_off<D>(lane, 8 * e, db);

  f32x16 dkacc[C::DB], dvacc[C::DB];
#pragma unroll
  for (int db = 0; db < C::DB; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      dkacc[db][i] = 0.f;
      dvacc[db][i] = 0.f;
    }

  float cst = 0.f;  // threads 0..63: LSE row, 64..127: delta row
  auto stage_load = [&](int t) __attribute__((always_inline)) {
    const int soff_q = t * C::BQ * q_rs, soff_do = t * C::BQ * do_rs;
    const int buf = t & 1;
#pragma unroll
    for (int i = 0; i < C::DMA_PER_MAT; ++i) {
      const int dst = buf * C::TILE_BYTES + (16 * wave + RPI * i) * C::ROWB;
      dma16(rq, lds_addr_of(smem + dst), dma_src[i], soff_q);
      dma16(rdo, lds_addr_of(smem + 2 * C::TILE_BYTES + dst), dma_src[i] + do_delta + RPI * i * (do_rs - q_rs), soff_do);
    }
    cst = buf_load_f32(rrc, (t * C::BQ + lane) * 4);
  };
  // tile t (fetched during the previous step) has landed: publish its pre-scaled row constants, then meet
  auto stage_write = [&](int t) __attribute__((always_inline)) {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(waitcnt_imm(0));
    FA_LDS float* rc = (FA_LDS float*)(smem + C::ROWC_OFF + (t & 1) * C::ROWC_BYTES);
    // rows past S_q must give P = 0 (K:355-356): exp2(-inf) = 0
    // LOCAL: so do rows with LSE = -inf (no visible key)
    const float lse_c = (t * C::BQ + lane < Sq && !(LOCAL && cst == -INFINITY)) ? -cst * kLog2e : -INFINITY;
    if (wave < 2) rc[tid] = wave == 0 ? lse_c : -cst;  // rc[row] = -LSE*log2e, rc[64 + row] = -delta
  };

  auto tile = [&](int t, auto masked_tag) __attribute__((always_inline)) {
    constexpr bool MASKED = decltype(masked_tag)::value;
    const int buf = t & 1;
    const FA_LDS char* qt = smem + buf * C::TILE_BYTES;
    const FA_LDS char* dt = smem + (2 + buf) * C::TILE_BYTES;
    const FA_LDS char* rc = smem + C::ROWC_OFF + buf * C::ROWC_BYTES;
    const int q0 = t * C::BQ;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int qb0 = q0 + 32 * b;
      if constexpr (MASKED) {
        if (!LOCAL && qb0 < kw0) continue;  // every row of the block is above the diagonal
        if (LOCAL && (qb0 + 31 < kw0 - wr || qb0 > kw0 + 31 + wl)) continue;  // no row of the block meets the band
      }
      const FA_LDS char* qbp = qt + b * 32 * C::ROWB;
      const FA_LDS char* dbp = dt + b * 32 * C::ROWB;
      // per-register row constants: reg i <-> row (i&3) + 8(i>>2) + 4h
      // both MFMA chains START from them: with K pre-scaled the first delivers s*c2 - LSE*log2e, the second dP - delta
      f32x16 nl, nd, pacc, sacc;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 a = *(const FA_LDS f32x4*)(rc + (32 * b + 8 * g + 4 * h) * 4);
        const f32x4 d = *(const FA_LDS f32x4*)(rc + (64 + 32 * b + 8 * g + 4 * h) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          nl[4 * g + j] = a[j];
          nd[4 * g + j] = d[j];
          sacc[4 * g + j] = (FOLD && !SOFTCAP) ? a[j] : 0.f;
          pacc[4 * g + j] = DROP ? 0.f : d[j];
        }
      }
      // DROP: one Philox call per lane and block -- registers 4g..4g+3 are query rows qb0 + 8g + 4h + 0..3 of key kw0 + r,
      // i.e. byte (key & 3) of the four words of patch g, and the quad's four lanes (four consecutive keys) need the same
      // four patches: lane j generates patch g = j (fa_common.h quad_bcast).  Issued here, beside the MFMA chains.
      u32x4 mine = {0, 0, 0, 0};
      if constexpr (DROP) {
        const Dropout dr{p.drop.thresh, p.drop.seed_lo, p.drop.seed_hi, p.drop.offset, p.drop.rp};
        mine = dropout_patch(dr, ((qb0 + 4 * h) >> 2) + 2 * (r & 3), (kw0 + r) >> 2, b_ * p.H + h_);
      }
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        vec8 a = as_vec8<T>(lds_read16(qbp + row_off[ks]));
        sacc = T::mfma(a, kf[ks], sacc);
      }
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        vec8 a = as_vec8<T>(lds_read16(dbp + row_off[ks]));
        pacc = T::mfma(a, vf[ks], pacc);
      }
      // ALIBI: (query - key) of register 0; register i is (i&3) + 8(i>>2) query rows further down
      const float qk = ALIBI ? (float)(qb0 + 4 * h - kw0 - r) : 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float tc = SOFTCAP ? softcap_tanh(sc, sacc[i]) : 0.f;
        float x = SOFTCAP ? __builtin_fmaf(sc.k2, tc, nl[i]) : (FOLD ? sacc[i] : __builtin_fmaf(sacc[i], c2, nl[i]));
        if constexpr (ALIBI) x = alibi_add(alibi_k, qk + (float)((i & 3) + 8 * (i >> 2)), x);
        if constexpr (MASKED) {
          const int qrow = qb0 + (i & 3) + 8 * (i >> 2) + 4 * h;
          if (!LOCAL) x = (kw0 + r > qrow) ? -INFINITY : x;
          if (LOCAL) x = (qrow < kw0 + r - wr || qrow > kw0 + r + wl) ? -INFINITY : x;
        }
        const float pe = __builtin_amdgcn_exp2f(x);
        sacc[i] = pe;             // P
        if constexpr (SOFTCAP) pacc[i] = pe * (pacc[i] * __builtin_fmaf(-tc, tc, 1.0f));   // dS = P o (dP - delta) o (1 - t^2)
        else if constexpr (!DROP) pacc[i] = pe * pacc[i];   // dS = P o (dP - delta)
      }
      if constexpr (DROP) {
        const Dropout dr{p.drop.thresh, p.drop.seed_lo, p.drop.seed_hi, p.drop.offset, p.drop.rp};
        const int key = kw0 + r;
        auto apply = [&](auto g_tag) __attribute__((always_inline)) {
          constexpr int g = decltype(g_tag)::value;
          const u32x4 patch = quad_bcast4<g>(mine);
#pragma unroll
          for (int j = 0; j < 4; ++j) {   // register 4g + j <-> query 4*qg + j: word j of the patch, byte key & 3
            const int i = 4 * g + j;
            const bool keep = ((patch[j] >> (8 * (key & 3))) & 255u) >= dr.thresh;
            const float pe = sacc[i];
            // dS = P o (dP - delta) with dP = mask / (1 - p) o (dO V^T): one fma, one select, one multiply
            const float t = __builtin_fmaf(pacc[i], dr.rp, nd[i]);
            pacc[i] = pe * (keep ? t : nd[i]);
            sacc[i] = keep ? pe : 0.f;                         // dropped P for dV (its 1 / (1 - p) is applied once, to dV)
          }
        };
        apply(std::integral_constant<int, 0>{});
        apply(std::integral_constant<int, 1>{});
        apply(std::integral_constant<int, 2>{});
        apply(std::integral_constant<int, 3>{});
      }
      const vec8 p0 = pack8<T, 0>(sacc), p1 = pack8<T, 1>(sacc);
      const vec8 s0 = pack8<T, 0>(pacc), s1 = pack8<T, 1>(pacc);
#pragma unroll
      for (int db = 0; db < C::DB; ++db) {
        vec8 a0 = lds_read_tr_frag<T>(dbp + tr_off[0][db], dbp + tr_off[1][db]);
        dvacc[db] = T::mfma(a0, p0, dvacc[db]);
        vec8 a1 = lds_read_tr_frag<T>(dbp + 16 * C::ROWB + tr_off[0][db], dbp + 16 * C::ROWB + tr_off[1][db]);
        dvacc[db] = T::mfma(a1, p1, dvacc[db]);
      }
#pragma unroll
      for (int db = 0; db < C::DB; ++db) {
        vec8 a0 = lds_read_tr_frag<T>(qbp + tr_off[0][db], qbp + tr_off[1][db]);
        dkacc[db] = T::mfma(a0, s0, dkacc[db]);
        vec8 a1 = lds_read_tr_frag<T>(qbp + 16 * C::ROWB + tr_off[0][db], qbp + 16 * C::ROWB + tr_off[1][db]);
        dkacc[db] = T::mfma(a1, s1, dkacc[db]);
      }
    }
  };

  if (Sq % C::BQ != 0) {  // a ragged last query tile must not expose uninitialised LDS
    lds_zero_fill(smem, C::LDS_BYTES, C::NT, tid);
    __syncthreads();
  }
  // GQA: the group's query heads in ascending order, one after the other through the same tile band (it depends on the
  // keys only), into the same fp32 accumulators.  Each head starts its own double-buffer prologue: the previous head's
  // last tile ended with a barrier, so both buffers are free.  The loop exists in the GQA kernel's text only
  // (FA_DKV_HEAD_LOOP): even a one-trip loop changes the plain kernels' register allocation.
#ifdef FA_DKV_HEAD_LOOP
  for (int gi = 0; gi < group; ++gi) {
  if (gi) {  // as rq, rdo, rrc above, for query head hq0 + gi
    const int hq = hq0 + gi;
    rq = make_rsrc((const char*)p.q + b_ * p.lq.sb + hq * p.lq.sh + (long long)si.q0 * q_rs, (unsigned)(Sq - 1) * q_rs + C::ROWB);
    rdo = make_rsrc((const char*)p.dout + b_ * p.ldo.sb + hq * p.ldo.sh + (long long)si.q0 * do_rs,
                    (unsigned)(Sq - 1) * do_rs + C::ROWB);
    rrc = make_rsrc((wave == 0 ? p.lse : p.delta) + (rowc_off + (long long)gi * p.lse_sh), wave < 2 ? (unsigned)Sq * 4 : 0u);
    if constexpr (ALIBI) alibi_k = alibi_slope(slopes, b_ * slopes_bstride + hq, kLog2e);  // the slope changes with the query head
  }
#endif
  if (t_start < ntiles) {
    stage_load(t_start);
    stage_write(t_start);
  }
  __syncthreads();
  int t = t_start;
  const int t_masked_end = min(ntiles, t_full);
  for (; t < t_masked_end; ++t) {
    const bool more = t + 1 < ntiles;
    if (more) stage_load(t + 1);
    tile(t, std::true_type{});
    if (more) stage_write(t + 1);
    __syncthreads();
  }
  if constexpr (LOCAL) {
    for (; t < t_full_end; ++t) {
      const bool more = t + 1 < ntiles;
      if (more) stage_load(t + 1);
      tile(t, std::false_type{});
      if (more) stage_write(t + 1);
      __syncthreads();
    }
    for (; t < ntiles; ++t) {  // masked tiles on the band's far edge
      const bool more = t + 1 < ntiles;
      if (more) stage_load(t + 1);
      tile(t, std::true_type{});
      if (more) stage_write(t + 1);
      __syncthreads();
    }
  }
  for (; t < ntiles; ++t) {
    const bool more = t + 1 < ntiles;
    if (more) stage_load(t + 1);
    tile(t, std::false_type{});
    if (more) stage_write(t + 1);
    __syncthreads();
  }
#ifdef FA_DKV_HEAD_LOOP
  }  // gi
#endif

  FA_LDS char* stage = smem + wave * 32 * C::ROWB;
  // dK = dS^T Q * scale; with the pre-scaled Q (= Q * scale * log2e) in LDS that is dS^T Q' * ln 2
    store_tile_rows<D, T>(dkacc, (FOLD && p.q_prescaled) ? kLn2 : p.scale, stage, rdk, kw0 * dk_rs, lane, dk_rs);
  store_tile_rows<D, T>(dvacc, DROP ? p.drop.rp : 1.0f, stage, rdv, kw0 * dv_rs, lane, dv_rs);
  }  // pass
