// Body of the MLA decoding attention kernel (fa_decode_mla.hip has the description), included once per kernel: the including
// kernel defines T, the parameter block p and RAGGED -- false in fa_decode_paged_kernel<MLA, T>, with placeholders for `cu_q`,
// `plan` and `total_q`; true in fa_decode_ragged_kernel<Latent, T>, which takes them from its own parameter block.  Kept as text
// rather than as a device function, as fa_decode_body.inc is, so that the rectangular kernel compiles exactly as it did before
// the packed form existed.
// RAGGED (include_mla_ragged/mi355fa_ragged_mla.h): packed queries [total_q, H, 576] with a length S_b per sequence.  The work
// item's (b, rb) comes from the device-built plan (fa_decode_ragged_plan_kernel with group = H) instead of from the grid, S_q of
// the item is S_b, and Q / O / LSE / the partials are addressed by packed row.  From there it is the same work item: the result
// has the bits of the rectangular kernel on sequence b alone.
  using C = MlaCfg;
  using vec8 = typename T::vec8;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  FA_LDS char* smem = (FA_LDS char*)smem_raw;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- work item: (b * RB + rb) * nsplit + split; RAGGED: k * nsplit + split, (b, rb) = entry k of the plan, whose end
  // marker (b outside [0, B)) leaves before any barrier -- pb is wave-uniform and the same in all four waves ----
  int Sq = p.Sq, q0 = 0;   // RAGGED: S_b and the first packed row of sequence b,
  int pb = 0, prb = 0;     // and the work item
  if constexpr (RAGGED) {
    // one wave-uniform 8-byte load; the plan kernel finished before this one started (constant address space, as the table)
    typedef const __attribute__((address_space(4))) int* const_plan_t;
    const const_plan_t e = (const_plan_t)plan + 4 + 2 * (long long)(blockIdx.x / p.nsplit);
    pb = __builtin_amdgcn_readfirstlane(e[0]);
    prb = __builtin_amdgcn_readfirstlane(e[1]);
    if ((unsigned)pb >= (unsigned)p.B) return;
    // ragged_len's clamp: both ends into [0, total_q], the second to the first -- the rows [q0, q0 + S_b) lie inside the packed
    // tensors whatever cu_q holds
    q0 = min(max(cu_q[pb], 0), total_q);
    Sq = min(max(cu_q[pb + 1], q0), total_q) - q0;
    // (cannot happen with the plan of this launch; with it the rows below stay inside S_b whatever the plan holds)
    if (prb < 0 || prb * kMlaRows >= p.H * Sq) return;
  }
  const int g = p.H, M = g * Sq, RB = (M + kMlaRows - 1) / kMlaRows;
  int w = blockIdx.x;
  const int split = w % p.nsplit;
  w /= p.nsplit;
  const int rb = RAGGED ? prb : w % RB, b = RAGGED ? pb : w / RB;
  const int L = min(max(p.seqlens[b] + (RAGGED ? (p.Snew ? Sq : 0) : p.Snew), 0), p.Scache);

  // ---- this row block's visible key tiles (from tile 0: `causal` is the only mask), and this split's share of them ----
  const int r0 = rb * kMlaRows, rlast = min(M, r0 + kMlaRows) - 1;
  const int pos1 = L - Sq + rlast / g;   // position of the block's last query
  const int hi = p.causal ? min(L, pos1 + 1) : L;
  const int nt = hi > 0 ? (hi + kMlaTile - 1) / kMlaTile : 0;
  const int s_beg = (int)((long long)nt * split / p.nsplit);
  const int s_end = (int)((long long)nt * (split + 1) / p.nsplit);

  // ---- this lane's query row: the Q^T fragments (B operand) of the wave's columns, its position ----
  const int qrow = r0 + r, qi = qrow / g, qh = qrow - qi * g;
  const int pos = L - Sq + qi;
  vec8 qf[C::KS + 1];
  {
    const bool valid = qrow < M;
    const char* qp;
    if constexpr (RAGGED)   // packed row q0 + qi (qi < S_b where valid: inside [0, total_q))
      qp = (const char*)p.q + (long long)qh * p.lq.sh + (long long)(q0 + qi) * p.lq.rs + 16 * h;
    else
      qp = (const char*)p.q + b * p.lq.sb + (long long)qh * p.lq.sh + (long long)qi * p.lq.rs + 16 * h;
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
  // rows of O / LSE / a split's partials (RAGGED: LSE is [H, total_q], the packed decode call's layout)
  const long long R = RAGGED ? (long long)p.H * total_q : (long long)p.B * p.H * Sq;
  for (int it = tid; it < kMlaRows * (kMlaDv / 4); it += 256) {
    const int row = it / (kMlaDv / 4), d4 = (it % (kMlaDv / 4)) * 4;
    const int qr = r0 + row;
    if (qr >= M) break;   // rows ascend with `it`
    const float mx = sm[row], lsum = sl[row];
    const f32x4 acc = *(const f32x4*)(stage + row * C::OST + d4);
    const int i = qr / g, head = qr - i * g;
    const long long ridx = RAGGED ? (long long)head * total_q + (q0 + i) : ((long long)b * p.H + head) * Sq + i;
    if (p.nsplit == 1) {
      const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
      typedef __attribute__((ext_vector_type(4))) typename T::elem e4;
      e4 ov;
#pragma unroll
      for (int j = 0; j < 4; ++j) ov[j] = (typename T::elem)(acc[j] * inv);
      char* op;
      if constexpr (RAGGED)
        op = (char*)p.o + (long long)head * p.lo.sh + (long long)(q0 + i) * p.lo.rs + d4 * 2;
      else
        op = (char*)p.o + b * p.lo.sb + (long long)head * p.lo.sh + (long long)i * p.lo.rs + d4 * 2;
      *(u32x2*)op = __builtin_bit_cast(u32x2, ov);
      if (d4 == 0 && p.lse) p.lse[ridx] = lsum > 0.f ? (mx + __builtin_log2f(lsum)) * kLn2 : -INFINITY;
    } else {
      const long long pr = split * R + ridx;
      *(f32x4*)(p.ws + pr * kMlaDv + d4) = acc;
      if (d4 == 0) *(f32x2_t*)(p.ws + (long long)p.nsplit * R * kMlaDv + 2 * pr) = f32x2_t{mx, lsum};
    }
  }
