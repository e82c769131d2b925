// Body of attn_prefill_kernel: included where VL_WG_X / VL_WG_Y / VL_WG_Z (the workgroup's place in its logical grid) and VL_GRID_X / VL_GRID_Y (that grid)
// are defined -- blockIdx / gridDim in the stand-alone kernel, arguments where the body runs as part of a co-hosted launch.  The text is the kernel's, so the
// stand-alone kernel compiles to what it was.
  constexpr int DC = HD / 32;   // d-chunks of 32 for S^T
  constexpr int DT = HD / 16;   // d-tiles of 16 for O^T
  constexpr int NC = TK / 32;   // 32-key chunks per tile
  constexpr int KCH = TK * HD / 2048;  // 16-byte chunks per thread for the K tile (TK*HD*2/16/256)
  constexpr int VCH = TK * HD / 2048;  // same for V^T tile
  constexpr int TILE_BYTES = 2 * TK * HD * 2;
  constexpr int MERGE_WAVE = (DT * 4 + 2) * 256;                 // one wave's (o[DT][4], m, l) as [slot][lane] fp32
  constexpr int MERGE_BYTES = (KS - 1) * 4 * MERGE_WAVE;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // max(KS * TILE_BYTES, MERGE_BYTES)
  const VlaserAttnArgs& a = p.a;
  const int lane = threadIdx.x & 63;
  const int grp = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8);      // key-split group of this wave
  const int tid = threadIdx.x & 255, wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // thread / wave index inside the group
  char* Ks = smem + grp * TILE_BYTES;
  char* Vs = Ks + TK * HD * 2;
  const int fr = lane & 15, g = lane >> 4;
  // TAIL launches are 1-D per batch element with the workgroups of the <= 16 tail rows LAST (ids >= n_full * heads): found with a lab switch that made those 16
  // workgroups exit at once -- the launch still took 22.5 us against 14.8 us for 256 workgroups, i.e. the dispatcher hands out CUs round-robin and, with the
  // light workgroups sprinkled through a 17 x 16 grid, doubles full workgroups up on some CUs while others idle.  All full workgroups first = one per CU
  // (empty tail workgroups dispatched last: 17.2 us; with their work 21.7 us -- a workgroup that walks a head's 256 KB of K / V beside a full one takes as long
  // as the full one, however little it computes: profiles/r04m_vit_attention_tail.md).
  int qb = VL_WG_X, h = VL_WG_Y;
  if constexpr (TAIL) {
    if (p.tail_qb >= 0) {
      const int nfull = p.tail_qb * a.n_q_heads;
      if ((int)VL_WG_X < nfull) { h = VL_WG_X / p.tail_qb; qb = VL_WG_X - h * p.tail_qb; }
      else { h = VL_WG_X - nfull; qb = p.tail_qb; }
    }
  }
  const int b = VL_WG_Z;
  const int kvh = h / (a.n_q_heads / a.n_kv_heads);
  // TAIL: workgroup p.tail_qb holds the LAST <= 16 query rows (FULL mode).  All four of its waves take those same rows and split the key TILES between them
  // (wave w computes tiles w, w + 4, ...; the staging and its barriers stay cooperative), flash-decoding merge through LDS at the end: a quarter of a full
  // workgroup's issue slots, so the full workgroup it shares a CU with (272 workgroups on 256 CUs at S = 1025) is slowed far less than by a second full one.
  // (First built as a workgroup pulling its chunks straight from global memory: latency-bound, as slow as the full workgroups -- profiles/r04l.)
  const bool tailwg = TAIL && !HOST && qb == p.tail_qb;
  // r04 (tail_host): the <= 16 tail rows ride in the LAST FULL workgroup of their head instead -- a second softmax state per wave, advanced over a quarter of the
  // keys of every tile (wave w: the w-th 32-key chunk), merged like the tail workgroup's.  The grid is exactly tail_qb x heads workgroups (ViT: 256 = one per CU, one
  // round) and 16 of them carry +25 % work, instead of 16 extra workgroups that each walk a head's K / V beside a full one.
  const bool hostwg = HOST && qb == p.tail_qb - 1;
  const int q_row = qb * 64 + (tailwg ? 0 : wave * 16) + fr;  // this lane's query row (within the batch element)

  const bf16_t* Q = reinterpret_cast<const bf16_t*>(a.q) + (size_t)b * a.q_bs + (size_t)h * a.q_hs;
  const bf16_t* K = reinterpret_cast<const bf16_t*>(a.k) + (size_t)b * a.k_bs + (size_t)kvh * a.k_hs;
  const bf16_t* VT = reinterpret_cast<const bf16_t*>(a.vt) + (size_t)b * a.vt_bs + (size_t)kvh * a.vt_hs;

  // visibility
  int lim1, lo2 = 0x7fffffff, hi2 = 0;
  int blk_lim1, blk_has2 = 0;
  {
    const int q_last = min(a.sq, qb * 64 + 64) - 1;
    if (a.mode == VL_ATTN_FULL || DENSE) {
      lim1 = blk_lim1 = a.kv_len;
    } else if (a.mode == VL_ATTN_CAUSAL) {
      lim1 = min(a.kv_len, q_row + 1 + a.causal_off);
      blk_lim1 = min(a.kv_len, q_last + 1 + a.causal_off);
    } else {
      const int vl = a.valid_len ? a.valid_len[b] : a.kv_len;
      lim1 = blk_lim1 = min(vl, a.kv_len);
      if (q_row + a.q_row_off >= a.blk_start) { lo2 = a.blk_start; hi2 = a.kv_len; }
      blk_has2 = (q_last + a.q_row_off >= a.blk_start);
    }
  }
  // VARLEN: first key of this lane's sequence, the largest such key among the wave's 16 rows (rows ascend with the lane: lane 15 holds it) and the first key
  // TILE any of the workgroup's 64 rows sees (row qb * 64 belongs to the earliest sequence)
  int seq_lo = 0, wave_lo = 0, t0 = 0;
  if constexpr (VARLEN) {
    const int32_t* cu = a.valid_len;
    seq_lo = cu[vl_seq_of_row(cu, a.n_splits, min(q_row, a.sq - 1))];
    wave_lo = __builtin_amdgcn_readlane(seq_lo, 15);
    t0 = min(max(cu[vl_seq_of_row(cu, a.n_splits, qb * 64)], 0), qb * 64) / TK;      // (clamped: a corrupt table must not move a tile out of the cache)
  }

  // Q fragments (MFMA-B: col = query fr, k = d)
  bf16x8 qf[DC];
#pragma unroll
  for (int dc = 0; dc < DC; ++dc) {
    u32x4 v = {0, 0, 0, 0};
    if (q_row < a.sq) v = ld_global_16(Q + (size_t)q_row * a.q_ss + dc * 32 + g * 8);
    qf[dc] = as_bf16x8(v);
  }

  f32x4 o[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) o[i] = f32x4{0, 0, 0, 0};
  float m_run = NEG_BIG, l_run = 0.f;
  // the host workgroup's second state: rows tail_qb * 64 + fr (rows >= sq: zero queries, never written)
  bf16x8 qf2[HOST ? DC : 1];
  f32x4 o2[HOST ? DT : 1];
  float m2 = NEG_BIG, l2 = 0.f;
  if constexpr (HOST) {
#pragma unroll
    for (int i = 0; i < DT; ++i) o2[i] = f32x4{0, 0, 0, 0};
    const int q_row2 = p.tail_qb * 64 + fr;
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) {
      u32x4 v = {0, 0, 0, 0};
      if (hostwg && q_row2 < a.sq) v = ld_global_16(Q + (size_t)q_row2 * a.q_ss + dc * 32 + g * 8);
      qf2[dc] = as_bf16x8(v);
    }
  }
  const float sc = a.scale * 1.4426950408889634f;  // softmax in base 2

  // the <= 32 keys behind the last full tile (FULL mode): requested now as one chunk straight from global memory, folded in after the tile loop
  DirectChunk<TAIL ? HD : 32> tailc;
  if constexpr (TAIL) { if (p.tail_key0 >= 0) tailc.load(K, VT, p.tail_key0, a.kv_len, a.ld_vt, fr, g); }

  // key-tile schedule: [0, n1) then tiles overlapping [blk_start, kv_len)
  int n1_ = (TAIL && p.tail_key0 >= 0) ? p.tail_key0 / TK : (blk_lim1 + TK - 1) / TK;
  if constexpr (VARLEN) n1_ -= t0;            // tiles [t0, diagonal]
  const int n1 = n1_;
  int t2_lo = 0, t2_hi = 0;
  if (blk_has2) { t2_lo = max(n1, a.blk_start / TK); t2_hi = (a.kv_len + TK - 1) / TK; }
  const int n_tiles = n1 + max(0, t2_hi - t2_lo);

  u32x4 rk[KCH], rv[VCH];
  // DENSE: this lane's mask values of the tile in flight (rmk) and of the tile being computed (cmk): row = its query row, 4 consecutive keys per (chunk, t)
  f32x4 rmk[DENSE ? NC : 1][2], cmk[DENSE ? NC : 1][2];
  const float* mrow = nullptr;
  const float inv_scale = DENSE ? 1.0f / a.scale : 0.f;
  if constexpr (DENSE) mrow = a.mask + (size_t)b * a.mask_bs + (size_t)min(q_row, a.sq - 1) * a.mask_rs;
  auto tile_key0 = [&](int it) {
    if constexpr (VARLEN) return (t0 + it) * TK;
    else return (it < n1 ? it : t2_lo + (it - n1)) * TK;
  };
  auto load_tile = [&](int it) {
    const int key0 = tile_key0(it);
    if constexpr (DENSE) {
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int t = 0; t < 2; ++t) rmk[c][t] = *reinterpret_cast<const f32x4*>(mrow + min(key0 + c * 32 + g * 8 + t * 4, (int)a.mask_rs - 4));
    }
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
      const int c = tid + i * 256;              // chunk id: row = c / (HD/8), slot = c % (HD/8)
      const int row = c / (HD / 8), slot = c % (HD / 8);
      const int key = min(key0 + row, a.kv_len - 1);      // clamped, unconditional: keys >= kv_len are never visible
      rk[i] = ld_global_16(K + (size_t)key * HD + slot * 8);
    }
#pragma unroll
    for (int i = 0; i < VCH; ++i) {
      const int c = tid + i * 256;              // row = d = c / (TK/8), slot = c % (TK/8) (8 keys each)
      const int row = c / (TK / 8), slot = c % (TK / 8);
      rv[i] = ld_global_16(VT + (size_t)row * a.ld_vt + min(key0 + slot * 8, a.ld_vt - 8));  // rows are padded to a multiple of 64 keys; clamped beyond
    }
  };
  auto store_tile = [&]() {
    if constexpr (DENSE) {
#pragma unroll
      for (int c = 0; c < NC; ++c) { cmk[c][0] = rmk[c][0]; cmk[c][1] = rmk[c][1]; }
    }
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
      const int c = tid + i * 256;
      *reinterpret_cast<u32x4*>(Ks + k_lds_off<HD>(c / (HD / 8), c % (HD / 8))) = rk[i];
    }
#pragma unroll
    for (int i = 0; i < VCH; ++i) {
      const int c = tid + i * 256;
      *reinterpret_cast<u32x4*>(Vs + vt_lds_off<TK>(c / (TK / 8), c % (TK / 8))) = rv[i];
    }
  };

  // one TK-key tile against this wave's 16 query rows; S^T tiles s[c][t], key(c,t,reg) = key0 + c*32 + g*8 + t*4 + reg
  // (nc_c chunks of 32 keys starting at chunk cb of the tile: the whole tile for a wave's own rows, ONE chunk for the hosted tail rows)
  auto tile_body = [&](int key0, auto masked_c, auto nc_c, int cb, const auto& qf, float& m_run, float& l_run, auto& o) __attribute__((always_inline)) {
    constexpr bool MASKED = decltype(masked_c)::value;
    constexpr int NC = decltype(nc_c)::value;
    f32x4 s[NC][2];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 acc = {0, 0, 0, 0};
        const int krow = (cb + c) * 32 + (fr >> 2) * 8 + t * 4 + (fr & 3);
#pragma unroll
        for (int dc = 0; dc < DC; ++dc) {
          bf16x8 kf = as_bf16x8(*reinterpret_cast<const u32x4*>(Ks + k_lds_off<HD>(krow, dc * 4 + g)));
          acc = mfma16(kf, qf[dc], acc);
        }
        s[c][t] = acc;
      }
    // online softmax in base 2 (lane-local per query; max all-reduced over the 4 lane groups); the scale is applied inside the
    // exponent's FMA: max(s) * sc == max(s * sc) for sc > 0
    float mx = NEG_BIG;
    bool vis[NC][2][4];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (MASKED && DENSE) {
            // score * scale + mask == (score + mask / scale) * scale: the mask enters before the scale that the exponent's FMA applies
            const int key = key0 + (cb + c) * 32 + g * 8 + t * 4 + r;
            const float mv = cmk[cb + c][t][r];
            const bool v = (key < lim1) && (mv > -1.0e30f);
            vis[c][t][r] = v;
            s[c][t][r] = v ? __builtin_fmaf(mv, inv_scale, s[c][t][r]) : s[c][t][r];
            if (v) mx = fmaxf(mx, s[c][t][r]);
          } else if constexpr (MASKED && VARLEN) {
            const int key = key0 + (cb + c) * 32 + g * 8 + t * 4 + r;
            const bool v = key < lim1 && key >= seq_lo;
            vis[c][t][r] = v;
            if (v) mx = fmaxf(mx, s[c][t][r]);
          } else if constexpr (MASKED) {
            const int key = key0 + (cb + c) * 32 + g * 8 + t * 4 + r;
            const bool v = (key < lim1) || (key >= lo2 && key < hi2);
            vis[c][t][r] = v;
            if (v) mx = fmaxf(mx, s[c][t][r]);
          } else {
            vis[c][t][r] = true;
            mx = fmaxf(mx, s[c][t][r]);
          }
        }
    mx = vl_xor32_max(vl_xor16_max(mx));          // (r05) permlane swaps instead of two ds_bpermute round trips in the softmax chain of every tile: same operands
    const float m_new = fmaxf(m_run, mx * sc);
    const float alpha = fast_exp2(m_run - m_new);
    m_run = m_new;
    float psum = 0.f;
    bf16x8 pf[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      float pv[8];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float pe = fast_exp2(__builtin_fmaf(s[c][t][r], sc, -m_new));
          if constexpr (MASKED) pe = vis[c][t][r] ? pe : 0.f;
          psum += pe;
          pv[t * 4 + r] = pe;
        }
      u32x4 pk = {pack_bf16x2(pv[0], pv[1]), pack_bf16x2(pv[2], pv[3]), pack_bf16x2(pv[4], pv[5]), pack_bf16x2(pv[6], pv[7])};
      pf[c] = as_bf16x8(pk);
    }
    l_run = l_run * alpha + psum;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      f32x4 acc = o[dt];
      acc[0] *= alpha; acc[1] *= alpha; acc[2] *= alpha; acc[3] *= alpha;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        bf16x8 vf = as_bf16x8(*reinterpret_cast<const u32x4*>(Vs + vt_lds_off<TK>(dt * 16 + fr, (cb + c) * 4 + g)));
        acc = mfma16(vf, pf[c], acc);
      }
      o[dt] = acc;
    }
  };
  // smallest prefix limit among this wave's 16 rows (wave-uniform): a tile ending at or below it needs no masks
  const int wave_lim1 = DENSE ? 0 : (a.mode == VL_ATTN_CAUSAL ? min(a.kv_len, qb * 64 + wave * 16 + 1 + a.causal_off) : blk_lim1);      // (DENSE: every tile takes the masked body)

  const int n_it = (n_tiles + KS - 1) / KS;                   // block-uniform trip count; a group past its last tile idles at the barriers
  if (n_tiles > 0) load_tile(min(grp, n_tiles - 1));
  for (int itg = 0; itg < n_it; ++itg) {
    const int it = itg * KS + grp;
    __syncthreads();  // previous tile's LDS reads are done
    store_tile();
    __syncthreads();
    load_tile(min(it + KS, n_tiles - 1));                      // unconditional (clamped): a conditional load costs a full vmcnt drain
    if (it >= n_tiles) continue;
    if (tailwg && (it & 3) != wave) continue;                  // (wave-uniform) the tail workgroup's waves take every fourth tile each
    const int key0 = tile_key0(it);

    // a tile every row of this wave sees in full (all interior tiles of FULL / PREFIX, the tiles left of the diagonal of CAUSAL)
    // skips the visibility arithmetic: the loop is VALU-issue bound (about 230 VALU + 17 transcendental instructions per tile
    // against 16 MFMAs at head_dim 64), and the masks were 40 % of it
    using all_c = std::integral_constant<int, NC>;
    bool whole = key0 + TK <= wave_lim1;
    if constexpr (VARLEN) whole = whole && key0 >= wave_lo;
    if (whole) tile_body(key0, std::false_type{}, all_c{}, 0, qf, m_run, l_run, o);
    else tile_body(key0, std::true_type{}, all_c{}, 0, qf, m_run, l_run, o);
    if constexpr (HOST) {
      // the hosted rows: wave w takes the w-th 32-key chunk of EVERY tile (+25 % per wave and tile; a whole tile every fourth trip would double the time
      // of every trip -- the tiles are barrier-stepped: measured 24.6 us against 21.5 for the tail workgroups).  FULL mode: the limits do not depend on the row
      static_assert(!HOST || NC == 4, "HOST deals one 32-key chunk of a 128-key tile to each of the 4 waves");
      if (hostwg) {
        using one_c = std::integral_constant<int, 1>;
        if (key0 + TK <= wave_lim1) tile_body(key0, std::false_type{}, one_c{}, wave, qf2, m2, l2, o2);
        else tile_body(key0, std::true_type{}, one_c{}, wave, qf2, m2, l2, o2);
      }
    }
  }

  if constexpr (TAIL) {
    if (p.tail_key0 >= 0 && grp == 0 && (!tailwg || wave == 0)) tailc.process(qf, p.tail_key0, a.kv_len, sc, g, m_run, l_run, o);
    if constexpr (HOST) { if (p.tail_key0 >= 0 && hostwg && wave == 0) tailc.process(qf2, p.tail_key0, a.kv_len, sc, g, m2, l2, o2); }
  }
  // merge of the four waves' partial softmax states (same rows, disjoint keys) through LDS, fixed order; writes rows out_qb * 64 ...
  auto merge4 = [&](float m_run, float l_run, const auto& o, int out_qb) __attribute__((always_inline)) {
    constexpr int WS = 32 + 16 * HD;
    __syncthreads();                                           // every wave is done with the staged tiles: the area becomes the merge buffer
    float* wm = reinterpret_cast<float*>(smem) + wave * WS;
    {
      float l_tot = vl_xor32_sum(vl_xor16_sum(l_run));
      if (g == 0) { wm[fr] = m_run; wm[16 + fr] = l_tot; }
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<f32x4*>(wm + 32 + fr * HD + dt * 16 + g * 4) = o[dt];
    }
    __syncthreads();
    constexpr int DPT = HD / 16;                               // head-dim columns per thread: 16 rows x HD over 256 threads
    const int row = threadIdx.x >> 4, d0 = (threadIdx.x & 15) * DPT;
    const float* base = reinterpret_cast<const float*>(smem);
    float M = NEG_BIG;
#pragma unroll
    for (int w = 0; w < 4; ++w) M = fmaxf(M, base[w * WS + row]);
    float L = 0.f, acc[DPT];
#pragma unroll
    for (int j = 0; j < DPT; ++j) acc[j] = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float f = fast_exp2(base[w * WS + row] - M);
      L += base[w * WS + 16 + row] * f;
#pragma unroll
      for (int j = 0; j < DPT; ++j) acc[j] += base[w * WS + 32 + row * HD + d0 + j] * f;
    }
    const int q_out = out_qb * 64 + row;
    if (q_out < a.sq) {
      const float inv = L > 0.f ? 1.0f / L : 0.f;
      if (a.lse_out && d0 == 0) a.lse_out[((size_t)b * a.n_q_heads + h) * a.sq + q_out] = M + __builtin_amdgcn_logf(L);
      bf16_t* O = reinterpret_cast<bf16_t*>(a.out) + (size_t)b * a.o_bs + (size_t)q_out * a.o_ss + h * HD + d0;
#pragma unroll
      for (int j = 0; j < DPT; j += 2) *reinterpret_cast<uint32_t*>(O + j) = pack_bf16x2(acc[j] * inv, acc[j + 1] * inv);
    }
  };
  if constexpr (TAIL) {
    if (tailwg) { merge4(m_run, l_run, o, qb); return; }
    if constexpr (HOST) { if (hostwg) merge4(m2, l2, o2, p.tail_qb); }
  }

  if constexpr (KS > 1) {
    // merge the groups' partial softmax states: lane-for-lane (every group holds the same (row, d) elements in the same registers)
    __syncthreads();                                           // all tile reads done: the staging area becomes the merge area
    if (grp > 0) {
      float* mw = reinterpret_cast<float*>(smem + ((grp - 1) * 4 + wave) * MERGE_WAVE) + lane;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) mw[(dt * 4 + r) * 64] = o[dt][r];
      mw[DT * 4 * 64] = m_run;
      mw[(DT * 4 + 1) * 64] = l_run;
    }
    __syncthreads();
    if (grp > 0) return;
#pragma unroll
    for (int j = 1; j < KS; ++j) {
      const float* rw = reinterpret_cast<const float*>(smem + ((j - 1) * 4 + wave) * MERGE_WAVE) + lane;
      const float m_o = rw[DT * 4 * 64], l_o = rw[(DT * 4 + 1) * 64];
      const float m_new = fmaxf(m_run, m_o);
      const float fa = fast_exp2(m_run - m_new), fb = fast_exp2(m_o - m_new);
      m_run = m_new;
      l_run = l_run * fa + l_o * fb;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[dt][r] = o[dt][r] * fa + rw[(dt * 4 + r) * 64] * fb;
    }
  }
  float l_tot = vl_xor32_sum(vl_xor16_sum(l_run));
  if (q_row < a.sq) {
    const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
    // base-2 log-sum-exp of the scaled scores, for the fused backward (vlaser_attn_bwd): P = exp2(s * scale * log2 e - lse)
    if (a.lse_out && g == 0) a.lse_out[((size_t)b * a.n_q_heads + h) * a.sq + q_row] = m_run + __builtin_amdgcn_logf(l_tot);
    bf16_t* O = reinterpret_cast<bf16_t*>(a.out) + (size_t)b * a.o_bs + (size_t)q_row * a.o_ss + h * HD;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      u32x2 pk = {pack_bf16x2(o[dt][0] * inv, o[dt][1] * inv), pack_bf16x2(o[dt][2] * inv, o[dt][3] * inv)};
      *reinterpret_cast<u32x2*>(O + dt * 16 + g * 4) = pk;
    }
  }
