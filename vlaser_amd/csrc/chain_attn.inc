// Body of chain_attn_kernel: included where VL_WG_X / VL_WG_Y / VL_WG_Z (the workgroup's place in its logical grid) and VL_GRID_X / VL_GRID_Y (that grid)
// are defined -- blockIdx / gridDim in the stand-alone kernel, arguments where the body runs as part of a co-hosted launch.  The text is the kernel's, so the
// stand-alone kernel compiles to what it was.
  constexpr int HD = 128, DC = 4, DT = 8;
  const int lane = threadIdx.x, fr = lane & 15, g = lane >> 4;
  const int kvh = VL_WG_X, split = VL_WG_Y >> p.tile_sh, tile0 = VL_WG_Y & p.tile_sh, b = VL_WG_Z;
  unsigned long long* dbg = DBG ? p.dbg + (((size_t)VL_WG_Z * VL_GRID_Y + VL_WG_Y) * VL_GRID_X + VL_WG_X) * 8 : nullptr;
  CH_STAMP(0);
  const int nq = p.sq, nrows = p.G * nq;
  const bf16_t* K = p.k + (size_t)b * p.k_bs + (size_t)kvh * p.k_hs;
  const bf16_t* VT = p.vt + (size_t)b * p.vt_bs + (size_t)kvh * p.vt_hs;
  const int n_chunks = (p.kv_len + 31) >> 5;
  // ---- every request of the wave: Q rows (written by the previous launch), then K / V^T of its NC chunks (clamped: a chunk past the end is fully masked)
  u32x4 qv[QT][DC];
  int row_hi2[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int r = min((tile0 + qt) * 16 + fr, nrows - 1);
    const int hg = (int)(((float)r + 0.5f) * __builtin_amdgcn_rcpf((float)nq)), tok = r - hg * nq;
    row_hi2[qt] = (tok == 0 && p.first_tok_kv_len > 0) ? p.first_tok_kv_len : 0x7fffffff;
    const bf16_t* Q = p.q + (size_t)b * p.q_bs + (size_t)(kvh * p.G + hg) * p.q_hs + (size_t)tok * p.q_ss;
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) qv[qt][dc] = ld_global_16(Q + dc * 32 + g * 8);
  }
  u32x4 kf[NC][2][DC], vf[NC][DT];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int key0 = min(split * NC + c, n_chunks - 1) << 5;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = key0 + (fr >> 2) * 8 + t * 4 + (fr & 3);
#pragma unroll
      for (int dc = 0; dc < DC; ++dc) kf[c][t][dc] = ld_global_16(K + (size_t)min(key, p.kv_len - 1) * HD + dc * 32 + g * 8);
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) vf[c][dt] = ld_global_16(VT + (size_t)(dt * 16 + fr) * p.ld_vt + key0 + g * 8);
  }
  f32x4 mk[DENSE ? QT : 1][DENSE ? NC : 1][2];
  if constexpr (DENSE) {
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      const int r = min((tile0 + qt) * 16 + fr, nrows - 1);
      const int hg = (int)(((float)r + 0.5f) * __builtin_amdgcn_rcpf((float)nq)), tok = r - hg * nq;
      const float* mrow = p.mask + (size_t)b * p.mask_bs + (size_t)tok * p.mask_rs;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int key0 = min(split * NC + c, n_chunks - 1) << 5;
#pragma unroll
        for (int t = 0; t < 2; ++t) mk[qt][c][t] = *reinterpret_cast<const f32x4*>(mrow + key0 + g * 8 + t * 4);
      }
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  // (behind the requests: the two scalar round trips -- pointer, value -- of the valid length run while the vector loads are in flight)
  int lim1 = p.kv_len, lo2 = 0x7fffffff, hi2 = 0;
  if (p.mode == VL_ATTN_PREFIX && !DENSE) {
    lim1 = min(p.valid_len ? vl_sload_i32(p.valid_len + b) : p.kv_len, p.kv_len);      // scalar cache: not in the vmcnt queue
    lo2 = p.blk_start; hi2 = p.kv_len;
  }
  f32x4 o[QT][DT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt)
#pragma unroll
    for (int i = 0; i < DT; ++i) o[qt][i] = f32x4{0, 0, 0, 0};
  float m_run[QT], l_run[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) { m_run[qt] = -1.0e30f; l_run[qt] = 0.f; }
  const float sc = p.scale * 1.4426950408889634f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int ci = split * NC + c;
    const int key0 = min(ci, n_chunks - 1) << 5;
    const bool live = ci < n_chunks;                         // wave-uniform
    bool visk[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = key0 + g * 8 + t * 4 + r;
        visk[t][r] = live & ((key < lim1) | ((key >= lo2) & (key < hi2)));        // bitwise: `&&` / `||` on lane-varying flags become exec-branch blocks
      }
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      f32x4 s[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 acc = {0, 0, 0, 0};
#pragma unroll
        for (int dc = 0; dc < DC; ++dc) acc = mfma16(as_bf16x8(kf[c][t][dc]), as_bf16x8(qv[qt][dc]), acc);
        s[t] = acc;
      }
      float mx = -1.0e30f;
      bool vis[2][4];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = key0 + g * 8 + t * 4 + r;
          vis[t][r] = visk[t][r] & ((key < lim1) | (key < row_hi2[qt]));
          s[t][r] *= sc;
          if constexpr (DENSE) {
            const float mv = mk[qt][c][t][r];
            vis[t][r] = vis[t][r] & (mv > -1.0e30f);
            s[t][r] = vis[t][r] ? __builtin_fmaf(mv, 1.4426950408889634f, s[t][r]) : s[t][r];
          }
          mx = vis[t][r] ? fmaxf(mx, s[t][r]) : mx;
        }
      mx = vl_xor32_max(vl_xor16_max(mx));
      const float m_new = fmaxf(m_run[qt], mx);
      const float alpha = __builtin_amdgcn_exp2f(m_run[qt] - m_new);
      m_run[qt] = m_new;
      float pv[8], psum = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pe = vis[t][r] ? __builtin_amdgcn_exp2f(s[t][r] - m_new) : 0.f;
          psum += pe;
          pv[t * 4 + r] = pe;
        }
      l_run[qt] = l_run[qt] * alpha + psum;
      const u32x4 pk = {pack_bf16x2(pv[0], pv[1]), pack_bf16x2(pv[2], pv[3]), pack_bf16x2(pv[4], pv[5]), pack_bf16x2(pv[6], pv[7])};
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        f32x4 acc = o[qt][dt];
        acc[0] *= alpha; acc[1] *= alpha; acc[2] *= alpha; acc[3] *= alpha;
        o[qt][dt] = mfma16(as_bf16x8(vf[c][dt]), as_bf16x8(pk), acc);
      }
    }
  }
  if constexpr (DBG) asm volatile("" ::"v"(o[0][0][0]));
  CH_STAMP(1);
  // ---- the split's partial: (m, l) and the normalised rows (bf16); lane (fr, g) holds d = 16 dt + 4 g .. + 4 of row 16 (tile0 + qt) + fr
  const size_t pidx = ((size_t)b * p.n_kv + kvh) * p.n_splits + split;
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const float l_tot = vl_xor32_sum(vl_xor16_sum(l_run[qt]));
    const int row = (tile0 + qt) * 16 + fr;
    if (row < nrows) {
      if (g == 0) *reinterpret_cast<f32x2_t*>(p.pml + (pidx * 32 + row) * 2) = f32x2_t{m_run[qt], l_tot};
      const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
      bf16_t* dst = p.po + (pidx * 32 + row) * 128 + g * 4;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        *reinterpret_cast<u32x2*>(dst + dt * 16) = u32x2{pack_bf16x2(o[qt][dt][0] * inv, o[qt][dt][1] * inv), pack_bf16x2(o[qt][dt][2] * inv, o[qt][dt][3] * inv)};
    }
  }
  CH_STAMP(3);
