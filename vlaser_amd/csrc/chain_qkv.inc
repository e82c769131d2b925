// Body of chain_qkv_kernel: included where VL_WG_X / VL_WG_Y / VL_WG_Z (the workgroup's place in its logical grid) and VL_GRID_X / VL_GRID_Y (that grid)
// are defined -- blockIdx / gridDim in the stand-alone kernel, arguments where the body runs as part of a co-hosted launch.  The text is the kernel's, so the
// stand-alone kernel compiles to what it was.
  constexpr int K = KS * 32, NCH = KS / 4, KSW = KS / NWV, NCW = NCH / NWV, XS = (K / NWV) * 2 + 16;        // NCH: 16-byte chunks of a row per lane of its 16-lane group
  static_assert(NWV == 1 || ((NWV == 2 || NWV == 4) && KS % (4 * NWV) == 0), "several waves: whole chunks per K part");
  extern __shared__ __attribute__((aligned(16))) char smem_q[];    // [NWV][4 RG][XS] normalised activations (bf16) | NWV = 2: f32x4[64] of wave 1's accumulator
  const int lane = threadIdx.x & 63, wv = NWV == 1 ? 0 : (int)(threadIdx.x >> 6), fr = lane & 15, g = lane >> 4, r4 = lane >> 4, j16 = lane & 15;
  char* xs = smem_q + wv * (4 * RG * XS);
  const int unit = VL_WG_X, M = p.M;
  unsigned long long* dbg = DBG ? p.dbg + (size_t)VL_WG_X * 8 : nullptr;
  CH_STAMP(0);
  // ---- requests, in issue order: position id of the lane's row (cos / sin hang off it), norm weight + residual stream (L2), epilogue bias, weights (HBM)
  const int pos = p.pos_ids[min(fr, M - 1)];
  u32x4 wn[NCH], hc[RG][NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) wn[i] = ld_global_16(p.norm_w + (j16 + 16 * i) * 8);
#pragma unroll
  for (int rg = 0; rg < RG; ++rg) {
    const int row = min(rg * 4 + r4, M - 1);
#pragma unroll
    for (int i = 0; i < NCH; ++i) hc[rg][i] = ld_global_16(p.h_in + (row * K + (j16 + 16 * i) * 8));
  }
  const u32x2 bias = *reinterpret_cast<const u32x2*>(p.bias + unit * 16 + g * 4);
  __builtin_amdgcn_sched_barrier(0);           // pin the issue order: vmcnt retires in order, the scheduler does not know
  u32x4 w[KSW];
  {
    const u32x4* src = p.W + (size_t)unit * (KS * 64) + wv * (KSW * 64) + lane;
#pragma unroll
    for (int f = 0; f < KSW; ++f) w[f] = __builtin_nontemporal_load(src + f * 64);
  }
  __builtin_amdgcn_sched_barrier(0);
  const int d = ((unit & 7) << 3) + 2 * g;
  int pos_l = pos;
  asm volatile("" : "+v"(pos_l));              // everything computed from the position id stays BEHIND the weight requests (hipcc hoisted its sign extension -- and with it
                                               // a wait for the id's round trip -- in front of them)
  const f32x2_t cs = *reinterpret_cast<const f32x2_t*>(p.rope_cos + (size_t)pos_l * 64 + d);     // behind the weights in the queue: only the epilogue needs them
  const f32x2_t sn = *reinterpret_cast<const f32x2_t*>(p.rope_sin + (size_t)pos_l * 64 + d);
  __builtin_amdgcn_sched_barrier(0);

  // ---- RMSNorm: xn = bf16(w * bf16(h * rsqrt(mean(h^2) + eps))), one row per 16-lane group and row group; wave-local (no barrier)
#pragma unroll
  for (int rg = 0; rg < RG; ++rg) {
    float ssq = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float lo = bf16lo_to_f32(hc[rg][i][e]), hi = bf16hi_to_f32(hc[rg][i][e]); ssq += lo * lo + hi * hi; }
    ssq = group16_sum(ssq);
    const float rs = rsqrtf(ssq / (float)K + p.eps);
    const int row = rg * 4 + r4;
#pragma unroll
    for (int i2 = 0; i2 < NCW; ++i2) {
      u32x4 hv, wv4;
      if constexpr (NWV == 1) { hv = hc[rg][i2]; wv4 = wn[i2]; }
      else {                                     // this wave's K part: chunks [wv NCW, (wv + 1) NCW) -- selected without indexing the register arrays dynamically
        hv = hc[rg][i2]; wv4 = wn[i2];
#pragma unroll
        for (int v = 1; v < NWV; ++v)
#pragma unroll
          for (int e = 0; e < 4; ++e) { hv[e] = wv == v ? hc[rg][v * NCW + i2][e] : hv[e]; wv4[e] = wv == v ? wn[v * NCW + i2][e] : wv4[e]; }
      }
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float lo = round_bf16(bf16lo_to_f32(hv[e]) * rs) * bf16lo_to_f32(wv4[e]);
        const float hi = round_bf16(bf16hi_to_f32(hv[e]) * rs) * bf16hi_to_f32(wv4[e]);
        o[e] = pack_bf16x2(lo, hi);
      }
      if (row < M) *reinterpret_cast<u32x4*>(xs + row * XS + (j16 + 16 * i2) * 16) = o;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  CH_STAMP(2);
  // ---- GEMV over the whole K: two accumulators so that consecutive MFMAs do not wait for each other
  const bool mok = fr < M;
  const char* xrow = xs + (mok ? fr : 0) * XS + g * 16;
  f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
#pragma unroll
  for (int f = 0; f < KSW; f += 2) {
    const u32x4 x0 = *reinterpret_cast<const u32x4*>(xrow + f * 64), x1 = *reinterpret_cast<const u32x4*>(xrow + (f + 1) * 64);     // rows >= M shadow row 0 (never stored)
    acc0 = mfma16(as_bf16x8(w[f]), as_bf16x8(x0), acc0);
    acc1 = mfma16(as_bf16x8(w[f + 1]), as_bf16x8(x1), acc1);
  }
  f32x4 acc;
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = acc0[e] + acc1[e];
  if constexpr (DBG) asm volatile("" ::"v"(acc[0]));
  CH_STAMP(3);
  if constexpr (NWV > 1) {                       // out = sum of the K parts in wave order, wave 0 finishes
    f32x4* red = reinterpret_cast<f32x4*>(smem_q + NWV * (4 * RG * XS));
    if (wv != 0) red[(wv - 1) * 64 + lane] = acc;
    __syncthreads();
    if (wv != 0) return;
#pragma unroll
    for (int v = 1; v < NWV; ++v) {
      const f32x4 o = red[(v - 1) * 64 + lane];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += o[e];
    }
  }
  // ---- epilogue: bias + RoPE + scatter (as skinny_epilogue16<QKV_ROPE>): lane -> row m = fr, values [d, d+1, d+64, d+65] of head unit / 8
  if (mok) {
    const int m = fr, head = unit >> 3;
    const float b0 = bf16lo_to_f32(bias[0]), b1 = bf16hi_to_f32(bias[0]), b2 = bf16lo_to_f32(bias[1]), b3 = bf16hi_to_f32(bias[1]);
    const float x1[2] = {round_bf16(acc[0] + b0), round_bf16(acc[1] + b1)}, x2[2] = {round_bf16(acc[2] + b2), round_bf16(acc[3] + b3)};
    const int b = ch_fdiv(m, __builtin_amdgcn_rcpf((float)p.tok_per_batch));
    const int slot = p.slot_base >= 0 ? p.slot_base + (m - b * p.tok_per_batch) : pos_l;
    const int nq = p.n_q_heads, nkv = p.n_kv_heads;
    if (head < nq + nkv) {
      float o1[2], o2[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        o1[e] = x1[e] * cs[e] - x2[e] * sn[e];
        o2[e] = x2[e] * cs[e] + x1[e] * sn[e];
      }
      bf16_t* dst = head < nq ? p.q_out + (size_t)m * nq * 128 + head * 128 : p.k_cache + (((size_t)b * nkv + (head - nq)) * p.s_max + slot) * 128;
      *reinterpret_cast<uint32_t*>(dst + d) = pack_bf16x2(o1[0], o1[1]);
      *reinterpret_cast<uint32_t*>(dst + d + 64) = pack_bf16x2(o2[0], o2[1]);
    } else {
      bf16_t* vt = p.vt_cache + ((size_t)b * nkv + (head - nq - nkv)) * 128 * p.s_max + slot;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        vt[(size_t)(d + e) * p.s_max] = f32_to_bf16(x1[e]);
        vt[(size_t)(d + 64 + e) * p.s_max] = f32_to_bf16(x2[e]);
      }
    }
  }
  CH_STAMP(5);
