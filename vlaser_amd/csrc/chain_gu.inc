// Body of chain_gu_kernel: included where VL_WG_X / VL_WG_Y / VL_WG_Z (the workgroup's place in its logical grid) and VL_GRID_X / VL_GRID_Y (that grid)
// are defined -- blockIdx / gridDim in the stand-alone kernel, arguments where the body runs as part of a co-hosted launch.  The text is the kernel's, so the
// stand-alone kernel compiles to what it was.
  static_assert(!W8 || (TPU == 1 && (NS == 3 || NS == 6)), "e4m3 weights: built for K = 768 / 1536 and 16-row units");
  constexpr int K = NS * 256, cpr = K / 8, ngr = cpr / 16, gstride = (ngr + 3) & ~3, XS = K * 2 + 16, NF = TPU * NS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, g = lane >> 4;
  unsigned long long* dbg = DBG ? p.dbg + (size_t)VL_WG_X * 8 : nullptr;
  CH_STAMP(0);
  const int M = p.M;
  const int ucount = p.ulo + ((int)VL_WG_X < p.urem ? 1 : 0);
  const int ustart = (int)VL_WG_X * p.ulo + min((int)VL_WG_X, p.urem);
  const int xs_bytes = (M * XS + 15) & ~15;
  char* xs = smem;
  float* red = reinterpret_cast<float*>(smem + xs_bytes);      // [UE][8][TPU][64] f32x4 partial tiles; group sums [M][gstride] during the prologue
  float* gs = red;
  const int nch = M * cpr, slab = M * K;

  // ---- every request of the kernel, in issue order: residual chunk(s), norm weight, the producer's slabs (L2), then the whole weight stream (HBM)
  u32x4 hv[CPT], wv[CPT];
  f32x4 q[CPT][SP > 0 ? 2 * SP : 1];
  int mm[CPT], cc[CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    const int ch = min(c * 512 + tid, nch - 1);
    mm[c] = ch_fdiv(ch, p.inv_cpr);
    cc[c] = (ch - mm[c] * cpr) << 3;
    const int off = mm[c] * K + cc[c];
    hv[c] = ld_global_16(p.h_in + off);
    wv[c] = ld_global_16(p.norm_w + cc[c]);
#pragma unroll
    for (int u = 0; u < SP; ++u) {
      const float* pp = p.partials + (off + u * slab);
      q[c][2 * u] = *reinterpret_cast<const f32x4*>(pp);
      q[c][2 * u + 1] = *reinterpret_cast<const f32x4*>(pp + 4);
    }
  }
  f32x4 wsc = {1.f, 1.f, 1.f, 1.f};          // W8: the scales of the four rows whose sums this lane finishes (wave u finishes unit u; waves beyond the workgroup's units shadow its last)
  if constexpr (W8) wsc = *reinterpret_cast<const f32x4*>(p.w_scale + (size_t)(ustart + min(wave, ucount - 1)) * 16 + g * 4);
  // (hipcc's scheduler moves loads freely -- it does not know that vmcnt retires in issue order: without the fences below it put the norm-weight chunk and two
  //  fragments of unit 0 BEHIND units 1 and 2, so the norm and the first MFMAs waited for the whole stream)
  __builtin_amdgcn_sched_barrier(0);
  // All 8 waves put their (L2-resident) prologue requests into the CU's memory pipeline BEFORE any wave queues weight requests: the pipeline is FIFO per CU, and a
  // wave that started late found its 8 small requests behind 7 x 18 KB of the others' HBM requests (in-chain timeline r05b: prologue data back 3.7 us after the start
  // instead of 2.3).  The barrier waits for instruction issue only -- nobody waits for data here.
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  // W8: NP 16-byte loads, each the lane's fragments of K-steps 2j and 2j + 1, then (odd NS: K = 768) one 8-byte load of the last K-step -- WB bytes per wave and unit
  constexpr int NP = NS / 2, WB = NS * 512;
  u32x4 w[UE][W8 ? NP : NF];
  u32x2 w2[W8 ? UE : 1];          // (even NS: never read)
  if constexpr (W8) {
    const char* wp = reinterpret_cast<const char*>(p.W) + (size_t)wave * WB;
#pragma unroll
    for (int u = 0; u < UE; ++u) {
      const char* src = wp + (size_t)(ustart + min(u, ucount - 1)) * (8 * WB);           // a workgroup with fewer units re-requests its last one
#pragma unroll
      for (int j = 0; j < NP; ++j) w[u][j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + j * 1024) + lane);
      if constexpr (NS & 1) w2[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(src + NP * 1024) + lane);
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
    const u32x4* wp = p.W + (size_t)wave * (NF * 64) + lane;
#pragma unroll
    for (int u = 0; u < UE; ++u) {
      const u32x4* src = wp + (size_t)(ustart + min(u, ucount - 1)) * (8 * NF * 64);      // a workgroup with fewer units re-requests its last one
#pragma unroll
      for (int f = 0; f < NF; ++f) w[u][f] = __builtin_nontemporal_load(src + f * 64);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- phase 1: h = bf16(h_in + sum slabs) (slabs first, residual last), sum of squares per 16-lane group -> LDS
  u32x4 hr[CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    float v[8], sl[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[2 * j] = bf16lo_to_f32(hv[c][j]); v[2 * j + 1] = bf16hi_to_f32(hv[c][j]); }
#pragma unroll
    for (int u = 0; u < SP; ++u) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { sl[j] += q[c][2 * u][j]; sl[4 + j] += q[c][2 * u + 1][j]; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) hr[c][j] = pack_bf16x2(sl[2 * j] + v[2 * j], sl[2 * j + 1] + v[2 * j + 1]);
    float ssq = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { const float lo = bf16lo_to_f32(hr[c][j]), hi = bf16hi_to_f32(hr[c][j]); ssq += lo * lo + hi * hi; }
    const bool on = c * 512 + tid < nch;
    if (!on) ssq = 0.f;                      // clamped duplicate chunk
    ssq = group16_sum(ssq);                 // same operand pairs as the xor butterfly of skinny_kernel: identical bits
    if ((lane & 15) == 0 && on) gs[mm[c] * gstride + (cc[c] >> 7)] = ssq;
  }
  __syncthreads();
  CH_STAMP(1);
  // ---- phase 2: row total in a fixed order, normalise the thread's own values, bf16 activations -> LDS
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    float tot = 0.f;
    const float* gr = gs + mm[c] * gstride;
#pragma unroll
    for (int i = 0; i < ngr; i += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(gr + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) tot += (i + j < ngr) ? t[j] : 0.f;
    }
    const float rs = rsqrtf(tot / (float)K + p.eps);
    u32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float lo = round_bf16(bf16lo_to_f32(hr[c][j]) * rs) * bf16lo_to_f32(wv[c][j]);
      const float hi = round_bf16(bf16hi_to_f32(hr[c][j]) * rs) * bf16hi_to_f32(wv[c][j]);
      o[j] = pack_bf16x2(lo, hi);
    }
    if (c * 512 + tid < nch) *reinterpret_cast<u32x4*>(xs + mm[c] * XS + cc[c] * 2) = o;
  }
  __syncthreads();          // (the group sums alias `red`: every thread has read them before any wave writes a partial accumulator)
  CH_STAMP(2);

  // ---- units: in-workgroup split-K over the 8 waves, reduced through LDS by wave 0 (same order as skinny_kernel: bit-identical)
  const bool mok = fr < M;
  const char* xrow = xs + (mok ? fr : 0) * XS + (wave * (NS * 32) + g * 8) * 2;       // lanes of rows >= M shadow row 0: MFMA columns are independent, their results are never stored
  bf16x8 xf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) xf[s] = as_bf16x8(*reinterpret_cast<const u32x4*>(xrow + s * 64));
  // Every unit's MFMAs as its fragments land (issue order), ALL eight waves leave their partial tiles in LDS, ONE barrier, then wave u finishes unit u: sum of the
  // eight K-slices in wave order (the order of skinny_kernel: wave 0's tile first -- identical bits) + SwiGLU + store.  r05b timeline: with wave 0 finishing the units
  // one after the other behind a barrier each, 1.6-2.1 us passed between "prologue done" and the end of the workgroup -- the weights had landed long before.
#pragma unroll
  for (int u = 0; u < UE; ++u) {
    if (u < ucount) {
      f32x4 a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if constexpr (W8) {
          a0 = mfma16(as_bf16x8(s < 2 * NP ? ch_e4m3x8(w[u][s >> 1][2 * (s & 1)], w[u][s >> 1][2 * (s & 1) + 1]) : ch_e4m3x8(w2[u][0], w2[u][1])), xf[s], a0);
        } else {
          a0 = mfma16(as_bf16x8(w[u][TPU * s]), xf[s], a0);
          if constexpr (TPU == 2) a1 = mfma16(as_bf16x8(w[u][2 * s + 1]), xf[s], a1);
        }
      }
      if (u == 0) { if constexpr (DBG) asm volatile("" ::"v"(a0[0])); CH_STAMP(3); }
      float* r = red + (((u * 8 + wave) * TPU) * 64 + lane) * 4;
      *reinterpret_cast<f32x4*>(r) = a0;
      if constexpr (TPU == 2) *reinterpret_cast<f32x4*>(r + 64 * 4) = a1;
    }
  }
  __syncthreads();
  CH_STAMP(4);
  if (wave < UE && wave < ucount) {
    const int u = wave;
    f32x4 a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};
#pragma unroll
    for (int w2 = 0; w2 < 8; ++w2) {
      const float* r = red + (((u * 8 + w2) * TPU) * 64 + lane) * 4;
      if (w2 == 0) {
        a0 = *reinterpret_cast<const f32x4*>(r);
        if constexpr (TPU == 2) a1 = *reinterpret_cast<const f32x4*>(r + 64 * 4);
      } else {
        a0 += *reinterpret_cast<const f32x4*>(r);
        if constexpr (TPU == 2) a1 += *reinterpret_cast<const f32x4*>(r + 64 * 4);
      }
    }
    const int unit = ustart + u;
    if constexpr (TPU == 2) {
      if (mok && unit * 32 < p.n_valid) {              // unit = [gate16 | up16] -> output columns unit*16 + g*4 + j
        bf16_t* o = p.out + (size_t)fr * p.ldo + unit * 16 + g * 4;
        float r4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r4[j] = round_bf16(silu(round_bf16(a0[j]))) * round_bf16(a1[j]);
        *reinterpret_cast<u32x2*>(o) = u32x2{pack_bf16x2(r4[0], r4[1]), pack_bf16x2(r4[2], r4[3])};
      }
    } else {
      if (mok && unit * 16 < p.n_valid) {              // lane group g: [gate 2g, gate 2g+1, up 2g, up 2g+1] -> output columns unit*8 + 2g, + 1
        bf16_t* o = p.out + (size_t)fr * p.ldo + unit * 8 + g * 2;
        if constexpr (W8) a0 *= wsc;                      // the row scales, on the reduced fp32 sums, before the first rounding
        const float r0 = round_bf16(silu(round_bf16(a0[0]))) * round_bf16(a0[2]);
        const float r1 = round_bf16(silu(round_bf16(a0[1]))) * round_bf16(a0[3]);
        *reinterpret_cast<uint32_t*>(o) = pack_bf16x2(r0, r1);
      }
    }
  }
  // the rounded residual stream (the down projection adds it back): workgroup 0, last -- nothing in this launch waits for these stores
  if (p.h_out && VL_WG_X == 0) {
#pragma unroll
    for (int c = 0; c < CPT; ++c)
      if (c * 512 + tid < nch) st_global_16(p.h_out + mm[c] * K + cc[c], hr[c]);
  }
  CH_STAMP(5);
