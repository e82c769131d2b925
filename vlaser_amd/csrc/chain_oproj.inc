// Body of chain_oproj_kernel: included where VL_WG_X / VL_WG_Y / VL_WG_Z (the workgroup's place in its logical grid) and VL_GRID_X / VL_GRID_Y (that grid)
// are defined -- blockIdx / gridDim in the stand-alone kernel, arguments where the body runs as part of a co-hosted launch.  The text is the kernel's, so the
// stand-alone kernel compiles to what it was.
  constexpr int KB = NS * 256, cpr = KB / 8, XS = KB * 2 + 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, g = lane >> 4;
  const int unit = VL_WG_X, ks = VL_WG_Y, M = p.M;
  unsigned long long* dbg = DBG ? p.dbg + ((size_t)VL_WG_Y * VL_GRID_X + VL_WG_X) * 8 : nullptr;
  CH_STAMP(0);
  const int xs_bytes = (M * XS + 15) & ~15;
  char* xs = smem;
  float* red = reinterpret_cast<float*>(smem + xs_bytes);        // [7][64] f32x4
  const int nch = M * cpr;
  const int ch = min(tid, nch - 1);
  const int mm = ch_fdiv(ch, p.inv_cpr), j = ch - mm * cpr;
  const int k = ks * KB + j * 8, h = k >> 7, d = k & 127;
  const int b = ch_fdiv(mm, __builtin_amdgcn_rcpf((float)p.nq)), tok = mm - b * p.nq, kvh = ch_fdiv(h, __builtin_amdgcn_rcpf((float)p.G)), hg = h - kvh * p.G,
            r = hg * p.nq + tok;
  const int nsp = (S == 7) ? 7 : p.n_splits;
  const size_t pbase = ((size_t)b * p.nkv + kvh) * nsp;
  f32x2_t ml[S];
  u32x4 ov[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int sc = (S == 7) ? s : min(s, nsp - 1);
    ml[s] = *reinterpret_cast<const f32x2_t*>(p.pml + ((pbase + sc) * 32 + r) * 2);
    ov[s] = ld_global_16(p.po + ((pbase + sc) * 32 + r) * 128 + d);
  }
  __builtin_amdgcn_sched_barrier(0);
  u32x4 w[NS];
  {
    const u32x4* src = p.W + (((size_t)ks * p.n_units + unit) * 8 + wave) * (NS * 64) + lane;
#pragma unroll
    for (int f = 0; f < NS; ++f) w[f] = __builtin_nontemporal_load(src + f * 64);
  }
  __builtin_amdgcn_sched_barrier(0);
  // ---- x[m][k] = sum_s w_s o_s / sum_s w_s,  w_s = l_s 2^(m_s - max m)
  float Mx = -1.0e30f;
#pragma unroll
  for (int s = 0; s < S; ++s) Mx = fmaxf(Mx, ml[s][0]);
  float Ls = 0.f, v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < S; ++s) {
    float f = ml[s][1] * __builtin_amdgcn_exp2f(ml[s][0] - Mx);
    if (S != 7) f = s < nsp ? f : 0.f;
    Ls += f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[2 * e] += f * bf16lo_to_f32(ov[s][e]); v[2 * e + 1] += f * bf16hi_to_f32(ov[s][e]); }
  }
  const float inv = Ls > 0.f ? 1.0f / Ls : 0.f;
  if (tid < nch) *reinterpret_cast<u32x4*>(xs + mm * XS + j * 16) = u32x4{pack_bf16x2(v[0] * inv, v[1] * inv), pack_bf16x2(v[2] * inv, v[3] * inv), pack_bf16x2(v[4] * inv, v[5] * inv), pack_bf16x2(v[6] * inv, v[7] * inv)};
  // more than 512 pieces (decode batches of 6 .. 16 rows): the remaining ones in further passes of the same arithmetic, their requests no longer up front (one exposed L2 round
  // trip per pass; never taken by the Euler phase or the batch-1 decode)
  for (int c2 = tid + 512; c2 < nch; c2 += 512) {
    const int mm2 = ch_fdiv(c2, p.inv_cpr), j2 = c2 - mm2 * cpr;
    const int k2 = ks * KB + j2 * 8, h2 = k2 >> 7, d2 = k2 & 127;
    const int b2 = ch_fdiv(mm2, __builtin_amdgcn_rcpf((float)p.nq)), tok2 = mm2 - b2 * p.nq, kvh2 = ch_fdiv(h2, __builtin_amdgcn_rcpf((float)p.G)), r2 = (h2 - kvh2 * p.G) * p.nq + tok2;
    const size_t pb2 = ((size_t)b2 * p.nkv + kvh2) * nsp;
    f32x2_t ml2[S];
    u32x4 ov2[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const int sc = (S == 7) ? s : min(s, nsp - 1);
      ml2[s] = *reinterpret_cast<const f32x2_t*>(p.pml + ((pb2 + sc) * 32 + r2) * 2);
      ov2[s] = ld_global_16(p.po + ((pb2 + sc) * 32 + r2) * 128 + d2);
    }
    float Mx2 = -1.0e30f;
#pragma unroll
    for (int s = 0; s < S; ++s) Mx2 = fmaxf(Mx2, ml2[s][0]);
    float Ls2 = 0.f, v2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < S; ++s) {
      float f = ml2[s][1] * __builtin_amdgcn_exp2f(ml2[s][0] - Mx2);
      if (S != 7) f = s < nsp ? f : 0.f;
      Ls2 += f;
#pragma unroll
      for (int e = 0; e < 4; ++e) { v2[2 * e] += f * bf16lo_to_f32(ov2[s][e]); v2[2 * e + 1] += f * bf16hi_to_f32(ov2[s][e]); }
    }
    const float inv2 = Ls2 > 0.f ? 1.0f / Ls2 : 0.f;
    *reinterpret_cast<u32x4*>(xs + mm2 * XS + j2 * 16) = u32x4{pack_bf16x2(v2[0] * inv2, v2[1] * inv2), pack_bf16x2(v2[2] * inv2, v2[3] * inv2), pack_bf16x2(v2[4] * inv2, v2[5] * inv2), pack_bf16x2(v2[6] * inv2, v2[7] * inv2)};
  }
  __syncthreads();
  CH_STAMP(2);
  const bool mok = fr < M;
  const char* xrow = xs + (mok ? fr : 0) * XS + (wave * (NS * 32) + g * 8) * 2;
  f32x4 acc = {0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < NS; ++s) acc = mfma16(as_bf16x8(w[s]), as_bf16x8(*reinterpret_cast<const u32x4*>(xrow + s * 64)), acc);
  if constexpr (DBG) asm volatile("" ::"v"(acc[0]));
  CH_STAMP(3);
  if (wave != 0) *reinterpret_cast<f32x4*>(red + ((wave - 1) * 64 + lane) * 4) = acc;
  __syncthreads();
  CH_STAMP(4);
  if (wave == 0) {
#pragma unroll
    for (int w2 = 0; w2 < 7; ++w2) acc += *reinterpret_cast<const f32x4*>(red + (w2 * 64 + lane) * 4);
    if (mok) *reinterpret_cast<f32x4*>(p.out + ((size_t)ks * M + fr) * p.N + unit * 16 + g * 4) = acc;
  }
  CH_STAMP(5);
