// Body of reduce_norm_exact_kernel: included where VL_WG_X / VL_WG_Y / VL_WG_Z (the workgroup's place in its logical grid) and VL_GRID_X / VL_GRID_Y (that grid)
// are defined -- blockIdx / gridDim in the stand-alone kernel, arguments where the body runs as part of a co-hosted launch.  The text is the kernel's, so the
// stand-alone kernel compiles to what it was.
  constexpr int C = NCH * 512;
  const int lane = threadIdx.x & 63, row = VL_WG_X;
  const size_t slab = (size_t)M * C;
  f32x4 q[NCH][2 * SX];
  u32x4 hi[NCH], bv[NCH], lv[NCH], wv[NCH], nbv[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (lane + 64 * i) * 8;
    const size_t off = (size_t)row * C + c;
#pragma unroll
    for (int u = 0; u < SX; ++u) {
      const float* pp = partials + off + (size_t)u * slab;
      q[i][2 * u] = *reinterpret_cast<const f32x4*>(pp);
      q[i][2 * u + 1] = *reinterpret_cast<const f32x4*>(pp + 4);
    }
    hi[i] = ld_global_16(h_in + off);
    if constexpr (BL) { bv[i] = ld_global_16(bias + c); lv[i] = ld_global_16(ls + c); }
    if constexpr (NORM != 0) wv[i] = ld_global_16(nw + c);
    if constexpr (NORM == 2) nbv[i] = ld_global_16(nb + c);
  }
  u32x4 hv[NCH];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < SX; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[j] += q[i][2 * u][j]; v[4 + j] += q[i][2 * u + 1][j]; }
    u32x4 hr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float lo = v[2 * j], hi2 = v[2 * j + 1];
      if constexpr (BL) {
        lo = (lo + bf16lo_to_f32(bv[i][j])) * bf16lo_to_f32(lv[i][j]);
        hi2 = (hi2 + bf16hi_to_f32(bv[i][j])) * bf16hi_to_f32(lv[i][j]);
      }
      hr[j] = pack_bf16x2(bf16lo_to_f32(hi[i][j]) + lo, bf16hi_to_f32(hi[i][j]) + hi2);
      const float a0 = bf16lo_to_f32(hr[j]), a1 = bf16hi_to_f32(hr[j]);
      s1 += a0 + a1;
      s2 += a0 * a0 + a1 * a1;
    }
    hv[i] = hr;
    st_global_16(h_out + (size_t)row * C + (lane + 64 * i) * 8, hr);
  }
  if constexpr (NORM == 0) return;
  s1 = wave_sum(s1);
  float mean = 0.f, rs;
  if constexpr (NORM == 1) {
    rs = rsqrtf(wave_sum(s2) / (float)C + eps);
  } else {
    mean = s1 / (float)C;
    float vs = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float a0 = bf16lo_to_f32(hv[i][j]) - mean, a1 = bf16hi_to_f32(hv[i][j]) - mean;
        vs += a0 * a0 + a1 * a1;
      }
    rs = rsqrtf(wave_sum(vs) / (float)C + eps);
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    u32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float lo, hi2;
      if constexpr (NORM == 1) {
        lo = round_bf16(bf16lo_to_f32(hv[i][j]) * rs) * bf16lo_to_f32(wv[i][j]);
        hi2 = round_bf16(bf16hi_to_f32(hv[i][j]) * rs) * bf16hi_to_f32(wv[i][j]);
      } else {
        lo = (bf16lo_to_f32(hv[i][j]) - mean) * rs * bf16lo_to_f32(wv[i][j]) + bf16lo_to_f32(nbv[i][j]);
        hi2 = (bf16hi_to_f32(hv[i][j]) - mean) * rs * bf16hi_to_f32(wv[i][j]) + bf16hi_to_f32(nbv[i][j]);
      }
      o[j] = pack_bf16x2(lo, hi2);
    }
    st_global_16(x_out + (size_t)row * C + (lane + 64 * i) * 8, o);
  }
