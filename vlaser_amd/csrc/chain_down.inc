// Body of chain_down_kernel: included where VL_WG_X / VL_WG_Y / VL_WG_Z (the workgroup's place in its logical grid) and VL_GRID_X / VL_GRID_Y (that grid)
// are defined -- blockIdx / gridDim in the stand-alone kernel, arguments where the body runs as part of a co-hosted launch.  The text is the kernel's, so the
// stand-alone kernel compiles to what it was.
  static_assert(NL % 2 == 0, "e4m3 weights: two loads per 16-byte request");
  constexpr int NR = W8 ? NL / 2 : NL;         // weight requests per column group
  __shared__ __attribute__((aligned(16))) float part[NW][CG][RG][4][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = lane >> 2, i = lane & 3;
  const int M = p.M, n0 = VL_WG_X * (COLS * CG);
  unsigned long long* dbg = DBG ? p.dbg + (size_t)VL_WG_X * 8 : nullptr;
  CH_STAMP(0);
  // ---- requests: residual (final phase: thread t -> row t / CG... see below), activations (L2), weights (HBM)
  const int fr_row = min(tid / CG, M - 1), fr_cg = tid % CG;            // final phase: thread t < M * CG finishes row t / CG of column group t % CG
  float rres[COLS];
  const bf16_t* rp = p.res + (size_t)fr_row * p.N + n0 + fr_cg * COLS;
#pragma unroll
  for (int c = 0; c < COLS; ++c) rres[c] = bf16_to_f32(rp[c]);          // unconditional (clamped): no branch in front of the load burst
  f32x4 wsc = {1.f, 1.f, 1.f, 1.f};
  if constexpr (W8) wsc = p.w_scale[VL_WG_X * CG + fr_cg];
  u32x4 xv[RG][NL], wv[CG][NR];
#pragma unroll
  for (int rg = 0; rg < RG; ++rg) {
    const bf16_t* xr = p.x + (size_t)min(rg * 4 + i, M - 1) * p.ldx + (wave * NL) * 128 + b * 8;
#pragma unroll
    for (int l = 0; l < NL; ++l) xv[rg][l] = ld_global_16(xr + l * 128);
  }
  __builtin_amdgcn_sched_barrier(0);           // activations (L2) strictly in front of the weights (HBM) in the queue
  {
    const u32x4* src = p.W + (((size_t)VL_WG_X * NW + wave) * NR) * (CG * 16 * COLS) + b * COLS + min(i, COLS - 1);
#pragma unroll
    for (int l = 0; l < NR; ++l)
#pragma unroll
      for (int c = 0; c < CG; ++c) wv[c][l] = __builtin_nontemporal_load(src + (l * CG + c) * (16 * COLS));
  }
  __builtin_amdgcn_sched_barrier(0);
  f32x4 acc[CG][RG];
#pragma unroll
  for (int c = 0; c < CG; ++c)
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) acc[c][rg] = f32x4{0, 0, 0, 0};
#pragma unroll
  for (int l = 0; l < NL; ++l) {
#pragma unroll
    for (int c = 0; c < CG; ++c) {
      u32x4 wb;
      if constexpr (W8) wb = ch_e4m3x8(wv[c][l >> 1][2 * (l & 1)], wv[c][l >> 1][2 * (l & 1) + 1]); else wb = wv[c][l];
      const s16x4 wlo = __builtin_bit_cast(s16x4, u32x2{wb[0], wb[1]}), whi = __builtin_bit_cast(s16x4, u32x2{wb[2], wb[3]});
#pragma unroll
      for (int rg = 0; rg < RG; ++rg) {
        const s16x4 xlo = __builtin_bit_cast(s16x4, u32x2{xv[rg][l][0], xv[rg][l][1]}), xhi = __builtin_bit_cast(s16x4, u32x2{xv[rg][l][2], xv[rg][l][3]});
        acc[c][rg] = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(wlo, xlo, acc[c][rg], 0, 0, 0);
        acc[c][rg] = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(whi, xhi, acc[c][rg], 0, 0, 0);
      }
    }
  }
  if constexpr (DBG) asm volatile("" ::"v"(acc[0][0][0]));
  CH_STAMP(3);
  // ---- sum of the 16 blocks (lanes with equal lane & 3), then of the waves
#pragma unroll
  for (int c = 0; c < CG; ++c)
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[c][rg][r] = vl_blocks16_sum(acc[c][rg][r]);
      if (lane < 4) *reinterpret_cast<f32x4*>(&part[wave][c][rg][lane][0]) = acc[c][rg];       // [row i of the group][column n]
    }
  __syncthreads();
  CH_STAMP(4);
  if (tid < M * CG) {
    const int rg = fr_row >> 2, ri = fr_row & 3;
    float s4[4] = {0, 0, 0, 0};
#pragma unroll
    for (int w2 = 0; w2 < NW; ++w2) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(&part[w2][fr_cg][rg][ri][0]);
#pragma unroll
      for (int r = 0; r < 4; ++r) s4[r] += t[r];
    }
    bf16_t* op = p.h_out + (size_t)fr_row * p.N + n0 + fr_cg * COLS;
#pragma unroll
    for (int c = 0; c < COLS; ++c) op[c] = f32_to_bf16((W8 ? s4[c] * wsc[c] : s4[c]) + rres[c]);       // the column's scale on the reduced fp32 sum, before the first rounding
  }
  CH_STAMP(5);
