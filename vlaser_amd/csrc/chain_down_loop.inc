// Body of the LOOPED down projection: one workgroup does, for the UNITS consecutive workgroup indices VL_WG_X * UNITS + u of chain_down_kernel, what chain_down.inc does
// for one -- the same MFMA sequence per accumulator, the same 16-block and wave sums in the same order, the same single rounding.  Included where VL_WG_X is defined,
// like chain_down.inc.  What differs is the schedule: every workgroup of the stand-alone launch reads the SAME activation slices (xv depends on the wave, not on the
// column group), so here they are requested once; the weights of unit u + 1 are requested in front of unit u's MFMAs (two register sets); the waves' partial sums of
// all units go to LDS slots of their own and ONE barrier stands in front of the final phase, in which thread 16 u + t finishes what thread t of unit u's workgroup would.
// One column group per unit.
// W8: e4m3 codes (ops.pack_down4_e4m3), as chain_down.inc's W8 form reads them: a lane's 16 bytes carry its 8 codes of load 2j, then of load 2j + 1 -- NL / 2 requests per
// unit (two register sets of NL / 2), the codes become the bf16 MFMA operand in registers (ch_e4m3x8), and the column group's fp32 scales (ops.pack_down4_scales)
// multiply the reduced sum in the final phase, before the one rounding.
  static_assert(!W8 || NL % 2 == 0, "e4m3 weights: two loads per 16-byte request");
  constexpr int NR = W8 ? NL / 2 : NL;         // weight requests per unit
  static_assert(CG == 1 && UNITS >= 1 && UNITS <= 4, "looped down projection: one column group per unit, <= 4 units (64 threads of 16 finish them)");
  __shared__ __attribute__((aligned(16))) float part[UNITS][NW][RG][4][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = lane >> 2, i = lane & 3;
  const int M = p.M, u0 = VL_WG_X * UNITS;
  // ---- requests: residual (final phase: thread 16 u + t -> row t of unit u), activations (L2, once), weights of unit 0 (HBM)
  const int fr_u = min(tid >> 4, UNITS - 1), fr_row = min(tid & 15, M - 1);
  float rres[COLS];
  const bf16_t* rp = p.res + (size_t)fr_row * p.N + (u0 + fr_u) * COLS;
#pragma unroll
  for (int c = 0; c < COLS; ++c) rres[c] = bf16_to_f32(rp[c]);          // unconditional (clamped): no branch in front of the load burst
  f32x4 wsc = {1.f, 1.f, 1.f, 1.f};
  if constexpr (W8) wsc = p.w_scale[u0 + fr_u];
  u32x4 xv[RG][NL], wv[2][NR];
#pragma unroll
  for (int rg = 0; rg < RG; ++rg) {
    const bf16_t* xr = p.x + (size_t)min(rg * 4 + i, M - 1) * p.ldx + (wave * NL) * 128 + b * 8;
#pragma unroll
    for (int l = 0; l < NL; ++l) xv[rg][l] = ld_global_16(xr + l * 128);
  }
  __builtin_amdgcn_sched_barrier(0);           // activations (L2) strictly in front of the weights (HBM) in the queue
  const u32x4* src = p.W + (((size_t)u0 * NW + wave) * NR) * (16 * COLS) + b * COLS + min(i, COLS - 1);
  constexpr size_t USTRIDE = (size_t)NW * NR * (16 * COLS);      // one unit's weights: consecutive units are consecutive in memory (ops.pack_down4 / pack_down4_e4m3)
#pragma unroll
  for (int l = 0; l < NR; ++l) wv[0][l] = __builtin_nontemporal_load(src + l * (16 * COLS));
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < UNITS; ++u) {
    if (u + 1 < UNITS) {                       // (compile-time: the loop is unrolled) the next unit's requests fly while this unit's MFMAs run
#pragma unroll
      for (int l = 0; l < NR; ++l) wv[(u + 1) & 1][l] = __builtin_nontemporal_load(src + (u + 1) * USTRIDE + l * (16 * COLS));
      __builtin_amdgcn_sched_barrier(0);
    }
    f32x4 acc[RG];
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) acc[rg] = f32x4{0, 0, 0, 0};
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      u32x4 wb;
      if constexpr (W8) wb = ch_e4m3x8(wv[u & 1][l >> 1][2 * (l & 1)], wv[u & 1][l >> 1][2 * (l & 1) + 1]); else wb = wv[u & 1][l];
      const s16x4 wlo = __builtin_bit_cast(s16x4, u32x2{wb[0], wb[1]}), whi = __builtin_bit_cast(s16x4, u32x2{wb[2], wb[3]});
#pragma unroll
      for (int rg = 0; rg < RG; ++rg) {
        const s16x4 xlo = __builtin_bit_cast(s16x4, u32x2{xv[rg][l][0], xv[rg][l][1]}), xhi = __builtin_bit_cast(s16x4, u32x2{xv[rg][l][2], xv[rg][l][3]});
        acc[rg] = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(wlo, xlo, acc[rg], 0, 0, 0);
        acc[rg] = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(whi, xhi, acc[rg], 0, 0, 0);
      }
    }
    // ---- sum of the 16 blocks (lanes with equal lane & 3); the waves' sums meet in LDS
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[rg][r] = vl_blocks16_sum(acc[rg][r]);
      if (lane < 4) *reinterpret_cast<f32x4*>(&part[u][wave][rg][lane][0]) = acc[rg];       // [row i of the group][column n]
    }
    __builtin_amdgcn_sched_barrier(0);         // unit u's sums are not moved behind unit u + 1's wait for its weights
  }
  __syncthreads();
  if (tid < 16 * UNITS && (tid & 15) < M) {
    const int rg = fr_row >> 2, ri = fr_row & 3;
    float s4[4] = {0, 0, 0, 0};
#pragma unroll
    for (int w2 = 0; w2 < NW; ++w2) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(&part[fr_u][w2][rg][ri][0]);
#pragma unroll
      for (int r = 0; r < 4; ++r) s4[r] += t[r];
    }
    bf16_t* op = p.h_out + (size_t)fr_row * p.N + (u0 + fr_u) * COLS;
#pragma unroll
    for (int c = 0; c < COLS; ++c) op[c] = f32_to_bf16((W8 ? s4[c] * wsc[c] : s4[c]) + rres[c]);       // the column's scale on the reduced fp32 sum, before the first rounding
  }
