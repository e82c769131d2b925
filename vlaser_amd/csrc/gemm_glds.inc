// Body of gemm_glds_kernel: included where VL_WG_X / VL_WG_Y / VL_WG_Z (the workgroup's place in its logical grid) and VL_GRID_X / VL_GRID_Y (that grid)
// are defined -- blockIdx / gridDim in the stand-alone kernel, arguments where the body runs as part of a co-hosted launch.  The text is the kernel's, so the
// stand-alone kernel compiles to what it was.
  static_assert(!PIPE || !IFIRST, "PIPE: the refill is spread or issued behind the first read block");
  constexpr int NW = WM * WN;
  constexpr int WTM = BM / WM, WTN = BNT / WN;
  constexpr int MT = WTM / 16, NT = WTN / 16;
  constexpr int STAGE = (BM + BNT) * 128;               // bytes: A tile | W tile (row-major, 128 B = 64 k per row)
  constexpr int NPA = BM / 8, NPW = BNT / 8;             // 1 KiB (8-row) pieces of the A / W tile (WKM: 64 k-rows x 2 BNT bytes = the same count)
  constexpr int WROWB = BNT * 2, WRPP = 1024 / WROWB, WSPR = BNT / 8;      // WKM: bytes per k-row, k-rows per piece, 16-byte slots per k-row
  constexpr int AROWB = BM * 2, ARPP = 1024 / AROWB, ASPR = BM / 8;        // AKM: the same for the A tile
  static_assert(!AKM || (WKM && (BM == 128 || BM == 256)), "AKM needs WKM and a power-of-two tile of >= 16 slots per k-row");
  constexpr int PA = (NPA + NW - 1) / NW, PW = (NPW + NW - 1) / NW;     // pieces per wave per K-tile; an uneven split re-issues the last piece
  constexpr int PIECES = PA + PW;                        // (same bytes to the same LDS address: benign) so every wave's vmcnt arithmetic is identical
  static_assert(NPA * 8 == BM && NPW * 8 == BNT, "tile rows must be multiples of 8");
  static_assert(NT % 2 == 0, "fused pair epilogues need an even number of 16-column tiles per wave");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const VlaserGemmArgs& a = p.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / WN, wc = wave % WN;
  GEMM_STAMP(0)
  const int bid = xcd_remap(VL_WG_X, VL_GRID_X);
  const int tile_m = bid % p.tiles_m, tile_n = bid / p.tiles_m;
  const int m0 = tile_m * BM, n0 = tile_n * BNT;
  const int kc = a.K / (int)VL_GRID_Y;
  const int kbase = VL_WG_Y * kc;
  const int bz = VL_WG_Z;
  const bf16_t* A = reinterpret_cast<const bf16_t*>(a.A) + (size_t)bz * a.a_bs;
  const bf16_t* W = reinterpret_cast<const bf16_t*>(a.W) + (size_t)(a.w_group > 1 ? bz / a.w_group : bz) * a.w_bs;
  const int nk = kc / BK;

  // per-lane source pointers of this wave's pieces (row clamped; the swizzle lives in the source slot)
  const int prow = lane >> 3, pslot = lane & 7;
  const bf16_t* srcA[PA];
  const bf16_t* srcW[PW];
#pragma unroll
  for (int i = 0; i < PA; ++i) {
    if constexpr (AKM) {
      const int krow = min(wave * PA + i, NPA - 1) * ARPP + lane / ASPR;
      const int slot = (lane % ASPR) ^ (2 * ((krow & 3) | (((krow >> 3) & 1) << 2)));
      srcA[i] = A + (size_t)(kbase + krow) * a.lda + min(m0 + slot * 8, ((a.M + 7) & ~7) - 8);
    } else {
      const int row = min(wave * PA + i, NPA - 1) * 8 + prow;
      srcA[i] = A + (size_t)min(m0 + row, a.M - 1) * a.lda + kbase + ((pslot ^ (row & 7)) << 3);
    }
  }
#pragma unroll
  for (int i = 0; i < PW; ++i) {
    if constexpr (WKM) {
      const int krow = min(wave * PW + i, NPW - 1) * WRPP + lane / WSPR;              // k-row of this lane inside the tile
      const int slot = (lane % WSPR) ^ (2 * ((krow & 3) | (((krow >> 3) & 1) << 2)));    // logical 16-byte slot fetched into physical slot lane % WSPR
      srcW[i] = W + (size_t)(kbase + krow) * a.ldw + min(n0 + slot * 8, ((a.N + 7) & ~7) - 8);   // columns past N (chunk-aligned clamp) only feed dropped outputs
    } else {
      const int row = min(wave * PW + i, NPW - 1) * 8 + prow;
      srcW[i] = W + (size_t)min(n0 + row, a.N - 1) * a.ldw + kbase + ((pslot ^ (row & 7)) << 3);
    }
  }
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;      // LDS byte address of the stage ring (low 32 bits of the generic pointer)
  constexpr int WRING = ASYM ? NST * BM * 128 : 0;      // ASYM: [NST A stages][NST + 1 W stages]; else [NST (A | W) stages]
  // the only place that turns a piece into a source address and an LDS destination: piece i of this wave's PA (PW) pieces of the A (W) tile at K offset ko into the stage at `base`
  auto k_off = [&](int kt) { return min(kt, nk - 1) * BK; };      // tiles past the end re-fetch the last one (never read)
  auto a_stage = [&](int sa) { return lds0 + sa * (ASYM ? BM * 128 : STAGE); };
  auto w_stage = [&](int sw2) { return ASYM ? lds0 + WRING + sw2 * (BNT * 128) : lds0 + sw2 * STAGE + BM * 128; };
  auto piece_a = [&](int i, int ko, uint32_t base) { glds16(srcA[i] + (AKM ? (size_t)ko * a.lda : (size_t)ko), __builtin_amdgcn_readfirstlane(base + min(wave * PA + i, NPA - 1) * 1024)); };
  auto piece_w = [&](int i, int ko, uint32_t base) { glds16(srcW[i] + (WKM ? (size_t)ko * a.ldw : (size_t)ko), __builtin_amdgcn_readfirstlane(base + min(wave * PW + i, NPW - 1) * 1024)); };
  // piece j of the PIECES of a refill (A pieces first, then W: the order the vmcnt arithmetic assumes): A tile kta into A stage sa, W tile ktw into W stage sw2
  auto issue_piece = [&](int j, int kta, int sa, int ktw, int sw2) {
    if (j < PA) piece_a(j, k_off(kta), a_stage(sa));
    else piece_w(j - PA, k_off(ktw), w_stage(sw2));
  };
  auto issue_a = [&](int kt, int sa) {
    const int ko = k_off(kt);
    const uint32_t base = a_stage(sa);
#pragma unroll
    for (int i = 0; i < PA; ++i) piece_a(i, ko, base);
  };
  auto issue_w = [&](int kt, int sw2) {
    const int ko = k_off(kt);
    const uint32_t base = w_stage(sw2);
#pragma unroll
    for (int i = 0; i < PW; ++i) piece_w(i, ko, base);
  };
  auto issue_tile = [&](int kt, int st) { issue_a(kt, st); issue_w(kt, st); };
  // the refill of step kt as one burst: the stage(s) read in step kt - 1 (stn; ASYM: A stage stn, W stage swn) take the tiles NST - 1 (ASYM, W: NST) ahead.  (The
  // arguments by reference and the two call sites of the plain loop are the form that leaves every kernel's register allocation where it was: profiles/gemm_dedup_ab.md.)
  auto refill = [&](const int& kt, const int& stn, const int& swn) {
    if constexpr (ASYM) { issue_a(kt + NST - 1, stn); issue_w(kt + NST, swn); }
    else issue_tile(kt + NST - 1, stn);
  };

  f32x4 acc[NT][MT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[i][j] = f32x4{0, 0, 0, 0};

#pragma unroll
  for (int st = 0; st < NST - 1; ++st) issue_tile(st, st);
  if constexpr (ASYM) issue_w(NST - 1, NST - 1);
  GEMM_STAMP(1)
  const int fr = lane & 15, fq = lane >> 4;
  int st = 0;                                            // stage of tile kt (ASYM: of its A tile)
  [[maybe_unused]] int sw = 0;                           // ASYM: stage of tile kt's W tile (ring of NST + 1)
  if constexpr (PIPE) {
    auto read_frags = [&](int ks, const char* As, const char* Ws, bf16x8 (&fa)[MT], bf16x8 (&fw)[NT]) __attribute__((always_inline)) {
#pragma unroll
      for (int t = 0; t < MT; ++t) fa[t] = tile_frag<AKM ? AROWB : 0>(As, wr * WTM + t * 16, ks, fr, fq);
#pragma unroll
      for (int t = 0; t < NT; ++t) fw[t] = tile_frag<WKM ? WROWB : 0>(Ws, wc * WTN + t * 16, ks, fr, fq);
    };
    // one block of MT x NT MFMAs; `blk` = 0 / 1: first / second block of the step (the spread refill counts MFMAs over both); kt / stn / swn: the step whose refill rides here
    auto mfma_block = [&](const bf16x8 (&fa)[MT], const bf16x8 (&fw)[NT], int blk, bool refill, int kt, int stn, int swn) __attribute__((always_inline)) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          acc[nt][mt] = mfma16(fw[nt], fa[mt], acc[nt][mt]);
          if constexpr (SPREAD) {
            constexpr int GAP = (2 * MT * NT) / (PIECES + 1) > 0 ? (2 * MT * NT) / (PIECES + 1) : 1;
            const int g = blk * (MT * NT) + nt * MT + mt + 1;
            if (refill && g % GAP == 0 && g / GAP - 1 < PIECES) {
              __builtin_amdgcn_sched_barrier(0);
              issue_piece(g / GAP - 1, kt + NST - 1, stn, ASYM ? kt + NST : kt + NST - 1, ASYM ? swn : stn);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
        }
    };
    bf16x8 faA[MT], fwA[NT], faB[MT], fwB[NT];
    for (int kt = 0; kt < nk; ++kt) {
      if constexpr (ASYM) wait_vmcnt<PA * (NST - 2) + PW * (NST - 1)>();
      else wait_vmcnt<PIECES * (NST - 2)>();               // this wave's pieces of tile kt have landed (younger tiles may fly)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // set B's reads of tile kt-1 (issued a whole MFMA block ago) are retired: stage kt-1 may be refilled behind the barrier
      __builtin_amdgcn_s_barrier();
      GEMM_STAMP(2 + kt)
      int stn = st + NST - 1; if (stn >= NST) stn -= NST;
      [[maybe_unused]] int swn = sw + NST; if (swn >= NST + 1) swn -= NST + 1;
      const char* As = smem + st * (ASYM ? BM * 128 : STAGE);
      const char* Ws = ASYM ? smem + WRING + sw * (BNT * 128) : As + BM * 128;
      read_frags(0, As, Ws, faA, fwA);
      // the refill of this step: spread over the step's two MFMA blocks, or -- burst form, and ALWAYS in step 0, which has no first block -- in one piece behind the first read
      // block, in the order the vmcnt arithmetic assumes (A pieces, then W pieces)
      if (!SPREAD || kt == 0) refill(kt, stn, swn);
      if (kt > 0) mfma_block(faB, fwB, 0, SPREAD, kt, stn, swn);
      read_frags(1, As, Ws, faB, fwB);
      mfma_block(faA, fwA, 1, SPREAD && kt > 0, kt, stn, swn);
      if (++st == NST) st = 0;
      if constexpr (ASYM) { if (++sw == NST + 1) sw = 0; }
    }
    mfma_block(faB, fwB, 0, false, 0, 0, 0);               // (nk - 1, h1)
  } else
  {
  for (int kt = 0; kt < nk; ++kt) {
    if constexpr (ASYM) wait_vmcnt<PA * (NST - 2) + PW * (NST - 1)>();
    else wait_vmcnt<PIECES * (NST - 2)>();               // this wave's pieces of tile kt have landed (younger tiles may fly)
    __builtin_amdgcn_s_barrier();                        // ... and everyone else's; also: all waves are done reading stage kt-1
    GEMM_STAMP(2 + kt)
    int stn = st + NST - 1; if (stn >= NST) stn -= NST;  // = (kt-1) % NST: the stage read in the previous step
    const char* As = smem + st * (ASYM ? BM * 128 : STAGE);
    const char* Ws = ASYM ? smem + WRING + sw * (BNT * 128) : As + BM * 128;
    [[maybe_unused]] int swn = sw + NST; if (swn >= NST + 1) swn -= NST + 1;      // ASYM: = (kt - 1) % (NST + 1): the W stage read in the previous step
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 fa[MT], fw[NT];
      // (r03) the refill of stage kt-1 is issued BEHIND the first half's fragment reads: an LDS-DMA piece costs ~100-185 issue cycles
      // (MI355X_MICROARCH.md), and in front of the reads the whole K-step sat behind PIECES of them before its first ds_read went out
      if constexpr (!SPREAD) {
        if (ks == 1 && !IFIRST) refill(kt, stn, swn);
        if (ks == 0 && IFIRST) refill(kt, stn, swn);
      }
#pragma unroll
      for (int t = 0; t < MT; ++t) fa[t] = tile_frag<AKM ? AROWB : 0>(As, wr * WTM + t * 16, ks, fr, fq);
#pragma unroll
      for (int t = 0; t < NT; ++t) fw[t] = tile_frag<WKM ? WROWB : 0>(Ws, wc * WTN + t * 16, ks, fr, fq);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          acc[nt][mt] = mfma16(fw[nt], fa[mt], acc[nt][mt]);
          if constexpr (SPREAD) {
            constexpr int GAP = (2 * MT * NT) / (PIECES + 1) > 0 ? (2 * MT * NT) / (PIECES + 1) : 1;
            const int g = ks * (MT * NT) + nt * MT + mt + 1;          // MFMAs of this K-step issued so far (a compile-time value after unrolling)
            if (g % GAP == 0 && g / GAP - 1 < PIECES) {
              __builtin_amdgcn_sched_barrier(0);
              issue_piece(g / GAP - 1, kt + NST - 1, stn, ASYM ? kt + NST : kt + NST - 1, ASYM ? swn : stn);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
        }
    }
    if (++st == NST) st = 0;
    if constexpr (ASYM) { if (++sw == NST + 1) sw = 0; }
  }
  }
  GEMM_STAMP(36)
  wait_vmcnt<0>();                                       // drain the clamped look-ahead tiles before the block retires

  VlaserGemmArgs ea = a;      // batched: shift the output (bf16 / fp32 / partial) of this batch element
  if (bz > 0) {
    if (ea.out) ea.out = reinterpret_cast<char*>(ea.out) + (size_t)bz * a.o_bs * (EPI == VL_EPI_F32 ? 4 : 2);
    if (ea.out_f32) ea.out_f32 += (size_t)bz * a.o_bs;
    if (ea.res) ea.res = reinterpret_cast<const char*>(ea.res) + (size_t)bz * a.o_bs * 2;
  }
  [[maybe_unused]] char* scr = nullptr;                // this wave's scratch for the row-contiguous stores: the stage ring, once every wave is out of the K loop
  if constexpr (EPI == VL_EPI_NONE || EPI == VL_EPI_BIAS || EPI == VL_EPI_BIAS_GELU || EPI == VL_EPI_BIAS_LS_RES || EPI == VL_EPI_RES) {
    static_assert(NW * EpiScratch<MT, NT>::BYTES <= NST * STAGE + (ASYM ? BNT * 128 : 0), "epilogue scratch exceeds the stage ring");
    __builtin_amdgcn_s_barrier();                        // (each wave drained its own LDS-DMA pieces above: nothing lands in the ring any more)
    scr = smem + wave * EpiScratch<MT, NT>::BYTES;
  }
  GEMM_STAMP(37)
  if constexpr (EPI == VL_EPI_NONE && AKM) {           // the weight-gradient form: optionally this wave's share of the gradient norm (one slot per wave,
    const float ssq = epilogue_tile<EPI, MT, NT, true>(ea, m0 + wr * WTM, n0 + wc * WTN, fr, fq, acc, scr);
    if (a.sumsq_part) {
      const float w = wave_sum(ssq);
      if (lane == 0) a.sumsq_part[(size_t)(VL_WG_X + VL_GRID_X * VL_WG_Z) * NW + wave] = w;
    }
  } else {
    if constexpr (EPI == VL_EPI_SWIGLU) {                // 16-byte stores where the tile allows them
      if (epilogue_tile_swiglu<MT, NT>(ea, m0 + wr * WTM, n0 + wc * WTN, fr, fq, acc)) {
        GEMM_STAMP(38)
        return;
      }
    }
    if (!tile_epilogue<EPI, MT, NT>(ea, m0 + wr * WTM, n0 + wc * WTN, fr, fq, acc, scr)) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int m = m0 + wr * WTM + mt * 16 + fr;
        if constexpr (EPI == VL_EPI_SWIGLU) {
#pragma unroll
          for (int nt = 0; nt < NT; nt += 2) epilogue<EPI>(ea, m, n0 + wc * WTN + nt * 16 + fq * 4, acc[nt][mt], acc[nt + 1][mt]);
        } else {
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) epilogue<EPI>(ea, m, n0 + wc * WTN + nt * 16 + fq * 4, acc[nt][mt], acc[nt][mt]);
        }
      }
    }
  }
  GEMM_STAMP(38)
