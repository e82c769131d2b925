// Flash-style attention for gfx950 (bf16 in, fp32 softmax/accumulate), two kernels:
//
//  attn_prefill<HD>  : many query rows (ViT S=1025, LLM prefill).  Block = 4 waves x 16 query rows; K tile
//                      [64 keys][HD] and V^T tile [HD][64 keys] staged through XOR-swizzled LDS.
//  attn_skinny       : <=16 query tokens per (q-head, batch) over a KV cache (10 Euler steps of the action
//                      expert, greedy decode).  Block = 16 waves, one 32-key chunk per wave straight from
//                      global memory (no LDS staging), flash-decoding merge through LDS.
//
// Both compute S^T = K Q^T with the K fragment as MFMA-A (rows = keys) and Q as MFMA-B (cols = queries) so that
// every lane owns ONE query column: softmax statistics are lane-local (2 xor-shuffles per tile for the max).
// The K rows fed to tile t of a 32-key chunk are permuted (key = (i>>2)*8 + t*4 + (i&3)) so that the two
// 16-key S^T tiles of a lane concatenate into 8 CONSECUTIVE keys = exactly the MFMA-B fragment of P^T for
// O^T = V^T P^T.  V is kept TRANSPOSED in memory ([.., HD, S]) so its MFMA-A fragment is one 16-byte load.
//
// Visibility of key j for query row i (replaces the dense additive masks of the reference,
// pizero_internvl.py:517-603 and HF causal masks):   j < lim1(i)  ||  lo2 <= j < hi2
//   FULL   : lim1 = kv_len                         (ViT, modeling_intern_vit.py:220-224: no mask)
//   CAUSAL : lim1 = min(kv_len, i + 1 + causal_off)
//   PREFIX : lim1 = valid_len[b]; rows >= blk_start additionally see [blk_start, kv_len)
//   VARLEN : (vlaser_attn_varlen) n sequences back to back, row i of sequence [lo, hi) sees lo <= j <= i
#include <type_traits>
#include "common.h"
#include "chain_kernels.h"
#include "../../include/vlaser_hip.h"

#define NEG_BIG (-1.0e30f)

struct AttnP {
  VlaserAttnArgs a;
  // (r04, FULL mode only) InternViT's 1025th token: 1025 keys = 8 tiles of 128 + ONE key, 1025 queries = 16 workgroups of 64 rows + ONE row.  r03 paid a ninth
  // key tile through LDS for the one key and a 17th workgroup walking every tile for the one row: 22.5 us against 14.65 us for 1024 tokens (DESIGN lesson 29).
  int tail_key0;      // >= 0: keys [tail_key0, kv_len) (<= 32) are NOT a tile: every wave takes them as one 32-key chunk straight from global memory
  int tail_qb;        // >= 0: workgroup tail_qb holds <= 16 query rows: its 4 waves take the same rows and split the key TILES between them
  int tail_host;      // 1: there is NO workgroup tail_qb -- workgroup tail_qb - 1 of each head carries those rows as a fifth 16-row tile dealt over its 4 waves
};

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// LDS images of the K tile [64 keys][HD] and the V^T tile [HD][64 keys], 16-byte slots XOR-swizzled per row.  A ds_read_b128 is served
// 16 lanes per cycle over 64 banks, so the 16 rows one lane group touches must land on 16 different 16-byte columns of the 256-byte
// bank row: the S^T fragment's 16 lanes read key rows {0-3, 8-11, 16-19, 24-27} (+4 t) at one slot, the O^T fragment's read 16
// consecutive d rows.  With 128-byte rows two rows share a bank row (row parity picks the half), so the swizzle key must separate
// the 8 rows of equal parity; with 256-byte rows (head_dim 128) all 16.  (r01/r02 used row & 7 / row & 15: 4-way conflicts on K at
// head_dim 64, 2-way on V^T and on K at head_dim 128.)
template <int HD>
__device__ __forceinline__ int k_lds_off(int row, int slot) {
  if constexpr (HD == 128) return row * 256 + ((slot ^ ((row & 3) | (((row >> 3) & 3) << 2))) << 4);
  else return row * 128 + ((slot ^ (((row >> 1) & 1) | (((row >> 3) & 3) << 1))) << 4);
}
template <int TK>
__device__ __forceinline__ int vt_lds_off(int row, int slot) {
  if constexpr (TK == 128) return row * 256 + ((slot ^ (row & 15)) << 4);
  else return row * 128 + ((slot ^ ((row >> 1) & 7)) << 4);
}

// One 32-key chunk straight from global memory against a wave's 16 query rows (the layout of attn_skinny's chunks: K-tile t row r <-> key
// key0 + (r >> 2) * 8 + t * 4 + (r & 3)), online softmax state (m, l, o) updated in place.  Keys >= kv_len are masked; loads are clamped.
template <int HD>
struct DirectChunk {
  static constexpr int DC = HD / 32, DT = HD / 16;
  u32x4 kf[2][DC], vf[DT];
  __device__ __forceinline__ void load(const bf16_t* K, const bf16_t* VT, int key0, int kv_len, int ld_vt, int fr, int g) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = key0 + (fr >> 2) * 8 + t * 4 + (fr & 3);
#pragma unroll
      for (int dc = 0; dc < DC; ++dc) kf[t][dc] = ld_global_16(K + (size_t)min(key, kv_len - 1) * HD + dc * 32 + g * 8);
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) vf[dt] = ld_global_16(VT + (size_t)(dt * 16 + fr) * ld_vt + min(key0 + g * 8, ld_vt - 8));
  }
  __device__ __forceinline__ void process(const bf16x8 (&qf)[DC], int key0, int kv_len, float sc, int g, float& m_run, float& l_run, f32x4 (&o)[DT]) {
    f32x4 s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x4 acc = {0, 0, 0, 0};
#pragma unroll
      for (int dc = 0; dc < DC; ++dc) acc = mfma16(as_bf16x8(kf[t][dc]), qf[dc], acc);
      s[t] = acc;
    }
    float mx = NEG_BIG;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = key0 + g * 8 + t * 4 + r < kv_len ? s[t][r] * sc : NEG_BIG;
        mx = fmaxf(mx, s[t][r]);
      }
    mx = vl_xor32_max(vl_xor16_max(mx));          // (r05) permlane swaps instead of two ds_bpermute round trips in the softmax chain of every tile: same operands
    const float m_new = fmaxf(m_run, mx);
    const float alpha = fast_exp2(m_run - m_new);
    m_run = m_new;
    const float meff = fmaxf(m_new, -1.0e20f);             // nothing visible yet: exp2(-1e30 + 1e20) = 0 without a select
    float pv[8], psum = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pe = fast_exp2(s[t][r] - meff);
        psum += pe;
        pv[t * 4 + r] = pe;
      }
    l_run = l_run * alpha + psum;
    const u32x4 pk = {pack_bf16x2(pv[0], pv[1]), pack_bf16x2(pv[2], pv[3]), pack_bf16x2(pv[4], pv[5]), pack_bf16x2(pv[6], pv[7])};
    // V^T columns past the cache row's padding were clamped (duplicates of real keys): their P is exactly 0
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      f32x4 acc = o[dt];
      acc[0] *= alpha; acc[1] *= alpha; acc[2] *= alpha; acc[3] *= alpha;
      o[dt] = mfma16(as_bf16x8(vf[dt]), as_bf16x8(pk), acc);
    }
  }
};

// KS = key splits INSIDE the workgroup: KS groups of 4 waves share the 64 query rows, group j walks key tiles j, j+KS, ... through
// its own K / V^T staging buffers, and group 0 merges the (m, l, o) triples through LDS at the end (fixed order: deterministic).
// The path's prefill grids are about one 4-wave workgroup per CU (ViT: 17 x 16 = 272, joint prefill 6 x 12 = 72), i.e. one wave
// per SIMD walking a serial chain of key tiles with nothing to hide a tile's load latency behind; the split shortens the chain KS
// times and puts KS waves on every SIMD.
// TK = keys per tile (64 / 128): with about one workgroup per CU a wave is alone on its SIMD and every tile is a serial chain
// barrier -> LDS store -> barrier -> S^T -> max (two cross-lane hops) -> exp -> P V; 128-key tiles halve the number of chains
// per key and give each one twice the independent MFMA / exp work to overlap.
// DENSE (ABI 8): VL_ATTN_DENSE -- every key tile is walked and the visibility comes from a.mask (fp32, additive): the mask values of a tile ride in registers with the tile's
// K / V^T (requested one tile ahead, 4 consecutive keys = 16 bytes per score quad); its own instantiation, so the descriptor modes do not carry its registers
// VARLEN (ABI 8, varlen): block-diagonal causal attention over concatenated sequences (vlaser_attn_varlen): CAUSAL with a per-row lower limit -- row r of sequence
// [lo, hi) sees keys lo <= j <= r.  Query rows, K rows and V^T columns are all indexed by the GLOBAL row; the tiles stay on the global 64-key grid, so one sequence
// starting at row 0 walks exactly the causal schedule (same bits).  Its own instantiation.  The boundary table rides in descriptor fields CAUSAL leaves unused
// (a.valid_len = cu_seqlens [n + 1], a.n_splits = n: sequence i = rows [cu[i], cu[i + 1])), so the kernel argument block of every other instantiation is untouched.
template <int HD, int KS, int TK, bool TAIL = false, bool HOST = false, bool DENSE = false, bool VARLEN = false>      // HOST: TAIL with the tail rows hosted by the last full workgroup (p.tail_host; its own instantiation: +2 x 16 registers); TAIL: the FULL-mode tail handling (p.tail_key0 / p.tail_qb); its own instantiation, so the other shapes do not carry its registers
__device__ __forceinline__ void attn_prefill_body(const AttnP& p, const int bx, const int by, const int bz) {      // (bx, by, bz): the workgroup's place in the launch's own grid
#define VL_WG_X bx
#define VL_WG_Y by
#define VL_WG_Z bz
#define VL_GRID_X gridDim.x
#define VL_GRID_Y gridDim.y
#include "attn_prefill.inc"
#include "wg_unbind.inc"
}

// ------------------------------------------------------------------------------------------------ skinny
// <= 16 query tokens per batch element over a KV cache, GQA-aware and key-split:
//   grid (n_kv_heads, n_splits, B); block = 4 waves; rows = (q-head-in-group hg, token) pairs of ONE kv head
//   (r = hg*nq + tok, G*nq <= 32 -> two 16-row MFMA tiles), so K / V^T of a kv head are read ONCE for all its
//   q heads; split s owns a contiguous run of 32-key chunks, one chunk per wave per pass, every K and V^T
//   fragment of the chunk requested up front.  Per-CU traffic is ~1/n_splits of the cache instead of all of it.
// Output = flash-decoding partials per (b, kv head, split): m, l [32] and unnormalised o [32][128] (fp32); they are
// merged by the CONSUMER (o_proj skinny kernel, VL_PRO_ATTN prologue) -- no second launch, no atomics.
// Visibility is uniform over the rows of a batch element: keys [0, lim1) U [lo2, hi2).
#define SKA_WAVES 4
__global__ __launch_bounds__(256) void attn_skinny_kernel(AttnP p) {
  constexpr int HD = 128, DC = 4, DT = 8;
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [4 waves][ m[32] l[32] o[32][128] ] fp32
  const VlaserAttnArgs& a = p.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int kvh = blockIdx.x, split = blockIdx.y, b = blockIdx.z;
  // optional in-kernel timeline (tools/micro/chain_timeline.py): [0] start, [1] first chunk processed, [2] merge barrier passed, [3] end
  unsigned long long* dbg = a.dbg ? a.dbg + (((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 8 : nullptr;
#define STAMP(i) do { if (dbg && tid == 0) dbg[i] = wall_clock64(); } while (0)
  STAMP(0);
  const int G = a.n_q_heads / a.n_kv_heads, nq = a.sq, nrows = G * nq;
  const bf16_t* K = reinterpret_cast<const bf16_t*>(a.k) + (size_t)b * a.k_bs + (size_t)kvh * a.k_hs;
  const bf16_t* VT = reinterpret_cast<const bf16_t*>(a.vt) + (size_t)b * a.vt_bs + (size_t)kvh * a.vt_hs;

  // chunk schedule depends on kernel arguments only (not on valid_len[b]): loads never wait for that value
  const int n_chunks = (a.kv_len + 31) >> 5;
  const int cps = (n_chunks + a.n_splits - 1) / a.n_splits;
  const int c_begin = split * cps, c_end = min(n_chunks, c_begin + cps);

  bf16x8 qf[2][DC];
  int row_hi2[2];                                      // per query row: end of the visible part of the [blk_start, kv_len) block
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    // rows past nrows shadow the last real row: their loads are unconditional (a load behind `if (r < nrows)` is its own basic block
    // and made hipcc drain ALL of Q with vmcnt(0) before the first K / V^T request: one extra memory round trip per launch) and
    // their results are never stored
    const int r = min(qt * 16 + fr, nrows - 1);
    const int hg = (int)(((float)r + 0.5f) * __builtin_amdgcn_rcpf((float)nq)), tok = r - hg * nq;     // r / nq without an integer division
    row_hi2[qt] = (tok == 0 && a.first_tok_kv_len > 0) ? a.first_tok_kv_len : 0x7fffffff;
    const bf16_t* Q = reinterpret_cast<const bf16_t*>(a.q) + (size_t)b * a.q_bs + (size_t)(kvh * G + hg) * a.q_hs + (size_t)tok * a.q_ss;
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) qf[qt][dc] = as_bf16x8(ld_global_16(Q + dc * 32 + g * 8));      // unconditional (row clamped above)
  }
  int lim1 = a.kv_len, lo2 = 0x7fffffff, hi2 = 0;
  if (a.mode == VL_ATTN_PREFIX) {
    lim1 = min(a.valid_len ? vl_sload_i32(a.valid_len + b) : a.kv_len, a.kv_len);      // scalar load: not in the vmcnt queue (see vl_sload_i32)
    lo2 = a.blk_start; hi2 = a.kv_len;
  }
  f32x4 o[2][DT];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int i = 0; i < DT; ++i) o[qt][i] = f32x4{0, 0, 0, 0};
  float m_run[2] = {NEG_BIG, NEG_BIG}, l_run[2] = {0.f, 0.f};
  const float sc = a.scale * 1.4426950408889634f;

  // The wave's FIRST chunk is requested unconditionally (clamped for waves without one) in straight-line code right behind the Q
  // loads: a load inside the chunk loop sits behind hipcc's loop-header `vmcnt(0)`, i.e. K / V^T used to wait for Q's round trip.
  auto load_chunk = [&](int key0, u32x4 (&kf)[2][DC], u32x4 (&vf)[DT]) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = key0 + (fr >> 2) * 8 + t * 4 + (fr & 3);
#pragma unroll
      for (int dc = 0; dc < DC; ++dc)
        kf[t][dc] = ld_global_16(K + (size_t)min(key, a.kv_len - 1) * HD + dc * 32 + g * 8);   // clamped, unconditional: keys >= kv_len are never visible
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) vf[dt] = ld_global_16(VT + (size_t)(dt * 16 + fr) * a.ld_vt + key0 + g * 8);
  };
  auto process_chunk = [&](int key0, u32x4 (&kf)[2][DC], u32x4 (&vf)[DT]) __attribute__((always_inline)) {
    bool visk[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = key0 + g * 8 + t * 4 + r;
        visk[t][r] = (key < lim1) || (key >= lo2 && key < hi2);
      }
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      if (qt * 16 >= nrows) continue;
      bool vis[2][4];                                  // this lane's query row (fr of tile qt) x its 8 keys
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = key0 + g * 8 + t * 4 + r;
          vis[t][r] = visk[t][r] && (key < lim1 || key < row_hi2[qt]);
        }
      f32x4 s[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 acc = {0, 0, 0, 0};
#pragma unroll
        for (int dc = 0; dc < DC; ++dc) acc = mfma16(as_bf16x8(kf[t][dc]), qf[qt][dc], acc);
        s[t] = acc;
      }
      float mx = NEG_BIG;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[t][r] *= sc;
          if (vis[t][r]) mx = fmaxf(mx, s[t][r]);
        }
      mx = vl_xor32_max(vl_xor16_max(mx));
      const float m_new = fmaxf(m_run[qt], mx);
      const float alpha = fast_exp2(m_run[qt] - m_new);
      m_run[qt] = m_new;
      float pv[8], psum = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pe = vis[t][r] ? fast_exp2(s[t][r] - m_new) : 0.f;
          psum += pe;
          pv[t * 4 + r] = pe;
        }
      l_run[qt] = l_run[qt] * alpha + psum;
      u32x4 pk = {pack_bf16x2(pv[0], pv[1]), pack_bf16x2(pv[2], pv[3]), pack_bf16x2(pv[4], pv[5]), pack_bf16x2(pv[6], pv[7])};
      const bf16x8 pf = as_bf16x8(pk);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        f32x4 acc = o[qt][dt];
        acc[0] *= alpha; acc[1] *= alpha; acc[2] *= alpha; acc[3] *= alpha;
        o[qt][dt] = mfma16(as_bf16x8(vf[dt]), pf, acc);
      }
    }
  };
  {
    u32x4 kf[2][DC], vf[DT];
    const int ci0 = c_begin + wave;
    load_chunk(min(ci0, n_chunks - 1) << 5, kf, vf);          // n_chunks >= 1; the chunk's keys lie inside the padded cache row
    if (ci0 < c_end) process_chunk(ci0 << 5, kf, vf);
    if (dbg) { asm volatile("" ::"v"(o[0][0][0])); STAMP(1); }
    for (int ci = ci0 + SKA_WAVES; ci < c_end; ci += SKA_WAVES) {
      load_chunk(ci << 5, kf, vf);
      process_chunk(ci << 5, kf, vf);
    }
  }

  // in-block merge of the 4 waves through LDS, then one partial per (b, kvh, split)
  constexpr int WS = 64 + 32 * 128;
  float* wm = reinterpret_cast<float*>(smem) + wave * WS;
  const int nwa = min(SKA_WAVES, c_end - c_begin);     // waves that owned at least one chunk (block-uniform)
  if (wave < nwa) {
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    float l_tot = vl_xor32_sum(vl_xor16_sum(l_run[qt]));
    if (g == 0) { wm[qt * 16 + fr] = m_run[qt]; wm[32 + qt * 16 + fr] = l_tot; }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<f32x4*>(wm + 64 + (qt * 16 + fr) * 128 + dt * 16 + g * 4) = o[qt][dt];
  }
  }
  __syncthreads();
  STAMP(2);
  {
    const size_t pidx = ((size_t)b * a.n_kv_heads + kvh) * a.n_splits + split;
    float* PM = a.part_m + pidx * 32;
    float* PL = a.part_l + pidx * 32;
    float* PO = a.part_o + pidx * 32 * 128;
    const float* base = reinterpret_cast<const float*>(smem);
    // thread -> (row = tid / 8, 16 consecutive d = (tid % 8) * 16)
    const int row = tid >> 3, d0 = (tid & 7) * 16;
    if (row < nrows) {
      float M = NEG_BIG;
#pragma unroll
      for (int w = 0; w < SKA_WAVES; ++w)
        if (w < nwa) M = fmaxf(M, base[w * WS + row]);
      float Lsum = 0.f;
      f32x4 acc[4] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};
#pragma unroll
      for (int w = 0; w < SKA_WAVES; ++w) {
        if (w >= nwa) break;
        const float* bw = base + w * WS;
        const float f = fast_exp2(bw[row] - M);
        Lsum += bw[32 + row] * f;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const f32x4 ov = *reinterpret_cast<const f32x4*>(bw + 64 + row * 128 + d0 + q4 * 4);
          acc[q4][0] += ov[0] * f; acc[q4][1] += ov[1] * f; acc[q4][2] += ov[2] * f; acc[q4][3] += ov[3] * f;
        }
      }
      if ((tid & 7) == 0) { PM[row] = M; PL[row] = Lsum; }
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) *reinterpret_cast<f32x4*>(PO + row * 128 + d0 + q4 * 4) = acc[q4];
    }
  }
  STAMP(3);
#undef STAMP
}
template <int HD, int KS, int TK, bool TAIL = false, bool HOST = false, bool DENSE = false, bool VARLEN = false>
__global__ __launch_bounds__(256 * KS) void attn_prefill_kernel(AttnP p) {
#include "wg_bind.inc"
#include "attn_prefill.inc"
#include "wg_unbind.inc"
}

// Co-hosted launch (csrc/chain_kernels.h): the prefill attention's (query block, head) grid, its x extent lengthened; workgroups bx >= host_gx run guest workgroup
// (bx - host_gx) * gridDim.y + blockIdx.y.  Batch 1.  The launch asks for the larger of the two bodies' LDS and never less than 96 KB, so that no two of its workgroups
// share a CU: a guest lands on a CU the 72 host workgroups left idle.
template <class G, int HD, int KS, int TK>
__global__ __launch_bounds__(256 * KS) void attn_prefill_cohost_kernel(AttnP p, typename G::P gp, int host_gx) {
  static_assert(G::THREADS <= 256 * KS, "the guest's block must fit the host's");
  if ((int)blockIdx.x < host_gx) {
    attn_prefill_body<HD, KS, TK, false, false, false, false>(p, blockIdx.x, blockIdx.y, 0);
  } else {
    if constexpr (G::THREADS < 256 * KS) { if ((int)threadIdx.x >= G::THREADS) return; }
    G::run(gp, ((int)blockIdx.x - host_gx) * (int)gridDim.y + (int)blockIdx.y);
  }
}

static int attn_prefill_entry(const VlaserAttnArgs* a, const VlaserCohostGuest* guest, int* hosted, vl_stream_t s) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(s);
  VL_CHECK(a && a->q && a->k && a->vt && a->out, "vlaser_attn_prefill: null pointer");
  VL_CHECK(a->head_dim == 64 || a->head_dim == 128, "vlaser_attn_prefill: head_dim %d unsupported", a->head_dim);
  VL_CHECK(a->n_q_heads % a->n_kv_heads == 0, "vlaser_attn_prefill: GQA group mismatch");
  VL_CHECK(a->ld_vt % 64 == 0, "vlaser_attn_prefill: V^T row length must be padded to a multiple of 64 keys");
  VL_CHECK(a->kv_len <= a->ld_vt, "vlaser_attn_prefill: kv_len exceeds cache");
  VL_CHECK(a->sq > 0 && a->batch > 0, "vlaser_attn_prefill: empty");
  AttnP p; p.a = *a; p.tail_key0 = -1; p.tail_qb = -1; p.tail_host = 0;
  dim3 grid((a->sq + 63) / 64, a->n_q_heads, a->batch);
  if (a->mode == VL_ATTN_DENSE) {
    VL_CHECK(a->head_dim == 128 && a->mask && a->mask_rs % 4 == 0 && a->mask_rs >= ((a->kv_len + 63) & ~63) && (((uintptr_t)a->mask) & 15) == 0 && a->mask_bs % 4 == 0,
             "vlaser_attn_prefill: VL_ATTN_DENSE needs head_dim 128 and a 16-byte aligned fp32 mask whose row stride is a multiple of 4 >= kv_len rounded up to 64");
    constexpr int lds = 2 * 64 * 128 * 2;
    if (int rc = set_max_lds_once(attn_prefill_kernel<128, 1, 64, false, false, true>, lds)) return rc;
    hipLaunchKernelGGL((attn_prefill_kernel<128, 1, 64, false, false, true>), grid, dim3(256), lds, stream, p);
    VL_LAUNCH_CHECK();
    return 0;
  }
  // tile / split choice, measured (profiles/r02k_attn.md): a 2-way in-workgroup key split pays only when
  // the grid does not even reach one workgroup per CU (joint prefill: 72 workgroups, 11.4 -> 10.8 us); 128-key tiles only for the
  // unmasked head_dim-64 case around one workgroup per CU (ViT, 1 tile: 23.9 -> 22.8 us); more registers per wave (a forced
  // 4 waves / SIMD) and a 4-way split both lose everywhere
  const long blocks = (long)grid.x * grid.y * grid.z;
  // r03: the split is 8 % faster alone at 108 workgroups (S = 560: 14.7 vs 15.9 us) but stretches x2.5 instead of x1.5 when the SFT step's AdamW streams
  // beside it (tools/micro/contention_lab.py; whole step 23.4 -> 22.8 ms with the split off): only grids below 96 workgroups split
  int ks = blocks <= 96 ? 2 : 1;
  const int tk = (a->head_dim == 64 && a->mode == VL_ATTN_FULL && blocks <= 512 && ks == 1) ? 128 : 64;
  if (a->kv_len <= tk) ks = 1;
  if (a->mode == VL_ATTN_FULL && ks == 1) {      // (the 2-way key-split variant at head_dim 128 has no registers to spare for the tail chunk)
    const int tail = a->kv_len % tk;
    if (tail >= 1 && tail <= 32 && a->kv_len > tk) p.tail_key0 = a->kv_len - tail;
    if (a->sq % 64 >= 1 && a->sq % 64 <= 16 && a->sq > 64) p.tail_qb = a->sq / 64;
    if (p.tail_qb >= 0 && tk == 128) p.tail_host = 1;          // the one-round grids (tk == 128 <=> <= 512 workgroups); larger grids keep the tail workgroups
  }
  if (guest && hosted && a->head_dim == 128 && ks == 2 && a->batch == 1 && p.tail_key0 < 0 && p.tail_qb < 0 && !p.tail_host) {
    // the one fused instantiation: the joint prefill's attention (72 workgroups of 512 threads) + the expert's q/k/v, ONE 16-row unit (one wave) per guest workgroup --
    // the stand-alone launch's geometry, 128 workgroups on 128 of the 184 idle CUs (eight units to a CU took as long as the host: profiles/cohost_ab.md)
    typedef GuestChainQkv G;
    G::P gp;
    int units, lds_unit;
    if (vl_cohost_chain_qkv(guest, &gp.q, &units, &lds_unit)) {
      gp.units = units;
      constexpr int tile = 2 * 64 * 128 * 2, tailm = 4 * 2 * (32 + 16 * 128) * 4;      // what VL_ATTN_LAUNCH(128, 2, 64) asks for: max(KS * tile, merge, tail merge) = the tail merge's 66 560
      constexpr int host_lds = 2 * tile > tailm ? 2 * tile : tailm;
      int lds = lds_unit > host_lds ? lds_unit : host_lds;
      if (lds < 96 * 1024) lds = 96 * 1024;
      const int gwgs = vl_cohost_lab_zero_guests() ? 0 : units;
      if (int rc = set_max_lds_once(attn_prefill_cohost_kernel<G, 128, 2, 64>, lds)) return rc;
      hipLaunchKernelGGL((attn_prefill_cohost_kernel<G, 128, 2, 64>), dim3(grid.x + (gwgs + grid.y - 1) / grid.y, grid.y, 1), dim3(512), lds, stream, p, gp, (int)grid.x);
      VL_LAUNCH_CHECK();
      vl_cohost_count_fused();
      *hosted = 1;
      return 0;
    }
  }
#define VL_ATTN_LAUNCH(HD_, KS_, TK_)                                                                                       \
  do {                                                                                                                      \
    constexpr int tile = 2 * TK_ * HD_ * 2, merge = (KS_ - 1) * 4 * (HD_ / 16 * 4 + 2) * 256;                                \
    constexpr int tailm = 4 * KS_ * (32 + 16 * HD_) * 4;                                                                    \
    constexpr int lds0 = KS_ * tile > merge ? KS_ * tile : merge;                                                           \
    constexpr int lds = lds0 > tailm ? lds0 : tailm;                                                                        \
    if (p.tail_host) {                                                                                                      \
      if constexpr (HD_ == 64 && KS_ == 1 && TK_ == 128) {                                                                  \
        if (int rc = set_max_lds_once(attn_prefill_kernel<HD_, KS_, TK_, true, true>, lds)) return rc;                      \
        hipLaunchKernelGGL((attn_prefill_kernel<HD_, KS_, TK_, true, true>), dim3((grid.x - 1) * grid.y, 1, grid.z), dim3(256 * KS_), lds, stream, p); \
      }                                                                                                                     \
    } else if (p.tail_key0 >= 0 || p.tail_qb >= 0) {                                                                        \
      if constexpr (KS_ == 1) {      /* tails are only set with ks == 1 (above): the 2-way key-split variant would spill (196 B of scratch) and is not built */ \
        if (int rc = set_max_lds_once(attn_prefill_kernel<HD_, KS_, TK_, true>, lds)) return rc;                            \
        const dim3 tgrid = p.tail_qb >= 0 ? dim3(grid.x * grid.y, 1, grid.z) : grid;                                        \
        hipLaunchKernelGGL((attn_prefill_kernel<HD_, KS_, TK_, true>), tgrid, dim3(256 * KS_), lds, stream, p);             \
      }                                                                                                                     \
    } else {                                                                                                                \
      if (int rc = set_max_lds_once(attn_prefill_kernel<HD_, KS_, TK_>, lds)) return rc;                                    \
      hipLaunchKernelGGL((attn_prefill_kernel<HD_, KS_, TK_>), grid, dim3(256 * KS_), lds, stream, p);                      \
    }                                                                                                                       \
  } while (0)
#define VL_ATTN_PICK(HD_)                                                                                                   \
  do {                                                                                                                      \
    if (ks == 2) VL_ATTN_LAUNCH(HD_, 2, 64);                                                                           \
    else if (tk == 128) VL_ATTN_LAUNCH(HD_, 1, 128);                                                                        \
    else VL_ATTN_LAUNCH(HD_, 1, 64);                                                                                        \
  } while (0)
  if (a->head_dim == 128) VL_ATTN_PICK(128); else VL_ATTN_PICK(64);
#undef VL_ATTN_PICK
#undef VL_ATTN_LAUNCH
  VL_LAUNCH_CHECK();
  return 0;
}

// Block-diagonal causal attention over n_seqs concatenated sequences: the CAUSAL schedule of vlaser_attn_prefill (same tile / split choice, made from the same
// numbers) with the per-row lower limit of the VARLEN instantiations.
extern "C" int vlaser_attn_varlen(const VlaserAttnArgs* a, const int32_t* cu_seqlens, int n_seqs, vl_stream_t s) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(s);
  VL_CHECK(a && a->q && a->k && a->vt && a->out && cu_seqlens, "vlaser_attn_varlen: null pointer");
  VL_CHECK(a->head_dim == 128, "vlaser_attn_varlen: head_dim %d -- the varlen kernels are built for head_dim 128 (Qwen2.5)", a->head_dim);
  VL_CHECK(a->n_q_heads % a->n_kv_heads == 0, "vlaser_attn_varlen: GQA group mismatch");
  VL_CHECK(a->ld_vt % 64 == 0, "vlaser_attn_varlen: V^T row length must be padded to a multiple of 64 keys");
  VL_CHECK(n_seqs >= 1 && a->sq >= 1, "vlaser_attn_varlen: empty");
  VL_CHECK(a->batch == 1 && a->kv_len == a->sq, "vlaser_attn_varlen: one batch element of sq = kv_len = cu_seqlens[n_seqs] concatenated rows");
  VL_CHECK(a->sq <= a->ld_vt, "vlaser_attn_varlen: %d rows exceed the cache (%d): the key of global row r lives in cache slot r", a->sq, a->ld_vt);
  AttnP p; p.a = *a; p.tail_key0 = -1; p.tail_qb = -1; p.tail_host = 0;
  p.a.mode = VL_ATTN_CAUSAL; p.a.causal_off = 0;
  p.a.valid_len = cu_seqlens; p.a.n_splits = n_seqs;      // the VARLEN instantiations read the boundary table from these two (unused by CAUSAL)
  const dim3 grid((a->sq + 63) / 64, a->n_q_heads, 1);
  const int ks = ((long)grid.x * grid.y <= 96 && a->kv_len > 64) ? 2 : 1;      // vlaser_attn_prefill's rule for head_dim 128 / CAUSAL
  if (ks == 2) {
    constexpr int lds = 2 * (2 * 64 * 128 * 2);      // two groups' K + V^T tiles (>= the merge area, 34 816 bytes)
    if (int rc = set_max_lds_once(attn_prefill_kernel<128, 2, 64, false, false, false, true>, lds)) return rc;
    hipLaunchKernelGGL((attn_prefill_kernel<128, 2, 64, false, false, false, true>), grid, dim3(512), lds, stream, p);
  } else {
    constexpr int lds = 2 * 64 * 128 * 2;
    if (int rc = set_max_lds_once(attn_prefill_kernel<128, 1, 64, false, false, false, true>, lds)) return rc;
    hipLaunchKernelGGL((attn_prefill_kernel<128, 1, 64, false, false, false, true>), grid, dim3(256), lds, stream, p);
  }
  VL_LAUNCH_CHECK();
  return 0;
}

extern "C" int vlaser_attn_skinny(const VlaserAttnArgs* a, vl_stream_t s) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(s);
  VL_CHECK(a && a->q && a->k && a->vt, "vlaser_attn_skinny: null pointer");
  VL_CHECK(a->part_m && a->part_l && a->part_o, "vlaser_attn_skinny: partial buffers null");
  VL_CHECK(a->head_dim == 128, "vlaser_attn_skinny: head_dim must be 128");
  VL_CHECK(a->n_q_heads % a->n_kv_heads == 0, "vlaser_attn_skinny: GQA group mismatch");
  VL_CHECK(a->sq >= 1 && a->sq * (a->n_q_heads / a->n_kv_heads) <= 32, "vlaser_attn_skinny: group*tokens must be <= 32 (tokens=%d)", a->sq);
  VL_CHECK(a->ld_vt % 32 == 0 && a->kv_len <= a->ld_vt, "vlaser_attn_skinny: bad cache geometry");
  VL_CHECK(a->n_splits >= 1 && a->n_splits <= 8, "vlaser_attn_skinny: n_splits must be 1..8");
  VL_CHECK(a->mode == VL_ATTN_FULL || a->mode == VL_ATTN_PREFIX, "vlaser_attn_skinny: mode must be FULL or PREFIX");
  AttnP p; p.a = *a;
  const int lds = SKA_WAVES * (64 + 32 * 128) * 4;
  if (int rc = set_max_lds_once(attn_skinny_kernel, lds)) return rc;
  hipLaunchKernelGGL(attn_skinny_kernel, dim3(a->n_kv_heads, a->n_splits, a->batch), dim3(64 * SKA_WAVES), lds, stream, p);
  VL_LAUNCH_CHECK();
  return 0;
}

extern "C" int vlaser_attn_prefill(const VlaserAttnArgs* a, vl_stream_t s) { return attn_prefill_entry(a, nullptr, nullptr, s); }
/* vlaser_attn_prefill + a guest launch (include/vlaser_hip.h, co-hosted launches): fused where the tile choice and the guest's shape have an instantiation, host then guest otherwise */
extern "C" int vlaser_attn_prefill_cohost(const VlaserAttnArgs* a, const VlaserCohostGuest* guest, vl_stream_t s) {
  int hosted = 0;
  if (int rc = attn_prefill_entry(a, guest, &hosted, s)) return rc;
  return hosted ? 0 : vl_cohost_guest_launch(guest, s);
}
