// The device side of csrc/chain.hip: the parameter structs and the kernel bodies of the <= 16-row layer-step chain, as __device__ functions of (parameters, logical
// workgroup index) so that a body can also run as the extra workgroups of another kernel's launch (the co-hosted launches of csrc/gemm.hip, csrc/misc.hip and csrc/attn.hip:
// a prefill launch whose single-round grid leaves CUs idle carries the action expert's launch of Euler step 0 behind its own workgroups).  The stand-alone __global__
// kernels are thin wrappers that pass blockIdx; a body never reads blockIdx, gridDim or blockDim itself.
#pragma once
#include "common.h"
#include "../../include/vlaser_hip.h"

typedef __attribute__((ext_vector_type(4))) short s16x4;

#define CH_STAMP(i) do { if constexpr (DBG) { if (threadIdx.x == 0) dbg[i] = wall_clock64(); } } while (0)

__device__ __forceinline__ int ch_fdiv(int x, float inv_d) { return (int)(((float)x + 0.5f) * inv_d); }

// W8 forms (ops.quantize_rows_e4m3): the MLP weights arrive as OCP e4m3 codes, one byte each, and become the bf16 MFMA operand in registers -- every finite e4m3 value is
// exact in bf16, so the MFMAs, their order and the reductions are those of the bf16 form; the row's fp32 scale multiplies the reduced sum once, in the epilogue.
// Two dwords = 8 codes in memory order -> the 8 bf16 of one 16-byte bf16 fragment.
typedef __attribute__((ext_vector_type(2))) __bf16 ch_bf16x2;
__device__ __forceinline__ uint32_t ch_e4m3x2_lo(uint32_t c) { return __builtin_bit_cast(uint32_t, (ch_bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c, 1.0f, false)); }
__device__ __forceinline__ uint32_t ch_e4m3x2_hi(uint32_t c) { return __builtin_bit_cast(uint32_t, (ch_bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c, 1.0f, true)); }
__device__ __forceinline__ u32x4 ch_e4m3x8(uint32_t c0, uint32_t c1) { return u32x4{ch_e4m3x2_lo(c0), ch_e4m3x2_hi(c0), ch_e4m3x2_lo(c1), ch_e4m3x2_hi(c1)}; }

// ------------------------------------------------------------------------------------------------------------------ gate / up
struct ChainGuP {
  const bf16_t* h_in; const float* partials; const bf16_t* norm_w; bf16_t* h_out;
  const u32x4* W; bf16_t* out;
  const float* w_scale;                 // W8: fp32 [units * 16], packed row order
  int M, ldo, ulo, urem, n_valid;
  float eps, inv_cpr;
  unsigned long long* dbg;
};

// NS = K / 256 (K-steps of 32 per wave), UE = units per workgroup, SP = split-K slabs of the producer, CPT = 16-byte chunks of the [M, K] residual stream per thread
// (ceil(M * K / 8 / 512)), TPU = MFMA tiles per unit: 2 = 32 packed rows [gate16 | up16] (ops.pack_gate_up), 1 = 16 rows whose lane group g holds
// [gate 2g, gate 2g+1, up 2g, up 2g+1] of the unit's 8 activation columns (ops.pack_gate_up8: 1120 instead of 560 units -> 224 workgroups x 5 instead of 187 x 3)
// W8: the unit's weights as e4m3 codes (ops.pack_gate_up8_e4m3).  K = 768 leaves a wave 3 K-steps = 24 bytes per lane and unit: ONE 16-byte load carries the lane's
// fragments of K-steps 0 and 1, ONE 8-byte load the fragment of K-step 2 (a wave's unit = 64 x 16 bytes, then 64 x 8 bytes: 1536 contiguous bytes) -- two requests per
// unit instead of three, the same (row, k) elements in every lane, consumed in the same order.  K = 1536 (the Vlaser-2B LLM) leaves a wave 6 K-steps = 48 bytes per lane
// and unit: THREE 16-byte loads, load j the lane's fragments of K-steps 2j and 2j + 1 (a wave's unit = [j][lane][16 bytes] = 3072 contiguous bytes), no 8-byte tail;
// w[UE][3] = 60 VGPRs at UE = 5 against the bf16 form's 120.
template <int NS, int UE, int SP, int CPT, int TPU, bool DBG, bool W8 = false>
__device__ __forceinline__ void chain_gu_body(const ChainGuP& p, const int wg) {
#define VL_WG_X wg
#define VL_WG_Y 0
#define VL_WG_Z 0
#define VL_GRID_X 1
#define VL_GRID_Y 1
#include "chain_gu.inc"
#include "wg_unbind.inc"
}
template <int NS, int UE, int SP, int CPT, int TPU, bool DBG, bool W8 = false>
__global__ __launch_bounds__(512) void chain_gu_kernel(ChainGuP p) {
#include "wg_bind.inc"
#include "chain_gu.inc"
#include "wg_unbind.inc"
}

// ------------------------------------------------------------------------------------------------------------------ q / k / v
struct ChainQkvP {
  const bf16_t* h_in; const float* partials; bf16_t* h_out; const bf16_t* norm_w; const u32x4* W; const bf16_t* bias;      // (partials, h_out: unread -- without them hipcc fetches the
                                                                                                                          // arguments in other pieces and schedules the prologue differently)
  bf16_t* q_out; bf16_t* k_cache; bf16_t* vt_cache; const float* rope_cos; const float* rope_sin; const int32_t* pos_ids;
  int M, n_q_heads, n_kv_heads, s_max, tok_per_batch, slot_base;
  float eps;
  unsigned long long* dbg;
};

// KS = K / 32 K-steps (24: hidden 768, 48: hidden 1536), RG = ceil(M / 4) row groups of the norm prologue.  One wave = one 16-row unit of the fused q/k/v
// matrix (head_perm16 packing: lane group g of a unit holds [d, d+1, d+64, d+65], d = 8 (unit % 8) + 2 g -- the RoPE partner of every value in the same lane).
// h_in is the residual stream itself (already reduced and rounded: the action encoder's output, or what vlaser_chain_down published).
// NWV = 2 (hidden 1536, the greedy decode): two waves per unit, each over one K half -- 24 weight requests and 24 dependent MFMAs per wave instead of 48 (6.6 -> 5.x us per
// launch); both waves load the whole row (3 KB from L2) for the row's sum of squares and normalise their own half into their own LDS rows (still wave-local); wave 1 hands its
// accumulator to wave 0 through LDS (the launch's only barrier).
template <int KS, int RG, int NWV, bool DBG>
__device__ __forceinline__ void chain_qkv_body(const ChainQkvP& p, const int unit_) {
#define VL_WG_X unit_
#define VL_WG_Y 0
#define VL_WG_Z 0
#define VL_GRID_X 1
#define VL_GRID_Y 1
#include "chain_qkv.inc"
#include "wg_unbind.inc"
}
template <int KS, int RG, int NWV, bool DBG>
__global__ __launch_bounds__(64 * NWV) void chain_qkv_kernel(ChainQkvP p) {
#include "wg_bind.inc"
#include "chain_qkv.inc"
#include "wg_unbind.inc"
}

// ------------------------------------------------------------------------------------------------------------------ down projection
struct ChainDownP {
  const bf16_t* x; const u32x4* W; const bf16_t* res; bf16_t* h_out; float* out_f32;      // (out_f32: unread, kept so that the kernel arguments stay where the measured kernels fetch them)
  int M, N, ldx;
  unsigned long long* dbg;
  const f32x4* w_scale;       // W8: fp32 [N / cols][4], the scales of a column group (the fourth repeats the third where cols = 3: ops.pack_down4_scales)
};

// A workgroup = CG groups of COLS (3 or 4) output columns over the WHOLE K = NW waves x NL loads x 128.  Lane (b = lane >> 2, i = lane & 3) of wave w, load l, group c
// holds W[n0 + c COLS + min(i, COLS - 1)][(w NL + l) 128 + 8 b .. + 8] (ops.pack_down4: one contiguous 16 x COLS x 16 bytes per wave-level load; with COLS = 3 the
// fourth lane of a block re-reads the third's 16 bytes) and x[row i of its row group][same k]; the two halves of the 16 bytes feed two v_mfma_f32_4x4x4_16b_bf16
// (layout probed on the GPU, tools/micro/mfma4_probe.hip: D[reg = lane & 3 of the A lane][lane of the B lane]; block b: D_b[n][m] += sum_k W[n0 + n][k] x[m][k] over
// 4 k): lane (b, m) accumulates out[m][n0 .. n0 + COLS) over its block's k, the 16 blocks are summed across the lanes, the NW waves through LDS in a fixed order.
// COLS = 3 puts N = 768 on 256 workgroups: a CU sustains ~35 GB/s of requests, so the launch lasts as long as the bytes of its busiest CU -- 54 KB of weights + the
// whole [M, K] activation (every workgroup contracts over all of K: the price of publishing the result once) instead of 72 + 71 KB on 192 CUs.
// RG = ceil(M / 4) row groups.
// W8: e4m3 codes (ops.pack_down4_e4m3): a lane's 16 bytes carry its 8 codes of load 2j, then its 8 codes of load 2j + 1 -- NL / 2 requests per group of the same
// 16 x COLS x 16-byte shape, the same (column, k) elements in every lane, consumed in the same order.
template <int NW, int NL, int RG, int COLS, int CG, bool DBG, bool W8 = false>
__device__ __forceinline__ void chain_down_body(const ChainDownP& p, const int wg) {
#define VL_WG_X wg
#define VL_WG_Y 0
#define VL_WG_Z 0
#define VL_GRID_X 1
#define VL_GRID_Y 1
#include "chain_down.inc"
#include "wg_unbind.inc"
}
template <int NW, int NL, int RG, int COLS, int CG, bool DBG, bool W8 = false>
__global__ __launch_bounds__(NW * 64) void chain_down_kernel(ChainDownP p) {
#include "wg_bind.inc"
#include "chain_down.inc"
#include "wg_unbind.inc"
}

// The looped form (chain_down_loop.inc): workgroup wg does the work of the stand-alone launch's workgroups wg * UNITS .. + UNITS - 1 -- the activation slices, which
// every one of those reads alike, requested once, the weights of unit u + 1 in flight under unit u's MFMAs.  Built for a launch that has few CUs to itself: the guest of
// the joint prefill's q/k/v GEMM (GuestChainDown4 below: 64 idle CUs, one workgroup each because the fused launch carries the host's 128 KB LDS request; four rounds of
// the stand-alone geometry there would outlast the host).  Bit-identical to chain_down_kernel in the same weight format (W8: the e4m3 codes of ops.pack_down4_e4m3, half the requests per unit); CG = 1.
template <int NW, int NL, int RG, int COLS, int CG, int UNITS, bool W8 = false>
__device__ __forceinline__ void chain_down_loop_body(const ChainDownP& p, const int wg) {
#define VL_WG_X wg
#include "chain_down_loop.inc"
#include "wg_unbind.inc"
}
template <int NW, int NL, int RG, int COLS, int CG, int UNITS, bool W8 = false>
__global__ __launch_bounds__(NW * 64) void chain_down_loop_kernel(ChainDownP p) {      // the looped body on its own (vlaser_chain_down_looped / _looped_w8: tests, tools)
#include "wg_bind.inc"
#include "chain_down_loop.inc"
#include "wg_unbind.inc"
}

// ------------------------------------------------------------------------------------------------------------------ attention over the KV cache, <= 16 query tokens
// One WAVE per (kv head, key split, 16-row tile, batch element), NC 32-key chunks each, no LDS, no barrier: Q of the tile's (q head, token) rows (the kv head has
// <= 32 rows = two MFMA tiles), then K and V^T of every chunk of the wave are requested in one burst (vlaser_attn_skinny staged the same work through 4-wave workgroups whose merge
// through LDS was 1.0 us of its 6.1 us, and its vector load of valid_len[b] put an `s_waitcnt vmcnt(0)` -- a second full round trip -- between the Q and the K / V^T
// requests).  A split leaves (m, l) fp32 and its NORMALISED output rows in bf16 (half the bytes of the fp32 partials for the 144 workgroups of the o_proj launch
// that each merge the splits of their K range); chain_oproj weights them by l 2^(m - max m).
struct ChainAttnP {
  const bf16_t* q; const bf16_t* k; const bf16_t* vt;
  float* pml; bf16_t* po;
  const int32_t* valid_len;
  long long q_bs, q_hs, q_ss, k_bs, k_hs, vt_bs, vt_hs;
  int sq, kv_len, G, ld_vt, mode, blk_start, first_tok_kv_len, n_splits, n_kv;
  int tile_sh;                                        // 1: grid.y = 2 split + row tile (one wave per 16-row tile), 0: grid.y = split
  float scale;
  unsigned long long* dbg;
  const float* mask; long long mask_bs, mask_rs;      // VL_ATTN_DENSE (ABI 8): fp32 additive mask, row = query TOKEN (the same for every head)
};

// DENSE: the visibility and a bias per (token, key) come from p.mask instead of the (valid_len, blk_start) descriptors; requested with the K / V^T of the chunks
// QT: the 16-row tiles a wave walks.  No row reads another row's result, so with more than 16 rows the launch gives every tile a wave of its own (QT = 1, grid.y =
// 2 splits + tile: the two waves of a split are neighbours and request the same K / V^T) instead of running the second tile's chain behind the first's; with
// <= 16 rows (a greedy decode step) the second tile has no row and is not computed.
template <int NC, int QT, bool DBG, bool DENSE = false>
__device__ __forceinline__ void chain_attn_body(const ChainAttnP& p, const int bx, const int by, const int bz, const int gx, const int gy) {      // a block of ONE wave
#define VL_WG_X bx
#define VL_WG_Y by
#define VL_WG_Z bz
#define VL_GRID_X gx
#define VL_GRID_Y gy
#include "chain_attn.inc"
#include "wg_unbind.inc"
}
template <int NC, int QT, bool DBG, bool DENSE = false>
__global__ __launch_bounds__(64) void chain_attn_kernel(ChainAttnP p) {
#include "wg_bind.inc"
#include "chain_attn.inc"
#include "wg_unbind.inc"
}

// ------------------------------------------------------------------------------------------------------------------ o_proj: merge of the attention splits -> GEMV -> split-K slabs
struct ChainOprojP {
  const float* pml; const bf16_t* po; const u32x4* W; float* out;
  int M, N, n_units, G, nq, nkv, n_splits;
  float inv_cpr;
  unsigned long long* dbg;
};

// grid (N / 16 units, ks K-splits); NS = K / (ks * 256) K-steps per wave; the K range of a workgroup = whole heads.  S = attention splits REQUESTED (all up front): the
// launch has p.n_splits <= S of them (the Euler phase exactly 7 = its S; a decode step over kvmax keys 8..16) -- the requests beyond re-read the last split and get weight 0
template <int NS, int S, bool DBG>
__device__ __forceinline__ void chain_oproj_body(const ChainOprojP& p, const int bx, const int by, const int gx) {
#define VL_WG_X bx
#define VL_WG_Y by
#define VL_WG_Z 0
#define VL_GRID_X gx
#define VL_GRID_Y 1
#include "chain_oproj.inc"
#include "wg_unbind.inc"
}
template <int NS, int S, bool DBG>
__global__ __launch_bounds__(512) void chain_oproj_kernel(ChainOprojP p) {
#include "wg_bind.inc"
#include "chain_oproj.inc"
#include "wg_unbind.inc"
}

// ------------------------------------------------------------------------------------------------------------------ co-hosted launches: the guest side
// A guest = the body of one chain kernel at the shape of Euler step 0 of a batch-1 chunk (5 rows: the proprio token + 4 action tokens), run by the workgroups that a
// prefill kernel's launch carries BEHIND its own (blockIdx.x >= host_grid).  P = the stand-alone kernel's parameters, THREADS = its block, run(p, gwg) = what guest
// workgroup gwg does.  The fused kernel's block is the larger of the two bodies'; the waves a body does not have return at once (a terminated wave no longer counts at
// s_barrier).  Host and guest never read what the other writes: the launch boundaries in front of and behind the fused launch order everything, as they did before.
struct GuestChainGu {
  typedef ChainGuP P;
  static constexpr int THREADS = 512;
  static __device__ __forceinline__ void run(const P& p, int gwg) { chain_gu_body<3, 5, 3, 1, 1, false>(p, gwg); }
};
struct GuestChainGuW8 {          // the e4m3 forms (an 'mlp8' expert): the stand-alone W8 kernels' bodies at the same shapes
  typedef ChainGuP P;
  static constexpr int THREADS = 512;
  static __device__ __forceinline__ void run(const P& p, int gwg) { chain_gu_body<3, 5, 3, 1, 1, false, true>(p, gwg); }
};
struct GuestChainOproj {
  typedef ChainOprojP P;
  static constexpr int THREADS = 512;
  static __device__ __forceinline__ void run(const P& p, int gwg) {
    const int ks = ch_fdiv(gwg, __builtin_amdgcn_rcpf((float)p.n_units));
    chain_oproj_body<2, 7, false>(p, gwg - ks * p.n_units, ks, p.n_units);
  }
};
struct GuestChainDown {
  typedef ChainDownP P;
  static constexpr int THREADS = 7 * 64;
  static __device__ __forceinline__ void run(const P& p, int gwg) { chain_down_body<7, 10, 2, 3, 1, false>(p, gwg); }
};
// the down projection as the guest of the NEXT layer's q/k/v GEMM (7 waves against the host's 4: the fused kernel's block is the guest's): four units per workgroup
struct GuestChainDown4 {
  typedef ChainDownP P;
  static constexpr int THREADS = 7 * 64, UNITS = 4;
  static __device__ __forceinline__ void run(const P& p, int gwg) {
    if ((gwg + 1) * (UNITS * 3) > p.N) return;          // (a grid rounded up past the guest's workgroups)
    chain_down_loop_body<7, 10, 2, 3, 1, UNITS>(p, gwg);
  }
};
struct GuestChainDownW8 {
  typedef ChainDownP P;
  static constexpr int THREADS = 7 * 64;
  static __device__ __forceinline__ void run(const P& p, int gwg) { chain_down_body<7, 10, 2, 3, 1, false, true>(p, gwg); }
};
struct GuestChainDown4W8 {
  typedef ChainDownP P;
  static constexpr int THREADS = 7 * 64, UNITS = 4;
  static __device__ __forceinline__ void run(const P& p, int gwg) {
    if ((gwg + 1) * (UNITS * 3) > p.N) return;          // (a grid rounded up past the guest's workgroups)
    chain_down_loop_body<7, 10, 2, 3, 1, UNITS, true>(p, gwg);
  }
};
// one-wave bodies: ONE wave per guest workgroup, the stand-alone launch's geometry (the host's other waves return at once).  Several to a workgroup were measured and
// lost: eight chain_attn waves pull 256 KB of K / V^T through one CU and outlast the o_proj GEMM (profiles/cohost_ab.md)
struct GuestChainAttn {
  typedef ChainAttnP P;
  static constexpr int THREADS = 64;
  static __device__ __forceinline__ void run(const P& p, int gwg) {      // batch 1: guest workgroup -> (kv head, split x row tile), the stand-alone grid's x and y
    const int gy = p.n_splits << p.tile_sh;
    if (gwg >= p.n_kv * gy) return;
    const int by = ch_fdiv(gwg, __builtin_amdgcn_rcpf((float)p.n_kv));
    chain_attn_body<2, 1, false, false>(p, gwg - by * p.n_kv, by, 0, p.n_kv, gy);
  }
};
struct GuestChainQkv {
  struct P { ChainQkvP q; int units; };
  static constexpr int THREADS = 64;
  static __device__ __forceinline__ void run(const P& p, int gwg) {
    if (gwg >= p.units) return;
    chain_qkv_body<24, 2, 1, false>(p.q, gwg);
  }
};

// host side (csrc/chain.hip); internal to the library: hidden, not part of the C ABI
#define VL_INTERNAL __attribute__((visibility("hidden")))
// (the gate/up and down preparations accept either kind of their launch and return 0 = not hostable here, 1 = the bf16 kind, 2 = its e4m3 counterpart VL_GUEST_CHAIN_GU_W8 /
// _DOWN_W8: the host picks the Guest... or Guest...W8 instantiation from the answer; the others return 0 / 1)
VL_INTERNAL int vl_cohost_chain_gu(const VlaserCohostGuest* g, ChainGuP* p, int* wgs, int* lds);
VL_INTERNAL int vl_cohost_chain_qkv(const VlaserCohostGuest* g, ChainQkvP* p, int* units, int* lds_unit);
VL_INTERNAL int vl_cohost_chain_attn(const VlaserCohostGuest* g, ChainAttnP* p, int* waves);
VL_INTERNAL int vl_cohost_chain_oproj(const VlaserCohostGuest* g, ChainOprojP* p, int* wgs, int* lds);
VL_INTERNAL int vl_cohost_chain_down(const VlaserCohostGuest* g, ChainDownP* p, int* wgs);
VL_INTERNAL int vl_cohost_chain_down4(const VlaserCohostGuest* g, ChainDownP* p, int* wgs);      // the looped form: *wgs = workgroups of four units
VL_INTERNAL int vl_cohost_guest_launch(const VlaserCohostGuest* g, vl_stream_t s);      // the guest on its own, behind its host: what every pair without a fused instantiation does
VL_INTERNAL void vl_cohost_count_fused();          // one more launch that carried its guest (vlaser_cohost_fused_count)
VL_INTERNAL bool vl_cohost_lab_zero_guests();      // vlaser_cohost_lab(1): fused kernels launched with no guest workgroups
