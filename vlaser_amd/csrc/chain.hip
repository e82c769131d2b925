// The <= 16-row layer-step chain (action-expert Euler steps, greedy decode), round 5: three kernels rebuilt around what the in-chain, in-kernel
// timeline showed (tools/micro/chain_timeline.py, profiles/r05a_chain_timeline.md): a dependent kernel boundary costs 1.4-1.6 us on this chip and a
// dependent load -> store kernel 1.75 us (tools/micro/launch_floor.hip) -- the r01-r04 "4.9 us floor" of a short kernel was its own serial structure:
//   * runtime-optional code paths (slab-count loops, second chunks, `if (ucount > u)` weight requests) make hipcc's waitcnt pass merge the worst case of
//     every path: `s_waitcnt vmcnt(0)` in front of units 1 and 2 of the gate/up stream (three dependent HBM round trips instead of one), in front of
//     the K / V^T requests of the attention, before the norm of every prologue;
//   * every workgroup of a consumer re-reduced the producer's fp32 split-K slabs (66-98 KB through one CU's L1 = 0.7 us before the first FLOP).
// Here every shape parameter is a template argument, every load of a kernel is issued in ONE straight-line block (small dependent data first, the
// weight stream behind it: vmcnt retires in issue order), and the down projection publishes the residual stream ONCE, as bf16:
//
//   chain_qkv  : one WAVE per 16-row unit (no LDS exchange between waves, no barrier): RMSNorm of the published bf16 residual stream, q/k/v GEMV over the
//                whole K, bias + RoPE + cache scatter (lane-local epilogue of skinny.hip's 16-row units; same packed weights)
//   chain_gu   : residual + o_proj's split-K slabs + RMSNorm -> gate/up GEMV -> SwiGLU with ALL units of the workgroup requested up front; same
//                arithmetic and summation order as skinny_kernel<NORM, SWIGLU> (bit-identical outputs)
//   chain_down : down projection WITHOUT cross-workgroup split-K: a workgroup owns 4 output columns over the whole K (v_mfma_f32_4x4x4_16b_bf16: 16
//                independent 4 x 4 x 4 blocks per instruction = 4 columns x 4 rows x 64 k), adds the residual and stores the next layer's bf16
//                residual stream -- the consumer loads 6 KB instead of 66 KB and runs no slab reduction

#include <cstddef>
#include "chain_kernels.h"


template <int NS, int UE, int SP, int CPT, int TPU, bool W8 = false>
static int chain_gu_launch(const ChainGuP& p, int gx, int lds, hipStream_t stream) {
  if (p.dbg) {
    if (int rc = set_max_lds_once(chain_gu_kernel<NS, UE, SP, CPT, TPU, true, W8>, lds)) return rc;
    hipLaunchKernelGGL((chain_gu_kernel<NS, UE, SP, CPT, TPU, true, W8>), dim3(gx), dim3(512), lds, stream, p);
  } else {
    if (int rc = set_max_lds_once(chain_gu_kernel<NS, UE, SP, CPT, TPU, false, W8>, lds)) return rc;
    hipLaunchKernelGGL((chain_gu_kernel<NS, UE, SP, CPT, TPU, false, W8>), dim3(gx), dim3(512), lds, stream, p);
  }
  VL_LAUNCH_CHECK();
  return 0;
}

/* tpu = tiles per unit of the packed weights (2: pack_gate_up, 1: pack_gate_up8).
   ONE list of the built variants {K / 256, units per workgroup, producer slabs, tiles per unit} per weight format: the predicates and the dispatch below are generated from
   them (the predicate admitted K = 768 / 2 slabs / 2 units per workgroup, which has no instantiation).  The e4m3 list holds what the action expert reaches,
   the second e4m3 list (the vlaser_chain_gu_w8_k1536 pair) what the Vlaser-2B greedy decode reaches.  fmt: 0 = bf16, 1 = e4m3, 2 = e4m3 at K = 1536. */
#define CG_VARIANTS(X) X(3, 3, 3, 2) X(3, 3, 2, 2) X(6, 3, 2, 2) X(3, 2, 3, 2) X(6, 2, 2, 2) X(3, 5, 3, 1) X(6, 5, 2, 1)
#define CG_W8_VARIANTS(X) X(3, 5, 3, 1)
#define CG_W8_K1536_VARIANTS(X) X(6, 5, 2, 1)
enum { CG_BF16 = 0, CG_W8 = 1, CG_W8_K1536 = 2 };
static int chain_gu_has(int M, int N, int K, int n_partials, int tpu, int fmt) {
  if (M < 1 || M > 16 || K % 256 || (tpu != 1 && tpu != 2) || N < 16 * tpu || N % (16 * tpu)) return 0;
  const int cpt = (M * (K / 8) + 511) / 512;
  if (cpt > 3) return 0;
  const int ns = K / 256, units = N / (16 * tpu), longest = (units + 255) / 256;
#define CG_HAS(NS_, UE_, SP_, TPU_) if (ns == NS_ && longest == UE_ && n_partials == SP_ && tpu == TPU_) return 1;
  if (fmt == CG_W8_K1536) { CG_W8_K1536_VARIANTS(CG_HAS) } else if (fmt == CG_W8) { CG_W8_VARIANTS(CG_HAS) } else { CG_VARIANTS(CG_HAS) }
#undef CG_HAS
  return 0;
}
extern "C" int vlaser_chain_gu_supported(int M, int N, int K, int n_partials, int tpu) { return chain_gu_has(M, N, K, n_partials, tpu, CG_BF16); }
extern "C" int vlaser_chain_gu_w8_supported(int M, int N, int K, int n_partials, int tpu) { return chain_gu_has(M, N, K, n_partials, tpu, CG_W8); }
extern "C" int vlaser_chain_gu_w8_k1536_supported(int M, int N, int K, int n_partials, int tpu) { return chain_gu_has(M, N, K, n_partials, tpu, CG_W8_K1536); }

struct ChainGuGeom { int gx, lds, ns, longest, cpt, tpu; };
/* validation + kernel parameters + launch geometry of a vlaser_chain_gu call: what the stand-alone launch and a co-hosted one share */
static int chain_gu_prepare(const VlaserSkinnyArgs* a, int fmt, ChainGuP& p, ChainGuGeom& q) {
  const bool w8 = fmt != CG_BF16;
  VL_CHECK(a && a->x && a->W && a->norm_w && a->out && a->partials, "vlaser_chain_gu: null operand");
  VL_CHECK(!w8 || a->w_scale, "vlaser_chain_gu_w8: null w_scale (fp32 row scales of the e4m3 weights, packed row order)");
  const int tpu = a->tiles_per_unit == 1 ? 1 : 2;
  VL_CHECK(a->tiles_per_unit == 2 || a->tiles_per_unit == 0 || a->tiles_per_unit == 1, "vlaser_chain_gu: weights packed in 32-row (pack_gate_up) or 16-row (pack_gate_up8) units");
  if (fmt == CG_W8_K1536)
    VL_CHECK(a->k_splits == 1 && chain_gu_has(a->M, a->N, a->K, a->n_partials, tpu, CG_W8_K1536),
             "vlaser_chain_gu_w8_k1536: built for K = 1536, 2 producer slabs, 5 16-row units per workgroup, M <= 8 (got M %d N %d K %d slabs %d tiles per unit %d)", a->M, a->N, a->K,
             a->n_partials, tpu);
  else if (fmt == CG_W8)
    VL_CHECK(a->k_splits == 1 && chain_gu_has(a->M, a->N, a->K, a->n_partials, tpu, CG_W8),
             "vlaser_chain_gu_w8: built for K = 768, 3 producer slabs, 5 16-row units per workgroup, M * K / 8 <= 1536 chunks (got M %d N %d K %d slabs %d tiles per unit %d)", a->M, a->N, a->K,
             a->n_partials, tpu);
  else
    VL_CHECK(a->k_splits == 1 && chain_gu_has(a->M, a->N, a->K, a->n_partials, tpu, CG_BF16),
             "vlaser_chain_gu: built for K = 768 / 1536, 2 or 3 producer slabs, 2-3 (32-row) or 5 (16-row) units per workgroup, M * K / 8 <= 1536 chunks (got M %d N %d K %d slabs %d)", a->M, a->N,
             a->K, a->n_partials);
  VL_CHECK(((uintptr_t)a->W & 15) == 0 && ((uintptr_t)a->x & 15) == 0 && ((uintptr_t)a->partials & 15) == 0 && ((uintptr_t)a->out & 7) == 0 && a->ldo % 4 == 0 &&
               (!w8 || ((uintptr_t)a->w_scale & 15) == 0),
           "vlaser_chain_gu: alignment");
  const int n_valid = a->n_valid > 0 ? a->n_valid : a->N;
  VL_CHECK(n_valid % (16 * tpu) == 0, "vlaser_chain_gu: whole [gate|up] groups");
  p.h_in = (const bf16_t*)a->x; p.partials = a->partials; p.norm_w = (const bf16_t*)a->norm_w; p.h_out = (bf16_t*)a->h_out;
  p.W = (const u32x4*)a->W; p.out = (bf16_t*)a->out; p.w_scale = w8 ? a->w_scale : nullptr;
  p.M = a->M; p.ldo = a->ldo; p.n_valid = n_valid; p.eps = a->eps; p.inv_cpr = 8.0f / (float)a->K; p.dbg = a->dbg;
  const int units = a->N / (16 * tpu), longest = (units + 255) / 256, gx = (units + longest - 1) / longest;
  p.ulo = units / gx; p.urem = units % gx;
  q.gx = gx; q.ns = a->K / 256; q.longest = longest; q.cpt = (a->M * (a->K / 8) + 511) / 512; q.tpu = tpu;
  q.lds = ((a->M * (a->K * 2 + 16) + 15) & ~15) + longest * 8 * tpu * 64 * 16;
  return 0;
}

static int chain_gu_entry(const VlaserSkinnyArgs* a, vl_stream_t s, int fmt) {
  ChainGuP p;
  ChainGuGeom q;
  if (int rc = chain_gu_prepare(a, fmt, p, q)) return rc;
  const int ns = q.ns, longest = q.longest, cpt = q.cpt, tpu = q.tpu, gx = q.gx, lds = q.lds;
  hipStream_t stream = (hipStream_t)s;
#define CG_CASE(NS_, UE_, SP_, CPT_, TPU_, W8_) if (ns == NS_ && longest == UE_ && a->n_partials == SP_ && cpt == CPT_ && tpu == TPU_) return chain_gu_launch<NS_, UE_, SP_, CPT_, TPU_, W8_>(p, gx, lds, stream);
#define CG_CPT(NS_, UE_, SP_, TPU_) CG_CASE(NS_, UE_, SP_, 1, TPU_, false) CG_CASE(NS_, UE_, SP_, 2, TPU_, false) CG_CASE(NS_, UE_, SP_, 3, TPU_, false)
#define CG_W8_CPT(NS_, UE_, SP_, TPU_) CG_CASE(NS_, UE_, SP_, 1, TPU_, true) CG_CASE(NS_, UE_, SP_, 2, TPU_, true) CG_CASE(NS_, UE_, SP_, 3, TPU_, true)
  if (fmt == CG_W8_K1536) { CG_W8_K1536_VARIANTS(CG_W8_CPT) } else if (fmt == CG_W8) { CG_W8_VARIANTS(CG_W8_CPT) } else { CG_VARIANTS(CG_CPT) }
#undef CG_W8_CPT
#undef CG_CPT
#undef CG_CASE
  vlaser_set_error("vlaser_chain_gu: no variant for K %d, %d units per workgroup, %d slabs, %d chunks per thread, %d tiles per unit", a->K, longest, a->n_partials, cpt, tpu);
  return -1;
}
extern "C" int vlaser_chain_gu(const VlaserSkinnyArgs* a, vl_stream_t s) { return chain_gu_entry(a, s, CG_BF16); }
extern "C" int vlaser_chain_gu_w8(const VlaserSkinnyArgs* a, vl_stream_t s) { return chain_gu_entry(a, s, CG_W8); }
extern "C" int vlaser_chain_gu_w8_k1536(const VlaserSkinnyArgs* a, vl_stream_t s) { return chain_gu_entry(a, s, CG_W8_K1536); }


extern "C" int vlaser_chain_qkv_supported(int M, int N, int K) { return M >= 1 && ((K == 768 && M <= 16) || (K == 1536 && M <= 8)) && N % 128 == 0; }      // (hidden 1536 x 16 rows would spill)

static int chain_qkv_prepare(const VlaserSkinnyArgs* a, ChainQkvP& p) {
  VL_CHECK(a && a->x && a->W && a->norm_w && a->bias && a->q_out && a->k_cache && a->vt_cache && a->rope_cos && a->rope_sin && a->pos_ids, "vlaser_chain_qkv: null operand");
  VL_CHECK(a->tiles_per_unit == 1 && a->k_splits == 1, "vlaser_chain_qkv: weights packed in 16-row lane-local units (pack_qkv16 + pack_skinny(..., 1, 1))");
  VL_CHECK(a->n_partials == 0, "vlaser_chain_qkv: reads the residual stream as published by vlaser_chain_down (no slabs; got %d)", a->n_partials);
  VL_CHECK(vlaser_chain_qkv_supported(a->M, a->N, a->K), "vlaser_chain_qkv: built for hidden 768 / 1536, M <= 16 (8 at 1536), whole heads (got M %d N %d K %d)", a->M, a->N, a->K);
  VL_CHECK(((uintptr_t)a->W & 15) == 0 && ((uintptr_t)a->x & 15) == 0 && ((uintptr_t)a->norm_w & 15) == 0 && ((uintptr_t)a->bias & 7) == 0, "vlaser_chain_qkv: alignment");
  p.h_in = (const bf16_t*)a->x; p.partials = a->partials; p.h_out = (bf16_t*)a->h_out; p.norm_w = (const bf16_t*)a->norm_w; p.W = (const u32x4*)a->W; p.bias = (const bf16_t*)a->bias;
  p.q_out = (bf16_t*)a->q_out; p.k_cache = (bf16_t*)a->k_cache; p.vt_cache = (bf16_t*)a->vt_cache; p.rope_cos = a->rope_cos; p.rope_sin = a->rope_sin;
  p.pos_ids = a->pos_ids; p.M = a->M; p.n_q_heads = a->n_q_heads; p.n_kv_heads = a->n_kv_heads; p.s_max = a->s_max; p.tok_per_batch = a->tok_per_batch;
  p.slot_base = a->slot_base; p.eps = a->eps; p.dbg = a->dbg;
  return 0;
}

extern "C" int vlaser_chain_qkv(const VlaserSkinnyArgs* a, vl_stream_t s) {
  ChainQkvP p;
  if (int rc = chain_qkv_prepare(a, p)) return rc;
  const int units = a->N / 16, rg = (a->M + 3) / 4, ks = a->K / 32;
  // waves per unit (K parts): hidden 1536 two (measured in the decode step: 0.9745 -> 0.9595 ms per token), hidden 768 one
  const int nwv = ks == 48 ? 2 : 1;
  const int lds = nwv * 4 * rg * (a->K / nwv * 2 + 16) + (nwv - 1) * 64 * 16;
  hipStream_t stream = (hipStream_t)s;
#define CQ_LAUNCH(KS_, RG_, NWV_, DBG_)                                                                                 \
  do {                                                                                                                  \
    if (int rc = set_max_lds_once(chain_qkv_kernel<KS_, RG_, NWV_, DBG_>, lds)) return rc;                               \
    hipLaunchKernelGGL((chain_qkv_kernel<KS_, RG_, NWV_, DBG_>), dim3(units), dim3(64 * NWV_), lds, stream, p);          \
    VL_LAUNCH_CHECK();                                                                                                  \
    return 0;                                                                                                           \
  } while (0)
#define CQ_CASE(KS_, RG_, NWV_) if (ks == KS_ && rg == RG_ && nwv == NWV_) { if (p.dbg) CQ_LAUNCH(KS_, RG_, NWV_, true); else CQ_LAUNCH(KS_, RG_, NWV_, false); }
  CQ_CASE(24, 1, 1) CQ_CASE(24, 2, 1) CQ_CASE(24, 3, 1) CQ_CASE(24, 4, 1)
  CQ_CASE(48, 1, 2) CQ_CASE(48, 2, 2)      // (measured and not kept: four waves at hidden 1536 0.9709 vs 0.9697 ms per token; two waves at hidden 768 11.656 vs 11.645 ms per chunk)
#undef CQ_CASE
#undef CQ_LAUNCH
  vlaser_set_error("vlaser_chain_qkv: no variant");
  return -1;
}


extern "C" int vlaser_chain_down_geometry(int N, int* cols, int* groups);
extern "C" int vlaser_chain_down_supported(int M, int N, int K) {
  if (!(M >= 1 && M <= 16 && (N % 3 == 0 || N % 4 == 0) && K == 8960)) return 0;
  int c, g;
  vlaser_chain_down_geometry(N, &c, &g);
  return g == 1 || M <= 8;            // two column groups per workgroup x 16 rows would spill
}
extern "C" int vlaser_chain_down_w8_supported(int M, int N, int K) { return vlaser_chain_down_supported(M, N, K); }      // every case of the one dispatch below, in both formats
/* column geometry of vlaser_chain_down / ops.pack_down4 for an output width N: cols per group (3 or 4) and groups per workgroup, chosen for ~256 workgroups */
extern "C" int vlaser_chain_down_geometry(int N, int* cols, int* groups) {
  const int c = (N % 3 == 0) ? 3 : 4;
  const int g = (N / c >= 512 && (N / c) % 2 == 0) ? 2 : 1;
  if (cols) *cols = c;
  if (groups) *groups = g;
  return N / (c * g);
}

template <bool W8>
static int chain_down_dispatch(const ChainDownP& p, int wgs, int cols, int groups, hipStream_t stream) {
  const int rg = (p.M + 3) / 4;
#define CD_LAUNCH(RG_, COLS_, CG_)                                                                                                         \
  do {                                                                                                                                     \
    if (p.dbg) hipLaunchKernelGGL((chain_down_kernel<7, 10, RG_, COLS_, CG_, true, W8>), dim3(wgs), dim3(7 * 64), 0, stream, p);             \
    else hipLaunchKernelGGL((chain_down_kernel<7, 10, RG_, COLS_, CG_, false, W8>), dim3(wgs), dim3(7 * 64), 0, stream, p);                  \
    VL_LAUNCH_CHECK();                                                                                                                     \
    return 0;                                                                                                                              \
  } while (0)
#define CD_CASE1(RG_) if (rg == RG_ && groups == 1) { if (cols == 3) CD_LAUNCH(RG_, 3, 1); else CD_LAUNCH(RG_, 4, 1); }
#define CD_CASE2(RG_) if (rg == RG_ && groups == 2) { if (cols == 3) CD_LAUNCH(RG_, 3, 2); else CD_LAUNCH(RG_, 4, 2); }
  CD_CASE1(1) CD_CASE1(2) CD_CASE1(3) CD_CASE1(4) CD_CASE2(1) CD_CASE2(2)
#undef CD_CASE1
#undef CD_CASE2
#undef CD_LAUNCH
  vlaser_set_error("vlaser_chain_down: no variant");
  return -1;
}

/* x bf16 [M, ldx] (ldx >= K), W = ops.pack_down4(down_proj.weight), res / h_out bf16 [M, N] (may not alias): h_out = bf16(res + x @ W^T).
   w8: W = ops.pack_down4_e4m3(codes), w_scale = ops.pack_down4_scales(scale): h_out = bf16(res + scale * (x @ codes^T)) */
static int chain_down_prepare(const void* x, int ldx, const void* W, const float* w_scale, const void* res, void* h_out, int M, int N, int K, unsigned long long* dbg, bool w8, ChainDownP& p) {
  VL_CHECK(x && W && res && h_out && res != h_out, "vlaser_chain_down: null operand (or res == h_out: every workgroup reads its residual columns while others store)");
  VL_CHECK(!w8 || w_scale, "vlaser_chain_down_w8: null w_scale (fp32 column scales of the e4m3 weights, ops.pack_down4_scales)");
  VL_CHECK(vlaser_chain_down_supported(M, N, K) && ldx >= K && ldx % 8 == 0, "vlaser_chain_down: built for K = 8960 (7 waves x 10 loads x 128), N %% 3 == 0 or N %% 4 == 0, M <= 16 (got M %d N %d K %d)", M, N, K);
  VL_CHECK(((uintptr_t)W & 15) == 0 && ((uintptr_t)x & 15) == 0 && (!w8 || ((uintptr_t)w_scale & 15) == 0), "vlaser_chain_down: alignment");
  p.x = (const bf16_t*)x; p.W = (const u32x4*)W; p.res = (const bf16_t*)res; p.h_out = (bf16_t*)h_out; p.out_f32 = nullptr; p.M = M; p.N = N; p.ldx = ldx; p.dbg = dbg;
  p.w_scale = w8 ? (const f32x4*)w_scale : nullptr;
  return 0;
}
static int chain_down_entry(const void* x, int ldx, const void* W, const float* w_scale, const void* res, void* h_out, int M, int N, int K, unsigned long long* dbg, vl_stream_t s, bool w8) {
  ChainDownP p;
  if (int rc = chain_down_prepare(x, ldx, W, w_scale, res, h_out, M, N, K, dbg, w8, p)) return rc;
  int cols, groups;
  const int wgs = vlaser_chain_down_geometry(N, &cols, &groups);
  return w8 ? chain_down_dispatch<true>(p, wgs, cols, groups, (hipStream_t)s) : chain_down_dispatch<false>(p, wgs, cols, groups, (hipStream_t)s);
}
extern "C" int vlaser_chain_down(const void* x, int ldx, const void* W, const void* res, void* h_out, int M, int N, int K, unsigned long long* dbg, vl_stream_t s) {
  return chain_down_entry(x, ldx, W, nullptr, res, h_out, M, N, K, dbg, s, false);
}
extern "C" int vlaser_chain_down_w8(const void* x, int ldx, const void* W, const float* w_scale, const void* res, void* h_out, int M, int N, int K, unsigned long long* dbg, vl_stream_t s) {
  return chain_down_entry(x, ldx, W, w_scale, res, h_out, M, N, K, dbg, s, true);
}


/* vlaser_attn_skinny's arguments (part_m = fp32 [B, n_kv, n_splits, 32, 2] (m, l) pairs, part_o = BF16 [B, n_kv, n_splits, 32, 128] normalised rows, part_l unused);
 * n_splits must equal ceil(ceil(kv_len / 32) / 2). */
extern "C" int vlaser_chain_attn_splits(int kv_len) { return (((kv_len + 31) >> 5) + 1) / 2; }
static int chain_attn_prepare(const VlaserAttnArgs* a, ChainAttnP& p) {
  VL_CHECK(a && a->q && a->k && a->vt && a->part_m && a->part_o, "vlaser_chain_attn: null pointer");
  VL_CHECK(a->head_dim == 128 && a->n_q_heads % a->n_kv_heads == 0 && a->sq >= 1 && a->sq * (a->n_q_heads / a->n_kv_heads) <= 32, "vlaser_chain_attn: head_dim 128, group * tokens <= 32");
  VL_CHECK(a->ld_vt % 32 == 0 && a->kv_len >= 1 && a->kv_len <= a->ld_vt && (a->mode == VL_ATTN_FULL || a->mode == VL_ATTN_PREFIX || a->mode == VL_ATTN_DENSE), "vlaser_chain_attn: bad cache geometry / mode");
  VL_CHECK(a->mode != VL_ATTN_DENSE || (a->mask && a->mask_rs % 4 == 0 && a->mask_rs >= ((a->kv_len + 31) & ~31) && (((uintptr_t)a->mask) & 15) == 0 && a->mask_bs % 4 == 0 && a->first_tok_kv_len == 0),
           "vlaser_chain_attn: VL_ATTN_DENSE needs a 16-byte aligned fp32 mask whose row stride is a multiple of 4 >= kv_len rounded up to 32 (and no riding first token)");
  VL_CHECK(a->n_splits == vlaser_chain_attn_splits(a->kv_len) && a->n_splits <= 16, "vlaser_chain_attn: n_splits must be ceil(chunks / 2) <= 16 (kv_len <= 1024)");
  p.q = (const bf16_t*)a->q; p.k = (const bf16_t*)a->k; p.vt = (const bf16_t*)a->vt; p.pml = a->part_m; p.po = (bf16_t*)a->part_o; p.valid_len = a->valid_len;
  p.q_bs = a->q_bs; p.q_hs = a->q_hs; p.q_ss = a->q_ss; p.k_bs = a->k_bs; p.k_hs = a->k_hs; p.vt_bs = a->vt_bs; p.vt_hs = a->vt_hs;
  p.sq = a->sq; p.kv_len = a->kv_len; p.G = a->n_q_heads / a->n_kv_heads; p.ld_vt = a->ld_vt; p.mode = a->mode; p.blk_start = a->blk_start;
  p.first_tok_kv_len = a->first_tok_kv_len; p.n_splits = a->n_splits; p.n_kv = a->n_kv_heads; p.scale = a->scale; p.dbg = a->dbg;
  p.mask = a->mask; p.mask_bs = a->mask_bs; p.mask_rs = a->mask_rs;
  p.tile_sh = a->sq * p.G > 16 ? 1 : 0;
  return 0;
}
extern "C" int vlaser_chain_attn(const VlaserAttnArgs* a, vl_stream_t s) {
  ChainAttnP p;
  if (int rc = chain_attn_prepare(a, p)) return rc;
  const dim3 grid(a->n_kv_heads, a->n_splits << p.tile_sh, a->batch);
  if (a->mode == VL_ATTN_DENSE) hipLaunchKernelGGL((chain_attn_kernel<2, 1, false, true>), grid, dim3(64), 0, (hipStream_t)s, p);
  else if (p.dbg) hipLaunchKernelGGL((chain_attn_kernel<2, 1, true>), grid, dim3(64), 0, (hipStream_t)s, p);
  else hipLaunchKernelGGL((chain_attn_kernel<2, 1, false>), grid, dim3(64), 0, (hipStream_t)s, p);
  VL_LAUNCH_CHECK();
  return 0;
}


extern "C" int vlaser_chain_oproj_supported(int M, int N, int K, int k_splits, int attn_splits, int group) {
  if (M < 1 || M > 16 || N % 16 || K % (k_splits * 256) || K % (128 * group) || (K / k_splits) % (128) ) return 0;
  const int ns = K / (k_splits * 256);
  if (!((ns == 2 || ns == 3) && attn_splits >= 1 && attn_splits <= 16)) return 0;
  return 1;            // (M (K / k_splits / 8) > 512 pieces of the activation tile: further passes of the merge prologue)
}

/* args as vlaser_skinny(VL_PRO_ATTN, VL_SK_PARTIAL) with tiles_per_unit = 1, attn_m = the (m, l) pairs and attn_o = the bf16 rows written by vlaser_chain_attn */
static int chain_oproj_prepare(const VlaserSkinnyArgs* a, ChainOprojP& p, int& ns, int& lds) {
  VL_CHECK(a && a->W && a->attn_m && a->attn_o && a->out_f32, "vlaser_chain_oproj: null operand");
  VL_CHECK(a->tiles_per_unit == 1 && vlaser_chain_oproj_supported(a->M, a->N, a->K, a->k_splits, a->attn_splits, a->attn_group),
           "vlaser_chain_oproj: built for 16-row units, 2 / 3 K-steps per wave, <= 16 attention splits (got M %d N %d K %d ks %d splits %d)", a->M, a->N, a->K,
           a->k_splits, a->attn_splits);
  p.pml = a->attn_m; p.po = (const bf16_t*)a->attn_o; p.W = (const u32x4*)a->W; p.out = a->out_f32;
  p.M = a->M; p.N = a->n_valid > 0 ? a->n_valid : a->N; p.n_units = a->N / 16; p.G = a->attn_group; p.nq = a->attn_nq; p.nkv = a->K / (128 * a->attn_group); p.n_splits = a->attn_splits;
  const int kb = a->K / a->k_splits;
  ns = kb / 256;
  p.inv_cpr = 8.0f / (float)kb; p.dbg = a->dbg;
  VL_CHECK(p.N % 16 == 0, "vlaser_chain_oproj: N must be a whole number of 16-column units");
  lds = ((a->M * (kb * 2 + 16) + 15) & ~15) + 7 * 64 * 16;
  return 0;
}
extern "C" int vlaser_chain_oproj(const VlaserSkinnyArgs* a, vl_stream_t s) {
  ChainOprojP p;
  int ns, lds;
  if (int rc = chain_oproj_prepare(a, p, ns, lds)) return rc;
  const dim3 grid(a->N / 16, a->k_splits);
  hipStream_t stream = (hipStream_t)s;
#define CO_LAUNCH(NS_, S_, DBG_)                                                                          \
  do {                                                                                                    \
    if (int rc = set_max_lds_once(chain_oproj_kernel<NS_, S_, DBG_>, lds)) return rc;                      \
    hipLaunchKernelGGL((chain_oproj_kernel<NS_, S_, DBG_>), grid, dim3(512), lds, stream, p);              \
    VL_LAUNCH_CHECK();                                                                                    \
    return 0;                                                                                             \
  } while (0)
#define CO_CASE(NS_, S_) if (ns == NS_ && sreq == S_) { if (p.dbg) CO_LAUNCH(NS_, S_, true); else CO_LAUNCH(NS_, S_, false); }
  const int sreq = p.n_splits == 7 ? 7 : (p.n_splits <= 10 ? 10 : 16);
  CO_CASE(2, 7) CO_CASE(3, 7) CO_CASE(2, 10) CO_CASE(3, 10) CO_CASE(2, 16) CO_CASE(3, 16)
#undef CO_CASE
#undef CO_LAUNCH
  vlaser_set_error("vlaser_chain_oproj: no variant");
  return -1;
}


// ------------------------------------------------------------------------------------------------------------------ co-hosted launches: the guest side on the host
// (include/vlaser_hip.h, VlaserCohostGuest).  vl_cohost_chain_*: non-zero (gate/up and down, which take either weight format: 1 = bf16, 2 = e4m3) when the guest is that launch AT THE SHAPE ITS FUSED INSTANTIATION IS BUILT FOR (Euler step 0 of a
// batch-1 chunk: 5 rows, no timeline stamps; bf16 weights, or for the *_W8 kinds the e4m3 codes and scales of the stand-alone W8 entries) and its arguments pass the stand-alone entry's checks -- then the parameters and the geometry are filled in;
// 0 otherwise: the caller launches host, then guest (vl_cohost_guest_launch, which reports a bad argument exactly as the stand-alone entry would).
VL_INTERNAL int vl_cohost_chain_gu(const VlaserCohostGuest* g, ChainGuP* p, int* wgs, int* lds) {
  if (!g || (g->kind != VL_GUEST_CHAIN_GU && g->kind != VL_GUEST_CHAIN_GU_W8) || !g->args) return 0;
  const bool w8 = g->kind == VL_GUEST_CHAIN_GU_W8;
  const VlaserSkinnyArgs* a = (const VlaserSkinnyArgs*)g->args;
  ChainGuGeom q;
  if (a->dbg || chain_gu_prepare(a, w8 ? CG_W8 : CG_BF16, *p, q)) return 0;
  if (!(q.ns == 3 && q.longest == 5 && a->n_partials == 3 && q.cpt == 1 && q.tpu == 1)) return 0;
  *wgs = q.gx; *lds = q.lds;
  return w8 ? 2 : 1;
}
VL_INTERNAL int vl_cohost_chain_qkv(const VlaserCohostGuest* g, ChainQkvP* p, int* units, int* lds_unit) {
  if (!g || g->kind != VL_GUEST_CHAIN_QKV || !g->args) return 0;
  const VlaserSkinnyArgs* a = (const VlaserSkinnyArgs*)g->args;
  if (a->dbg || chain_qkv_prepare(a, *p)) return 0;
  if (!(a->K == 768 && (a->M + 3) / 4 == 2)) return 0;
  *units = a->N / 16; *lds_unit = 4 * 2 * (a->K * 2 + 16);
  return 1;
}
VL_INTERNAL int vl_cohost_chain_attn(const VlaserCohostGuest* g, ChainAttnP* p, int* waves) {
  if (!g || g->kind != VL_GUEST_CHAIN_ATTN || !g->args) return 0;
  const VlaserAttnArgs* a = (const VlaserAttnArgs*)g->args;
  if (a->dbg || a->mode == VL_ATTN_DENSE || a->batch != 1 || chain_attn_prepare(a, *p)) return 0;
  *waves = a->n_kv_heads * (a->n_splits << p->tile_sh);
  return 1;
}
VL_INTERNAL int vl_cohost_chain_oproj(const VlaserCohostGuest* g, ChainOprojP* p, int* wgs, int* lds) {
  if (!g || g->kind != VL_GUEST_CHAIN_OPROJ || !g->args) return 0;
  const VlaserSkinnyArgs* a = (const VlaserSkinnyArgs*)g->args;
  int ns;
  if (a->dbg || chain_oproj_prepare(a, *p, ns, *lds)) return 0;
  if (!(ns == 2 && p->n_splits == 7 && a->M * (a->K / a->k_splits / 8) <= 512)) return 0;
  *wgs = (a->N / 16) * a->k_splits;
  return 1;
}
// The two down kinds share one argument prefix (VlaserChainDownW8Args = VlaserChainDownArgs + w_scale): both are read through it, w_scale only where the kind has it.
#define CD_SHARED(F) static_assert(offsetof(VlaserChainDownW8Args, F) == offsetof(VlaserChainDownArgs, F) && sizeof(VlaserChainDownW8Args::F) == sizeof(VlaserChainDownArgs::F), #F)
CD_SHARED(x); CD_SHARED(ldx); CD_SHARED(W); CD_SHARED(res); CD_SHARED(h_out); CD_SHARED(M); CD_SHARED(N); CD_SHARED(K); CD_SHARED(dbg);
#undef CD_SHARED
static bool chain_down_guest(const VlaserCohostGuest* g, const VlaserChainDownArgs** a, bool* w8, const float** w_scale) {
  if (!g || (g->kind != VL_GUEST_CHAIN_DOWN && g->kind != VL_GUEST_CHAIN_DOWN_W8) || !g->args) return false;
  *a = (const VlaserChainDownArgs*)g->args;
  *w8 = g->kind == VL_GUEST_CHAIN_DOWN_W8;
  *w_scale = *w8 ? ((const VlaserChainDownW8Args*)g->args)->w_scale : nullptr;
  return true;
}
VL_INTERNAL int vl_cohost_chain_down(const VlaserCohostGuest* g, ChainDownP* p, int* wgs) {
  const VlaserChainDownArgs* a; bool w8; const float* w_scale;
  if (!chain_down_guest(g, &a, &w8, &w_scale)) return 0;
  if (a->dbg || chain_down_prepare(a->x, a->ldx, a->W, w_scale, a->res, a->h_out, a->M, a->N, a->K, nullptr, w8, *p)) return 0;
  int cols, groups;
  *wgs = vlaser_chain_down_geometry(a->N, &cols, &groups);
  if (!((a->M + 3) / 4 == 2 && cols == 3 && groups == 1)) return 0;
  return w8 ? 2 : 1;
}
// the looped form (chain_down_loop_kernel / GuestChainDown4): the same shape, and a workgroup count that four divides; *wgs = workgroups of four units
VL_INTERNAL int vl_cohost_chain_down4(const VlaserCohostGuest* g, ChainDownP* p, int* wgs) {
  static_assert(GuestChainDown4W8::UNITS == GuestChainDown4::UNITS, "one looped geometry for both weight formats");
  int units;
  const int fmt = vl_cohost_chain_down(g, p, &units);
  if (!fmt || units % GuestChainDown4::UNITS) return 0;
  *wgs = units / GuestChainDown4::UNITS;
  return fmt;
}
/* vlaser_chain_down / _w8 at the shape the looped form is built for (M in 5..8, cols 3, one group, workgroups a multiple of 4), run by the looped kernel of the weight format
   on its own: a quarter of the workgroups, four units each -- what the guest workgroups of the co-hosted q/k/v GEMM run.  Bit-identical to the stand-alone entry of the same
   format (W8: W = ops.pack_down4_e4m3, w_scale = ops.pack_down4_scales).  Tests and tools. */
template <bool W8>
static int chain_down_looped(const void* x, int ldx, const void* W, const float* w_scale, const void* res, void* h_out, int M, int N, int K, vl_stream_t s) {
  const VlaserChainDownW8Args a = {x, ldx, W, res, h_out, M, N, K, nullptr, w_scale};
  const VlaserCohostGuest g = {W8 ? VL_GUEST_CHAIN_DOWN_W8 : VL_GUEST_CHAIN_DOWN, &a};
  ChainDownP p;
  int wgs;
  if (!vl_cohost_chain_down4(&g, &p, &wgs)) {
    if (chain_down_prepare(x, ldx, W, w_scale, res, h_out, M, N, K, nullptr, W8, p)) return -1;      // (its message: W8, null or misaligned scales among them)
    vlaser_set_error("vlaser_chain_down_looped%s: built for 5..8 rows, 3-column units, a workgroup count that 4 divides (got M %d N %d)", W8 ? "_w8" : "", M, N);
    return -1;
  }
  hipLaunchKernelGGL((chain_down_loop_kernel<7, 10, 2, 3, 1, GuestChainDown4::UNITS, W8>), dim3(wgs), dim3(7 * 64), 0, (hipStream_t)s, p);
  VL_LAUNCH_CHECK();
  return 0;
}
extern "C" int vlaser_chain_down_looped(const void* x, int ldx, const void* W, const void* res, void* h_out, int M, int N, int K, vl_stream_t s) {
  return chain_down_looped<false>(x, ldx, W, nullptr, res, h_out, M, N, K, s);
}
extern "C" int vlaser_chain_down_looped_w8(const void* x, int ldx, const void* W, const float* w_scale, const void* res, void* h_out, int M, int N, int K, vl_stream_t s) {
  return chain_down_looped<true>(x, ldx, W, w_scale, res, h_out, M, N, K, s);
}
VL_INTERNAL int vl_cohost_guest_launch(const VlaserCohostGuest* g, vl_stream_t s) {
  if (!g || g->kind == VL_GUEST_NONE) return 0;
  VL_CHECK(g->args, "co-hosted launch: guest kind %d without arguments", g->kind);
  switch (g->kind) {
    case VL_GUEST_CHAIN_QKV: return vlaser_chain_qkv((const VlaserSkinnyArgs*)g->args, s);
    case VL_GUEST_CHAIN_ATTN: return vlaser_chain_attn((const VlaserAttnArgs*)g->args, s);
    case VL_GUEST_CHAIN_OPROJ: return vlaser_chain_oproj((const VlaserSkinnyArgs*)g->args, s);
    case VL_GUEST_CHAIN_GU: return vlaser_chain_gu((const VlaserSkinnyArgs*)g->args, s);
    case VL_GUEST_CHAIN_GU_W8: return vlaser_chain_gu_w8((const VlaserSkinnyArgs*)g->args, s);
    case VL_GUEST_CHAIN_DOWN:
    case VL_GUEST_CHAIN_DOWN_W8: {
      const VlaserChainDownArgs* a; bool w8; const float* w_scale;
      chain_down_guest(g, &a, &w8, &w_scale);
      return chain_down_entry(a->x, a->ldx, a->W, w_scale, a->res, a->h_out, a->M, a->N, a->K, a->dbg, s, w8);
    }
    default: break;
  }
  vlaser_set_error("co-hosted launch: unknown guest kind %d", g->kind);
  return -1;
}

// How many launches so far carried their guest as workgroups of their own grid (process-wide): lets a caller tell a co-hosted launch from the host-then-guest fallback,
// which computes the same and returns the same 0.
#include <atomic>
static std::atomic<long long> g_cohost_fused{0};
static std::atomic<int> g_cohost_lab{0};
VL_INTERNAL void vl_cohost_count_fused() { g_cohost_fused.fetch_add(1, std::memory_order_relaxed); }
VL_INTERNAL bool vl_cohost_lab_zero_guests() { return g_cohost_lab.load(std::memory_order_relaxed) == 1; }
extern "C" int vlaser_cohost_fused_count(void) { return (int)(g_cohost_fused.load(std::memory_order_relaxed) & 0x7fffffff); }
/* lab switch (tools/micro/cohost_host_alone.py): mode 1 = every fused kernel is launched with ZERO guest workgroups and the guest is NOT run -- the host's body inside the
   fused kernel, timed against the stand-alone host; 0 = normal.  Returns the previous mode.  Results are incomplete in mode 1: never set it outside a timing tool. */
extern "C" int vlaser_cohost_lab(int mode) { return g_cohost_lab.exchange(mode == 1 ? 1 : 0); }
