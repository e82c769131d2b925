"""Kernel sequencing for the three hot loops: InternViT tile encoder, Qwen2.5 prefill / greedy
decode, and the pi0 joint prefill + 10-step Euler sampler.  Every arithmetic step is a launch of a gfx950 kernel
from libvlaser_hip.so through vlaser_amd.ops; PyTorch only owns buffers and the stream.  All launches are
asynchronous and allocation-free after construction, so whole phases can be captured in one HIP graph.  A <= 16-row layer is a plan (_build_plan): one argument
struct and one (name, launch, args) entry per launch, its kernel path from layer_path and its MLP weight format from ops.chain_format.

Weights are stored in HBM in the layouts the kernels want (packed once at load):
  * q/k/v fused into one [N,K] matrix with in-head row permutation (RoPE pair in one MFMA lane),
  * gate/up interleaved in 16-row groups (SwiGLU is lane-local),
  * patch-embedding conv flattened to [1024, 640] (K zero-padded from 588 to a multiple of 64),
  * K cache [L][B,n_kv,S_max,128], V cache TRANSPOSED [L][B,n_kv,128,S_max] (MFMA A-fragment = one 16-byte load).
"""

import torch
from types import SimpleNamespace

from . import _lib as L
from . import ops
from .config import LLMConfig, VlaserConfig

BF = torch.bfloat16


def _dev(t, device):
    return t.to(device=device, dtype=BF).contiguous()


class QwenLayerWeights:
    """One Qwen2DecoderLayer in kernel layout: row-major packed matrices for the MFMA GEMM (prefill) and/or
    fragment-major copies for the weight-streaming skinny kernel (decode / action tokens)."""

    def __init__(self, sd, p, llm: LLMConfig, device, ks_o, ks_down, gemm=True, skinny=True, tpu_down=2, tpu_o=2, i_pad=None, opts=()):
        g = lambda k: _dev(sd[p + k], device)
        wqkv, self.bqkv = ops.pack_qkv(g('self_attn.q_proj.weight'), g('self_attn.k_proj.weight'),
                                       g('self_attn.v_proj.weight'), g('self_attn.q_proj.bias'),
                                       g('self_attn.k_proj.bias'), g('self_attn.v_proj.bias'), llm.head_dim)
        wo = g('self_attn.o_proj.weight')
        mlp8 = 'mlp8' in opts
        if mlp8:
            # 'mlp8': the MLP weights as e4m3 codes + power-of-two row scales (ops.quantize_rows_e4m3, on the host at load), in the packings of the W8 chain kernels; the
            # bf16 weight-streaming packings below are read only by the launches those replace and are not built.  A stack that also carries GEMM packings (the VLM's LLM:
            # prefill and forward()) builds them from the DEQUANTISED weights -- exact in bf16 -- so that prefill, forward() and the decode compute one and the same model.
            H, I = llm.hidden_size, llm.intermediate_size
            if not skinny or 'gu16' not in opts or not chain_packed(opts, H, I) or H not in (768, 1536):
                raise ValueError("'mlp8' serves the weight-streaming chain path only: needs 'chain', 'qkv16', 'gu16', hidden 768 / 1536 and MLP width 8960")
            q = lambda k: ops.quantize_rows_e4m3(sd[p + k])
            (gc, gs), (uc, us), (dc, ds) = q('mlp.gate_proj.weight'), q('mlp.up_proj.weight'), q('mlp.down_proj.weight')
            self.gu8 = ops.pack_gate_up8_e4m3(gc, gs, uc, us).to(device)
            self.down8, self.down8_scale = ops.pack_down4_e4m3(dc).to(device), ops.pack_down4_scales(ds).to(device)
            self.sk_gu = self.sk_down = None
            if gemm:
                dq = lambda c, sc: _dev(ops.dequantize_rows_e4m3(c, sc), device)
                wgu, wdown = ops.pack_gate_up(dq(gc, gs), dq(uc, us)), dq(dc, ds)
        else:
            wgu = ops.pack_gate_up(g('mlp.gate_proj.weight'), g('mlp.up_proj.weight'))
            wdown = g('mlp.down_proj.weight')
        self.ln_in = g('input_layernorm.weight')
        self.ln_post = g('post_attention_layernorm.weight')
        if gemm:
            self.wqkv, self.wo, self.wgu, self.wdown = wqkv, wo, wgu, wdown
        self.sk_down4 = None
        if skinny:
            self.bqkv_sk = self.bqkv
            if 'qkv16' in opts:           # 16-row lane-local units (r03): 2x the workgroups on the q/k/v GEMV
                w16, self.bqkv_sk = ops.pack_qkv16(g('self_attn.q_proj.weight'), g('self_attn.k_proj.weight'), g('self_attn.v_proj.weight'),
                                                   g('self_attn.q_proj.bias'), g('self_attn.k_proj.bias'), g('self_attn.v_proj.bias'), llm.head_dim)
                self.sk_qkv = ops.pack_skinny(w16, 1, 1)
            else:
                self.sk_qkv = ops.pack_skinny(wqkv, 1)
            self.sk_o = ops.pack_skinny(wo, ks_o, tpu_o)
            if not mlp8:
                # wide output + short K (action expert: 17920 x 768): 96-row units (tpu = 6) measured slower on MI355X (12.3 vs 11.2 us) and left
                # the kernel in r05; 16-row lane-local units ('gu16', r03) balance 1120 units over 256 workgroups (80 vs 96 rows on the longest)
                if 'gu16' in opts:
                    self.sk_gu = ops.pack_skinny(ops.pack_gate_up8(g('mlp.gate_proj.weight'), g('mlp.up_proj.weight')), 1, 1)
                else:
                    self.sk_gu = ops.pack_skinny(wgu, 1, 2)
                self.sk_down = ops.pack_skinny(wdown, ks_down, tpu_down, k_pad=i_pad)
                # 'chain' (r05, csrc/chain.hip): the down projection without cross-workgroup split-K (4 output columns per workgroup over the whole K) publishes the next
                # layer's residual stream as bf16
                if chain_packed(opts, wdown.shape[0], wdown.shape[1]):
                    self.sk_down4 = ops.pack_down4(wdown)


def chain_packed(opts, H, I):
    """Whether a stack carries the packings of the csrc/chain.hip kernels: asked for ('chain'), with the 16-row q/k/v units they read ('qkv16'), at the widths
    ops.pack_down4 / vlaser_chain_down serve."""
    return 'chain' in opts and 'qkv16' in opts and I == ops.DOWN4_WAVES * ops.DOWN4_LOADS * 128 and (H % 3 == 0 or H % 4 == 0)


def stack_geometry(llm: LLMConfig):
    """(tpu_o, ks_o, tpu_down, ks_down, I_pad): tiles per unit and split-K factors of the o / down projections of the weight-streaming kernels, and the padded MLP width."""
    H, I = llm.hidden_size, llm.intermediate_size
    nqd = llm.num_attention_heads * llm.head_dim
    # o_proj on 16-row units where the kernel has the variant: the same ~144 workgroups with half the split-K slabs for the
    # gate/up prologue to sum (chunk time unchanged, the dominant gate/up GEMV 8.9 -> 8.6 us; same-box A/B)
    ks16o = ops.pick_k_splits(nqd, H, rows_per_unit=16)
    tpu_o = 1 if (ks16o is not None and nqd // (ks16o * 256) in (2, 3)) else 2
    ks_o = ks16o if tpu_o == 1 else ops.skinny_geometry(nqd, H)[1]
    # down_proj (narrow output, long K): 16-row units double the workgroups that stream it (48 units x 5 splits = 240 for the expert)
    # when the kernel has that variant (5 or 7 K-steps per wave); measured +0.9 % chunks/s over 32-row units x 7 splits
    ks16 = ops.pick_k_splits(I, H, rows_per_unit=16)
    tpu_down = 1 if (ks16 is not None and I // (ks16 * 256) in (5, 7)) else 2
    I_pad, ks32 = ops.skinny_geometry(I, H)            # widths that do not factor (Vlaser-8B: 18944) are zero-padded: act buffer + down weight
    return tpu_o, ks_o, tpu_down, (ks16 if tpu_down == 1 else ks32), I_pad


def path_geometry(llm: LLMConfig, opts):
    """What layer_path reads of a stack, as integers and booleans: the widths, and the rows (ops.skinny_rows, as ops.pack_skinny pads them) and units of the
    q/k/v, gate/up and o matrices as QwenLayerWeights packs them under `opts` (QwenStack checks its packed layers against this)."""
    H, I, nq, nkv, hd = llm.hidden_size, llm.intermediate_size, llm.num_attention_heads, llm.num_key_value_heads, llm.head_dim
    tpu_o, ks_o = stack_geometry(llm)[:2]
    tpu_gu = 1 if 'gu16' in opts else 2
    return dict(chain_packed=chain_packed(opts, H, I), mlp8='mlp8' in opts, H=H, I=I, n_qkv=ops.skinny_rows((nq + 2 * nkv) * hd, 1 if 'qkv16' in opts else 2),
                n_gu=ops.skinny_rows(2 * I, tpu_gu), tpu_gu=tpu_gu, n_o=ops.skinny_rows(H, tpu_o), tpu_o=tpu_o, ks_o=ks_o, nq=nq, nkv=nkv, hd=hd)


def layer_path(*, chain_packed, H, I, n_qkv, n_gu, tpu_gu, n_o, tpu_o, ks_o, nq, nkv, hd, act_width, M, tok_per_batch, kv_len, n_partials=0, input_is_hB=False,
               skip_post_attn=False, dense_mask=False, mlp8=False):
    """(chain, chain_ao) of one skinny_layer call -- the ONE place that decides between the kernels of csrc/chain.hip and of csrc/skinny.hip (and the only caller of
    the library's *_supported predicates; those of the MLP through ops.chain_format, the one place that knows the weight formats).  Integers and booleans in
    (path_geometry of the stack + the call), no tensors.
    chain: q/k/v, gate/up and down on the latency-built kernels -- the layer takes a residual stream that is already reduced (n_partials == 0: the action encoder's output,
    or what the previous layer's vlaser_chain_down published; not hB, which this layer's gate/up launch overwrites while its other workgroups still read their input) and hands
    on (hC, None, 0).
    chain_ao: attention + o_proj on the one-wave-per-split attention / bf16-partial merge pair, when the key count gives a split count they are built for.
    A dense additive mask (ABI 8) is served by the chain attention only (every <= 16-row launch of the VLA at its shipped widths): NotImplementedError elsewhere.
    mlp8: the stack holds its MLP weights as e4m3 codes, which only the W8 forms of the chain gate/up and down kernels read: chain means those two launches, and a call
    that would run the MLP off the chain path raises NotImplementedError (a call that stops after q/k/v reads no MLP weight)."""
    fmt = ops.chain_format('e4m3' if mlp8 else 'bf16', H)
    mlp_ok = fmt.gu_supported(M, n_gu, H, ks_o, tpu_gu) and fmt.down_supported(M, H, I)
    chain = chain_packed and act_width == I and n_partials == 0 and not input_is_hB and ops.chain_qkv_supported(M, n_qkv, H) and mlp_ok
    if mlp8 and not chain and not skip_post_attn:
        raise NotImplementedError("'mlp8' (e4m3 MLP weights) needs the chain path: hidden 768 (<= 16 rows) / 1536 (<= 8 rows), MLP width 8960, an already reduced residual stream")
    chain_ao = (chain and not skip_post_attn and tpu_o == 1 and tok_per_batch * (nq // nkv) <= 32
                and ops.chain_oproj_supported(M, n_o, nq * hd, ks_o, ops.chain_attn_splits(kv_len), nq // nkv))
    if dense_mask and not (chain_ao or (chain and skip_post_attn)):
        raise NotImplementedError('dense additive masks need the chain attention (hidden 768 / 1536, <= 16 rows, group * tokens <= 32)')
    return chain, chain_ao


class QwenStack:
    """Weights + geometry of one Qwen2 decoder stack (the VLM LLM or the action expert)."""

    def __init__(self, sd, prefix, llm: LLMConfig, device, with_embed=True, with_head=True, gemm=True, skinny=True, opts=()):
        self.llm = llm
        self.opts = tuple(opts)
        self.nqd = llm.num_attention_heads * llm.head_dim
        self.tpu_o, self.ks_o, self.tpu_down, self.ks_down, self.I_pad = stack_geometry(llm)
        self.layers = [QwenLayerWeights(sd, f'{prefix}model.layers.{i}.', llm, device, self.ks_o, self.ks_down, gemm, skinny, self.tpu_down, self.tpu_o, self.I_pad, self.opts)
                       for i in range(llm.num_hidden_layers)]
        self.norm = _dev(sd[prefix + 'model.norm.weight'], device)
        self.embed = _dev(sd[prefix + 'model.embed_tokens.weight'], device) if with_embed else None
        self.head = _dev(sd[prefix + 'lm_head.weight'], device) if with_head and (prefix + 'lm_head.weight') in sd else None
        self.sk_head = ops.pack_skinny(self.head, 1) if (self.head is not None and skinny) else None
        self.path = p = path_geometry(llm, self.opts)
        for lw in self.layers if skinny else ():
            gu = lw.gu8 if p['mlp8'] else lw.sk_gu
            assert (lw.sk_qkv.N, gu.N, gu.tpu, lw.sk_o.N, lw.sk_o.tpu, (lw.down8 if p['mlp8'] else lw.sk_down4) is not None) == \
                (p['n_qkv'], p['n_gu'], p['tpu_gu'], p['n_o'], p['tpu_o'], p['chain_packed']), 'path_geometry disagrees with the packed weights'

    @property
    def nq(self):
        return self.llm.num_attention_heads

    @property
    def nkv(self):
        return self.llm.num_key_value_heads


class KVCache:
    """K [L][B,n_kv,S_max,128] and V^T [L][B,n_kv,128,S_max], zero-initialised (padding must stay finite)."""

    def __init__(self, n_layers, batch, n_kv, s_max, device, head_dim=128):
        assert s_max % 64 == 0
        self.s_max, self.batch, self.n_kv, self.hd = s_max, batch, n_kv, head_dim
        self.k = torch.zeros(n_layers, batch, n_kv, s_max, head_dim, dtype=BF, device=device)
        self.vt = torch.zeros(n_layers, batch, n_kv, head_dim, s_max, dtype=BF, device=device)

    def strides(self):
        return (self.n_kv * self.s_max * self.hd, self.s_max * self.hd), (self.n_kv * self.hd * self.s_max, self.hd * self.s_max)


# ------------------------------------------------------------------------------------------------------ ViT
class VitEngine:
    """InternViT-300M + pixel_shuffle + mlp1 (modeling_intern_vit.py:133-431, modeling_internvl_chat.py:257-291)."""

    KPAD = 640

    def __init__(self, sd, cfg: VlaserConfig, device, max_tiles=1):
        v = cfg.vision
        self.cfg, self.v, self.device = cfg, v, device
        g = lambda k: _dev(sd[k], device)
        e = 'vision_model.embeddings.'
        self.w_pe = ops.pack_patch_embed(g(e + 'patch_embedding.weight'), self.KPAD)
        self.b_pe = g(e + 'patch_embedding.bias')
        self.cls = g(e + 'class_embedding').reshape(-1)
        self.pos = g(e + 'position_embedding').reshape(v.num_positions, v.hidden_size)
        self.layers = []
        for i in range(v.num_hidden_layers):
            p = f'vision_model.encoder.layers.{i}.'
            self.layers.append({k: g(p + n) for k, n in [
                ('wqkv', 'attn.qkv.weight'), ('bqkv', 'attn.qkv.bias'), ('wproj', 'attn.proj.weight'), ('bproj', 'attn.proj.bias'),
                ('wfc1', 'mlp.fc1.weight'), ('bfc1', 'mlp.fc1.bias'), ('wfc2', 'mlp.fc2.weight'), ('bfc2', 'mlp.fc2.bias'),
                ('n1w', 'norm1.weight'), ('n1b', 'norm1.bias'), ('n2w', 'norm2.weight'), ('n2b', 'norm2.bias'),
                ('ls1', 'ls1'), ('ls2', 'ls2')]})
        self.m0w, self.m0b = g('mlp1.0.weight'), g('mlp1.0.bias')
        self.m1w, self.m1b = g('mlp1.1.weight'), g('mlp1.1.bias')
        self.m3w, self.m3b = g('mlp1.3.weight'), g('mlp1.3.bias')
        self.max_tiles = 0
        self._alloc(max_tiles)

    def _alloc(self, T):
        if T <= self.max_tiles:
            return
        v, dev = self.v, self.device
        S, C, Hn = v.num_positions, v.hidden_size, v.num_attention_heads
        self.s_pad = (S + 63) // 64 * 64
        z = lambda *s: torch.zeros(*s, dtype=BF, device=dev)
        self.col = z(T * v.num_patches, self.KPAD)
        self.patch = z(T * v.num_patches, C)
        self.h = z(T * S, C)
        self.x = z(T * S, C)
        self.q = z(T, Hn, self.s_pad, v.head_dim)
        self.k = z(T, Hn, self.s_pad, v.head_dim)
        self.vt = z(T, Hn, v.head_dim, self.s_pad)
        self.ao = z(T * S, C)
        self.f = z(T * S, v.intermediate_size)
        n_tok = T * self.cfg.num_image_token
        self.psln = z(n_tok, 4 * C)
        self.g = z(n_tok, self.cfg.llm.hidden_size)
        self.feat = z(n_tok, self.cfg.llm.hidden_size)
        self.part = torch.zeros(ops.split_slab_elems(T * S, C), dtype=torch.float32, device=dev)      # split-K slabs of proj / fc2
        self.max_tiles = T

    def forward(self, pixel_values, return_layers=False, project=True):
        """pixel_values bf16 [T,3,448,448] -> projected visual tokens bf16 [T*256, H_llm] (view into a workspace).  `project=False` stops after the
        encoder (last hidden state in `self.h`): the SFT step runs the trainable projector itself, keeping the intermediates its backward needs."""
        v, cfg = self.v, self.cfg
        T = pixel_values.shape[0]
        assert pixel_values.dtype == BF and pixel_values.is_contiguous() and pixel_values.shape[1:] == (3, v.image_size, v.image_size)
        self._alloc(T)
        S, C, Hn, hd, sp = v.num_positions, v.hidden_size, v.num_attention_heads, v.head_dim, self.s_pad
        M = T * S
        h, x, ao, f = self.h[:M], self.x[:M], self.ao[:M], self.f[:M]
        ops.im2col(pixel_values, self.col, T, v.image_size, self.KPAD)
        ops.linear(self.col[:T * v.num_patches], self.w_pe, self.b_pe, out=self.patch[:T * v.num_patches])
        ops.vit_assemble(self.patch, self.cls, self.pos, h, T, v.num_patches, C)
        layers_out = []
        if return_layers:
            layers_out.append(h.clone())
        # split-K factors for the two N = C outputs (proj, fc2): M*C/128^2 tiles alone cannot fill 256 CUs
        sp_proj, sp_fc2 = ops.gemm_splits(M, C, C, self.part.numel()), ops.gemm_splits(M, C, v.intermediate_size, self.part.numel())
        nl = len(self.layers)
        ops.layernorm(h, self.layers[0]['n1w'], self.layers[0]['n1b'], v.layer_norm_eps, out=x)
        for li, lw in enumerate(self.layers):
            ops.gemm(L.EPI_VIT_QKV, x, lw['wqkv'], bias=lw['bqkv'], vq=self.q, vk=self.k, vvt=self.vt, vit_heads=Hn, vit_seq=S,
                     vit_seq_pad=sp, q_scale=hd ** -0.5)
            ops.attn_prefill(self.q, self.k, self.vt, ao, T, S, S, Hn, Hn, hd, (Hn * sp * hd, sp * hd, hd), (Hn * sp * hd, sp * hd),
                             (Hn * hd * sp, hd * sp), (S * C, C), sp, 1.0, L.ATTN_FULL)
            # h += ls1 * (proj(ao) + b); x = LN2(h)      (modeling_intern_vit.py:291)
            residual_seam(ao, lw['wproj'], h, self.part, M, C, C, x, bias=lw['bproj'], ls=lw['ls1'], norm=2, norm_w=lw['n2w'], norm_b=lw['n2b'],
                          eps=v.layer_norm_eps, splits=sp_proj)
            ops.gemm(L.EPI_BIAS_GELU, x, lw['wfc1'], out=f, bias=lw['bfc1'])
            # h += ls2 * (fc2(f) + b); x = LN1 of the NEXT layer (:293)
            nxt = self.layers[li + 1] if li + 1 < nl else None
            residual_seam(f, lw['wfc2'], h, self.part, M, C, v.intermediate_size, x if nxt else None, bias=lw['bfc2'], ls=lw['ls2'], norm=2 if nxt else 0,
                          norm_w=nxt['n1w'] if nxt else None, norm_b=nxt['n1b'] if nxt else None, eps=v.layer_norm_eps, splits=sp_fc2)
            if return_layers:
                layers_out.append(h.clone())
        if not project:
            return layers_out if return_layers else None
        n_tok = T * cfg.num_image_token
        G = v.image_size // v.patch_size
        ops.pixel_shuffle_ln(h, self.m0w, self.m0b, self.psln, T, G, C, 1e-5, 1 if cfg.ps_version == 'v1' else 0)
        ops.gemm(L.EPI_BIAS_GELU, self.psln[:n_tok], self.m1w, out=self.g[:n_tok], bias=self.m1b)
        ops.gemm(L.EPI_BIAS, self.g[:n_tok], self.m3w, out=self.feat[:n_tok], bias=self.m3b)
        if return_layers:
            return self.feat[:n_tok], layers_out
        return self.feat[:n_tok]


def seam_is_split(sp, M):
    """Whether residual_seam takes its split-K GEMM + fused reduce / residual / norm composition (two launches) for `sp` slabs of M rows."""
    return sp >= 3 or (sp == 2 and M < 2048)


def residual_seam(a, w, h, part, M, N, K, x_out=None, bias=None, ls=None, norm=0, norm_w=None, norm_b=None, eps=1e-6, splits=None):
    """The seam behind an N = hidden GEMM: h += [ls *] (a @ w^T [+ bias]); x_out = norm(h) (norm: 0 none / 1 RMS / 2 LayerNorm).  Two compositions of the same arithmetic
    and the same rounding points (h rounded to bf16 once, the norm taken of the rounded h):
      * few row tiles, long K (the output tiles alone cannot fill 256 CUs): split-K GEMM -> fp32 slabs -> ONE fused reduce + residual + norm launch;
      * ONE slab, or two slabs of >= 2048 rows: whole-K GEMM with the residual in its epilogue + a stand-alone norm launch.  Measured (r06, tools/micro/seam_ab.py,
        profiles/r06x_seam_ab.md): 9-13 us less for the 13-tile ViT proj / fc2 (1 slab), 11 us for the 8B o_proj (1 slab), 96 us for the 8B down_proj at S = 3408 (2 slabs):
        with one or two large slabs the fp32 slab round trip (2 x 49 MB at 3408 x 3584) costs more than the split buys.  One slab is bit-identical to the slab path; two differ in
        the fp32 summation order.  (The one-tile ViT proj, 2 slabs of 1025 rows, is 3 us faster as a pair in isolation and EQUAL inside the chunk -- same-box A/B 11.775 vs
        11.778 ms -- so the small shapes keep the slab path and their bit-exact history.)"""
    sp = ops.gemm_splits(M, N, K, part.numel()) if splits is None else splits
    if seam_is_split(sp, M):
        ops.gemm(L.EPI_PARTIAL, a, w, out_f32=part, k_splits=sp)
        ops.reduce_norm(h, part, sp, M, N, h, x_out, bias=bias, ls=ls, norm=norm if x_out is not None else 0, norm_w=norm_w, norm_b=norm_b, eps=eps)
        return
    if ls is not None:
        ops.gemm(L.EPI_BIAS_LS_RES, a, w, out=h, bias=bias, res=h, ls=ls)
    else:
        assert bias is None
        ops.gemm(L.EPI_RES, a, w, out=h, res=h)
    if x_out is not None and norm == 2:
        ops.layernorm(h, norm_w, norm_b, eps, out=x_out)
    elif x_out is not None and norm == 1:
        ops.rmsnorm(h, norm_w, eps, out=x_out)


# ------------------------------------------------------------------------------------------------------ LLM
class PrefillBuffers:
    def __init__(self, stack: QwenStack, max_rows, device):
        llm = stack.llm
        z = lambda *s: torch.zeros(*s, dtype=BF, device=device)
        self.x = z(max_rows, llm.hidden_size)
        self.q = z(max_rows, stack.nq * llm.head_dim)
        self.ao = z(max_rows, stack.nq * llm.head_dim)
        self.act = z(max_rows, llm.intermediate_size)
        self.max_rows = max_rows
        # split-K slabs of o_proj / down_proj: sized once (a HIP graph may have captured the address)
        self.part = torch.zeros(ops.split_slab_elems(max_rows, llm.hidden_size), dtype=torch.float32, device=device)
        self.device = device


def prefill_begin(stack: QwenStack, buf: PrefillBuffers, h, M):
    """x = input_layernorm_0(h): the only stand-alone norm launch of a prefill (later norms are fused into the split-K seam)."""
    ops.rmsnorm(h, stack.layers[0].ln_in, stack.llm.rms_norm_eps, out=buf.x[:M])


def prefill_layer_launches(stack: QwenStack, lw: QwenLayerWeights, buf: PrefillBuffers, h, cache: KVCache, layer, rope, pos_ids, batch,
                           tok_per_batch, attn_mode, valid_len=None, blk_start=0, causal_off=0, kv_len=None, skip_post_attn=False,
                           next_norm_w=None, slot_base=0, dense_mask=None):
    """prefill_layer as its launches in order: [(name, fn)], run as fn() -- or fn(guest=...) for a co-hosted launch (ops.cohost_guest; PiZero._run_joint).  Names: 'qkv',
    'attn', then per split-K seam its GEMM and its reduce + residual + norm launch: 'o', 'seam_o', 'gu', 'down', 'seam_d'.  A seam that residual_seam composes
    the other way (whole-K GEMM with the residual in its epilogue + a norm launch) is ONE entry, 'o' / 'down', that takes no guest."""
    llm = stack.llm
    M = batch * tok_per_batch
    nq, nkv, hd = stack.nq, stack.nkv, llm.head_dim
    H, I = llm.hidden_size, llm.intermediate_size
    x, q, ao, act = buf.x[:M], buf.q[:M], buf.ao[:M], buf.act[:M]
    out = [('qkv', lambda guest=None: ops.gemm(L.EPI_QKV_ROPE, x, lw.wqkv, bias=lw.bqkv, q_out=q, k_cache=cache.k[layer], vt_cache=cache.vt[layer], rope_cos=rope[0],
                                              rope_sin=rope[1], pos_ids=pos_ids, n_q_heads=nq, n_kv_heads=nkv, s_max=cache.s_max, tok_per_batch=tok_per_batch,
                                              slot_base=slot_base, guest=guest))]
    if skip_post_attn:          # the last layer of a mixture whose hidden states nobody reads (the VLM / proprio rows of the VLA): only its K / V are needed
        return out
    ks, vs = cache.strides()
    out.append(('attn', lambda guest=None: ops.attn_prefill(
        q, cache.k[layer], cache.vt[layer], ao, batch, tok_per_batch, tok_per_batch if kv_len is None else kv_len, nq, nkv, hd,
        (tok_per_batch * nq * hd, hd, nq * hd), ks, vs, (tok_per_batch * nq * hd, nq * hd), cache.s_max, hd ** -0.5,
        L.ATTN_DENSE if dense_mask is not None else attn_mode, causal_off=causal_off, valid_len=valid_len, blk_start=blk_start, q_row_off=slot_base,
        dense_mask=dense_mask, guest=guest)))        # dense_mask: fp32 view [B, tok_per_batch, >= kv_len] of the reference's additive mask (general masks, ABI 8)
    part = buf.part
    eps = llm.rms_norm_eps

    def seam(name, a, w, K, x_out, norm_w):
        sp = ops.gemm_splits(M, H, K, part.numel())
        norm = 1 if x_out is not None else 0
        if not seam_is_split(sp, M):
            def whole(guest=None):
                assert guest is None, 'a whole-K seam hosts no guest'
                residual_seam(a, w, h, part, M, H, K, x_out, norm=norm, norm_w=norm_w, eps=eps, splits=sp)
            return [(name, whole)]
        return [(name, lambda guest=None: ops.gemm(L.EPI_PARTIAL, a, w, out_f32=part, k_splits=sp, guest=guest)),
                ('seam_' + name[0], lambda guest=None: ops.reduce_norm(h, part, sp, M, H, h, x_out, norm=norm, norm_w=norm_w, eps=eps, guest=guest))]

    out += seam('o', ao, lw.wo, nq * hd, x, lw.ln_post)
    out.append(('gu', lambda guest=None: ops.gemm(L.EPI_SWIGLU, x, lw.wgu, out=act, guest=guest)))
    out += seam('down', act, lw.wdown, I, x if next_norm_w is not None else None, next_norm_w)
    return out


def prefill_layer(stack: QwenStack, lw: QwenLayerWeights, buf: PrefillBuffers, h, cache: KVCache, layer, rope, pos_ids, batch,
                  tok_per_batch, attn_mode, valid_len=None, blk_start=0, causal_off=0, kv_len=None, skip_post_attn=False,
                  next_norm_w=None, slot_base=0, dense_mask=None):
    """One Qwen2DecoderLayer over M = batch*tok_per_batch rows with the big-GEMM kernels; K/V written to slots
    [slot_base, slot_base + tok_per_batch) of the cache (slot_base > 0: decode steps of models too wide for the
    weight-streaming kernels).  Expects buf.x = input_layernorm(h); leaves buf.x = next_norm(h_out) when
    next_norm_w is given (next layer's input_layernorm or the final norm).  h is updated in place.
    o_proj / down_proj run split-K (their [M, H] outputs have too few tiles to fill 256 CUs); the fp32 slabs are
    reduced by ONE fused kernel that also adds the residual and applies the following RMSNorm."""
    for _, fn in prefill_layer_launches(stack, lw, buf, h, cache, layer, rope, pos_ids, batch, tok_per_batch, attn_mode, valid_len, blk_start, causal_off, kv_len,
                                        skip_post_attn, next_norm_w, slot_base, dense_mask):
        fn()


class SkinnyBuffers:
    """Workspace of the M <= 16 weight-streaming path (decode / proprio row / action tokens)."""

    def __init__(self, stack: QwenStack, max_rows, device):
        llm = stack.llm
        H, I = llm.hidden_size, llm.intermediate_size
        z = lambda *s: torch.zeros(*s, dtype=BF, device=device)
        self.hA, self.hB, self.hC = z(max_rows, H), z(max_rows, H), z(max_rows, H)      # hC: the residual stream as `vlaser_chain_down` publishes it
        self.q = z(max_rows, stack.nq * llm.head_dim)
        self.ao = z(max_rows, stack.nq * llm.head_dim)
        self.act = z(max_rows, getattr(stack, 'I_pad', I))      # zero padding columns (never written) feed the zero-padded down weight
        self.attn_parts = ops.attn_partial_buffers(max_rows, stack.nkv, device)
        self.chain_parts = ops.chain_attn_buffers(max_rows, stack.nkv, device)          # r05: (m, l) pairs + normalised bf16 rows of vlaser_chain_attn
        self.part_o = torch.zeros(stack.ks_o, max_rows, H, dtype=torch.float32, device=device)
        self.part_d = torch.zeros(stack.ks_down, max_rows, H, dtype=torch.float32, device=device)
        self.plans = {}      # cached launch argument structs of skinny_layer


def skinny_layer(stack: QwenStack, lw: QwenLayerWeights, sb: SkinnyBuffers, h_in, partials, n_partials, cache: KVCache, layer, rope,
                 pos_ids, batch, tok_per_batch, slot_base, kv_len, attn_mode, valid_len=None, blk_start=0, skip_post_attn=False,
                 first_tok_kv_len=0, skip=(), dense_mask=None):
    """One decoder layer over M = batch*tok_per_batch <= 16 rows with the weight-streaming kernels (5 launches).
    Input residual = h_in + sum(partials) (partials = down_proj slabs of the previous layer).  Returns
    (h, partials, n_partials) describing this layer's output residual the same way.
    The kernel path (layer_path), the argument structs and the launch list of a (layer, input buffers, geometry) are built once and re-launched: only the cache slot,
    the key count and its split factor change from step to step (greedy decode is otherwise host-bound on deciding and struct building)."""
    plan = skinny_layer_plan(stack, lw, sb, h_in, partials, n_partials, cache, layer, rope, pos_ids, batch, tok_per_batch, slot_base, kv_len, attn_mode, valid_len,
                             blk_start, skip_post_attn, first_tok_kv_len, dense_mask)
    stream = torch.cuda.current_stream().cuda_stream
    for name, launch, args in plan.launches:
        if name not in skip:                  # `skip` (bench.py only): in-chain timing of one launch = chain with it - chain without it
            launch(*args, stream)
    return plan.result


def skinny_layer_plan(stack, lw, sb, h_in, partials, n_partials, cache, layer, rope, pos_ids, batch, tok_per_batch, slot_base, kv_len, attn_mode, valid_len=None,
                      blk_start=0, skip_post_attn=False, first_tok_kv_len=0, dense_mask=None):
    """The plan of a skinny_layer call, brought up to date for this call (cache slot, key count, split factor), without launching anything: .launches in order,
    .result = what the layer hands on."""
    M = batch * tok_per_batch
    # the key holds what the plan depends on; of kv_len, the path only reads whether the chain attention + o_proj pair is built for its split count (1..16)
    key = (layer, M, tok_per_batch, attn_mode, h_in.data_ptr(), 0 if partials is None else partials.data_ptr(), n_partials,
           0 if valid_len is None else valid_len.data_ptr(), pos_ids.data_ptr(), cache.k.data_ptr(), skip_post_attn, first_tok_kv_len,
           0 < ops.chain_attn_splits(kv_len) <= 16, 0 if dense_mask is None else dense_mask.data_ptr())
    plan = sb.plans.get(key)
    if plan is None:
        plan = _build_plan(stack, lw, sb, h_in, partials, n_partials, cache, layer, rope, pos_ids, batch, tok_per_batch, slot_base, kv_len, attn_mode, valid_len,
                           blk_start, skip_post_attn, first_tok_kv_len, dense_mask)
        if len(sb.plans) > 4096:         # keys hold buffer addresses of per-call tensors (ragged lengths): bound the cache
            sb.plans.clear()
        sb.plans[key] = plan
    nsp = ops.chain_attn_splits(kv_len) if plan.chain_ao else ops.attn_splits(kv_len)
    plan.qkv[0].slot_base = slot_base
    a = plan.attn
    a.kv_len, a.n_splits, a.blk_start = kv_len, nsp, blk_start
    if not skip_post_attn:
        plan.o[0].attn_splits = nsp          # (the key count, hence the split count, moves from step to step in an eager decode)
    return plan


def plan_guest(plan, name):
    """Launch `name` of a chain plan (chain and chain_ao) as the guest descriptor of a co-hosted launch; built once per plan.  Its kind is the plan's weight format's
    (ops.chain_format: the gate/up and down launches of an 'mlp8' plan are the W8 kinds); it points at the plan's own argument struct for `name`, so what skinny_layer_plan
    brings up to date is what the host's launch reads (a struct whose `dbg` is set is refused by the fused path and runs host-then-guest)."""
    g = plan.guests.get(name)
    if g is None:
        assert plan.chain and plan.chain_ao
        kind, a = plan.format.guests[name], getattr(plan, name)
        assert kind is not None, (name, 'has no guest form in this weight format')
        g = plan.guests[name] = ops.cohost_guest(kind, a[0] if isinstance(a, tuple) else a)
    return g


def _build_plan(stack, lw, sb, h_in, partials, n_partials, cache, layer, rope, pos_ids, batch, tok_per_batch, slot_base, kv_len, attn_mode, valid_len, blk_start,
                skip_post_attn, first_tok_kv_len, dense_mask):
    """The plan of one skinny_layer key: .chain / .chain_ao (layer_path), .format (ops.chain_format of the stack's MLP weights), the argument structs .qkv / .attn / .o / .gu / .down
    (every launch has one; tools set their `dbg`, read at launch time), .launches =
    [(name, launch, args)] in launch order, run as launch(*args, stream) (tuples, not closures over the plan: a cleared cache frees its plans at once), .result = the (h, partials, n_partials) the layer hands on.
    (The two fused launches of r03 / r04 -- o_proj -> gate/up with an in-launch hand-off, attention + o_proj in one launch -- lost to the r05 chain kernels and were
    removed from the library: DESIGN.md section 3)"""
    llm = stack.llm
    M = batch * tok_per_batch
    nq, nkv, hd = stack.nq, stack.nkv, llm.head_dim
    H, I = llm.hidden_size, llm.intermediate_size
    chain, chain_ao = layer_path(**stack.path, act_width=sb.act.shape[1], M=M, tok_per_batch=tok_per_batch, kv_len=kv_len, n_partials=n_partials,
                                 input_is_hB=h_in.data_ptr() == sb.hB.data_ptr(), skip_post_attn=skip_post_attn, dense_mask=dense_mask is not None)
    if dense_mask is not None:
        attn_mode = L.ATTN_DENSE
    ks, vs = cache.strides()
    mlp8 = stack.path['mlp8']          # (layer_path has raised if the MLP of an 'mlp8' stack would leave the chain path)
    plan = SimpleNamespace(chain=chain, chain_ao=chain_ao, format=ops.chain_format('e4m3' if mlp8 else 'bf16', H), guests={})
    plan.qkv = ops.skinny_args(h_in, lw.sk_qkv, M, partials=partials, n_partials=n_partials, norm_w=lw.ln_in, eps=llm.rms_norm_eps,
                               h_out=sb.hA, bias=lw.bqkv_sk, q_out=sb.q, k_cache=cache.k[layer], vt_cache=cache.vt[layer], rope_cos=rope[0],
                               rope_sin=rope[1], pos_ids=pos_ids, n_q_heads=nq, n_kv_heads=nkv, s_max=cache.s_max,
                               tok_per_batch=tok_per_batch, slot_base=slot_base)
    # chain_ao: (m, l) pairs + normalised bf16 rows per split; else flash-decoding partials that the o_proj prologue merges straight into its activation tile
    attn_parts = (sb.chain_parts[0], sb.chain_parts[0], sb.chain_parts[1]) if chain_ao else sb.attn_parts
    plan.attn = ops.attn_skinny_args(sb.q, cache.k[layer], cache.vt[layer], attn_parts, batch, tok_per_batch, kv_len, nq, nkv, hd,
                                     (tok_per_batch * nq * hd, hd, nq * hd), ks, vs, cache.s_max, hd ** -0.5, attn_mode, 1,
                                     valid_len=valid_len, blk_start=blk_start, first_tok_kv_len=first_tok_kv_len, dense_mask=dense_mask if chain_ao else None)
    plan.launches = [('qkv', ops.launch_chain_qkv, (plan.qkv[0],)) if chain else ('qkv', ops.launch_skinny, (L.PRO_NORM, L.SK_QKV_ROPE, plan.qkv[0]))]
    if skip_post_attn:          # only this layer's K / V are needed (written by the qkv launch); the chain q/k/v leaves no rounded copy of its input behind -- it IS the rounded stream
        plan.result = (h_in if chain else sb.hA, None, 0)
        return plan
    if chain_ao:
        plan.o = ops.skinny_args(None, lw.sk_o, M, out_f32=sb.part_o, attn_m=sb.chain_parts[0], attn_o=sb.chain_parts[1], attn_splits=1,
                                 attn_group=nq // nkv, attn_nq=tok_per_batch)
        plan.launches += [('attn', ops.launch_chain_attn, (plan.attn,)), ('o', ops.launch_chain_oproj, (plan.o[0],))]
    else:
        plan.o = ops.skinny_args(None, lw.sk_o, M, out_f32=sb.part_o, attn_m=sb.attn_parts[0], attn_l=sb.attn_parts[1],
                                 attn_o=sb.attn_parts[2], attn_splits=1, attn_group=nq // nkv, attn_nq=tok_per_batch)
        plan.launches += [('attn', ops.launch_attn_skinny, (plan.attn,)), ('o', ops.launch_skinny, (L.PRO_ATTN, L.SK_PARTIAL, plan.o[0]))]
    plan.gu = ops.skinny_args(h_in if chain else sb.hA, lw.gu8 if mlp8 else lw.sk_gu, M, partials=sb.part_o, n_partials=stack.ks_o, norm_w=lw.ln_post,
                              eps=llm.rms_norm_eps, h_out=sb.hB, out=sb.act, ldo=sb.act.shape[1])
    if chain:
        plan.down = ops.chain_down_args(sb.act, lw.down8 if mlp8 else lw.sk_down4, sb.hB, sb.hC, M, H, I, lw.down8_scale if mlp8 else None)
        plan.launches += [('gu', plan.format.launch_gu, (plan.gu[0],)), ('down', ops.launch_chain_down, (plan.down,))]
        plan.result = (sb.hC, None, 0)
    else:
        plan.down = ops.skinny_args(sb.act, lw.sk_down, M, out_f32=sb.part_d)
        plan.launches += [('gu', ops.launch_skinny, (L.PRO_NORM, L.SK_SWIGLU, plan.gu[0])), ('down', ops.launch_skinny, (L.PRO_PLAIN, L.SK_PARTIAL, plan.down[0]))]
        plan.result = (sb.hB, sb.part_d, stack.ks_down)
    return plan
