"""CPU: the host side of the Vlaser-2B LLM's one-byte MLP weights (decode option 'mlp8', InternVLChatModel(llm_mlp_weights='fp8')): the e4m3 gate/up packing at
K = 1536 and its inverse against the bf16 packing's lane contents, the predicate / refusals of vlaser_chain_gu_w8_k1536, the kernel-path decision at hidden 1536, the
pure resolution of the decode options, and what a QwenStack with GEMM packings holds under 'mlp8'.  Needs the built library (host functions only), no GPU."""
import ctypes

import pytest
import torch

from vlaser_amd import config as C
from vlaser_amd import engine as E
from vlaser_amd import ops, synth
from vlaser_amd.internvl_chat import DECODE_DEFAULT, resolve_decode_opts

BF = torch.bfloat16
H, I2B = 1536, 8960
CHAIN = ('qkv16', 'gu16', 'chain')


def _codes(N, K, seed):
    """random codes over all 254 finite e4m3 values"""
    finite = torch.tensor([v for v in range(256) if v & 0x7F != 0x7F], dtype=torch.uint8)
    return finite[torch.randint(0, 254, (N, K), generator=torch.Generator().manual_seed(seed))]


@pytest.mark.parametrize('I', [8960, 8208])
def test_gate_up_packing_k1536_roundtrip_and_lanes(I):
    cg, cu = _codes(I, H, 1), _codes(I, H, 2)
    sg, su = torch.rand(I, generator=torch.Generator().manual_seed(3)) + 0.5, torch.rand(I, generator=torch.Generator().manual_seed(4)) + 0.5
    W = ops.pack_gate_up8_e4m3(cg, sg, cu, su)
    assert (W.N, W.n_valid, W.K, W.k_splits, W.tpu) == (2 * I, 2 * I, H, 1, 1)
    assert W.t.dtype == torch.uint8 and W.t.numel() == 2 * I * H and W.scale.dtype == torch.float32 and W.scale.numel() == 2 * I        # no padding
    a, b, c, d = ops.unpack_gate_up8_e4m3(W)
    assert torch.equal(a, cg) and torch.equal(b, sg) and torch.equal(c, cu) and torch.equal(d, su)
    # every lane receives the elements of the bf16 packing, in its order: bf16 [u][wave][K-step s][lane][8]; e4m3 [u][wave][load j][lane][s = 2j, 2j + 1][8]
    ref = ops.pack_skinny(ops.pack_gate_up8(cg, cu).to(torch.int16), 1, 1)            # (a permutation: any dtype)
    assert ref.N == W.N
    ref = ref.t.view(W.N // 16, 8, 6, 64, 8)
    t = W.t.view(W.N // 16, 8, 3, 64, 2, 8)              # a wave's share of a unit: 3 x 64 x 16 = 3072 contiguous bytes
    for j in range(3):
        for s2 in range(2):
            assert torch.equal(t[:, :, j, :, s2].to(torch.int16), ref[:, :, 2 * j + s2]), (j, s2)
    assert torch.equal(W.scale, ops.pack_gate_up8(sg[:, None], su[:, None]).reshape(-1))      # scales in packed row order
    assert ops.GU8_WAVE_BYTES == 1536                     # the K = 768 layout keeps its constant


def test_k1536_predicate_mirrors_its_dispatch_table():
    from vlaser_amd import _lib
    lib = _lib.lib()
    built = {(6, 5, 2, 1)}                   # {K / 256, units per workgroup, slabs, tiles per unit}: what the Vlaser-2B decode reaches
    for ns in (2, 3, 4, 6):
        for longest in (1, 2, 3, 4, 5, 6):
            for sp in (1, 2, 3, 4):
                for tpu in (1, 2):
                    N = 16 * tpu * (256 * (longest - 1) + 100)
                    got = lib.vlaser_chain_gu_w8_k1536_supported(4, N, ns * 256, sp, tpu)
                    assert got == int((ns, longest, sp, tpu) in built), (ns, longest, sp, tpu, got)
    for M in range(1, 9):                    # every chunks-per-thread value (1, 2, 3)
        assert lib.vlaser_chain_gu_w8_k1536_supported(M, 17920, H, 2, 1) == 1 and lib.vlaser_chain_gu_w8_k1536_supported(M, 16416, H, 2, 1) == 1
    assert lib.vlaser_chain_gu_w8_k1536_supported(0, 17920, H, 2, 1) == 0 and lib.vlaser_chain_gu_w8_k1536_supported(9, 17920, H, 2, 1) == 0
    assert ops.chain_gu_w8_k1536_supported(8, 17920, H, 2) and not ops.chain_gu_w8_k1536_supported(9, 17920, H, 2)
    # the down projection's W8 form already serves N = 1536 up to 8 rows
    assert ops.chain_down_w8_supported(8, H, I2B) and not ops.chain_down_w8_supported(9, H, I2B)


def test_k1536_bad_arguments_return_errors_not_crashes():
    """Argument validation happens on the host before any launch: exercised without a GPU."""
    from vlaser_amd import _lib
    lib = _lib.lib()
    P = 4096
    call = lambda s: lib.vlaser_chain_gu_w8_k1536(ctypes.byref(s), None)
    s = _lib.SkinnyArgs()
    assert call(s) != 0 and b'null' in lib.vlaser_last_error()
    s.x, s.W, s.norm_w, s.out, s.partials = P, P, P, P, P
    s.M, s.N, s.K, s.n_partials, s.tiles_per_unit, s.k_splits, s.ldo = 4, 17920, H, 2, 1, 1, 8960
    assert call(s) != 0 and b'null w_scale' in lib.vlaser_last_error()
    s.w_scale = P + 4
    assert call(s) != 0 and b'alignment' in lib.vlaser_last_error()
    s.w_scale, s.W = P, P + 8
    assert call(s) != 0 and b'alignment' in lib.vlaser_last_error()
    s.W = P
    for field, bad in (('K', 768), ('n_partials', 3), ('tiles_per_unit', 2), ('M', 9)):
        good = getattr(s, field)
        setattr(s, field, bad)
        assert call(s) != 0 and b'vlaser_chain_gu_w8_k1536: built for' in lib.vlaser_last_error(), field
        setattr(s, field, good)


def _path(opts, M, tok, kv_len, **kw):
    llm = C.vlaser_2b().llm
    return E.layer_path(**E.path_geometry(llm, opts), act_width=E.stack_geometry(llm)[4], M=M, tok_per_batch=tok, kv_len=kv_len, **kw)


def test_layer_path_mlp8_at_hidden_1536():
    assert (C.vlaser_2b().llm.hidden_size, C.vlaser_2b().llm.intermediate_size) == (H, I2B)
    assert E.path_geometry(C.vlaser_2b().llm, CHAIN + ('mlp8',))['mlp8'] is True
    for M in range(1, 9):
        assert _path(CHAIN + ('mlp8',), M, 1, 300)[0] is True
        assert _path(CHAIN + ('mlp8',), M, 1, 300) == _path(CHAIN, M, 1, 300)          # the same launches of the other kernels
    with pytest.raises(NotImplementedError, match='mlp8'):          # never a silent fallback to kernels that would read codes as bf16
        _path(CHAIN + ('mlp8',), 9, 1, 300)
    with pytest.raises(NotImplementedError, match='mlp8'):
        _path(CHAIN + ('mlp8',), 4, 1, 300, n_partials=2)
    # a call that stops after q/k/v reads no MLP weight
    assert _path(CHAIN + ('mlp8',), 9, 1, 300, skip_post_attn=True) == (False, False)
    assert _path(CHAIN + ('mlp8',), 4, 1, 300, skip_post_attn=True) == (True, False)
    # without the option 9 rows go to the skinny kernels as before
    assert _path(CHAIN, 9, 1, 300) == (False, False)


def test_resolve_decode_opts():
    llm2, llm8 = C.vlaser_2b().llm, C.vlaser_8b().llm
    assert resolve_decode_opts(llm2) == (CHAIN, 16) == (tuple(DECODE_DEFAULT.split(',')), 16)
    assert resolve_decode_opts(llm2, 'bf16', None) == (CHAIN, 16)
    assert resolve_decode_opts(llm8) == ((), 16)
    assert resolve_decode_opts(llm2, 'bf16', 'none') == ((), 16) and resolve_decode_opts(llm2, 'bf16', 'qkv16') == (('qkv16',), 16)
    assert resolve_decode_opts(llm2, 'fp8') == (CHAIN + ('mlp8',), 8)
    assert resolve_decode_opts(llm2, 'bf16', 'qkv16,gu16,chain,mlp8') == (CHAIN + ('mlp8',), 8)          # the env form
    assert resolve_decode_opts(llm2, 'fp8', 'qkv16,gu16,chain,mlp8') == (CHAIN + ('mlp8',), 8)
    assert resolve_decode_opts(llm2, 'fp8', 'chain,gu16,qkv16') == (('chain', 'gu16', 'qkv16', 'mlp8'), 8)
    # the 768-wide stack (the action expert's widths) keeps the 16-row limit of its kernels
    assert resolve_decode_opts(C.VLAConfig(base=C.vlaser_2b()).expert, 'fp8') == (CHAIN + ('mlp8',), 16)
    with pytest.raises(ValueError, match='llm_mlp_weights'):
        resolve_decode_opts(llm2, 'int8')
    with pytest.raises(ValueError, match='chain, gu16'):
        resolve_decode_opts(llm2, 'bf16', 'qkv16,mlp8')
    with pytest.raises(ValueError, match='chain, qkv16, gu16'):
        resolve_decode_opts(llm2, 'fp8', 'none')
    with pytest.raises(ValueError, match='gu16'):
        resolve_decode_opts(llm2, 'fp8', 'qkv16,chain')
    with pytest.raises(ValueError, match='Vlaser-8B'):
        resolve_decode_opts(llm8, 'fp8')
    with pytest.raises(ValueError, match='Vlaser-8B'):
        resolve_decode_opts(llm8, 'bf16', 'qkv16,gu16,chain,mlp8')


def test_qwen_stack_with_gemm_packings_under_mlp8():
    """The VLM's LLM stack: e4m3 packings for the decode, GEMM packings of the DEQUANTISED weights for prefill / forward(), no bf16 weight-streaming MLP packing."""
    llm = C.truncated(C.vlaser_2b(), 1, 1).llm
    sd = synth.qwen2_state_dict('language_model.', llm, with_embed=False, with_head=False)
    st = E.QwenStack(sd, 'language_model.', llm, 'cpu', with_embed=False, with_head=False, gemm=True, skinny=True, opts=CHAIN + ('mlp8',))
    assert st.path['mlp8'] and st.path['chain_packed']
    Hh, I = llm.hidden_size, llm.intermediate_size
    p = 'language_model.model.layers.0.'
    dq = lambda k: ops.dequantize_rows_e4m3(*ops.quantize_rows_e4m3(sd[p + k]))
    lw = st.layers[0]
    assert lw.wgu.dtype == BF and torch.equal(lw.wgu, ops.pack_gate_up(dq('mlp.gate_proj.weight'), dq('mlp.up_proj.weight')))
    assert lw.wdown.dtype == BF and torch.equal(lw.wdown, dq('mlp.down_proj.weight'))
    assert not torch.equal(lw.wdown, sd[p + 'mlp.down_proj.weight'].to(BF))          # (the quantisation is not a no-op on these weights)
    assert lw.gu8.t.dtype == torch.uint8 and lw.gu8.t.numel() == 2 * I * Hh and lw.gu8.K == Hh and lw.gu8.scale.numel() == 2 * I
    assert lw.down8.dtype == torch.uint8 and lw.down8.numel() == Hh * I and lw.down8_scale.dtype == torch.float32
    gc, gs, uc, us = ops.unpack_gate_up8_e4m3(lw.gu8)
    assert torch.equal(ops.dequantize_rows_e4m3(gc, gs), dq('mlp.gate_proj.weight')) and torch.equal(ops.dequantize_rows_e4m3(uc, us), dq('mlp.up_proj.weight'))
    assert torch.equal(ops.dequantize_rows_e4m3(ops.unpack_down4_e4m3(lw.down8, Hh), ops.unpack_down4_scales(lw.down8_scale, Hh)), dq('mlp.down_proj.weight'))
    assert lw.sk_gu is None and lw.sk_down is None and lw.sk_down4 is None
    for name, v in vars(lw).items():
        t = v.t if isinstance(v, ops.PackedW) else v
        if isinstance(t, torch.Tensor) and name not in ('gu8', 'down8', 'wgu', 'wdown'):
            assert t.numel() < I * Hh, f'{name}: one more copy of an MLP matrix'
    # the refusals that stay: a stack without the chain packings
    for opts in (('qkv16', 'gu16', 'mlp8'), ('gu16', 'chain', 'mlp8'), ('qkv16', 'chain', 'mlp8')):
        with pytest.raises(ValueError, match='hidden 768 / 1536'):
            E.QwenStack(sd, 'language_model.', llm, 'cpu', with_embed=False, with_head=False, gemm=True, skinny=True, opts=opts)
