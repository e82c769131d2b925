"""GPU: the Vlaser-2B LLM's MLP on one-byte weights in the greedy decode (decode option 'mlp8', InternVLChatModel(llm_mlp_weights='fp8')): vlaser_chain_gu_w8_k1536
streams OCP e4m3 codes at K = 1536 (three 16-byte loads per lane and unit), vlaser_chain_down_w8 already serves N = 1536.  Every finite e4m3 value is exact in bf16 and a
power-of-two scale is exact on a bf16 value and on an fp32 sum, so the W8 kernel must return the BITS of the bf16 kernel run on the dequantised weights, and the fp8 model
-- whose prefill / forward() GEMMs read the dequantised weights -- the bits of the default model loaded with dequantize(quantize(.)) of the six MLP matrices:
torch.equal on ids and logits, kernel by kernel and through generate() / forward().  One kernel case with scales that are no powers of two goes against fp64 under the
bound the bf16 kernel has for the same contraction length plus one fp32 rounding (of the scaled sum); the model goes against the CPU oracle on the dequantised weights
under the default model's own bounds."""
import os

import numpy as np
import pytest
import torch

from bounds import D64, FLOOR, U, ULP, f32s, h64, rbf
from parity import parity, relmax

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
SENT = 7.0
H = 1536
TOL_LOGITS = 2.7e-2          # TOL['logits'] of tests/test_models_gpu.py: the fp8 model is bit-identical to the default model on the dequantised weights, whose bound this is


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vlaser_amd import ops as o
    return o


def rnd(*s, std=1.0, seed=0):
    return (torch.randn(*s, generator=torch.Generator().manual_seed(seed)) * std).to(BF).cuda()


def _codes(N, K, seed):
    """random codes over all 254 finite e4m3 values (subnormals and -0 included), CPU uint8"""
    finite = torch.tensor([v for v in range(256) if v & 0x7F != 0x7F], dtype=torch.uint8)
    return finite[torch.randint(0, 254, (N, K), generator=torch.Generator().manual_seed(seed))]


def _pow2_scales(N, seed):
    return 2.0 ** torch.randint(-12, -3, (N,), generator=torch.Generator().manual_seed(seed)).float()          # 2^-12 .. 2^-4


@pytest.fixture(scope='module')
def side():
    return torch.cuda.Stream(), torch.randn(2048, 2048, device='cuda')


def _busy(side, junk):
    with torch.cuda.stream(side):
        junk @ junk


def _gu_inputs(M, npart=2):
    h, nw = rnd(M, H), (1 + 0.1 * rnd(H, seed=5).float()).to(BF)
    parts = (torch.randn(npart, M, H, generator=torch.Generator().manual_seed(7)) * 0.3).cuda()
    return h, nw, parts


@pytest.mark.parametrize('I', [8960, 8208])              # 8208: 1026 units on 206 workgroups of 5 and 4 -- the workgroups of 4 re-request their last unit
@pytest.mark.parametrize('M', [2, 5, 8])                 # 1, 2 and 3 chunks of the residual stream per thread
def test_chain_gu_w8_k1536_bit_identical_to_bf16_on_dequantised_weights(ops, side, M, I):
    npart = 2
    assert ops.chain_gu_w8_k1536_supported(M, 2 * I, H, npart) and ops.chain_gu_supported(M, 2 * I, H, npart, 1)
    assert (M * (H // 8) + 511) // 512 == {2: 1, 5: 2, 8: 3}[M]
    h, nw, parts = _gu_inputs(M)
    cg, cu, sg, su = _codes(I, H, 1), _codes(I, H, 2), _pow2_scales(I, 3), _pow2_scales(I, 4)
    w8 = ops.pack_gate_up8_e4m3(cg, sg, cu, su).to('cuda')
    dg, du = ops.dequantize_rows_e4m3(cg, sg), ops.dequantize_rows_e4m3(cu, su)
    assert torch.equal(dg.double(), cg.view(F8).double() * sg.double()[:, None])           # exact in bf16
    wb = ops.pack_skinny(ops.pack_gate_up8(dg.cuda(), du.cuda()), 1, 1)

    def run(launch, W):
        out, hb = torch.full((M + 1, I), SENT, dtype=BF, device='cuda'), torch.full((M + 1, H), SENT, dtype=BF, device='cuda')
        a, _ = ops.skinny_args(h, W, M, partials=parts, n_partials=npart, norm_w=nw, h_out=hb, out=out, ldo=I)
        _busy(*side)
        launch(a)
        return out, hb

    o0, h0 = run(ops.launch_chain_gu, wb)
    assert bool((o0[:M] != SENT).any()) and bool(torch.isfinite(o0[:M].float()).all())
    for rep in range(2):
        o1, h1 = run(ops.launch_chain_gu_w8_k1536, w8)
        assert torch.equal(o1, o0) and torch.equal(h1, h0), rep
        assert bool((o1[M] == SENT).all()) and bool((h1[M] == SENT).all())
    torch.cuda.synchronize()


def _n_row(C):
    return 8 * ((C + 511) // 512) + 6         # as tests/test_fwd_ops_gpu.py: fp32 additions behind the sum of squares of a row


def _dsilu(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def _general_scales(N, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(N, generator=g) + 0.5) * 2.0 ** torch.randint(-10, -6, (N,), generator=g).float()).float()


def test_chain_gu_w8_k1536_general_scales_vs_fp64(ops):
    """Scales that are no powers of two: out = bf16(bf16(silu(bf16(s_g G))) * bf16(s_u U)) with G = sum_k code[n, k] x[k] in fp64, x = the fp64 RMSNorm of the residual
    stream the kernel itself published (h_out).  The bound of tests/test_fp8_mlp_gpu.py::test_chain_gu_w8_general_scales_vs_fp64 at H = 1536: each normalised element
    within its two roundings, the fp32 sum of H / 32 + 24 + n_row(H) terms, plus ONE fp32 rounding for the scaled sum, carried through the SwiGLU."""
    M, I, npart, eps = 5, 8960, 2, 1e-6
    h, nw, parts = _gu_inputs(M)
    cg, cu, sg, su = _codes(I, H, 11), _codes(I, H, 12), _general_scales(I, 13), _general_scales(I, 14)
    w8 = ops.pack_gate_up8_e4m3(cg, sg, cu, su).to('cuda')
    out, hb = torch.full((M + 1, I), SENT, dtype=BF, device='cuda'), torch.full((M + 1, H), SENT, dtype=BF, device='cuda')
    a, _ = ops.skinny_args(h, w8, M, partials=parts, n_partials=npart, norm_w=nw, h_out=hb, out=out, ldo=I, eps=eps)
    ops.launch_chain_gu_w8_k1536(a)
    hk = h64(hb[:M])
    y = hk / torch.sqrt((hk * hk).mean(-1, keepdim=True) + f32s(eps)) * h64(nw)
    Cg, Cu = cg.view(F8).to(D64), cu.view(F8).to(D64)
    g, u = (y @ Cg.t()) * sg.double(), (y @ Cu.t()) * su.double()
    g_abs, u_abs = (y.abs() @ Cg.abs().t()) * sg.double(), (y.abs() @ Cu.abs().t()) * su.double()
    n = H // 32 + 24 + _n_row(H) + 1
    e_g, e_u = ULP * g.abs() + (ULP * (1 + 2.0 ** -7) + U * n) * g_abs, ULP * u.abs() + (ULP * (1 + 2.0 ** -7) + U * n) * u_abs
    gr, ur = rbf(g), rbf(u)
    s_r = rbf(torch.nn.functional.silu(gr))
    ref = s_r * ur
    tol = ULP * ref.abs() + ur.abs() * ((_dsilu(gr).abs() + 0.5 * e_g) * e_g + ULP * s_r.abs()) + s_r.abs() * e_u + FLOOR
    got = h64(out[:M])
    assert torch.isfinite(got).all() and bool((out[M] == SENT).all())
    parity('chain_gu_w8_k1536.general_scales', ((got - ref).abs() / tol).max().item(), 1.0, note='max |got - ref| / tol')


# ------------------------------------------------------------------------------------------------ the model
LLM_MLP = ('mlp.gate_proj.weight', 'mlp.up_proj.weight', 'mlp.down_proj.weight')


def _is_llm_mlp(k):
    return k.startswith('language_model.') and k.endswith(LLM_MLP)


def _pv(seed):
    return torch.randn(1, 3, 448, 448, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope='module')
def g56(golden_dir):
    return np.load(os.path.join(golden_dir, 'g5g6_vlm.npz'))


@pytest.fixture(scope='module')
def sdq(golden_model):
    """sd with the six language_model.*.mlp.* matrices replaced by dequantize(quantize(.))"""
    from vlaser_amd import ops as o
    cfg, _, sd = golden_model
    assert sum(_is_llm_mlp(k) for k in sd) == 3 * cfg.llm.num_hidden_layers == 6
    return {k: (o.dequantize_rows_e4m3(*o.quantize_rows_e4m3(v)).to(v.dtype) if _is_llm_mlp(k) else v) for k, v in sd.items()}


@pytest.fixture(scope='module')
def pair(golden_model, sdq):
    """(the fp8 model on sd, the default model on sdq)"""
    from vlaser_amd.internvl_chat import InternVLChatModel
    cfg, _, sd = golden_model
    m = InternVLChatModel(cfg, max_seq_len=512, max_batch=8, llm_mlp_weights='fp8')
    assert m.llm_mlp_weights == 'fp8' and m.decode_group == 8 and 'mlp8' in m.decode_opts
    m.load_state_dict(sd, strict=False)          # VLA superset: action_expert.* etc. are unexpected keys for the chat model
    d = InternVLChatModel(cfg, max_seq_len=512, max_batch=8)
    assert d.llm_mlp_weights == 'bf16' and d.decode_group == 16 and 'mlp8' not in d.decode_opts
    d.load_state_dict(sdq, strict=False)
    m.img_context_token_id = d.img_context_token_id = cfg.img_context_token_id
    return m, d


def _on_chain(m):
    assert m.llm.path['mlp8'] and m.sbuf.plans and all(p.chain for p in m.sbuf.plans.values())


def _same(a, b):
    (ia, la), (ib, lb) = a, b
    assert torch.equal(ia, ib) and torch.equal(la, lb) and bool(torch.isfinite(la).all())


def test_generate_graph_decode_equals_default_on_dequantised_weights(pair, g56):
    m, d = pair
    pv, ids = _pv(0), torch.from_numpy(g56['input_ids'])
    for rep in range(2):          # 12 new tokens: the step graph is warmed, captured and replayed; the second pass replays the cached graph
        _same(m.generate(pv, ids, max_new_tokens=12, return_logits=True), d.generate(pv, ids, max_new_tokens=12, return_logits=True))
    assert any(not isinstance(g, str) for g in m._dec_graphs.values())      # a graph was really captured and replayed
    _on_chain(m)


def test_generate_eager_decode_equals_default_on_dequantised_weights(pair, g56):
    m, d = pair
    pv, ids = _pv(0), torch.from_numpy(g56['input_ids'])
    try:
        m.decode_graph = d.decode_graph = False
        _same(m.generate(pv, ids, max_new_tokens=6, return_logits=True), d.generate(pv, ids, max_new_tokens=6, return_logits=True))
    finally:
        m.decode_graph = d.decode_graph = True
    _on_chain(m)


def test_generate_ragged_batch_equals_default_on_dequantised_weights(pair, golden_dir):
    m, d = pair
    r = np.load(os.path.join(golden_dir, 'g6b_ragged.npz'))
    pv = torch.cat([_pv(int(s)) for s in r['seeds']])
    ids, am = torch.from_numpy(r['input_ids']), torch.from_numpy(r['attention_mask'])
    assert not bool(am.bool().all())          # a padded batch: the PREFIX-descriptor decode
    _same(m.generate(pv, ids, attention_mask=am, max_new_tokens=6, return_logits=True), d.generate(pv, ids, attention_mask=am, max_new_tokens=6, return_logits=True))
    _on_chain(m)


def test_generate_batches_of_8_and_10_equal_default_on_dequantised_weights(pair, g56):
    m, d = pair
    ids1 = torch.from_numpy(g56['input_ids'])
    pv, ids = torch.cat([_pv(20 + i) for i in range(10)]), ids1.repeat(10, 1)
    a = m.generate(pv[:8], ids[:8], max_new_tokens=5, return_logits=True)
    _same(a, d.generate(pv[:8], ids[:8], max_new_tokens=5, return_logits=True))
    assert not torch.equal(a[1][0], a[1][1])          # the rows differ (their images do)
    # 10 sequences: the fp8 model decodes groups of 8 + 2 (the chain kernels' row limit at hidden 1536), the default model one group
    with pytest.raises(NotImplementedError, match='<= 8 sequences'):
        m.generate(pv, ids, max_new_tokens=5, return_logits=True)
    got = m.generate(pv, ids, max_new_tokens=5)
    want = torch.cat([d.generate(pv[:8], ids[:8], max_new_tokens=5), d.generate(pv[8:], ids[8:], max_new_tokens=5)], 0)
    assert got.shape == (10, 5) and torch.equal(got, want) and torch.equal(got[:8], a[0])
    _on_chain(m)


def test_forward_equals_default_on_dequantised_weights(pair, g56):
    m, d = pair
    pv, ids = _pv(0), torch.from_numpy(g56['input_ids'])
    flags = torch.ones(1, 1, dtype=torch.long)
    lm, ld = m.forward(pv, ids, image_flags=flags).logits, d.forward(pv, ids, image_flags=flags).logits
    assert torch.equal(lm, ld) and bool(torch.isfinite(lm).all())


def test_generate_vs_cpu_oracle_on_dequantised_weights(pair, g56, golden_model, sdq):
    """Greedy ids equal to the fp32 CPU oracle's on the dequantised weights (guarded by the oracle's own top-2 margin, as test_greedy_ids_bit_exact is by the golden
    margins) and the logits within the default model's bound."""
    from oracle import vlm as ovlm
    cfg, _, sd = golden_model
    m, _ = pair
    pv, ids = _pv(0), torch.from_numpy(g56['input_ids'])
    oi, ol = ovlm.generate(sdq, cfg, pv, ids, max_new_tokens=8, return_logits=True)
    top2 = ol[0].topk(2, dim=-1).values
    margin = (top2[:, 0] - top2[:, 1]).min().item()
    print(f'[parity] oracle on the dequantised weights: ids {oi[0].tolist()}, smallest top-2 margin {margin:.3f}')
    assert margin > 0.05
    gi, gl = m.generate(pv, ids, max_new_tokens=8, return_logits=True)
    assert gi.cpu().tolist() == oi.tolist()
    parity('fp8 LLM MLP: decode logits vs oracle on the dequantised weights max|err|/max|ref|', relmax(gl, ol), TOL_LOGITS)


def test_llm_mlp8_footprint(pair, golden_model):
    m, d = pair
    cfg = golden_model[0]
    Hh, I = cfg.llm.hidden_size, cfg.llm.intermediate_size
    for lw in m.llm.layers:
        assert lw.gu8.t.dtype == torch.uint8 and lw.gu8.t.is_cuda and lw.gu8.t.numel() == 2 * I * Hh and lw.gu8.scale.is_cuda
        assert lw.down8.dtype == torch.uint8 and lw.down8.is_cuda and lw.down8.numel() == Hh * I and lw.down8_scale.is_cuda
        assert lw.sk_gu is None and lw.sk_down is None and lw.sk_down4 is None
    for lw in d.llm.layers:          # the default model still holds the bf16 packings the option replaces
        assert lw.sk_gu is not None and lw.sk_down is not None and lw.sk_down4 is not None and not hasattr(lw, 'gu8')


def test_llm_mlp8_refusals_through_the_constructor(golden_model, monkeypatch):
    from vlaser_amd import config as C
    from vlaser_amd.internvl_chat import DECODE_DEFAULT, InternVLChatModel
    cfg = golden_model[0]
    with pytest.raises(ValueError, match='llm_mlp_weights'):
        InternVLChatModel(cfg, llm_mlp_weights='int8')
    with pytest.raises(ValueError, match='Vlaser-8B'):
        InternVLChatModel(C.truncated(C.vlaser_8b(), 1, 1), llm_mlp_weights='fp8')
    monkeypatch.setenv('VLASER_DECODE_OPTS', DECODE_DEFAULT + ',mlp8')
    e = InternVLChatModel(cfg)
    assert e.llm_mlp_weights == 'fp8' and e.decode_group == 8
    monkeypatch.setenv('VLASER_DECODE_OPTS', 'qkv16,mlp8')
    with pytest.raises(ValueError, match='chain, gu16'):
        InternVLChatModel(cfg)
    monkeypatch.delenv('VLASER_DECODE_OPTS')
    e = InternVLChatModel(cfg)
    assert e.llm_mlp_weights == 'bf16' and e.decode_group == 16
