"""GPU: the lagged pair of the co-hosted joint prefill (Euler option 'cohost=...+down_next'): the expert's down projection of layer l as the guest of the q/k/v GEMM of VLM
layer l + 1, run there by the LOOPED body (csrc/chain_down_loop.inc: four of vlaser_chain_down's workgroups to one).  The looped body keeps every accumulator's MFMA
sequence, both reductions and the single rounding of the stand-alone kernel, and a co-hosted launch computes what `host; guest` compute: everything here is bit-for-bit.
  (a) the looped kernel on its own against vlaser_chain_down on the same inputs, M = 5, production widths (N = 768 = 256 units of 3 columns, K = 8960)
  (b) the q/k/v GEMM with its guest against the GEMM, then the stand-alone down projection, on every buffer of the model; the fused count tells the fused launch
      (production shape: 6 x 32 tiles of 64 x 64) from the fallback (32 rows: the register-staged tile, no fused instantiation)
  (c) a model of 3 LLM / expert layers (two lagged guests, the un-hosted last layer): 'cohost=qkv+attn+o+gu+down_next' against the un-hosted options, graph and eager
  (d) 'down' and 'down_next' together are refused
"""
import pytest
import torch

from bounds import SENT
from test_cohost_gpu import OPTS, _call, _grad_off, _model, _obs, _pair, _same, staged, weights      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
LAG = OPTS + ',cohost=qkv+attn+o+gu+down_next'


def _down_operands(m):
    llm = m.cfg.expert
    return m.sb_pro.act, m.expert.layers[0].sk_down4, m.sb_pro.hB, m.sb_pro.hC, m.num_action_tokens + 1, llm.hidden_size, llm.intermediate_size


def test_looped_kernel_equals_chain_down(staged):
    from vlaser_amd import ops
    m, bufs, snap = staged
    act, W4, res, out, M, H, I = _down_operands(m)
    assert (M, H, I) == (5, 768, 8960)
    got = {}
    for name, fn in (('chain_down', ops.chain_down), ('looped', ops.chain_down_looped)):
        for k, t in bufs.items():
            t.copy_(snap[k])
        out.fill_(SENT)
        before = {k: v.clone() for k, v in bufs.items()}
        fn(act, W4, res, out, M, H, I)
        torch.cuda.synchronize()
        got[name] = {k: v.clone() for k, v in bufs.items()}
        assert all(_same(got[name][k], before[k]) for k in bufs if k != 'sb.hC'), f'{name} wrote a buffer that is not its output'
        assert not (got[name]['sb.hC'][:M] == SENT).any() and _same(got[name]['sb.hC'][M:], before['sb.hC'][M:])
    assert _same(got['looped']['sb.hC'], got['chain_down']['sb.hC'])
    # the residual stream moved: the product is not lost in the rounding
    assert not _same(got['looped']['sb.hC'][:M], snap['sb.hB'][:M])


def test_looped_kernel_refuses_other_shapes(staged):
    from vlaser_amd import _lib as L, ops
    m = staged[0]
    act, W4, res, out, M, H, I = _down_operands(m)
    with pytest.raises(L.VlaserHipError, match='looped'):
        ops.chain_down_looped(act, W4, res, out, 4, H, I)          # one row group: the stand-alone kernel's shape, not the looped one's


def _run_qkv(staged, rows, cohosted):
    """The q/k/v GEMM of layer 0 over `rows` rows (the same launch as layer l + 1's: shape and buffers) with the expert's down projection of layer 0 as its guest."""
    from vlaser_amd import _lib as L, ops
    from vlaser_amd.engine import plan_guest
    m, bufs, snap = staged
    _, plan, _ = _pair(m, 'down')
    for k, t in bufs.items():
        t.copy_(snap[k])
    for k in ('pbuf.q', 'sb.hC'):
        bufs[k].fill_(SENT)
    before = {k: v.clone() for k, v in bufs.items()}
    lw = m.vlm.layers[0]
    guest = plan_guest(plan, 'down') if cohosted else None
    ops.gemm(L.EPI_QKV_ROPE, m.pbuf.x[:rows], lw.wqkv, bias=lw.bqkv, q_out=m.pbuf.q[:rows], k_cache=m.cache.k[0], vt_cache=m.cache.vt[0], rope_cos=m.rope[0],
             rope_sin=m.rope[1], pos_ids=m.pos_vlm, n_q_heads=m.vlm.nq, n_kv_heads=m.vlm.nkv, s_max=m.cache.s_max, tok_per_batch=rows, slot_base=0, guest=guest)
    if not cohosted:
        _, launch, args = next(l for l in plan.launches if l[0] == 'down')
        launch(*args, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return before, {k: v.clone() for k, v in bufs.items()}


@pytest.mark.parametrize('rows,fused', [(384, 1), (32, 0)], ids=['production-64x64', 'fallback-32-rows'])
def test_qkv_gemm_with_guest_equals_gemm_then_down(staged, rows, fused):
    from vlaser_amd import _lib as L
    n0 = L.lib().vlaser_cohost_fused_count()
    before, seq = _run_qkv(staged, rows, cohosted=False)
    assert L.lib().vlaser_cohost_fused_count() == n0
    before2, co = _run_qkv(staged, rows, cohosted=True)
    assert L.lib().vlaser_cohost_fused_count() == n0 + fused
    assert all(_same(before[k], before2[k]) for k in before)
    owned = ('pbuf.q', 'sb.hC', 'cache.k', 'cache.vt')
    for k in seq:
        assert _same(co[k], seq[k]), f'{k} differs between the co-hosted launch and host-then-guest'
        if k not in owned:
            assert _same(co[k], before[k]), f'{k} is not the pair\'s and was written'
    assert not (co['pbuf.q'][:rows] == SENT).any() and not (co['sb.hC'][:5] == SENT).any()
    # the host writes cache slots < rows of its layer only
    T = staged[0].max_image_text_tokens
    assert _same(co['cache.k'][0, :, :, T:], before['cache.k'][0, :, :, T:]) and _same(co['cache.k'][1:], before['cache.k'][1:])
    assert _same(co['cache.vt'][0, :, :, :, T:], before['cache.vt'][0, :, :, :, T:]) and _same(co['cache.vt'][1:], before['cache.vt'][1:])


@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
def test_model_down_next_equals_unhosted(weights, use_graph):
    from vlaser_amd import _lib as L
    cfg = weights[0]
    a, b = _model(weights, LAG, use_graph), _model(weights, OPTS, use_graph)
    assert a.cohost_pairs == ('qkv', 'attn', 'o', 'gu') and a.cohost_lagged == ('down',) and a._cohost_ok(1) and not b._cohost_ok(1)
    for seed, n_text in ((31, 11), (32, 118)):          # the second call of a graph model is a replay; 118 text tokens: valid_len = 384, no padding
        obs = _obs(cfg, seed, n_text)
        n0 = L.lib().vlaser_cohost_fused_count()
        ra = _call(a, cfg, obs, False)
        if not use_graph:      # 3 layers: four pairs in each of the two hosted layers, d(0) in the q/k/v GEMM of layer 1, d(1) in that of layer 2
            assert L.lib().vlaser_cohost_fused_count() == n0 + 10
        rb = _call(b, cfg, obs, False)
        assert torch.isfinite(ra[0]).all()
        for what, x, y in zip(('chunk', 'velocities', 'K slots T..T+4', 'V^T slots T..T+4'), ra, rb):
            assert _same(x, y), f'{what} differs (seed {seed})'


def test_down_next_alone_equals_unhosted(weights):
    cfg = weights[0]
    a, b = _model(weights, OPTS + ',cohost=down_next', False), _model(weights, OPTS, False)
    assert a.cohost_pairs == () and a.cohost_lagged == ('down',) and a._cohost_ok(1)
    obs = _obs(cfg, 33)
    for x, y in zip(_call(a, cfg, obs, False), _call(b, cfg, obs, False)):
        assert _same(x, y)


def test_down_and_down_next_are_exclusive(weights):
    from vlaser_amd.pizero import PiZeroInference
    with pytest.raises(ValueError, match='down_next'):
        PiZeroInference(weights[1], euler_opts=OPTS + ',cohost=qkv+attn+o+gu+down+down_next')
    with pytest.raises(ValueError, match='unknown pair'):
        PiZeroInference(weights[1], euler_opts=OPTS + ',cohost=qkv+down_later')
