"""GPU: the co-hosted launches of the joint prefill (Euler option 'cohost'; csrc/chain_kernels.h).  A co-hosted launch must compute exactly what `host; guest`
compute -- the bodies and their summation orders are the stand-alone kernels' -- so everything here is bit-for-bit, with no tolerance:
  per pair    one host launch + one guest launch at the production widths (B = 1, T = 384, 5 expert rows), every pure output pre-filled with a sentinel: the co-hosted
              launch against host-then-guest on EVERY buffer of the model (what the pair owns: equal; what it does not own: untouched)
  fallback    a host shape without a fused instantiation (a 64-row GEMM) + a guest: success and the same bits
  model       a model of 2 ViT + 3 LLM / expert layers at full widths (hosted layers, the un-hosted last layer, the hand-over): infer_action with 'cohost' against
              without it on the chunk, the velocities of every Euler step and the expert's K / V^T cache slots T .. T + 4 of every layer; graph and eager, the
              reference's eight-tensor call and valid_len=
"""
import pytest
import torch

from bounds import SENT

pytestmark = pytest.mark.gpu
OPTS = 'qkv16,gu16,glue1,chain'
PAIRS = ['qkv', 'attn', 'o', 'gu', 'down']


@pytest.fixture(autouse=True)
def _grad_off():
    with torch.no_grad():
        yield


def _obs(cfg, seed, n_text=11):
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((1, 384), cfg.pad_token_id)
    ids[:, :10] = torch.randint(0, 151643, (1, 10), generator=g)
    ids[:, 10:266] = cfg.img_context_token_id
    ids[:, 266:266 + n_text] = torch.randint(0, 151643, (1, n_text), generator=g)
    return ids, torch.randn(1, 3, 448, 448, generator=g), torch.rand(1, 1, 7, generator=g) * 2 - 1, torch.randn(1, 4, 7, generator=g)


@pytest.fixture(scope='module')
def weights():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vlaser_amd import config as C, synth
    cfg = C.truncated(C.vlaser_2b(), 2, 3)
    vla = C.VLAConfig(base=cfg)
    return cfg, vla, synth.vla_state_dict(vla)


def _model(weights, opts, use_graph):
    from vlaser_amd.pizero import PiZeroInference
    m = PiZeroInference(weights[1], max_batch=1, use_graph=use_graph, euler_opts=opts)
    m.load_state_dict(weights[2])
    return m


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ per pair
@pytest.fixture(scope='module')
def staged(weights):
    """A model whose buffers hold the values of a real chunk (one eager call on today's schedule), and a snapshot of all of them."""
    m = _model(weights, OPTS, use_graph=False)
    ids, pv, pro, noise = _obs(weights[0], 5)
    m.infer_action(ids, pv, proprios=pro, noise=noise).cpu()
    bufs = {'h_vlm': m.h_vlm, 'h5': m.h5, 'cache.k': m.cache.k, 'cache.vt': m.cache.vt, 'valid_len': m.valid_len}
    bufs.update({'pbuf.' + k: getattr(m.pbuf, k) for k in ('x', 'q', 'ao', 'act', 'part')})
    bufs.update({'sb.' + k: getattr(m.sb_pro, k) for k in ('hA', 'hB', 'hC', 'q', 'ao', 'act', 'part_o', 'part_d')})
    bufs.update({f'sb.chain_parts{i}': t for i, t in enumerate(m.sb_pro.chain_parts)})
    return m, bufs, {k: v.clone() for k, v in bufs.items()}


def _pair(m, name):
    """(host launch, expert plan) of layer 0 for the pair whose GUEST is `name`, and the buffers host and guest write: {buffer: True if it is a pure output}."""
    from vlaser_amd import _lib as L
    from vlaser_amd.engine import prefill_layer_launches, skinny_layer_plan
    from vlaser_amd.pizero import COHOST_PAIRS
    T, na = m.max_image_text_tokens, m.num_action_tokens
    hosts = dict(prefill_layer_launches(m.vlm, m.vlm.layers[0], m.pbuf, m.h_vlm[:T], m.cache, 0, m.rope, m.pos_vlm, 1, T, L.ATTN_PREFIX, valid_len=m.valid_len,
                                        blk_start=T, next_norm_w=m.vlm.layers[1].ln_in))
    plan = skinny_layer_plan(m.expert, m.expert.layers[0], m.sb_pro, m.h5, None, 0, m.cache, 0, m.rope, m.pos5, 1, na + 1, T, T + 1 + na, L.ATTN_PREFIX,
                             valid_len=m.valid_len, blk_start=T, first_tok_kv_len=T + 1)
    assert plan.chain and plan.chain_ao and [n for n, _, _ in plan.launches] == PAIRS
    owned = {'qkv': {'pbuf.ao': True, 'sb.q': True, 'cache.k': False, 'cache.vt': False},
             'attn': {'pbuf.part': True, 'sb.chain_parts0': True, 'sb.chain_parts1': True},
             'o': {'h_vlm': False, 'pbuf.x': True, 'sb.part_o': True},
             'gu': {'pbuf.act': True, 'sb.act': True, 'sb.hB': True},
             'down': {'h_vlm': False, 'pbuf.x': True, 'sb.hC': True}}[name]
    return hosts[COHOST_PAIRS[name]], plan, owned


def _run_pair(staged, name, valid_len, cohosted):
    from vlaser_amd.engine import plan_guest
    m, bufs, snap = staged
    T = m.max_image_text_tokens
    host, plan, owned = _pair(m, name)
    for k, t in bufs.items():
        t.copy_(snap[k])
    m.valid_len.fill_(valid_len)
    for k, pure in owned.items():
        if pure:
            bufs[k].fill_(SENT)
    if name == 'qkv':          # the slots the guest writes (and everything behind them) of layer 0: the host reads slots < T only
        m.cache.k[0, :, :, T:].fill_(SENT)
        m.cache.vt[0, :, :, :, T:].fill_(SENT)
    before = {k: v.clone() for k, v in bufs.items()}
    if cohosted:
        host(guest=plan_guest(plan, name))
    else:
        host()
        _, launch, args = next(l for l in plan.launches if l[0] == name)
        launch(*args, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return before, {k: v.clone() for k, v in bufs.items()}, owned


@pytest.mark.parametrize('name,valid_len', [('qkv', 1), ('qkv', 277), ('qkv', 384), ('attn', 1), ('attn', 277), ('attn', 384), ('o', 277), ('gu', 277), ('down', 277)])
def test_pair_equals_host_then_guest(staged, name, valid_len):
    from vlaser_amd import _lib as L
    n0 = L.lib().vlaser_cohost_fused_count()
    before, seq, owned = _run_pair(staged, name, valid_len, cohosted=False)
    assert L.lib().vlaser_cohost_fused_count() == n0
    before2, co, _ = _run_pair(staged, name, valid_len, cohosted=True)
    # at the production shapes the guest rode in the host's launch: the host-then-guest fallback returns the same 0 and the same bits
    assert L.lib().vlaser_cohost_fused_count() == n0 + 1, f'{name}: the co-hosted entry fell back to host-then-guest at the production shape'
    assert all(_same(before[k], before2[k]) for k in before)
    for k in seq:
        assert _same(co[k], seq[k]), f'{name}: {k} differs between the co-hosted launch and host-then-guest'
        if k not in owned:
            assert _same(co[k], before[k]), f'{name}: {k} is not the pair\'s and was written'
    # the pair did write: every pure output lost its sentinel somewhere, in both forms
    for k, pure in owned.items():
        if pure:
            assert not _same(seq[k], before[k]), f'{name}: {k} was never written'


def test_fallback_host_without_a_fused_instantiation(staged):
    """A 64-row gate/up GEMM takes another tile than the joint prefill's: vlaser_gemm_cohost launches host, then guest, and says so with success."""
    from vlaser_amd import _lib as L, ops
    from vlaser_amd.engine import plan_guest
    m, bufs, snap = staged
    _, plan, owned = _pair(m, 'gu')
    outs = []
    for cohosted in (False, True):
        for k, t in bufs.items():
            t.copy_(snap[k])
        for k in owned:
            bufs[k].fill_(SENT)
        x, act = m.pbuf.x[:64], m.pbuf.act[:64]
        if cohosted:
            n0 = L.lib().vlaser_cohost_fused_count()
            ops.gemm(L.EPI_SWIGLU, x, m.vlm.layers[0].wgu, out=act, guest=plan_guest(plan, 'gu'))
            assert L.lib().vlaser_cohost_fused_count() == n0          # no fused instantiation for this tile
        else:
            ops.gemm(L.EPI_SWIGLU, x, m.vlm.layers[0].wgu, out=act)
            ops.launch_chain_gu(plan.gu[0])
        torch.cuda.synchronize()
        outs.append({k: v.clone() for k, v in bufs.items()})
    assert all(_same(outs[0][k], outs[1][k]) for k in bufs)
    assert not _same(outs[1]['pbuf.act'][:64], torch.full_like(outs[1]['pbuf.act'][:64], SENT)) and _same(outs[1]['pbuf.act'][64:], torch.full_like(outs[1]['pbuf.act'][64:], SENT))


# ------------------------------------------------------------------------------------------------ whole model
def _call(m, cfg, obs, dense):
    ids, pv, pro, noise = obs
    if dense:
        mask, vp, pp, ap = m.build_causal_mask_and_position_ids((ids != cfg.pad_token_id).long(), torch.float32)
        m1, m2 = m.split_full_mask_into_submasks(mask)
        act = m.infer_action(ids, pv, m1, m2, vp, pp, ap, pro, noise=noise)
    else:
        act = m.infer_action(ids, pv, proprios=pro, noise=noise, valid_len=(ids != cfg.pad_token_id).sum(-1))
    T = m.max_image_text_tokens
    act = act.cpu()
    return act, m.last_velocities().cpu(), m.cache.k[:, :, :, T:T + 5].cpu(), m.cache.vt[:, :, :, :, T:T + 5].cpu()


@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
def test_model_cohost_equals_default(weights, use_graph):
    cfg = weights[0]
    a, b = _model(weights, OPTS + ',cohost', use_graph), _model(weights, OPTS, use_graph)
    assert a._cohost_ok(1) and not b._cohost_ok(1)
    for dense in (True, False):
        for seed, n_text in ((11, 11), (12, 118)):          # the second call of a graph model is a replay; 118 text tokens: valid_len = 384, no padding
            obs = _obs(cfg, seed, n_text)
            ra, rb = _call(a, cfg, obs, dense), _call(b, cfg, obs, dense)
            assert torch.isfinite(ra[0]).all()
            for what, x, y in zip(('chunk', 'velocities', 'K slots T..T+4', 'V^T slots T..T+4'), ra, rb):
                assert _same(x, y), f'{what} differs (dense masks {dense}, seed {seed})'


def test_model_subset_of_pairs_equals_default(weights):
    """Pairs switched off run their guests as launches of their own behind their hosts: the same bits again."""
    cfg = weights[0]
    a, b = _model(weights, OPTS + ',cohost=qkv+gu', False), _model(weights, OPTS, False)
    assert a.cohost_pairs == ('qkv', 'gu')
    obs = _obs(cfg, 21)
    for x, y in zip(_call(a, cfg, obs, False), _call(b, cfg, obs, False)):
        assert _same(x, y)


def test_option_needs_the_chain_path(weights):
    from vlaser_amd.pizero import PiZeroInference
    with pytest.raises(ValueError, match='needs'):
        PiZeroInference(weights[1], euler_opts='qkv16,gu16,chain,cohost')
    with pytest.raises(ValueError, match='unknown pair'):
        PiZeroInference(weights[1], euler_opts=OPTS + ',cohost=qkv+up')
