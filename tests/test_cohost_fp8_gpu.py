"""GPU: the co-hosted joint prefill of an 'mlp8' expert (e4m3 MLP weights): its gate/up and down launches of Euler step 0 ride in the prefill's launches as the W8 guest
kinds (VL_GUEST_CHAIN_GU_W8 / VL_GUEST_CHAIN_DOWN_W8), the lagged down projection by the looped W8 body (csrc/chain_down_loop.inc).  The bodies are the stand-alone W8
kernels' -- same MFMA sequence per accumulator, same reductions, the scale on the reduced sum, one rounding -- so everything here is bit-for-bit, with no tolerance:
  (1) the looped W8 kernel on its own against vlaser_chain_down_w8 and against vlaser_chain_down on the dequantised weights (random codes over all finite e4m3 values,
      power-of-two scales), M = 5 and 8, production widths (N = 768 = 256 units of 3 columns, K = 8960)
  (2) each fused pair with an mlp8 plan as guest against host, then the stand-alone guest, on every buffer of the model; the fused count tells the fused launch from the
      fallback (a host shape without a fused instantiation: 32 rows for the two GEMMs, 6 slabs for the seam)
  (3) a model of 3 LLM / expert layers: co-hosted mlp8 against un-hosted mlp8, graph and eager, lagged and seam-hosted down projection
  (4) batch 2 stays un-hosted, next to a hosted batch-1 graph of the same instance
  (5) expert_mlp_weights='fp8' with the default options co-hosts
"""
import pytest
import torch

from bounds import SENT
from test_cohost_gpu import OPTS, _call, _grad_off, _model, _obs, _pair, _same, weights      # noqa: F401  (fixtures)
from test_fp8_mlp_gpu import _codes, _pow2_scales

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
MLP8 = OPTS + ',mlp8'
LAG8 = OPTS + ',cohost=qkv+attn+o+gu+down_next,mlp8'
SEAM8 = OPTS + ',cohost=qkv+attn+o+gu+down,mlp8'
N, K = 768, 8960


# ------------------------------------------------------------------------------------------------ (1) the looped W8 kernel
@pytest.fixture(scope='module')
def down_case():
    """Codes, scales and both packings of one down projection at the production widths; the activations and the residual for up to 8 rows.  Computed once, never written."""
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vlaser_amd import ops
    c, s = _codes(N, K, 101), _pow2_scales(N, 102)
    g = torch.Generator().manual_seed(103)
    x = (torch.randn(8, K, generator=g) * 0.7).to(BF).cuda()
    res = (torch.randn(8, N, generator=g) * 1.5).to(BF).cuda()
    return dict(x=x, res=res, p8=ops.pack_down4_e4m3(c).cuda(), s4=ops.pack_down4_scales(s).cuda(), w4=ops.pack_down4(ops.dequantize_rows_e4m3(c, s).cuda()))


def _out(rows=9):
    flat = torch.full((rows * N + 8,), SENT, dtype=BF, device='cuda')          # (8 sentinels behind the last row: a store past the end shows)
    return flat, flat[:rows * N].view(rows, N)


@pytest.mark.parametrize('M', [5, 8])          # both ends of the two-row-group shape the guest is built for
def test_looped_w8_equals_chain_down_w8_equals_bf16_on_dequantised_weights(down_case, M):
    from vlaser_amd import ops
    d = down_case
    snap = {k: v.clone() for k, v in d.items()}
    runs = {'looped_w8': lambda o: ops.chain_down_looped_w8(d['x'], d['p8'], d['s4'], d['res'], o, M, N, K),
            'chain_down_w8': lambda o: ops.chain_down_w8(d['x'], d['p8'], d['s4'], d['res'], o, M, N, K),
            'chain_down': lambda o: ops.chain_down(d['x'], d['w4'], d['res'], o, M, N, K)}
    got = {}
    for name, fn in runs.items():
        flat, o = _out()
        fn(o)
        torch.cuda.synchronize()
        got[name] = flat
        assert not (o[:M] == SENT).all(dim=1).any(), f'{name}: a row was never written'
        assert bool((o[M:] == SENT).all()) and bool((flat[9 * N:] == SENT).all()), f'{name}: wrote behind row {M - 1}'
        assert all(torch.equal(d[k], snap[k]) for k in d), f'{name} wrote one of its inputs'
    assert torch.equal(got['looped_w8'], got['chain_down_w8']) and torch.equal(got['looped_w8'], got['chain_down'])
    # the residual stream moved: the product is not lost in the rounding
    assert not torch.equal(got['looped_w8'][:M * N].view(M, N), d['res'][:M])


def test_looped_w8_refuses_other_shapes(down_case):
    from vlaser_amd import _lib as L, ops
    d = down_case
    flat, o = _out()
    with pytest.raises(L.VlaserHipError, match='looped'):
        ops.chain_down_looped_w8(d['x'], d['p8'], d['s4'], d['res'], o, 4, N, K)          # one row group: the stand-alone kernel's shape, not the looped one's
    torch.cuda.synchronize()
    assert bool((flat == SENT).all())


# ------------------------------------------------------------------------------------------------ (2) per pair
@pytest.fixture(scope='module')
def staged8(weights):
    """An mlp8 model whose buffers hold the values of a real chunk (one eager call on the un-hosted schedule), and a snapshot of all of them."""
    m = _model(weights, MLP8, use_graph=False)
    assert m.expert_mlp_weights == 'fp8' and not m._cohost_ok(1)
    ids, pv, pro, noise = _obs(weights[0], 5)
    m.infer_action(ids, pv, proprios=pro, noise=noise).cpu()
    bufs = {'h_vlm': m.h_vlm, 'h5': m.h5, 'cache.k': m.cache.k, 'cache.vt': m.cache.vt, 'valid_len': m.valid_len}
    bufs.update({'pbuf.' + k: getattr(m.pbuf, k) for k in ('x', 'q', 'ao', 'act', 'part')})
    bufs.update({'sb.' + k: getattr(m.sb_pro, k) for k in ('hA', 'hB', 'hC', 'q', 'ao', 'act', 'part_o', 'part_d')})
    bufs.update({f'sb.chain_parts{i}': t for i, t in enumerate(m.sb_pro.chain_parts)})
    return m, bufs, {k: v.clone() for k, v in bufs.items()}


def _hosts(m, which, fallback):
    """The host launch of pair `which` as fn(guest=None), and the prefill rows it covers: the launch prefill_layer issues for VLM layer 0 (T = 384 rows), on the model's
    own buffers -- or, fallback, a shape of that host without a fused instantiation: 32 rows for the two GEMMs (the register-staged tile), 6 of the 7 slabs for the seam."""
    from vlaser_amd import _lib as L, ops
    lw, llm = m.vlm.layers[0], m.cfg.base.llm
    T = m.max_image_text_tokens
    rows = 32 if fallback and which != 'down' else T
    return _host_fn(m, which, rows, lw, llm, L, ops, 6 if fallback else 7), rows


def _host_fn(m, which, rows, lw, llm, L, ops, slabs):
    if which == 'gu':            # gate/up GEMM + the expert's gate/up
        return lambda guest=None: ops.gemm(L.EPI_SWIGLU, m.pbuf.x[:rows], lw.wgu, out=m.pbuf.act[:rows], guest=guest)
    if which == 'down_next':     # q/k/v GEMM (the same launch as layer l + 1's: shape and buffers) + the expert's down projection, looped
        return lambda guest=None: ops.gemm(L.EPI_QKV_ROPE, m.pbuf.x[:rows], lw.wqkv, bias=lw.bqkv, q_out=m.pbuf.q[:rows], k_cache=m.cache.k[0], vt_cache=m.cache.vt[0],
                                           rope_cos=m.rope[0], rope_sin=m.rope[1], pos_ids=m.pos_vlm, n_q_heads=m.vlm.nq, n_kv_heads=m.vlm.nkv, s_max=m.cache.s_max,
                                           tok_per_batch=rows, slot_base=0, guest=guest)
    assert which == 'down'       # the 7-slab seam + the expert's down projection
    assert ops.gemm_splits(rows, llm.hidden_size, llm.intermediate_size, m.pbuf.part.numel()) == 7          # what the model's own seam reduces
    return lambda guest=None: ops.reduce_norm(m.h_vlm[:rows], m.pbuf.part, slabs, rows, llm.hidden_size, m.h_vlm[:rows], m.pbuf.x[:rows], norm=1,
                                              norm_w=m.vlm.layers[1].ln_in, eps=llm.rms_norm_eps, guest=guest)


OWNED = {'gu': {'pbuf.act': True, 'sb.act': True, 'sb.hB': True},
         'down_next': {'pbuf.q': True, 'sb.hC': True, 'cache.k': False, 'cache.vt': False},
         'down': {'h_vlm': False, 'pbuf.x': True, 'sb.hC': True}}


def _run8(staged8, which, fallback, cohosted):
    from vlaser_amd import _lib as L
    from vlaser_amd.engine import plan_guest
    m, bufs, snap = staged8
    name = 'gu' if which == 'gu' else 'down'
    _, plan, _ = _pair(m, name)
    host, rows = _hosts(m, which, fallback)
    for k, t in bufs.items():
        t.copy_(snap[k])
    m.valid_len.fill_(277)
    for k, pure in OWNED[which].items():
        if pure:
            bufs[k].fill_(SENT)
    before = {k: v.clone() for k, v in bufs.items()}
    if cohosted:
        g = plan_guest(plan, name)
        assert g.kind == {'gu': L.GUEST_CHAIN_GU_W8, 'down': L.GUEST_CHAIN_DOWN_W8}[name]
        host(guest=g)
    else:
        host()
        _, launch, args = next(l for l in plan.launches if l[0] == name)
        launch(*args, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return before, {k: v.clone() for k, v in bufs.items()}, rows


@pytest.mark.parametrize('fallback', [False, True], ids=['production', 'fallback'])
@pytest.mark.parametrize('which', ['gu', 'down_next', 'down'])
def test_w8_pair_equals_host_then_guest(staged8, which, fallback):
    from vlaser_amd import _lib as L
    owned = OWNED[which]
    n0 = L.lib().vlaser_cohost_fused_count()
    before, seq, rows = _run8(staged8, which, fallback, cohosted=False)
    assert L.lib().vlaser_cohost_fused_count() == n0
    before2, co, _ = _run8(staged8, which, fallback, cohosted=True)
    # at the production shape the guest rode in the host's launch; the host-then-guest fallback returns the same 0 and the same bits
    assert L.lib().vlaser_cohost_fused_count() == n0 + (0 if fallback else 1)
    assert all(_same(before[k], before2[k]) for k in before)
    for k in seq:
        assert _same(co[k], seq[k]), f'{which}: {k} differs between the co-hosted launch and host-then-guest'
        if k not in owned:
            assert _same(co[k], before[k]), f'{which}: {k} is not the pair\'s and was written'
    # both sides wrote: no pure output kept its sentinel in the rows the launches cover
    guest_out = {'gu': ('sb.act', 'sb.hB'), 'down_next': ('sb.hC',), 'down': ('sb.hC',)}[which]
    host_out = {'gu': 'pbuf.act', 'down_next': 'pbuf.q', 'down': 'pbuf.x'}[which]
    for k in guest_out:
        assert not _same(co[k][:5], before[k][:5]), f'{which}: {k} was never written'
        assert _same(co[k][5:], before[k][5:]), f'{which}: {k} was written behind the guest\'s 5 rows'
    assert not (co[host_out][:rows] == SENT).all(dim=-1).any() and _same(co[host_out][rows:], before[host_out][rows:])


# ------------------------------------------------------------------------------------------------ (3) whole model
@pytest.fixture(scope='module')
def unhosted(weights):
    """What the un-hosted mlp8 model returns for the two observations of the lag test (eager and graph give the same bits: checked where it is used)."""
    cfg = weights[0]
    out = {}
    for use_graph in (True, False):
        b = _model(weights, MLP8, use_graph)
        assert not b._cohost_ok(1) and b.expert_mlp_weights == 'fp8'
        out[use_graph] = [_call(b, cfg, _obs(cfg, seed, n_text), False) for seed, n_text in ((31, 11), (32, 118))]
        del b
    return out


@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('opts', [LAG8, SEAM8], ids=['down_next', 'down'])
def test_model_mlp8_cohost_equals_unhosted(weights, unhosted, opts, use_graph):
    from vlaser_amd import _lib as L
    cfg = weights[0]
    a = _model(weights, opts, use_graph)
    assert a._cohost_ok(1) and a.expert_mlp_weights == 'fp8'
    assert a.cohost_lagged == (('down',) if opts is LAG8 else ()) and a.cohost_pairs == (('qkv', 'attn', 'o', 'gu') if opts is LAG8 else ('qkv', 'attn', 'o', 'gu', 'down'))
    for i, (seed, n_text) in enumerate(((31, 11), (32, 118))):          # the second call of a graph model is a replay; 118 text tokens: valid_len = 384, no padding
        n0 = L.lib().vlaser_cohost_fused_count()
        ra = _call(a, cfg, _obs(cfg, seed, n_text), False)
        if not use_graph:      # 3 layers: the two hosted layers carry four pairs each + two down projections (lagged: in the q/k/v GEMMs of layers 1 and 2; else: in the two seams)
            assert L.lib().vlaser_cohost_fused_count() == n0 + 10
        assert torch.isfinite(ra[0]).all()
        for what, x, y in zip(('chunk', 'velocities', 'K slots T..T+4', 'V^T slots T..T+4'), ra, unhosted[use_graph][i]):
            assert _same(x, y), f'{what} differs (seed {seed})'


# ------------------------------------------------------------------------------------------------ (4) batch 2 next to a hosted batch-1 graph
def test_batch2_stays_unhosted_next_to_a_hosted_batch1_graph(weights):
    from vlaser_amd import _lib as L
    from vlaser_amd.pizero import PiZeroInference
    cfg = weights[0]

    def model(opts):
        m = PiZeroInference(weights[1], max_batch=2, use_graph=True, euler_opts=opts)
        m.load_state_dict(weights[2])
        return m
    a, b = model(LAG8), model(MLP8)
    assert a._cohost_ok(1) and not a._cohost_ok(2) and not b._cohost_ok(1) and not b._cohost_ok(2)
    one = _obs(cfg, 41)
    two = tuple(torch.cat([x, y]) for x, y in zip(_obs(cfg, 42), _obs(cfg, 43, 118)))
    for obs in (one, two, one):          # batch 1 (hosted in a), batch 2 (un-hosted in both), batch 1 again: a replay of the hosted graph
        ids, pv, pro, noise = obs
        B = ids.shape[0]
        vl = (ids != cfg.pad_token_id).sum(-1)
        ra, rb = a.infer_action(ids, pv, proprios=pro, noise=noise, valid_len=vl).cpu(), b.infer_action(ids, pv, proprios=pro, noise=noise, valid_len=vl).cpu()
        assert torch.isfinite(ra).all() and _same(ra, rb), f'batch {B}'
        assert _same(a.last_velocities(B), b.last_velocities(B)), f'batch {B}'
    assert L.lib().vlaser_cohost_fused_count() > 0


# ------------------------------------------------------------------------------------------------ (5) the public switch
def test_expert_mlp_weights_fp8_cohosts_by_default(weights, monkeypatch):
    from vlaser_amd import _lib as L
    from vlaser_amd.pizero import PiZeroInference
    monkeypatch.delenv('VLASER_EULER', raising=False)
    m = PiZeroInference(weights[1], use_graph=False, expert_mlp_weights='fp8')
    m.load_state_dict(weights[2])
    assert m.expert_mlp_weights == 'fp8' and m._cohost_ok(1)
    # the default pair set of an mlp8 model: the default's, minus what the per-pair A/B switched off under mlp8 (profiles/cohost_fp8_ab.md); the bf16 default did not move
    from vlaser_amd.pizero import COHOST_MLP8_DEFAULT_OFF
    d = PiZeroInference(weights[1], use_graph=False)
    assert d.cohost_pairs == ('qkv', 'attn', 'o', 'gu') and d.cohost_lagged == ('down',) and d.expert_mlp_weights == 'bf16'
    assert m.cohost_pairs == tuple(x for x in d.cohost_pairs if x not in COHOST_MLP8_DEFAULT_OFF) and m.cohost_lagged == d.cohost_lagged
    assert PiZeroInference(weights[1], euler_opts=PiZeroInference.EULER_DEFAULT, expert_mlp_weights='fp8').cohost_pairs == d.cohost_pairs          # named pairs are honoured
    ids, pv, pro, noise = _obs(weights[0], 51)
    n0 = L.lib().vlaser_cohost_fused_count()
    act = m.infer_action(ids, pv, proprios=pro, noise=noise).cpu()
    assert torch.isfinite(act).all() and L.lib().vlaser_cohost_fused_count() > n0
