"""`VLATrainer(batch_rows=True)` on the GPU: the two batched kernels bit for bit against their per-sample forms, the batched pass against the
oracle's autograd on the same [2, ...] batch and against the sequential step, B = 1 bit-identical to the one-sample pass, groups, refusals.
Bounds: those of tests/test_vla_train_gpu.py against the oracle (loss 1e-2, rel 4e-2, cos 0.999); batched against sequential twice that
(both sit within 4e-2 of the oracle) -- the bounds of tests/test_sft_batch_rows_gpu.py."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bounds import BF, SENT, bits, sentinel
from parity import parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vlaser_amd import ops as o
    return o


def rnd(*shape, std=1.0, seed=0, dtype=BF):
    g = torch.Generator(device='cpu').manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * std).to(dtype).cuda()


# ------------------------------------------------------------------------------------------------ 1. attention backward of B samples' rows in one call
@pytest.mark.parametrize('first_tok_self', [True, False])
@pytest.mark.parametrize('geom', [(64, 128, (64, 1, 37)), (384, 448, (277, 300, 384))])
@pytest.mark.parametrize('R', [5, 2])
@pytest.mark.parametrize('heads', [(12, 2), (4, 2)])
def test_attn_rows_bwd_batched_is_the_per_sample_kernel(ops, heads, R, geom, first_tok_self):
    """Full prefix, a single key, ragged counts that are no multiple of the 256-thread stride; the cache is [B + 1, ...] and slices 1..B are used, so a
    wrong batch stride reads another sample; rows >= B*R of the outputs keep the sentinel."""
    (n_q, n_kv), (blk_start, s_max, vls), B = heads, geom, 3
    scale = 1.0 / math.sqrt(128)
    seed = 100 * n_q + 10 * R + blk_start
    q, dO, O = rnd(B * R, n_q * 128, seed=seed), rnd(B * R, n_q * 128, seed=seed + 1), rnd(B * R, n_q * 128, std=0.5, seed=seed + 2)
    K, VT = rnd(B + 1, n_kv, s_max, 128, seed=seed + 3), rnd(B + 1, n_kv, 128, s_max, seed=seed + 4)
    vl = torch.tensor(vls, dtype=torch.int32).cuda()
    runs = []
    for _ in range(2):
        dq, dk, dv = sentinel(B * R + 3, n_q * 128), sentinel(B * R + 3, n_kv * 128), sentinel(B * R + 3, n_kv * 128)
        ops.attn_rows_bwd_batched(q, K[1:], VT[1:], dO, O, dq, dk, dv, B, R, n_q, n_kv, s_max, vl, blk_start, first_tok_self, scale)
        runs.append((dq, dk, dv))
    for a, b in zip(*runs):
        assert torch.equal(bits(a), bits(b)), 'two runs differ'
    dq, dk, dv = runs[0]
    for t in (dq, dk, dv):
        assert bool((t[B * R:] == SENT).all()), 'rows behind the B*R outputs written'
        assert bool(torch.isfinite(t[:B * R].float()).all())
    for b in range(B):
        rows = slice(b * R, (b + 1) * R)
        rq, rk, rv = sentinel(R, n_q * 128), sentinel(R, n_kv * 128), sentinel(R, n_kv * 128)
        ops.attn_rows_bwd(q[rows], K[1 + b], VT[1 + b], dO[rows], O[rows], rq, rk, rv, R, n_q, n_kv, s_max, vls[b], blk_start, first_tok_self, scale)
        for name, got, ref in (('dq', dq, rq), ('dk', dk, rk), ('dv', dv, rv)):
            assert torch.equal(bits(got[rows]), bits(ref)), f'{name} of sample {b} differs from vlaser_attn_rows_bwd'


def test_attn_rows_bwd_batched_clamps_valid_len_and_checks_arguments(ops):
    """valid_len beyond blk_start is clamped in the kernel (== blk_start); bad geometry is an error, not a launch."""
    from vlaser_amd import _lib as L
    B, R, n_q, n_kv, blk_start, s_max, scale = 2, 5, 4, 2, 64, 128, 0.1
    q, dO, O = rnd(B * R, n_q * 128, seed=1), rnd(B * R, n_q * 128, seed=2), rnd(B * R, n_q * 128, std=0.5, seed=3)
    K, VT = rnd(B, n_kv, s_max, 128, seed=4), rnd(B, n_kv, 128, s_max, seed=5)
    outs = []
    for vls in ((64, 64), (100, 9999)):
        dq, dk, dv = sentinel(B * R, n_q * 128), sentinel(B * R, n_kv * 128), sentinel(B * R, n_kv * 128)
        ops.attn_rows_bwd_batched(q, K, VT, dO, O, dq, dk, dv, B, R, n_q, n_kv, s_max, torch.tensor(vls, dtype=torch.int32).cuda(), blk_start, True, scale)
        outs.append((dq, dk, dv))
    for a, b in zip(*outs):
        assert torch.equal(bits(a), bits(b))
    vl = torch.tensor((64, 64), dtype=torch.int32).cuda()
    q, dO, O = rnd(64, n_q * 128, seed=1), rnd(64, n_q * 128, seed=2), rnd(64, n_q * 128, std=0.5, seed=3)      # rows enough for every R tried: the C check must refuse, not the wrapper
    for kw in (dict(R=17), dict(R=0), dict(blk_start=s_max - R + 1)):
        a = dict(R=R, blk_start=blk_start); a.update(kw)
        with pytest.raises(L.VlaserHipError):
            ops.attn_rows_bwd_batched(q, K, VT, dO, O, sentinel(64, n_q * 128), sentinel(64, n_kv * 128), sentinel(64, n_kv * 128), B, a['R'], n_q, n_kv, s_max, vl,
                                      a['blk_start'], True, scale, ws=torch.zeros(B * 2 * n_q * 256, device='cuda'))


# ------------------------------------------------------------------------------------------------ 2. vla_prep with one t per sample
@pytest.mark.parametrize('W', [768, 1536])
def test_vla_prep_rows_is_vla_prep_per_sample(ops, W):
    B, na, adim = 3, 4, 7
    t = torch.tensor([0.0, 0.35, 0.999], dtype=torch.float32)
    act = rnd(B * na, adim, seed=W, dtype=torch.float32)
    w1, b1 = rnd(W, adim, std=0.3, seed=W + 1), rnd(W, std=0.1, seed=W + 2)
    xcat = sentinel(B * na + 3, 2 * W)
    ops.vla_prep_rows(act, w1, b1, xcat, B * na, W, adim, t.cuda(), na, 10000.0)
    assert bool((xcat[B * na:] == SENT).all()), 'rows behind the B*na outputs written'
    for b in range(B):
        ref = sentinel(na, 2 * W)
        ops.vla_prep(act[b * na:(b + 1) * na].contiguous(), w1, b1, ref, na, W, adim, float(t[b]), 10000.0)
        assert torch.equal(bits(xcat[b * na:(b + 1) * na]), bits(ref)), f'sample {b} (t = {float(t[b])}) differs from vlaser_vla_prep'


# ------------------------------------------------------------------------------------------------ the trainer
def _case(golden_dir, case):
    d = np.load(os.path.join(golden_dir, 'g7_vla.npz'))
    f = np.load(os.path.join(golden_dir, 'g10_flow_matching.npz'))
    pv = torch.randn(1, 3, 448, 448, generator=torch.Generator().manual_seed(int(d[f'{case}_seed'])))
    smp = dict(input_ids=torch.from_numpy(d[f'{case}_input_ids']), pixel_values=pv, proprios=torch.from_numpy(d[f'{case}_proprio']),
               actions=torch.from_numpy(f[f'{case}_actions']), t=torch.from_numpy(f[f'{case}_t']), x0=torch.from_numpy(f[f'{case}_x0']))
    return smp, f


def _cat(samples):
    return {k: torch.cat([s[k] for s in samples], 0) for k in samples[0]}


@pytest.fixture(scope='module')
def samples(golden_dir):
    a, _ = _case(golden_dir, 'a')
    b, _ = _case(golden_dir, 'b')
    g = torch.Generator().manual_seed(6)
    c = dict(a, actions=torch.rand(1, 4, 7, generator=g) * 2 - 1, x0=torch.randn(1, 4, 7, generator=g), t=torch.tensor([0.6]))
    return a, b, c


def _trainer(golden_model, **kw):
    from vlaser_amd.vla_train import VLATrainer
    _, vla, sd = golden_model
    return VLATrainer(vla, **kw).load_state_dict(sd)


@pytest.fixture(scope='module')
def seq(golden_model):
    return _trainer(golden_model, lr=0.0, max_grad_norm=0.0)


@pytest.fixture(scope='module')
def bat(golden_model):
    return _trainer(golden_model, lr=0.0, max_grad_norm=0.0, batch_rows=True, max_batch=2)


def _grads(m):
    return {k: g.float().cpu().flatten() for k, g in m.named_grads().items()}


def _compare(tag, got, ref, rel_bound, cos_bound):
    assert set(got) == set(ref)
    worst_rel, worst_cos = (0.0, ''), (2.0, '')
    for k in ref:
        rel = ((got[k] - ref[k]).norm() / (ref[k].norm() + 1e-30)).item()
        cos = F.cosine_similarity(got[k], ref[k], dim=0).item()
        worst_rel, worst_cos = max(worst_rel, (rel, k)), min(worst_cos, (cos, k))
    parity(f'vla_batch_rows.{tag}.rel', worst_rel[0], rel_bound, note=f'worst per-tensor relative Frobenius error ({worst_rel[1]})')
    if cos_bound is not None:
        parity(f'vla_batch_rows.{tag}.cos', worst_cos[0], cos_bound, lower=True, note=f'worst per-tensor cosine ({worst_cos[1]})')


def test_batch_of_two_vs_oracle_autograd(bat, samples, golden_model):
    """Batch [a, b] (277 and 300 valid tokens, t = 0.35 / 0.8) against torch autograd through the fp32 oracle on the same [2, ...] tensors."""
    from oracle import vla as ovla
    _, vla, sd = golden_model
    batch = _cat(samples[:2])
    am = (batch['input_ids'] != vla.base.pad_token_id).long()
    mask, vp, pp, ap = ovla.build_causal_mask_and_position_ids(am, torch.float32, vla)
    loss = bat.forward_backward_batch(vlm_position_ids=vp, proprio_position_ids=pp, action_position_ids=ap, causal_mask=mask, **batch)
    got = _grads(bat)
    with torch.enable_grad():
        sdg = {k: (v.clone().requires_grad_(True) if k in got else v) for k, v in sd.items()}
        ref = ovla.flow_matching_loss(sdg, vla, batch['input_ids'], batch['pixel_values'], mask, vp, pp, ap, batch['proprios'], batch['actions'], batch['t'], batch['x0'])
        ref.backward()
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g10_flow_matching.npz'))
    assert set(got) == {str(n) for n in f['a_names']}                      # exactly the reference's action_expert_parameters group
    parity('vla_batch_rows.oracle.loss', abs(loss.item() - ref.item()), 1e-2, note=f'|loss - oracle| (loss {loss.item():.6f}, oracle {ref.item():.6f})')
    _compare('oracle', got, {k: sdg[k].grad.flatten() for k in got}, 4e-2, 0.999)


def test_batched_step_vs_sequential_step(bat, seq, samples):
    a, b, _ = samples
    out_s = seq.step([a, b]); gs = _grads(seq)
    out_b = bat.step([a, b]); gb = _grads(bat)
    parity('vla_batch_rows.seq.loss', abs(out_b.loss.item() - out_s.loss.item()), 2e-2, note=f'|batched - sequential| loss ({out_b.loss.item():.6f} vs {out_s.loss.item():.6f})')
    _compare('seq', gb, gs, 8e-2, 0.998)


def test_one_sample_batch_is_bit_identical_to_the_one_sample_pass(bat, seq, samples):
    a = samples[0]
    l_s = seq.forward_backward(**a); g_s = seq.fp.g.clone()
    l_b = bat.forward_backward_batch(**a)
    assert l_b.item() == l_s.item(), (l_b.item(), l_s.item())
    if not torch.equal(bits(bat.fp.g), bits(g_s)):
        gs, gb = seq.named_grads(), bat.named_grads()
        raise AssertionError(f'gradients differ in {[k for k in gs if not torch.equal(bits(gs[k]), bits(gb[k]))]}')


def test_groups(golden_model, samples):
    """max_batch = 2 over three samples: groups of 2 + 1 weighing 2/3 and 1/3 through accumulate_bucket, against ONE group of three; reproducible to the bit."""
    a, b, c = samples
    one = _trainer(golden_model, lr=0.0, max_grad_norm=0.0, batch_rows=True, max_batch=32)
    two = _trainer(golden_model, lr=0.0, max_grad_norm=0.0, batch_rows=True, max_batch=2)
    o1 = one.step([a, b, c]); g1 = _grads(one)
    o2 = two.step([a, b, c]); g2 = _grads(two)
    parity('vla_batch_rows.groups.loss', abs(o1.loss.item() - o2.loss.item()), 2e-2, note='|2+1 groups - one group| loss')
    _compare('groups', g2, g1, 8e-2, None)
    del one, two
    runs = []
    for _ in range(2):
        m = _trainer(golden_model, lr=1e-4, max_grad_norm=1.0, batch_rows=True, max_batch=2)
        l0 = m.forward_backward_batch(**a).item()
        outs = [m.step([a, b, c]) for _ in range(3)]
        l1 = m.forward_backward_batch(**a).item()
        runs.append((l0, l1, [o.loss.item() for o in outs], m.fp.p.clone()))
    assert runs[0][1] < runs[0][0], runs[0][:2]
    assert runs[0][2] == runs[1][2] and torch.equal(bits(runs[0][3]), bits(runs[1][3]))


def test_refusals(bat, samples, golden_model):
    from vlaser_amd.vla_train import VLATrainer
    _, vla, _ = golden_model
    with pytest.raises(ValueError, match='vla_vlm_group.py.*vlaser_attn_rows_bwd_ex'):
        VLATrainer(vla, train_vlm=True, batch_rows=True)
    a, b, _ = samples
    bad = dict(b, input_ids=b['input_ids'].clone())
    bad['input_ids'][0, 5] = vla.base.pad_token_id
    with pytest.raises(ValueError, match='sample 1'):
        bat.step([a, bad])
    with pytest.raises(ValueError, match='max_batch'):
        bat.forward_backward_batch(**_cat([a, b, a]))
