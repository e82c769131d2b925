"""optimizer='adamw8bit' on the GPU: vlaser_adamw8_clipped element by element against an fp64 restatement of its definition, applied to the state the
kernel was given, and the two trainers running on it.

Reference.  The state the kernel is given is (code, absmax) per block of 128; the moment it stands for is the fp32 product table[code] * absmax (ONE rounding:
`ops.adamw8_dequant` forms the same product).  From there, in fp64, with the hyperparameters as the C ABI holds them:
    gs = g gfac;  m' = b1 m + c1 gs;  v' = b2 v + c2 gs^2;  w' = w decay - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)          (c = f32(1 - b))
and tol_m / tol_v / tol_w are the derivation of section F of tests/test_sft_ops_gpu.py for the fp32 kernel, restated in `_ref` (the 8-bit kernel evaluates the
same expressions with the same roundings; k_g = 1 rounding on gs, 5 with the clip factor).  Then per block
  (a) absmax' = max |x'|: max is 1-Lipschitz in every argument, so |absmax' - max |x'_ref|| <= max over the block of tol_x;
  (b) nearest code: |T[code] A - x'| <= min_k |T[k] A - x'| + tol_q with A the absmax the kernel stored and
        tol_q = 2 tol_x + 24 U |x'| + 2e-6 U A + FLOOR:
      the kernel holds x'_k within tol_x of x' (both sides of the inequality move by that: 2 tol_x); it normalises a = x'_k (1 / A): two roundings, 2 U |x'| on each
      side (4 U |x'|); the last compare takes two rounded differences, so it may prefer a neighbour that is farther by <= 2 U gap, and a gap of the tables is
      <= 9 |a| + 5.5e-7 (<= 0.9 of a decade whose smallest entry is >= 0.1 of it; 5.5e-7 next to zero): 18 U |x'| + 1.1e-6 U A.  Ties fall inside the bound.
      The one exception is exact: a second moment the kernel certainly holds as positive (x' > tol_v) never has code 0, and where the nearest entry would be 0
      its code is 1.
  (c) master within tol_w; param == bf16(master) bit for bit;   (d) nothing non-finite.
Blocks of five kinds sit next to each other (`_state`): random state (all 256 codes of both tables occur in the large case); all-zero state and gradient (zero
codes, absmax 0, master = fl(w decay) exactly: unchanged at wd = 0); state without gradient; a single gradient element on zero state; gradients spread over
4 decades on zero state (v' spans 8: the code-1 rule).  128 sentinel elements / one sentinel block behind every array must survive.

Sizes: one block; three; 16 x cap + 5 blocks (cap = the workgroup cap the library reports: 16 blocks per workgroup, so the grid-stride loop wraps once and its
last round is a partial workgroup)."""
import math
import os

import numpy as np
import pytest
import torch

from bounds import BF, F32, FLOOR, SENT, U, Worst, f32s, pow2, same_bits

pytestmark = pytest.mark.gpu
U8 = torch.uint8
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
PAD = 128


@pytest.fixture(scope='module')
def ops():
    from vlaser_amd import ops as o
    return o


def _cap(ops):
    return min(ops.get_cu_budget(), torch.cuda.get_device_properties(0).multi_processor_count)


def _sizes(ops):
    return (128, 384, 128 * (16 * _cap(ops) + 5))


def _state(n, seed, shift=0):
    """CPU operands of one call; block b is of kind (b + shift) % 6: 0 / 5 random, 1 all zero, 2 no gradient, 3 one gradient element, 4 four decades of gradients"""
    g_ = torch.Generator().manual_seed(seed)
    nb = n // 128
    kind = (torch.arange(nb) + shift) % 6
    ke = kind.repeat_interleave(128)
    sc = pow2(nb, -6, 2)
    sce = sc.repeat_interleave(128)
    mc = torch.randint(0, 256, (n,), generator=g_, dtype=U8)
    vc = torch.randint(0, 256, (n,), generator=g_, dtype=U8)
    for b in range(nb - 1):                                  # two adjacent random blocks carry every code of both tables
        if kind[b] == 5 and kind[b + 1] == 0:
            mc[b * 128:(b + 2) * 128] = torch.randperm(256, generator=g_).to(U8)
            vc[b * 128:(b + 2) * 128] = torch.randperm(256, generator=g_).to(U8)
            break
    mam = 0.01 * sc * (0.5 + torch.rand(nb, generator=g_))
    vam = (0.01 * sc) ** 2 * (0.5 + torch.rand(nb, generator=g_))
    w = torch.randn(n, generator=g_) * 0.05
    grad = torch.randn(n, generator=g_) * 0.01 * sce
    zero_state = (kind == 1) | (kind == 3) | (kind == 4)
    zs = zero_state.repeat_interleave(128)
    mc[zs], vc[zs] = 127, 0
    mam[zero_state], vam[zero_state] = 0.0, 0.0
    grad[(ke == 1) | (ke == 2) | (ke == 3)] = 0.0
    one = torch.nonzero(kind == 3).flatten() * 128 + 37
    grad[one] = 0.02 * sc[kind == 3]
    j = torch.arange(128).float()
    spread = 0.5 * 10.0 ** (-4.0 * j / 127) * torch.where(j % 2 == 0, 1.0, -1.0)
    for b in torch.nonzero(kind == 4).flatten().tolist():
        grad[b * 128:(b + 1) * 128] = spread
    return dict(n=n, kind=kind, w=w, mc=mc, vc=vc, mam=mam.to(F32), vam=vam.to(F32), grad=grad.to(BF))


def _padded(t, fill, pad):
    return torch.cat([t, torch.full((pad,), fill, dtype=t.dtype)]).cuda()


def _run(ops, st, step, wd, gscale, gnorm2=None, max_norm=0.0, slot=None, m32=None, v32=None):
    """the kernel on device copies of `st` (a sentinel block behind every array); returns the CPU results"""
    n = st['n']
    d = dict(p=_padded(torch.zeros(n, dtype=BF), SENT, PAD), w=_padded(st['w'], SENT, PAD), mc=_padded(st['mc'], 7, PAD), vc=_padded(st['vc'], 7, PAD),
             mam=_padded(st['mam'], SENT, 1), vam=_padded(st['vam'], SENT, 1), g=_padded(st['grad'], SENT, PAD))
    small = (None, None, None)
    if slot is not None:
        small = (_padded(slot, 77, 1), _padded(m32, SENT, PAD), _padded(v32, SENT, PAD))
    gn = None if gnorm2 is None else torch.tensor([gnorm2], dtype=F32, device='cuda')
    ops.adamw8_clipped(d['p'][:n], d['w'], d['mc'], d['vc'], d['mam'], d['vam'], *small, d['g'], f32s(LR), f32s(B1), f32s(B2), f32s(EPS), f32s(wd), f32s(gscale),
                       gn, f32s(max_norm), step)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in d.items()}
    if slot is not None:
        out['slot'], out['m32'], out['v32'] = (t.cpu() for t in small)
        assert torch.equal(out['slot'][:-1], slot) and int(out['slot'][-1]) == 77
        assert bool((out['m32'][-PAD:] == SENT).all()) and bool((out['v32'][-PAD:] == SENT).all()), 'm32 / v32 written past their end'
    for k in ('p', 'w', 'g'):
        assert bool((out[k][n:].float() == SENT).all()), f'{k} written past n'
    assert bool((out['mc'][n:] == 7).all()) and bool((out['vc'][n:] == 7).all()), 'codes written past n'
    assert float(out['mam'][-1]) == SENT and float(out['vam'][-1]) == SENT, 'absmax written past the last block'
    assert same_bits(out['g'][:n], st['grad']), 'the gradient was modified'
    return {k: (v[:n] if k in ('p', 'w', 'mc', 'vc', 'g') else v[:-1] if k in ('mam', 'vam') else v) for k, v in out.items()}


def _ref(w, m, v, grad, wd, gfac, k_g, step):
    """fp64 AdamW from fp32 state + the tolerances of section F of tests/test_sft_ops_gpu.py (restated; the module docstring)"""
    lr, b1, b2, eps, wd = f32s(LR), f32s(B1), f32s(B2), f32s(EPS), f32s(wd)
    w, m, v, grad = (t.double() for t in (w, m, v, grad))
    c1, c2 = float(torch.tensor(1.0, dtype=F32) - torch.tensor(b1, dtype=F32)), float(torch.tensor(1.0, dtype=F32) - torch.tensor(b2, dtype=F32))
    gs = grad * gfac
    m1, v1 = b1 * m + c1 * gs, b2 * v + c2 * gs * gs
    tol_m = U * (2 * (b1 * m).abs() + (2 + k_g) * (c1 * gs).abs()) + FLOOR
    tol_v = U * (2 * b2 * v + (3 + 2 * k_g) * c2 * gs * gs) + FLOOR
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    e1, e2 = 2 * U * b1 ** step / bc1 + U, 2 * U * b2 ** step / bc2 + U
    rbc2, decay, stp = 1.0 / math.sqrt(bc2), 1.0 - lr * wd, lr / bc1
    sq = torch.sqrt(v1)
    den = sq * rbc2 + eps
    e_sqrt = torch.minimum(tol_v / sq.clamp_min(1e-300), torch.sqrt(tol_v)) + 2 * U * sq
    e_den = e_sqrt * rbc2 + sq * rbc2 * (e2 / 2 + 3 * U) + U * den
    upd = stp * m1 / den
    e_upd = stp * (tol_m / den + m1.abs() * e_den / den ** 2 + 2 * U * (m1 / den).abs()) + upd.abs() * (e1 + 2 * U)
    ref = w * decay - upd
    tol_w = 4 * U * (w * decay).abs() + e_upd + U * upd.abs() + U * ref.abs() + FLOOR
    return m1, v1, ref, tol_m, tol_v, tol_w


def _clip(gscale, gnorm2, max_norm):
    """(gfac in fp64, k_g) as section F forms them"""
    gscale = f32s(gscale)
    if gnorm2 is None:
        return gscale, 1
    gn, mx = math.sqrt(f32s(gnorm2)), f32s(max_norm)
    if mx > 0 and gn > mx:
        return gscale * mx / (gn + f32s(1e-6)), 5
    return gscale, 1


def _excess(table, code, absmax, x, tol_x):
    """(|T[code] A - x| - min_k |T[k] A - x|) / tol_q per element, and the fp64-nearest code's value being T[0] (unsigned: "would be stored as 0")"""
    T = table.double()
    A = absmax.double().repeat_interleave(128)
    a = torch.where(A > 0, x / A.clamp_min(1e-300), torch.zeros_like(x))
    hi = torch.searchsorted(T, a).clamp(1, 255)
    d_lo, d_hi = (T[hi - 1] * A - x).abs(), (T[hi] * A - x).abs()
    best = torch.minimum(d_lo, d_hi)
    got = (T[code.long()] * A - x).abs()
    tol_q = 2 * tol_x + 24 * U * x.abs() + 2e-6 * U * A + FLOOR
    nearest_is_first = (hi == 1) & (d_lo <= d_hi)
    return (got - best) / tol_q, nearest_is_first


def _check(ops, worst, tag, st, out, step, wd, gfac, k_g, where, blocks=None):
    """assertions (a) - (d) of the module docstring on the 8-bit blocks `blocks` (default: all)"""
    Ts, Tu = ops.adamw8_codes()
    n, nb = st['n'], st['n'] // 128
    sel = torch.ones(nb, dtype=torch.bool) if blocks is None else blocks
    se = sel.repeat_interleave(128)
    m0, v0 = ops.adamw8_dequant(st['mc'], st['mam'], Ts), ops.adamw8_dequant(st['vc'], st['vam'], Tu)
    m1, v1, ref, tol_m, tol_v, tol_w = _ref(st['w'], m0, v0, st['grad'].float(), wd, gfac, k_g, step)
    for k in ('w', 'mam', 'vam'):
        assert bool(torch.isfinite(out[k]).all()), f'{tag} {where}: non-finite {k}'
    blk = lambda t: t.view(nb, 128)
    # (a)
    worst.add(f'{tag}.m_absmax', out['mam'][sel], blk(m1.abs()).max(1).values[sel], blk(tol_m).max(1).values[sel], where)
    worst.add(f'{tag}.v_absmax', out['vam'][sel], blk(v1).max(1).values[sel], blk(tol_v).max(1).values[sel], where)
    # (b)
    ex_m, _ = _excess(Ts, out['mc'], out['mam'], m1, tol_m)
    ex_v, first = _excess(Tu, out['vc'], out['vam'], v1, tol_v)
    positive = v1 > tol_v
    ruled = positive & first                                 # nearest rounding would store 0: the code is 1, exactly
    assert bool((out['vc'][se & positive] != 0).all()), f'{tag} {where}: a positive second moment was stored as code 0'
    assert bool((out['vc'][se & ruled] == 1).all()), f'{tag} {where}: the code-1 rule'
    ambiguous = (v1 > 0) & ~positive & (out['vc'] == 1)      # the kernel may hold a FLOOR-sized moment as positive or as zero
    f_m = float(ex_m[se].max()) if bool(se.any()) else 0.0
    keep = se & ~ruled & ~ambiguous
    f_v = float(ex_v[keep].max()) if bool(keep.any()) else 0.0
    for name, f in ((f'{tag}.m_code', f_m), (f'{tag}.v_code', f_v)):
        if name not in worst.figs or f > worst.figs[name][0]:
            worst.figs[name] = (f, where)
    # (c)
    worst.add(f'{tag}.master', out['w'][se], ref[se], tol_w[se], where)
    assert same_bits(out['p'], out['w'].to(BF)), f'{tag} {where}: p is not bf16(master)'
    # the kinds of blocks
    kind = st['kind']
    z = sel & (kind == 1)
    ze = z.repeat_interleave(128)
    if bool(z.any()):
        assert bool((out['mc'][ze] == 127).all()) and bool((out['vc'][ze] == 0).all()), f'{tag} {where}: an all-zero block must keep the zero codes'
        assert bool((out['mam'][z] == 0).all()) and bool((out['vam'][z] == 0).all()), f'{tag} {where}: an all-zero block must keep absmax 0'
        if wd == 0:                                          # (with decay the master is fl(w decay): assertion (c))
            assert same_bits(out['w'][ze], st['w'][ze]), f'{tag} {where}: an all-zero block moved its master'
    s4 = (sel & (kind == 4)).repeat_interleave(128)
    if bool(s4.any()):
        assert bool((out['vc'][s4] != 0).all()), f'{tag} {where}: the 8-decade block lost a second moment'
        assert bool((ruled & s4).any()), 'the 8-decade block does not exercise the code-1 rule'
    return ruled


@pytest.mark.parametrize('step', [1, 2, 1000])
def test_one_step_from_prepared_state(ops, step):
    """sizes x (wd, grad_scale) in ((0, 1), (0.05, 0.37)); the block kinds rotate with the case so that the one- and three-block sizes meet all of them"""
    worst = Worst()
    seen, shift = set(), 0
    for n in _sizes(ops):
        for wd, gscale in ((0.0, 1.0), (0.05, 0.37)):
            for sh in ((0, 1, 2, 3, 4, 5) if n == 128 else (shift, shift + 3)):
                st = _state(n, seed=n + step + sh, shift=sh)
                seen.update(st['kind'].tolist())
                if n > 384:
                    assert len(set(st['mc'].tolist())) == 256 and len(set(st['vc'].tolist())) == 256
                out = _run(ops, st, step, wd, gscale)
                _check(ops, worst, 'adamw8', st, out, step, wd, f32s(gscale), 1, f'n={n},step={step},wd={wd:g},gscale={gscale:g},shift={sh}')
            shift += 1
    assert seen == set(range(6))
    worst.flush()


def _slot_case(ops, n, step, gnorm2, max_norm):
    st = _state(n, seed=n + 17, shift=2)
    nb = n // 128
    odd = torch.arange(nb) % 2 == 1
    oe = odd.repeat_interleave(128)
    slot = torch.where(odd, torch.arange(nb) // 2, torch.full((nb,), -1)).to(torch.int32)
    n32 = int(odd.sum()) * 128
    g_ = torch.Generator().manual_seed(n)
    m32 = (torch.randn(n32, generator=g_) * 0.01).to(F32)
    v32 = ((torch.randn(n32, generator=g_) * 0.01) ** 2).to(F32)
    wd, gscale = 0.05, 0.37
    plain = _run(ops, st, step, wd, gscale, gnorm2, max_norm)
    mixed = _run(ops, st, step, wd, gscale, gnorm2, max_norm, slot=slot, m32=m32, v32=v32)
    where = f'n={n},step={step},gnorm2={gnorm2},max_norm={max_norm}'
    # the 8-bit blocks do not see their neighbours
    for k in ('p', 'w', 'mc', 'vc'):
        assert torch.equal(mixed[k][~oe], plain[k][~oe]), f'{where}: {k} of the 8-bit blocks'
    for k in ('mam', 'vam'):
        assert same_bits(mixed[k][~odd], plain[k][~odd]), f'{where}: {k} of the 8-bit blocks'
        assert same_bits(mixed[k][odd], st[k][odd]) and torch.equal(mixed['mc'][oe], st['mc'][oe]) and torch.equal(mixed['vc'][oe], st['vc'][oe]), \
            f'{where}: an fp32-slot block wrote 8-bit state'
    if n32 == 0:
        return
    # the fp32-slot blocks alone through the fp32 kernel
    p = torch.zeros(n32, dtype=BF).cuda()
    w, m, v, g = st['w'][oe].cuda(), m32.cuda(), v32.cuda(), st['grad'][oe].cuda()
    gn = torch.tensor([gnorm2 if gnorm2 is not None else 0.0], dtype=F32, device='cuda')
    ops.adamw_clipped(p, w, m, v, g, f32s(LR), f32s(B1), f32s(B2), f32s(EPS), f32s(wd), f32s(gscale), gn, f32s(max_norm), step)
    torch.cuda.synchronize()
    assert same_bits(mixed['m32'][:n32], m.cpu()), f'{where}: m32'
    assert same_bits(mixed['v32'][:n32], v.cpu()), f'{where}: v32'
    assert same_bits(mixed['w'][oe], w.cpu()), f'{where}: master of the fp32-slot blocks'
    assert same_bits(mixed['p'][oe], p.cpu()), f'{where}: param of the fp32-slot blocks'


def test_fp32_slot_blocks_are_the_fp32_kernel_bit_for_bit(ops):
    """every other block fp32: those blocks equal vlaser_adamw_clipped run on them alone, the 8-bit blocks equal the run without slots -- with and without
    an active clip factor, at three blocks and at the size that wraps the grid"""
    for n in _sizes(ops):
        for step, gnorm2, max_norm in ((1, None, 0.0), (2, 9.0, 2.0), (1000, 1.0, 2.0)):
            _slot_case(ops, n, step, gnorm2, max_norm)


def test_clipping(ops):
    """gnorm2 below, equal to and above max_norm^2, and max_norm = 0, at n = 384: the reference with the clip factor formed in fp64; no gnorm2 == max_norm 0"""
    worst = Worst()
    n, step, wd, gscale = 384, 2, 0.05, 0.37
    for sh in (0, 3):
        st = _state(n, seed=5 + sh, shift=sh)
        for gnorm2, max_norm in ((1.0, 2.0), (4.0, 2.0), (9.0, 2.0), (1e6, 0.0)):
            out = _run(ops, st, step, wd, gscale, gnorm2, max_norm)
            gfac, k_g = _clip(gscale, gnorm2, max_norm)
            _check(ops, worst, 'adamw8_clip', st, out, step, wd, gfac, k_g, f'shift={sh},gnorm2={gnorm2:g},max_norm={max_norm:g}')
        off, none = _run(ops, st, step, wd, gscale, 1e6, 0.0), _run(ops, st, step, wd, gscale, None, 0.0)
        for k in ('p', 'w', 'mc', 'vc', 'mam', 'vam'):
            assert torch.equal(off[k], none[k]), k
        clipped = _run(ops, st, step, wd, gscale, 9.0, 2.0)
        assert not torch.equal(clipped['w'], none['w'])      # the factor really arrived
    worst.flush()


def test_determinism(ops):
    n = _sizes(ops)[-1]
    st = _state(n, seed=3, shift=1)
    a, b = _run(ops, st, 7, 0.05, 0.37, 9.0, 2.0), _run(ops, st, 7, 0.05, 0.37, 9.0, 2.0)
    for k in ('p', 'w', 'mc', 'vc', 'mam', 'vam'):
        assert torch.equal(a[k], b[k]), k


# ================================================================================================ the trainers
def _sft_inputs(golden_dir):
    d = np.load(os.path.join(golden_dir, 'g5g6_vlm.npz'))
    ids = torch.from_numpy(d['input_ids'])
    pv = torch.randn(1, 3, 448, 448, generator=torch.Generator().manual_seed(0))
    labels = torch.full_like(ids, -100)
    labels[0, -16:] = ids[0, -16:]
    return pv, ids, labels


def _state_tensors(g):
    return dict(master=g.master, m_code=g.m_code, v_code=g.v_code, m_absmax=g.m_absmax, v_absmax=g.v_absmax, slot=g.slot, m32=g.m32, v32=g.v32)


def test_sft_model_trains_on_8bit_moments(golden_model, golden_dir):
    """6 steps on one sample (lr 1e-3, wd 0.05: the multi-step settings of tests/test_sft_gpu.py) beside an 'adamw' model.  Step 1 starts from zero moments in
    both and updates from the fresh fp32 moments: the masters agree within the rounding of the update, 4 U (|w| + lr).  The 8-bit loss falls and recovers at
    least half of the fp32 run's decrease (a guard against a mis-scaled state, not a measured tolerance).  State: no fp32 tensor of shard size besides the
    master; <= 6.1 B per shard element + 8 B per fp32-slot element."""
    from vlaser_amd.sft import SFTModel
    cfg, _, sd = golden_model
    pv, ids, labels = _sft_inputs(golden_dir)
    mk = lambda opt: SFTModel(cfg, max_seq_len=ids.shape[1], lr=1e-3, weight_decay=0.05, optimizer=opt).load_state_dict(sd)
    a, b = mk('adamw'), mk('adamw8bit')
    assert b.optimizer == 'adamw8bit' and a.optimizer == 'adamw' and not hasattr(b, 'm') and not hasattr(b, 'v')
    curves = {'adamw': [], 'adamw8bit': []}
    worst_diff = 0.0
    for s in range(6):
        for m in (a, b):
            curves[m.optimizer].append(float(m.step(pv, ids, labels).loss))
        if s == 0:
            a.wait_optimizer(); b.wait_optimizer()
            wa, wb = a.master.double(), b.master.double()
            worst_diff = float((wa - wb).abs().max())
            assert bool(((wa - wb).abs() <= 4 * U * (wa.abs() + 1e-3)).all()), f'after step 1 the masters differ by up to {worst_diff:g}'
    for m in (a, b):
        curves[m.optimizer].append(float(m.forward_backward(pv, ids, labels)))
    a.wait_optimizer(); b.wait_optimizer()
    print('adamw8bit SFT loss curves (6 steps + the loss after them):', curves, 'largest master difference after step 1:', worst_diff,
          'largest bf16 parameter difference after 6 steps:', float((a.fp.p.float() - b.fp.p.float()).abs().max()))
    l32, l8 = curves['adamw'], curves['adamw8bit']
    assert all(math.isfinite(x) for x in l8) and l8[-1] < l8[0], l8
    assert l32[0] - l32[-1] > 0 and l8[0] - l8[-1] >= 0.5 * (l32[0] - l32[-1]), (l32, l8)
    n_shard = b.master.numel()
    big = [k for k, t in vars(b).items() if torch.is_tensor(t) and t.dtype == F32 and t.numel() >= n_shard and k != 'master']
    assert not big, f'fp32 tensors of shard size besides the master: {big}'
    n_small = int((b.slot >= 0).sum()) * 128
    assert 0 < n_small < n_shard // 100 and b.m32.numel() == n_small
    nbytes = sum(t.numel() * t.element_size() for t in _state_tensors(b).values())
    assert nbytes <= 6.1 * n_shard + 8 * n_small, (nbytes / n_shard, n_small)
    assert bool((b.m_code != 127).any()) and bool((b.v_absmax > 0).any())


def _vla_case(golden_dir, case='a'):
    d = np.load(os.path.join(golden_dir, 'g7_vla.npz'))
    f = np.load(os.path.join(golden_dir, 'g10_flow_matching.npz'))
    pv = torch.randn(1, 3, 448, 448, generator=torch.Generator().manual_seed(int(d[f'{case}_seed'])))
    return dict(input_ids=torch.from_numpy(d[f'{case}_input_ids']), pixel_values=pv, proprios=torch.from_numpy(d[f'{case}_proprio']),
                actions=torch.from_numpy(f[f'{case}_actions']), t=torch.from_numpy(f[f'{case}_t']), x0=torch.from_numpy(f[f'{case}_x0']))


def _vla(vla, sd, optimizer='adamw8bit', lr=1e-4, vlm_lr=2e-5):
    from vlaser_amd.vla_train import VLATrainer
    return VLATrainer(vla, lr=lr, max_grad_norm=1.0, train_vlm=True, vlm_lr=vlm_lr, optimizer=optimizer).load_state_dict(sd)


def test_vla_trainer_both_groups_carry_code_state(golden_model, golden_dir):
    """train_vlm=True on the G10b inputs, 2 steps: the action-expert group AND the VLM group hold codes, the loss is finite and falls on the repeated sample,
    the norm weights' blocks keep fp32 moments.

    Learning rates 1e-5 / 2e-6.  Adam's first update moves EVERY element by lr whatever its gradient, so whether the loss of this 2 + 2-layer model falls
    right after it is a property of lr, not of the moments' storage: step 1 starts from zero moments and is bit-identical under both optimizers.  Measured
    with the fp32 optimizer ('adamw', the code as it was) on this sample -- loss of step 1, of step 2, after step 2: 1e-4 / 2e-5 (the rates of
    test_vla_train_gpu.py's 3-step test): 1.1089, 2.5448, 1.0637 (it rises after the first update, then recovers); 5e-5 / 5e-5: 1.1089, 1.2526, 0.7902;
    1e-5 / 2e-6: 1.1089, 1.0511, 0.9083 -- the rates at which the fp32 run falls at every step, so the same is asked of the 8-bit run (it gave 1.1089,
    1.0511, 0.9085)."""
    _, vla, sd = golden_model
    smp = _vla_case(golden_dir)
    m = _vla(vla, sd, lr=1e-5, vlm_lr=2e-6)
    losses = [float(m.step([smp]).loss) for _ in range(2)]
    losses.append(float(m.forward_backward(**smp)))
    torch.cuda.synchronize()
    print('adamw8bit vla_train losses (step 1, step 2, after):', losses)
    assert all(math.isfinite(x) for x in losses) and losses[2] < losses[1] < losses[0], losses
    assert m.vg.optimizer == 'adamw8bit'
    for g in m.groups():
        assert g.optimizer == 'adamw8bit' and not hasattr(g, 'm')
        assert bool((g.m_code != 127).any()) and bool((g.v_code != 0).any()) and bool((g.m_absmax > 0).any()) and bool((g.v_absmax > 0).any())
        assert bool(torch.isfinite(g.master).all())
        slot = g.slot.cpu()                                  # world 1: the shards are the buckets, back to back = the flat buffer
        assert slot.numel() == g.fp.n // 128
        norms = [(nm, shape, off) for nm, shape, off in g.fp.specs if nm == 'norm' or nm.endswith(('.ln_in', '.ln_post', '.n1w', '.n2w'))]
        assert norms
        for nm, shape, off in norms:
            numel = int(np.prod(shape))
            assert numel < 4096 and bool((slot[off // 128:(off + numel + 127) // 128] >= 0).all()), nm
        big = [nm for nm, shape, off in g.fp.specs if int(np.prod(shape)) >= 4096]
        off = g.fp.offset_of(big[0])
        assert int(slot[off // 128]) == -1


def test_checkpoint_resume_is_bit_identical_and_modes_do_not_mix(golden_model, golden_dir, tmp_path):
    _, vla, sd = golden_model
    smp = _vla_case(golden_dir)
    a = _vla(vla, sd)
    for _ in range(2):
        a.step([smp])
    path = str(tmp_path / 'step2.pt')
    a.save_checkpoint(path, sd)
    c = _vla(vla, sd)
    c.load_checkpoint(path)
    assert c.step_count == 2
    a.step([smp]); c.step([smp])
    torch.cuda.synchronize()
    for ga, gc in zip(a.groups(), c.groups()):
        assert torch.equal(ga.fp.p, gc.fp.p)
        for k, t in _state_tensors(ga).items():
            assert torch.equal(t, _state_tensors(gc)[k]), k
    st = torch.load(a._opt_shard_path(path), map_location='cpu', weights_only=True)
    assert st['optimizer'] == 'adamw8bit' and st['vlm_optimizer'] == 'adamw8bit'
    for k in ('exp_avg_code', 'exp_avg_absmax', 'exp_avg_sq_code', 'exp_avg_sq_absmax', 'exp_avg_small', 'exp_avg_sq_small', 'master'):
        assert k in st and 'vlm_' + k in st, k
    assert 'exp_avg' not in st
    d = _vla(vla, sd, 'adamw')
    with pytest.raises(ValueError, match='adamw8bit.*adamw|adamw.*adamw8bit'):
        d.load_checkpoint(path)
    path32 = str(tmp_path / 'fp32.pt')
    d.save_checkpoint(path32, sd)
    with pytest.raises(ValueError, match='adamw8bit'):
        c.load_checkpoint(path32)


def test_unknown_optimizer_is_refused(golden_model):
    from vlaser_amd.sft import SFTModel
    from vlaser_amd.vla_train import VLATrainer
    cfg, vla, _ = golden_model
    with pytest.raises(ValueError, match='adam8'):
        SFTModel(cfg, optimizer='adam8')
    with pytest.raises(ValueError, match='adam8'):
        VLATrainer(vla, optimizer='adam8')
