"""Helpers shared by the op-level fp64 parity files (tests/test_train_ops_gpu.py, tests/test_fwd_ops_gpu.py, tests/test_sft_ops_gpu.py): the constants of the
derived bounds, the element-by-element comparison that logs its worst figure through tests/parity.py, bit views, sentinel buffers, operand generators with
exact power-of-two scales and the LayerNorm row families, and the fp64 closed form of the fused attention backward with its error model (checked against autograd by tests/test_sft_ops_closed_form.py).
A plain module: it holds no fixture and no pytest hook."""
import math

import torch

from parity import parity

BF = torch.bfloat16
D64 = torch.float64
F32 = torch.float32
U = 2.0 ** -24              # fp32 unit roundoff
ULP = 2.0 ** -7             # one bf16 ulp, relative
FLOOR = 2.0 ** -100         # flush-to-zero near the bottom of the normal range is not an error
SENT = 7.0                  # sentinel of every output buffer before the call
LOG2E32 = float(torch.tensor(1.4426950408889634, dtype=F32))       # log2(e) as the attention kernels hold it


def sentinel(*shape, dtype=BF):
    return torch.full(shape, SENT, dtype=dtype, device='cuda')


def h64(t):
    return t.detach().cpu().to(D64)


def bound(name, got, ref, tol):
    """worst element of |got - ref| / tol; a non-finite output fails"""
    got = h64(got)
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    fig = ((got - ref).abs() / tol).max().item()
    parity(name, fig, 1.0, note='max |got - ref| / tol')


def elementwise(name, got, ref, ulps=1):
    bound(name, got, ref, ulps * ULP * ref.abs() + FLOOR)


def reduction(name, got, ref, ref_abs, n_seq, bf16_out=True):
    bound(name, got, ref, (ULP * ref.abs() if bf16_out else 0.0) + U * n_seq * ref_abs + FLOOR)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def pow2(n, lo=-10, hi=2):
    """2^e with e cycling over lo .. hi"""
    return 2.0 ** ((torch.arange(n) % (hi - lo + 1)) + lo).float()


def randb(*shape, seed=0, std=1.0):
    """bf16-valued fp32 CPU tensor"""
    g = torch.Generator().manual_seed(seed + 7 * sum(shape))
    return (torch.randn(*shape, generator=g) * std).to(BF).float()


def dev(t, dtype=BF):
    return t.to(dtype).cuda().contiguous()


def dev_off(t):
    """device bf16 copy that starts 2 bytes past an aligned address"""
    buf = sentinel(t.numel() + 8)
    buf[1:1 + t.numel()] = t.flatten().to(BF).cuda()
    return buf[1:1 + t.numel()].view(t.shape)


def f32s(x):
    """a Python scalar as the C ABI's float argument holds it"""
    return float(torch.tensor(x, dtype=F32))


def rbf(t):
    """round an fp64 tensor to bf16 (through fp32: a double rounding only on exact fp32 ties of fp64 data, which these products of bf16 values never hit)"""
    return t.to(F32).to(BF).to(D64)


def same_bits(a, b):
    it = torch.int32 if a.dtype == F32 else torch.int16
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def is_sent(t):
    return bool((t == SENT).all())


class Worst:
    """worst |got - ref| / tol over the cases of one test, logged once per name (with the case that gave it)"""

    def __init__(self):
        self.figs = {}

    def add(self, name, got, ref, tol, where=''):
        got = h64(got)
        assert torch.isfinite(got).all(), f'{name} {where}: non-finite output'
        assert got.shape == ref.shape, (name, where, got.shape, ref.shape)
        f = ((got - ref).abs() / tol).max().item() if got.numel() else 0.0
        if name not in self.figs or f > self.figs[name][0]:
            self.figs[name] = (f, where)
        return f

    def flush(self):
        bad = []
        for name, (f, where) in self.figs.items():
            try:
                parity(name, f, 1.0, note=f'max |got - ref| / tol at {where}')
            except AssertionError as e:
                bad.append(str(e))
        assert not bad, '\n'.join(bad)


def attn_bwd_ref(q, k, v, d_o, o, lse2, vis, scale, log2e=LOG2E32):
    """The closed form of csrc/attn_bwd.hip's header in fp64 and the error each step of the kernel's arithmetic allows.  q / d_o / o [H, S, hd], k / v [H, Sk, hd]
    (already repeated over the kv group), lse2 [H, S] (base 2), vis [S, Sk] bool; log2e: the kernel's fp32 constant (the exact one makes the form exact).
    Returns dq [H, S, hd], per-head dk / dv [H, Sk, hd], D [H, S] and their tolerances."""
    S, Sk = q.shape[1], k.shape[1]
    sc = scale * log2e
    s2, s_abs = (q @ k.transpose(1, 2)) * sc, (q.abs() @ k.abs().transpose(1, 2)) * sc
    P = torch.where(vis, torch.exp2(s2 - lse2[..., None]), torch.zeros_like(s2))
    D, D_abs = (d_o * o).sum(-1), (d_o * o).abs().sum(-1)
    dP, dP_abs = d_o @ v.transpose(1, 2), d_o.abs() @ v.abs().transpose(1, 2)
    dS = P * (dP - D[..., None]) * scale
    n14 = 128 // 32 + 10
    e_P = P * (math.log(2) * (U * n14 * s_abs + 2 * U * (s2.abs() + lse2.abs()[..., None])) + 2 * U)
    e_D = U * 34 * D_abs
    e_dS = e_P * (dP - D[..., None]).abs() * scale + P * scale * (U * n14 * dP_abs + e_D[..., None]) + 3 * U * dS.abs()
    n_red = -(-max(S, Sk) // 32) + 11
    red = lambda w, x, e: ULP * (w @ x).abs() + ULP * (w.abs() @ x.abs()) + e @ x.abs() + U * n_red * (w.abs() @ x.abs()) + FLOOR
    return dict(dq=dS @ k, dq_tol=red(dS, k, e_dS), dk=dS.transpose(1, 2) @ q, dk_tol=red(dS.transpose(1, 2), q, e_dS.transpose(1, 2)),
                dv=P.transpose(1, 2) @ d_o, dv_tol=red(P.transpose(1, 2), d_o, e_P.transpose(1, 2)), D=D, D_tol=e_D + FLOOR, P=P, dS=dS)


def _ln_rows(kind, S, C, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 'normal':
        x = torch.randn(S, C, generator=g)
    elif kind == 'offset':          # |mean| / std in 100 .. 200
        m = (100 + 100 * torch.rand(S, 1, generator=g)) * torch.where(torch.rand(S, 1, generator=g) < 0.5, -1.0, 1.0)
        x = m + torch.randn(S, C, generator=g)
    elif kind == 'outlier':         # a few channels 50 x the rest
        x = torch.randn(S, C, generator=g)
        idx = torch.randint(0, C, (S, 4), generator=g)
        x.scatter_(1, idx, 50 * torch.where(torch.rand(S, 4, generator=g) < 0.5, -1.0, 1.0))
    else:                           # near-constant: 8, 64 or 1000 with 1 or 16 channels one bf16 step up
        v = torch.tensor([8.0, 64.0, 1000.0])[torch.arange(S) % 3][:, None]
        x = v.expand(S, C).clone()
        step = 2.0 ** (torch.floor(torch.log2(v)) - 7)
        for s in range(S):
            k = min(1 if s % 2 == 0 else 16, C - 1)
            idx = torch.randperm(C, generator=g)[:k]
            x[s, idx] += step[s, 0]
    return x.to(BF)


LN_KINDS = ('normal', 'offset', 'outlier', 'flat')
