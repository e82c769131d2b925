"""Helpers shared by the op-level fp64 parity files (tests/test_train_ops_gpu.py, tests/test_fwd_ops_gpu.py): the constants of the derived
bounds, the element-by-element comparison that logs its worst figure through tests/parity.py, bit views, sentinel buffers and the LayerNorm
row families.  A plain module: it holds no fixture and no pytest hook."""
import torch

from parity import parity

BF = torch.bfloat16
D64 = torch.float64
U = 2.0 ** -24              # fp32 unit roundoff
ULP = 2.0 ** -7             # one bf16 ulp, relative
FLOOR = 2.0 ** -100         # flush-to-zero near the bottom of the normal range is not an error
SENT = 7.0                  # sentinel of every output buffer before the call


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
