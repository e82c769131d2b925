"""Varlen attention (block-diagonal causal over concatenated sequences, csrc/attn.hip + csrc/attn_bwd.hip `VARLEN`) op by op:
against fp64 autograd of the masked softmax on the same bf16 inputs, bit for bit against the causal kernels for one sequence, run to run, and
sequence against sequence (nothing leaks across a boundary).  Bounds are `close()` of tests/test_ops_gpu.py and that file's lse / delta bounds."""
import pytest
import torch

from test_ops_gpu import close, rnd

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
HD = 128
LOG2E = 1.4426950408889634


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vlaser_amd import ops as o
    return o


def _inputs(M, nq, nkv, smax, seed=0):
    q = rnd(M, nq * HD, seed=seed + 1)
    k = rnd(1, nkv, smax, HD, seed=seed + 2)
    v = rnd(1, nkv, smax, HD, seed=seed + 3)
    d_o = rnd(M, nq * HD, seed=seed + 4)
    return q, k, v, d_o


def _cu(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu, torch.tensor(cu, dtype=torch.int32, device='cuda')


SENT = 7.0


def _run_varlen(ops, q, k, v, d_o, lens, nq, nkv, smax):
    """Forward + backward through the varlen kernels; every output starts from a sentinel and has rows beyond M."""
    cu_h, cu = _cu(lens)
    M = cu_h[-1]
    vt = v.transpose(-1, -2).contiguous()
    sc = HD ** -0.5
    out = torch.full((smax, nq * HD), SENT, dtype=BF, device='cuda')
    lse = torch.full((nq * M + 64,), SENT, dtype=torch.float32, device='cuda')
    ops.attn_varlen(q, k, vt, out, M, nq, nkv, HD, smax, sc, cu, lse_out=lse, cu_host=cu_h)
    dq, dk, dv = (torch.full((smax, nq * HD), SENT, dtype=BF, device='cuda') for _ in range(3))
    delta = torch.full((nq * M + 64,), SENT, dtype=torch.float32, device='cuda')
    ops.attn_bwd_varlen(q, k, vt, out, d_o, lse, delta, dq, dk, dv, M, nq, nkv, smax, sc, cu, cu_host=cu_h)
    torch.cuda.synchronize()
    return dict(out=out, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv)


def _reference(q, k, v, d_o, lens, nq, nkv):
    """fp64 autograd of the masked softmax, one sequence at a time (the block-diagonal causal mask: nothing outside a sequence's own block is visible)."""
    G, sc = nq // nkv, HD ** -0.5
    M = sum(lens)
    o_ref = torch.zeros(M, nq * HD, dtype=torch.float64, device='cuda')
    lse_ref = torch.zeros(nq, M, dtype=torch.float64, device='cuda')
    dq_ref = torch.zeros(M, nq * HD, dtype=torch.float64, device='cuda')
    dk_ref = torch.zeros(nkv, M, HD, dtype=torch.float64, device='cuda')
    dv_ref = torch.zeros(nkv, M, HD, dtype=torch.float64, device='cuda')
    lo = 0
    for n in lens:
        hi = lo + n
        if n == 0:
            continue
        with torch.enable_grad():
            qf = q[lo:hi].double().view(n, nq, HD).permute(1, 0, 2).clone().requires_grad_(True)
            kf = k[0, :, lo:hi].double().clone().requires_grad_(True)
            vf = v[0, :, lo:hi].double().clone().requires_grad_(True)
            s_ = (qf @ kf.repeat_interleave(G, 0).transpose(-1, -2)) * sc
            i = torch.arange(n, device='cuda')
            s_ = s_.masked_fill(~(i[None, :] <= i[:, None])[None], float('-inf'))
            o = (s_.softmax(-1) @ vf.repeat_interleave(G, 0)).permute(1, 0, 2).reshape(n, nq * HD)
            lse_ref[:, lo:hi] = (torch.logsumexp(s_, -1) * LOG2E).detach()
            o.backward(d_o[lo:hi].double())
        o_ref[lo:hi] = o.detach()
        dq_ref[lo:hi] = qf.grad.permute(1, 0, 2).reshape(n, nq * HD)
        dk_ref[:, lo:hi] = kf.grad
        dv_ref[:, lo:hi] = vf.grad
        lo = hi
    return dict(out=o_ref, lse=lse_ref, dq=dq_ref, dk=dk_ref, dv=dv_ref)


def _kv_sum(t, M, nq, nkv):
    """The per-Q-head dK / dV partials summed over each kv group (what vlaser_rope_bwd_pack does): [nkv, M, HD] fp32."""
    return t[:M].float().view(M, nkv, nq // nkv, HD).sum(2).permute(1, 0, 2)


def _max_err(got, ref):
    return (got.double() - ref.double()).abs().max().item()


LENGTH_SETS = [[64], [1], [63, 65], [1, 1, 130, 64, 5], [288, 301, 277, 295], [560] * 4, [1100, 37, 200]]


@pytest.mark.parametrize('nq,nkv', [(12, 2), (28, 4)])
@pytest.mark.parametrize('lens', LENGTH_SETS, ids=lambda l: 'x'.join(map(str, l)))
def test_attn_varlen_vs_fp64_autograd(ops, lens, nq, nkv):
    """out, lse, delta, dq, summed dk / dv of the varlen kernels against fp64 autograd; rows >= M of every output keep their sentinel.
    The set with a sequence > 1024: if `close()` does not hold there, the existing single-sequence kernels run on that sequence alone and the varlen error
    against fp64 must stay within 1.25 x theirs (same algorithm, only the first tile's alignment differs) -- the bound itself is not widened.  (Measured:
    the [1100, 37, 200] set meets `close()` outright, dq 0.0126-0.0131 of a reference max of 3.0-3.6, so that branch has not been taken yet.)

    Lengths `[1]`: one row of one key, P = 1 and dS = 0, so the reference of dq and dk is identically zero and `close()` allows 1e-6.  The varlen backward writes
    exact zeros there (a one-token sequence's dS is set to 0 instead of being formed as the difference of two equal fp32 sums taken in different orders, which
    measured 1.3e-6)."""
    M = sum(lens)
    smax = (M + 63) // 64 * 64 + 64
    q, k, v, d_o = _inputs(M, nq, nkv, smax, seed=len(lens))
    got = _run_varlen(ops, q, k, v, d_o, lens, nq, nkv, smax)
    ref = _reference(q, k, v, d_o, lens, nq, nkv)
    # rows >= M untouched
    for nm in ('out', 'dq', 'dk', 'dv'):
        assert bool((got[nm][M:] == SENT).all()), f'{nm}: rows >= M were written'
    assert bool((got['lse'][nq * M:] == SENT).all()) and bool((got['delta'][nq * M:] == SENT).all())
    lse_err = _max_err(got['lse'][:nq * M].view(nq, M), ref['lse'])
    d_ref = (d_o.float() * got['out'][:M].float()).view(M, nq, HD).sum(-1).t()
    delta_err = _max_err(got['delta'][:nq * M].view(nq, M), d_ref)
    pairs = {'out': (got['out'][:M], ref['out']), 'dq': (got['dq'][:M], ref['dq']),
             'dk': (_kv_sum(got['dk'], M, nq, nkv), ref['dk']), 'dv': (_kv_sum(got['dv'], M, nq, nkv), ref['dv'])}
    for nm, (g, r) in pairs.items():
        print(f'varlen {lens} heads ({nq},{nkv}) {nm}: max|err| {_max_err(g, r):.4g} of ref max {r.abs().max().item():.4g}')
    print(f'varlen {lens} heads ({nq},{nkv}) lse err {lse_err:.3g} delta err {delta_err:.3g}')
    assert lse_err < 2e-2
    assert delta_err < 1e-3 * max(1.0, d_ref.abs().max().item())
    long_seq = max(lens) > 1024
    for nm, (g, r) in pairs.items():
        try:
            close(g, r, name=nm)
        except AssertionError:
            if not long_seq:
                raise
            # the long sequence alone through the existing causal kernels: same inputs, rows [lo, hi) moved to the front of a cache of their own
            b = lens.index(max(lens))
            lo = sum(lens[:b]); n = lens[b]; hi = lo + n
            single, _ = _run_single(ops, q[lo:hi].contiguous(), k[:, :, lo:hi], v[:, :, lo:hi], d_o[lo:hi].contiguous(), nq, nkv)
            sl = {'out': lambda t: t[lo:hi], 'dq': lambda t: t[lo:hi], 'dk': lambda t: t[:, lo:hi], 'dv': lambda t: t[:, lo:hi]}[nm]
            gs = single[nm][:n] if nm in ('out', 'dq') else _kv_sum(single[nm], n, nq, nkv)
            e_var, e_one = _max_err(sl(g), sl(r)), _max_err(gs, sl(r))
            print(f'varlen {lens} {nm}: close() not met; long sequence alone: varlen err {e_var:.4g}, single-sequence kernels {e_one:.4g}')
            assert e_var <= 1.25 * e_one, (nm, e_var, e_one)
            other = torch.ones(M, dtype=torch.bool, device='cuda'); other[lo:hi] = False
            if bool(other.any()):
                close(g[other] if nm in ('out', 'dq') else g[:, other], r[other] if nm in ('out', 'dq') else r[:, other], name=nm + ' (other sequences)')


def _run_single(ops, q, k, v, d_o, nq, nkv):
    """One sequence through the existing causal forward + fused backward; returns the outputs and the (K, V) caches it built."""
    from vlaser_amd import _lib as L
    S = q.shape[0]
    smax = (S + 63) // 64 * 64 + 64
    kc = torch.zeros(1, nkv, smax, HD, dtype=BF, device='cuda'); kc[:, :, :S] = k
    vc = torch.zeros(1, nkv, smax, HD, dtype=BF, device='cuda'); vc[:, :, :S] = v
    vt = vc.transpose(-1, -2).contiguous()
    sc = HD ** -0.5
    out = torch.full((smax, nq * HD), SENT, dtype=BF, device='cuda')
    lse = torch.full((nq * S + 64,), SENT, dtype=torch.float32, device='cuda')
    ops.attn_prefill(q, kc, vt, out, 1, S, S, nq, nkv, HD, (S * nq * HD, HD, nq * HD), (nkv * smax * HD, smax * HD), (nkv * HD * smax, HD * smax),
                     (S * nq * HD, nq * HD), smax, sc, L.ATTN_CAUSAL, lse_out=lse)
    dq, dk, dv = (torch.full((smax, nq * HD), SENT, dtype=BF, device='cuda') for _ in range(3))
    delta = torch.full((nq * S + 64,), SENT, dtype=torch.float32, device='cuda')
    ops.attn_bwd(q, kc, vt, out, d_o, lse, delta, dq, dk, dv, S, nq, nkv, smax, sc, causal=True)
    torch.cuda.synchronize()
    return dict(out=out, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv), (kc, vc)


@pytest.mark.parametrize('nq,nkv', [(12, 2), (28, 4)])
@pytest.mark.parametrize('S', [70, 336, 389, 560])
def test_one_sequence_is_bit_equal_to_the_causal_kernels(ops, S, nq, nkv):
    """n_seqs == 1 (cu_seqlens = [0, S]): the tile walk is the causal one, so out, lse, delta, dq, dk, dv carry the bits of attn_prefill(ATTN_CAUSAL) +
    attn_bwd(causal=1) on the same inputs -- the shared kernel bodies were not disturbed."""
    smax = (S + 63) // 64 * 64 + 64
    q, k, v, d_o = _inputs(S, nq, nkv, smax, seed=S)
    one, (kc, vc) = _run_single(ops, q, k[:, :, :S], v[:, :, :S], d_o, nq, nkv)
    var = _run_varlen(ops, q, kc, vc, d_o, [S], nq, nkv, smax)
    for nm in ('out', 'lse', 'delta', 'dq', 'dk', 'dv'):
        assert torch.equal(var[nm], one[nm]), f'{nm} differs from the causal kernels'


@pytest.mark.parametrize('lens', [[1, 1, 130, 64, 5], [288, 301, 277, 295]], ids=lambda l: 'x'.join(map(str, l)))
def test_two_runs_are_bit_identical(ops, lens):
    nq, nkv = 12, 2
    M = sum(lens)
    smax = (M + 63) // 64 * 64
    q, k, v, d_o = _inputs(M, nq, nkv, smax, seed=11)
    a = _run_varlen(ops, q, k, v, d_o, lens, nq, nkv, smax)
    b = _run_varlen(ops, q, k, v, d_o, lens, nq, nkv, smax)
    for nm in a:
        assert torch.equal(a[nm], b[nm]), nm


@pytest.mark.parametrize('lens', [[288, 301, 277, 295], [40, 3, 70, 129]], ids=lambda l: 'x'.join(map(str, l)))
def test_sequences_are_independent(ops, lens):
    """Changing q / k / v / d_o of sequence 2 leaves every output row of sequences 0, 1, 3 bit-identical."""
    nq, nkv = 12, 2
    cu_h, _ = _cu(lens)
    M = cu_h[-1]
    smax = (M + 63) // 64 * 64
    q, k, v, d_o = _inputs(M, nq, nkv, smax, seed=5)
    a = _run_varlen(ops, q, k, v, d_o, lens, nq, nkv, smax)
    lo, hi = cu_h[2], cu_h[3]
    q2, k2, v2, d2 = q.clone(), k.clone(), v.clone(), d_o.clone()
    q2[lo:hi] = rnd(hi - lo, nq * HD, seed=91) * 3
    k2[:, :, lo:hi] = rnd(1, nkv, hi - lo, HD, seed=92) * 3
    v2[:, :, lo:hi] = rnd(1, nkv, hi - lo, HD, seed=93) * 3
    d2[lo:hi] = rnd(hi - lo, nq * HD, seed=94) * 3
    b = _run_varlen(ops, q2, k2, v2, d2, lens, nq, nkv, smax)
    keep = torch.ones(M, dtype=torch.bool, device='cuda'); keep[lo:hi] = False
    for nm in ('out', 'dq', 'dk', 'dv'):
        assert torch.equal(a[nm][:M][keep], b[nm][:M][keep]), nm
        assert not torch.equal(a[nm][lo:hi], b[nm][lo:hi]), f'{nm}: sequence 2 did not change'
    for nm in ('lse', 'delta'):
        assert torch.equal(a[nm][:nq * M].view(nq, M)[:, keep], b[nm][:nq * M].view(nq, M)[:, keep]), nm


def test_bad_varlen_arguments_are_refused_before_any_launch(ops):
    """cu_seqlens not ascending (host copy), more rows than cache slots, head_dim != 128: an error, never a launch."""
    from vlaser_amd import _lib as L
    nq, nkv, smax, M = 12, 2, 128, 100
    q, k, v, d_o = _inputs(M, nq, nkv, smax)
    vt = v.transpose(-1, -2).contiguous()
    out = torch.zeros(smax, nq * HD, dtype=BF, device='cuda')
    lse = torch.zeros(nq * M, dtype=torch.float32, device='cuda')
    cu = torch.tensor([0, 60, 100], dtype=torch.int32, device='cuda')
    with pytest.raises(L.VlaserHipError, match='ascend'):
        ops.attn_varlen(q, k, vt, out, M, nq, nkv, HD, smax, 0.1, cu, lse_out=lse, cu_host=[0, 70, 60])
    with pytest.raises(L.VlaserHipError, match='ascend'):
        ops.attn_bwd_varlen(q, k, vt, out, d_o, lse, lse, out, out, out, M, nq, nkv, smax, 0.1, cu, cu_host=[0, 60, 99])
    with pytest.raises(L.VlaserHipError, match='exceed the cache'):
        ops.attn_varlen(q, k, vt, out, 200, nq, nkv, HD, smax, 0.1, cu, lse_out=lse)
    with pytest.raises(L.VlaserHipError, match='exceed the cache'):
        ops.attn_bwd_varlen(q, k, vt, out, d_o, lse, lse, out, out, out, 200, nq, nkv, smax, 0.1, cu)
    with pytest.raises(L.VlaserHipError, match='head_dim 64'):
        ops.attn_varlen(q, k, vt, out, M, nq * 2, nkv * 2, 64, smax, 0.1, cu, lse_out=lse)
    with pytest.raises(L.VlaserHipError, match='head_dim 64'):
        ops.attn_bwd_varlen(q, k, vt, out, d_o, lse, lse, out, out, out, M, nq, nkv, smax, 0.1, cu, head_dim=64)
    with pytest.raises(L.VlaserHipError, match='int32'):
        ops.attn_varlen(q, k, vt, out, M, nq, nkv, HD, smax, 0.1, cu.long(), lse_out=lse)
