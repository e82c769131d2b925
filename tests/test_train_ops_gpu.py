"""Op-level parity of the training-side kernels (backward, gradient bookkeeping) against fp64 references computed on the CPU from the same inputs
the kernel reads (GPU box only).

Error criteria are derived from the arithmetic of each kernel, element by element (a max-normalised figure lets an outright wrong small element
through):
  element-wise ops     |got - ref| <= k 2^-7 |ref| + FLOOR          (k = 1 bf16 ulp; 2 where the kernel uses __expf / erf)
  reductions           |got - ref| <= [2^-7 |ref|] + 2^-24 n_seq ref_abs + FLOOR
                       ([..] only for a bf16 output; ref_abs = the same expression on the absolute values of the terms; n_seq = the longest chain
                       of sequential fp32 additions in the kernel, stated next to each bound)
  permutations, casts  bit for bit on view(torch.int16)
Every bounded figure is the worst element of |got - ref| / tol (<= 1 passes), logged through tests/parity.py.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bounds import BF, D64, FLOOR, SENT, U, ULP, _ln_rows, bits, bound, elementwise, h64, reduction, sentinel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vlaser_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def _grad_on():
    """the references use autograd; other modules' fixtures switch grad off for the whole session"""
    with torch.enable_grad():
        yield


def rnd(*shape, std=1.0, seed=0, dtype=BF):
    g = torch.Generator(device='cpu').manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * std).to(dtype).cuda()


# ------------------------------------------------------------------------------------------------ 1. LayerNorm backward (+ forward, colsum_mul mode 3)
def _ln_stats(x, eps):
    mean = x.mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    return mean, rs


@pytest.mark.parametrize('C', [1024, 4096, 520, 8])
@pytest.mark.parametrize('S', [1, 3, 256, 1025])
def test_layernorm_bwd(ops, S, C):
    """Guards the one-pass variance: E[x^2] - mean^2 is 0 in fp32 on near-constant rows (rs = 1/sqrt(eps) instead of the true rs that the
    forward and the weight gradient use on the same row); layernorm_bwd_kernel now computes the variance in two passes."""
    w, b = rnd(C, std=0.5, seed=1) + 1.0, rnd(C, std=0.2, seed=2)
    h_w, h_b = h64(w), h64(b)
    n_row = 8 * ((C + 511) // 512) + 6        # one wave per row: 8 adds per 16-byte chunk of a lane, then the 6-level butterfly
    for ki, kind in enumerate(['normal', 'offset', 'outlier', 'flat']):
        for dres_on, eps in [(False, 1e-6), (True, 1e-5)]:
            tag = f'ln_bwd[{kind},S={S},C={C},dres={int(dres_on)},eps={eps:g}]'
            x = _ln_rows(kind, S, C, seed=10 * ki + S + C).cuda()
            dy = rnd(S, C, seed=3 + ki)
            dres = rnd(S, C, std=0.3, seed=5 + ki) if dres_on else None
            dx = sentinel(S, C)
            ops.layernorm_bwd(dy, x, w, dres, dx, S, C, eps)
            hx, hdy = h64(x).requires_grad_(True), h64(dy)
            y = F.layer_norm(hx, (C,), h_w, h_b, eps)
            (gx,) = torch.autograd.grad(y, hx, hdy)
            ref = gx + (h64(dres) if dres_on else 0.0)
            # ref_abs: rs (|g| + mean|g| + |xh| mean|g xh|) (+ |dres|) for the sums sg, sgx of g = w dy and the statistics, plus the shift of xh by
            # the fp32 error of the mean (<= n_row u mean|x|): rs (mean|x| rs) (mean|g xh| + |xh| mean|g|); the tail adds ~8 rounded operations
            hx = hx.detach()
            mean, rs = _ln_stats(hx, eps)
            xh, g = (hx - mean) * rs, (hdy * h_w).abs()
            mg, mgx = g.mean(-1, keepdim=True), (g * xh.abs()).mean(-1, keepdim=True)
            ref_abs = rs * (g + mg + xh.abs() * mgx) + rs * (hx.abs().mean(-1, keepdim=True) * rs) * (mgx + xh.abs() * mg)
            if dres_on:
                ref_abs = ref_abs + h64(dres).abs()
            # n_seq: n_row for sg / sgx, up to 1.5 n_row + 9 again through rs (dx has rs and rs^3 terms; rs carries n_row / 2 + 3), the tail ~8
            reduction(tag, dx, ref, ref_abs, 3 * n_row + 17)
            # the forward and the LN-weight gradient (colsum_mul mode 3) on the same rows: both two-pass
            yk = ops.layernorm(x, w, b, eps, out=sentinel(S, C))
            fwd_abs = (xh.abs() + hx.abs().mean(-1, keepdim=True) * rs) * h_w.abs()       # (x - mean) rs w: the mean's error shifts xh
            reduction(tag.replace('ln_bwd', 'ln_fwd'), yk, y.detach(), fwd_abs, n_row + 8)
            out = torch.full((C,), SENT, dtype=torch.float32, device='cuda')
            ws = torch.empty(2 * S + 16 * C, dtype=torch.float32, device='cuda')
            ops.colsum_mul(dy, x, out, S, C, mode=3, eps=eps, ws=ws)
            cref = (hdy * xh).sum(0)
            cabs = (hdy.abs() * (xh.abs() + hx.abs().mean(-1, keepdim=True) * rs)).sum(0)
            # rowstat_kernel: <= 64 adds per lane + 6 (registers hold C <= 4096); colsum: ceil(ceil(S/16)/4) per row lane + 4 + the 16 slices
            n_cs = 70 + 8 * ((C + 511) // 512) + (S + 63) // 64 + 20
            reduction(tag.replace('ln_bwd', 'colsum_mul3'), out, cref, cabs, n_cs, bf16_out=False)


# ------------------------------------------------------------------------------------------------ 2. attention backward of the expert rows
def _rows_ref(q, K, VT, dO, O, R, n_q, n_kv, valid_len, blk_start, first_tok_self, scale):
    """fp64 closed form of attn_rows_bwd + the error bounds (absolute, fp32 part) that the kernel's arithmetic allows"""
    G, kv_len = n_q // n_kv, blk_start + R
    qh = h64(q).view(R, n_q, 128).transpose(0, 1)                     # [n_q, R, 128]
    Kh = h64(K)[:, :kv_len].repeat_interleave(G, 0)                   # [n_q, kv, 128]
    Vh = h64(VT)[:, :, :kv_len].transpose(1, 2).repeat_interleave(G, 0)
    dOh, Oh = h64(dO).view(R, n_q, 128).transpose(0, 1), h64(O).view(R, n_q, 128).transpose(0, 1)
    j = torch.arange(kv_len)
    vis = ((j < valid_len) | (j >= blk_start))[None].repeat(R, 1)
    if first_tok_self:
        vis[0, blk_start + 1:] = False
    s = scale * qh @ Kh.transpose(1, 2)
    s_abs = scale * qh.abs() @ Kh.abs().transpose(1, 2)
    sm = s.masked_fill(~vis, -math.inf)
    mx = sm.amax(-1, keepdim=True)
    P = torch.softmax(sm, -1)
    dP, dP_abs = dOh @ Vh.transpose(1, 2), dOh.abs() @ Vh.abs().transpose(1, 2)
    Dv, D_abs = (dOh * Oh).sum(-1, keepdim=True), (dOh * Oh).abs().sum(-1, keepdim=True)
    dS = P * (dP - Dv) * scale
    # p = exp(s - mx) / sum: s carries 128 sequential adds (e_s = 128 u s_abs), exp / the subtraction of mx a few u (x |s - mx|);
    # the normaliser (ceil(kv/256) per thread + 6 + 3 adds) the worst term's error again
    n_sum = (kv_len + 255) // 256 + 9
    e = U * (128 * s_abs + 2 * (sm - mx).abs().nan_to_num(0.0, posinf=0.0) + 4)
    e = torch.where(vis, e, torch.zeros_like(e))
    relP = e + e.amax(-1, keepdim=True) + U * (n_sum + 2)
    errP = relP * P
    # dS = p (dP - D) scale: dP 128 sequential adds, D a block sum of 128 products (6 + 3 adds)
    errS = relP * dS.abs() + U * 130 * P * (dP_abs + D_abs) * scale
    dq = dS @ Kh
    # dQ: two halves of kv_len / 2 sequential adds each, then one add
    dq_tol = ULP * dq.abs() + U * (kv_len // 2 + 2) * (dS.abs() @ Kh.abs()) + errS @ Kh.abs() + FLOOR
    # block keys: sum over the G heads x R rows of a kv group (G R sequential adds)
    dSb, Pb, errSb, errPb = dS[:, :, blk_start:], P[:, :, blk_start:], errS[:, :, blk_start:], errP[:, :, blk_start:]
    grp = lambda t: t.view(n_kv, G, *t.shape[1:])
    dk = torch.einsum('kgrj,kgrd->jkd', grp(dSb), grp(qh))
    dv = torch.einsum('kgrj,kgrd->jkd', grp(Pb), grp(dOh))
    dk_tol = ULP * dk.abs() + U * (G * R + 1) * torch.einsum('kgrj,kgrd->jkd', grp(dSb.abs()), grp(qh.abs())) + \
        torch.einsum('kgrj,kgrd->jkd', grp(errSb), grp(qh.abs())) + FLOOR
    dv_tol = ULP * dv.abs() + U * (G * R + 1) * torch.einsum('kgrj,kgrd->jkd', grp(Pb), grp(dOh.abs())) + \
        torch.einsum('kgrj,kgrd->jkd', grp(errPb), grp(dOh.abs())) + FLOOR
    return dict(P=P, dS=dS, vis=vis, errP=errP, errS=errS, dq=dq.transpose(0, 1).reshape(R, n_q * 128),
                dq_tol=dq_tol.transpose(0, 1).reshape(R, n_q * 128), dk=dk.reshape(R, n_kv * 128), dk_tol=dk_tol.reshape(R, n_kv * 128),
                dv=dv.reshape(R, n_kv * 128), dv_tol=dv_tol.reshape(R, n_kv * 128))


def _rows_inputs(R, n_q, n_kv, s_max, seed):
    q, dO, O = rnd(R, n_q * 128, seed=seed), rnd(R, n_q * 128, seed=seed + 1), rnd(R, n_q * 128, std=0.5, seed=seed + 2)
    K, VT = rnd(n_kv, s_max, 128, seed=seed + 3), rnd(n_kv, 128, s_max, seed=seed + 4)
    return q, K, VT, dO, O


@pytest.mark.parametrize('first_tok_self', [True, False])
@pytest.mark.parametrize('blk', ['384/448', '2048-R/2048'])
@pytest.mark.parametrize('vl', ['1', '277', 'blk_start'])
@pytest.mark.parametrize('R', [1, 4, 5, 16])
def test_attn_rows_bwd(ops, R, vl, blk, first_tok_self):
    """Every key tile, the first_tok_self row and the block keys' dK / dV against fp64; the second pairing fills the 2048-key LDS row exactly."""
    n_q, n_kv, scale = 12, 2, 1.0 / math.sqrt(128)
    blk_start, s_max = (384, 448) if blk == '384/448' else (2048 - R, 2048)
    valid_len = {'1': 1, '277': 277, 'blk_start': blk_start}[vl]
    kv_len = blk_start + R
    q, K, VT, dO, O = _rows_inputs(R, n_q, n_kv, s_max, seed=R + valid_len)
    ref = _rows_ref(q, K, VT, dO, O, R, n_q, n_kv, valid_len, blk_start, first_tok_self, scale)
    tag = f'rows_bwd[R={R},vl={valid_len},blk={blk_start}/{s_max},fts={int(first_tok_self)}]'
    outs = []
    for ex in (False, True, True):
        dq, dk, dv = sentinel(R, n_q * 128), sentinel(R, n_kv * 128), sentinel(R, n_kv * 128)
        p_out = ds_out = None
        if ex:
            p_out, ds_out = sentinel(n_q, 16, s_max), sentinel(n_q, 16, s_max)
        ops.attn_rows_bwd(q, K, VT, dO, O, dq, dk, dv, R, n_q, n_kv, s_max, valid_len, blk_start, first_tok_self, scale, p_out=p_out, ds_out=ds_out)
        outs.append((dq, dk, dv, p_out, ds_out))
    dq, dk, dv, p_out, ds_out = outs[1]
    bound(tag + '.dq', dq, ref['dq'], ref['dq_tol'])
    bound(tag + '.dk', dk, ref['dk'], ref['dk_tol'])
    bound(tag + '.dv', dv, ref['dv'], ref['dv_tol'])
    # P / dS of every key j < kv_len (rows R..15 and keys >= kv_len stay at the sentinel); invisible keys exactly 0
    p, ds = h64(p_out), h64(ds_out)
    bound(tag + '.P', p[:, :R, :kv_len], ref['P'], ULP * ref['P'] + ref['errP'] + FLOOR)
    bound(tag + '.dS', ds[:, :R, :kv_len], ref['dS'], ULP * ref['dS'].abs() + ref['errS'] + FLOOR)
    hidden = ~ref['vis'][None].expand(n_q, R, kv_len)
    assert (p[:, :R, :kv_len][hidden] == 0).all() and (ds[:, :R, :kv_len][hidden] == 0).all(), 'P / dS of an invisible key not 0'
    assert (p[:, R:] == SENT).all() and (ds[:, R:] == SENT).all(), 'rows R..15 of p_out / ds_out written'
    assert (p[:, :, kv_len:] == SENT).all() and (ds[:, :, kv_len:] == SENT).all(), 'keys >= kv_len of p_out / ds_out written'
    # deterministic, and p_out / ds_out do not change dq / dk / dv
    for a, b in zip(outs[1], outs[2]):
        assert torch.equal(bits(a), bits(b)), 'two runs differ'
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(bits(a), bits(b)), 'attn_rows_bwd and attn_rows_bwd_ex differ'


def test_attn_rows_closed_form_is_autograd():
    """The closed form above (D = <dO, O>) is the gradient of the masked softmax attention when O is its exact forward output."""
    R, n_q, n_kv, s_max, valid_len, blk_start, scale = 5, 4, 2, 64, 21, 40, 1.0 / math.sqrt(128)
    g = torch.Generator().manual_seed(7)
    q, K, V, dO = (torch.randn(*s, generator=g, dtype=D64) for s in [(R, n_q, 128), (n_kv, s_max, 128), (n_kv, s_max, 128), (R, n_q, 128)])
    G, kv_len = n_q // n_kv, blk_start + R
    q.requires_grad_(True); K.requires_grad_(True); V.requires_grad_(True)
    j = torch.arange(kv_len)
    vis = ((j < valid_len) | (j >= blk_start))[None].repeat(R, 1)
    vis[0, blk_start + 1:] = False
    s = scale * torch.einsum('rhd,hjd->hrj', q, K[:, :kv_len].repeat_interleave(G, 0))
    O = torch.einsum('hrj,hjd->rhd', torch.softmax(s.masked_fill(~vis, -math.inf), -1), V[:, :kv_len].repeat_interleave(G, 0))
    gq, gK, gV = torch.autograd.grad(O, (q, K, V), dO)
    VT = V.detach().transpose(1, 2)
    to = lambda t: t.detach().reshape(R, n_q * 128)
    ref = _rows_ref(to(q), K.detach(), VT, to(dO), to(O), R, n_q, n_kv, valid_len, blk_start, True, scale)
    assert torch.allclose(ref['dq'], to(gq), rtol=1e-10, atol=1e-12)
    assert torch.allclose(ref['dk'], gK[:, blk_start:kv_len].transpose(0, 1).reshape(R, n_kv * 128), rtol=1e-10, atol=1e-12)
    assert torch.allclose(ref['dv'], gV[:, blk_start:kv_len].transpose(0, 1).reshape(R, n_kv * 128), rtol=1e-10, atol=1e-12)
    assert (gK[:, valid_len:blk_start] == 0).all()


# ------------------------------------------------------------------------------------------------ 3. inverse RoPE + packing
def _rope64(x, cos, sin, pos):
    # x [S, heads, 128]; the kernel's own fp32 table, read in fp64
    c, s = h64(cos)[pos], h64(sin)[pos]
    c, s = torch.cat([c, c], -1)[:, None], torch.cat([s, s], -1)[:, None]
    return x * c + torch.cat([-x[..., 64:], x[..., :64]], -1) * s


@pytest.mark.parametrize('heads', ['12/2', '28/4'])
@pytest.mark.parametrize('S', [1, 5, 389])
@pytest.mark.parametrize('kv_per_q_head', [False, True])
@pytest.mark.parametrize('extra', [False, True])
def test_rope_bwd_pack(ops, heads, S, kv_per_q_head, extra):
    """Gradient w.r.t. the packed pre-RoPE q/k/v columns: autograd through natural order -> RoPE -> ops.head_perm packing."""
    n_q, n_kv = map(int, heads.split('/'))
    G, nh, n_pos = n_q // n_kv, n_q + 2 * n_kv, 4096
    cos, sin = ops.rope_table(n_pos)
    g = torch.Generator().manual_seed(S + n_q)
    pos = torch.randint(0, n_pos, (S,), generator=g)
    pos[-1] = n_pos - 1                                              # the last row of the table
    pos_d = pos.to(torch.int32).cuda()
    kvw = n_q if kv_per_q_head else n_kv
    dq, dk, dv = rnd(S, n_q * 128, seed=1), rnd(S, kvw * 128, seed=2), rnd(S, kvw * 128, seed=3)
    dk_x, dv_x = (rnd(S, n_kv * 128, seed=4), rnd(S, n_kv * 128, seed=5)) if extra else (None, None)
    out = sentinel(S, nh * 128)
    ops.rope_bwd_pack_ex(dq, dk, dv, cos, sin, pos_d, out, S, n_q, n_kv, kv_per_q_head=kv_per_q_head, dk_extra=dk_x, dv_extra=dv_x)
    # reference: packed column (h, p) = natural column (h, head_perm[p])
    packed = torch.zeros(S, nh * 128, dtype=D64, requires_grad=True)
    idx = (torch.arange(nh)[:, None] * 128 + ops.head_perm()[None, :]).reshape(-1)
    nat = torch.zeros(S, nh * 128, dtype=D64).index_add(1, idx, packed).view(S, nh, 128)
    qn, kn, vn = nat[:, :n_q], nat[:, n_q:n_q + n_kv], nat[:, n_q + n_kv:]
    qr, kr = _rope64(qn, cos, sin, pos), _rope64(kn, cos, sin, pos)
    rep = (lambda t: t.repeat_interleave(G, 1)) if kv_per_q_head else (lambda t: t)
    loss = (h64(dq).view(S, n_q, 128) * qr).sum() + (h64(dk).view(S, kvw, 128) * rep(kr)).sum() + (h64(dv).view(S, kvw, 128) * rep(vn)).sum()
    if extra:
        loss = loss + (h64(dk_x).view(S, n_kv, 128) * kr).sum() + (h64(dv_x).view(S, n_kv, 128) * vn).sum()
    (ref,) = torch.autograd.grad(loss, packed)
    # ref_abs: the same gradient from |inputs| and |cos|, |sin|; n_seq: G partials (+ the extra) summed, then g1 c + g2 s
    a_dq, a_dk, a_dv = h64(dq).abs().view(S, n_q, 128), h64(dk).abs().view(S, kvw, 128), h64(dv).abs().view(S, kvw, 128)
    sumg = (lambda t: t.view(S, n_kv, G, 128).sum(2)) if kv_per_q_head else (lambda t: t)
    gk, gv = sumg(a_dk), sumg(a_dv)
    if extra:
        gk, gv = gk + h64(dk_x).abs().view(S, n_kv, 128), gv + h64(dv_x).abs().view(S, n_kv, 128)
    c, s = h64(cos)[pos].abs(), h64(sin)[pos].abs()
    rot_abs = lambda t: torch.cat([t[..., :64] * c[:, None] + t[..., 64:] * s[:, None], t[..., 64:] * c[:, None] + t[..., :64] * s[:, None]], -1)
    nat_abs = torch.cat([rot_abs(a_dq), rot_abs(gk), gv], 1).reshape(S, nh * 128)
    ref_abs = nat_abs[:, idx]
    tag = f'rope_bwd_pack[{heads},S={S},kvq={int(kv_per_q_head)},extra={int(extra)}]'
    reduction(tag, out, ref, ref_abs, (G if kv_per_q_head else 1) + 3)
    if not extra:       # the plain entry point is the _ex one without the extra gradients
        out2 = sentinel(S, nh * 128)
        ops.rope_bwd_pack(dq, dk, dv, cos, sin, pos_d, out2, S, n_q, n_kv, kv_per_q_head=kv_per_q_head)
        assert torch.equal(bits(out), bits(out2))


# ------------------------------------------------------------------------------------------------ 4. softmax + dS through materialised scores
@pytest.mark.parametrize('case', [
    # name, H, hd, S, ld, causal, kv_valid, q_off
    ('short,bidir,kv_valid<ld', 12, 128, 300, 320, 0, 277, 0),
    ('short,causal,q_off', 12, 128, 100, 512, 1, 512, 450),
    ('long,ViT', 16, 64, 1025, 1088, 0, 1025, 0),
    ('long,causal,q_off,kv_valid<ld', 4, 128, 64, 1536, 1, 1500, 1400),
], ids=lambda c: c[0])
def test_attn_bwd_pds_masked(ops, case):
    name, H, hd, S, ld, causal, kv_valid, q_off = case
    scale = 1.0 / math.sqrt(hd)
    g = torch.Generator().manual_seed(S + ld)
    scores = (torch.randn(H, S, ld, generator=g) * 3).cuda()
    dP = torch.randn(H, S, ld, generator=g).cuda()
    dO, O = rnd(S, H * hd, seed=1), rnd(S, H * hd, std=0.5, seed=2)
    n = H * S * ld
    Pbuf, dSbuf = sentinel(n + 64), sentinel(n + 64)
    P, dS = Pbuf[:n].view(H, S, ld), dSbuf[:n].view(H, S, ld)
    ops.attn_bwd_pds_masked(scores, dP, dO, O, P, dS, H, S, ld, hd, scale, causal, kv_valid, q_off)
    k, qq = torch.arange(ld)[None], torch.arange(S)[:, None]
    vis = (k < kv_valid) & ((k <= qq + q_off) if causal else torch.ones(S, 1, dtype=torch.bool))
    vis = vis[None].expand(H, S, ld)
    x = (h64(scores) * scale).masked_fill(~vis, -math.inf)
    Pr = torch.softmax(x, -1)
    dOh, Oh = h64(dO).view(S, H, hd).transpose(0, 1), h64(O).view(S, H, hd).transpose(0, 1)
    Dv, D_abs = (dOh * Oh).sum(-1, keepdim=True), (dOh * Oh).abs().sum(-1, keepdim=True)
    dPh = h64(dP)
    dSr = Pr * (dPh - Dv) * scale
    # p: scale * s and the subtraction of the max rounded (u |x|, u |x - mx|), __expf, the normaliser (<= 16 per lane or ceil(kv/64), + 6)
    n_sum = max(16, (kv_valid + 63) // 64) + 6
    mx = x.amax(-1, keepdim=True)
    e = torch.where(vis, U * (2 * x.abs() + 2 * (x - mx).abs() + 4), torch.zeros_like(x)).nan_to_num(0.0)
    relP = e + e.amax(-1, keepdim=True) + U * (n_sum + 2)
    tag = f'pds_masked[{name}]'
    bound(tag + '.P', P, Pr, 2 * ULP * Pr + relP * Pr + FLOOR)
    # dS = bf16(P) (dP - D) scale: the stored P's rounding (2^-8) on top; D = 2 ceil(hd/128) adds per lane + 6
    n_d = 2 * ((hd + 127) // 128) + 6
    bound(tag + '.dS', dS, dSr, ULP * dSr.abs() + (2.0 ** -8 + relP + 3 * U) * dSr.abs() + U * (n_d + 2) * Pr * (dPh.abs() + D_abs) * scale + FLOOR)
    pk, dk = h64(P), h64(dS)
    assert (pk[~vis] == 0).all() and (dk[~vis] == 0).all(), 'P / dS not exactly 0 on a masked column'
    assert (h64(Pbuf[n:]) == SENT).all() and (h64(dSbuf[n:]) == SENT).all(), 'written past [H, S, ld]'


# ------------------------------------------------------------------------------------------------ 5. pixel_unshuffle
@pytest.mark.parametrize('ps_v1', [0, 1])
@pytest.mark.parametrize('T', [1, 3])
def test_pixel_unshuffle(ops, T, ps_v1):
    from oracle import vit as ovit
    G, C = 32, 1024
    x = rnd(T, G * G + 1, C, seed=T)
    sh = sentinel(T * (G // 2) ** 2, 4 * C)
    ops.pixel_shuffle(x, sh, T, G, C, ps_v1)
    dx = sentinel(T, G * G + 1, C)
    ops.pixel_unshuffle(sh, dx, T, G, C, ps_v1)
    want = x.clone()
    want[:, 0] = 0
    assert torch.equal(bits(dx), bits(want)), 'pixel_unshuffle is not the inverse of pixel_shuffle'
    assert (bits(dx[:, 0]) == 0).all(), 'CLS row not +0'
    # against autograd of the oracle's permutation (extract_feature drops CLS first)
    dout = rnd(T * (G // 2) ** 2, 4 * C, seed=9)
    dx2 = sentinel(T, G * G + 1, C)
    ops.pixel_unshuffle(dout, dx2, T, G, C, ps_v1)
    xin = torch.zeros(T, G * G + 1, C, dtype=D64, requires_grad=True)
    y = ovit.pixel_shuffle(xin[:, 1:].reshape(T, G, G, C), ps_version='v1' if ps_v1 else 'v2')
    (gref,) = torch.autograd.grad(y.reshape(-1, 4 * C), xin, h64(dout))
    assert torch.equal(bits(dx2), bits(gref.to(BF))), 'pixel_unshuffle != autograd of oracle.vit.pixel_shuffle'


# ------------------------------------------------------------------------------------------------ 6. element-wise ops, scaling, casts
def _all_finite_bf16():
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF)
    x = x[torch.isfinite(x.float())]                                  # 65 280 = 255 x 256 patterns ...
    return torch.cat([x, x[:77]])                                     # ... made not a multiple of 256


def test_gelu_silu_all_bf16(ops):
    """gelu_bwd guards Phi(v) for v < -5: 0.5 (1 + erf(v / sqrt2)) cancels to 0 there (3 % off at v = -5.5625); the kernel uses erfc."""
    x = _all_finite_bf16().cuda()
    n = x.numel()
    assert n % 256 != 0
    dy = rnd(n, seed=1)
    xd, dyd = h64(x), h64(dy)
    phi = 0.5 * torch.special.erfc(-xd / math.sqrt(2))
    pdf = torch.exp(-0.5 * xd * xd) / math.sqrt(2 * math.pi)
    sig = torch.sigmoid(xd)
    refs = {'gelu_bwd': dyd * (phi + xd * pdf), 'silu': xd * sig,
            'silu_bwd': dyd * sig * (1 + xd * (1 - sig))}
    for name, ref in refs.items():
        out = sentinel(n)
        if name == 'gelu_bwd':
            ops.gelu_bwd(x, dy, out)
        elif name == 'silu':
            ops.silu(x, out)
        else:
            ops.silu_bwd(x, dy, out)
        elementwise(f'{name}[all finite bf16]', out, ref, ulps=2)        # __expf / erfc: two ulps


@pytest.mark.parametrize('vec', [True, False])
def test_scale_cols(ops, vec):
    S, C, ldx, ldo = 37, 520, 1040, 528
    base = rnd(S, ldx, seed=1)
    x = base[:, :C]
    v = rnd(C, std=0.5, seed=2) if vec else None
    for alpha in (1.0, 0.125, -0.3):
        obuf = sentinel(S, ldo)
        ops.scale_cols(x, v, obuf, S, C, alpha=alpha, ldx=ldx, ldo=ldo)
        ref = h64(x) * (h64(v) if vec else 1.0) * float(torch.tensor(alpha, dtype=torch.float32))
        elementwise(f'scale_cols[vec={int(vec)},alpha={alpha}]', obuf[:, :C], ref)      # two fp32 products, one bf16 rounding
        assert (h64(obuf[:, C:]) == SENT).all(), 'scale_cols wrote past C'
    if not vec:
        obuf = sentinel(S, ldo)
        ops.scale_cols(x, None, obuf, S, C, alpha=1.0, ldx=ldx, ldo=ldo)
        assert torch.equal(bits(obuf[:, :C]), bits(x)), 'alpha = 1, vec = None is not the identity'
    # in place on the strided rows
    y = base.clone()
    ops.scale_cols(y[:, :C], v, y, S, C, alpha=0.5, ldx=ldx, ldo=ldx)
    ref = h64(x) * (h64(v) if vec else 1.0) * 0.5
    elementwise(f'scale_cols_inplace[vec={int(vec)}]', y[:, :C], ref)
    assert torch.equal(bits(y[:, C:]), bits(base[:, C:]))


def test_cast_f32_bf16(ops):
    """Round-to-nearest-even ties, denormals, +-Inf and NaN == tensor.to(torch.bfloat16)."""
    ties = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x7F7F8000, 0x7F7FFFFF, 0xFF7FFFFF,
                         0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80000001, 0x807FFFFF, 0x00800000, 0x7F800000, 0xFF800000,
                     0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0x00000000, 0x80000000], dtype=np.uint32)
    rand_bits = np.random.default_rng(3).integers(0, 2 ** 32, 100_003, dtype=np.uint32)
    x = torch.from_numpy(np.concatenate([ties, rand_bits]).view(np.float32).copy())
    y = sentinel(x.numel() + 8)
    ops.cast_f32_bf16(x.cuda(), y[:x.numel()])
    ref = x.to(BF)
    nan = torch.isnan(x)
    got = y[:x.numel()].cpu()
    assert torch.equal(bits(got)[~nan], bits(ref)[~nan]), 'cast differs from tensor.to(bfloat16)'
    assert torch.isnan(got.float()[nan]).all(), 'NaN not kept NaN'
    assert (h64(y[x.numel():]) == SENT).all()


# ------------------------------------------------------------------------------------------------ 7. cross-entropy backward
@pytest.mark.parametrize('V', [7, 1001, 151674])
def test_ce_dlogits(ops, V):
    R, scale, ignore = 6, 0.37, -100
    ld_in, ld_out = V + 3, V + (8 - V % 8) + 8                       # ld_out > V: the pad must be 0
    g = torch.Generator().manual_seed(V)
    lbuf = (torch.randn(R, ld_in, generator=g) * 4).cuda()
    logits = lbuf[:, :V]
    labels = torch.randint(0, V, (R,), generator=g)
    labels[2] = ignore
    labels[4] = V - 1
    labels = labels.cuda()
    loss_r, lse = torch.empty(R, dtype=torch.float32, device='cuda'), torch.empty(R, dtype=torch.float32, device='cuda')
    ops.ce_rows(logits, labels, loss_r, lse, ignore_index=ignore)
    out = sentinel(R, ld_out)
    ops.ce_dlogits(logits, lse, labels, out, scale, ignore_index=ignore)
    hl = h64(logits).requires_grad_(True)
    loss = float(torch.tensor(scale, dtype=torch.float32)) * F.cross_entropy(hl, labels.cpu(), reduction='sum', ignore_index=ignore)
    (ref,) = torch.autograd.grad(loss, hl)
    # the kernel reads ce_rows' fp32 lse: lse = mx + log(sum exp(l - mx)), sum of <= 2 ceil(V / 2048) + 2 adds per thread, + 6 + 16;
    # each term's exp carries u |l - mx| + a few u; then the log and the add of mx (u |lse|)
    hl = hl.detach()
    lse64 = torch.logsumexp(hl, -1, keepdim=True)
    n_lse = 2 * ((V + 2047) // 2048) + 2 + 22
    mx = hl.amax(-1, keepdim=True)
    e_lse = U * (n_lse + 2 * (mx - hl.amin(-1, keepdim=True)) + 4 + 2 * (lse64.abs() + mx.abs() + math.log(V)))
    p = torch.exp(hl - lse64)
    tol = 2 * ULP * ref.abs() + abs(scale) * p * (e_lse + U * ((hl - lse64).abs() + 4)) + FLOOR
    bound(f'ce_dlogits[V={V}]', out[:, :V], ref, tol)
    assert (h64(out[2]) == 0).all(), 'ignore_index row not 0'
    assert (h64(out[:, V:]) == 0).all(), 'pad columns not 0'


# ------------------------------------------------------------------------------------------------ 8. gradient accumulation
def test_grad_accumulate(ops):
    n, off = 100_003, 4                         # n % 4 != 0: block 0's tail loop; g offset by 8 bytes, acc by 16
    gbuf, abuf = sentinel(n + 16), torch.full((n + 16,), SENT, dtype=torch.float32, device='cuda')
    g, acc = gbuf[off:off + n], abuf[off:off + n]
    ws = [float(torch.tensor(w, dtype=torch.float32)) for w in (1 / 3, 1 / 3, 1 / 3)]
    gs = [rnd(n, seed=i) for i in range(3)]
    ref, ref_abs = torch.zeros(n, dtype=D64), torch.zeros(n, dtype=D64)
    for i, (w, gi) in enumerate(zip(ws, gs)):
        g.copy_(gi)
        ops.grad_accumulate(g, acc, w, first=(i == 0), finalize=(i == 2))
        ref, ref_abs = ref + w * h64(gi), ref_abs + abs(w) * h64(gi).abs()
    # three rounded products and two rounded additions: within u (sum |w g|) + 2 u (sum |w g|) -- one fp32 ulp of the magnitude per step
    reduction('grad_accumulate.acc', acc, ref, ref_abs, 3, bf16_out=False)
    assert torch.equal(bits(g), bits(acc.to(BF))), 'finalize: g != bf16(acc)'
    assert (h64(gbuf[:off]) == SENT).all() and (h64(gbuf[off + n:]) == SENT).all() and (h64(abuf[:off]) == SENT).all() and (h64(abuf[off + n:]) == SENT).all()


# ------------------------------------------------------------------------------------------------ 9. sum of squares
@pytest.mark.parametrize('n', [1, 7, 8, 1_000_003, 2 ** 25 + 3])
def test_sumsq(ops, n):
    x = rnd(n, seed=5)
    out = torch.full((1,), 1.5, dtype=torch.float32, device='cuda')           # accumulates into a non-zero out
    ws = torch.empty(1024, dtype=torch.float32, device='cuda')
    ops.sumsq(x, out, ws)
    ref = 1.5 + (h64(x) ** 2).sum()
    # n_seq: the grid is one workgroup per CU (<= 1024): 8 ceil(n / 8 / (256 nb)) adds per thread, 1 for block 0's tail, 6 + 3 in the workgroup,
    # ceil(nb / 64) partials per lane of the final wave + 6, the add into out; + 1 for the squares
    from vlaser_amd import _lib as L
    nb = min(torch.cuda.get_device_properties(0).multi_processor_count, L.lib().vlaser_get_cu_budget(), 1024)
    n_seq = 8 * ((n // 8 + nb * 256 - 1) // (nb * 256)) + 1 + 9 + (nb + 63) // 64 + 6 + 1 + 1
    reduction(f'sumsq[n={n}]', out[0], ref, ref, n_seq, bf16_out=False)


# ------------------------------------------------------------------------------------------------ 10. column sums
@pytest.mark.parametrize('C', [768, 1536, 100])
def test_colsum_partials_multi(ops, C):
    S, n_t = 203, 3
    n_part = (S + 3) // 4
    slot = n_part * C + 64
    ws = torch.zeros(n_t * slot, dtype=torch.float32, device='cuda')
    offs = [5 * C + 3, 0, 2 * C + 1][:n_t]
    out_base = sentinel(7 * C)
    if C % 8 == 0:
        per_call = []
        for t in range(n_t):
            dy, x, w = rnd(S, C, seed=t), rnd(S, C, seed=t + 10), rnd(C, seed=t + 20)
            dx, dw = sentinel(S, C), sentinel(C)
            ops.rmsnorm_bwd(dy, x, w, None, dx, S, C, 1e-6, dw_out=dw, dw_ws=torch.empty(n_part * C, dtype=torch.float32, device='cuda'))
            per_call.append(dw)
            ops.rmsnorm_bwd(dy, x, w, None, dx, S, C, 1e-6, dw_ws=ws[t * slot:t * slot + n_part * C])
    else:   # rmsnorm_bwd needs C % 8 == 0: partials made here (the reduction itself has no such limit)
        for t in range(n_t):
            ws[t * slot:t * slot + n_part * C] = (rnd(n_part * C, seed=t, dtype=torch.float32))
        per_call = None
    out_off = torch.tensor(offs, dtype=torch.int64, device='cuda')
    ops.colsum_partials_multi(ws, slot, n_t, n_part, C, out_base, out_off)
    written = torch.zeros(7 * C, dtype=torch.bool)
    for t in range(n_t):
        got = out_base[offs[t]:offs[t] + C]
        part = h64(ws[t * slot:t * slot + n_part * C]).view(n_part, C)
        # 4 row slices x 4 accumulators: ceil(n_part / 16) sequential adds, <= 3 tail adds, then 2 + 2 levels
        reduction(f'colsum_partials_multi[C={C},t={t}]', got, part.sum(0), part.abs().sum(0), (n_part + 15) // 16 + 7)
        if per_call is not None:
            assert torch.equal(bits(got), bits(per_call[t])), 'colsum_partials_multi differs from the per-call reduction'
        written[offs[t]:offs[t] + C] = True
    assert (h64(out_base)[~written] == SENT).all(), 'colsum_partials_multi wrote outside its outputs'


@pytest.mark.parametrize('S,C', [(1, 8), (257, 100), (1025, 1024)])
@pytest.mark.parametrize('mode', [0, 1])
def test_colsum_mul_modes01(ops, S, C, mode):
    a, b = rnd(S, C, seed=1), rnd(S, C, seed=2)
    out = torch.full((C + 8,), SENT, dtype=torch.float32, device='cuda')
    ws = torch.empty(2 * S + 16 * C, dtype=torch.float32, device='cuda')
    ops.colsum_mul(a, b if mode else None, out[:C], S, C, mode=mode, ws=ws)
    t = h64(a) * (h64(b) if mode else 1.0)
    # ceil(ceil(S / 16) / 4) adds per row lane, 3 across the lanes, 16 across the slices (+ 1 for the product)
    reduction(f'colsum_mul[mode={mode},S={S},C={C}]', out[:C], t.sum(0), t.abs().sum(0), ((S + 15) // 16 + 3) // 4 + 3 + 16 + mode, bf16_out=False)
    assert (h64(out[C:]) == SENT).all()


# ------------------------------------------------------------------------------------------------ 11. small_linear
@pytest.mark.parametrize('M', [1, 4])
@pytest.mark.parametrize('N', [1, 300, 1024])
@pytest.mark.parametrize('K', [1, 7, 32])
def test_small_linear(ops, M, N, K):
    x = rnd(M, K, seed=1, dtype=torch.float32)
    w, b = rnd(N, K, std=0.3, seed=2), rnd(N, std=0.5, seed=3)
    obuf = sentinel(M * N + 16)
    ops.small_linear(x, w, b, obuf, M, N, K)
    xb = h64(x.to(BF))                       # the kernel rounds x to bf16 first (the reference module runs in bf16)
    ref = xb @ h64(w).t() + h64(b)
    ref_abs = xb.abs() @ h64(w).abs().t() + h64(b).abs()
    reduction(f'small_linear[M={M},N={N},K={K}]', obuf[:M * N].view(M, N), ref, ref_abs, K + 1)      # bias, then K sequential adds
    assert (h64(obuf[M * N:]) == SENT).all()


# ------------------------------------------------------------------------------------------------ 12. refusals before any launch
def test_refusals(ops):
    from vlaser_amd._lib import VlaserHipError
    n_q, n_kv, s_max = 12, 2, 2064
    q, K, VT, dO, O = _rows_inputs(17, n_q, n_kv, s_max, seed=0)
    ws = torch.zeros(4 * n_q * 256, dtype=torch.float32, device='cuda')       # room for R = 17 should a check be missing
    dq, dk, dv = sentinel(17, n_q * 128), sentinel(17, n_kv * 128), sentinel(17, n_kv * 128)
    torch.cuda.synchronize()
    for R, valid_len, blk_start in [(17, 100, 384), (9, 100, 2040), (4, 385, 384)]:      # R > 16; blk_start + R > 2048; valid_len > blk_start
        with pytest.raises(VlaserHipError, match='bad geometry'):
            ops.attn_rows_bwd(q, K, VT, dO, O, dq, dk, dv, R, n_q, n_kv, s_max, valid_len, blk_start, True, 0.1, ws=ws)
    x, w = rnd(4, 24), rnd(24)           # C = 20 in rows of 24: room should a check be missing
    dx = sentinel(4, 24)
    with pytest.raises(VlaserHipError, match='bad args'):
        ops.layernorm_bwd(x, x, w, None, dx, 4, 20, 1e-6)
    with pytest.raises(VlaserHipError, match='bad args'):
        ops.scale_cols(x[:, :20], None, dx, 4, 20, alpha=2.0, ldx=24, ldo=24)
    torch.cuda.synchronize()
    for t in (dq, dk, dv, dx):
        assert (h64(t) == SENT).all(), 'a refused call wrote its output'
    assert (h64(ws) == 0).all()
