"""Op-level parity of the forward kernels (GEMM epilogues, batched GEMM, prefill / skinny / chain attention, norm seams) against fp64 references
computed on the CPU from the very bf16 / fp32 tensors the kernel reads (GPU box only).

Conventions (as tests/test_train_ops_gpu.py):
  sentinels       every output buffer is larger than what the call may write (ldo = N + pad, 3 spare rows, spare rows between batch elements, spare
                  cache slots) and starts at SENT; everything outside the contract must still be SENT bit for bit
  dynamic range   operands carry exact power-of-two scales (A rows / W rows / V keys: 2^e, e cycling over -10 .. 2): an exact scaling scales the
                  kernel's own error with it, so the derived bound still holds and a wrong element of a small row cannot hide under the tensor's maximum
Error criteria, element by element (ULP = 2^-7: one bf16 ulp, i.e. two half-ulp roundings; U = 2^-24; FLOOR = 2^-100):
  GEMM, bf16 out       |got - ref| <= ULP |ref| + U n_seq ref_abs + FLOOR        ref_abs = the same product on absolute values
  GEMM, fp32 out/slabs |got - ref| <= U n_seq ref_abs + FLOOR
                       n_seq = K / 32 + 10: an MFMA 16x16x32 adds a 32-term dot product to the accumulator -- at most 8 sequential additions inside a lane's
                       k-group, 2 levels across the four groups -- then one accumulation per MFMA (K / 32 of them); + the epilogue's additions (<= K always)
  epilogues            the reference applies the kernel's documented rounding points (q / k / v rounded after the bias, gate and up before SiLU); a value that
                       was rounded on the way in may land on the neighbouring bf16 (its fp32 error crossing a tie): one bf16 ulp of that term per later step
  GELU                 |got - ref| <= ULP |ref| + 2^-21 |z| + FLOOR (z = the pre-activation): 0.5 z (1 + erf) cancels below z = -4.84, in torch's fp32
                       formula as in gelu_erf (Abramowitz-Stegun 7.1.26, |err| <= 1.5e-7 = 2^-22.7 on erf -> 2^-23.7 |z|, + the fp32 roundings of 1 + erf)
  attention out        |got - ref| <= ULP |ref| + ULP ref_abs + FLOOR, ref_abs = sum_j p_j |v_j| (P rounded to bf16 in the numerator, the denominator, the output)
  lse_out (base 2)     |got - ref| <= 2^-22 |ref| + 2^-20: v_log_f32 (1 ulp) of an fp32 sum of <= 2048 terms of v_exp_f32 (1 ulp), + the score's fp32 error
  norms                LayerNorm: ULP |ref| + U (n_row + 8) (|xh| + mean|x| rs) |w| (the criteria of test_train_ops_gpu.py); RMSNorm w * bf16(x rs): two half-ulp
                       roundings, ULP (1 + 2^-7) |ref| + U (n_row + 8) |ref|
  permutations, copies bit for bit on view(torch.int16)
Every bounded figure is the worst element of |got - ref| / tol (<= 1 passes), logged through tests/parity.py.
"""
import math

import pytest
import torch

from bounds import (BF, D64, F32, FLOOR, LN_KINDS, SENT, U, ULP, Worst, _ln_rows, bits, bound, dev, dev_off, f32s, h64, is_sent, pow2, randb, rbf, same_bits,
                    sentinel)

pytestmark = pytest.mark.gpu
LOG2E = 1.4426950408889634


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vlaser_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def _grad_off():
    with torch.no_grad():
        yield


# ------------------------------------------------------------------------------------------------ helpers
def gelu64(z):
    return 0.5 * z * torch.special.erfc(-z / math.sqrt(2))


# ================================================================================================ A. vlaser_gemm epilogues at the edges of epilogue_tile
# (tile height, tile width) of every force_bm; 0 = the heuristic, which takes the 64 x 64 LDS-DMA tile at these sizes
TILE = {0: (64, 64), 32: (32, 128), 64: (64, 128), 128: (128, 128), 1100: (128, 128), 1200: (128, 256), 1300: (256, 256), 1440: (144, 128), 1500: (64, 128),
        1900: (192, 256)}
EPIS = ('none', 'bias', 'gelu', 'gelu_aux', 'ls_res', 'res', 'res_inplace', 'f32')


def _obuf(rows, ld, dtype=BF, off=False):
    """sentinel buffer [rows, ld] (+ slack on both sides); off: the view starts one element past the aligned base"""
    flat = torch.full((rows * ld + 16,), SENT, dtype=dtype, device='cuda')
    o = 1 if off else 0
    return flat, flat[o:o + rows * ld].view(rows, ld), o


def _outside_clean(flat, view, o, M, N):
    n = view.numel()
    return is_sent(view[:M, N:]) and is_sent(view[M:]) and is_sent(flat[:o]) and is_sent(flat[o + n:])


def _epilogue_case(ops, L, worst, bm, M, N, K):
    a = randb(M, K, seed=1) * pow2(M)[:, None]
    w = randb(N, K, seed=2) * pow2(N)[:, None]
    bias = randb(N, seed=3) * pow2(N) * 2.0 ** -4
    ls = randb(N, seed=4, std=0.5)
    res = (randb(M, N, seed=5) * pow2(M)[:, None] * pow2(N)[None] * 8).to(BF).float()
    A64, W64, b64, l64, r64 = a.double(), w.double(), bias.double(), ls.double(), res.double()
    acc, acc_abs = A64 @ W64.t(), A64.abs() @ W64.abs().t()
    n = K // 32 + 10
    assert n <= K
    z, z_abs = acc + b64, acc_abs + b64.abs()
    lsr = r64 + l64 * z
    refs = {                                                                              # name: (ref, tol)
        'none': (acc, ULP * acc.abs() + U * n * acc_abs),
        'bias': (z, ULP * z.abs() + U * (n + 1) * z_abs),
        # gelu' <= 1.13: the pre-activation's fp32 error passes through at most that much amplified
        'gelu': (gelu64(z), ULP * gelu64(z).abs() + 2.0 ** -21 * z.abs() + 1.13 * U * (n + 1) * z_abs),
        'ls_res': (lsr, ULP * lsr.abs() + U * (n + 3) * (r64.abs() + l64.abs() * z_abs)),
        'res': (r64 + acc, ULP * (r64 + acc).abs() + U * (n + 1) * (r64.abs() + acc_abs)),
        'f32': (acc, U * n * acc_abs),
    }
    refs['gelu_aux'], refs['res_inplace'] = refs['gelu'], refs['res']
    code = {'none': L.EPI_NONE, 'bias': L.EPI_BIAS, 'gelu': L.EPI_BIAS_GELU, 'gelu_aux': L.EPI_BIAS_GELU, 'ls_res': L.EPI_BIAS_LS_RES, 'res': L.EPI_RES,
            'res_inplace': L.EPI_RES, 'f32': L.EPI_F32}
    a_d, w_d, res_d = dev(a), dev(w), dev(res)
    vec = {False: (dev(bias), dev(ls)), True: (dev_off(bias), dev_off(ls))}
    ld8 = (N + 7) // 8 * 8
    # rows through LDS (ldo % 8 == 0, LDS-DMA tiles), 8-byte fragment stores (ldo % 8 == 4), the per-fragment fallback (odd ldo; operands 2 bytes off)
    variants = [('lds', ld8, False), ('frag8', ld8 + 4, False)] + ([('odd', N + 1, False)] if N % 2 else []) + [('unal', ld8, True)]
    firsts = {}
    for epi in EPIS:
        ref, tol = refs[epi]
        first = first_aux = None
        for vname, ldo, off in variants:
            if off and epi in ('none', 'res_inplace'):        # nothing but `out` could be moved there, and `out` keeps its alignment
                continue
            where = f'bm={bm},M={M},N={N},K={K},{vname}'
            flat, out, o = _obuf(M + 3, ldo, F32 if epi == 'f32' else BF, off and epi == 'f32')
            kw = dict(N=N, force_bm=bm)
            if epi in ('bias', 'gelu', 'gelu_aux', 'ls_res'):
                kw['bias'] = vec[off][0]
            if epi == 'ls_res':
                kw['ls'] = vec[off][1]
            rflat = None
            if epi in ('ls_res', 'res'):
                rflat, rbuf, ro = _obuf(M + 3, ldo, BF, off)
                rbuf[:M, :N] = res_d
                rkeep = rflat.clone()
                kw['res'] = rbuf
            if epi == 'res_inplace':
                out[:M, :N] = res_d
                kw['res'] = out
            if epi == 'gelu_aux':
                ld_aux = ld8 + 4                                # % 4 == 0, 8-byte aligned rows: the contract
                aflat, aux, ao = _obuf(M + 3, ld_aux)
                kw.update(aux_out=aux, ld_aux=ld_aux)
            ops.gemm(code[epi], a_d, w_d, out=out, **kw)
            assert _outside_clean(flat, out, o, M, N), f'{epi} {where}: written outside [M, N]'
            if rflat is not None:
                assert same_bits(rflat, rkeep), f'{epi} {where}: res modified'
            got = out[:M, :N]
            if first is None:
                first = got.clone()
                worst.add(f'gemm.{epi}[bm={bm}]', got, ref, tol + FLOOR, where)
            else:
                assert same_bits(got, first), f'{epi} {where}: differs from the first store path'
            if epi == 'gelu_aux':
                assert _outside_clean(aflat, aux, ao, M, N), f'{epi} {where}: aux_out written outside [M, N]'
                if first_aux is None:
                    first_aux = aux[:M, :N].clone()
                    worst.add(f'gemm.gelu_aux.z[bm={bm}]', first_aux, refs['bias'][0], refs['bias'][1] + FLOOR, where)
                else:
                    assert same_bits(aux[:M, :N], first_aux), f'{epi} {where}: aux_out differs from the first store path'
        firsts[epi] = first
    assert same_bits(firsts['gelu'], firsts['gelu_aux']), f'bm={bm},M={M},N={N},K={K}: aux_out changes `out`'
    assert same_bits(firsts['res'], firsts['res_inplace']), f'bm={bm},M={M},N={N},K={K}: the in-place residual differs'


@pytest.mark.parametrize('bm', list(TILE))
def test_gemm_epilogue_edges(ops, bm):
    """Every bf16-row / fp32 epilogue on every tile height, M one short of and one past the tile height, N = the tile width, + 4, odd and even ragged:
    the three store paths of epilogue_tile (rows through LDS, 8-byte fragments, per-fragment fallback) give the same bits, the first meets the fp64 bound
    (so all do), nothing outside [M, N] is written, aligned or 2 bytes off."""
    from vlaser_amd import _lib as L
    th, tw = TILE[bm]
    worst = Worst()
    for M, K in ((th - 1, 64), (th + 1, 192)):               # K = 192: three K tiles, across the stage ring of the two-stage configurations
        for N in (tw, tw + 4, 1001, 1002):
            _epilogue_case(ops, L, worst, bm, M, N, K)
    worst.flush()


def _all_bf16_upto(lim):
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF).float()
    return x[torch.isfinite(x) & (x.abs() <= lim)]


@pytest.mark.parametrize('bm', [0, 64, 1100])
def test_gemm_gelu_every_bf16(ops, bm):
    """z over every finite bf16 in [-64, 64] through a real GEMM (x = identity, W = the values, bias 0: z is exact): the fast path (N / ldo aligned) and the
    per-fragment path (odd ldo) of BIAS_GELU, and aux_out = z bit for bit."""
    from vlaser_amd import _lib as L
    v = _all_bf16_upto(64.0)
    K = M = 64
    N = (v.numel() + K - 1) // K
    assert v.numel() == 2 * (133 * 128 + 1) and N % 2 == 1
    w = torch.zeros(N * K)
    w[:v.numel()] = v
    w = w.view(N, K)
    z = w.t().double()                                           # out[m, n] = W[n, m]
    ref = gelu64(z)
    tol = ULP * ref.abs() + 2.0 ** -21 * z.abs() + FLOOR
    a_d, w_d, b_d = dev(torch.eye(K)), dev(w), dev(torch.zeros(N))
    ld8 = (N + 7) // 8 * 8
    first = None
    for vname, ldo in (('lds', ld8), ('frag8', ld8 + 4), ('odd', N + 1)):
        flat, out, o = _obuf(M + 3, ldo)
        aflat, aux, ao = _obuf(M + 3, ld8 + 4)
        ops.gemm(L.EPI_BIAS_GELU, a_d, w_d, out=out, bias=b_d, N=N, force_bm=bm, aux_out=aux, ld_aux=ld8 + 4)
        assert _outside_clean(flat, out, o, M, N) and _outside_clean(aflat, aux, ao, M, N)
        bound(f'gemm.gelu[every bf16 |z| <= 64,bm={bm},{vname}]', out[:M, :N], ref, tol)
        # (bf16 denormals may be flushed by the MFMA: compared as values, +-0 == +-0)
        bound(f'gemm.gelu_aux.z[every bf16,bm={bm},{vname}]', aux[:M, :N], z, 0 * z + FLOOR)
        if first is None:
            first = out[:M, :N].clone()
        else:
            assert same_bits(out[:M, :N], first), f'{vname}: differs from the first store path'


def _dsilu(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


@pytest.mark.parametrize('bm', list(TILE))
def test_gemm_fused_epilogues_ragged_m(ops, bm):
    """SWIGLU with aux_out, QKV_ROPE and VIT_QKV on a ragged M (70 rows) of every tile height, into sentinel outputs / caches.  N = 384 of the two fused q/k/v
    epilogues is 1.5 tiles of the 256-column configurations (1200 / 1300 / 1900): guards the per-fragment fallback of both, which had no `n0 < N` test -- the columns
    384 .. 511 of the second tile were stored as a fourth "which" over V^T (vit_qkv.v: 3.1e7 of its bound, now 0.49), and as kv heads behind the V^T cache."""
    from vlaser_amd import _lib as L
    worst = Worst()
    M, K = 70, 64
    n = K // 32 + 10
    x = randb(M, K, seed=1) * pow2(M)[:, None]
    x_d, X64 = dev(x), x.double()
    # ---- SWIGLU + aux_out: I = 64 activation columns, packed [gate16 | up16]
    I = 64
    g_w, u_w = randb(I, K, seed=2) * pow2(I)[:, None] * 8, randb(I, K, seed=3) * pow2(I, -3, 3)[:, None]
    Wp = ops.pack_gate_up(dev(g_w), dev(u_w))
    g, u = X64 @ g_w.double().t(), X64 @ u_w.double().t()
    g_abs, u_abs = X64.abs() @ g_w.double().abs().t(), X64.abs() @ u_w.double().abs().t()
    gr, ur = rbf(g), rbf(u)
    s_r = rbf(torch.nn.functional.silu(gr))
    ref = s_r * ur
    e_g, e_u = ULP * g.abs() + U * n * g_abs, ULP * u.abs() + U * n * u_abs      # the kernel's rounded gate / up against the reference's (a tie crossed: one ulp)
    # silu'' <= 0.5: silu' moves by at most 0.5 e_g over the interval; silu itself (__expf, v_rcp_f32: a few fp32 ulps) and its rounding: one ulp
    tol = ULP * ref.abs() + ur.abs() * ((_dsilu(gr).abs() + 0.5 * e_g) * e_g + ULP * s_r.abs()) + s_r.abs() * e_u + FLOOR
    packed = Wp.float().cpu().double()
    pre, pre_abs = X64 @ packed.t(), X64.abs() @ packed.abs().t()
    first = None
    for vname, ldo, ld_aux in (('tile', I + 8, 2 * I + 8), ('frag', I + 4, 2 * I + 4)):
        flat, out, o = _obuf(M + 3, ldo)
        aflat, aux, ao = _obuf(M + 3, ld_aux)
        ops.gemm(L.EPI_SWIGLU, x_d, Wp, out=out, force_bm=bm, aux_out=aux, ld_aux=ld_aux)
        assert _outside_clean(flat, out, o, M, I) and _outside_clean(aflat, aux, ao, M, 2 * I), f'swiglu {vname}: written outside its outputs'
        worst.add(f'gemm.swiglu[bm={bm}]', out[:M, :I], ref, tol, vname)
        worst.add(f'gemm.swiglu.aux[bm={bm}]', aux[:M, :2 * I], pre, ULP * pre.abs() + U * n * pre_abs + FLOOR, vname)
        if first is None:
            first = (out[:M, :I].clone(), aux[:M, :2 * I].clone())
        else:
            assert same_bits(out[:M, :I], first[0]) and same_bits(aux[:M, :2 * I], first[1]), 'swiglu: the tile and the per-fragment path differ'
    # ---- QKV_ROPE: 1 q head + 1 kv head (N = 384: the 256-column tiles have a ragged right edge), 2 batch elements of 35 tokens into slots [5, 40) of 48
    B, tok, nq, nkv, smax, slot0, n_pos = 2, 35, 1, 1, 48, 5, 4096
    nh = nq + 2 * nkv
    wn = randb(nh * 128, K, seed=4) * pow2(nh * 128)[:, None] * 4
    bn = randb(nh * 128, seed=5) * pow2(nh * 128) * 2.0 ** -3
    qs, ks_ = slice(0, nq * 128), slice(nq * 128, (nq + nkv) * 128)
    vs = slice((nq + nkv) * 128, nh * 128)
    Wq, Bq = ops.pack_qkv(dev(wn[qs]), dev(wn[ks_]), dev(wn[vs]), dev(bn[qs]), dev(bn[ks_]), dev(bn[vs]))
    cos, sin = ops.rope_table(n_pos)
    pos = ((torch.arange(M) * 117 + 3) % n_pos).int()
    pos[0], pos[-1] = n_pos - 1, 0
    zq = X64 @ wn.double().t() + bn.double()
    zq_abs = X64.abs() @ wn.double().abs().t() + bn.double().abs()
    zr = rbf(zq).view(M, nh, 128)
    e_z = (ULP * zq.abs() + U * (n + 1) * zq_abs).view(M, nh, 128)
    c, s = h64(cos)[pos.long()][:, None], h64(sin)[pos.long()][:, None]            # [M, 1, 64]: the kernel's own fp32 table is an input
    lo, hi, elo, ehi = zr[..., :64], zr[..., 64:], e_z[..., :64], e_z[..., 64:]
    rot = torch.cat([lo * c - hi * s, hi * c + lo * s], -1)
    rot_abs = torch.cat([lo.abs() * c.abs() + hi.abs() * s.abs(), hi.abs() * c.abs() + lo.abs() * s.abs()], -1)
    rot_e = torch.cat([elo * c.abs() + ehi * s.abs(), ehi * c.abs() + elo * s.abs()], -1)
    rot_tol = ULP * rot.abs() + rot_e + 3 * U * rot_abs + FLOOR
    v_ref, v_tol = zq.view(M, nh, 128)[:, nq + nkv:], (ULP * zq.abs() + U * (n + 1) * zq_abs).view(M, nh, 128)[:, nq + nkv:] + FLOOR
    n_c = B * nkv * smax * 128
    q_out, kc_flat, vtc_flat = sentinel(M + 3, nq * 128), sentinel(n_c + 2 * smax * 128), sentinel(n_c + 2 * smax * 128)      # (room for a whole stray kv head behind each cache)
    kc, vtc = kc_flat[:n_c].view(B, nkv, smax, 128), vtc_flat[:n_c].view(B, nkv, 128, smax)
    ops.gemm(L.EPI_QKV_ROPE, x_d, Wq, bias=Bq, q_out=q_out, k_cache=kc, vt_cache=vtc, rope_cos=cos, rope_sin=sin, pos_ids=pos.cuda(), n_q_heads=nq, n_kv_heads=nkv,
             s_max=smax, tok_per_batch=tok, slot_base=slot0, force_bm=bm)
    worst.add(f'gemm.qkv_rope.q[bm={bm}]', q_out[:M].view(M, nq, 128), rot[:, :nq], rot_tol[:, :nq])
    kk = kc[:, :, slot0:slot0 + tok].permute(0, 2, 1, 3).reshape(M, nkv, 128)
    worst.add(f'gemm.qkv_rope.k[bm={bm}]', kk, rot[:, nq:nq + nkv], rot_tol[:, nq:nq + nkv])
    vv = vtc[:, :, :, slot0:slot0 + tok].permute(0, 3, 1, 2).reshape(M, nkv, 128)
    worst.add(f'gemm.qkv_rope.v[bm={bm}]', vv, v_ref, v_tol)
    assert is_sent(q_out[M:]) and is_sent(kc[:, :, :slot0]) and is_sent(kc[:, :, slot0 + tok:]), 'qkv_rope: q rows >= M or K-cache slots outside the call written'
    assert is_sent(vtc[:, :, :, :slot0]) and is_sent(vtc[:, :, :, slot0 + tok:]), 'qkv_rope: V^T-cache slots outside the call written'
    assert is_sent(kc_flat[n_c:]) and is_sent(vtc_flat[n_c:]), 'qkv_rope: written behind the caches'
    # ---- VIT_QKV: 2 tiles of 35 tokens, 2 heads, rows padded to 40
    T, S, Hn, Sp = 2, 35, 2, 40
    C = Hn * 64
    wv_, bv_ = randb(3 * C, K, seed=6) * pow2(3 * C)[:, None] * 4, randb(3 * C, seed=7) * pow2(3 * C) * 2.0 ** -3
    zv = X64 @ wv_.double().t() + bv_.double()
    zv_abs = X64.abs() @ wv_.double().abs().t() + bv_.double().abs()
    zt = ULP * zv.abs() + U * (n + 1) * zv_abs + FLOOR
    lay = lambda t: t.view(T, S, 3, Hn, 64).permute(2, 0, 3, 1, 4)                  # [3, T, Hn, S, 64]
    vq, vk, vvt = sentinel(T, Hn, Sp, 64), sentinel(T, Hn, Sp, 64), sentinel(T, Hn, 64, Sp)
    ops.gemm(L.EPI_VIT_QKV, x_d, dev(wv_), bias=dev(bv_), vq=vq, vk=vk, vvt=vvt, vit_heads=Hn, vit_seq=S, vit_seq_pad=Sp, q_scale=0.125, force_bm=bm)
    worst.add(f'gemm.vit_qkv.q[bm={bm}]', vq[:, :, :S], lay(zv)[0] * 0.125, lay(zt)[0] * 0.125)     # (the power-of-two q scale is exact)
    worst.add(f'gemm.vit_qkv.k[bm={bm}]', vk[:, :, :S], lay(zv)[1], lay(zt)[1])
    worst.add(f'gemm.vit_qkv.v[bm={bm}]', vvt[:, :, :, :S].transpose(-1, -2), lay(zv)[2], lay(zt)[2])
    assert is_sent(vq[:, :, S:]) and is_sent(vk[:, :, S:]) and is_sent(vvt[:, :, :, S:]), 'vit_qkv: rows / columns >= vit_seq written'
    worst.flush()


def test_gemm_refusals(ops):
    """ld_aux % 4 != 0, a misaligned aux_out and ldo < N are refused on the host, before any launch."""
    from vlaser_amd import _lib as L
    M, N, K = 20, 128, 64
    x, w, b = dev(randb(M, K)), dev(randb(N, K, seed=1)), dev(randb(N, seed=2))
    out, big = sentinel(M, N), sentinel(M * (N + 8) + 8)
    torch.cuda.synchronize()
    with pytest.raises(L.VlaserHipError, match='aux_out'):
        ops.gemm(L.EPI_BIAS_GELU, x, w, out=out, bias=b, aux_out=big, ld_aux=N + 2)
    with pytest.raises(L.VlaserHipError, match='aux_out'):
        ops.gemm(L.EPI_BIAS_GELU, x, w, out=out, bias=b, aux_out=big[1:], ld_aux=N + 4)
    with pytest.raises(L.VlaserHipError, match='aux_out'):
        ops.gemm(L.EPI_BIAS_GELU, x, w, out=out, bias=b, aux_out=big, ld_aux=N - 4)
    with pytest.raises(L.VlaserHipError, match='aux_out'):
        ops.gemm(L.EPI_SWIGLU, x, w, out=out, aux_out=big[1:], ld_aux=N + 4)
    narrow = big[:M * (N - 8)].view(M, N - 8)
    for epi, kw in ((L.EPI_NONE, {}), (L.EPI_BIAS, dict(bias=b)), (L.EPI_RES, dict(res=narrow)), (L.EPI_BIAS_GELU, dict(bias=b))):
        with pytest.raises(L.VlaserHipError, match='ldo'):
            ops.gemm(epi, x, w, out=narrow, **kw)
    with pytest.raises(L.VlaserHipError, match='ldo'):
        ops.gemm(L.EPI_F32, x, w, out=torch.full((M, N - 8), SENT, device='cuda'))
    torch.cuda.synchronize()
    assert is_sent(out) and is_sent(big), 'a refused call wrote its output'


# ================================================================================================ B. batched GEMM as the backward uses it
def _batched_case(ops, L, worst, name, nn, epi, M, N, K, lda, ldw, ldo, batch, a_bs, w_bs, o_bs, w_group):
    """out[z] (+ z o_bs, rows of ldo) = A[z] (+ z a_bs, rows of lda) @ W[z / w_group] (+ w_bs; NT: [N, K] rows of ldw, NN: [K, N] rows of ldw); every
    operand lives in one flat buffer, so interleaved heads (a_bs < lda) and shared caches are what the kernel sees."""
    f32 = epi == L.EPI_F32
    nb = max(batch, 1)
    wg = w_group if w_group > 1 else 1
    nw = (nb - 1) // wg + 1
    wr, wc = (K, N) if nn else (N, K)
    a_n = (nb - 1) * a_bs + (M - 1) * lda + K
    w_n = (nw - 1) * w_bs + (wr - 1) * ldw + wc
    o_n = (nb - 1) * o_bs + (M - 1) * ldo + N
    a_n, w_n = (a_n + 71) // 8 * 8, (w_n + 71) // 8 * 8
    fa = randb(a_n, seed=1) * pow2((a_n + lda - 1) // lda).repeat_interleave(lda)[:a_n]
    # W slices must be distinguishable (a wrong z / w_group shows): a scale per slice on top of fresh values
    fw = randb(w_n, seed=2) * (2.0 ** ((torch.arange(w_n) // max(w_bs, 1)) % 5 - 2).float() if nw > 1 else 1.0)
    A = torch.as_strided(fa, (nb, M, K), (a_bs, lda, 1)).double()
    Wm = torch.as_strided(fw, (nw, wr, wc), (w_bs, ldw, 1)).double()
    if not nn:
        Wm = Wm.transpose(1, 2)                                  # [nw, K, N]
    Wz = Wm[torch.arange(nb) // wg]
    ref, ref_abs = A @ Wz, A.abs() @ Wz.abs()
    n = K // 32 + 10
    kw = {}
    if epi == L.EPI_BIAS:
        bias = randb(N, seed=3) * 0.25
        ref, ref_abs, n = ref + bias.double(), ref_abs + bias.double().abs(), n + 1
        kw['bias'] = dev(bias)
    tol = (0.0 if f32 else ULP * ref.abs()) + U * n * ref_abs + FLOOR
    a_d, w_d = dev(fa), dev(fw)
    o_d = torch.full((o_n + 64,), SENT, dtype=F32 if f32 else BF, device='cuda')
    (ops.gemm_raw_nn if nn else ops.gemm_raw)(epi, a_d, w_d, o_d, M, N, K, lda, ldw, ldo, batch=batch, a_bs=a_bs, w_bs=w_bs, o_bs=o_bs, w_group=w_group, **kw)
    got = torch.as_strided(o_d.cpu(), (nb, M, N), (o_bs, ldo, 1))
    worst.add(name, got, ref, tol, f'batch={batch},w_group={w_group},M={M},N={N},K={K}')
    written = torch.zeros(o_n + 64, dtype=torch.bool)
    torch.as_strided(written, (nb, M, N), (o_bs, ldo, 1)).fill_(True)
    assert bool((o_d.cpu()[~written] == SENT).all()), f'{name}: written outside the batch slices (batch={batch}, w_group={w_group})'


@pytest.mark.parametrize('batch', [1, 3, 12])
@pytest.mark.parametrize('w_group', [1, 6])
def test_gemm_batched_decoder_shapes(ops, batch, w_group):
    """The three batched calls of backward.attn_bwd_materialised (5 query rows, head_dim 128, keys 64 .. 96 in a cache of 160 slots), nq = batch heads:
    Q K^T (NT, F32), dO V^T (NN, F32), dQ = dS K (NN, NONE) and an NT BIAS form, with spare rows between the batch slices of the score matrices."""
    from vlaser_amd import _lib as L
    worst = Worst()
    nb, hd, sm, nq = 5, 128, 160, batch
    for nk in (64, 96):
        kp = (nk + 63) // 64 * 64
        o_bs = (nb + 2) * kp                                                                     # two sentinel rows between heads
        _batched_case(ops, L, worst, 'gemm_batched.nt_f32[q k^T]', False, L.EPI_F32, nb, nk, hd, nq * hd, hd, kp, batch, hd, sm * hd, o_bs, w_group)
        _batched_case(ops, L, worst, 'gemm_batched.nt_bias[q k^T]', False, L.EPI_BIAS, nb, nk, hd, nq * hd, hd, kp + 4, batch, hd, sm * hd, (nb + 2) * (kp + 4), w_group)
        _batched_case(ops, L, worst, 'gemm_batched.nn_f32[dO v^T]', True, L.EPI_F32, nb, kp, hd, nq * hd, sm, kp, batch, hd, hd * sm, o_bs, w_group)
        _batched_case(ops, L, worst, 'gemm_batched.nn_none[dS k]', True, L.EPI_NONE, nb, hd, kp, kp, hd, nq * hd + 8, batch, nb * kp, sm * hd, hd, w_group)
    worst.flush()


@pytest.mark.parametrize('batch', [1, 3, 12])
def test_gemm_batched_vit_shapes(ops, batch):
    """The batched calls of the ViT attention backward (vla_vlm_group.py) at S = 70 tokens (rows padded to 128), head_dim 64, Hn = batch heads."""
    from vlaser_amd import _lib as L
    worst = Worst()
    S, hdv, sp, Hn = 70, 64, 128, batch
    C = Hn * hdv
    _batched_case(ops, L, worst, 'gemm_batched.vit.nt_f32[q k^T]', False, L.EPI_F32, S, S, hdv, hdv, hdv, sp, batch, sp * hdv, sp * hdv, (S + 2) * sp, 0)
    _batched_case(ops, L, worst, 'gemm_batched.vit.nn_f32[dO v^T]', True, L.EPI_F32, S, sp, hdv, C, sp, sp, batch, hdv, hdv * sp, (S + 2) * sp, 0)
    _batched_case(ops, L, worst, 'gemm_batched.vit.nn_none[dS k]', True, L.EPI_NONE, S, hdv, sp, sp, hdv, 3 * C, batch, S * sp, sp * hdv, hdv, 0)
    worst.flush()


# ================================================================================================ C. vlaser_attn_prefill, one case per instantiation
def _attn_pick(hd, mode, B, sq, kv, n_q):
    """mirror of the choice in vlaser_attn_prefill (csrc/attn.hip): (ks, tk, tail_key0, tail_qb, host)"""
    blocks = (sq + 63) // 64 * n_q * B
    if mode == 3:
        return (1, 64, -1, -1, 0)
    ks = 2 if blocks <= 96 else 1
    tk = 128 if (hd == 64 and mode == 0 and blocks <= 512 and ks == 1) else 64
    if kv <= tk:
        ks = 1
    tail_key0 = tail_qb = -1
    host = 0
    if mode == 0 and ks == 1:
        t = kv % tk
        if 1 <= t <= 32 and kv > tk:
            tail_key0 = kv - t
        if 1 <= sq % 64 <= 16 and sq > 64:
            tail_qb = sq // 64
        if tail_qb >= 0 and tk == 128:
            host = 1
    return (ks, tk, tail_key0, tail_qb, host)


def _qkv_inputs(B, n_q, n_kv, sq, kv_len, ld, hd, vpat, seed):
    """q [B, sq, n_q, hd] with, in every 16-row tile, one all-zero query (uniform softmax) and one scaled by 4 (peaky: the running maximum moves across
    tiles); K [B, n_kv, ld, hd] (rows >= kv_len: garbage that is never visible); V [B, n_kv, ld, hd]: key-scaled randn, or the decoding pattern
    v_j = 2^(j % 5 - 2) e_((7 j) % hd) -- each output channel sums the weights of about kv / hd keys; zero beyond kv_len (the V^T contract)."""
    q = randb(B, sq, n_q, hd, seed=seed)
    r = torch.arange(sq)
    q[:, r % 16 == 3] = 0
    q[:, r % 16 == 9] *= 4
    k = randb(B, n_kv, ld, hd, seed=seed + 1)
    k[:, :, kv_len:] = 3.0
    j = torch.arange(ld)
    if vpat == 'scaled':
        v = randb(B, n_kv, ld, hd, seed=seed + 2) * pow2(ld)[None, None, :, None]
    else:
        v = torch.zeros(B, n_kv, ld, hd)
        v[:, :, j, (7 * j) % hd] = (2.0 ** (j % 5 - 2).float())
    v[:, :, kv_len:] = 0
    return q, k, v


def _attn_ref(q, k, v, kv_len, scale, vis, add=None):
    """q [B, sq, n_q, hd], k / v [B, n_kv, ld, hd], vis [B, sq, kv_len] -> out, out_abs [B, sq, n_q, hd], lse2 [B, n_q, sq], rows with a visible key [B, sq]"""
    G = q.shape[2] // k.shape[1]
    qh = q.double().permute(0, 2, 1, 3)
    kh, vh = k[:, :, :kv_len].double().repeat_interleave(G, 1), v[:, :, :kv_len].double().repeat_interleave(G, 1)
    s = scale * (qh @ kh.transpose(-1, -2))
    if add is not None:
        s = s + add[:, None]
    s = s.masked_fill(~vis[:, None], -math.inf)
    seen = vis.any(-1)
    P = torch.softmax(s, -1).nan_to_num(0.0)
    lse2 = torch.logsumexp(s, -1) * LOG2E
    return (P @ vh).permute(0, 2, 1, 3), (P @ vh.abs()).permute(0, 2, 1, 3), lse2, seen


ATTN_CASES = [
    # id, hd, mode, B, n_q, n_kv, sq, kv_len, extra, expected (ks, tk, tail_key0, tail_qb, host), rows without a visible key
    ('hd64-FULL-ks1-tk128-plain[blocks=100]', 64, 0, 1, 50, 50, 128, 320, {}, (1, 128, -1, -1, 0), 0),
    ('hd64-FULL-ks1-tk128-TAIL-keys[kv=272]', 64, 0, 1, 50, 50, 128, 272, {}, (1, 128, 256, -1, 0), 0),
    ('hd64-FULL-ks1-tk128-HOST[sq=140,kv=272]', 64, 0, 1, 33, 33, 140, 272, {}, (1, 128, 256, 2, 1), 0),
    ('hd64-FULL-ks1-tk128-HOST[sq=140,kv=320]', 64, 0, 1, 33, 33, 140, 320, {}, (1, 128, -1, 2, 1), 0),
    ('hd64-FULL-ks1-tk64-TAIL-wgs[blocks=514]', 64, 0, 1, 257, 257, 70, 70, {}, (1, 64, 64, 1, 0), 0),
    ('hd64-FULL-ks2[blocks=8]', 64, 0, 1, 2, 2, 200, 200, {}, (2, 64, -1, -1, 0), 0),
    ('hd128-CAUSAL-ks1[blocks=120,off=40]', 128, 1, 2, 12, 2, 260, 300, dict(causal_off=40), (1, 64, -1, -1, 0), 0),
    ('hd128-CAUSAL-ks2[blocks=36]', 128, 1, 1, 12, 2, 130, 130, {}, (2, 64, -1, -1, 0), 0),
    ('hd128-PREFIX-ks1[blocks=112,q_row_off=193]', 128, 2, 4, 28, 4, 20, 213, dict(valid=[1, 64, 200, 137], blk_start=200, q_row_off=193), (1, 64, -1, -1, 0), 0),
    ('hd128-PREFIX-ks2[blocks=24,q_row_off=193]', 128, 2, 2, 12, 2, 20, 213, dict(valid=[64, 200], blk_start=200, q_row_off=193), (2, 64, -1, -1, 0), 0),
    ('hd128-PREFIX-ks2[blocks=96,q_row_off=0]', 128, 2, 2, 12, 2, 213, 213, dict(valid=[1, 137], blk_start=200, q_row_off=0), (2, 64, -1, -1, 0), 0),
    ('hd128-FULL-ks1-plain[blocks=112]', 128, 0, 1, 28, 4, 256, 256, {}, (1, 64, -1, -1, 0), 0),
    ('hd128-FULL-ks1-TAIL[sq=200,kv=200]', 128, 0, 1, 28, 4, 200, 200, {}, (1, 64, 192, 3, 0), 0),
    ('hd128-DENSE[blocks=24]', 128, 3, 2, 12, 2, 70, 150, {}, (1, 64, -1, -1, 0), 2),
]


@pytest.mark.parametrize('vpat', ['scaled', 'decode'])
@pytest.mark.parametrize('case', ATTN_CASES, ids=[c[0] for c in ATTN_CASES])
def test_attn_prefill_instantiations(ops, case, vpat):
    """Each (HD, KS, TK, TAIL, HOST, DENSE) instantiation the host can pick, at the smallest shape that selects it; padded o_bs / o_ss and lse_out with
    sentinels; lse_out for every mode."""
    name, hd, mode, B, n_q, n_kv, sq, kv_len, extra, expect, n_unseen = case
    assert _attn_pick(hd, mode, B, sq, kv_len, n_q) == expect, 'the case no longer selects the instantiation its id names'
    ld = (kv_len + 63) // 64 * 64 + 64
    scale = f32s(hd ** -0.5)
    q, k, v = _qkv_inputs(B, n_q, n_kv, sq, kv_len, ld, hd, vpat, seed=len(name))
    i, j = torch.arange(sq)[None, :, None], torch.arange(kv_len)[None, None, :]
    kw, add = {}, None
    if mode == 0:
        vis = torch.ones(B, sq, kv_len, dtype=torch.bool)
    elif mode == 1:
        off = extra.get('causal_off', 0)
        vis = (j <= i + off).expand(B, sq, kv_len)
        kw['causal_off'] = off
    elif mode == 2:
        valid = torch.tensor(extra['valid'], dtype=torch.int32)
        assert valid.numel() == B
        vis = (j < valid[:, None, None]) | ((j >= extra['blk_start']) & (i + extra['q_row_off'] >= extra['blk_start']))
        kw.update(valid_len=valid.cuda(), blk_start=extra['blk_start'], q_row_off=extra['q_row_off'])
    else:
        g = torch.Generator().manual_seed(5)
        mask_rs = (kv_len + 63) // 64 * 64 + 4
        hidden = torch.rand(B, sq, mask_rs, generator=g) < 0.3
        hidden[0, 5] = True                                      # two rows without a visible key
        hidden[1, 64] = True
        hidden[0, 7, :] = True
        hidden[0, 7, 149] = False                                # one visible key: the last
        soft = (torch.rand(B, sq, mask_rs, generator=g) * -2.0).to(F32)
        mask = torch.where(hidden, torch.full_like(soft, torch.finfo(F32).min), soft)
        mask[:, :, kv_len:] = 0.0                                # values past kv_len are read and ignored
        vis = ~hidden[:, :, :kv_len]
        add = mask[:, :, :kv_len].double()
        kw['dense_mask'] = mask.cuda()
    ref, ref_abs, lse_ref, seen = _attn_ref(q, k, v, kv_len, scale, vis, add)
    assert int((~seen).sum()) == n_unseen, 'rows without a visible key: only these may be left out'
    # device layouts: hd 64 as the ViT holds q ([B, H, S, 64]), hd 128 as the decoder does ([B, S, H * 128])
    if hd == 64:
        q_d = dev(q.permute(0, 2, 1, 3))
        q_str = (n_q * sq * hd, sq * hd, hd)
    else:
        q_d = dev(q)
        q_str = (sq * n_q * hd, hd, n_q * hd)
    k_d, vt_d = dev(k), dev(v.transpose(-1, -2))
    o_ss = n_q * hd + 8
    o_bs = (sq + 3) * o_ss
    out = sentinel(B, sq + 3, o_ss)
    lse = torch.full((B * n_q * sq + 16,), SENT, dtype=F32, device='cuda')
    ops.attn_prefill(q_d, k_d, vt_d, out, B, sq, kv_len, n_q, n_kv, hd, q_str, (n_kv * ld * hd, ld * hd), (n_kv * hd * ld, hd * ld), (o_bs, o_ss), ld, scale, mode,
                     lse_out=lse, **kw)
    assert is_sent(out[:, sq:]) and is_sent(out[:, :, n_q * hd:]) and is_sent(lse[B * n_q * sq:]), 'written outside out / lse_out'
    got = h64(out[:, :sq, :n_q * hd]).view(B, sq, n_q, hd)
    tag = f'attn_prefill[{name},{vpat}]'
    bound(tag + '.out', got[seen], ref[seen], ULP * ref[seen].abs() + ULP * ref_abs[seen] + FLOOR)
    got_lse = h64(lse[:B * n_q * sq]).view(B, n_q, sq).permute(0, 2, 1)[seen]
    lr = lse_ref.permute(0, 2, 1)[seen]
    bound(tag + '.lse', got_lse, lr, 2.0 ** -22 * lr.abs() + 2.0 ** -20)


# ================================================================================================ E. norm seams on hard rows
def _n_row(C):
    return 8 * ((C + 511) // 512) + 6         # one wave per row: 8 adds per 16-byte chunk of a lane, then the 6-level butterfly


def _ln_ref(x, w, b, eps):
    """fp64 LayerNorm of x [S, C] and the absolute bound of test_train_ops_gpu.py's forward check: (|xh| + mean|x| rs) |w| (the mean's fp32 error shifts xh)"""
    mean = x.mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    xh = (x - mean) * rs
    return xh * w + b, (xh.abs() + x.abs().mean(-1, keepdim=True) * rs) * w.abs()


def _ln_tol(ref, ref_abs, C):
    return ULP * ref.abs() + U * (_n_row(C) + 8) * ref_abs + FLOOR


def _rms_ref(x, w, eps):
    rs = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
    return x * rs * w


def _rms_tol(ref, C):
    """w * bf16(x rs) rounded once more on the way out: two half-ulp roundings (ULP, + their product), rs from an fp32 sum of C squares"""
    return ULP * (1 + 2.0 ** -7) * ref.abs() + U * (_n_row(C) + 8) * ref.abs() + FLOOR


@pytest.mark.parametrize('C', [8, 520, 1536, 4096])
def test_norms_hard_rows(ops, C):
    worst = Worst()
    S = 7
    w, b = randb(C, seed=1, std=0.5) + 1.0, randb(C, seed=2, std=0.2)
    w, b = w.to(BF).float(), b.to(BF).float()
    for ki, kind in enumerate(LN_KINDS):
        x = _ln_rows(kind, S, C, seed=10 * ki + C)
        x64 = x.double()
        for eps in (1e-6, 1e-5):
            out = sentinel(S + 2, C)
            ops.layernorm(x.cuda(), dev(w), dev(b), eps, out=out[:S])
            ref, ref_abs = _ln_ref(x64, w.double(), b.double(), f32s(eps))
            worst.add(f'layernorm[C={C}]', out[:S], ref, _ln_tol(ref, ref_abs, C), f'{kind},eps={eps:g}')
            assert is_sent(out[S:]), 'layernorm wrote past its rows'
            out = sentinel(S + 2, C)
            ops.rmsnorm(x.cuda(), dev(w), eps, out=out[:S])
            ref = _rms_ref(x64, w.double(), f32s(eps))
            worst.add(f'rmsnorm[C={C}]', out[:S], ref, _rms_tol(ref, C), f'{kind},eps={eps:g}')
            assert is_sent(out[S:]), 'rmsnorm wrote past its rows'
    worst.flush()


@pytest.mark.parametrize('ps_v1', [0, 1])
@pytest.mark.parametrize('C', [8, 1024])
def test_pixel_shuffle_ln_hard_rows(ops, C, ps_v1):
    from oracle import vit as ovit
    worst = Worst()
    T, G = 2, 4
    n_tok = T * (G // 2) ** 2
    w, b = (randb(4 * C, seed=1, std=0.5) + 1.0).to(BF).float(), randb(4 * C, seed=2, std=0.2)
    for ki, kind in enumerate(LN_KINDS):
        x = torch.zeros(T, G * G + 1, C, dtype=BF)
        x[:, 1:] = _ln_rows(kind, T * G * G, C, seed=ki + C).view(T, G * G, C)
        x[:, 0] = 300.0                                           # the CLS row is dropped: it must not reach any statistic
        sh = ovit.pixel_shuffle(x[:, 1:].reshape(T, G, G, C).double(), ps_version='v1' if ps_v1 else 'v2').reshape(n_tok, 4 * C)
        perm = sentinel(n_tok + 1, 4 * C)
        ops.pixel_shuffle(x.cuda(), perm, T, G, C, ps_v1)
        assert torch.equal(bits(perm[:n_tok]), bits(sh.to(BF))) and is_sent(perm[n_tok:]), 'pixel_shuffle is not the oracle permutation'
        out = sentinel(n_tok + 1, 4 * C)
        ops.pixel_shuffle_ln(x.cuda(), dev(w), dev(b), out, T, G, C, 1e-5, ps_v1)
        ref, ref_abs = _ln_ref(sh, w.double(), b.double(), f32s(1e-5))
        worst.add(f'pixel_shuffle_ln[C={C},v1={ps_v1}]', out[:n_tok], ref, _ln_tol(ref, ref_abs, 4 * C), kind)
        assert is_sent(out[n_tok:]), 'pixel_shuffle_ln wrote past its tokens'
    worst.flush()


RN_CASES = [
    # id, C, S, norm (0 none / 1 RMS / 2 LN), bias, ls, h_in, in place
    *[(f'exact-1024-LN-S{S}', 1024, S, 2, True, True, True, False) for S in (1, 4, 8)],
    *[(f'exact-1024-none-S{S}', 1024, S, 0, True, True, True, False) for S in (1, 4, 8)],
    *[(f'exact-1536-RMS-S{S}', 1536, S, 1, False, False, True, False) for S in (1, 4, 8)],
    *[(f'exact-1536-none-S{S}', 1536, S, 0, False, False, True, False) for S in (1, 4, 8)],
    *[(f'exact-3584-RMS-S{S}', 3584, S, 1, False, False, True, False) for S in (1, 4, 8)],       # (S = 8 at 3584: the generic kernel, 8 exact slabs)
    *[(f'exact-3584-none-S{S}', 3584, S, 0, False, False, True, False) for S in (1, 4, 8)],
    ('generic-520-S3-LN', 520, 3, 2, True, True, True, False),
    ('generic-2048-S9-RMS', 2048, 9, 1, False, False, True, False),
    ('generic-2048-S17-LN', 2048, 17, 2, True, True, True, False),
    ('generic-2048-S17-none', 2048, 17, 0, False, False, True, False),
    ('generic-4096-S2-RMS', 4096, 2, 1, False, False, True, False),
    ('generic-1536-S0-RMS', 1536, 0, 1, False, False, True, False),
    ('generic-1024-S0-LN-bias-ls', 1024, 0, 2, True, True, True, False),
    ('generic-1536-S3-RMS-no-h_in', 1536, 3, 1, False, False, False, False),
    ('generic-1024-S4-LN-no-h_in', 1024, 4, 2, True, True, False, False),
    ('generic-1024-S4-LN-bias-without-ls', 1024, 4, 2, True, False, True, False),
    ('generic-1536-S9-RMS-bias-without-ls', 1536, 9, 1, True, False, True, False),
    ('exact-1024-LN-S4-in-place', 1024, 4, 2, True, True, True, True),
    ('generic-2048-S9-RMS-in-place', 2048, 9, 1, False, False, True, True),
    ('generic-520-S3-none-in-place', 520, 3, 0, False, False, True, True),
]


@pytest.mark.parametrize('case', RN_CASES, ids=[c[0] for c in RN_CASES])
def test_reduce_norm_dispatch(ops, case):
    """Every branch of vlaser_reduce_norm's dispatch on the four row families: h_out = bf16(h + [ls *] (sum + bias)) within one rounding of the fp64 sum
    (S slabs, then bias, layer-scale, residual: S + 3 sequential operations), x_out normalised from the bits h_out actually holds."""
    name, C, S, norm, has_bias, has_ls, has_h, inplace = case
    worst = Worst()
    M, eps = 5, 1e-6
    nw, nb = (randb(C, seed=1, std=0.5) + 1.0).to(BF).float(), randb(C, seed=2, std=0.2)
    bias, ls = randb(C, seed=3, std=0.3), randb(C, seed=4, std=0.5)
    for ki, kind in enumerate(LN_KINDS):
        h = _ln_rows(kind, M, C, seed=ki + C + S)
        g = torch.Generator().manual_seed(S + ki)
        part = (torch.randn(max(S, 1), M, C, generator=g) * 0.3 * pow2(M, -6, 0)[None, :, None]).to(F32)
        sm = part[:S].double().sum(0) if S else torch.zeros(M, C, dtype=D64)
        sm_abs = part[:S].double().abs().sum(0) if S else torch.zeros(M, C, dtype=D64)
        t, t_abs = sm, sm_abs
        if has_bias:
            t, t_abs = t + bias.double(), t_abs + bias.double().abs()
        if has_ls:
            t, t_abs = t * ls.double(), t_abs * ls.double().abs()
        h64_ = h.double() if has_h else torch.zeros(M, C, dtype=D64)
        ref_h, ref_h_abs = h64_ + t, h64_.abs() + t_abs
        hbuf, xbuf = sentinel(M + 2, C), sentinel(M + 2, C)
        h_in = None
        if has_h:
            if inplace:
                hbuf[:M] = h.cuda()
                h_in = hbuf
            else:
                h_in = h.cuda()
        ops.reduce_norm(h_in, part.cuda() if S else None, S, M, C, hbuf, xbuf if norm else None, bias=dev(bias) if has_bias else None, ls=dev(ls) if has_ls else None,
                        norm=norm, norm_w=dev(nw) if norm else None, norm_b=dev(nb) if norm == 2 else None, eps=eps)
        where = kind
        worst.add(f'reduce_norm.h[{name}]', hbuf[:M], ref_h, ULP * ref_h.abs() + U * (S + 3) * ref_h_abs + FLOOR, where)
        if S == 0 and has_h and not has_bias:
            assert torch.equal(bits(hbuf[:M]), bits(h)), 'S = 0 without a bias: h_out must be h_in bit for bit'
        assert is_sent(hbuf[M:]), 'reduce_norm wrote past its rows (h_out)'
        hk = h64(hbuf[:M])
        if norm == 2:
            ref, ref_abs = _ln_ref(hk, nw.double(), nb.double(), f32s(eps))
            worst.add(f'reduce_norm.x[{name}]', xbuf[:M], ref, _ln_tol(ref, ref_abs, C), where)
        elif norm == 1:
            ref = _rms_ref(hk, nw.double(), f32s(eps))
            worst.add(f'reduce_norm.x[{name}]', xbuf[:M], ref, _rms_tol(ref, C), where)
        assert is_sent(xbuf[M:]) and (norm or is_sent(xbuf)), 'reduce_norm wrote past its rows (x_out)'
    worst.flush()


@pytest.mark.parametrize('n_partials', [0, 2, 8])
@pytest.mark.parametrize('H', [768, 1536, 3584])
def test_skinny_norm_prologue_hard_rows(ops, H, n_partials):
    """The NORM prologue of vlaser_skinny read through SK_F32 logits with N = 40: rows 0 .. 31 of W are scaled unit vectors, so logit n IS element k_n of the
    normalised row (one non-zero product: exact) and is held to the RMSNorm criterion; rows 32 .. 39 are dense (every normalised element within its two
    roundings: ULP (1 + 2^-7) of the absolute product, + the GEMV's fp32 sum).  h_out = bf16(h + sum of the slabs) within one rounding of the fp64 sum."""
    from vlaser_amd import _lib as L
    worst = Worst()
    M, N, eps = 6, 40, 1e-6
    nw = (randb(H, seed=1, std=0.5) + 1.0).to(BF).float()
    W = torch.zeros(N, H)
    cols = [(n * (H - 1)) // 31 for n in range(32)]                # first and last column, and 30 between
    for n_, c_ in enumerate(cols):
        W[n_, c_] = 2.0 ** (n_ % 3 - 1)
    W[32:] = randb(8, H, seed=2, std=0.05)
    pw = ops.pack_skinny(dev(W))
    for ki, kind in enumerate(LN_KINDS):
        h = _ln_rows(kind, M, H, seed=ki + H + n_partials)
        g = torch.Generator().manual_seed(ki + n_partials)
        part = (torch.randn(max(n_partials, 1), M, H, generator=g) * 0.3 * pow2(M, -6, 0)[None, :, None]).to(F32)
        sm, sm_abs = part[:n_partials].double().sum(0), part[:n_partials].double().abs().sum(0)
        ref_h, ref_h_abs = h.double() + sm, h.double().abs() + sm_abs
        hbuf = sentinel(M + 2, H)
        lg = torch.full((M * N + 8,), SENT, dtype=F32, device='cuda')
        ops.skinny(L.PRO_NORM, L.SK_F32, h.cuda(), pw, M, partials=part.cuda(), n_partials=n_partials, norm_w=dev(nw), h_out=hbuf, out_f32=lg, eps=eps)
        worst.add(f'skinny_norm.h[H={H},S={n_partials}]', hbuf[:M], ref_h, ULP * ref_h.abs() + U * (n_partials + 2) * ref_h_abs + FLOOR, kind)
        assert is_sent(hbuf[M:]) and is_sent(lg[M * N:]), 'skinny NORM + F32 wrote outside h_out / its logits'
        y = _rms_ref(h64(hbuf[:M]), nw.double(), f32s(eps))
        got = h64(lg[:M * N]).view(M, N)
        ref1 = y[:, cols] * W[torch.arange(32), cols].double()
        worst.add(f'skinny_norm.x[H={H},S={n_partials}]', got[:, :32], ref1, _rms_tol(ref1, H), kind)
        Wd = W[32:].double()
        ref2, ref2_abs = y @ Wd.t(), y.abs() @ Wd.abs().t()
        worst.add(f'skinny_norm.logits[H={H},S={n_partials}]', got[:, 32:], ref2, (ULP * (1 + 2.0 ** -7) + U * (H // 32 + 24 + _n_row(H))) * ref2_abs + FLOOR, kind)
    worst.flush()


@pytest.mark.parametrize('n_partials', [0, 3, 8])
def test_vla_euler_velocity_hard_rows(ops, n_partials):
    """vel = bf16(Wd y + bd), y = bf16(bf16(v rs) w), v = bf16(h + sum of the slabs), against the UNROUNDED fp64 chain: v within 2^-8, rs (from the rounded v)
    within 2^-8, the two roundings of y 2^-8 each -- 2 ULP of every |y wd| term --, the output's rounding, and the fp32 sums (8 per thread, 6 + 4 across the
    block, the bias: 19, + the sum of squares behind rs: 19 again)."""
    worst = Worst()
    Wd_, adim, M, eps = 768, 7, 8, 1e-6
    nw = (randb(Wd_, seed=1, std=0.5) + 1.0).to(BF).float()
    wd, bd = randb(adim, Wd_, seed=2, std=0.05), randb(adim, seed=3, std=0.1)
    for ki, kind in enumerate(LN_KINDS):
        h = _ln_rows(kind, M, Wd_, seed=ki + n_partials)
        g = torch.Generator().manual_seed(ki + n_partials)
        part = (torch.randn(max(n_partials, 1), M, Wd_, generator=g) * 0.3).to(F32)
        v = h.double() + part[:n_partials].double().sum(0)
        y = _rms_ref(v, nw.double(), f32s(eps))
        ref = y @ wd.double().t() + bd.double()
        ref_abs = y.abs() @ wd.double().abs().t() + bd.double().abs()
        act0 = torch.randn(M, adim, generator=g)
        act = torch.full((M * adim + 8,), SENT, dtype=F32, device='cuda')
        act[:M * adim] = act0.flatten().cuda()
        vel = torch.full((M * adim + 8,), SENT, dtype=F32, device='cuda')
        ops.vla_euler(h.cuda(), part.cuda(), n_partials, M, dev(nw), eps, dev(wd), dev(bd), act, Wd_, adim, 0.1, 1.0, False, vel)
        worst.add(f'vla_euler.vel[S={n_partials}]', vel[:M * adim].view(M, adim), ref, ULP * ref.abs() + (2 * ULP * (1 + 2.0 ** -6) + U * 40) * ref_abs + FLOOR, kind)
        assert is_sent(vel[M * adim:]) and is_sent(act[M * adim:]), 'vla_euler wrote past its rows'
        # the update itself: torch's arithmetic on the kernel's own velocity, bit for bit
        want = act0 + torch.tensor(0.1, dtype=F32) * vel[:M * adim].view(M, adim).cpu()
        assert torch.equal(act[:M * adim].view(M, adim).cpu(), want), 'a += dt * vel differs from torch'
    worst.flush()


# ================================================================================================ D. skinny and chain attention partials
def _rows_vis(B, tok, kv_len, valid, blk_start, first):
    """visibility of vlaser_attn_skinny / vlaser_chain_attn (PREFIX): key j < valid_len[b], or blk_start <= j < kv_len -- for token 0, when the proprio row rides
    in front (first_tok_kv_len > 0), only up to first_tok_kv_len"""
    j = torch.arange(kv_len)[None, None, :]
    vis = ((j < torch.tensor(valid)[:, None, None]) | (j >= blk_start)).expand(B, tok, kv_len).clone()
    if first:
        vis[:, 0] &= (j[0] < torch.tensor(valid)[:, None]) | (j[0] < first)
    return vis


def _perm_weight(N, K):
    """a scaled permutation matrix [N, K] (N <= K): output n IS input column (7 n + 3) % K times 2^(n % 3 - 1) -- one non-zero product, exact in any order"""
    cols = (7 * torch.arange(N) + 3) % K
    assert cols.unique().numel() == N
    W = torch.zeros(N, K)
    W[torch.arange(N), cols] = 2.0 ** (torch.arange(N) % 3 - 1).float()
    return W, cols


def _rows_to_heads(t, B, nkv, G, tok):
    """partial rows r = hg * tok + t of every kv head [B, nkv, 32, 128] -> [B, tok, n_q, 128]"""
    return t[:, :, :G * tok].reshape(B, nkv, G, tok, 128).permute(0, 3, 1, 2, 4).reshape(B, tok, nkv * G, 128)


def _oproj_checks(worst, tag, where, slabs, x, x_abs, S, M, ks, K, Wp, cols, W2=None):
    """the o_proj slabs over the merged rows bf16(x): through a scaled permutation every element is read back exactly -- one rounding of the fp64 merge x, + the
    merge's fp32 operations (S products and sums, the division: S + 3, on x_abs = the merge of the |o_s|); through a dense W the split-K bound of A on top"""
    x, x_abs = x.reshape(M, K), x_abs.reshape(M, K)
    got = h64(slabs).sum(0)
    if W2 is None:
        wv = Wp[torch.arange(Wp.shape[0]), cols].double()
        ref = x[:, cols] * wv
        worst.add(tag + '.oproj_perm', got, ref, ULP * ref.abs() + U * (S + 3) * x_abs[:, cols] * wv + FLOOR, where)
    else:
        Wa = W2.double().abs()
        ref, ref_abs = x @ W2.double().t(), x.abs() @ Wa.t()
        worst.add(tag + '.oproj_dense', got, ref, (ULP + U * (K // 32 + 10 + ks)) * ref_abs + U * (S + 3) * (x_abs @ Wa.t()) + FLOOR, where)


@pytest.mark.parametrize('vpat', ['scaled', 'decode'])
@pytest.mark.parametrize('first', [0, 385])
@pytest.mark.parametrize('n_splits', [1, 2, 7, 8])
def test_attn_skinny_partials_and_merge(ops, n_splits, first, vpat):
    """vlaser_attn_skinny's (m, l, o) partials merged in fp64 from what the kernel wrote, against the fp64 attention; a split whose keys are all hidden has
    l = 0 and o = 0 (weight exactly 0 in any merge); rows >= group * tokens and everything behind the last split stay SENT; then the VL_PRO_ATTN merge
    of vlaser_skinny read back through a permutation and through a dense o_proj."""
    from vlaser_amd import _lib as L
    worst = Worst()
    B, tok, n_q, n_kv, hd, kv_len, blk, ld = 2, 4, 12, 2, 128, 389, 384, 448
    G, valid = n_q // n_kv, [277, 20]
    scale = f32s(hd ** -0.5)
    q, k, v = _qkv_inputs(B, n_q, n_kv, tok, kv_len, ld, hd, vpat, seed=n_splits)
    q[:, 1], q[:, 2] = 0, q[:, 2] * 4                          # (4 rows only: one zero query, one peaky)
    vis = _rows_vis(B, tok, kv_len, valid, blk, first)
    ref, ref_abs, _, seen = _attn_ref(q, k, v, kv_len, scale, vis)
    assert bool(seen.all())
    nr = G * tok
    n_el = B * n_kv * n_splits * 32
    pm, pl = torch.full((n_el + 32,), SENT, dtype=F32, device='cuda'), torch.full((n_el + 32,), SENT, dtype=F32, device='cuda')
    po = torch.full((n_el * 128 + 4096,), SENT, dtype=F32, device='cuda')
    ops.attn_skinny(dev(q).view(B * tok, n_q * hd), dev(k), dev(v.transpose(-1, -2)), (pm, pl, po), B, tok, kv_len, n_q, n_kv, hd, (tok * n_q * hd, hd, n_q * hd),
                    (n_kv * ld * hd, ld * hd), (n_kv * hd * ld, hd * ld), ld, scale, L.ATTN_PREFIX, n_splits, valid_len=torch.tensor(valid, dtype=torch.int32).cuda(),
                    blk_start=blk, first_tok_kv_len=first)
    assert is_sent(pm[n_el:]) and is_sent(pl[n_el:]) and is_sent(po[n_el * 128:]), 'partials written behind the last split'
    m_, l_, o_ = pm[:n_el].view(B, n_kv, n_splits, 32), pl[:n_el].view(B, n_kv, n_splits, 32), po[:n_el * 128].view(B, n_kv, n_splits, 32, 128)
    assert is_sent(m_[..., nr:]) and is_sent(l_[..., nr:]) and is_sent(o_[..., nr:, :]), 'partial rows >= group * tokens written'
    m64, l64, o64 = h64(m_[..., :nr]), h64(l_[..., :nr]), h64(o_[..., :nr, :])
    # splits without a visible key
    n_chunks = (kv_len + 31) // 32
    cps = (n_chunks + n_splits - 1) // n_splits
    n_dead = 0
    for s in range(n_splits):
        lo, hi = min(s * cps * 32, kv_len), min((s + 1) * cps * 32, kv_len)
        for b in range(B):
            if not bool(vis[b, :, lo:hi].any()):
                n_dead += 1
                assert bool((l64[b, :, s] == 0).all()) and bool((o64[b, :, s] == 0).all()), f'split {s} of batch element {b} sees no key: l and o must be 0'
    assert n_dead >= (1 if n_splits >= 7 else 0)
    Mx = m64.amax(2, keepdim=True)
    f = torch.exp2(m64 - Mx)
    merged = (o64 * f[..., None]).sum(2) / (l64 * f).sum(2)[..., None]              # [B, n_kv, nr, 128]
    tag, where = f'attn_skinny[S={n_splits}]', f'first={first},{vpat}'
    worst.add(tag + '.merged', _rows_to_heads(merged, B, n_kv, G, tok), ref, ULP * ref.abs() + ULP * ref_abs + FLOOR, where)
    # the consumer: VL_PRO_ATTN merges the same partials, rounds to bf16 and runs the o_proj GEMV
    M, K = B * tok, n_q * hd
    x = _rows_to_heads(merged, B, n_kv, G, tok)
    x_abs = _rows_to_heads((o64.abs() * f[..., None]).sum(2) / (l64 * f).sum(2)[..., None], B, n_kv, G, tok)
    Wp, cols = _perm_weight(K, K)
    for W, ks, W2 in ((Wp, 2, None), (randb(768, K, seed=9, std=0.05), 3, True)):
        N = W.shape[0]
        out = torch.full((ks * M * N + 64,), SENT, dtype=F32, device='cuda')
        ops.skinny(L.PRO_ATTN, L.SK_PARTIAL, None, ops.pack_skinny(dev(W), ks), M, out_f32=out, attn_m=pm, attn_l=pl, attn_o=po, attn_splits=n_splits, attn_group=G,
                   attn_nq=tok)
        assert is_sent(out[ks * M * N:]), 'o_proj slabs written past [ks, M, N]'
        _oproj_checks(worst, tag, where, out[:ks * M * N].view(ks, M, N), x, x_abs, n_splits, M, ks, K, Wp, cols, W if W2 else None)
    worst.flush()


CHAIN_CASES = [
    # id, kv_len, blk_start, first_tok_kv_len, valid_len (B = 2), query tokens
    ('kv33-1split', 33, 32, 0, [20, 5], 4),
    ('kv33-1split-first', 33, 32, 33, [20, 5], 1),
    ('kv64-1full-split', 64, 64, 0, [40, 64], 1),
    ('kv389-ragged-7splits', 389, 384, 0, [277, 20], 4),
    ('kv389-ragged-7splits-first', 389, 384, 385, [277, 20], 5),
    ('kv1024-16splits', 1024, 1024, 0, [1000, 3], 1),
]


@pytest.mark.parametrize('vpat', ['scaled', 'decode'])
@pytest.mark.parametrize('case', CHAIN_CASES, ids=[c[0] for c in CHAIN_CASES])
def test_chain_attn_partials_and_oproj(ops, case, vpat):
    """vlaser_chain_attn leaves (m, l) and NORMALISED bf16 rows per split: merged in fp64 (weights l 2^(m - max m)) against the fp64 attention -- the rows'
    rounding and P's, 2^-8 of ref_abs each --; a split without a visible key has l = 0; then vlaser_chain_oproj as in the skinny test."""
    from vlaser_amd import _lib as L
    name, kv_len, blk, first, valid, tok = case
    worst = Worst()
    B, n_q, n_kv, hd = 2, 12, 2, 128
    ld = max(448, (kv_len + 63) // 64 * 64)
    G, nr = n_q // n_kv, (n_q // n_kv) * tok
    nsp = ops.chain_attn_splits(kv_len)
    assert nsp == {33: 1, 64: 1, 389: 7, 1024: 16}[kv_len]
    scale = f32s(hd ** -0.5)
    q, k, v = _qkv_inputs(B, n_q, n_kv, tok, kv_len, ld, hd, vpat, seed=kv_len)
    if tok >= 4:
        q[:, 1], q[:, 2] = 0, q[:, 2] * 4
    else:
        q[1] = q[1] * 4
    vis = _rows_vis(B, tok, kv_len, valid, blk, first)
    ref, ref_abs, _, seen = _attn_ref(q, k, v, kv_len, scale, vis)
    assert bool(seen.all())
    n_el = B * n_kv * nsp * 32
    ml = torch.full((n_el * 2 + 64,), SENT, dtype=F32, device='cuda')
    po = sentinel(n_el * 128 + 4096)
    strides = ((tok * n_q * hd, hd, n_q * hd), (n_kv * ld * hd, ld * hd), (n_kv * hd * ld, hd * ld))
    q_d, k_d, vt_d, vl_d = dev(q), dev(k), dev(v.transpose(-1, -2)), torch.tensor(valid, dtype=torch.int32).cuda()      # (the argument block holds raw pointers)
    a = ops.attn_skinny_args(q_d, k_d, vt_d, (ml, ml, po), B, tok, kv_len, n_q, n_kv, hd, *strides, ld, scale, L.ATTN_PREFIX, nsp, valid_len=vl_d, blk_start=blk,
                             first_tok_kv_len=first)
    ops.launch_chain_attn(a)
    assert is_sent(ml[n_el * 2:]) and is_sent(po[n_el * 128:]), 'partials written behind the last split'
    ml_, o_ = ml[:n_el * 2].view(B, n_kv, nsp, 32, 2), po[:n_el * 128].view(B, n_kv, nsp, 32, 128)
    assert is_sent(ml_[..., nr:, :]) and is_sent(o_[..., nr:, :]), 'partial rows >= group * tokens written'
    m64, l64, o64 = h64(ml_[..., :nr, 0]), h64(ml_[..., :nr, 1]), h64(o_[..., :nr, :])
    n_dead = 0
    for s in range(nsp):
        lo, hi = min(s * 64, kv_len), min((s + 1) * 64, kv_len)
        for b in range(B):
            if not bool(vis[b, :, lo:hi].any()):
                n_dead += 1
                assert bool((l64[b, :, s] == 0).all()), f'split {s} of batch element {b} sees no key: l must be 0'
    assert n_dead >= (1 if kv_len >= 389 else 0)
    w = l64 * torch.exp2(m64 - m64.amax(2, keepdim=True))
    merged = (o64 * w[..., None]).sum(2) / w.sum(2)[..., None]
    tag = f'chain_attn[{name}]'
    x = _rows_to_heads(merged, B, n_kv, G, tok)
    x_abs = _rows_to_heads((o64.abs() * w[..., None]).sum(2) / w.sum(2)[..., None], B, n_kv, G, tok)
    worst.add(tag + '.merged', x, ref, ULP * ref.abs() + ULP * (1 + 2.0 ** -6) * ref_abs + FLOOR, vpat)
    M, K = B * tok, n_q * hd
    Wp, cols = _perm_weight(K, K)
    for W, ks, dense in ((Wp, 2, False), (randb(768, K, seed=9, std=0.05), 3, True)):
        N = W.shape[0]
        assert ops.chain_oproj_supported(M, N, K, ks, nsp, G)
        out = torch.full((ks * M * N + 64,), SENT, dtype=F32, device='cuda')
        pw = ops.pack_skinny(dev(W), ks, 1)
        o_args, _ = ops.skinny_args(None, pw, M, out_f32=out, attn_m=ml, attn_o=po, attn_splits=nsp, attn_group=G, attn_nq=tok)
        ops.launch_chain_oproj(o_args)
        assert is_sent(out[ks * M * N:]), 'o_proj slabs written past [ks, M, N]'
        _oproj_checks(worst, tag, vpat, out[:ks * M * N].view(ks, M, N), x, x_abs, nsp, M, ks, K, Wp, cols, W if dense else None)
    worst.flush()
