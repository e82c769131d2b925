"""CPU: the host side of the action expert's one-byte MLP weights (Euler option 'mlp8', PiZero(expert_mlp_weights='fp8')): the row quantiser to OCP e4m3 with
power-of-two scales, the two e4m3 packings and their inverses, the lane contents of the packings against the bf16 ones, the host-side predicates / refusals of
vlaser_chain_gu_w8 and vlaser_chain_down_w8, and the kernel-path decision.  Needs the built library (host functions only), no GPU."""
import ctypes

import pytest
import torch

from vlaser_amd import config as C
from vlaser_amd import engine as E
from vlaser_amd import ops

BF = torch.bfloat16
F8 = torch.float8_e4m3fn


def _hard_rows(K=768):
    """rows spanning 12 binades, a zero row, a row of one value, rows whose absmax is exactly 448 * 2^e, a row with -0 and tiny values next to a large one"""
    g = torch.Generator().manual_seed(3)
    rows = [torch.randn(K, generator=g) * 2.0 ** e for e in range(-9, 3)]                       # absmax over 12 binades
    rows.append(torch.randn(K, generator=g) * 2.0 ** (torch.randint(-12, 1, (K,), generator=g).float()))    # 12 binades INSIDE one row (subnormal codes)
    rows.append(torch.zeros(K))
    rows.append(torch.full((K,), 0.037))
    for e in (-9, 0, 3):
        r = torch.randn(K, generator=g).clamp(-1, 1) * 100 * 2.0 ** e
        r[5] = -448.0 * 2.0 ** e
        rows.append(r)
    r = torch.randn(K, generator=g) * 1e-4
    r[0], r[1], r[2] = 3.0, -0.0, 1e-30
    rows.append(r)
    return torch.stack(rows)


def test_quantiser_properties():
    w = _hard_rows()
    wb = w.to(BF).double()
    codes, scale = ops.quantize_rows_e4m3(w)
    assert codes.dtype == torch.uint8 and codes.shape == w.shape and scale.dtype == torch.float32 and scale.shape == (w.shape[0],)
    m, _ = torch.frexp(scale)
    assert bool((m == 0.5).all()), 'scales are powers of two'
    assert not bool(((codes & 0x7F) == 0x7F).any()), 'a NaN code'
    amax = wb.abs().amax(1)
    s = scale.double()
    assert bool((amax / s <= 448).all())
    nz = amax > 0
    assert bool((amax[nz] / s[nz] > 224).all()), 'the scale is the SMALLEST power of two that fits the row'
    assert bool((s[~nz] == 1).all())
    exact = codes.view(F8).double() * s[:, None]
    deq = ops.dequantize_rows_e4m3(codes, scale)
    assert deq.dtype == BF and torch.equal(deq.double(), exact), 'every dequantised value is exact in bf16'
    err = (exact - wb).abs()
    # e4m3: 3 mantissa bits, round to nearest -> half an ulp = 2^-4 relative in the normal range (|w / scale| >= 2^-6); below it the spacing is 2^-9 (subnormals)
    normal = wb.abs() / s[:, None] >= 2.0 ** -6
    assert bool((err[normal] <= 2.0 ** -4 * wb.abs()[normal]).all())
    assert bool((err[~normal] <= (2.0 ** -10 * s[:, None]).expand_as(err)[~normal]).all())
    # the rows with absmax = 448 * 2^e sit exactly on the largest code, with scale 2^e
    for i, e in zip((15, 16, 17), (-9, 0, 3)):
        assert float(scale[i]) == 2.0 ** e and int(codes[i, 5]) == 0xFE
    # any float dtype in, rounded to bf16 first
    c2, s2 = ops.quantize_rows_e4m3(w.to(BF))
    c3, s3 = ops.quantize_rows_e4m3(w.double())
    assert torch.equal(c2, codes) and torch.equal(s2, scale) and torch.equal(c3, codes) and torch.equal(s3, scale)


def _codes(N, K, seed):
    """random codes over all 254 finite e4m3 values"""
    c = torch.randint(0, 254, (N, K), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    finite = torch.tensor([v for v in range(256) if v & 0x7F != 0x7F], dtype=torch.uint8)
    return finite[c.long()]


@pytest.mark.parametrize('I', [8960, 8208])
def test_gate_up_packing_roundtrip_and_lanes(I):
    H = 768
    cg, cu = _codes(I, H, 1), _codes(I, H, 2)
    sg, su = torch.rand(I, generator=torch.Generator().manual_seed(3)) + 0.5, torch.rand(I, generator=torch.Generator().manual_seed(4)) + 0.5
    W = ops.pack_gate_up8_e4m3(cg, sg, cu, su)
    assert (W.N, W.n_valid, W.K, W.k_splits, W.tpu) == (2 * I, 2 * I, H, 1, 1)
    assert W.t.dtype == torch.uint8 and W.t.numel() == 2 * I * H and W.scale.dtype == torch.float32 and W.scale.numel() == 2 * I        # no padding
    a, b, c, d = ops.unpack_gate_up8_e4m3(W)
    assert torch.equal(a, cg) and torch.equal(b, sg) and torch.equal(c, cu) and torch.equal(d, su)
    # every lane receives the elements of the bf16 packing, in its order: bf16 [u][wave][K-step s][lane][8]; e4m3 [u][wave]{[lane][s = 0, 1][8], [lane][s = 2][8]}
    rows = ops.pack_gate_up8(cg, cu)
    ref = ops.pack_skinny(rows.to(torch.int16), 1, 1)            # (a permutation: any dtype)
    assert ref.N == W.N
    ref = ref.t.view(W.N // 16, 8, 3, 64, 8)
    t = W.t.view(W.N // 16, 8, ops.GU8_WAVE_BYTES)
    lo, hi = t[:, :, :1024].reshape(-1, 8, 64, 2, 8), t[:, :, 1024:].reshape(-1, 8, 64, 8)
    assert torch.equal(lo[:, :, :, 0].to(torch.int16), ref[:, :, 0]) and torch.equal(lo[:, :, :, 1].to(torch.int16), ref[:, :, 1]) and torch.equal(hi.to(torch.int16), ref[:, :, 2])
    # scales in packed row order: row n of the packed matrix carries the scale of the gate / up row it holds
    assert torch.equal(W.scale, ops.pack_gate_up8(sg[:, None], su[:, None]).reshape(-1))


@pytest.mark.parametrize('N', [768, 772, 1536])
def test_down_packing_roundtrip_and_lanes(N):
    K = 8960
    c = _codes(N, K, N)
    s = torch.rand(N, generator=torch.Generator().manual_seed(N)) + 0.5
    p = ops.pack_down4_e4m3(c)
    assert p.dtype == torch.uint8 and p.numel() == N * K
    assert torch.equal(ops.unpack_down4_e4m3(p, N), c)
    wgs, cols, groups = ops.chain_down_geometry(N)
    s4 = ops.pack_down4_scales(s)
    assert s4.shape == (N // cols, 4) and s4.is_contiguous() and torch.equal(ops.unpack_down4_scales(s4, N), s)
    if cols == 3:
        assert torch.equal(s4[:, 3], s4[:, 2])
    # lane (block b, column i) of load l = 2j + l2 holds what it holds in pack_down4
    ref = ops.pack_down4(c.to(torch.int16)).view(wgs, 7, 5, 2, groups, 16, cols, 8)          # [wg, w, j, l2, c, b, i, e]
    got = p.view(wgs, 7, 5, groups, 16, cols, 2, 8).permute(0, 1, 2, 6, 3, 4, 5, 7)
    assert torch.equal(got.to(torch.int16), ref)


def test_w8_predicates_mirror_the_dispatch_tables():
    from vlaser_amd import _lib
    lib = _lib.lib()
    built = {(3, 5, 3, 1)}                   # {K / 256, units per workgroup, slabs, tiles per unit}: what the action expert reaches
    for ns in (2, 3, 4, 6):
        for longest in (1, 2, 3, 4, 5, 6):
            for sp in (1, 2, 3, 4):
                for tpu in (1, 2):
                    N = 16 * tpu * (256 * (longest - 1) + 100)
                    got = lib.vlaser_chain_gu_w8_supported(4, N, ns * 256, sp, tpu)
                    assert got == int((ns, longest, sp, tpu) in built), (ns, longest, sp, tpu, got)
    for M in range(1, 17):                   # every chunks-per-thread value
        assert lib.vlaser_chain_gu_w8_supported(M, 17920, 768, 3, 1) == 1 and lib.vlaser_chain_gu_w8_supported(M, 16416, 768, 3, 1) == 1
    assert lib.vlaser_chain_gu_w8_supported(17, 17920, 768, 3, 1) == 0 and lib.vlaser_chain_gu_w8_supported(0, 17920, 768, 3, 1) == 0
    # down: every (row groups, cols, groups) case of the bf16 dispatch
    for M in (0, 1, 4, 5, 8, 9, 13, 16, 17):
        for N in (768, 772, 1536, 770, 1540):
            for K in (8960, 8832, 18944):
                assert lib.vlaser_chain_down_w8_supported(M, N, K) == lib.vlaser_chain_down_supported(M, N, K), (M, N, K)
    assert lib.vlaser_chain_down_w8_supported(16, 768, 8960) == 1 and lib.vlaser_chain_down_w8_supported(8, 1536, 8960) == 1
    assert lib.vlaser_chain_down_w8_supported(9, 1536, 8960) == 0
    assert ops.chain_gu_w8_supported(4, 17920, 768, 3) and ops.chain_down_w8_supported(4, 768, 8960)


def test_w8_bad_arguments_return_errors_not_crashes():
    """Argument validation happens on the host before any launch: exercised without a GPU."""
    from vlaser_amd import _lib
    lib = _lib.lib()
    P = 4096
    s = _lib.SkinnyArgs()
    assert lib.vlaser_chain_gu_w8(ctypes.byref(s), None) != 0 and b'null' in lib.vlaser_last_error()
    s.x, s.W, s.norm_w, s.out, s.partials = P, P, P, P, P
    s.M, s.N, s.K, s.n_partials, s.tiles_per_unit, s.k_splits, s.ldo = 4, 17920, 768, 3, 1, 1, 8960
    assert lib.vlaser_chain_gu_w8(ctypes.byref(s), None) != 0 and b'null w_scale' in lib.vlaser_last_error()
    s.w_scale = P + 4
    assert lib.vlaser_chain_gu_w8(ctypes.byref(s), None) != 0 and b'alignment' in lib.vlaser_last_error()
    s.w_scale, s.W = P, P + 8
    assert lib.vlaser_chain_gu_w8(ctypes.byref(s), None) != 0 and b'alignment' in lib.vlaser_last_error()
    s.W = P
    for field, bad in (('K', 1536), ('n_partials', 2), ('tiles_per_unit', 2), ('M', 17), ('N', 17920 * 2)):       # shapes the bf16 form serves or nobody does
        good = getattr(s, field)
        setattr(s, field, bad)
        assert lib.vlaser_chain_gu_w8(ctypes.byref(s), None) != 0 and b'vlaser_chain_gu_w8: built for' in lib.vlaser_last_error(), field
        setattr(s, field, good)
    down = lambda x=P, ldx=8960, W=P, sc=P, res=P, out=2 * P, M=4, N=768, K=8960: lib.vlaser_chain_down_w8(x, ldx, W, sc, res, out, M, N, K, None, None)
    assert down(sc=None) != 0 and b'null w_scale' in lib.vlaser_last_error()
    assert down(W=None) != 0 and b'null' in lib.vlaser_last_error()
    assert down(sc=P + 4) != 0 and b'alignment' in lib.vlaser_last_error()
    assert down(W=P + 8) != 0 and b'alignment' in lib.vlaser_last_error()
    for kw in (dict(M=17), dict(K=18944), dict(N=770), dict(M=9, N=1536), dict(ldx=8000)):
        assert down(**kw) != 0 and b'built for' in lib.vlaser_last_error(), kw
    assert down(out=P) != 0                  # res == h_out


def _path(opts, M, tok, kv_len, **kw):
    llm = C.VLAConfig(base=C.vlaser_2b()).expert
    geo = {**E.path_geometry(llm, opts), **{k: kw.pop(k) for k in ('mlp8',) if k in kw}}
    return E.layer_path(**geo, act_width=E.stack_geometry(llm)[4], M=M, tok_per_batch=tok, kv_len=kv_len, **kw)


def test_layer_path_mlp8():
    CHAIN = ('qkv16', 'gu16', 'chain')
    assert E.path_geometry(C.VLAConfig(base=C.vlaser_2b()).expert, CHAIN)['mlp8'] is False
    assert E.path_geometry(C.VLAConfig(base=C.vlaser_2b()).expert, CHAIN + ('mlp8',))['mlp8'] is True
    for M, tok in ((4, 4), (5, 5), (8, 4), (16, 4)):
        assert _path(CHAIN + ('mlp8',), M, tok, 389) == (True, True) == _path(CHAIN, M, tok, 389, mlp8=True)
    assert _path(CHAIN + ('mlp8',), 6, 6, 391) == (True, False)
    assert _path(CHAIN + ('mlp8',), 1, 1, 385, skip_post_attn=True) == (True, False)
    # off the chain path there is no kernel that reads the e4m3 weights
    for opts, kw in ((CHAIN, dict(n_partials=3)), (CHAIN, dict(input_is_hB=True)), (('qkv16', 'gu16'), {}), (('qkv16', 'chain'), {}), ((), {})):
        with pytest.raises(NotImplementedError, match='mlp8'):
            _path(opts, 4, 4, 389, mlp8=True, **kw)
    # a call that stops after q/k/v reads no MLP weight
    assert _path(CHAIN, 1, 1, 385, skip_post_attn=True, input_is_hB=True, mlp8=True) == (False, False)
    # the default keyword leaves the decision as it was
    assert _path(CHAIN, 4, 4, 389, n_partials=3) == (False, False)
