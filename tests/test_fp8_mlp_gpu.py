"""GPU: the action expert's MLP on one-byte weights (Euler option 'mlp8', PiZero(expert_mlp_weights='fp8')): vlaser_chain_gu_w8 / vlaser_chain_down_w8 stream OCP e4m3
codes with one fp32 scale per weight row, turn them into the bf16 MFMA operand in registers and scale the reduced fp32 sum once.  Every finite e4m3 value is exact in
bf16 and a power-of-two scale is exact on a bf16 value and on an fp32 sum, so with such scales the W8 kernels must return the BITS of the bf16 kernels run on the
dequantised weights -- checked with torch.equal, kernel by kernel and on the whole action chunk.  One case per kernel with scales that are no powers of two goes
against fp64 under the bound the bf16 kernel has for the same contraction length plus one fp32 rounding (of the scaled sum)."""
import pytest
import torch

from bounds import D64, FLOOR, U, ULP, f32s, h64, rbf
from parity import parity

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
SENT = 7.0
EXPERT_MLP = ('mlp.gate_proj.weight', 'mlp.up_proj.weight', 'mlp.down_proj.weight')


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vlaser_amd import ops as o
    return o


def rnd(*s, std=1.0, seed=0):
    return (torch.randn(*s, generator=torch.Generator().manual_seed(seed)) * std).to(BF).cuda()


def _codes(N, K, seed):
    """random codes over all 254 finite e4m3 values (subnormals and -0 included), CPU uint8"""
    finite = torch.tensor([v for v in range(256) if v & 0x7F != 0x7F], dtype=torch.uint8)
    return finite[torch.randint(0, 254, (N, K), generator=torch.Generator().manual_seed(seed))]


def _pow2_scales(N, seed):
    return 2.0 ** torch.randint(-12, -3, (N,), generator=torch.Generator().manual_seed(seed)).float()          # 2^-12 .. 2^-4


def _busy(side, junk):
    with torch.cuda.stream(side):
        junk @ junk


@pytest.fixture(scope='module')
def side():
    return torch.cuda.Stream(), torch.randn(2048, 2048, device='cuda')


def _gu_inputs(M, H, npart=3):
    h, nw = rnd(M, H), (1 + 0.1 * rnd(H, seed=5).float()).to(BF)
    parts = (torch.randn(npart, M, H, generator=torch.Generator().manual_seed(7)) * 0.3).cuda()
    return h, nw, parts


@pytest.mark.parametrize('I', [8960, 8208])              # 8208: 1026 units on 206 workgroups of 5 and 4 -- the workgroups of 4 re-request their last unit
@pytest.mark.parametrize('M', [4, 5, 16])                # 1, 2 and 3 chunks of the residual stream per thread
def test_chain_gu_w8_bit_identical_to_bf16_on_dequantised_weights(ops, side, M, I):
    H, npart = 768, 3
    assert ops.chain_gu_w8_supported(M, 2 * I, H, npart) and ops.chain_gu_supported(M, 2 * I, H, npart, 1)
    h, nw, parts = _gu_inputs(M, H)
    cg, cu, sg, su = _codes(I, H, 1), _codes(I, H, 2), _pow2_scales(I, 3), _pow2_scales(I, 4)
    w8 = ops.pack_gate_up8_e4m3(cg, sg, cu, su).to('cuda')
    dg, du = ops.dequantize_rows_e4m3(cg, sg), ops.dequantize_rows_e4m3(cu, su)
    assert torch.equal(dg.double(), cg.view(F8).double() * sg.double()[:, None])           # exact in bf16
    wb = ops.pack_skinny(ops.pack_gate_up8(dg.cuda(), du.cuda()), 1, 1)

    def run(launch, W):
        out, hb = torch.full((M + 1, I), SENT, dtype=BF, device='cuda'), torch.full((M + 1, H), SENT, dtype=BF, device='cuda')
        a, _ = ops.skinny_args(h, W, M, partials=parts, n_partials=npart, norm_w=nw, h_out=hb, out=out, ldo=I)
        _busy(*side)
        launch(a)
        return out, hb

    o0, h0 = run(ops.launch_chain_gu, wb)
    assert bool((o0[:M] != SENT).any()) and bool(torch.isfinite(o0[:M].float()).all())
    for rep in range(2):
        o1, h1 = run(ops.launch_chain_gu_w8, w8)
        assert torch.equal(o1, o0) and torch.equal(h1, h0), rep
        assert bool((o1[M] == SENT).all()) and bool((h1[M] == SENT).all())
    torch.cuda.synchronize()


def _down_inputs(M, N, K=8960):
    return rnd(M, K, std=0.7), rnd(M, N, std=1.5, seed=2)


def _down_out(M, N):
    flat = torch.full(((M + 1) * N + 8,), SENT, dtype=BF, device='cuda')
    return flat, flat[:(M + 1) * N].view(M + 1, N)


@pytest.mark.parametrize('M,N', [(4, 768), (5, 768), (13, 768), (16, 768), (4, 772), (5, 772), (13, 772), (16, 772), (8, 1536)])
def test_chain_down_w8_bit_identical_to_bf16_on_dequantised_weights(ops, side, M, N):
    K = 8960
    assert ops.chain_down_w8_supported(M, N, K)
    x, res = _down_inputs(M, N)
    c, s = _codes(N, K, N + 1), _pow2_scales(N, N + 2)
    p8, s4 = ops.pack_down4_e4m3(c).cuda(), ops.pack_down4_scales(s).cuda()
    w4 = ops.pack_down4(ops.dequantize_rows_e4m3(c, s).cuda())
    f0, o0 = _down_out(M, N)
    ops.chain_down(x, w4, res, o0, M, N, K)
    for rep in range(2):
        f1, o1 = _down_out(M, N)
        _busy(*side)
        ops.chain_down_w8(x, p8, s4, res, o1, M, N, K)
        assert torch.equal(f1, f0), rep
        assert bool((o1[M] == SENT).all()) and bool((f1[(M + 1) * N:] == SENT).all()) and bool((o1[:M] != SENT).any())
    # the engine's strided [16, K + 64] activation workspace
    xs = torch.zeros(16, K + 64, dtype=BF, device='cuda')
    xs[:M, :K] = x
    f2, o2 = _down_out(M, N)
    ops.chain_down_w8(xs, p8, s4, res, o2, M, N, K)
    assert torch.equal(f2, f0)
    torch.cuda.synchronize()


def _n_row(C):
    return 8 * ((C + 511) // 512) + 6         # as tests/test_fwd_ops_gpu.py: fp32 additions behind the sum of squares of a row


def _dsilu(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def _general_scales(N, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(N, generator=g) + 0.5) * 2.0 ** torch.randint(-10, -6, (N,), generator=g).float()).float()


def test_chain_gu_w8_general_scales_vs_fp64(ops):
    """Scales that are no powers of two: out = bf16(bf16(silu(bf16(s_g G))) * bf16(s_u U)) with G = sum_k code[n, k] x[k] in fp64, x = the fp64 RMSNorm of the residual
    stream the kernel itself published (h_out).  Bound: that of the NORM prologue's dense logits in tests/test_fwd_ops_gpu.py for the same contraction length -- each
    normalised element within its two roundings, the fp32 sum of H / 32 + 24 + n_row(H) terms -- plus ONE fp32 rounding for the scaled sum, carried through the SwiGLU
    as test_gemm_fused_epilogues_ragged_m carries the GEMM's."""
    M, H, I, npart, eps = 5, 768, 8960, 3, 1e-6
    h, nw, parts = _gu_inputs(M, H)
    cg, cu, sg, su = _codes(I, H, 11), _codes(I, H, 12), _general_scales(I, 13), _general_scales(I, 14)
    w8 = ops.pack_gate_up8_e4m3(cg, sg, cu, su).to('cuda')
    out, hb = torch.full((M + 1, I), SENT, dtype=BF, device='cuda'), torch.full((M + 1, H), SENT, dtype=BF, device='cuda')
    a, _ = ops.skinny_args(h, w8, M, partials=parts, n_partials=npart, norm_w=nw, h_out=hb, out=out, ldo=I, eps=eps)
    ops.launch_chain_gu_w8(a)
    hk = h64(hb[:M])
    y = hk / torch.sqrt((hk * hk).mean(-1, keepdim=True) + f32s(eps)) * h64(nw)
    Cg, Cu = cg.view(F8).to(D64), cu.view(F8).to(D64)
    g, u = (y @ Cg.t()) * sg.double(), (y @ Cu.t()) * su.double()
    g_abs, u_abs = (y.abs() @ Cg.abs().t()) * sg.double(), (y.abs() @ Cu.abs().t()) * su.double()
    n = H // 32 + 24 + _n_row(H) + 1
    e_g, e_u = ULP * g.abs() + (ULP * (1 + 2.0 ** -7) + U * n) * g_abs, ULP * u.abs() + (ULP * (1 + 2.0 ** -7) + U * n) * u_abs
    gr, ur = rbf(g), rbf(u)
    s_r = rbf(torch.nn.functional.silu(gr))
    ref = s_r * ur
    tol = ULP * ref.abs() + ur.abs() * ((_dsilu(gr).abs() + 0.5 * e_g) * e_g + ULP * s_r.abs()) + s_r.abs() * e_u + FLOOR
    got = h64(out[:M])
    assert torch.isfinite(got).all() and bool((out[M] == SENT).all())
    parity('chain_gu_w8.general_scales', ((got - ref).abs() / tol).max().item(), 1.0, note='max |got - ref| / tol')


def test_chain_down_w8_general_scales_vs_fp64(ops):
    """h_out = bf16(res + s_n sum_k code[n, k] x[k]) against fp64: the bf16-output GEMM bound of tests/bounds.py at K = 8960 (n_seq = K / 32 + 10) with one more fp32
    rounding, of the scaled sum."""
    M, N, K = 5, 772, 8960
    x, res = _down_inputs(M, N)
    c, s = _codes(N, K, 21), _general_scales(N, 22)
    _, o = _down_out(M, N)
    ops.chain_down_w8(x, ops.pack_down4_e4m3(c).cuda(), ops.pack_down4_scales(s).cuda(), res, o, M, N, K)
    Cd, X = c.view(F8).to(D64), h64(x)
    ref = h64(res) + (X @ Cd.t()) * s.double()
    ref_abs = h64(res).abs() + (X.abs() @ Cd.abs().t()) * s.double()
    tol = ULP * ref.abs() + U * (K // 32 + 10 + 1) * ref_abs + FLOOR
    got = h64(o[:M])
    assert torch.isfinite(got).all() and bool((o[M] == SENT).all())
    parity('chain_down_w8.general_scales', ((got - ref).abs() / tol).max().item(), 1.0, note='max |got - ref| / tol')


# ------------------------------------------------------------------------------------------------ the whole action chunk
def _obs(cfg, seed, B=1):
    """the observation of tests/test_general_masks_gpu.py::_obs"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((B, 384), cfg.pad_token_id)
    ids[:, :10] = torch.randint(0, 151643, (B, 10), generator=g)
    ids[:, 10:266] = cfg.img_context_token_id
    ids[:, 266:277] = torch.randint(0, 151643, (B, 11), generator=g)
    return ids, torch.randn(B, 3, 448, 448, generator=g), torch.rand(B, 1, 7, generator=g) * 2 - 1, torch.randn(B, 4, 7, generator=g)


def _is_expert_mlp(k):
    return k.startswith('action_expert.') and k.endswith(EXPERT_MLP)


@pytest.fixture(scope='module')
def cases(golden_model):
    """Per batch size: the observation, the state dict with the expert's MLP weights replaced by dequantize(quantize(.)), and the CPU oracle's chunks on both."""
    from oracle import vla as ovla
    from vlaser_amd import ops as o
    cfg, vla, sd = golden_model
    sdq = {k: (o.dequantize_rows_e4m3(*o.quantize_rows_e4m3(v)).to(v.dtype) if _is_expert_mlp(k) else v) for k, v in sd.items()}
    assert sum(_is_expert_mlp(k) for k in sd) == 3 * vla.expert.num_hidden_layers
    made = {}

    def get(B):
        if B not in made:
            ids, pv, pro, noise = _obs(cfg, 39 + B, B)
            am = (ids != cfg.pad_token_id).long()
            mask, vp, pp, ap = ovla.build_causal_mask_and_position_ids(am, torch.float32, vla)
            m1, m2 = ovla.split_full_mask_into_submasks(mask, vla)
            call = (ids, pv, m1, m2, vp, pp, ap, pro)
            made[B] = (call, noise, ovla.infer_action(sdq, vla, *call, noise), ovla.infer_action(sd, vla, *call, noise))
        return made[B]
    return sdq, get


@pytest.mark.parametrize('use_graph', [True, False])
@pytest.mark.parametrize('B', [1, 2])
def test_infer_action_fp8_equals_default_on_dequantised_weights(golden_model, cases, B, use_graph):
    from vlaser_amd.pizero import PiZeroInference
    cfg, vla, sd = golden_model
    sdq, get = cases
    call, noise, ref_q, ref = get(B)
    m = PiZeroInference(vla, max_batch=B, use_graph=use_graph, expert_mlp_weights='fp8')
    assert 'mlp8' in m.euler_opts and m.expert_mlp_weights == 'fp8'
    m.load_state_dict(sd)
    d = PiZeroInference(vla, max_batch=B, use_graph=use_graph)
    assert 'mlp8' not in d.euler_opts and d.expert_mlp_weights == 'bf16'
    d.load_state_dict(sdq)
    act, want = m.infer_action(*call, noise=noise), d.infer_action(*call, noise=noise)
    assert torch.equal(act, want)
    assert torch.equal(m.last_velocities(B), d.last_velocities(B))
    err_q, err = (act.cpu() - ref_q).abs().max().item(), (act.cpu() - ref).abs().max().item()
    print(f'[parity] infer_action mlp8 B={B} graph={use_graph}: max|err| vs oracle on the dequantised weights = {err_q:.3e} (bound 1e-2); '
          f'vs oracle on the unquantised weights = {err:.3e} (the format\'s deviation, not asserted); oracle quantised vs unquantised = {(ref_q - ref).abs().max().item():.3e}')
    assert err_q < 1e-2
    again = m.infer_action(*call, noise=noise)
    assert torch.equal(act, again)
    m.check_errors()
    d.check_errors()


def test_infer_action_fp8_with_general_masks_and_output_ring(golden_model, cases):
    """The opt-in plumbing around the Euler phase is untouched by the option: dense masks served as given + a result ring, captured in the HIP graph."""
    from vlaser_amd.pizero import PiZeroInference
    cfg, vla, sd = golden_model
    sdq, get = cases
    call, noise, ref_q, _ = get(1)
    m = PiZeroInference(vla, max_batch=1, general_masks=True, output_ring=2, euler_opts='qkv16,gu16,glue1,chain,mlp8')
    m.load_state_dict(sd)
    d = PiZeroInference(vla, max_batch=1, general_masks=True, output_ring=2)
    d.load_state_dict(sdq)
    for _ in range(3):
        act, want = m.infer_action(*call, noise=noise), d.infer_action(*call, noise=noise)
        assert torch.equal(act, want)
    assert (act.cpu() - ref_q).abs().max().item() < 1e-2
    m.check_errors()


def test_mlp8_needs_the_chain_options(golden_model, monkeypatch):
    from vlaser_amd.pizero import PiZero, PiZeroInference
    cfg, vla, sd = golden_model
    with pytest.raises(ValueError, match='chain'):
        PiZeroInference(vla, euler_opts='qkv16,gu16,glue1,mlp8')
    with pytest.raises(ValueError, match='gu16'):
        PiZeroInference(vla, euler_opts='qkv16,glue1,chain', expert_mlp_weights='fp8')
    with pytest.raises(ValueError, match='qkv16, gu16'):
        PiZero(vla, euler_opts='chain,mlp8')
    with pytest.raises(ValueError, match='expert_mlp_weights'):
        PiZeroInference(vla, expert_mlp_weights='int8')
    monkeypatch.setenv('VLASER_EULER', PiZero.EULER_DEFAULT + ',mlp8')
    assert PiZeroInference(vla).expert_mlp_weights == 'fp8'
    monkeypatch.setenv('VLASER_EULER', 'qkv16,mlp8')
    with pytest.raises(ValueError, match='chain, gu16'):
        PiZeroInference(vla)
    monkeypatch.delenv('VLASER_EULER')
    assert PiZeroInference(vla).expert_mlp_weights == 'bf16'


def test_mlp8_footprint(golden_model, ops):
    """The expert's MLP weights of an 'mlp8' model: one byte per weight + the scale arrays + what the packers pad (nothing for gate/up; a fourth scale per 3-column
    group of the down projection), and no bf16 gate/up/down packing alive."""
    from vlaser_amd.pizero import PiZeroInference
    cfg, vla, sd = golden_model
    H, I = vla.expert.hidden_size, vla.expert.intermediate_size
    m = PiZeroInference(vla, expert_mlp_weights='fp8')
    m.load_state_dict(sd)
    # what the packers make of matrices of these shapes (CPU)
    zc = lambda n, k: torch.zeros(n, k, dtype=torch.uint8)
    gu = ops.pack_gate_up8_e4m3(zc(I, H), torch.ones(I), zc(I, H), torch.ones(I))
    packed = (gu.t.numel() + 4 * gu.scale.numel(), ops.pack_down4_e4m3(zc(H, I)).numel() + 4 * ops.pack_down4_scales(torch.ones(H)).numel())
    padding = sum(packed) - (3 * I * H + 4 * (2 * I + H))
    assert 0 <= padding <= 4 * H // 3
    nbytes = lambda t: t.numel() * t.element_size()
    for lw in m.expert.layers:
        held = nbytes(lw.gu8.t) + nbytes(lw.gu8.scale) + nbytes(lw.down8) + nbytes(lw.down8_scale)
        assert held <= 2 * I * H + H * I + 4 * (2 * I + H) + padding
        assert lw.gu8.t.dtype == torch.uint8 and lw.down8.dtype == torch.uint8 and lw.gu8.t.is_cuda and lw.down8.is_cuda
        assert lw.sk_gu is None and lw.sk_down is None and lw.sk_down4 is None
        for name, v in vars(lw).items():
            t = v.t if isinstance(v, ops.PackedW) else v
            if isinstance(t, torch.Tensor) and name not in ('gu8', 'down8'):
                assert t.numel() < I * H, f'{name}: a second copy of an MLP matrix'
    # the default model holds the bf16 packings the option replaces
    dflt = PiZeroInference(vla)
    dflt.load_state_dict(sd)
    lw = dflt.expert.layers[0]
    assert nbytes(lw.sk_gu.t) + nbytes(lw.sk_down4) == 2 * (3 * I * H) and not hasattr(lw, 'gu8')
