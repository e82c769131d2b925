"""GPU: the chain down projection launched from its argument struct (ops.chain_down_args + ops.launch_chain_down), in both weight formats, returns the bits of the
tensor-taking forms, and a stamp buffer set on the struct AFTER it was built is what the next launch uses (tools/micro/chain_timeline.py does that to a plan's struct)."""
import pytest
import torch

from test_fp8_mlp_gpu import _codes, _down_inputs, _down_out, _pow2_scales

pytestmark = pytest.mark.gpu
N, K = 768, 8960


@pytest.mark.parametrize('w8', [False, True], ids=['bf16', 'e4m3'])
@pytest.mark.parametrize('M', [4, 5])              # one and two row groups
def test_struct_launch_equals_tensor_form_and_reads_dbg_at_launch_time(M, w8):
    from vlaser_amd import ops
    x, res = _down_inputs(M, N)
    c, s = _codes(N, K, 11), _pow2_scales(N, 12)
    if w8:
        W, s4 = ops.pack_down4_e4m3(c).cuda(), ops.pack_down4_scales(s).cuda()
        ref = lambda o: ops.chain_down_w8(x, W, s4, res, o, M, N, K)
    else:
        W, s4 = ops.pack_down4(ops.dequantize_rows_e4m3(c, s).cuda()), None
        ref = lambda o: ops.chain_down(x, W, res, o, M, N, K)
    f0, o0 = _down_out(M, N)
    ref(o0)
    wgs = ops.chain_down_geometry(N)[0]
    stamps = torch.zeros(512 * 8, dtype=torch.int64, device='cuda')          # as chain_timeline.py allocates: 8 stamps per workgroup
    assert wgs * 8 <= stamps.numel()
    f1, o1 = _down_out(M, N)
    a = ops.chain_down_args(x, W, res, o1, M, N, K, s4)
    ops.launch_chain_down(a)
    torch.cuda.synchronize()
    assert torch.equal(f1, f0) and bool((o1[:M] != 7.0).any())
    assert not bool(stamps.any()), 'a launch without a stamp buffer wrote stamps'
    f1.fill_(7.0)
    a.dbg = stamps.data_ptr()
    ops.launch_chain_down(a)
    torch.cuda.synchronize()
    assert torch.equal(f1, f0)
    st = stamps.view(-1, 8)
    assert bool((st[:wgs, 0] != 0).all()) and bool((st[:wgs, 5] != 0).all()), 'a workgroup left no stamp'
    assert not bool(st[wgs:].any())
