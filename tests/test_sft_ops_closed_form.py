"""The closed form that tests/test_sft_ops_gpu.py uses as the reference of the fused attention backward (bounds.attn_bwd_ref) is the gradient of the masked
softmax attention: checked against fp64 autograd.  Needs no GPU."""
import math

import torch

from bounds import D64, attn_bwd_ref


def test_attn_bwd_closed_form_is_autograd():
    """The closed form above is the gradient of the masked softmax attention when o and lse are its exact forward output (needs no GPU)."""
    H, S, hd, scale = 3, 7, 128, 1.0 / math.sqrt(128)
    g = torch.Generator().manual_seed(11)
    q, k, v, d_o = (torch.randn(H, S, hd, generator=g, dtype=D64) for _ in range(4))
    for vis in (torch.tril(torch.ones(S, S, dtype=torch.bool)), (torch.arange(S) < 4)[None].expand(S, S)):
        with torch.enable_grad():
            qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
            s = ((qg @ kg.transpose(1, 2)) * scale).masked_fill(~vis, -math.inf)
            o = torch.softmax(s, -1) @ vg
            gq, gk, gv = torch.autograd.grad(o, (qg, kg, vg), d_o)
        lse2 = torch.logsumexp(s.detach(), -1) / math.log(2)
        r = attn_bwd_ref(q, k, v, d_o, o.detach(), lse2, vis, scale, log2e=1 / math.log(2))
        for name, want in (('dq', gq), ('dk', gk), ('dv', gv)):
            assert torch.allclose(r[name], want, rtol=1e-10, atol=1e-12), name
        assert (r['dk'][:, ~vis.any(0)] == 0).all() and (r['dv'][:, ~vis.any(0)] == 0).all()
