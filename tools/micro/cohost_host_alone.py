"""Host-alone check of the co-hosted launches: each fused kernel launched with ZERO guest workgroups (vlaser_cohost_lab(1)) against the stand-alone host, on the joint
prefill's own buffers and shapes -- what sharing a kernel with a guest body (registers, LDS request, block size, packed seam rows) costs the host by itself.
Each form: a HIP graph of 40 launches, replayed in turn, HIP events; median us per launch."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    import bench
    from vlaser_amd import _lib as L, config as C, synth
    from vlaser_amd.engine import plan_guest, prefill_layer_launches, skinny_layer_plan
    from vlaser_amd.pizero import COHOST_LAGGED, COHOST_PAIRS, PiZeroInference
    torch.set_grad_enabled(False)
    vla = C.VLAConfig(base=C.truncated(C.vlaser_2b(), 2, 2))
    dev = 'cuda:0'
    sd = synth.vla_state_dict(vla, device=dev, dtype=torch.bfloat16)
    ids, pv, proprio, noise = bench.make_inputs(vla.base, 1, seed=0)
    m = PiZeroInference(vla, device=dev, max_batch=1, use_graph=False, euler_opts='qkv16,gu16,glue1,chain')
    m.load_state_dict(sd)
    m.infer_action(ids.to(dev), pv.to(dev).to(torch.bfloat16), proprios=proprio.to(dev), noise=noise.to(dev), valid_len=(ids != vla.base.pad_token_id).sum(-1).to(dev))
    torch.cuda.synchronize()
    T, na = m.max_image_text_tokens, m.num_action_tokens
    hosts = dict(prefill_layer_launches(m.vlm, m.vlm.layers[0], m.pbuf, m.h_vlm[:T], m.cache, 0, m.rope, m.pos_vlm, 1, T, L.ATTN_PREFIX, valid_len=m.valid_len,
                                        blk_start=T, next_norm_w=m.vlm.layers[1].ln_in))
    plan = skinny_layer_plan(m.expert, m.expert.layers[0], m.sb_pro, m.h5, None, 0, m.cache, 0, m.rope, m.pos5, 1, na + 1, T, T + 1 + na, L.ATTN_PREFIX,
                             valid_len=m.valid_len, blk_start=T, first_tok_kv_len=T + 1)
    lib, N, R = L.lib(), 40, 15
    print('| host launch | stand-alone us | fused kernel, zero guests, us | with its guest, us |')
    print('|---|---|---|---|')
    # (the lagged pair: the q/k/v GEMM of layer 0 stands for that of layer l + 1 -- the same shape and buffers; the guest is the same launch either way)
    for guest, host, lag in [(g, h, '') for g, h in COHOST_PAIRS.items()] + [(g, h, ', lagged') for g, h in COHOST_LAGGED.items()]:
        forms = []
        for mode, g in ((0, None), (1, plan_guest(plan, guest)), (0, plan_guest(plan, guest))):
            lib.vlaser_cohost_lab(mode)
            hosts[host](guest=g) if g is not None else hosts[host]()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(N):
                    hosts[host](guest=g) if g is not None else hosts[host]()
            forms.append(gr)
        lib.vlaser_cohost_lab(0)
        ts = [[] for _ in forms]
        for _ in range(R):
            for i, gr in enumerate(forms):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); gr.replay(); e1.record()
                torch.cuda.synchronize()
                ts[i].append(e0.elapsed_time(e1) * 1e3 / N)
        med = [sorted(t)[len(t) // 2] for t in ts]
        print(f'| {host} (guest: expert {guest}{lag}) | {med[0]:.2f} | {med[1]:.2f} | {med[2]:.2f} |')


if __name__ == '__main__':
    main()
