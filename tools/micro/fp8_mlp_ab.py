"""A/B of the action expert's MLP weights on one MI355X, one process: the default (bf16) model against `expert_mlp_weights='fp8'` (Euler option 'mlp8'), both at full
depth with bench.py's synthetic weights and inputs, alternating rounds.  Per round and mode: ms per infer_action call (bench.py's timed loop), ms of the Euler phase
replayed from its own HIP graph (bench.py `phases.euler_ms`), and the in-chain cost of the gate/up and down launches (Euler graph with - without them, per launch).
    python tools/micro/fp8_mlp_ab.py [--rounds 3] [--steps 50] [--out FILE]
profiles/fp8_mlp_ab.md holds the figures."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--out')
    a = ap.parse_args()
    import bench
    from vlaser_amd import config as C, synth
    from vlaser_amd.pizero import PiZeroInference
    torch.set_grad_enabled(False)
    vla = C.VLAConfig(base=C.vlaser_2b())
    sd = synth.vla_state_dict(vla, device='cuda', dtype=torch.bfloat16)
    models = {}
    for mode in ('bf16', 'fp8'):
        models[mode] = PiZeroInference(vla, max_batch=1, euler_opts=PiZeroInference.EULER_DEFAULT, expert_mlp_weights=mode)
        models[mode].load_state_dict(sd)
    del sd
    torch.cuda.empty_cache()
    ids, pv, proprio, noise = bench.make_inputs(vla.base, 1, seed=0)
    m0 = models['bf16']
    mask, vp, pp, ap_ = m0.build_causal_mask_and_position_ids((ids != vla.base.pad_token_id).long(), torch.bfloat16)
    m1, m2 = m0.split_full_mask_into_submasks(mask)
    dev = [t.cuda() for t in (ids, pv.to(torch.bfloat16), m1, m2, vp, pp, ap_, proprio)]
    noise = noise.cuda()
    calls = {k: (lambda m=m: m.infer_action(*dev, noise=noise)) for k, m in models.items()}
    for c in calls.values():
        for _ in range(5):
            c()
    torch.cuda.synchronize()
    n = vla.expert.num_hidden_layers * vla.num_inference_steps
    rows = {k: [] for k in models}
    for r in range(a.rounds):
        for k, m in models.items():
            calls[k]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                calls[k]()
            torch.cuda.synchronize()
            chunk = (time.perf_counter() - t0) / a.steps * 1e3
            eul = bench._graph_ms(lambda: m._run_euler(1))
            wo_gu = bench._graph_ms(lambda: m._run_euler(1, skip=('gu',)))
            wo_down = bench._graph_ms(lambda: m._run_euler(1, skip=('down',)))
            rows[k].append(dict(chunk_ms=chunk, euler_ms=eul, gu_us_in_chain=(eul - wo_gu) * 1e3 / n, down_us_in_chain=(eul - wo_down) * 1e3 / n))
            print(f'round {r} {k}: ' + ', '.join(f'{kk} {vv:.4f}' for kk, vv in rows[k][-1].items()), flush=True)
    for m in models.values():
        m.check_errors()
    H, I = vla.expert.hidden_size, vla.expert.intermediate_size
    out = {'rounds': a.rounds, 'steps': a.steps, 'launches_per_chunk': n,
           'bytes_per_launch': {'bf16': {'gate_up_weights': 2 * I * H * 2, 'down_weights': H * I * 2},
                                'fp8': {'gate_up_weights': 2 * I * H + 2 * I * 4, 'down_weights': H * I + (H // 3) * 16}}}
    for k, rs in rows.items():
        out[k] = {key: {'median': statistics.median(x[key] for x in rs), 'min': min(x[key] for x in rs), 'max': max(x[key] for x in rs)} for key in rs[0]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
