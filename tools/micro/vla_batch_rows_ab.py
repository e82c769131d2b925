"""Lab: `VLATrainer(batch_rows=True)` beside the sample-by-sample step of the same build, in ONE process -- full-depth synthetic Vlaser-2B-VLA, the inputs of
bench.vla_train_bench, per-device batch B in {1, 4, 16, 32}; ms per optimizer step, device-synchronised; 2 warm-up steps, then >= 10 steps and >= 1 s;
off / on alternated for three rounds.  Prints one JSON line (profiles/vla_batch_rows_ab.md).
    python tools/micro/vla_batch_rows_ab.py [--batches 1,4,16,32] [--rounds 3] [--only on|off]      (--only on --batches 32 --rounds 1: the run to put under a kernel trace)"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vlaser_amd import config as C, synth          # noqa: E402
from vlaser_amd.vla_train import VLATrainer        # noqa: E402
from bench import make_inputs                      # noqa: E402


def timed(m, samples, min_steps=10, min_s=1.0):
    for _ in range(2):
        r = m.step(samples)
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while n < min_steps or time.perf_counter() - t0 < min_s:
        r = m.step(samples)
        torch.cuda.synchronize()
        n += 1
    return (time.perf_counter() - t0) / n * 1e3, n, float(r.loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,4,16,32')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', choices=('on', 'off'), default=None)
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(',')]
    torch.set_grad_enabled(False)
    vla = C.VLAConfig(base=C.vlaser_2b())
    sd = synth.vla_state_dict(vla, device='cuda', dtype=torch.bfloat16)
    ids, pv, pro, _ = make_inputs(vla.base, 1, seed=5)
    g = torch.Generator().manual_seed(6)
    na, A = vla.num_action_tokens, vla.action_dim
    samples = [dict(input_ids=ids, pixel_values=pv, proprios=pro, actions=torch.rand(1, na, A, generator=g) * 2 - 1, t=torch.rand(1, generator=g) * 0.999,
                    x0=torch.randn(1, na, A, generator=g)) for _ in range(max(batches))]
    paths = {}
    if a.only != 'on':
        paths['off'] = VLATrainer(vla, lr=5e-5, max_grad_norm=1.0).load_state_dict(sd)
    if a.only != 'off':
        paths['on'] = VLATrainer(vla, lr=5e-5, max_grad_norm=1.0, batch_rows=True, max_batch=max(batches)).load_state_dict(sd)
    ms = {p: {B: [] for B in batches} for p in paths}
    loss = {p: {} for p in paths}
    for _ in range(a.rounds):
        for B in batches:
            for p, m in paths.items():
                t, n, l = timed(m, samples[:B])
                ms[p][B].append(round(t, 3))
                loss[p][B] = round(l, 4)
    out = {'config': 'Vlaser-2B-VLA flow-matching training step, full depth, action-expert group, 384-token prompt (277 valid), 4 action tokens; ms per optimizer step; '
                     'rounds alternate batch_rows off / on in one process', 'batches': batches, 'rounds': a.rounds}
    for p in paths:
        out[f'batch_rows_{p}_ms'] = {str(B): ms[p][B] for B in batches}
        out[f'batch_rows_{p}_last_loss'] = {str(B): loss[p][B] for B in batches}
    if len(paths) == 2:
        med = lambda v: sorted(v)[len(v) // 2]
        out['speedup_median'] = {str(B): round(med(ms['off'][B]) / med(ms['on'][B]), 3) for B in batches}
        out['spread_rel'] = {p: {str(B): round((max(ms[p][B]) - min(ms[p][B])) / med(ms[p][B]), 4) for B in batches} for p in paths}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
