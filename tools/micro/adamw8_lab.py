"""fp32 AdamW against block-wise 8-bit AdamW (optimizer='adamw8bit'): the two kernels alone, and the training steps that run on them.

    python tools/micro/adamw8_lab.py [--kernels-only] [--out profiles/adamw8bit_ab.md]

Kernels: `vlaser_adamw_clipped` and `vlaser_adamw8_clipped` on the same gradients at three sizes -- a 198 M-element bucket (the size the grid comment in
csrc/train.hip was tuned on), one decoder layer of Vlaser-2B, a 1 M-element bucket.  One stream, both warmed up, then rounds that alternate the two
(device events around `reps` launches each); the median round is reported with the spread.  Bytes per element as the kernels move them: 28 (fp32) and
16 + 16 / 128 (8-bit: 2 x 128 codes + 2 absmax read and written per block); the byte counts predict 16.125 / 28 = 0.58 x the time at equal bandwidth.
Steps: one SFT step of Vlaser-2B (bench.py's sample) and one VLA flow-matching step without and with the VLM group, under both optimizers, alternating
whole models in one process."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
HP = (5e-5, 0.9, 0.999, 1e-8, 0.05, 1.0)


def kernel_ab(ops, n, reps, rounds=7):
    dev = 'cuda'
    g_ = torch.Generator(device=dev).manual_seed(n % 1000)
    grad = (torch.randn(n, device=dev, generator=g_) * 0.01).to(BF)
    w0 = torch.randn(n, device=dev, generator=g_) * 0.05
    gn = torch.ones(1, device=dev)
    p32, w32, m, v = torch.empty(n, dtype=BF, device=dev), w0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    p8, w8 = torch.empty(n, dtype=BF, device=dev), w0.clone()
    mc, vc = torch.full((n,), 127, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    mam, vam = torch.zeros(n // 128, device=dev), torch.zeros(n // 128, device=dev)
    del w0
    step = [0]

    def f32():
        ops.adamw_clipped(p32, w32, m, v, grad, *HP, gn, 0.0, step[0])

    def e8():
        ops.adamw8_clipped(p8, w8, mc, vc, mam, vam, None, None, None, grad, *HP, gn, 0.0, step[0])
    for _ in range(5):                       # warm-up: code objects, and a state that is not all zero codes
        step[0] += 1
        f32(); e8()
    torch.cuda.synchronize()
    t = {'fp32': [], '8bit': []}
    for _ in range(rounds):
        for name, fn in (('fp32', f32), ('8bit', e8)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            step[0] += 1
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            t[name].append(a.elapsed_time(b) / reps)
    byts = {'fp32': 28.0 * n, '8bit': 16.0 * n + 16.0 * (n // 128)}
    row = {'n': n}
    for name in t:
        med = statistics.median(t[name])
        row[name] = (med, min(t[name]), max(t[name]), byts[name] / (med * 1e-3) / 1e9)
    return row


def step_ab(make, run, steps, warmup=3, rounds=3):
    """`make(optimizer)` -> model; ms per step of both models, alternating blocks of `steps` steps"""
    models = {o: make(o) for o in ('adamw', 'adamw8bit')}
    for m in models.values():
        for _ in range(warmup):
            run(m)
    torch.cuda.synchronize()
    t = {o: [] for o in models}
    for _ in range(rounds):
        for o, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                run(m)
            torch.cuda.synchronize()
            t[o].append((time.perf_counter() - t0) / steps * 1e3)
    del models
    torch.cuda.empty_cache()
    return {o: (statistics.median(x), min(x), max(x)) for o, x in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--out', default=None, help='also append the tables (markdown) to this file')
    a = ap.parse_args()
    from vlaser_amd import config as C, ops, synth
    from vlaser_amd.param_group import decoder_layer_specs
    import math
    cfg = C.vlaser_2b()
    layer = sum((math.prod(s) + 127) // 128 * 128 for _, s in decoder_layer_specs(cfg.llm))
    lines = ['| elements | fp32 ms (min-max) | fp32 GB/s | 8-bit ms (min-max) | 8-bit GB/s | 8-bit / fp32 time |', '|---|---|---|---|---|---|']
    for n, reps in ((198 * 1024 * 1024 // 128 * 128, 10), (layer, 40), (1 << 20, 200)):
        r = kernel_ab(ops, n, reps)
        f, e = r['fp32'], r['8bit']
        lines.append(f'| {n} | {f[0]:.4f} ({f[1]:.4f}-{f[2]:.4f}) | {f[3]:.0f} | {e[0]:.4f} ({e[1]:.4f}-{e[2]:.4f}) | {e[3]:.0f} | {e[0] / f[0]:.3f} |')
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    if not a.kernels_only:
        import bench
        from vlaser_amd.sft import SFTModel
        from vlaser_amd.vla_train import VLATrainer
        lines += ['', '| step | adamw ms (min-max) | adamw8bit ms (min-max) | 8-bit / fp32 |', '|---|---|---|---|']
        g = torch.Generator().manual_seed(1000)
        S, R = 560, 128
        ids = torch.cat([torch.randint(1, 151643, (41,), generator=g), torch.full((256,), cfg.img_context_token_id),
                         torch.randint(1, 151643, (S - 41 - 256,), generator=g)])[None]
        labels = torch.full_like(ids, -100)
        labels[0, -R:] = ids[0, -R:]
        pv = torch.randn(1, 3, 448, 448, generator=g).cuda().to(BF)
        sd = synth.vlm_state_dict(cfg, device='cuda', dtype=BF)
        res = {'SFT Vlaser-2B, S = 560': step_ab(lambda o: SFTModel(cfg, max_seq_len=576, optimizer=o).load_state_dict(sd), lambda m: m.step(pv, ids, labels), a.steps)}
        del sd
        torch.cuda.empty_cache()
        vla = C.VLAConfig(base=cfg)
        sd = synth.vla_state_dict(vla, device='cuda', dtype=BF)
        vids, vpv, pro, _ = bench.make_inputs(vla.base, 1, seed=5)
        g = torch.Generator().manual_seed(6)
        smp = dict(input_ids=vids, pixel_values=vpv, proprios=pro, actions=torch.rand(1, vla.num_action_tokens, vla.action_dim, generator=g) * 2 - 1,
                   t=torch.rand(1, generator=g) * 0.999, x0=torch.randn(1, vla.num_action_tokens, vla.action_dim, generator=g))
        for name, kw in (('vla_train, action-expert group', {}), ('vla_train, train_vlm=True', {'train_vlm': True})):
            res[name] = step_ab(lambda o: VLATrainer(vla, lr=5e-5, max_grad_norm=1.0, optimizer=o, **kw).load_state_dict(sd), lambda m: m.step([smp]), a.steps)
        for name, r in res.items():
            f, e = r['adamw'], r['adamw8bit']
            lines.append(f'| {name} | {f[0]:.2f} ({f[1]:.2f}-{f[2]:.2f}) | {e[0]:.2f} ({e[1]:.2f}-{e[2]:.2f}) | {e[0] / f[0]:.3f} |')
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
