"""A/B of the co-hosted joint prefill's pairs on ONE model instance (tools/micro/ab_chunk.py builds a model per variant, and two instances of the same variant differ
by up to 0.06 ms per chunk -- more than a pair is worth).  Every variant = one set of pairs = its own HIP graph over the SAME weights and buffers; rounds replay the
variants in turn.

    python tools/micro/cohost_ab.py                      # off, all five, each pair alone, each pair left out
    python tools/micro/cohost_ab.py off qkv+attn all     # named sets
    python tools/micro/cohost_ab.py lag                  # the lagged pair: off, the four default pairs, those + down_next, down_next alone, all, off
    python tools/micro/cohost_ab.py mlp8                 # an 'mlp8' model (e4m3 expert MLP weights, W8 guests): off, each default pair alone, the default set, the set minus each pair, off
    python tools/micro/cohost_ab.py mlp8 off gu all      # named sets on an 'mlp8' model

`down_next` in a set = the down projection rides in the next layer's q/k/v GEMM (pizero.COHOST_LAGGED); `all` = the five pairs of COHOST_PAIRS.

Prints median / min ms per chunk and, against `off` and against `all` (under `mlp8` without named sets: against the default set), the difference of the medians with
the spread of `off` over its rounds."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    import bench
    from vlaser_amd import config as C, synth
    from vlaser_amd.pizero import COHOST_PAIRS, LAG_TOKENS, PiZeroInference
    names = list(COHOST_PAIRS)
    argv = sys.argv[1:]
    mlp8 = argv[:1] == ['mlp8']
    argv = argv[1:] if mlp8 else argv
    ref_set = 'all'
    if mlp8 and not argv:          # the per-pair rule on the DEFAULT set: alone against off, left out against the set
        default = next(o for o in PiZeroInference.EULER_DEFAULT.split(',') if o.startswith('cohost='))[len('cohost='):].split('+')
        ref_set = '+'.join(default)
        argv = ['off'] + default + [ref_set] + ['+'.join(x for x in default if x != n) for n in default] + ['off']
    variants = argv or (['off', 'all'] + names + ['+'.join(x for x in names if x != n) for n in names] + ['off'])
    if variants == ['lag']:
        variants = ['off', 'qkv+attn+o+gu', 'qkv+attn+o+gu+down_next', 'down_next', 'all', 'off']
    toks = [() if v == 'off' else tuple(names) if v == 'all' else tuple(v.split('+')) for v in variants]
    assert all(t in COHOST_PAIRS or t in LAG_TOKENS for ts in toks for t in ts), 'unknown pair'
    # a variant = (pairs on | None for the un-hosted schedule, lagged guests)
    sets = [(None if v == 'off' else tuple(t for t in ts if t in COHOST_PAIRS), tuple(LAG_TOKENS[t] for t in ts if t in LAG_TOKENS)) for v, ts in zip(variants, toks)]
    rounds, n = int(os.environ.get('AB_ROUNDS', 9)), 20
    torch.set_grad_enabled(False)
    vla = C.VLAConfig(base=C.vlaser_2b())
    dev = 'cuda:0'
    sd = synth.vla_state_dict(vla, device=dev, dtype=torch.bfloat16)
    ids, pv, proprio, noise = bench.make_inputs(vla.base, 1, seed=0)
    ids_d, pv_d, pro_d, noise_d = ids.to(dev), pv.to(dev).to(torch.bfloat16), proprio.to(dev), noise.to(dev)
    valid = (ids != vla.base.pad_token_id).sum(-1).to(dev)
    m = PiZeroInference(vla, device=dev, max_batch=1, euler_opts='qkv16,gu16,glue1,chain,cohost' + (',mlp8' if mlp8 else ''))
    m.load_state_dict(sd)
    assert m._cohost_ok(1) and m.expert_mlp_weights == ('fp8' if mlp8 else 'bf16')
    call = lambda: m.infer_action(ids_d, pv_d, proprios=pro_d, noise=noise_d, valid_len=valid)
    graphs, ref = [], None
    for v, s in zip(variants, sets):
        (m.cohost_pairs, m.cohost_lagged), m._graphs = s, {}
        for _ in range(3):
            o = call()
        torch.cuda.synchronize()
        graphs.append(m._graphs)
        ref = o.clone() if ref is None else ref
        assert torch.equal(o, ref), f'variant {v}: the chunk differs'
    times = [[] for _ in variants]
    for r in range(rounds):
        for i, s in enumerate(sets):
            (m.cohost_pairs, m.cohost_lagged), m._graphs = s, graphs[i]
            call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                call()
            torch.cuda.synchronize()
            times[i].append((time.perf_counter() - t0) / n * 1e3)
    med = lambda ts: sorted(ts)[len(ts) // 2]
    off = [ts for v, ts in zip(variants, times) if v == 'off']
    spread = max(max(ts) - min(ts) for ts in off) if off else float('nan')
    m_off = med(off[0]) if off else float('nan')
    m_all = next((med(ts) for v, ts in zip(variants, times) if v == ref_set), float('nan'))
    print(f'{"mlp8 (e4m3 expert MLP weights), " if mlp8 else ""}one model instance, {rounds} rounds x {n} chunks per variant; spread of `off` over its rounds {spread:.3f} ms; all chunks bit-identical\n')
    print(f'| pairs on | median ms/chunk | min | max | - off | - {"all" if ref_set == "all" else "`" + ref_set + "`"} |')
    print('|---|---|---|---|---|---|')
    for v, ts in zip(variants, times):
        print(f'| `{v}` | {med(ts):.3f} | {min(ts):.3f} | {max(ts):.3f} | {med(ts) - m_off:+.3f} | {med(ts) - m_all:+.3f} |')


if __name__ == '__main__':
    main()
