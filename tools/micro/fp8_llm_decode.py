"""One mode of the Vlaser-2B greedy decode on one MI355X: `python tools/micro/fp8_llm_decode.py bf16|fp8` loads the full-depth synthetic model with
InternVLChatModel(llm_mlp_weights=MODE) and prints one JSON line: load time and the share of it spent in ops.quantize_rows_e4m3 (fp64 on the host), device memory held
after load, bytes of the LLM's MLP packings, and bench.py's qa figures (S = 560 prompt, 32 decode steps, batch 1 and 8).  Run it under `rocprofv3 --kernel-trace --stats`
for the per-kernel times of the gate/up and down launches of that mode (profiles/fp8_llm_decode_ab.md)."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vlaser_amd import config as C, ops, synth            # noqa: E402
from vlaser_amd.internvl_chat import InternVLChatModel  # noqa: E402


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else 'bf16'
    dev = 'cuda:0'
    torch.set_grad_enabled(False)
    cfg = C.vlaser_2b()
    sd = synth.vlm_state_dict(cfg, device=dev, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    quant, real = [0.0], ops.quantize_rows_e4m3

    def timed(w):
        t0 = time.perf_counter()
        r = real(w)
        quant[0] += time.perf_counter() - t0
        return r
    ops.quantize_rows_e4m3 = timed
    t0 = time.perf_counter()
    m = InternVLChatModel(cfg, device=dev, max_seq_len=640, max_batch=8, llm_mlp_weights=mode)
    m.load_state_dict(sd)
    torch.cuda.synchronize()
    load_s = time.perf_counter() - t0
    ops.quantize_rows_e4m3 = real
    del sd
    torch.cuda.empty_cache()
    m.img_context_token_id = cfg.img_context_token_id
    nb = lambda t: 0 if t is None else (t.t if isinstance(t, ops.PackedW) else t).numel() * (t.t if isinstance(t, ops.PackedW) else t).element_size()
    mlp = {k: sum(nb(getattr(lw, k, None)) for lw in m.llm.layers) for k in ('wgu', 'wdown', 'sk_gu', 'sk_down', 'sk_down4', 'gu8', 'down8')}
    out = {'mode': m.llm_mlp_weights, 'decode_opts': ','.join(m.decode_opts), 'load_s': round(load_s, 2), 'quantize_rows_e4m3_s': round(quant[0], 2),
           'device_bytes_held_after_load': torch.cuda.memory_allocated(), 'synthetic_state_dict_bytes': base, 'llm_mlp_packing_bytes': mlp}
    for B in (1, 8):
        g = torch.Generator().manual_seed(7)
        pv = torch.randn(B, 3, 448, 448, generator=g).to(dev).to(torch.bfloat16)
        ids = torch.cat([torch.randint(0, 151643, (B, 41), generator=g), torch.full((B, 256), cfg.img_context_token_id), torch.randint(0, 151643, (B, 263), generator=g)], 1)
        ts = []
        for n_new in (1, 33):                      # time(33 tokens) - time(1 token) = 32 decode steps, as bench.py's qa_bench
            m.generate(pv, ids, max_new_tokens=n_new, min_new_tokens=n_new)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                m.generate(pv, ids, max_new_tokens=n_new, min_new_tokens=n_new)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / 3)
        out[f'batch{B}'] = {'prefill_ms': round(ts[0] * 1e3, 2), 'decode_ms_per_step': round((ts[1] - ts[0]) / 32 * 1e3, 4)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
