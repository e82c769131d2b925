"""SFT `batch_rows` mode (GPU): a per-device batch of B > 1 samples as ONE forward / backward over its concatenated rows (varlen attention) --
against torch autograd through the fp32 CPU oracle with the bounds of tests/test_sft_gpu.py (loss |err| <= 5e-3; per-tensor relative Frobenius
error <= 4e-2, cosine >= 0.999), against the one-sample-at-a-time path of the same build, and bit for bit where the kernels and values are the same."""
import os

import pytest
import torch

from test_sft_gpu import _four_samples, _rel

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
KEYS = ['language_model.model.layers.1.mlp.down_proj.weight', 'language_model.model.layers.0.self_attn.q_proj.weight', 'mlp1.3.weight',
        'language_model.model.norm.weight', 'language_model.lm_head.weight']


def _oracle(cfg, sd, pvs, rows, labs, weights):
    """Loss and gradients of sum_b weights[b] * (mean CE of sample b) by torch autograd through the fp32 CPU oracle."""
    from oracle import vlm as ovlm
    torch.set_grad_enabled(True)
    try:
        sdg = {k: (v.clone().requires_grad_(True) if k in KEYS else v) for k, v in sd.items()}
        tot = 0
        for b in range(len(rows)):
            tot = tot + weights[b] * ovlm.sft_loss(ovlm.forward_logits(sdg, cfg, pvs[b], rows[b][None]), labs[b][None])
        tot.backward()
        return tot.item(), {k: sdg[k].grad for k in KEYS}
    finally:
        torch.set_grad_enabled(False)


def _model(cfg, sd, S, **kw):
    from vlaser_amd.sft import SFTModel
    kw = dict(dict(max_grad_norm=0.0, lr=0.0, weight_decay=0.0), **kw)      # lr 0: the step leaves the weights alone
    m = SFTModel(cfg, max_seq_len=S, **kw)
    m.load_state_dict(sd)
    return m


FLAGS4 = torch.ones(4, 1, dtype=torch.long)


def test_batch4_as_one_pass_equals_the_oracle_batch_gradient(golden_model):
    """The oracle check of test_batch4_equals_accumulation_of_4_and_oracle_batch_gradient ('batch' weights R_b / R: the mean over ALL supervised tokens)
    with batch_rows=True: same keys, same bounds; a second run is bit-identical."""
    cfg, _, sd = golden_model
    pv, ids, lab, rows, labs, pvs = _four_samples(cfg)
    R = torch.tensor([float((l[1:] != -100).sum()) for l in labs])
    m = _model(cfg, sd, ids.shape[1], batch_rows=True)
    assert m.batch_rows
    out = m.train_step([(pv, ids, lab, FLAGS4)])
    ref_loss, ref_g = _oracle(cfg, sd, pvs, rows, labs, (R / R.sum()).tolist())
    print(f'batch rows: loss {out.loss.item():.6f} vs oracle {ref_loss:.6f}')
    assert abs(out.loss.item() - ref_loss) < 5e-3, (out.loss.item(), ref_loss)
    grads = m.named_grads()
    for k in KEYS:
        rel, cos = _rel(grads[k], ref_g[k])
        print(f'batch rows: {k} rel {rel:.4g} cos {cos:.6f}')
        assert rel < 4e-2 and cos > 0.999, (k, rel, cos)
    assert m.M_max >= sum(len(r) for r in rows) > m.S_max                   # the row buffers grew; max_seq_len still bounds one sample
    m2 = _model(cfg, sd, ids.shape[1], batch_rows=True)
    out2 = m2.train_step([(pv, ids, lab, FLAGS4)])
    assert torch.equal(m2.fp.g, m.fp.g) and out2.loss.item() == out.loss.item() and out2.grad_norm.item() == out.grad_norm.item()


def test_single_sample_micro_batches_take_the_unchanged_path(golden_model):
    """batch_rows=True with B == 1 micro-batches: gradients, loss and gradient norm bit-equal to batch_rows=False (one sample per step, and the same
    four samples as four accumulation micro-batches)."""
    cfg, _, sd = golden_model
    pv, ids, lab, rows, labs, pvs = _four_samples(cfg)
    for mbs in ([(pvs[0], rows[0][None], labs[0][None], None)], [(pvs[b], rows[b][None], labs[b][None], None) for b in range(4)]):
        res = []
        for br in (False, True):
            m = _model(cfg, sd, ids.shape[1], batch_rows=br, max_grad_norm=1.0)
            out = m.train_step(mbs)
            res.append((m.fp.g.clone(), out.loss.item(), out.grad_norm.item()))
        assert torch.equal(res[0][0], res[1][0]) and res[0][1:] == res[1][1:], (res[0][1:], res[1][1:])


def test_switch_by_environment_equals_switch_by_argument(golden_model, monkeypatch):
    cfg, _, sd = golden_model
    pv, ids, lab, rows, labs, pvs = _four_samples(cfg)
    a = _model(cfg, sd, ids.shape[1], batch_rows=True)
    oa = a.train_step([(pv, ids, lab, FLAGS4)])
    monkeypatch.setenv('VLASER_SFT_BATCH_ROWS', '1')
    b = _model(cfg, sd, ids.shape[1])
    assert b.batch_rows
    ob = b.train_step([(pv, ids, lab, FLAGS4)])
    assert torch.equal(a.fp.g, b.fp.g) and oa.loss.item() == ob.loss.item() and oa.grad_norm.item() == ob.grad_norm.item()
    monkeypatch.setenv('VLASER_SFT_BATCH_ROWS', '0')
    c = _model(cfg, sd, ids.shape[1], batch_rows=True)
    assert not c.batch_rows                                                  # the environment wins, as for VLASER_SFT_ATTN_BWD
    monkeypatch.delenv('VLASER_SFT_BATCH_ROWS')
    from vlaser_amd.sft import SFTModel
    with pytest.raises(ValueError):
        SFTModel(cfg, batch_rows=True, attn_bwd='materialised')


def test_recompute_equals_kept_activations_in_batch_rows_mode(golden_model):
    cfg, _, sd = golden_model
    pv, ids, lab, rows, labs, pvs = _four_samples(cfg)
    res = []
    for rc in (False, True):
        m = _model(cfg, sd, ids.shape[1], batch_rows=True, recompute=rc, max_grad_norm=1.0)
        out = m.train_step([(pv, ids, lab, FLAGS4)])
        assert m.x1.shape[0] == (1 if rc else cfg.llm.num_hidden_layers)
        res.append((m.fp.g.clone(), out.loss.item(), out.grad_norm.item()))
    assert torch.equal(res[0][0], res[1][0]) and res[0][1:] == res[1][1:], (res[0][1:], res[1][1:])


def test_two_optimizer_steps_batch_rows_vs_sequential(golden_model):
    """lr > 0, clipping on.  Both paths are bf16 realisations of the same fp32 step, each within (rel 4e-2, cos 0.999) of the oracle, so their gradients may
    differ by at most twice that (rel < 8e-2, cos > 0.998) and the reported gradient norm -- from the producers in one mode, from the buffer pass in the
    other -- by the same relative margin: a mis-scaled loss or a double-counted norm shows here, not in the lr = 0 oracle test."""
    cfg, _, sd = golden_model
    pv, ids, lab, rows, labs, pvs = _four_samples(cfg)
    res = []
    for br in (False, True):
        m = _model(cfg, sd, ids.shape[1], batch_rows=br, lr=1e-3, weight_decay=0.05, max_grad_norm=1.0)
        steps = []
        for _ in range(2):
            out = m.train_step([(pv, ids, lab, FLAGS4)])
            steps.append((out.loss.item(), out.grad_norm.item(), {k: v.clone() for k, v in m.named_grads().items() if k in KEYS}))
        m.wait_optimizer()
        res.append(steps)
    for s in range(2):
        (la, na, ga), (lb, nb, gb) = res[0][s], res[1][s]
        print(f'step {s}: loss {la:.6f} / {lb:.6f}, grad norm {na:.6f} / {nb:.6f}')
        if s == 0:                      # same weights: both losses are within 5e-3 of the oracle's.  (Step 1 runs on weights AdamW moved by ~lr per element whatever the
            assert abs(la - lb) < 2 * 5e-3, (s, la, lb)      # gradient's size, so near-zero gradients may have stepped in opposite directions: its loss is printed, not bounded)
        assert abs(na - nb) < 8e-2 * na, (s, na, nb)
        for k in KEYS:
            rel, cos = _rel(gb[k], ga[k])
            print(f'step {s}: {k} rel {rel:.4g} cos {cos:.6f}')
            assert rel < 8e-2 and cos > 0.998, (s, k, rel, cos)
    assert res[0][1][0] < res[0][0][0] and res[1][1][0] < res[1][0][0]       # the step moved the weights: the loss on the same batch went down


def test_two_micro_batches_of_two_samples_vs_oracle(golden_model):
    """GA = 2: each micro-batch is one pass over its two samples; HF semantics = the mean over each micro-batch's supervised tokens, divided by GA:
    sample b weighs 0.5 * R_b / R_mb."""
    cfg, _, sd = golden_model
    pv, ids, lab, rows, labs, pvs = _four_samples(cfg)
    R = [float((l[1:] != -100).sum()) for l in labs]
    w = [0.5 * R[0] / (R[0] + R[1]), 0.5 * R[1] / (R[0] + R[1]), 0.5 * R[2] / (R[2] + R[3]), 0.5 * R[3] / (R[2] + R[3])]
    m = _model(cfg, sd, ids.shape[1], batch_rows=True)
    fl = torch.ones(2, 1, dtype=torch.long)
    out = m.train_step([(pv[:2], ids[:2], lab[:2], fl), (pv[2:], ids[2:], lab[2:], fl)])
    ref_loss, ref_g = _oracle(cfg, sd, pvs, rows, labs, w)
    assert abs(out.loss.item() - ref_loss) < 5e-3, (out.loss.item(), ref_loss)
    grads = m.named_grads()
    for k in KEYS:
        rel, cos = _rel(grads[k], ref_g[k])
        print(f'GA 2 x 2: {k} rel {rel:.4g} cos {cos:.6f}')
        assert rel < 4e-2 and cos > 0.999, (k, rel, cos)


def test_one_pass_per_step_is_counted(golden_model, monkeypatch):
    """A count, not a time: with four samples the batch-rows step issues no `grad_accumulate` and ONE varlen attention forward (and backward) per layer; the
    default path issues four causal forwards per layer and accumulates."""
    from vlaser_amd import ops
    cfg, _, sd = golden_model
    pv, ids, lab, rows, labs, pvs = _four_samples(cfg)
    counts = {}

    def counted(name):
        fn = getattr(ops, name)

        def wrapper(*a, **kw):
            counts[name] = counts.get(name, 0) + 1
            return fn(*a, **kw)
        monkeypatch.setattr(ops, name, wrapper)

    for name in ('grad_accumulate', 'attn_varlen', 'attn_bwd_varlen', 'attn_prefill', 'attn_bwd'):
        counted(name)
    Lyr = cfg.llm.num_hidden_layers
    m = _model(cfg, sd, ids.shape[1], batch_rows=True)
    counts.clear()
    m.train_step([(pv, ids, lab, FLAGS4)])
    llm_causal = counts.get('attn_bwd', 0)                                   # (the ViT's attention goes through attn_prefill too: count the LLM by its backward)
    assert counts.get('grad_accumulate', 0) == 0 and counts.get('attn_varlen', 0) == Lyr and counts.get('attn_bwd_varlen', 0) == Lyr and llm_causal == 0, counts
    m = _model(cfg, sd, ids.shape[1])
    counts.clear()
    m.train_step([(pv, ids, lab, FLAGS4)])
    assert counts.get('grad_accumulate', 0) > 0 and counts.get('attn_varlen', 0) == 0 and counts.get('attn_bwd', 0) == 4 * Lyr, counts


def test_zero_supervised_positions_keep_the_zero_gradient_path(golden_model):
    cfg, _, sd = golden_model
    pv, ids, lab, rows, labs, pvs = _four_samples(cfg)
    m = _model(cfg, sd, ids.shape[1], batch_rows=True)
    m.train_step([(pv, ids, lab, FLAGS4)])                                   # leaves gradients behind
    out = m.train_step([(pv, ids, torch.full_like(lab, -100), FLAGS4)])
    assert out.loss.item() == 0.0 and out.grad_norm.item() == 0.0 and not bool(m.fp.g.any())


# ------------------------------------------------------------------------------------------------ data parallel (world size 1, forced exchange)
def _dp_steps(pg):
    from vlaser_amd import config as C, synth
    from vlaser_amd.sft import SFTModel
    cfg = C.truncated(C.vlaser_2b(), 1, 2)
    m = SFTModel(cfg, max_seq_len=320, lr=1e-3, max_grad_norm=1.0, process_group=pg, bucket_layers=1, batch_rows=True)
    m.load_state_dict(synth.vlm_state_dict(cfg, device='cuda'))
    pv, ids, lab, rows, labs, pvs = _four_samples(cfg, seed=5)
    outs = [m.train_step([(pv, ids, lab, FLAGS4)]) for _ in range(2)]
    m.wait_optimizer()
    torch.cuda.synchronize()
    return m, [float(o.loss) for o in outs], [float(o.grad_norm) for o in outs]


def _dp_worker(rank, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), VLASER_FORCE_DP='1', HSA_ENABLE_IPC_MODE_LEGACY='0', VLASER_DP_EXCHANGE='pg')
    # the single-rank reference takes the gradient norm from the gradient buffer, like the data-parallel path (tests/test_rccl_world1_gpu.py)
    os.environ['VLASER_SFT_NO_FUSED_NORM'] = '1'
    torch.set_grad_enabled(False)
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1)
    a, la, na = _dp_steps(None)
    b, lb, nb = _dp_steps(dist.group.WORLD)
    assert not a.dp_active and b.dp_active and a.batch_rows and b.batch_rows
    res = dict(same_p=torch.equal(a.fp.p, b.fp.p), same_m=torch.equal(a.m, b.m), same_v=torch.equal(a.v, b.v), same_master=torch.equal(a.master, b.master),
               la=la, lb=lb, na=na, nb=nb)
    torch.save(res, os.path.join(out_dir, 'res.pt'))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_batch_rows_steps_with_the_exchange_are_bit_identical_to_no_dp(tmp_path):
    """The way tests/test_rccl_world1_gpu.py checks the exchange: a fresh child process, world size 1, VLASER_FORCE_DP=1, `pg` exchange -- two batch-rows
    steps are bit-identical to the same steps without a process group (each bucket is exchanged once per step, in the same order)."""
    import torch.multiprocessing as mp
    port = 29700 + (os.getpid() % 50)
    mp.spawn(_dp_worker, args=(port, str(tmp_path)), nprocs=1, join=True)
    r = torch.load(tmp_path / 'res.pt')
    assert r['la'] == r['lb'] and r['na'] == r['nb'], r
    assert r['same_p'] and r['same_m'] and r['same_v'] and r['same_master'], r


# ------------------------------------------------------------------------------------------------ full size
def test_full_size_batch_rows_vs_sequential():
    """2B widths, 28 layers, 4 x 560 tokens: batch-rows against the one-sample-at-a-time path of the same build on the same batch -- the loss and the gradient
    tensors tests/test_fullsize_gpu.py samples.  Each path is granted that file's bound against the fp32 oracle, so the two may differ by twice it (triangle
    inequality): loss 2 x 2.5e-3, relative Frobenius error 2 x GRAD_REL, cosine deviation 2 x (1 - GRAD_COS).  (The CPU oracle at 4 x full depth is too slow.)"""
    from test_fullsize_gpu import GRAD_COS, GRAD_REL
    from vlaser_amd import config as C, synth
    from vlaser_amd.sft import SFTModel
    torch.set_grad_enabled(False)
    cfg = C.vlaser_2b()
    sd = synth.vlm_state_dict(cfg, device='cuda', dtype=BF)
    g = torch.Generator().manual_seed(79)
    S, B = 560, 4
    ids = torch.stack([torch.cat([torch.randint(1, 151643, (41,), generator=g), torch.full((256,), cfg.img_context_token_id),
                                  torch.randint(1, 151643, (S - 41 - 256,), generator=g)]) for _ in range(B)])
    labels = torch.full_like(ids, -100); labels[:, -128:] = ids[:, -128:]
    pv = torch.randn(B, 3, 448, 448, generator=g)
    L_ = 'language_model.model.layers.'
    keys = ['language_model.lm_head.weight', 'language_model.model.norm.weight', 'mlp1.1.weight']
    for i in (27, 14, 0):
        keys += [f'{L_}{i}.self_attn.q_proj.weight', f'{L_}{i}.self_attn.v_proj.weight', f'{L_}{i}.mlp.down_proj.weight']
    res = []
    for br in (False, True):
        m = SFTModel(cfg, max_seq_len=576, lr=0.0, weight_decay=0.0, max_grad_norm=1.0, batch_rows=br)
        m.load_state_dict(sd)
        out = m.train_step([(pv, ids, labels, torch.ones(B, 1, dtype=torch.long))])
        ng = m.named_grads()
        res.append((out.loss.item(), out.grad_norm.item(), {k: ng[k].double().flatten().cpu() for k in keys}))
        del m, ng
        torch.cuda.empty_cache()
    (la, na, ga), (lb, nb, gb) = res
    print(f'full size 4 x 560: loss sequential {la:.6f} batch rows {lb:.6f}; grad norm {na:.6f} / {nb:.6f}')
    assert abs(la - lb) < 2 * 2.5e-3, (la, lb)
    for k in keys:
        a, b = ga[k], gb[k]
        rel = ((b - a).norm() / (a.norm() + 1e-30)).item()
        cos = (torch.dot(a, b) / (a.norm() * b.norm() + 1e-300)).item()
        print(f'full size 4 x 560: {k} rel {rel:.4g} cos {cos:.6f}')
        assert rel < 2 * GRAD_REL.get(k, GRAD_REL['default']), (k, rel)
        assert cos > 1 - 2 * (1 - GRAD_COS.get(k, GRAD_COS['default'])), (k, cos)
