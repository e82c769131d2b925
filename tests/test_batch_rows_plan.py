"""`plan_batch_rows` (vlaser_amd/sft.py): the host-side row layout of a per-device batch that runs as one varlen pass.  No GPU: the planner and
`SFTModel._split_batch` (called unbound on a stand-in that carries the two attributes it reads) are pure index bookkeeping.  Also here, because it needs no GPU either: the varlen entry points' host-side argument validation."""
from types import SimpleNamespace

import torch

from test_sft_gpu import _four_samples
from vlaser_amd import config as C
from vlaser_amd.sft import SFTModel, plan_batch_rows


def _cfg():
    return C.truncated(C.vlaser_2b(), 2, 2)


def _split(cfg, pv, ids, lab, flags, am=None):
    return SFTModel._split_batch(SimpleNamespace(cfg=cfg, img_context_token_id=cfg.img_context_token_id), pv, ids, lab, flags, am)


def _check_plan(plan, samples):
    """The properties every plan must have, from the samples alone."""
    lens = [int(s[1].numel()) for s in samples]
    cu = plan.cu_seqlens.tolist()
    assert plan.cu_seqlens.dtype == torch.int32 and plan.pos_ids.dtype == torch.int32
    assert cu == [sum(lens[:b]) for b in range(len(lens) + 1)]
    M = cu[-1]
    assert plan.ids.shape == (M,) and plan.pos_ids.shape == (M,) and plan.targets.shape == (M,)
    R = 0
    for b, s in enumerate(samples):
        lo, hi = cu[b], cu[b + 1]
        ids_b, lab_b = s[1].reshape(-1), s[2].reshape(-1)
        assert torch.equal(plan.ids[lo:hi], ids_b)                                      # trimmed to its own length, no pad rows
        assert plan.pos_ids[lo:hi].tolist() == list(range(hi - lo))                      # positions restart at 0
        assert torch.equal(plan.targets[lo:hi - 1], lab_b[1:])                           # shifted inside the sample
        assert int(plan.targets[hi - 1]) == -100                                         # the last token predicts nothing: no target crosses a boundary
        R += int((lab_b[1:] != -100).sum())
    assert plan.R == R == int(plan.rows.numel()) == sum(s[4] for s in samples)
    assert torch.equal(plan.rows, (plan.targets != -100).nonzero().flatten())


def test_plan_of_the_four_ragged_samples():
    cfg = _cfg()
    pv, ids, lab, rows, labs, pvs = _four_samples(cfg)
    flags = torch.ones(4, 1, dtype=torch.long)
    smp = _split(cfg, pv, ids, lab, flags)
    plan = plan_batch_rows(smp, cfg.img_context_token_id)
    assert plan.cu_seqlens.tolist() == [0, 288, 589, 866, 1161]
    _check_plan(plan, smp)
    assert plan.R == int(sum((l[1:] != -100).sum() for l in labs))
    # the samples back to back are exactly the un-padded rows of the collated batch
    assert torch.equal(plan.ids, torch.cat(rows))
    # tile ranges: the samples' tiles, concatenated in order, are the batch's tiles (what the one ViT pass consumes)
    assert torch.equal(torch.cat([s[0] for s in smp]), pv)
    assert [int(s[0].shape[0]) for s in smp] == [1, 1, 1, 1]
    # every <IMG_CONTEXT> row of the plan corresponds to one visual token of those tiles
    assert plan.n_img == int((plan.ids == cfg.img_context_token_id).sum()) == 4 * cfg.num_image_token


def test_plan_edge_cases():
    """A text-only sample with its dummy tile, a sample of length 1, a sample whose last id is 0 ("!") under a supervised label."""
    cfg = _cfg()
    img, nt = cfg.img_context_token_id, cfg.num_image_token
    g = torch.Generator().manual_seed(3)
    a = torch.cat([torch.randint(1, 1000, (5,), generator=g), torch.full((nt,), img), torch.randint(1, 1000, (7,), generator=g)])      # one real tile
    b = torch.randint(1, 1000, (9,), generator=g)                                                                                       # text only
    c = torch.tensor([17])                                                                                                               # length 1
    d = torch.cat([torch.randint(1, 1000, (6,), generator=g), torch.tensor([0])])                                                        # ends in id 0
    la = torch.full_like(a, -100); la[-4:] = a[-4:]
    lb = torch.full_like(b, -100); lb[-3:] = b[-3:]
    lc = torch.tensor([17])              # a supervised label on a sample's only token: nothing predicts it
    ld = torch.full_like(d, -100); ld[-2:] = d[-2:]
    S = max(map(len, (a, b, c, d)))
    ids = torch.zeros(4, S, dtype=torch.long); lab = torch.full((4, S), -100)
    for i, (x, l) in enumerate(((a, la), (b, lb), (c, lc), (d, ld))):
        ids[i, :len(x)] = x; lab[i, :len(x)] = l
    pv = torch.randn(4, 3, 8, 8, generator=g)                            # (tile contents are irrelevant to the plan)
    flags = torch.tensor([[1], [0], [0], [0]])                           # b, c, d are text-only: one dummy tile each
    smp = _split(cfg, pv, ids, lab, flags)
    assert [int(s[1].numel()) for s in smp] == [len(a), len(b), 1, len(d)]      # d keeps its trailing id 0 (it carries a label)
    plan = plan_batch_rows(smp, img)
    _check_plan(plan, smp)
    assert plan.R == 4 + 3 + 0 + 2
    cu = plan.cu_seqlens.tolist()
    assert int(plan.ids[cu[4] - 1]) == 0 and int(plan.targets[cu[4] - 2]) == 0          # the supervised "!" is predicted from inside its own sample
    assert not bool(((plan.rows >= cu[2]) & (plan.rows < cu[3])).any())                 # the length-1 sample supervises nothing
    assert int(plan.targets[cu[2] - 1]) == -100                                          # ... and sample b's last token does not predict its token
    # tile ranges as `_split_batch` cut them: one tile per sample, in order
    assert [tuple(s[3].reshape(-1).tolist()) for s in smp] == [(1,), (0,), (0,), (0,)]
    assert torch.equal(torch.cat([s[0] for s in smp]), pv)


def test_plan_refuses_inconsistent_samples():
    import pytest
    ids = torch.tensor([[5, 6, 7]]); lab = torch.tensor([[-100, 6, 7]])
    with pytest.raises(ValueError):
        plan_batch_rows([(None, ids, lab, None, 1)], 3)                  # R_b does not match the labels
    with pytest.raises(ValueError):
        plan_batch_rows([(None, ids, lab[:, :2], None, 1)], 3)


def test_varlen_entry_points_refuse_bad_arguments_before_any_launch():
    """The C ABI's host-side validation (no GPU needed, as tests/test_layout.py::test_bad_arguments_return_errors_not_crashes): more rows than cache slots,
    head_dim other than 128, a null boundary table."""
    import ctypes
    from vlaser_amd import _lib
    lib = _lib.lib()
    P = 4096
    a = _lib.AttnArgs()
    a.q = a.k = a.vt = a.out = P
    a.batch, a.sq, a.kv_len, a.n_q_heads, a.n_kv_heads, a.head_dim, a.ld_vt = 1, 200, 200, 12, 2, 128, 128
    assert lib.vlaser_attn_varlen(ctypes.byref(a), P, 2, None) != 0
    assert b'exceed the cache' in lib.vlaser_last_error()
    assert lib.vlaser_attn_varlen(ctypes.byref(a), None, 2, None) != 0
    assert b'null' in lib.vlaser_last_error()
    a.head_dim = 64
    assert lib.vlaser_attn_varlen(ctypes.byref(a), P, 2, None) != 0
    assert b'head_dim 64' in lib.vlaser_last_error()
    assert lib.vlaser_attn_bwd_varlen(P, P, P, P, P, P, P, P, P, P, 200, 12, 2, 128, 0.1, P, 2, 128, None) != 0
    assert b'exceed the cache' in lib.vlaser_last_error()
    assert lib.vlaser_attn_bwd_varlen(P, P, P, P, P, P, P, P, P, P, 64, 12, 2, 100, 0.1, P, 2, 128, None) != 0
    assert b'bad geometry' in lib.vlaser_last_error()
    assert lib.vlaser_attn_bwd_varlen(P, P, P, P, P, P, P, P, P, P, 64, 12, 2, 128, 0.1, P, 2, 64, None) != 0
    assert b'head_dim 64' in lib.vlaser_last_error()
    assert lib.vlaser_attn_bwd_varlen(P, P, P, P, P, P, P, P, P, P, 64, 12, 2, 128, 0.1, None, 2, 128, None) != 0
    assert b'null' in lib.vlaser_last_error()
