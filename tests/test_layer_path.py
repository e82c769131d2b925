"""The kernel-path decision of the <= 16-row layers (engine.layer_path) on the CPU: which calls take the csrc/chain.hip kernels, which keep the csrc/skinny.hip
ones, for the three shipped stacks.  Needs the built library (its *_supported predicates are host functions), no GPU."""
import pytest

from vlaser_amd import config as C
from vlaser_amd import engine as E

CHAIN = ('qkv16', 'gu16', 'chain')
STACKS = {'expert': lambda: C.VLAConfig(base=C.vlaser_2b()).expert, '2b': lambda: C.vlaser_2b().llm, '8b': lambda: C.vlaser_8b().llm}


def _path(stack, opts, M, tok, kv_len, **kw):
    llm = STACKS[stack]()
    return E.layer_path(**E.path_geometry(llm, opts), act_width=E.stack_geometry(llm)[4], M=M, tok_per_batch=tok, kv_len=kv_len, **kw)


def test_stack_geometry():
    """(H, I, nq / nkv) and what QwenStack derives from them: o_proj / down units (1 = 16 rows, 2 = 32), their split-K factors, the padded MLP width."""
    dims = lambda llm: (llm.hidden_size, llm.intermediate_size, llm.num_attention_heads, llm.num_key_value_heads)
    assert dims(STACKS['expert']()) == (768, 8960, 12, 2) and dims(STACKS['2b']()) == (1536, 8960, 12, 2) and dims(STACKS['8b']()) == (3584, 18944, 28, 4)
    # (tpu_o, ks_o, tpu_down, ks_down, I_pad)
    assert E.stack_geometry(STACKS['expert']()) == (1, 3, 1, 5, 8960)
    assert E.stack_geometry(STACKS['2b']()) == (1, 2, 1, 5, 8960)
    assert E.stack_geometry(STACKS['8b']()) == (2, 2, 2, 5, 20480)


@pytest.mark.parametrize('stack', ['expert', '2b', '8b'])
@pytest.mark.parametrize('opts', [(), CHAIN])
def test_path_geometry_rows_are_pack_skinny_rows(stack, opts):
    """The row counts layer_path is given are the ones ops.pack_skinny pads a matrix of the stack's true row count to (K = 256: one K-step, a CPU tensor)."""
    import torch
    from vlaser_amd import ops
    llm = STACKS[stack]()
    p = E.path_geometry(llm, opts)
    for n, tpu, key in [((llm.num_attention_heads + 2 * llm.num_key_value_heads) * llm.head_dim, 1 if 'qkv16' in opts else 2, 'n_qkv'),
                        (2 * llm.intermediate_size, p['tpu_gu'], 'n_gu'), (llm.hidden_size, p['tpu_o'], 'n_o')]:
        w = ops.pack_skinny(torch.zeros(n, 256, dtype=torch.bfloat16), 1, tpu)
        assert (w.N, w.tpu, w.n_valid) == (p[key], tpu, n)


@pytest.mark.parametrize('stack,opts,M,tok,kv_len,kw,want', [
    ('expert', CHAIN, 4, 4, 389, {}, (True, True)),
    ('expert', CHAIN, 5, 5, 389, {}, (True, True)),
    ('expert', CHAIN, 8, 4, 389, {}, (True, True)),
    ('expert', CHAIN, 12, 4, 389, {}, (True, True)),
    ('expert', CHAIN, 16, 4, 389, {}, (True, True)),
    ('expert', CHAIN, 6, 6, 391, {}, (True, False)),                                # 36 rows per kv head: more than the two MFMA tiles of the chain attention
    ('expert', CHAIN, 1, 1, 385, dict(skip_post_attn=True), (True, False)),
    ('expert', CHAIN, 4, 4, 389, dict(n_partials=3), (False, False)),               # fp32 slabs of a skinny down projection still to be reduced
    ('expert', CHAIN, 4, 4, 389, dict(input_is_hB=True), (False, False)),
    ('expert', ('qkv16', 'chain'), 4, 4, 389, {}, (True, True)),
    ('expert', ('qkv16', 'chain'), 5, 5, 389, {}, (True, True)),
    ('expert', ('qkv16', 'gu16'), 4, 4, 389, {}, (False, False)),
    ('expert', (), 4, 4, 389, {}, (False, False)),
    ('2b', CHAIN, 1, 1, 300, {}, (True, True)),
    ('2b', CHAIN, 8, 1, 300, {}, (True, True)),
    ('2b', CHAIN, 9, 1, 300, {}, (False, False)),                                   # hidden 1536 x > 8 rows would spill in the chain q/k/v
    ('2b', CHAIN, 16, 1, 300, {}, (False, False)),
    ('2b', CHAIN, 1, 1, 1024, {}, (True, True)),                                    # 16 key splits: the last count the chain attention + o_proj pair is built for
    ('2b', CHAIN, 1, 1, 1025, {}, (True, False)),
    ('2b', CHAIN, 1, 1, 4000, {}, (True, False)),
    ('8b', (), 1, 1, 300, {}, (False, False)),
    ('8b', CHAIN, 1, 1, 300, {}, (False, False)),                                   # MLP width 18944 (workspace padded to 20480): not the width pack_down4 serves
])
def test_layer_path(stack, opts, M, tok, kv_len, kw, want):
    assert _path(stack, opts, M, tok, kv_len, **kw) == want


def test_dense_mask_needs_the_chain_attention():
    assert _path('expert', CHAIN, 4, 4, 389, dense_mask=True) == (True, True)
    assert _path('expert', CHAIN, 1, 1, 385, skip_post_attn=True, dense_mask=True) == (True, False)          # only K / V are written: no attention launch to mask
    for stack, opts, M, tok, kv_len, kw in [('expert', ('qkv16', 'gu16'), 4, 4, 389, {}), ('expert', CHAIN, 6, 6, 391, {}), ('expert', CHAIN, 4, 4, 389, dict(n_partials=3)),
                                            ('2b', CHAIN, 9, 1, 300, {}), ('2b', CHAIN, 1, 1, 1025, {}), ('8b', CHAIN, 1, 1, 300, {})]:
        with pytest.raises(NotImplementedError):
            _path(stack, opts, M, tok, kv_len, dense_mask=True, **kw)
