"""optimizer='adamw8bit' without a GPU: the two code tables, the plan of fp32-slot blocks, and the argument checks of vlaser_adamw8_clipped.

The tables are bitsandbytes' "dynamic map" with 7 exponent bits: decade i = 0..6 holds the midpoints of linspace(0.1, 1, 2^i + 1) (unsigned: 2^(i+1) + 1)
times 10^(i-6); plus 0 and 1; the signed table carries both signs.  That gives 127 positive midpoints, their 127 negatives, 0 and 1: the signed table is
symmetric about its zero at [127] -- signed[127 - k] == -signed[127 + k] for k = 1..127 -- and only 1.0 at [255] has no partner.  (The request for this
feature stated the symmetry one index off, signed[127 - k] == -signed[128 + k] with -0.99296874, 5.5e-7 and 1.0 unpaired; its own formula and its own
spot values, all of which hold below, contradict that: -5.5e-7 sits at [126], 5.5e-7 at [128], and -0.99296874 = -signed[254].)"""
import numpy as np
import pytest
import torch


def _tables_fp64():
    out = []
    for signed in (True, False):
        vals = [0.0, 1.0]
        for i in range(7):
            b = np.linspace(0.1, 1, (2 ** i if signed else 2 ** (i + 1)) + 1)
            mid = (b[:-1] + b[1:]) / 2 * 10.0 ** (i - 6)
            vals += list(mid) + (list(-mid) if signed else [])
        out.append(np.sort(np.array(vals, dtype=np.float64)))
    return out


def test_code_tables():
    from vlaser_amd import ops
    signed, unsigned = ops.adamw8_codes()
    ref_s, ref_u = _tables_fp64()
    for t, ref in ((signed, ref_s), (unsigned, ref_u)):
        assert t.dtype == torch.float32 and t.shape == (256,)
        assert np.array_equal(t.numpy(), ref.astype(np.float32))
        assert bool((t[1:] > t[:-1]).all())
    f32 = lambda x: float(np.float32(x))
    assert signed[0].item() == f32(-0.99296875) and abs(signed[0].item() - -0.99296874) < 1e-8
    assert signed[127].item() == 0.0 and signed[128].item() == f32(5.5e-7) and signed[255].item() == 1.0
    assert unsigned[0].item() == 0.0 and unsigned[1].item() == f32(3.25e-7) and unsigned[254].item() == f32(0.99648437500) and unsigned[255].item() == 1.0
    assert abs(unsigned[254].item() - 0.9964844) < 1e-7
    for k in range(1, 128):
        assert signed[127 - k].item() == -signed[127 + k].item(), k
    assert signed[0].item() == -signed[254].item() and signed[126].item() == -signed[128].item()


def _synthetic_layout(world):
    """tensors of 128, 1536, 4095, 4096, 8960 and 300 000 elements in that order, as a trainer lays them out: a bucket boundary (aligned to 128 x world)
    after the first four, the end padded to 128 x world x 8"""
    from vlaser_amd.param_group import FlatParams, cut_buckets

    class _Flat(FlatParams):
        def finalize(self, pad_to=1):          # offsets only: no buffers (and no device) needed for a plan
            self.n = (self.n + pad_to - 1) // pad_to * pad_to
    fp = _Flat('cpu')
    sizes = (128, 1536, 4095, 4096, 8960, 300000)
    bounds = []
    for i, n in enumerate(sizes):
        fp.add(f't{i}', (n,))
        if i == 3:
            fp.align(128 * world); bounds.append(fp.n)
    fp.finalize(pad_to=128 * world * 8)
    return fp, cut_buckets(bounds + [fp.n]), sizes


@pytest.mark.parametrize('world', [1, 2, 8])
def test_block_plan(world):
    from vlaser_amd import dp
    from vlaser_amd.param_group import plan_state_blocks
    fp, buckets, sizes = _synthetic_layout(world)
    assert all(off % 128 == 0 for _, _, off in fp.specs)
    expect = set()                                          # absolute indices of the fp32 blocks: those of the 128-, 1536- and 4095-element tensors
    for (_, shape, off) in fp.specs:
        if shape[0] in (128, 1536, 4095):
            expect.update(range(off // 128, (off + shape[0] + 127) // 128))
    assert len(expect) == 1 + 12 + 32
    got = {}
    for rank in range(world):
        shards = dp.plan_shards(buckets, world, rank)
        plan = plan_state_blocks(fp.specs, shards)
        assert len(plan) == len(shards)
        for (lo, hi, _), slots in zip(shards, plan):
            assert len(slots) == (hi - lo) // 128
            dense = [k for k in slots if k >= 0]
            assert dense == list(range(len(dense)))         # 0..k-1 in block order, per shard
            assert all(k >= -1 for k in slots)
            for j, k in enumerate(slots):
                b = lo // 128 + j
                assert b not in got
                got[b] = k >= 0
    assert set(got) == set(range(fp.n // 128))              # the ranks' shards tile the buffer
    assert {b for b, f in got.items() if f} == expect       # the same kind for every world: `expect` does not depend on it beyond the padding


def test_block_plan_kind_is_the_same_for_every_world():
    """block -> kind through each tensor's own blocks (the padding between buckets moves with the world size, the tensors' blocks do not)"""
    from vlaser_amd import dp
    from vlaser_amd.param_group import plan_state_blocks
    kinds = []
    for world in (1, 2, 8):
        fp, buckets, _ = _synthetic_layout(world)
        by_block = {}
        for rank in range(world):
            shards = dp.plan_shards(buckets, world, rank)
            for (lo, hi, _), slots in zip(shards, plan_state_blocks(fp.specs, shards)):
                for j, k in enumerate(slots):
                    by_block[lo // 128 + j] = k >= 0
        kinds.append([[by_block[off // 128 + j] for j in range((shape[0] + 127) // 128)] for _, shape, off in fp.specs])
    assert kinds[0] == kinds[1] == kinds[2]
    assert [all(k) for k in kinds[0]] == [True, True, True, False, False, False] and [any(k) for k in kinds[0]] == [True, True, True, False, False, False]


def test_unknown_optimizer_is_refused():
    from vlaser_amd.param_group import check_optimizer
    assert check_optimizer('adamw') == 'adamw' and check_optimizer('adamw8bit') == 'adamw8bit'
    with pytest.raises(ValueError):
        check_optimizer('adam8')


def test_bad_arguments_launch_nothing():
    """every check happens on the host before the launch: the calls return non-zero on a machine without a GPU (and would fault on one if they launched)"""
    from vlaser_amd import _lib
    lib = _lib.lib()
    P = 4096                                                # a "pointer" that passes the NULL / alignment checks and is never dereferenced
    ok = dict(p=P, master=P, mc=P, vc=P, mam=P, vam=P, slot=None, m32=None, v32=None, tm=P, tv=P, g=P, n=128, step=1)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.vlaser_adamw8_clipped(a['p'], a['master'], a['mc'], a['vc'], a['mam'], a['vam'], a['slot'], a['m32'], a['v32'], a['tm'], a['tv'], a['g'],
                                         a['n'], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None, 0.0, a['step'], None)
    for name in ('p', 'master', 'mc', 'vc', 'mam', 'vam', 'tm', 'tv', 'g'):
        assert call(**{name: None}) != 0, name
        assert b'vlaser_adamw8_clipped' in lib.vlaser_last_error()
    assert call(n=0) != 0 and call(n=130) != 0 and call(n=-128) != 0
    assert b'128' in lib.vlaser_last_error()
    assert call(step=0) != 0
    assert call(master=P + 4) != 0
    assert b'alignment' in lib.vlaser_last_error()
    assert call(slot=P) != 0 and call(slot=P, m32=P) != 0 and call(m32=P, v32=P) != 0          # slot / m32 / v32 go together
