"""Host-side checks (no GPU) of the one weight-format axis of the chain MLP: ops.chain_down_args builds the struct of either format and carries the one copy of the
operand asserts, ops.launch_chain_down / launch_chain_down_looped pick the library entry by the struct's class (a bad shape is refused by the library before any
launch), and the predicates of ops.CHAIN_FORMATS are the library's."""
import pytest
import torch

from vlaser_amd import _lib as L, ops

BF = torch.bfloat16
M, N, K = 5, 768, 8960


def _operands():
    x, res, out = torch.zeros(16, K + 64, dtype=BF), torch.zeros(M, N, dtype=BF), torch.zeros(M, N, dtype=BF)
    return x, res, out, torch.zeros(N * K, dtype=BF), torch.zeros(N * K, dtype=torch.uint8), torch.ones(N // 3, 4)


def test_chain_down_args_builds_either_struct():
    x, res, out, w4, w8, s4 = _operands()
    a = ops.chain_down_args(x, w4, res, out, M, N, K)
    assert type(a) is L.ChainDownArgs
    b = ops.chain_down_args(x, w8, res, out, M, N, K, s4)
    assert type(b) is L.ChainDownW8Args and b.w_scale == s4.data_ptr()
    for s, W in ((a, w4), (b, w8)):
        assert (s.x, s.ldx, s.W, s.res, s.h_out, s.M, s.N, s.K, s.dbg) == (x.data_ptr(), K + 64, W.data_ptr(), res.data_ptr(), out.data_ptr(), M, N, K, None)
        assert any(t is W for t in s._keep) and any(t is x for t in s._keep)          # the struct keeps what it points at alive
    s = torch.zeros(8, dtype=torch.int64)
    a.dbg = s.data_ptr()                                                              # tools set it after the struct is built
    assert a.dbg == s.data_ptr()


def test_chain_down_args_refuses_bad_operands():
    x, res, out, w4, w8, s4 = _operands()
    bad = [dict(res=out),                                          # res is h_out
           dict(x=torch.zeros(K, 16, dtype=BF).t()),               # inner stride != 1
           dict(x=x.float()),
           dict(scale4=s4.double(), W=w8),
           dict(scale4=torch.ones(4, N // 3).t(), W=w8),           # not contiguous
           dict(scale4=s4, W=w4)]                                  # scales with bf16 weights
    for kw in bad:
        args = dict(x=x, W=w4, res=res, h_out=out, M=M, N=N, K=K, scale4=None)
        args.update(kw)
        with pytest.raises(AssertionError):
            ops.chain_down_args(**args)


@pytest.mark.parametrize('w8', [False, True], ids=['bf16', 'e4m3'])
def test_launchers_go_by_the_struct_and_the_library_validates_first(w8):
    """M = 17: no entry is built for it, and the library says so before any launch -- no GPU needed (stream 0 is never used)."""
    x, res, out, w4, w8t, s4 = _operands()
    a = ops.chain_down_args(x, w8t if w8 else w4, res, out, 17, N, K, s4 if w8 else None)
    for launch, entry in ((ops.launch_chain_down, 'vlaser_chain_down'), (ops.launch_chain_down_looped, 'vlaser_chain_down_looped')):
        with pytest.raises(L.VlaserHipError, match='built for') as e:
            launch(a, stream=0)
        assert (entry + ('_w8' if w8 else '')) in str(e.value)
    if w8:          # the W8 entries were reached: only they look at the scales
        a.w_scale = None
        with pytest.raises(L.VlaserHipError, match='null w_scale'):
            ops.launch_chain_down(a, stream=0)


def test_format_table_predicates_are_the_librarys():
    lib = L.lib()
    bf, e8, e8k = ops.chain_format('bf16', 768), ops.chain_format('e4m3', 768), ops.chain_format('e4m3', 1536)
    assert ops.chain_format('bf16', 1536) is bf and ops.chain_format('e4m3', 3584) is e8 and set(ops.CHAIN_FORMATS) == {('bf16', None), ('e4m3', None), ('e4m3', 1536)}
    assert (bf.gu_supported, bf.launch_gu, bf.down_supported) == (ops.chain_gu_supported, ops.launch_chain_gu, ops.chain_down_supported)
    assert (e8.gu_supported, e8.launch_gu, e8.down_supported) == (ops.chain_gu_w8_supported, ops.launch_chain_gu_w8, ops.chain_down_w8_supported)
    assert (e8k.gu_supported, e8k.launch_gu, e8k.down_supported) == (ops.chain_gu_w8_k1536_supported, ops.launch_chain_gu_w8_k1536, ops.chain_down_w8_supported)
    assert (bf.guests['gu'], bf.guests['down']) == (L.GUEST_CHAIN_GU, L.GUEST_CHAIN_DOWN) and (e8.guests['gu'], e8.guests['down']) == (L.GUEST_CHAIN_GU_W8, L.GUEST_CHAIN_DOWN_W8)
    assert e8k.guests['gu'] is None and all(f.guests[n] == bf.guests[n] for f in (e8, e8k) for n in ('qkv', 'attn', 'o'))
    for ns in (2, 3, 4, 6):          # the walk of test_fp8_mlp.py::test_w8_predicates_mirror_the_dispatch_tables
        for longest in (1, 2, 3, 4, 5, 6):
            for sp in (1, 2, 3, 4):
                for tpu in (1, 2):
                    s = (4, 16 * tpu * (256 * (longest - 1) + 100), ns * 256, sp, tpu)
                    assert bf.gu_supported(*s) == bool(lib.vlaser_chain_gu_supported(*s)), s
                    assert e8.gu_supported(*s) == bool(lib.vlaser_chain_gu_w8_supported(*s)), s
                    assert e8k.gu_supported(*s) == bool(lib.vlaser_chain_gu_w8_k1536_supported(*s)), s
    for m in range(0, 18):
        for n, k in ((17920, 768), (16416, 768), (17920, 1536)):
            s = (m, n, k, 3 if k == 768 else 2, 1)
            assert bf.gu_supported(*s) == bool(lib.vlaser_chain_gu_supported(*s)) and e8.gu_supported(*s) == bool(lib.vlaser_chain_gu_w8_supported(*s)), s
            assert e8k.gu_supported(*s) == bool(lib.vlaser_chain_gu_w8_k1536_supported(*s)), s
    for m in (0, 1, 4, 5, 8, 9, 13, 16, 17):
        for n in (768, 772, 1536, 770, 1540):
            for k in (8960, 8832, 18944):
                assert bf.down_supported(m, n, k) == bool(lib.vlaser_chain_down_supported(m, n, k)), (m, n, k)
                assert e8.down_supported(m, n, k) == e8k.down_supported(m, n, k) == bool(lib.vlaser_chain_down_w8_supported(m, n, k)), (m, n, k)
