"""GPU: the row tiles of vlaser_chain_attn.  With more than 16 (q head, token) rows per kv head the launch gives each 16-row MFMA tile a wave of its own
(grid.y = 2 splits + tile); with <= 16 rows the second tile is not computed.  No row reads another row's result, so which wave holds a row must not change
one stored byte:
  row independence   a launch of sq tokens leaves, in every split, the (m, l) pairs and the bf16 rows of sq launches of ONE token over the same cache
  one-tile path      rows >= group * tokens keep their sentinel in every split
  against fp64       the splits merged in fp64 (weights l 2^(m - max m)) against the fp64 attention, element by element (tests/bounds.py): P and the rows are
                     rounded to bf16 -- |got - ref| <= ULP |ref| + ULP (1 + 2^-6) ref_abs + FLOOR, the criterion of tests/test_fwd_ops_gpu.py for the same
                     kernel; the fp32 error of a score (U (hd / 32 + 12) |s| ln 2 relative on p, < 2^-16 here) is far inside the second term
  through o_proj     vlaser_chain_oproj over the same partials == merge (fp32 torch) -> bf16 -> GEMV, to the bound of tests/test_ops_gpu.py's chain o_proj test
"""
import math

import pytest
import torch

from bounds import BF, F32, FLOOR, SENT, ULP, Worst, dev, f32s, h64, is_sent, pow2, randb, same_bits, sentinel

pytestmark = pytest.mark.gpu
N_Q, N_KV, HD = 12, 2, 128
G = N_Q // N_KV
FMIN = torch.finfo(torch.float32).min


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vlaser_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def _grad_off():
    with torch.no_grad():
        yield


def _inputs(B, sq, kv_len, ld, seed):
    """q [B, sq, n_q, hd] (one zero query, one peaky), K [B, n_kv, ld, hd] (rows >= kv_len: garbage no row may see), V key-scaled by 2^e, zero beyond kv_len"""
    q = randb(B, sq, N_Q, HD, seed=seed)
    if sq >= 3:
        q[:, 1], q[:, 2] = 0, q[:, 2] * 4
    k = randb(B, N_KV, ld, HD, seed=seed + 1)
    k[:, :, kv_len:] = 3.0
    v = randb(B, N_KV, ld, HD, seed=seed + 2) * pow2(ld)[None, None, :, None]
    v[:, :, kv_len:] = 0
    return q, k, v


def _vis(B, sq, kv_len, valid, blk, first):
    """PREFIX: key j < valid_len[b], or blk_start <= j < kv_len -- for token 0 only up to first_tok_kv_len when that is set"""
    j = torch.arange(kv_len)[None, None, :]
    vis = ((j < torch.tensor(valid)[:, None, None]) | (j >= blk)).expand(B, sq, kv_len).clone()
    if first:
        vis[:, 0] &= (j[0] < torch.tensor(valid)[:, None]) | (j[0] < first)
    return vis


def _ref64(q, k, v, kv_len, scale, vis, add=None):
    """fp64 attention: out, sum_j p_j |v_j|  [B, sq, n_q, hd]"""
    qh = q.double().permute(0, 2, 1, 3)
    kh, vh = k[:, :, :kv_len].double().repeat_interleave(G, 1), v[:, :, :kv_len].double().repeat_interleave(G, 1)
    s = scale * (qh @ kh.transpose(-1, -2))
    if add is not None:
        s = s + add[:, None].double()
    P = torch.softmax(s.masked_fill(~vis[:, None], -math.inf), -1)
    return (P @ vh).permute(0, 2, 1, 3), (P @ vh.abs()).permute(0, 2, 1, 3)


def _rows_to_heads(t, B, sq):
    """partial rows r = hg * sq + tok of every kv head [B, n_kv, 32, 128] -> [B, sq, n_q, 128]"""
    return t[:, :, :G * sq].reshape(B, N_KV, G, sq, HD).permute(0, 3, 1, 2, 4).reshape(B, sq, N_KV * G, HD)


class _Cache:
    """device copies of one (q, K, V^T) set and the launches over it; the argument block holds raw pointers, so the tensors live here"""

    def __init__(self, ops, q, k, v, kv_len, ld, valid=None, dense=None):
        from vlaser_amd import _lib as L
        self.ops, self.L, self.B, self.sq, self.kv_len, self.ld = ops, L, q.shape[0], q.shape[1], kv_len, ld
        self.q, self.k, self.vt = dev(q), dev(k), dev(v.transpose(-1, -2))
        self.valid = None if valid is None else torch.tensor(valid, dtype=torch.int32).cuda()
        self.dense = dense
        self.nsp = ops.chain_attn_splits(kv_len)
        self.scale = f32s(HD ** -0.5)

    def launch(self, tok0, n_tok, blk=0, first=0):
        """tokens tok0 .. tok0 + n_tok of the set as one launch into fresh sentinel buffers; returns ((m, l) [B, n_kv, nsp, 32, 2], rows [B, n_kv, nsp, 32, 128])"""
        B, nsp, sq, ld = self.B, self.nsp, self.sq, self.ld
        n_el = B * N_KV * nsp * 32
        ml = torch.full((n_el * 2 + 64,), SENT, dtype=F32, device='cuda')
        po = sentinel(n_el * HD + 4096)
        strides = ((sq * N_Q * HD, HD, N_Q * HD), (N_KV * ld * HD, ld * HD), (N_KV * HD * ld, HD * ld))
        kw = dict(dense_mask=self.dense[:, tok0:tok0 + n_tok]) if self.dense is not None else dict(valid_len=self.valid, blk_start=blk, first_tok_kv_len=first)
        a = self.ops.attn_skinny_args(self.q[:, tok0:], self.k, self.vt, (ml, ml, po), B, n_tok, self.kv_len, N_Q, N_KV, HD, *strides, ld, self.scale,
                                      self.L.ATTN_DENSE if self.dense is not None else self.L.ATTN_PREFIX, nsp, **kw)
        self.ops.launch_chain_attn(a)
        torch.cuda.synchronize()
        assert is_sent(ml[n_el * 2:]) and is_sent(po[n_el * HD:]), 'partials written behind the last split'
        ml_, po_ = ml[:n_el * 2].view(B, N_KV, nsp, 32, 2), po[:n_el * HD].view(B, N_KV, nsp, 32, HD)
        nr = G * n_tok
        assert is_sent(ml_[..., nr:, :]) and is_sent(po_[..., nr:, :]), 'partial rows >= group * tokens written'
        self.raw = (ml, po)
        return ml_, po_


def _assert_rows_of_single_token_launches(c, sq, blk, first):
    ml, po = c.launch(0, sq, blk, first)
    for t in range(sq):
        ml1, po1 = c.launch(t, 1, blk, first if t == 0 else 0)
        rows = torch.arange(G) * sq + t
        assert same_bits(ml[:, :, :, rows], ml1[:, :, :, :G]), f'(m, l) of token {t} differ from its own launch'
        assert same_bits(po[:, :, :, rows], po1[:, :, :, :G]), f'rows of token {t} differ from its own launch'


@pytest.mark.parametrize('sq,first', [(4, 0), (5, 65)])
def test_rows_do_not_depend_on_their_wave(ops, sq, first):
    """24 / 30 rows = two tiles, one wave each; 70 keys = 3 chunks in 2 splits with a ragged last chunk; token 0 of the 30-row launch with its own key limit"""
    kv_len, ld = 70, 96
    q, k, v = _inputs(1, sq, kv_len, ld, seed=sq)
    c = _Cache(ops, q, k, v, kv_len, ld, valid=[41])
    assert c.nsp == 2
    _assert_rows_of_single_token_launches(c, sq, 64, first)


@pytest.mark.parametrize('sq', [1, 2])
def test_one_tile_leaves_the_second_alone(ops, sq):
    """6 / 12 rows: nothing is written for the tile without a row (nor for the rows of the first tile behind the last one -- checked in _Cache.launch);
    the rows that are written are those of the single-token launches"""
    kv_len, ld = 70, 96
    q, k, v = _inputs(1, sq, kv_len, ld, seed=10 + sq)
    c = _Cache(ops, q, k, v, kv_len, ld, valid=[41])
    ml, po = c.launch(0, sq, 64, 0)
    assert is_sent(ml[..., 16:, :]) and is_sent(po[..., 16:, :]), 'the second row tile was written'
    assert is_sent(ml[..., G * sq:, :]) and is_sent(po[..., G * sq:, :])
    assert not bool((ml[..., :G * sq, :] == SENT).any()), 'a live row was not written'
    _assert_rows_of_single_token_launches(c, sq, 64, 0)


def _merge_and_bound(worst, tag, ml, po, B, sq, ref, ref_abs, vis, kv_len):
    nr = G * sq
    m64, l64, o64 = h64(ml[..., :nr, 0]), h64(ml[..., :nr, 1]), h64(po[..., :nr, :])
    n_dead = 0
    for s in range(ml.shape[2]):
        lo, hi = min(s * 64, kv_len), min((s + 1) * 64, kv_len)
        for b in range(B):
            if not bool(vis[b, :, lo:hi].any()):
                n_dead += 1
                assert bool((l64[b, :, s] == 0).all()) and bool((o64[b, :, s] == 0).all()), f'split {s} of batch element {b} sees no key: l and the rows must be 0'
    assert n_dead >= 1
    w = l64 * torch.exp2(m64 - m64.amax(2, keepdim=True))
    merged = (o64 * w[..., None]).sum(2) / w.sum(2)[..., None]
    worst.add(tag + '.merged', _rows_to_heads(merged, B, sq), ref, ULP * ref.abs() + ULP * (1 + 2.0 ** -6) * ref_abs + FLOOR, tag)


def test_two_tiles_against_fp64_prefix(ops):
    """the Euler phase's shape (24 rows, 389 keys = 7 splits, a valid prefix per batch element + the trailing block); batch element 1 sees 20 keys: splits 1 .. 5
    are fully masked"""
    B, sq, kv_len, blk, ld, valid = 2, 4, 389, 384, 448, [277, 20]
    q, k, v = _inputs(B, sq, kv_len, ld, seed=389)
    c = _Cache(ops, q, k, v, kv_len, ld, valid=valid)
    assert c.nsp == 7
    vis = _vis(B, sq, kv_len, valid, blk, 0)
    ref, ref_abs = _ref64(q, k, v, kv_len, c.scale, vis)
    ml, po = c.launch(0, sq, blk, 0)
    worst = Worst()
    _merge_and_bound(worst, 'chain_attn_rowtiles[prefix]', ml, po, B, sq, ref, ref_abs, vis, kv_len)
    worst.flush()


def test_two_tiles_against_fp64_dense(ops):
    """the same through VL_ATTN_DENSE: the prefix pattern as a mask, + a hole over the whole of split 1 (keys 64 .. 127) and scattered ones, + a finite bias
    on every visible key (a different one per token)"""
    B, sq, kv_len, blk, ld, valid = 2, 4, 389, 384, 448, [277, 20]
    q, k, v = _inputs(B, sq, kv_len, ld, seed=390)
    g = torch.Generator().manual_seed(5)
    vis = _vis(B, sq, kv_len, valid, blk, 0)
    vis[:, :, 64:128] = False
    vis &= torch.rand(B, sq, kv_len, generator=g) >= 0.2
    vis[:, :, 3] = True
    bias = (torch.randn(B, sq, kv_len, generator=g) * 2.0).to(F32)
    slot = torch.full((B, sq + 2, ld), -3.0e38, dtype=F32)
    slot[:, 1:1 + sq, :kv_len] = torch.where(vis, bias, torch.tensor(FMIN))
    slot = slot.cuda()
    c = _Cache(ops, q, k, v, kv_len, ld, dense=slot[:, 1:1 + sq])
    ref, ref_abs = _ref64(q, k, v, kv_len, c.scale, vis, add=bias)
    ml, po = c.launch(0, sq)
    worst = Worst()
    _merge_and_bound(worst, 'chain_attn_rowtiles[dense]', ml, po, B, sq, ref, ref_abs, vis, kv_len)
    worst.flush()
    # and a dense launch's rows do not depend on their wave either
    for t in range(sq):
        ml1, po1 = c.launch(t, 1)
        rows = torch.arange(G) * sq + t
        assert same_bits(ml[:, :, :, rows], ml1[:, :, :, :G]) and same_bits(po[:, :, :, rows], po1[:, :, :, :G]), f'token {t} differs from its own launch'


def test_two_tiles_through_chain_oproj(ops):
    """the consumer reads rows r = hg * tokens + tok of [B, n_kv, splits, 32, ...]: its slabs over the partials of a two-wave launch against merge (fp32) ->
    bf16 -> GEMV in torch, to the bound of tests/test_ops_gpu.py::test_chain_attn_oproj_vs_fp32 (2e-2 |ref| + 1e-2 max |ref| + 1e-6)"""
    B, sq, kv_len, blk, ld, H, ks = 1, 4, 389, 384, 448, 768, 3
    K = N_Q * HD
    q, k, v = _inputs(B, sq, kv_len, ld, seed=391)
    c = _Cache(ops, q, k, v, kv_len, ld, valid=[277])
    assert ops.chain_oproj_supported(B * sq, H, K, ks, c.nsp, G)
    ml, po = c.launch(0, sq, blk, 0)
    ml_raw, po_raw = c.raw
    wo = randb(H, K, seed=9, std=0.03)
    out = torch.full((ks * B * sq * H + 64,), SENT, dtype=F32, device='cuda')
    o_args, _ = ops.skinny_args(None, ops.pack_skinny(dev(wo), ks, 1), B * sq, out_f32=out, attn_m=ml_raw, attn_o=po_raw, attn_splits=c.nsp, attn_group=G, attn_nq=sq)
    ops.launch_chain_oproj(o_args)
    torch.cuda.synchronize()
    assert is_sent(out[ks * B * sq * H:]), 'o_proj slabs written past [ks, M, N]'
    nr = G * sq
    m, l, o = ml[..., :nr, 0].cpu(), ml[..., :nr, 1].cpu(), po[..., :nr, :].cpu().float()
    w = l * torch.exp2(m - m.amax(2, keepdim=True))
    merged = (o * w[..., None]).sum(2) / w.sum(2)[..., None]
    x = _rows_to_heads(merged, B, sq).reshape(B * sq, K).to(BF).float()
    ref = x @ wo.t()
    got = out[:ks * B * sq * H].view(ks, B * sq, H).sum(0).cpu()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    tol = 1e-2 * ref.abs().max().item() + 1e-6 + 2e-2 * ref.abs()
    assert not bool((err > tol).any()), f'o_proj over the merged partials: max err {err.max().item():.4g} (ref max {ref.abs().max().item():.4g})'
