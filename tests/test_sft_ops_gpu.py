"""Op-level parity of the kernels that do most of the arithmetic of an SFT step -- the weight-gradient (TN) GEMMs, the NN dgrad GEMMs with their
SwiGLU-backward epilogue, the fused attention backward, the RMSNorm backward and the column sums, swiglu / swiglu_bwd, AdamW, the embedding gradient and
the transpose -- against fp64 references computed on the CPU from the very bf16 / fp32 tensors the kernel reads (GPU box only; the closed form used as the
attention reference lives in tests/bounds.py and is checked against fp64 autograd, without a GPU, by tests/test_sft_ops_closed_form.py).

Conventions (as tests/test_train_ops_gpu.py, tests/test_fwd_ops_gpu.py): every output goes into a sentinel buffer (spare rows, a padded leading dimension,
spare batch gaps) and everything outside the contract must still be SENT bit for bit; operands carry exact power-of-two row / column scales (2^e,
e cycling over -10 .. 2); every figure is the worst element of |got - ref| / tol (<= 1 passes), logged through tests/parity.py; no element is left out.
ULP = 2^-7 (one bf16 ulp: two half-ulp roundings), U = 2^-24, FLOOR = 2^-100 (the only absolute slack).

Bounds, element by element (ref_abs = the same expression on the absolute values of its terms):
  A  gemm_tn / gemm_tn_lds / gemm_tn_grouped (bf16 out)   ULP |ref| + U n_seq ref_abs + FLOOR,   n_seq = groups x ceil(K / 32) + 10 (groups = 1 outside the grouped form): an MFMA
     16x16x32 adds a 32-term dot product to its accumulator (<= 8 sequential additions in a lane's k-group, 2 levels across the four groups), one
     accumulation per MFMA.  Pad rows of Wt hold +-the largest finite bf16 against zero rows of At: their products are exact zeros, the bound does not move.
     sumsq_part: |sum_fp64(slots) - sum(out_bf16^2)| <= U 48 sum(out_bf16^2): all terms positive; a lane adds at most 32 fragment sums in sequence, each a
     2-level tree over four squares (1 rounding each), then the 6-level wave butterfly: <= 41 roundings, 48 taken.
  B  gemm_nn NONE as A; F32 / PARTIAL (the slabs summed in fp64) without the ULP term, n_seq = K / (32 k_splits) + 10 per slab.
     SWIGLU_BWD: d = bf16(acc) in the kernel, rbf(A B) in the reference; the two may be neighbouring bf16 when the fp32 error crosses a tie:
     e_d = ULP |d| + U n_seq d_abs.  d(gate) = d u sig (1 + g (1 - sig)), d(up) = d g sig in fp32 with __expf:
       tol_dg = 2 ULP |ref| + |u silu'(g)| e_d + 4 U |d u| sig (1 + |g|) + FLOOR     (k = 2 for __expf; the third term: 1 + g (1 - sig) cancels near g = -1.28
                                                                                      and 1 - sig near sig = 1: four fp32 roundings of the un-cancelled terms)
       tol_du = 2 ULP |ref| + |g sig| e_d + FLOOR
     and, bit for bit, the stand-alone swiglu_bwd on the bf16 output of the NONE launch of the same product ("the same expressions, in the same order").
  C  attn_bwd / attn_bwd_varlen, from o = bf16(O) and lse = fp32(log2-sum-exp) computed in fp64 and handed in.  Per (head, query q, key k), n14 = 128/32 + 10:
       P    = exp2(s sc - lse), sc = f32(scale) f32(log2 e)        e_P  = P (ln2 (U n14 s_abs sc + 2 U (|s sc| + |lse|)) + 2 U)     (v_exp_f32: 1 ulp)
       D    = <dO, o>   (delta_ws)                                  e_D  = U 34 sum|dO||o|          (32 sequential FMAs per lane + a 2-level butterfly)
       dP   = <dO, v>                                               e_dP = U n14 sum|dO||v|
       dS   = P (dP - D) scale                                      e_dS = e_P |dP - D| scale + P scale (e_dP + e_D) + 3 U |dS|
     (the second term is the cancelling (dP - D): P scale (sum|dO||v| + sum|dO||o|) times U n), then P and dS are rounded to bf16 for the second product:
       dV_k = sum_q bf16(P) dO_q        tol = ULP |ref| + ULP sum P |dO| + sum e_P |dO| + U n_q sum P |dO| + FLOOR
       dK_k = sum_q bf16(dS) Q_q        tol = ULP |ref| + ULP sum |dS||Q| + sum e_dS |Q| + U n_q sum |dS||Q| + FLOOR
       dQ_q = sum_k bf16(dS) K_k        tol = ULP |ref| + ULP sum |dS||K| + sum e_dS |K| + U n_q sum |dS||K| + FLOOR
     n_q = ceil(S / 32) + 11 (one accumulation per 32 queries / keys, + the merge of the two wave groups).  dk / dv are compared per Q HEAD.
     Keys at or past kv_valid: exact zeros; rows past S: SENT.  A one-token sequence of the varlen form: dq = dk = 0 exactly (documented), dv = dO.
  D  rmsnorm_bwd: dx = dres + rs g - coef x, g = w dy, coef = rs^3 mean(x g): the result cancels on purpose, so
       tol_dx = ULP |ref| + U (3 n_row + 17) (|dres| + rs |g| + rs |xh| mean|g xh|) + FLOOR,    xh = x rs, n_row = 8 ceil(C / 512) + 6
     (one wave per row: 8 additions per 16-byte chunk of a lane, the 6-level butterfly; the dot carries n_row + 3, rs carries n_row / 2 + 3 and enters
     up to three times, the tail ~6: the count of test_layernorm_bwd, whose structure this kernel shares).  The third term is mean|g xh|, not |coef x|:
     sum(x g) cancels, its fp32 error does not.
       dw (bf16)  ULP |ref| + U n_dw sum_s |dy x rs| + FLOOR,  n_dw = 3 (the four rows of a workgroup) + ceil(ceil(S/4) / 16) + 1 (a slice's accumulator
                  chain) + 4 (two 2-level trees) + 2 (the products) + n_row / 2 + 3 (rs);  dw_ws alone (fp32 partials, summed in fp64): n = n_row / 2 + 8
       colsum_mul mode 2 (fp32 out)  U n_cs sum|dy x rs|,  n_cs = 70 + 8 ceil(C/512) + ceil(S/64) + 20 (rowstat_kernel <= 65 adds per lane + 6; <= ceil(S/64)
                  per row lane + 4 + the 16 slices): the count of test_layernorm_bwd's mode 3
       colsum_bf16  ULP |ref| + U (ceil(S / 64) + 19) sum|a| + FLOOR  (a row lane's accumulator chain, a 2-level tree, 16 row lanes in sequence)
  E  swiglu: act = bf16(bf16(silu(g)) u): 2 ULP |ref| + FLOOR, ref = rbf(silu(g)) u (the inner rounding may land on the neighbour: one ulp; the outer: one);
     swiglu_bwd: tol_dg / tol_du of B with e_d = 0.
  F  adamw: fp64 DeepSpeed FusedAdam (adam_w_mode) from the same fp32 state, hyperparameters as the C ABI holds them; gs = g gscale (k_g U: 1 rounding; 5
     with the clip factor: sqrt, +1e-6, /, x):
       tol_m = U (2 |b1 m| + (2 + k_g) |c1 gs|) + FLOOR      c1 = f32(1 - b1); each product one rounding, the sum one (on <= the sum of the terms), gs k_g
       tol_v = U (2 b2 v + (3 + 2 k_g) c2 gs^2) + FLOOR      two products and gs twice
       den = sqrt(v') / sqrt(bc2) + eps:  e_den = e_sqrt rbc2 + sqrt(v') rbc2 (e2 / 2 + 3 U) + U den,   e_sqrt = min(tol_v / sqrt(v'), sqrt(tol_v)) + 2 U sqrt(v')
       upd = (lr / bc1) m' / den:         e_upd = (lr / bc1) (tol_m / den + |m'| e_den / den^2 + 2 U |m' / den|) + |upd| (e1 + 2 U)
       tol_master = 4 U |w decay| + e_upd + U |upd| + U |ref| + FLOOR           (decay = 1 - lr wd: two roundings, the product, the subtraction)
     e1, e2: the bias corrections 1 - powf(b, t) are formed in fp32; a powf within 1 ulp (2 U relative) moves 1 - b^t by 2 U b^t / (1 - b^t), + U for the
     subtraction -- b1 = 0.9 / b2 = 0.999: t = 1: 18 U / 1998 U; t = 2: 8.5 U / 998 U; t = 1000: 0 / 1.2 U; t = 100000: 0 / 0 (+ U each).
     p == bf16(master) bit for bit; everything past n keeps its sentinel.
  G  embed_scatter_add: per element ULP |ref| + U L (|base| + sum|dh|) + FLOOR, L = the run's text positions (a sequential fp32 sum, one addition to the
     table row, one bf16 rounding); untouched rows bit for bit.  sumsq_rows: per slot U 16 sum(row^2) (<= 5 roundings per lane, the butterfly, 3 waves).
  H  transpose: bit for bit.
"""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch

from bounds import (BF, D64, F32, FLOOR, LN_KINDS, LOG2E32, SENT, U, ULP, Worst, _ln_rows, attn_bwd_ref, bound, dev, f32s, h64, is_sent, pow2, randb, rbf, same_bits,
                    sentinel)
from parity import parity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 3.3895313892515355e38                  # the largest finite bf16


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vlaser_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def _grad_off():
    with torch.no_grad():
        yield


def _obuf(rows, ld, dtype=BF, off=0):
    """sentinel buffer [rows, ld] (+ slack on both sides); the view starts `off` elements past the aligned base"""
    flat = torch.full((rows * ld + 16,), SENT, dtype=dtype, device='cuda')
    return flat, flat[off:off + rows * ld].view(rows, ld), off


def _outside_clean(flat, view, o, M, N):
    n = view.numel()
    return is_sent(view[:M, N:]) and is_sent(view[M:]) and is_sent(flat[:o]) and is_sent(flat[o + n:])


def _c8(n):
    return (n + 7) // 8 * 8


def _note(worst, name, fig, where):
    """a figure computed by the test itself, kept like Worst.add keeps its own"""
    if name not in worst.figs or fig > worst.figs[name][0]:
        worst.figs[name] = (fig, where)


def _refused(L, fn, match):
    with pytest.raises(L.VlaserHipError, match=match):
        fn()


# ================================================================================================ A. weight-gradient GEMMs
def _tn_big(M, N, batch=1):
    """mirror of gemm_tn_launch (csrc/gemm.hip): the 128-row tile kernel when it still fills 512 workgroups"""
    return -(-M // 128) * -(-N // 128) * batch >= 512


def _tn_raw(L, At, Wt, out, M, N, K, part=None):
    L.check(L.lib().vlaser_gemm_tn(At.data_ptr(), Wt.data_ptr(), out.data_ptr(), M, N, K, At.stride(0), Wt.stride(0), out.stride(0),
                                   None if part is None else part.data_ptr(), 0 if part is None else part.numel(), None), 'vlaser_gemm_tn')


def _tn_operands(M, N, K, seed, pad_rows=3):
    """At [K, M] / Wt [K, N]: column-offset, row-truncated views of wider buffers whose spare rows hold +-BIG (never read)"""
    a = randb(K, M, seed=seed) * pow2(M)[None]
    w = randb(K, N, seed=seed + 1) * pow2(N, -6, 3)[None]
    big_a = torch.full((K + pad_rows, _c8(M) + 16), BIG)
    big_w = torch.full((K + pad_rows, _c8(N) + 16), -BIG)
    big_a[:K] = 0.5
    big_w[:K] = -0.5                                          # the columns M .. c8(M) of a row are read (they feed dropped outputs): finite
    big_a[:K, 8:8 + M], big_w[:K, 8:8 + N] = a, w
    da, dw = dev(big_a), dev(big_w)
    return a.double(), w.double(), da[:K, 8:8 + M], dw[:K, 8:8 + N]


def _check_slots(name, part, n_written, out_view, where):
    """the first n_written slots add up to the squares of the bf16 values stored; the others keep their sentinel"""
    assert not bool((part[:n_written] == SENT).any()) and is_sent(part[n_written:]), \
        f'{name} {where}: {int((part != SENT).sum())} slots written, expected the first {n_written}'
    want = h64(out_view).pow(2).sum().item()
    got = h64(part[:n_written]).sum().item()
    return abs(got - want) / (U * 48 * want + FLOOR)


@pytest.mark.parametrize('K', [1, 63, 64, 65, 130])
def test_gemm_tn_small_tile(ops, K):
    """The 64-row register-staged kernel, M = 77 / N = 140 (a full and a ragged tile each way, neither a multiple of 8), K = a single row, one short of /
    exactly / one past a tile (the clamped prefetch of a tile that does not exist), an odd number of tiles; ldo % 4 == 0 (8-byte stores) and != 0 (element
    stores, `out` 2 bytes off) give the same bits; sumsq slots."""
    from vlaser_amd import _lib as L
    M, N = 77, 140
    assert not _tn_big(M, N)
    A64, W64, At, Wt = _tn_operands(M, N, K, seed=K)
    ref, ref_abs = A64.t() @ W64, A64.abs().t() @ W64.abs()
    tol = ULP * ref.abs() + U * (K // 32 + 10) * ref_abs + FLOOR
    worst, first = Worst(), None
    n_slots = -(-M // 64) * -(-N // 128) * 4
    for vname, ldo, off in (('vec', N + 4, 0), ('scalar', N + 3, 1), ('scalar-ld141', N + 1, 0)):
        where = f'K={K},{vname}'
        flat, out, o = _obuf(M + 3, ldo, off=off)
        part = torch.full((ops.tn_sumsq_slots(M, N) + 5,), SENT, dtype=F32, device='cuda')
        _tn_raw(L, At, Wt, out, M, N, K, part)
        assert _outside_clean(flat, out, o, M, N), f'{where}: written outside [M, N]'
        worst.add('gemm_tn64', out[:M, :N], ref, tol, where)
        _note(worst, 'gemm_tn64.sumsq', _check_slots('gemm_tn64', part, n_slots, out[:M, :N], where), where)
        if first is None:
            first = out[:M, :N].clone()
        else:
            assert same_bits(out[:M, :N], first), f'{where}: differs from the vector-store path'
    _refused(L, lambda: _tn_raw(L, At, Wt, out, M, N, K, part[:n_slots - 1]), 'slots')
    worst.flush()


@pytest.mark.parametrize('K,ldo_pad,off', [(1, 4, 0), (65, 3, 1)])
def test_gemm_tn_128_row_tile(ops, K, ldo_pad, off):
    """The 128-row kernel at the smallest shape that reaches 512 workgroups (16 x 32 tiles, both edges ragged), a single K row and two K tiles."""
    from vlaser_amd import _lib as L
    M, N = 15 * 128 + 5, 31 * 128 + 12
    assert _tn_big(M, N) and not _tn_big(M - 128, N) and M % 8 and N % 8
    A64, W64, At, Wt = _tn_operands(M, N, K, seed=K + 3)
    ref, ref_abs = A64.t() @ W64, A64.abs().t() @ W64.abs()
    flat, out, o = _obuf(M + 3, N + ldo_pad, off=off)
    n_slots = 16 * 32 * 4
    part = torch.full((n_slots + 5,), SENT, dtype=F32, device='cuda')
    _tn_raw(L, At, Wt, out, M, N, K, part)
    assert _outside_clean(flat, out, o, M, N), 'written outside [M, N]'
    bound(f'gemm_tn128[K={K},ldo=N+{ldo_pad}]', out[:M, :N], ref, ULP * ref.abs() + U * (K // 32 + 10) * ref_abs + FLOOR)
    parity(f'gemm_tn128.sumsq[K={K}]', _check_slots('gemm_tn128', part, n_slots, out[:M, :N], f'K={K}'), 1.0)
    _refused(L, lambda: _tn_raw(L, At, Wt, out, M, N, K, part[:n_slots - 1]), 'slots')


def test_gemm_tn_refuses_misaligned_out(ops):
    """Rows of `out` are stored in 8-byte pieces when ldo % 4 == 0: an `out` (or a batch stride) that breaks their alignment is refused on the host, as is
    ldo < N; an ldo that takes the element stores needs no alignment (test_gemm_tn_small_tile runs it 2 bytes off)."""
    from vlaser_amd import _lib as L
    M, N, K = 16, 16, 8
    At, Wt = dev(randb(K, M)), dev(randb(K, N))
    flat, out, _ = _obuf(M, N + 4, off=1)
    _refused(L, lambda: _tn_raw(L, At, Wt, out, M, N, K), 'out must be 8-byte aligned')
    flat2, out2, _ = _obuf(M, N + 4, off=2)                 # 4 bytes off
    _refused(L, lambda: _tn_raw(L, At, Wt, out2, M, N, K), 'out must be 8-byte aligned')
    flat3, out3, _ = _obuf(2 * M, N + 4)
    _refused(L, lambda: ops.gemm_tn_grouped(At, Wt, out3, M, N, K, M, N, N + 4, 1, 0, 0, 2, 0, 0, M * (N + 4) + 2), 'o_bs a multiple of 4')
    _refused(L, lambda: ops.gemm_tn_grouped(At, Wt, out3, M, N, K, M, N, N - 4, 1, 0, 0, 1, 0, 0, 0), 'is smaller than N')
    assert is_sent(flat) and is_sent(flat2) and is_sent(flat3), 'a refused call wrote'


@pytest.mark.parametrize('K', [5, 83, 130])
def test_gemm_tn_grouped(ops, K):
    """vlaser_gemm_tn_grouped with the strides of the attention backward (At = dS [heads, K queries, ld], Wt = q [K, heads * hd], out = dk [keys, n_kv * hd]):
    groups 1 / 6 / 7, batch 1 / 2 / 4, K rows per group short of / past one tile / two tiles + 2 (the group boundary inside and on a 64-row tile); every
    batch element compared, none summed."""
    M, hd = 77, 128
    ld = _c8(M) + 8
    worst = Worst()
    for groups in (1, 6, 7):
        for batch in (1, 2, 4):
            H = groups * batch
            where = f'K={K},groups={groups},batch={batch}'
            ds = randb(H, K, M, seed=groups) * pow2(M)[None, None]
            q = randb(K, H, hd, seed=batch) * pow2(hd, -4, 2)[None, None]
            ds_buf = torch.full((H, K, ld), 0.25)
            ds_buf[:, :, :M] = ds
            ds_d, q_d = dev(ds_buf), dev(q.reshape(K, H * hd))
            ldo = batch * hd + 4
            flat, out, o = _obuf(M + 3, ldo)
            ops.gemm_tn_grouped(ds_d, q_d, out, M, hd, K, ld, H * hd, ldo, groups, K * ld, hd, batch, groups * K * ld, groups * hd, hd)
            assert _outside_clean(flat, out, o, M, batch * hd), f'{where}: written outside the output'
            D, Q = ds.double().view(batch, groups, K, M), q.double().view(K, batch, groups, hd)
            ref = torch.einsum('bgkm,kbgd->mbd', D, Q).reshape(M, batch * hd)
            ref_abs = torch.einsum('bgkm,kbgd->mbd', D.abs(), Q.abs()).reshape(M, batch * hd)
            n_seq = groups * -(-K // 32) + 10                    # (the zero-selected pad rows of a group's last tile add exact zeros: no rounding)
            worst.add('gemm_tn_grouped', out[:M, :batch * hd], ref, ULP * ref.abs() + U * n_seq * ref_abs + FLOOR, where)
    worst.flush()


TN_LDS_TILE = {0: (128, 128), 1100: (128, 128), 1105: (128, 128), 1110: (128, 128), 1200: (128, 256), 1210: (128, 256), 1300: (256, 256), 1140: (128, 128),
               1240: (128, 256), 1340: (256, 256)}


@pytest.mark.parametrize('cfg', list(TN_LDS_TILE))
def test_gemm_tn_lds(ops, cfg):
    """vlaser_gemm_tn_lds at every configuration, one full + one ragged tile in M and N, a contraction of 1 and 3 tiles; the staggered rings also a true K of 96: the C ABI takes whole
    64-row tiles only, so the launch is K_pad = 128 with 32 zero rows -- the true rows end on the boundary of a 32-deep ring buffer, the kernel walks all four).  The tail rows of At are zero, those of Wt +-the largest finite bf16: their contribution must be exactly zero, so the
    bound is that of the true K; sumsq slots."""
    from vlaser_amd import _lib as L
    bm, bn = TN_LDS_TILE[cfg]
    M, N = bm + 13, bn + 20
    if cfg == 0:
        assert -(-M // 128) * -(-N // 128) <= ops.get_cu_budget()          # mirror of launch<..., AKM>: the heuristic takes 1100 here
    worst = Worst()
    n_slots = -(-M // bm) * -(-N // bn) * 8
    for K in (57, 185) + ((96,) if cfg in (1140, 1240, 1340) else ()):
        where = f'cfg={cfg},K={K}'
        Kp = (K + 63) // 64 * 64
        a = randb(K, M, seed=K) * pow2(M)[None]
        w = randb(K, N, seed=K + 1) * pow2(N, -6, 3)[None]
        a_buf, w_buf = torch.zeros(Kp, _c8(M) + 8), torch.full((Kp, _c8(N) + 8), BIG)
        w_buf[K:] *= torch.where((torch.arange(Kp - K)[:, None] + torch.arange(_c8(N) + 8)[None]) % 2 == 0, 1.0, -1.0)
        w_buf[:K] = 0.5
        a_buf[:K, :M], w_buf[:K, :N] = a, w
        a_buf[:K, M:] = 0.5
        At, Wt = dev(a_buf)[:, :M], dev(w_buf)[:, :N]
        A64, W64 = a.double(), w.double()
        ref, ref_abs = A64.t() @ W64, A64.abs().t() @ W64.abs()
        flat, out, o = _obuf(M + 3, N + 4)
        part = torch.full((ops.tn_sumsq_slots(M, N) + 5,), SENT, dtype=F32, device='cuda')
        ops.gemm_tn_lds(At, Wt, out, Kp, force_cfg=cfg, sumsq_part=part)
        assert _outside_clean(flat, out, o, M, N), f'{where}: written outside [M, N]'
        worst.add(f'gemm_tn_lds[{cfg}]', out[:M, :N], ref, ULP * ref.abs() + U * (Kp // 32 + 10) * ref_abs + FLOOR, where)
        _note(worst, f'gemm_tn_lds.sumsq[{cfg}]', _check_slots(f'gemm_tn_lds[{cfg}]', part, n_slots, out[:M, :N], where), where)
    _refused(L, lambda: ops.gemm_tn_lds(At, Wt, out, Kp, force_cfg=cfg, sumsq_part=part[:n_slots - 1]), 'slots')
    worst.flush()


# ================================================================================================ B. NN dgrad GEMMs, the SwiGLU-backward epilogue
NN_TILE = {0: None, 1100: (128, 128), 1105: (128, 128), 1200: (128, 256), 1300: (256, 256), 1440: (144, 128), 1500: (64, 128), 1506: (64, 128), 1532: (32, 128),
           1900: (192, 256)}


def _nn(L, epi, A, B, out=None, **kw):
    """vlaser_gemm_nn on a B view with ldw > N (ops.gemm_nn takes contiguous operands only)"""
    a = L.GemmArgs()
    (M, K), N = A.shape, B.shape[1]
    a.A, a.W, a.M, a.N, a.K, a.lda, a.ldw = A.data_ptr(), B.data_ptr(), M, N, K, A.stride(0), B.stride(0)
    if out is not None:
        a.out, a.ldo = out.data_ptr(), out.stride(0)
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    L.check(L.lib().vlaser_gemm_nn(epi, ctypes.byref(a), None), 'vlaser_gemm_nn')


def _nn_tile_height(ops, bm, N):
    """tile height of a force_bm code; 0: the heuristic, which takes the 64 x 128 tile for the few workgroups of these shapes (mirrored by ops.gemm_tile_config)"""
    if bm:
        return NN_TILE[bm][0]
    assert all(ops.gemm_tile_config(M, N, s, nn=True)[0] == 1500 for M in (1, 61, 65) for s in (1, 3))
    return 64


def _nn_operands(M, N, K, seed):
    a = randb(M, K, seed=seed) * pow2(M)[:, None]
    b = randb(K, N, seed=seed + 1) * pow2(N, -6, 3)[None]
    b_buf = torch.full((K, N + 8), BIG)                       # ldw > N: the spare columns are never read
    b_buf[:, :N] = b
    return a.double(), b.double(), dev(a), dev(b_buf)[:, :N]


@pytest.mark.parametrize('bm', list(NN_TILE))
def test_gemm_nn_plain_epilogues(ops, bm):
    """NONE / F32 / PARTIAL (1 and 3 slabs) of vlaser_gemm_nn at every force_bm: ragged M, N = 280 (a multiple of 8, not of 16 / 64 / 256), ldw > N, padded ldo."""
    from vlaser_amd import _lib as L
    N = 280
    th = _nn_tile_height(ops, bm, N)
    worst = Worst()
    for M, K, splits in ((th + 1, 64, 1), (th - 3, 192, 3)):
        where = f'bm={bm},M={M},K={K}'
        A64, B64, a_d, b_d = _nn_operands(M, N, K, seed=bm + K)
        ref, ref_abs = A64 @ B64, A64.abs() @ B64.abs()
        n = K // 32 + 10
        flat, out, o = _obuf(M + 3, N + 8)
        _nn(L, L.EPI_NONE, a_d, b_d, out=out, force_bm=bm)
        assert _outside_clean(flat, out, o, M, N), f'none {where}: written outside [M, N]'
        worst.add(f'gemm_nn.none[bm={bm}]', out[:M, :N], ref, ULP * ref.abs() + U * n * ref_abs + FLOOR, where)
        flat, out, o = _obuf(M + 3, N + 4, F32)
        _nn(L, L.EPI_F32, a_d, b_d, out=out, force_bm=bm)
        assert _outside_clean(flat, out, o, M, N), f'f32 {where}: written outside [M, N]'
        worst.add(f'gemm_nn.f32[bm={bm}]', out[:M, :N], ref, U * n * ref_abs + FLOOR, where)
        slabs = torch.full((splits * M * N + 16,), SENT, dtype=F32, device='cuda')
        _nn(L, L.EPI_PARTIAL, a_d, b_d, out_f32=slabs, k_splits=splits, force_bm=bm)
        assert is_sent(slabs[splits * M * N:]), f'partial {where}: written past the slabs'
        got = h64(slabs[:splits * M * N]).view(splits, M, N).sum(0)
        worst.add(f'gemm_nn.partial[bm={bm}]', got, ref, U * (K // splits // 32 + 10) * ref_abs + FLOOR, where + f',splits={splits}')
    worst.flush()


def _sig(g):
    return torch.sigmoid(g)


def _swiglu_bwd_ref(g, u, d, e_d):
    """fp64 d(gate), d(up) and their tolerances; g / u / d fp64 tensors of one shape, e_d the error of d (0: d is an input)"""
    s = _sig(g)
    ds = s * (1 + g * (1 - s))
    dg, du = d * u * ds, d * g * s
    tol_dg = 2 * ULP * dg.abs() + (u * ds).abs() * e_d + 4 * U * (d * u).abs() * s * (1 + g.abs()) + FLOOR
    tol_du = 2 * ULP * du.abs() + (g * s).abs() * e_d + FLOOR
    return dg, du, tol_dg, tol_du


def _pack_gu(g, u):
    """[M, I] gate / up -> the packed [M, 2 I] layout: columns [32 j, 32 j + 16) = gate channels 16 j .., the next 16 = up"""
    M, I = g.shape
    return torch.stack([g.view(M, I // 16, 16), u.view(M, I // 16, 16)], 2).reshape(M, 2 * I)


def _unpack_gu(p, I):
    M = p.shape[0]
    v = p.reshape(M, I // 16, 2, 16)
    return v[:, :, 0].reshape(M, I), v[:, :, 1].reshape(M, I)


# (name, ldo - 2 N, offset of out / res in elements): the 16-byte path, ldo % 8 != 0, out 8- but not 16-byte aligned
SB_PATHS = (('wide', 0, 0), ('ld4', 4, 0), ('off8', 8, 4))


def _sb_launch(ops, L, a_d, b_d, gu, M, N, pad, off, bm):
    ldo = 2 * N + pad
    flat, out, o = _obuf(M + 3, ldo, off=off)
    rflat, res, _ = _obuf(M + 3, ldo, off=off)
    res[:M, :2 * N] = gu
    keep = rflat.clone()
    _nn(L, L.EPI_SWIGLU_BWD, a_d, b_d, out=out, res=res, force_bm=bm)
    assert (out.data_ptr() % 16 == 0) == (off == 0)
    assert _outside_clean(flat, out, o, M, 2 * N), 'written outside [M, 2 N]'
    assert same_bits(rflat, keep), 'res modified'
    return out[:M, :2 * N]


@pytest.mark.parametrize('bm', list(NN_TILE))
def test_gemm_nn_swiglu_bwd(ops, bm):
    """VL_EPI_SWIGLU_BWD (the down_proj dgrad of the SFT step) at every force_bm, N = 16 / 48 / 272 (a ragged right edge at every wave-tile width), M = 1 and a
    ragged tile: (i) against fp64, (ii) bit for bit against the stand-alone swiglu_bwd on the NONE launch's output, (iii) the three store paths give the
    same bits and write nothing outside [M, 2 N]."""
    from vlaser_amd import _lib as L
    th = _nn_tile_height(ops, bm, 272)
    worst = Worst()
    for N in (16, 48, 272):
        for M, K in ((1, 64), (th + 1, 192)):
            where = f'bm={bm},M={M},N={N},K={K}'
            A64, B64, a_d, b_d = _nn_operands(M, N, K, seed=bm + N)
            g = randb(M, N, seed=N + 2, std=2.0)
            u = randb(M, N, seed=N + 3) * pow2(M, -6, 3)[:, None]
            gu = dev(_pack_gu(g, u))
            d, d_abs = A64 @ B64, A64.abs() @ B64.abs()
            e_d = ULP * d.abs() + U * (K // 32 + 10) * d_abs
            dg, du, tol_dg, tol_du = _swiglu_bwd_ref(g.double(), u.double(), rbf(d), e_d)
            dact = torch.empty(M, N, dtype=BF, device='cuda')
            _nn(L, L.EPI_NONE, a_d, b_d, out=dact, force_bm=bm)
            alone = sentinel(M, 2 * N)
            ops.swiglu_bwd(gu, dact, alone, M, N)
            for pname, pad, off in SB_PATHS:
                got = _sb_launch(ops, L, a_d, b_d, gu, M, N, pad, off, bm)
                assert same_bits(got, alone), f'{where},{pname}: differs from swiglu_bwd(gemm_nn NONE)'
            got_g, got_u = _unpack_gu(got, N)
            worst.add(f'gemm_nn.swiglu_bwd.dgate[bm={bm}]', got_g, dg, tol_dg, where)
            worst.add(f'gemm_nn.swiglu_bwd.dup[bm={bm}]', got_u, du, tol_du, where)
    worst.flush()


def _all_finite_bf16(lim=None):
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF).float()
    x = x[torch.isfinite(x)]
    return x if lim is None else x[x.abs() <= lim]


def test_gemm_nn_swiglu_bwd_every_gate(ops):
    """Every finite bf16 gate in [-64, 64] in `res`, against a few u and d of both signs and several scales (A = identity: d = B exactly, e_d = 0); the wide
    and the narrow store path."""
    from vlaser_amd import _lib as L
    v = _all_finite_bf16(64.0)
    M = K = 64
    N = (-(-v.numel() // M) + 15) // 16 * 16
    g = torch.zeros(M * N)
    g[:v.numel()] = v
    g = g.view(M, N)
    i = torch.arange(M * N).view(M, N)
    u = torch.tensor([1.0, -0.75, 3 * 2.0 ** -9, -320.0])[(i // 3) % 4]
    d = torch.tensor([-1.0, 0.625, 2.0 ** -12, 48.0, -5 * 2.0 ** -6])[(i // 7) % 5]
    a_d, b_d, gu = dev(torch.eye(K)), dev(d), dev(_pack_gu(g, u))
    dg, du, tol_dg, tol_du = _swiglu_bwd_ref(g.double(), u.double(), d.double(), 0.0)
    first = None
    for pname, pad, off in SB_PATHS[:2]:
        got = _sb_launch(ops, L, a_d, b_d, gu, M, N, pad, off, 0)
        got_g, got_u = _unpack_gu(got, N)
        bound(f'gemm_nn.swiglu_bwd.dgate[every gate |g| <= 64,{pname}]', got_g, dg, tol_dg)
        bound(f'gemm_nn.swiglu_bwd.dup[every gate |g| <= 64,{pname}]', got_u, du, tol_du)
        if first is None:
            first = got.clone()
        else:
            assert same_bits(got, first), 'the narrow store path differs from the wide one'


def test_gemm_nn_swiglu_bwd_refusals(ops):
    from vlaser_amd import _lib as L
    M, K = 8, 64
    a_d = dev(randb(M, K))
    call = lambda N, ldo, off_o=0, off_r=0, **kw: ops.gemm_nn(L.EPI_SWIGLU_BWD, a_d, dev(randb(K, N)), out=_obuf(M, ldo, off=off_o)[1], res=_obuf(M, ldo, off=off_r)[1], **kw)
    _refused(L, lambda: call(24, 48), 'swiglu_bwd')                       # N % 16 != 0
    _refused(L, lambda: call(32, 60), 'swiglu_bwd')                       # ldo < 2 N
    _refused(L, lambda: call(32, 66), 'swiglu_bwd')                       # ldo % 4 != 0
    _refused(L, lambda: call(32, 64, off_o=1), '8-byte aligned')
    _refused(L, lambda: call(32, 64, off_r=2), '8-byte aligned')
    _refused(L, lambda: call(32, 64, batch=2, a_bs=0, w_bs=0, o_bs=0), 'batched')


# ================================================================================================ C. fused attention backward
def _attn_inputs(S, n_q, n_kv, s_max, seed):
    """q / d_o [S, n_q, hd]; k / v [n_kv, s_max, hd]: in every 16-row tile one all-zero query and one scaled by 4, key-scaled V, power-of-two row scales on d_o;
    K rows past S: finite garbage of the largest magnitude; V^T columns past S: zero (the cache contract)"""
    hd = 128
    q = randb(S, n_q, hd, seed=seed)
    r = torch.arange(S)
    q[r % 16 == 3] = 0
    q[r % 16 == 9] *= 4
    k = randb(n_kv, s_max, hd, seed=seed + 1)
    k[:, S:] = BIG * torch.where(torch.arange(hd) % 2 == 0, 1.0, -1.0)
    v = randb(n_kv, s_max, hd, seed=seed + 2) * pow2(s_max)[None, :, None]
    v[:, S:] = 0
    d_o = randb(S, n_q, hd, seed=seed + 3) * pow2(S, -8, 2)[:, None, None]
    return q, k, v, d_o


def _attn_forward64(q, k, v, vis, scale, G):
    """o = bf16(O) [S, n_q, hd] and lse = fp32(log2-sum-exp) [n_q, S] of the masked attention, in fp64"""
    qh, kh, vh = q.double().transpose(0, 1), k.double().repeat_interleave(G, 0), v.double().repeat_interleave(G, 0)
    s2 = ((qh @ kh.transpose(1, 2)) * (scale * LOG2E32)).masked_fill(~vis, -math.inf)
    lse2 = torch.logsumexp(s2 * math.log(2), -1) / math.log(2)
    P = torch.exp2(s2 - lse2[..., None])
    return (P @ vh).transpose(0, 1).to(F32).to(BF), lse2.to(F32)


def _attn_bwd_case(ops, worst, tag, S, n_q, n_kv, vis, call, zero_dq_rows=None, where=''):
    """run `call(q, k, vt, o, d_o, lse, delta, dq, dk, dv)` on sentinel outputs and compare dq, delta_ws and each Q head's dk / dv"""
    hd, G = 128, n_q // n_kv
    s_max = (S + 63) // 64 * 64 + 64
    scale = f32s(hd ** -0.5)
    q, k, v, d_o = _attn_inputs(S, n_q, n_kv, s_max, seed=S + n_q)
    o, lse = _attn_forward64(q, k[:, :S], v[:, :S], vis, scale, G)
    vt = v.transpose(1, 2).contiguous()
    dq, dk, dv = (sentinel(S + 3, n_q * hd) for _ in range(3))
    delta = torch.full((n_q * S + 8,), SENT, dtype=F32, device='cuda')
    call(dev(q.reshape(S, n_q * hd)), dev(k), dev(vt), o.reshape(S, n_q * hd).cuda(), dev(d_o.reshape(S, n_q * hd)), lse.reshape(-1).cuda(), delta, dq, dk, dv, s_max, scale)
    for name, t in (('dq', dq), ('dk', dk), ('dv', dv)):
        assert is_sent(t[S:]), f'{tag} {where}: {name} rows past S written'
    assert is_sent(delta[n_q * S:]), f'{tag} {where}: delta_ws written past [n_q, S]'
    heads = lambda t: t.double().transpose(0, 1)
    r = attn_bwd_ref(heads(q), k[:, :S].double().repeat_interleave(G, 0), v[:, :S].double().repeat_interleave(G, 0), heads(d_o), heads(o.float()),
                     lse.double(), vis, scale)
    rows = lambda t: t.transpose(0, 1).reshape(S, n_q * hd)
    worst.add(f'{tag}.delta', delta[:n_q * S].view(n_q, S), r['D'], r['D_tol'], where)
    worst.add(f'{tag}.dq', dq[:S], rows(r['dq']), rows(r['dq_tol']), where)
    worst.add(f'{tag}.dk', dk[:S], rows(r['dk']), rows(r['dk_tol']), where)           # one partial per Q HEAD: column block h = kv head h // G, member h % G
    worst.add(f'{tag}.dv', dv[:S], rows(r['dv']), rows(r['dv_tol']), where)
    dead = ~vis.any(0)                                                                    # keys no query sees
    if dead.any():
        assert (dk[:S][dead.cuda()] == 0).all() and (dv[:S][dead.cuda()] == 0).all(), f'{tag} {where}: dk / dv of an invisible key is not zero'
    if zero_dq_rows is not None and zero_dq_rows.any():
        z = zero_dq_rows.cuda()
        assert (dq[:S][z] == 0).all() and (dk[:S][z] == 0).all(), f'{tag} {where}: a one-token sequence must give exact zeros in dq / dk'
    return dq, dk, dv, delta


def _attn_ks(S):
    """mirror of vlaser_attn_bwd / _varlen: wave groups per workgroup"""
    return 2 if S > 128 else 1


@pytest.mark.parametrize('heads', ['12/2', '28/4'])
@pytest.mark.parametrize('S', [1, 63, 64, 65, 128, 129, 200])
def test_attn_bwd_fused(ops, S, heads):
    """vlaser_attn_bwd alone (o and lse from fp64, not from the forward kernel): causal, and non-causal with kv_valid = 1 / 64 / 137 / S (clamped to S);
    S = 128 is the last size with one wave group, 129 the first with two."""
    n_q, n_kv = (int(x) for x in heads.split('/'))
    assert _attn_ks(128) == 1 and _attn_ks(129) == 2
    worst = Worst()
    i, j = torch.arange(S)[:, None], torch.arange(S)[None]
    masks = [('causal', True, S, j <= i)] + [(f'kv_valid={kv}', False, kv, (j < kv).expand(S, S)) for kv in sorted({min(x, S) for x in (1, 64, 137, S)})]
    for mname, causal, kvv, vis in masks:
        call = lambda q, k, vt, o, d_o, lse, delta, dq, dk, dv, s_max, scale: ops.attn_bwd(q, k, vt, o, d_o, lse, delta, dq, dk, dv, S, n_q, n_kv, s_max, scale,
                                                                                          causal=causal, kv_valid=kvv)
        _attn_bwd_case(ops, worst, f'attn_bwd[{heads}]', S, n_q, n_kv, vis, call, where=f'S={S},{mname}')
    worst.flush()


def test_attn_bwd_kv_valid_contract(ops):
    """A non-causal prefix longer than S is refused (dk / dv have S rows); a causal call clamps kv_valid to S."""
    from vlaser_amd import _lib as L
    S, n_q, n_kv = 5, 2, 1
    worst = Worst()
    vis = torch.tril(torch.ones(S, S, dtype=torch.bool))
    call = lambda q, k, vt, o, d_o, lse, delta, dq, dk, dv, s_max, scale: ops.attn_bwd(q, k, vt, o, d_o, lse, delta, dq, dk, dv, S, n_q, n_kv, s_max, scale,
                                                                                      causal=True, kv_valid=s_max)
    _attn_bwd_case(ops, worst, 'attn_bwd[kv_valid > S, causal]', S, n_q, n_kv, vis, call)
    worst.flush()
    bad = lambda q, k, vt, o, d_o, lse, delta, dq, dk, dv, s_max, scale: ops.attn_bwd(q, k, vt, o, d_o, lse, delta, dq, dk, dv, S, n_q, n_kv, s_max, scale,
                                                                                     causal=False, kv_valid=S + 1)
    with pytest.raises(L.VlaserHipError, match='kv_valid'):
        _attn_bwd_case(ops, Worst(), 'refused', S, n_q, n_kv, vis, bad)


@pytest.mark.parametrize('heads', ['12/2', '28/4'])
@pytest.mark.parametrize('lens', [[1], [63, 65], [1, 1, 130, 64, 5], [40, 3, 70, 129]], ids=lambda l: '-'.join(map(str, l)))
def test_attn_bwd_varlen(ops, lens, heads):
    """vlaser_attn_bwd_varlen under the same bounds: block-diagonal causal over concatenated sequences (boundaries inside and on the 64-row tiles, one-token
    sequences, more than one wave group)."""
    n_q, n_kv = (int(x) for x in heads.split('/'))
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    S = cu[-1]
    seq = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))
    i, j = torch.arange(S)[:, None], torch.arange(S)[None]
    vis = (j <= i) & (seq[:, None] == seq[None])
    solo = torch.tensor(lens)[seq] == 1
    cu_d = torch.tensor(cu, dtype=torch.int32, device='cuda')
    call = lambda q, k, vt, o, d_o, lse, delta, dq, dk, dv, s_max, scale: ops.attn_bwd_varlen(q, k, vt, o, d_o, lse, delta, dq, dk, dv, S, n_q, n_kv, s_max, scale,
                                                                                             cu_d, cu_host=cu)
    worst = Worst()
    _attn_bwd_case(ops, worst, f'attn_bwd_varlen[{heads}]', S, n_q, n_kv, vis, call, zero_dq_rows=solo, where=f'lens={lens}')
    worst.flush()


_TWO_LAUNCH_SCRIPT = """
import hashlib, sys, torch
sys.path.insert(0, %r)
from vlaser_amd import ops
BF = torch.bfloat16
S, n_q, n_kv, hd, s_max = 129, 12, 2, 128, 192
g = torch.Generator().manual_seed(5)
rnd = lambda *s: torch.randn(*s, generator=g).to(BF).cuda()
q, d_o, o = rnd(S, n_q * hd), rnd(S, n_q * hd), rnd(S, n_q * hd) * 0.1
k, v = rnd(n_kv, s_max, hd), rnd(n_kv, s_max, hd)
v[:, S:] = 0
vt = v.transpose(1, 2).contiguous()
lse = (torch.rand(n_q * S, generator=g) * 2 + 6).cuda()
h = hashlib.sha256()
for causal, kvv in ((True, S), (False, 70)):
    dq, dk, dv = (torch.full((S, n_q * hd), 7.0, dtype=BF, device='cuda') for _ in range(3))
    delta = torch.full((n_q * S,), 7.0, device='cuda')
    ops.attn_bwd(q, k, vt, o, d_o, lse, delta, dq, dk, dv, S, n_q, n_kv, s_max, hd ** -0.5, causal=causal, kv_valid=kvv)
    torch.cuda.synchronize()
    for t in (dq, dk, dv):
        h.update(t.view(torch.int16).cpu().numpy().tobytes())
    h.update(delta.view(torch.int32).cpu().numpy().tobytes())
print('SHA', h.hexdigest())
"""


def test_attn_bwd_two_launch_form_same_bits():
    """VLASER_ATTN_BWD_TWO_LAUNCHES=1 (read once per process: two child processes) gives the default one-launch form's bits at S = 129 (two wave groups)."""
    outs = []
    for two in ('0', '1'):
        env = dict(os.environ, VLASER_ATTN_BWD_TWO_LAUNCHES=two)
        r = subprocess.run([sys.executable, '-c', _TWO_LAUNCH_SCRIPT % ROOT], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append([l for l in r.stdout.splitlines() if l.startswith('SHA')][0])
    assert outs[0] == outs[1], outs


# ================================================================================================ D. RMSNorm backward, column sums
def _rb_rows(kind, S, C, seed):
    if kind == 'tiny':                     # |x| ~ 2^-60: eps dominates the mean square
        return (randb(S, C, seed=seed) * 2.0 ** -60).to(BF)
    if kind == 'huge':                     # rows scaled by 2^40
        return (randb(S, C, seed=seed) * 2.0 ** 40).to(BF)
    return _ln_rows(kind, S, C, seed)


RB_KINDS = LN_KINDS + ('tiny', 'huge')
RB_VARIANTS = [(dres, dyf, dwm) for dres in (True, False) for dyf in (0, 1, 3, 8) for dwm in ('out', 'ws', 'none')]


RB_C = [8, 520, 512, 1536, 4096, 4104]


def _rb_variant(ci, case):
    """the call variant of case (S, kind) number `case` at the ci-th C: each C meets all 24 once, and the shift by 5 per C lets every dw mode and every dy form
    meet every row kind and every S over the sweep"""
    return RB_VARIANTS[(case + 5 * ci) % len(RB_VARIANTS)]


def test_rmsnorm_bwd_variant_plan():
    """(needs no kernel) over the C sweep -- the weight gradient over C <= 4096 only -- each dw mode meets every row kind and every S, each dy form every kind,
    and S = 258 (more than 16 row blocks per slice) every (dres, dy form)"""
    seen = set()
    for ci, C in enumerate(RB_C):
        assert len({_rb_variant(ci, c) for c in range(24)}) == 24
        for si in range(4):
            for ki in range(len(RB_KINDS)):
                dres, dyf, dwm = _rb_variant(ci, si * len(RB_KINDS) + ki)
                seen |= {('kind-dy', ki, dyf), ('kind-dres', ki, dres), ('S-dy', si, dres, dyf)}
                if C <= 4096:
                    seen |= {('kind-dw', ki, dwm), ('S-dw', si, dwm)}
    n = lambda tag: sum(1 for t in seen if t[0] == tag)
    assert (n('kind-dw'), n('S-dw'), n('kind-dy'), n('kind-dres'), n('S-dy')) == (18, 12, 24, 12, 32)


@pytest.mark.parametrize('C', RB_C)
def test_rmsnorm_bwd(ops, C):
    """vlaser_rmsnorm_bwd on the loop kernel (C = 8, 520, 4104) and the register kernels 1 / 3 / 8, S = 1 / 3 / 5 / 258, the four LayerNorm row families + tiny
    and huge rows; each of the 24 call variants (dres given or not; dy as bf16 or as 1 / 3 / 8 fp32 slabs; dw_out, dw_ws alone or neither) once per C, shifted from C to C
    (test_rmsnorm_bwd_variant_plan); colsum_mul mode 2 on every one of the same rows (with the slabs: on the bf16 dy they reduce to).  Above C = 4096 the weight-gradient workspace is refused."""
    from vlaser_amd import _lib as L
    eps = f32s(1e-6)
    w = randb(C, seed=1, std=0.5) + 1.0
    w = w.to(BF).float()
    w_d, w64 = dev(w), w.double()
    n_row = 8 * ((C + 511) // 512) + 6
    worst = Worst()
    case = 0
    for S in (1, 3, 5, 258):
        nb = (S + 3) // 4
        for ki, kind in enumerate(RB_KINDS):
            dres_on, n_slab, dwm = _rb_variant(RB_C.index(C), case)
            case += 1
            where = f'C={C},S={S},{kind},dres={int(dres_on)},slabs={n_slab},dw={dwm}'
            x = _rb_rows(kind, S, C, seed=10 * ki + S + C).float()
            dres = randb(S, C, seed=5 + ki, std=0.3) * pow2(S)[:, None] if dres_on else None
            if n_slab:
                slabs = torch.randn(n_slab, S, C, generator=torch.Generator().manual_seed(case)) * 0.3 * pow2(S)[None, :, None]
                acc = torch.zeros(S, C)
                for u in range(n_slab):                      # the kernel's own fp32 additions, in slab order, then one bf16 rounding
                    acc = acc + slabs[u]
                dy = acc.to(BF).float()
                slab_buf = torch.full((n_slab * S * C + 16,), SENT, dtype=F32, device='cuda')
                slab_buf[:n_slab * S * C] = slabs.reshape(-1).cuda()
            else:
                dy = randb(S, C, seed=3 + ki) * pow2(S)[:, None]
            if dwm != 'none' and C > 4096:
                ws = torch.full((nb * C,), SENT, dtype=F32, device='cuda')
                _refused(L, lambda: ops.rmsnorm_bwd(dev(dy), dev(x), w_d, None, sentinel(S, C), S, C, eps, dw_out=sentinel(C), dw_ws=ws), 'C <= 4096')
                assert is_sent(ws)
                dwm = 'none'
            dx = sentinel(S + 3, C)
            dw = sentinel(C + 8)
            ws = torch.full((nb * C + 16,), SENT, dtype=F32, device='cuda') if dwm != 'none' else None
            ops.rmsnorm_bwd(None if n_slab else dev(dy), dev(x), w_d, None if dres is None else dev(dres), dx, S, C, eps,
                            dw_out=dw if dwm == 'out' else None, dw_ws=ws, dy_partials=slab_buf if n_slab else None, n_partials=n_slab)
            assert is_sent(dx[S:]), f'{where}: dx rows past S written'
            if n_slab:
                assert is_sent(slab_buf[n_slab * S * C:])
            x64, dy64 = x.double(), dy.double()
            rs = 1.0 / torch.sqrt((x64 ** 2).mean(-1, keepdim=True) + eps)
            xh, g = x64 * rs, dy64 * w64
            ref = rs * (g - xh * (g * xh).mean(-1, keepdim=True)) + (dres.double() if dres_on else 0.0)
            ref_abs = rs * (g.abs() + xh.abs() * (g * xh).abs().mean(-1, keepdim=True)) + (dres.double().abs() if dres_on else 0.0)
            worst.add('rmsnorm_bwd.dx', dx[:S], ref, ULP * ref.abs() + U * (3 * n_row + 17) * ref_abs + FLOOR, where)
            dw_ref, dw_abs = (dy64 * xh).sum(0), (dy64 * xh).abs().sum(0)
            if dwm == 'out':
                assert is_sent(dw[C:]) and is_sent(ws[nb * C:]), f'{where}: dw_out / dw_ws written past their ends'
                n_dw = 3 + -(-nb // 16) + 1 + 4 + 2 + n_row // 2 + 3
                worst.add('rmsnorm_bwd.dw', dw[:C], dw_ref, ULP * dw_ref.abs() + U * n_dw * dw_abs + FLOOR, where)
            elif dwm == 'ws':
                assert is_sent(dw) and is_sent(ws[nb * C:]), f'{where}: dw_ws alone must leave dw_out and the spare slots alone'
                worst.add('rmsnorm_bwd.dw_ws', h64(ws[:nb * C]).view(nb, C).sum(0), dw_ref, U * (n_row // 2 + 8) * dw_abs + FLOOR, where)
            out = torch.full((C + 8,), SENT, dtype=F32, device='cuda')
            cws = torch.empty(2 * S + 16 * C, dtype=F32, device='cuda')
            ops.colsum_mul(dev(dy), dev(x), out, S, C, mode=2, eps=eps, ws=cws)
            assert is_sent(out[C:])
            n_cs = 70 + 8 * ((C + 511) // 512) + (S + 63) // 64 + 20
            worst.add('colsum_mul2', out[:C], dw_ref, U * n_cs * dw_abs + FLOOR, where)
    worst.flush()


@pytest.mark.parametrize('S', [1, 77, 1025])
def test_colsum_bf16(ops, S):
    """The bias gradient's column sum with lda > C, C = 200 (three full 64-column workgroups and 8 columns of a fourth)."""
    C, lda = 200, 216
    a = randb(S, C, seed=S) * pow2(C)[None] * pow2(S, -3, 3)[:, None]
    buf = torch.full((S, lda), BIG)
    buf[:, :C] = a
    out = sentinel(C + 8)
    ops.colsum_bf16(dev(buf)[:, :C], out, S, C)
    assert is_sent(out[C:])
    ref, ref_abs = a.double().sum(0), a.double().abs().sum(0)
    bound(f'colsum_bf16[S={S}]', out[:C], ref, ULP * ref.abs() + U * ((S + 63) // 64 + 19) * ref_abs + FLOOR)


# ================================================================================================ E. swiglu, swiglu_bwd stand-alone
@pytest.mark.parametrize('I,S', [(16, 4080), (48, 10923)])
def test_swiglu_fwd_bwd_every_gate(ops, I, S):
    """Every finite bf16 gate (cycled over the S x I elements) against u and d of both signs and several scales; S x I = 48 x 10923 is past 2048 x 256 threads:
    the grid-stride loop wraps.  |u|, |d| <= 1 where |g| > 2^64 (the products stay finite)."""
    if I == 48:
        assert S * I > 2048 * 256 >= (S - 1) * I
    v = _all_finite_bf16()
    n = S * I
    assert n >= v.numel()
    i = torch.arange(n)
    g = v[(i * 7919) % v.numel()].view(S, I)                    # 7919 is prime to 65280: every value occurs
    assert torch.unique(g).numel() == torch.unique(v).numel()
    small = g.abs() <= 2.0 ** 64
    u = torch.tensor([1.0, -0.75, 3 * 2.0 ** -9, -2.0 ** -20])[(i // 3) % 4].view(S, I) * torch.where(small, pow2(n, 0, 6).view(S, I), torch.ones(S, I))
    d = torch.tensor([-1.0, 0.625, 2.0 ** -12, -5 * 2.0 ** -6, 0.0])[(i // 5) % 5].view(S, I) * torch.where(small, pow2(n, 0, 5).view(S, I), torch.ones(S, I))
    gu = dev(_pack_gu(g, u))
    act = sentinel(n + 16)
    ops.swiglu(gu, act, S, I)
    assert is_sent(act[n:])
    g64, u64 = g.double(), u.double()
    ref = rbf(g64 * _sig(g64)) * u64
    bound(f'swiglu[every bf16 gate,I={I}]', act[:n].view(S, I), ref, 2 * ULP * ref.abs() + FLOOR)
    dgu = sentinel(2 * n + 16)
    ops.swiglu_bwd(gu, dev(d), dgu, S, I)
    assert is_sent(dgu[2 * n:])
    dg, du, tol_dg, tol_du = _swiglu_bwd_ref(g64, u64, d.double(), 0.0)
    got_g, got_u = _unpack_gu(dgu[:2 * n].view(S, 2 * I), I)
    bound(f'swiglu_bwd.dgate[every bf16 gate,I={I}]', got_g, dg, tol_dg)
    bound(f'swiglu_bwd.dup[every bf16 gate,I={I}]', got_u, du, tol_du)


# ================================================================================================ F. AdamW
def _adamw_blocks(n, cap):
    """mirror of vlaser_adamw (csrc/train.hip): workgroups of 256 threads x 4 elements, at most one per CU the budget leaves"""
    return min((n + 1023) // 1024, cap)


def _adamw_cap(ops):
    return min(ops.get_cu_budget(), torch.cuda.get_device_properties(0).multi_processor_count)


def _adamw_state(n, step, seed):
    g_ = torch.Generator().manual_seed(seed)
    i = torch.arange(n)
    kind = (i + n) % 8
    sc = pow2(n, -10, 2)
    w = torch.randn(n, generator=g_) * 0.05 * sc
    grad = (torch.randn(n, generator=g_) * 0.01 * sc).to(BF).float()
    m = torch.randn(n, generator=g_) * 0.01 * sc if step > 1 else torch.zeros(n)
    v = (torch.randn(n, generator=g_) * 0.01 * sc) ** 2 if step > 1 else torch.zeros(n)
    sign = torch.where(i % 2 == 0, 1.0, -1.0)
    grad = torch.where(kind == 0, torch.zeros(n), grad)                                   # g = 0 with m = v = 0: the update is 0 / eps
    m, v = torch.where(kind == 0, torch.zeros(n), m), torch.where(kind == 0, torch.zeros(n), v)
    grad = torch.where(kind == 1, sign * 2.0 ** -70, grad)                                # g^2 underflows
    grad = torch.where(kind == 2, sign * 2.0 ** 60, grad)
    return w, m, v, grad


def _adamw_ref(w, m, v, grad, lr, b1, b2, eps, wd, gfac, k_g, step):
    """fp64 FusedAdam (adam_w_mode) + the tolerances of the docstring; gfac = the factor on the gradient (fp64), k_g its roundings"""
    w, m, v, grad = (t.double() for t in (w, m, v, grad))
    c1, c2 = float(torch.tensor(1.0, dtype=F32) - torch.tensor(b1, dtype=F32)), float(torch.tensor(1.0, dtype=F32) - torch.tensor(b2, dtype=F32))
    gs = grad * gfac
    m1, v1 = b1 * m + c1 * gs, b2 * v + c2 * gs * gs
    tol_m = U * (2 * (b1 * m).abs() + (2 + k_g) * (c1 * gs).abs()) + FLOOR
    tol_v = U * (2 * b2 * v + (3 + 2 * k_g) * c2 * gs * gs) + FLOOR
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    e1, e2 = 2 * U * b1 ** step / bc1 + U, 2 * U * b2 ** step / bc2 + U
    rbc2, decay, stp = 1.0 / math.sqrt(bc2), 1.0 - lr * wd, lr / bc1
    sq = torch.sqrt(v1)
    den = sq * rbc2 + eps
    e_sqrt = torch.minimum(tol_v / sq.clamp_min(1e-300), torch.sqrt(tol_v)) + 2 * U * sq
    e_den = e_sqrt * rbc2 + sq * rbc2 * (e2 / 2 + 3 * U) + U * den
    upd = stp * m1 / den
    e_upd = stp * (tol_m / den + m1.abs() * e_den / den ** 2 + 2 * U * (m1 / den).abs()) + upd.abs() * (e1 + 2 * U)
    ref = w * decay - upd
    tol_w = 4 * U * (w * decay).abs() + e_upd + U * upd.abs() + U * ref.abs() + FLOOR
    return m1, v1, ref, tol_m, tol_v, tol_w


def _adamw_case(ops, worst, tag, n, step, wd, gscale, clip=None):
    lr, b1, b2, eps, wd, gscale = f32s(1e-3), f32s(0.9), f32s(0.999), f32s(1e-8), f32s(wd), f32s(gscale)
    w, m, v, grad = _adamw_state(n, step, seed=n + step)
    pad = 8
    mk = lambda t, dt: torch.cat([t.to(dt), torch.full((pad,), SENT, dtype=dt)]).cuda()
    p_d, w_d, m_d, v_d, g_d = sentinel(n + pad), mk(w, F32), mk(m, F32), mk(v, F32), mk(grad, BF)
    gfac, k_g = gscale, 1
    where = f'n={n},step={step},wd={wd:g},gscale={gscale:g}'
    if clip is None:
        ops.adamw(p_d[:n], w_d, m_d, v_d, g_d, lr, b1, b2, eps, wd, gscale, step)
    else:
        gnorm2, max_norm = f32s(clip[0]), f32s(clip[1])
        gn = math.sqrt(gnorm2)
        if max_norm > 0 and gn > max_norm:
            gfac, k_g = gscale * max_norm / (gn + f32s(1e-6)), 5
        where += f',gnorm2={gnorm2:g},max_norm={max_norm:g}'
        ops.adamw_clipped(p_d[:n], w_d, m_d, v_d, g_d, lr, b1, b2, eps, wd, gscale, torch.tensor([gnorm2], dtype=F32, device='cuda'), max_norm, step)
    for name, t in (('p', p_d), ('master', w_d), ('m', m_d), ('v', v_d), ('g', g_d)):
        assert is_sent(t[n:]), f'{tag} {where}: {name} written past n'
    assert same_bits(g_d[:n].cpu(), grad.to(BF)), f'{tag} {where}: the gradient was modified'
    m1, v1, ref, tol_m, tol_v, tol_w = _adamw_ref(w, m, v, grad, lr, b1, b2, eps, wd, gfac, k_g, step)
    worst.add(f'{tag}.m', m_d[:n], m1, tol_m, where)
    worst.add(f'{tag}.v', v_d[:n], v1, tol_v, where)
    worst.add(f'{tag}.master', w_d[:n], ref, tol_w, where)
    assert same_bits(p_d[:n].cpu(), w_d[:n].cpu().to(BF)), f'{tag} {where}: p is not bf16(master)'


@pytest.mark.parametrize('step', [1, 2, 1000, 100000])
def test_adamw(ops, step):
    """vlaser_adamw: n = 1 / 3 (the scalar tail alone), 4, 5, 1027 (vector body + tail), and 1024 x the workgroup cap + 8 + 3 (the grid-stride loop wraps, then the
    tail); g = 0 with m = v = 0, |g| = 2^-70 and 2^60 among the elements; weight decay 0 / 0.05, grad_scale 1 / 0.37."""
    cap = _adamw_cap(ops)
    n_wrap = 1024 * cap + 8 + 3
    assert _adamw_blocks(n_wrap, cap) == cap and (n_wrap >> 2) > cap * 256 and n_wrap & 3
    worst = Worst()
    for n in (1, 3, 4, 5, 1027, n_wrap):
        for wd, gscale in ((0.0, 1.0), (0.05, 0.37)):
            _adamw_case(ops, worst, 'adamw', n, step, wd, gscale)
    worst.flush()


def test_adamw_clipped(ops):
    """vlaser_adamw_clipped: gnorm2 below, equal to and above max_norm^2, and max_norm = 0 (off); the clip factor formed in fp64 in the reference."""
    worst = Worst()
    for gnorm2, max_norm in ((1.0, 2.0), (4.0, 2.0), (9.0, 2.0), (1e6, 0.0), (2.0 ** -40, 2.0 ** -30)):
        for n, step in ((5, 1), (1027, 2), (1024 * _adamw_cap(ops) + 11, 1000)):
            _adamw_case(ops, worst, 'adamw_clipped', n, step, 0.05, 0.37, clip=(gnorm2, max_norm))
    worst.flush()


# ================================================================================================ G. embedding gradient
def _esa(L, ids, rank, dh, table, n, H, vocab, part=None):
    """vlaser_embed_scatter_add (+ vlaser_sumsq_rows) with an explicit vocab: the table buffer may hold spare rows behind it"""
    order = torch.sort(ids.reshape(-1)[:n], stable=True).indices.to(torch.int32)
    L.check(L.lib().vlaser_embed_scatter_add(ids.data_ptr(), rank.data_ptr(), order.data_ptr(), dh.data_ptr(), table.data_ptr(), n, H, vocab, None),
            'vlaser_embed_scatter_add')
    if part is not None:
        L.check(L.lib().vlaser_sumsq_rows(ids.data_ptr(), order.data_ptr(), table.data_ptr(), n, H, vocab, part.data_ptr(), part.numel(), None), 'vlaser_sumsq_rows')


VOCAB = 40


def _esa_runs():
    """(id, length, text positions) in sorted order: out-of-range ids at both ends, runs of 1 / 3 / 4 / 5 / 9 starting on positions 0 and 3 of the 4-position
    chunks and right behind a run that ended on a chunk boundary, <IMG_CONTEXT> positions (rank >= 0) inside runs and one run made only of them"""
    return [(-5, 2, None), (-1, 1, None), (2, 5, None), (3, 4, None), (5, 3, None), (7, 9, None), (8, 1, None), (11, 1, None), (12, 1, None), (13, 3, None),
            (17, 9, (0, 2, 3, 8)), (20, 4, ()), (21, 5, (1, 4)), (30, 1, None), (VOCAB, 2, None), (VOCAB + 7, 1, None)]


def _esa_patterns():
    runs = _esa_runs()
    ids = torch.tensor([i for i, l, _ in runs for _ in range(l)])
    text = torch.tensor([t is None or k in t for _, l, t in runs for k in range(l)])
    starts, lens = [], []
    pos = 0
    for i, l, _ in runs:
        if 0 <= i < VOCAB:
            starts.append(pos % 4)
            lens.append(l)
        pos += l
    assert {0, 3} <= set(starts) and {1, 3, 4, 5, 9} <= set(lens) and ids[0] < 0 and ids[-1] >= VOCAB
    perm = torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(3))          # the positions are not sorted: `order` is not the identity
    return {'runs': (ids[perm], text[perm]), 'one-id': (torch.full((70,), 9), torch.arange(70) % 5 != 2), 'n=1': (torch.tensor([4]), torch.tensor([True]))}


@pytest.mark.parametrize('H', [2, 510, 514, 8, 520])
def test_embed_scatter_add(ops, H):
    """vlaser_embed_scatter_add: every run summed once by the workgroup whose 4-position chunk holds its start; H = 514 / 520 reach the second column block;
    H % 8 == 0: vlaser_sumsq_rows on the same ids (per slot, duplicates once, slots past n zero)."""
    from vlaser_amd import _lib as L
    worst = Worst()
    for pname, (ids, text) in _esa_patterns().items():
        n = ids.numel()
        rank = torch.where(text, -1, 5).to(torch.int32)
        dh = randb(n, H, seed=n) * pow2(n)[:, None]
        base = randb(VOCAB + 2, H, seed=H, std=0.01) * pow2(VOCAB + 2, -4, 4)[:, None]
        table = dev(base)
        part = torch.full((n + 5,), SENT, dtype=F32, device='cuda') if H % 8 == 0 else None
        _esa(L, ids.cuda(), rank.cuda(), dev(dh), table, n, H, VOCAB, part)
        ok = text & (ids >= 0) & (ids < VOCAB)
        ref, ref_abs, cnt = base.double().clone(), base.double().abs().clone(), torch.zeros(VOCAB + 2)
        ref.index_add_(0, ids[ok], dh[ok].double())
        ref_abs.index_add_(0, ids[ok], dh[ok].double().abs())
        cnt.index_add_(0, ids[ok], torch.ones(int(ok.sum())))
        touched = cnt > 0
        where = f'H={H},{pname}'
        assert same_bits(table[~touched.cuda()].cpu(), base[~touched].to(BF)), f'{where}: a row no text position names was modified'
        worst.add('embed_scatter_add', table[touched.cuda()], ref[touched], ULP * ref[touched].abs() + U * cnt[touched, None] * ref_abs[touched] + FLOOR, where)
        if part is not None:
            srt = torch.sort(ids, stable=True).values
            head = torch.ones(n, dtype=torch.bool)
            head[1:] = srt[1:] != srt[:-1]
            head &= (srt >= 0) & (srt < VOCAB)
            want = torch.zeros(n + 5, dtype=D64)
            want[:n][head] = h64(table)[srt[head]].pow(2).sum(-1)
            worst.add('sumsq_rows', part, want, U * 16 * want + FLOOR, where)
    worst.flush()


# ================================================================================================ H. transpose
@pytest.mark.parametrize('name,rows,cols,ld_in,ld_out,pad_rows,off', [('vec', 72, 136, 144, 88, 80, 0), ('odd-ld', 72, 136, 145, 88, 80, 0),
                                                                      ('odd-shape', 77, 130, 136, 99, 90, 0), ('offset-base', 72, 136, 144, 88, 80, 1)])
def test_transpose(ops, name, rows, cols, ld_in, ld_out, pad_rows, off):
    """vlaser_transpose bit for bit on both kernels (the 16-byte one needs every size and stride a multiple of 8 and aligned bases), pad_rows > rows zero-filled,
    the two-level batch with inner > 1; nothing else written."""
    batch, inner = 2, 3
    vec = all(x % 8 == 0 for x in (rows, cols, ld_in, ld_out, pad_rows)) and off == 0         # mirror of vlaser_transpose's choice
    assert vec == (name == 'vec')
    in_is, in_bs = rows * ld_in + 8, inner * (rows * ld_in + 8) + 16
    out_is, out_bs = cols * ld_out + 8, inner * (cols * ld_out + 8) + 24
    src = randb(batch * in_bs + 8, seed=rows)
    src_d = dev(src)
    dst = sentinel(batch * out_bs + 16)
    ops.transpose(src_d[off:], dst[off:], rows, cols, ld_in, ld_out, pad_rows, batch, in_bs, out_bs, inner, in_is, out_is)
    want = torch.full((batch * out_bs + 16,), SENT)
    for b in range(batch):
        for i in range(inner):
            s0, d0 = off + b * in_bs + i * in_is, off + b * out_bs + i * out_is
            blk = src[s0:s0 + rows * ld_in].view(rows, ld_in)[:, :cols]
            o = want[d0:d0 + cols * ld_out].view(cols, ld_out)
            o[:, :rows] = blk.t()
            o[:, rows:pad_rows] = 0
    assert same_bits(dst.cpu(), want.to(BF)), f'{name}: transpose differs'
