"""Backward pieces the SFT step (sft.py) and the VLM group of the VLA step (vla_vlm_group.py) share.  Free functions: every buffer is an argument, every
launch goes through `ops`.  Each is called once per step or once per layer, never once per launch."""
from . import _lib as L
from . import ops


def dgrad_nn(dY, W, out, part, keep_slabs=False):
    """out[S,K] = dY[S,N] @ W[N,K], W as the forward stores it (NN GEMM); long contractions over few output tiles run split-K through the fp32 slab
    workspace `part`.  `keep_slabs`: a split-K product is NOT reduced -- returns (slabs, count) for a consumer that sums them itself
    (`vlaser_rmsnorm_bwd`'s dy_partials), else None."""
    S = dY.shape[0]
    Nin, Kout = W.shape
    # measured at S = 560, 1536 outputs (tools/micro/nn_lab.py): contraction <= 2048 -> one pass (11.5-14.6 us) beats split-K slabs +
    # their reduction (9-11 + 5 us); longer contractions (8960 / 17920) keep split-K
    sp = 1 if Nin <= 2048 else ops.gemm_splits(S, Kout, Nin, part.numel(), nn=True)
    if sp > 1:
        slabs = part[:sp * S * Kout]
        ops.gemm_nn(L.EPI_PARTIAL, dY, W, out_f32=slabs, k_splits=sp)
        if keep_slabs:
            return slabs, sp
        ops.reduce_norm(None, slabs, sp, S, Kout, out)
    else:
        ops.gemm_nn(L.EPI_NONE, dY, W, out=out)
    return None


def wgrad_tn(dY, X, out, bias_out=None):
    """out[N,K] = dY[S,N]^T @ X[S,K] by the register-staged TN GEMM (both operands read as they lie), + the bias gradient = column sums of dY."""
    ops.gemm_tn(dY, X, out)
    if bias_out is not None:
        ops.colsum_bf16(dY, bias_out, dY.shape[0], dY.shape[1])


def projector_forward(h_vit, v, ps_raw, ps_ln, z1, g1, feat, T, G_, C1, ps_v1):
    """mlp1 on the vision tower's last hidden state of T tiles (modeling_internvl_chat.py:89-94, 257-291) with what its backward needs kept: the
    un-normalised pixel-shuffled rows `ps_raw`, the LayerNorm output `ps_ln`, the GELU's pre-activation `z1` and output `g1`."""
    ops.pixel_shuffle(h_vit, ps_raw, T, G_, C1, ps_v1)
    ops.pixel_shuffle_ln(h_vit, v['mlp1.m0w'], v['mlp1.m0b'], ps_ln, T, G_, C1, 1e-5, ps_v1)
    ops.gemm(L.EPI_BIAS_GELU, ps_ln, v['mlp1.m1w'], out=g1, bias=v['mlp1.m1b'], aux_out=z1, ld_aux=z1.stride(0))      # g1 + the pre-activation z1 (GELU backward)
    ops.gemm(L.EPI_BIAS, g1, v['mlp1.m3w'], out=feat, bias=v['mlp1.m3b'])


def projector_backward(dfeat, v, gv, ps_raw, ps_ln, z1, g1, dg1, dz1, dln, col, rowstat):
    """feat = m3(gelu(m1(LN(ps_raw)))) backwards from `dfeat`: the six mlp1 gradients into `gv`, d loss / d LN output left in `dln` (the VLM group goes on
    from there into the vision tower)."""
    nt, C4 = dln.shape
    ops.gemm_nn(L.EPI_NONE, dfeat, v['mlp1.m3w'], out=dg1)
    wgrad_tn(dfeat, g1, gv['mlp1.m3w'], bias_out=gv['mlp1.m3b'])
    ops.gelu_bwd(z1, dg1, dz1)
    wgrad_tn(dz1, ps_ln, gv['mlp1.m1w'], bias_out=gv['mlp1.m1b'])
    ops.gemm_nn(L.EPI_NONE, dz1, v['mlp1.m1w'], out=dln)
    ops.colsum_mul(dln, ps_raw, col, nt, C4, 3, 1e-5, rowstat)       # LayerNorm weight: sum over the rows of dy * normalised x
    gv['mlp1.m0w'].copy_(col[:C4])
    ops.colsum_mul(dln, None, col, nt, C4, 0, ws=rowstat)            # LayerNorm bias: column sums
    gv['mlp1.m0b'].copy_(col[:C4])


def attn_bwd_materialised(q, Kc, VTc, dao, ao, sc, dP, P, dS, dq, dk, dv, nb, nk, kp, nq, G, hd, sm, scale, causal, kv_valid, q_off=0):
    """Attention backward of `nb` query rows of a decoder layer against the keys [0, nk) through materialised [nq, nb, kp] score matrices (kp = nk
    rounded up to 64; sc / dP fp32, P / dS bf16).  q / dao / ao / dq: [nb, nq * hd] row views starting at the first query row; Kc [nkv, sm, hd] and
    VTc [nkv, hd, sm] as the cache holds them.  Leaves dQ in dq and one dK / dV partial per Q head in rows [0, nk) of dk / dv (summed over the kv group
    by rope_bwd_pack).  Visibility: key k < kv_valid, and with `causal` k <= q_off + row."""
    ops.gemm_raw(L.EPI_F32, q, Kc, sc, nb, nk, hd, nq * hd, hd, kp, batch=nq, a_bs=hd, w_bs=sm * hd, o_bs=nb * kp, w_group=G)     # Q K^T
    # dP = dO V^T and (below) dQ = dS K in the NN form: V^T [hd, keys] and K [keys, hd] are read as the cache holds them (r01/r02
    # transposed both per layer); dS is zero beyond the visible range, so cache rows past it only need to be finite
    ops.gemm_raw_nn(L.EPI_F32, dao, VTc, dP, nb, kp, hd, nq * hd, sm, kp, batch=nq, a_bs=hd, w_bs=hd * sm, o_bs=nb * kp, w_group=G)   # dO V^T
    ops.attn_bwd_pds_masked(sc, dP, dao, ao, P, dS, nq, nb, kp, hd, scale, causal, kv_valid, q_off)      # P = softmax(S), dS = P o (dP - D) * scale
    ops.gemm_raw_nn(L.EPI_NONE, dS, Kc, dq, nb, hd, kp, kp, hd, nq * hd, batch=nq, a_bs=nb * kp, w_bs=sm * hd, o_bs=hd, w_group=G)  # dQ = dS K
    # dK[kvh] = sum_g dS[kvh*G+g]^T Q_g, dV[kvh] = sum_g P[kvh*G+g]^T dO_g: contraction along the rows (q) of both operands,
    # summed over the q heads of the kv group, straight from dS / P [head, q, k] and q / dO [q, head*hd]
    # one TN GEMM per Q head (108 workgroups instead of 18 serial ones); the sum over the group happens in rope_bwd_pack
    ops.gemm_tn_grouped(dS, q, dk, nk, hd, nb, kp, nq * hd, nq * hd, 1, 0, 0, nq, nb * kp, hd, hd)
    ops.gemm_tn_grouped(P, dao, dv, nk, hd, nb, kp, nq * hd, nq * hd, 1, 0, 0, nq, nb * kp, hd, hd)
