"""What the three trainers (sft.py, vla_train.py, vla_vlm_group.py) share about their parameters:

  * `FlatParams`: one flat bf16 parameter buffer + one gradient buffer with named views;
  * `ParamGroup`: such a buffer cut into buckets, of which this rank owns a ZeRO-1 shard (fp32 masters + AdamW moments), with the per-bucket
    operations of a step (gradient norm, AdamW, reduce-scatter / all-gather, fp32 accumulation) and the optimizer state of a checkpoint;
  * the codec of a Qwen decoder layer and of the projector `mlp1`: names and shapes in the flat layout, HF names <-> kernel layout.

No arithmetic besides dtype casts happens here: the kernels own the math (ops.py), dp.py the collectives.
"""
import contextlib

import torch

from . import dp, ops

BF = torch.bfloat16
F32 = torch.float32


class FlatParams:
    """Flat bf16 parameter / gradient buffers with named views."""

    def __init__(self, device):
        self.device = device
        self.specs = []          # (name, shape, offset)
        self.n = 0

    def add(self, name, shape):
        numel = 1
        for s in shape:
            numel *= s
        self.specs.append((name, tuple(shape), self.n))
        self.n += (numel + 127) // 128 * 128          # 256-byte aligned views
        return len(self.specs) - 1

    def align(self, multiple):
        """Pad so that the next tensor starts at a multiple of `multiple` elements (bucket boundaries: every ZeRO-1 bucket
        then divides evenly over the ranks and the collectives run in place, without staging copies)."""
        self.n = (self.n + multiple - 1) // multiple * multiple

    def finalize(self, pad_to=1):
        self.n = (self.n + pad_to - 1) // pad_to * pad_to
        self.p = torch.zeros(self.n, dtype=BF, device=self.device)
        self.g = torch.zeros(self.n, dtype=BF, device=self.device)
        self.view = {}
        self.gview = {}
        for name, shape, off in self.specs:
            numel = 1
            for s in shape:
                numel *= s
            self.view[name] = self.p[off:off + numel].view(shape)
            self.gview[name] = self.g[off:off + numel].view(shape)

    def offset_of(self, name):
        for n, _, off in self.specs:
            if n == name:
                return off
        raise KeyError(name)


def cut_buckets(bounds):
    """[(lo, hi)] from the ascending list of bucket ends; an end that repeats (a model with fewer layers than one bucket holds) makes no empty bucket."""
    buckets, lo = [], 0
    for hi in bounds:
        if hi > lo:
            buckets.append((lo, hi))
            lo = hi
    return buckets


OPTIMIZERS = ('adamw', 'adamw8bit')


def check_optimizer(optimizer):
    if optimizer not in OPTIMIZERS:
        raise ValueError(f"optimizer={optimizer!r}: 'adamw' (fp32 moments) | 'adamw8bit' (block-wise 8-bit moments)")
    return optimizer


def plan_state_blocks(specs, shards, block=128, min_8bit=4096):
    """Which blocks of this rank's shards keep fp32 moments under optimizer='adamw8bit': every block of a tensor with fewer than `min_8bit` elements
    (bitsandbytes' `min_8bit_size`: norm weights and small biases stay exact in the reference).  `specs` = FlatParams.specs [(name, shape, offset)],
    `shards` = [(lo, hi, per)] per bucket.  Returns one list per shard, an entry per block: -1 = 8-bit state, k >= 0 = the block's moments are the
    k-th 128 of the shard's fp32 side arrays (dense, in block order).  Tensors start on multiples of `block` and shards start and end on them, so a block
    belongs to one tensor (or to padding, which stays 8-bit: zero codes forever) and its kind does not depend on the world size."""
    small = set()
    for _, shape, off in specs:
        numel = 1
        for s in shape:
            numel *= s
        assert off % block == 0, 'tensors start on block boundaries'
        if numel < min_8bit:
            small.update(range(off // block, (off + numel + block - 1) // block))
    out = []
    for lo, hi, _ in shards:
        assert lo % block == 0 and hi % block == 0, 'shards start and end on block boundaries'
        slots, k = [], 0
        for b in range(lo // block, hi // block):
            if b in small:
                slots.append(k)
                k += 1
            else:
                slots.append(-1)
        out.append(slots)
    return out


@contextlib.contextmanager
def behind_current(stream):
    """`stream` as the current stream, behind everything the current stream has queued so far."""
    ev = torch.cuda.Event()
    ev.record()
    with torch.cuda.stream(stream):
        stream.wait_event(ev)
        yield


class ParamGroup:
    """A finalised `FlatParams` (`fp`) cut into `buckets` [(lo, hi)]; ZeRO-1: rank r owns the slice `shards[b]` = (lo, hi, per) of every bucket and keeps
    its fp32 `master` weights and AdamW moments `m` / `v`, all shards back to back (`shard_off[b]` = where bucket b's begins).  Base class of the trainers:
    WHEN a bucket is reduced, updated or gathered, and on which stream, is their policy.

    optimizer='adamw8bit' (the reference VLA trainer's bnb.optim.AdamW8bit, train.py:251-255,278-282): no fp32 `m` / `v`; per 128-element block of the
    shard 128 uint8 codes in `m_code` / `v_code` and one fp32 `m_absmax` / `v_absmax` each (moment = code table[code] * absmax, ops.adamw8_codes()); the
    blocks of tensors below 4096 elements keep fp32 moments in `m32` / `v32`, found through `slot` (`plan_state_blocks`).  The masters stay fp32."""

    def init_group(self, fp, bounds, world, rank, optimizer='adamw'):
        self.fp, self.world, self.rank = fp, world, rank
        self.optimizer = check_optimizer(optimizer)
        self.buckets = cut_buckets(bounds)
        # (bucket lengths are multiples of 128 * world: every rank's slice is whole and the collectives run in place)
        assert all((hi - lo) % (128 * world) == 0 for lo, hi in self.buckets), 'ZeRO-1 buckets must divide evenly over the ranks'
        self.shards = dp.plan_shards(self.buckets, world, rank)
        n_shard = sum(hi - lo for lo, hi, _ in self.shards)
        self.master = torch.zeros(n_shard, dtype=F32, device=fp.device)
        eight = self.optimizer == 'adamw8bit'
        if eight:
            # (every shard starts and ends on a multiple of 128: the block grid is the same for every world size, and no block straddles two tensors)
            assert all(lo % 128 == 0 and hi % 128 == 0 for lo, hi, _ in self.shards), 'ZeRO-1 shards must start and end on 128-element blocks'
            plan = plan_state_blocks(fp.specs, self.shards)
            n_small = 128 * sum(sum(1 for k in sl if k >= 0) for sl in plan)
            self.m_code = torch.full((n_shard,), 127, dtype=torch.uint8, device=fp.device)          # the zero code of the signed table
            self.v_code = torch.zeros(n_shard, dtype=torch.uint8, device=fp.device)                 # ... of the unsigned one
            self.m_absmax = torch.zeros(n_shard // 128, dtype=F32, device=fp.device)
            self.v_absmax = torch.zeros(n_shard // 128, dtype=F32, device=fp.device)
            self.slot = torch.tensor([k for sl in plan for k in sl], dtype=torch.int32).to(fp.device)
            self.m32 = torch.zeros(n_small, dtype=F32, device=fp.device)
            self.v32 = torch.zeros(n_small, dtype=F32, device=fp.device)
        else:
            self.m = torch.zeros(n_shard, dtype=F32, device=fp.device)
            self.v = torch.zeros(n_shard, dtype=F32, device=fp.device)
        self.shard_off, self._opt_args, o, o32 = [], [], 0, 0
        for b, (lo, hi, _) in enumerate(self.shards):
            n = hi - lo
            self.master[o:o + n].copy_(fp.p[lo:hi].float())
            self.shard_off.append(o)
            # AdamW's operands of the bucket, sliced once: (param, master, m, v, grad), or None where this rank owns nothing of it; 8-bit mode:
            # (param, master, m_code, v_code, m_absmax, v_absmax, slot, m32, v32, grad) -- the slots of a shard count from its own slice of m32 / v32
            if n == 0:
                self._opt_args.append(None)
            elif eight:
                n32 = 128 * sum(1 for k in plan[b] if k >= 0)
                small = (self.slot[o // 128:(o + n) // 128], self.m32[o32:o32 + n32], self.v32[o32:o32 + n32]) if n32 else (None, None, None)
                self._opt_args.append((fp.p[lo:hi], self.master[o:o + n], self.m_code[o:o + n], self.v_code[o:o + n], self.m_absmax[o // 128:(o + n) // 128],
                                       self.v_absmax[o // 128:(o + n) // 128], *small, fp.g[lo:hi]))
                o32 += n32
            else:
                self._opt_args.append((fp.p[lo:hi], self.master[o:o + n], self.m[o:o + n], self.v[o:o + n], fp.g[lo:hi]))
            o += n
        self.gacc = None         # fp32 gradient accumulator (allocated by the first step of several samples)

    def add_sumsq(self, gnorm2, ws, b=None):
        """gnorm2 += the sum of squares of this rank's (reduced) gradient shards: of every bucket, or of bucket b alone."""
        for a in self._opt_args if b is None else self._opt_args[b:b + 1]:
            if a is not None:
                ops.sumsq(a[-1], gnorm2, ws)

    def adamw_bucket(self, b, lr, betas, eps, wd, gnorm2, max_norm, step):
        """AdamW on this rank's shard of bucket b; the clip factor max_norm / (||g|| + 1e-6) is resolved inside the kernel from the device-resident
        squared norm."""
        a = self._opt_args[b]
        if a is None:
            return
        if self.optimizer == 'adamw8bit':
            ops.adamw8_clipped(*a, lr, betas[0], betas[1], eps, wd, 1.0, gnorm2, max_norm, step)
        else:
            ops.adamw_clipped(*a, lr, betas[0], betas[1], eps, wd, 1.0, gnorm2, max_norm, step)

    def reduce_scatter_bucket(self, b, comm_stream, pg, capi=None):
        """Mean reduce-scatter of bucket b's gradients on the comm stream (RCCL), behind what the current stream has queued."""
        with behind_current(comm_stream):
            dp.reduce_scatter_mean(self.fp.g, self.buckets[b], self.shards[b], pg, capi=capi)

    def all_gather_bucket(self, b, pg, capi=None):
        """All-gather of bucket b's updated bf16 parameters, on the CURRENT stream (the callers differ in the stream and in how many buckets share one event)."""
        dp.all_gather_params(self.fp.p, self.buckets[b], self.shards[b], pg, capi=capi)

    def accumulate_bucket(self, b, w, first, last):
        """Sample-wise gradient accumulation: acc (fp32) += w * g over bucket b (`first`: acc = w * g); on the `last` sample the sum is rounded back to
        bf16 into the gradient buffer."""
        if self.gacc is None:
            self.gacc = torch.zeros(self.fp.n, dtype=F32, device=self.fp.device)
        lo, hi = self.buckets[b]
        ops.grad_accumulate(self.fp.g[lo:hi], self.gacc[lo:hi], w, first, last)

    def params_from(self, src=None):
        """bf16 parameters of this rank's shards from fp32 values laid out like the masters (default: the masters themselves, after a resume -- the run
        then continues bit for bit; or an average of them, ModelAveraging)."""
        src = self.master if src is None else src
        for (lo, hi, _), o in zip(self.shards, self.shard_off):
            if hi > lo:
                self.fp.p[lo:hi].copy_(src[o:o + hi - lo].to(BF))

    def optimizer_state(self, prefix=''):
        """This rank's optimizer shard for a checkpoint (CPU tensors).  fp32 mode: `exp_avg` / `exp_avg_sq`; 8-bit mode: `optimizer: 'adamw8bit'`, the codes
        and absmax of both moments and the fp32 moments of the small tensors (`exp_avg_small` / `exp_avg_sq_small`)."""
        st = {prefix + 'shards': self.shards, prefix + 'master': self.master.cpu()}
        if self.optimizer == 'adamw8bit':
            st.update({prefix + 'optimizer': self.optimizer, prefix + 'exp_avg_code': self.m_code.cpu(), prefix + 'exp_avg_absmax': self.m_absmax.cpu(),
                       prefix + 'exp_avg_sq_code': self.v_code.cpu(), prefix + 'exp_avg_sq_absmax': self.v_absmax.cpu(),
                       prefix + 'exp_avg_small': self.m32.cpu(), prefix + 'exp_avg_sq_small': self.v32.cpu()})
        else:
            st.update({prefix + 'exp_avg': self.m.cpu(), prefix + 'exp_avg_sq': self.v.cpu()})
        return st

    def load_optimizer_state(self, st, prefix=''):
        """Inverse of `optimizer_state` (+ the file's `world` / `rank`): a shard written for another world size, rank or bucket layout raises -- resuming
        with someone else's moments would silently change the run.  The bf16 parameters are re-derived from the masters."""
        if prefix + 'master' not in st:
            raise ValueError(f"the optimizer shard holds no state '{prefix}master' for this parameter group")
        if st['world'] != self.world or st['rank'] != self.rank or [tuple(x) for x in st[prefix + 'shards']] != [tuple(x) for x in self.shards]:
            raise ValueError(f"optimizer shard '{prefix}master' was written for rank {st['rank']} of {st['world']} / another bucket layout")
        theirs = st.get(prefix + 'optimizer', 'adamw')          # (a shard without the key predates the 8-bit mode: fp32 moments)
        if theirs != self.optimizer:
            raise ValueError(f"optimizer shard '{prefix}master' holds optimizer={theirs!r} state, this trainer runs optimizer={self.optimizer!r}")
        self.master.copy_(st[prefix + 'master'])
        if self.optimizer == 'adamw8bit':
            self.m_code.copy_(st[prefix + 'exp_avg_code']); self.m_absmax.copy_(st[prefix + 'exp_avg_absmax'])
            self.v_code.copy_(st[prefix + 'exp_avg_sq_code']); self.v_absmax.copy_(st[prefix + 'exp_avg_sq_absmax'])
            self.m32.copy_(st[prefix + 'exp_avg_small']); self.v32.copy_(st[prefix + 'exp_avg_sq_small'])
        else:
            self.m.copy_(st[prefix + 'exp_avg']); self.v.copy_(st[prefix + 'exp_avg_sq'])
        self.params_from()


# ------------------------------------------------------------------------------------------------ layer codec
MLP1_KEYS = (('m0w', 'mlp1.0.weight'), ('m0b', 'mlp1.0.bias'), ('m1w', 'mlp1.1.weight'), ('m1b', 'mlp1.1.bias'), ('m3w', 'mlp1.3.weight'), ('m3b', 'mlp1.3.bias'))
DECODER_LAYER_NAMES = ('wqkv', 'bqkv', 'wo', 'wgu', 'wdown', 'ln_in', 'ln_post')


def decoder_layer_specs(llm):
    """(short name, shape) of the seven tensors of one Qwen decoder layer in kernel layout: q/k/v fused and permuted inside each head (ops.pack_qkv),
    gate/up interleaved in groups of 16 rows (ops.pack_gate_up)."""
    H, I = llm.hidden_size, llm.intermediate_size
    nq, nkv, hd = llm.num_attention_heads, llm.num_key_value_heads, llm.head_dim
    NQ = (nq + 2 * nkv) * hd
    return list(zip(DECODER_LAYER_NAMES, [(NQ, H), (NQ,), (H, nq * hd), (2 * I, H), (H, I), (H,), (H,)]))


def mlp1_specs(H, C4):
    """(short name, shape) of the projector: LayerNorm(C4) -> Linear(C4, H) -> GELU -> Linear(H, H)."""
    return list(zip([nm for nm, _ in MLP1_KEYS], [(C4,), (C4,), (H, C4), (H,), (H, H), (H,)]))


def pack_decoder_layer(sd, prefix, views, vp, head_dim):
    """HF tensors `sd[prefix + ...]` of one decoder layer -> kernel layout, written into `views[vp + short name]`."""
    g = lambda k: sd[prefix + k].to(device=views[vp + 'wo'].device, dtype=BF)
    wqkv, bqkv = ops.pack_qkv(g('self_attn.q_proj.weight'), g('self_attn.k_proj.weight'), g('self_attn.v_proj.weight'),
                              g('self_attn.q_proj.bias'), g('self_attn.k_proj.bias'), g('self_attn.v_proj.bias'), head_dim)
    views[vp + 'wqkv'].copy_(wqkv)
    views[vp + 'bqkv'].copy_(bqkv)
    views[vp + 'wo'].copy_(g('self_attn.o_proj.weight'))
    views[vp + 'wgu'].copy_(ops.pack_gate_up(g('mlp.gate_proj.weight'), g('mlp.up_proj.weight')))
    views[vp + 'wdown'].copy_(g('mlp.down_proj.weight'))
    views[vp + 'ln_in'].copy_(g('input_layernorm.weight'))
    views[vp + 'ln_post'].copy_(g('post_attention_layernorm.weight'))


def unpack_decoder_layer(views, vp, prefix, llm):
    """{HF name: tensor} of one decoder layer from the kernel-layout `views[vp + short name]` (parameters or gradients): copies in natural row order."""
    nq, nkv, hd, H = llm.num_attention_heads, llm.num_key_value_heads, llm.head_dim, llm.hidden_size
    w, b = views[vp + 'wqkv'], views[vp + 'bqkv']
    inv = torch.empty(hd, dtype=torch.long)
    inv[ops.head_perm(hd)] = torch.arange(hd)
    idx = (torch.arange(nq + 2 * nkv)[:, None] * hd + inv[None, :]).reshape(-1).to(w.device)
    wn, bn = w[idx], b[idx]              # natural row order: packed[head*128 + inv[d]] = natural[head*128 + d]
    out = {}
    for nm, lo, hi in (('q_proj', 0, nq * hd), ('k_proj', nq * hd, (nq + nkv) * hd), ('v_proj', (nq + nkv) * hd, (nq + 2 * nkv) * hd)):
        out[f'{prefix}self_attn.{nm}.weight'], out[f'{prefix}self_attn.{nm}.bias'] = wn[lo:hi].clone(), bn[lo:hi].clone()
    out[prefix + 'self_attn.o_proj.weight'] = views[vp + 'wo'].clone()
    gu = views[vp + 'wgu'].view(-1, 2, 16, H)
    out[prefix + 'mlp.gate_proj.weight'] = gu[:, 0].reshape(-1, H).clone()
    out[prefix + 'mlp.up_proj.weight'] = gu[:, 1].reshape(-1, H).clone()
    out[prefix + 'mlp.down_proj.weight'] = views[vp + 'wdown'].clone()
    out[prefix + 'input_layernorm.weight'] = views[vp + 'ln_in'].clone()
    out[prefix + 'post_attention_layernorm.weight'] = views[vp + 'ln_post'].clone()
    return out


def pack_mlp1(sd, views):
    for nm, k in MLP1_KEYS:
        views['mlp1.' + nm].copy_(sd[k].to(device=views['mlp1.' + nm].device, dtype=BF))


def unpack_mlp1(views):
    return {k: views['mlp1.' + nm].clone() for nm, k in MLP1_KEYS}
