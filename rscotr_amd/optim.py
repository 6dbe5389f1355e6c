"""Optimizer side of the co-training step.

* `build_param_groups` — mtl/utils/optimizer.py:25-55 (`MTLOptimizerConstructor`) on top of mmcv's
  `DefaultOptimizerConstructor.add_params`: ONE group per parameter, `custom_keys` matched as
  substrings of the parameter name, longest key first (ties alphabetical), first match wins.
* `FlatAdamW` — zero_grad -> (backward) -> clip_grad_norm_ -> AdamW.step of mmcv's OptimizerHook
  (mtl/apis/train.py:66-83; cfg ...potsdam.py:203-213) as two HIP launches over flat arenas.
  torch-1.11 semantics are kept: `zero_grad()` zero-fills, so once a parameter has received its
  first gradient it is updated on EVERY step (momentum decay + weight decay on steps of other
  tasks), and parameters that never receive one (e.g. `backbone.norm0.*`) are never touched.
* `FlatSGD` — the same hook with torch.optim.SGD (configs/_base_/seg/schedule_80k.py) on the same arenas
  (`FlatArena` is what the two share), without a second-moment arena.
* `LrUpdater` — mmcv 1.x `LrUpdaterHook` (step / poly / CosineAnnealing, with warm-up) as forced to iteration
  mode by `IterBasedRunner`: one rate per parameter group, a function of the iteration alone.
* `StepLrUpdater` — the decay factor of mmcv's `StepLrUpdaterHook` (`LrUpdater` uses it for policy 'step').
"""
import math

import numpy as np
import torch

from . import ops
from ._lib import lib

CHUNK = 4096  # elements per workgroup in the optimizer kernels (16 KB per arena)


def build_param_groups(model, optimizer_cfg):
    """-> list of dict(name, param, lr, weight_decay) in `named_parameters()` order."""
    if hasattr(model, 'module'):
        model = model.module
    cfg = dict(optimizer_cfg)
    base_lr = cfg['lr']
    base_wd = cfg.get('weight_decay', None)
    pw = cfg.get('paramwise_cfg') or {}
    custom_keys = pw.get('custom_keys', {})
    sorted_keys = sorted(sorted(custom_keys.keys()), key=len, reverse=True)
    bias_lr_mult = pw.get('bias_lr_mult', 1.)
    bias_decay_mult = pw.get('bias_decay_mult', 1.)
    norm_decay_mult = pw.get('norm_decay_mult', 1.)
    norm_types = (torch.nn.modules.batchnorm._BatchNorm, torch.nn.GroupNorm, torch.nn.LayerNorm,
                  torch.nn.modules.instancenorm._InstanceNorm)
    groups, seen = [], set()

    def add(module, prefix):
        is_norm = isinstance(module, norm_types)
        for name, param in module.named_parameters(recurse=False):
            if id(param) in seen:
                continue
            seen.add(id(param))
            full = f'{prefix}.{name}' if prefix else name
            g = dict(name=full, param=param, lr=base_lr, weight_decay=base_wd if base_wd is not None else 0.0)
            if param.requires_grad:
                for key in sorted_keys:
                    if key in f'{prefix}.{name}':
                        g['lr'] = base_lr * custom_keys[key].get('lr_mult', 1.)
                        if base_wd is not None:
                            g['weight_decay'] = base_wd * custom_keys[key].get('decay_mult', 1.)
                        break
                else:
                    if name == 'bias' and not is_norm:
                        g['lr'] = base_lr * bias_lr_mult
                    if base_wd is not None:
                        if is_norm:
                            g['weight_decay'] = base_wd * norm_decay_mult
                        elif name == 'bias':
                            g['weight_decay'] = base_wd * bias_decay_mult
            groups.append(g)
        for child_name, child in module.named_children():
            add(child, f'{prefix}.{child_name}' if prefix else child_name)

    add(model, '')
    return groups


class StepLrUpdater:
    """lr_config = dict(policy='step', step=[...], gamma=0.1) evaluated per iteration."""

    def __init__(self, step, gamma=0.1, min_lr=None, **kwargs):
        self.step, self.gamma, self.min_lr = step, gamma, min_lr

    def factor(self, cur_iter):
        if isinstance(self.step, int):
            exp = cur_iter // self.step
        else:
            exp = len(self.step)
            for i, s in enumerate(self.step):
                if cur_iter < s:
                    exp = i
                    break
        return self.gamma ** exp


class LrUpdater:
    """`lr_config` of an mmcv 1.x config in iteration mode: `rates(base_lr, cur_iter, max_iters)` is the vector of the
    groups' rates for that iteration.  Per group, with b its base rate, t = cur_iter, T = max_iters:
      step             b * gamma**k, then max(., min_lr) when min_lr is given
      poly             (b - min_lr) * (1 - t / T)**power + min_lr
      CosineAnnealing  target + 0.5 * (b - target) * (cos(pi * t / T) + 1), target = b * min_lr_ratio or the absolute min_lr
    and for t < warmup_iters that rate times ratio ('constant'), 1 - (1 - t / warmup_iters) * (1 - ratio) ('linear') or
    ratio**(1 - t / warmup_iters) ('exp').  `min_lr` is an absolute rate, so groups with different base rates share no common
    factor: the schedule is a vector, not a scalar.  Every key is either honoured or refused by name."""

    POLICIES = dict(step=dict(step=None, gamma=0.1, min_lr=None), poly=dict(power=1.0, min_lr=0.0),
                    CosineAnnealing=dict(min_lr=None, min_lr_ratio=None))
    NEEDS_MAX_ITERS = ('poly', 'CosineAnnealing')

    def __init__(self, policy=None, by_epoch=False, warmup=None, warmup_iters=0, warmup_ratio=0.1, warmup_by_epoch=False,
                 **kwargs):
        if policy not in self.POLICIES:
            raise NotImplementedError(f'lr_config policy={policy!r}: one of {sorted(self.POLICIES)}')
        if by_epoch:
            raise NotImplementedError('lr_config by_epoch=True: the runner counts iterations (IterBasedRunner)')
        if warmup_by_epoch:
            raise NotImplementedError('lr_config warmup_by_epoch=True: the runner counts iterations (IterBasedRunner)')
        if warmup not in (None, 'constant', 'linear', 'exp'):
            raise NotImplementedError(f"lr_config warmup={warmup!r}: None, 'constant', 'linear' or 'exp'")
        unknown = sorted(set(kwargs) - set(self.POLICIES[policy]))
        if unknown:
            raise NotImplementedError(f'lr_config policy={policy!r} does not take {unknown}')
        self.policy = policy
        self.args = dict(self.POLICIES[policy], **kwargs)
        if policy == 'step':
            if self.args['step'] is None:
                raise ValueError("lr_config policy='step' needs step=int or [int, ...]")
            self.step_updater = StepLrUpdater(self.args['step'], self.args['gamma'])
        if policy == 'CosineAnnealing' and (self.args['min_lr'] is None) == (self.args['min_lr_ratio'] is None):
            raise ValueError("lr_config policy='CosineAnnealing' needs exactly one of min_lr and min_lr_ratio")
        self.warmup, self.warmup_iters, self.warmup_ratio = warmup, int(warmup_iters), float(warmup_ratio)
        if warmup is not None and not (self.warmup_iters > 0 and 0 < self.warmup_ratio <= 1.0):
            raise ValueError('lr_config warmup needs warmup_iters > 0 and 0 < warmup_ratio <= 1')

    def regular(self, base_lr, t, max_iters=None):
        b, a = np.asarray(base_lr, dtype=np.float64), self.args
        if self.policy == 'step':
            lr = b * self.step_updater.factor(t)
            return lr if a['min_lr'] is None else np.maximum(lr, a['min_lr'])
        if max_iters is None:
            raise ValueError(f'lr_config policy={self.policy!r} needs max_iters (runner=dict(max_iters=...) or run(max_iters))')
        if self.policy == 'poly':
            return (b - a['min_lr']) * (1 - t / max_iters) ** a['power'] + a['min_lr']
        target = b * a['min_lr_ratio'] if a['min_lr_ratio'] is not None else a['min_lr']
        return target + 0.5 * (b - target) * (math.cos(math.pi * t / max_iters) + 1)

    def rates(self, base_lr, t, max_iters=None):
        lr = self.regular(base_lr, t, max_iters)
        if self.warmup is None or t >= self.warmup_iters:
            return lr
        r, frac = self.warmup_ratio, t / self.warmup_iters
        k = r if self.warmup == 'constant' else 1 - (1 - frac) * (1 - r) if self.warmup == 'linear' else r ** (1 - frac)
        return lr * k


class FlatArena:
    """What the flat optimizers share: the arena layout and chunk tables, the GRAD_SINK protocol, liveness and step counts,
    zero_grad / grad_norm, the per-segment host table and the parameters' range words.  A subclass names its state arenas
    (`STATE`: (checkpoint key, attribute, snapshot key)), fills its columns of the table and launches its update kernel."""

    STATE = ()
    # Does a tensor whose backward node announced "no gradient" (no_gradient()) stay not live?  FlatAdamW: no — it keeps the
    # liveness rule it has always had (the leaf hook ran: live), so that its trajectories do not move by a bit; there the
    # difference is a decay of 1 - lr * wd = 1 - 5e-10 on norm weights of 1 and bias corrections that start a few iterations early.
    HONOUR_NO_GRADIENT = False

    def __init__(self, groups, grad_clip=None, order=None):
        """groups: output of build_param_groups. order: optional permutation of group indices that
        fixes the arena layout (used to make each task's parameter subset contiguous)."""
        self.groups = groups
        self.max_norm = float(grad_clip['max_norm']) if grad_clip else 0.0
        if grad_clip:
            assert grad_clip.get('norm_type', 2) == 2
        order = list(range(len(groups))) if order is None else list(order)
        params = [g['param'] for g in groups]
        device = params[0].device
        self.device = device
        offs, off = {}, 0
        for gi in order:
            offs[gi] = off
            off += (params[gi].numel() + 3) // 4 * 4  # 16-byte aligned segments
        self.total = off
        self.offsets = [offs[i] for i in range(len(groups))]
        ops.WPLANES.reset()  # (plane sets are keyed by arena addresses)
        self.flat_p = torch.zeros(off, dtype=torch.float32, device=device)
        self.flat_g = torch.zeros(off, dtype=torch.float32, device=device)
        for _, attr, _ in self.STATE:
            setattr(self, attr, torch.zeros(off, dtype=torch.float32, device=device))
        with torch.no_grad():
            for p, o in zip(params, self.offsets):
                n = p.numel()
                self.flat_p[o:o + n].copy_(p.detach().reshape(-1))
                p.data = self.flat_p[o:o + n].view(p.shape)
                p.grad = self.flat_g[o:o + n].view(p.shape)
        # static chunk tables
        seg, coff, clen = [], [], []
        for si, (p, o) in enumerate(zip(params, self.offsets)):
            n = (p.numel() + 3) // 4 * 4
            for c in range(0, n, CHUNK):
                seg.append(si)
                coff.append(o + c)
                clen.append(min(CHUNK, n - c))
        self.nchunks = len(seg)
        self.chunk_seg = torch.tensor(seg, dtype=torch.int32, device=device)
        self.chunk_off = torch.tensor(coff, dtype=torch.int64, device=device)
        self.chunk_len = torch.tensor(clen, dtype=torch.int32, device=device)
        n = len(groups)
        self.steps = np.zeros(n, dtype=np.int64)
        self.live = np.zeros(n, dtype=bool)
        self.base_lr = np.array([g['lr'] for g in groups], dtype=np.float64)
        self.wd = np.array([g['weight_decay'] for g in groups], dtype=np.float64)
        self.lr_factor = 1.0
        self.lrs = self.base_lr.copy()  # the groups' current rates: column 0 of the next step's table
        self._dyn_host = torch.zeros((n, 8), dtype=torch.float32, pin_memory=device.type == 'cuda')
        self.seg_dyn = torch.zeros((n, 8), dtype=torch.float32, device=device)
        self._dyn_event = None
        self.sumsq = torch.zeros(1 + 1024, dtype=torch.float32, device=device)  # [0] = total, [1:] = partials
        # value ranges of the parameters (bit pattern of max |w| per tensor) for the fp16 split product of the GEMMs:
        # refreshed by the update kernel for every tensor it steps, recomputed from the arena after any other change
        # (words of the operator layer's range buffer, ops.RANGES: one per parameter tensor, at the top of the buffer)
        self.seg_amax_ptr = ops.RANGES.param_region(max(n, 1), device) if device.type == 'cuda' else 0
        self.chunk_amax = torch.zeros(4 * max(self.nchunks, 1), dtype=torch.int32, device=device)  # (scratch: per-wavefront maxima of a chunk)
        self._seg_order = np.argsort(np.asarray(self.offsets, dtype=np.int64), kind='stable')
        self._seg_starts = np.asarray(self.offsets, dtype=np.int64)[self._seg_order]
        self.amax_dirty = True
        # gradient-ready notifications: autograd's AccumulateGrad (post hook) or the direct-write path
        # of rscotr_amd.ops (GRAD_SINK) both end in _on_ready(i)
        self.ready_callbacks = []
        self.written_callbacks = []  # grad_written(i) observers (GradSync: flush the deferred work bucket by bucket)
        self._no_grad = set()  # (no_gradient(): tensors whose hook will run in this backward pass without a gradient)
        self._hooks = [p.register_post_accumulate_grad_hook(self._make_hook(i))
                       for i, p in enumerate(params) if p.requires_grad]
        self._by_ptr = {p.data_ptr(): i for i, p in enumerate(params) if p.requires_grad and p.numel() > 0}
        ops.STATE.grad_sink = self

    def _make_hook(self, i):
        def hook(param):
            if i in self._no_grad:  # (the observers still hear of it: a gradient bucket waits for all its members)
                self._no_grad.discard(i)
                for cb in self.ready_callbacks:
                    cb(i)
            else:
                self._on_ready(i)
        return hook

    def no_gradient(self, *tensors):
        """A backward node returns None for these parameters (the out-norm of a backbone stage whose output no head of this
        task reads: ops.layer_norm_fork).  Autograd runs a leaf's hooks for an undefined gradient too; that is not "has received
        a gradient" and must not start the tensor's weight decay (torch leaves `.grad` None and skips it)."""
        for t in tensors:
            i = self._by_ptr.get(t.data_ptr()) if t is not None and self.HONOUR_NO_GRADIENT else None
            if i is not None:
                self._no_grad.add(i)

    def _on_ready(self, i):
        self.live[i] = True
        for cb in self.ready_callbacks:
            cb(i)

    # ---- GRAD_SINK protocol (rscotr_amd.ops): backward kernels add a parameter's gradient straight
    # into its slice of the (zero-filled) gradient arena instead of returning a tensor that autograd
    # would add with one more element-wise kernel per parameter.
    def is_param_ptr(self, ptr):
        """Does `ptr` point into the flat parameter arena (a parameter, or a slice of one)?"""
        base = self.flat_p.data_ptr()
        return base <= ptr < base + self.flat_p.numel() * 4

    def params_changed(self):
        """The arena was written by something other than the update kernel (checkpoint load, restore, state-dict copy)."""
        self.amax_dirty = True

    def refresh_amax(self):
        if self.device.type == 'cuda':
            lib.call('rscotr_param_amax', self.flat_p.data_ptr(), self.chunk_seg.data_ptr(), self.chunk_off.data_ptr(),
                     self.chunk_len.data_ptr(), self.nchunks, self.seg_amax_ptr, len(self.groups), self.chunk_amax.data_ptr(),
                     ops._stream())
        self.amax_dirty = False

    def amax_slot(self, ptr):
        """Address of the value-range word of the parameter that holds arena address `ptr` (0: not a parameter's memory)."""
        off = (ptr - self.flat_p.data_ptr()) // 4
        if not 0 <= off < self.total:
            return 0
        if self.amax_dirty:
            self.refresh_amax()
        k = int(np.searchsorted(self._seg_starts, off, side='right')) - 1
        return self.seg_amax_ptr + 4 * int(self._seg_order[k])

    def grad_view(self, tensor):
        """-> (index, view of the gradient arena shaped like `tensor`) if `tensor` IS a registered
        parameter or a contiguous reshaped alias of all of it (same storage start and size), else None."""
        i = self._by_ptr.get(tensor.data_ptr())
        if i is None:
            return None
        p = self.groups[i]['param']
        if p.numel() != tensor.numel() or not tensor.is_contiguous():
            return None
        # (a reshaped alias of the whole parameter — a convolution weight flattened to (O, C * k * k) for the GEMM — is the
        # same memory: its gradient goes to the same rows of the arena)
        return i, (p.grad if p.shape == tensor.shape else p.grad.view(tensor.shape))

    def grad_written(self, i):
        # while split-K weight gradients wait for their deferred combine (ops.DEFER), "written" is not true yet for any
        # of them: the notifications are replayed by ops.flush_deferred()
        if ops.DEFER.pending():
            ops.DEFER.notify.append(i)
        else:
            self._on_ready(i)
        for cb in self.written_callbacks:
            cb(i)

    def close(self):
        if ops.STATE.grad_sink is self:
            ops.STATE.grad_sink = None

    def mark_live(self, names):
        name2i = {g['name']: i for i, g in enumerate(self.groups)}
        for n in names:
            self.live[name2i[n]] = True

    def zero_grad(self):
        """torch 1.11 `Optimizer.zero_grad()`: zero-fill (never set to None) — one memset."""
        if ops.DEFER.pending() or ops.DEFER.notify:  # a backward pass that never reached its flush (exception path)
            ops.DEFER.drop()
        self._no_grad.clear()
        self.flat_g.zero_()

    def set_lr_factor(self, f):
        """Every group at its base rate times `f`."""
        self.lr_factor = float(f)
        self.lrs = self.base_lr * self.lr_factor

    def set_lrs(self, lrs):
        """One rate per group (LrUpdater.rates): what a schedule with an absolute floor or per-group base rates needs."""
        lrs = np.asarray(lrs, dtype=np.float64)
        if lrs.shape != self.base_lr.shape:
            raise ValueError(f'set_lrs: {lrs.shape} rates for {self.base_lr.shape[0]} parameter groups')
        self.lrs = lrs.copy()

    def grad_norm(self):
        """Device 0-d tensor with the pre-clip global L2 norm of the last step (no sync)."""
        ops.flush_deferred()
        return self.sumsq.sqrt()[0]

    def new_host_table(self):
        """A pinned per-segment table of its own for a captured iteration: the captured H2D copy reads it
        asynchronously, so it must not be the table the next (eager) iteration refills."""
        return torch.zeros_like(self._dyn_host).pin_memory() if self.device.type == 'cuda' else torch.zeros_like(self._dyn_host)

    def prepare_step(self, table=None):
        """Host half of a step: advance the per-tensor step counts of the live tensors and fill the
        pinned per-segment table {lr, wd, [the update rule's columns], live}.  No device work."""
        live = self.live
        self.steps[live] += 1
        if table is None and self._dyn_event is not None:
            # the shared pinned table is read by the previous step's asynchronous upload: do not refill it under that copy
            # (captured iterations own a table each and guard it with their `done` event)
            self._dyn_event.synchronize()
        dyn = (self._dyn_host if table is None else table).numpy()
        dyn[:, 0] = self.lrs
        dyn[:, 1] = self.wd
        dyn[:, 4] = live.astype(np.float32)
        self._fill_table(dyn)

    def launch_step(self, table=None):
        """Device half: table upload + global-norm pass + fused clip/update pass (capturable)."""
        ops.flush_deferred()  # (no-op unless a caller skipped the flush after backward)
        self.seg_dyn.copy_(self._dyn_host if table is None else table, non_blocking=True)
        if table is None and self.device.type == 'cuda':
            self._dyn_event = torch.cuda.Event()
            self._dyn_event.record()
        s = ops._stream()
        if self.max_norm > 0:
            lib.call('rscotr_grad_sumsq', self.flat_g.data_ptr(), self.chunk_seg.data_ptr(), self.chunk_off.data_ptr(),
                     self.chunk_len.data_ptr(), self.seg_dyn.data_ptr(), self.nchunks, self.sumsq.data_ptr(), s)
        ops.WPLANES.bump(by_optimizer=True)  # the parameters change: their pre-split planes are stale from here on
        if self.amax_dirty:  # (the words of the tensors this step does not touch must be valid too)
            self.refresh_amax()
        self._launch_update(s)

    def step(self):
        self.prepare_step()
        self.launch_step()

    def _state_views(self, i):
        g, o = self.groups[i], self.offsets[i]
        n = g['param'].numel()
        return {key: getattr(self, attr)[o:o + n].view(g['param'].shape) for key, attr, _ in self.STATE}

    def snapshot(self):
        """Weights, optimizer state and step counts (GraphedTask restores them after its warm-up iterations)."""
        return dict(p=self.flat_p.clone(), steps=self.steps.copy(), live=self.live.copy(),
                    **{k: getattr(self, attr).clone() for _, attr, k in self.STATE})

    def restore(self, snap):
        ops.WPLANES.bump()
        self.amax_dirty = True
        self.flat_p.copy_(snap['p'])
        for _, attr, k in self.STATE:
            getattr(self, attr).copy_(snap[k])
        self.steps[:] = snap['steps']
        self.live[:] = snap['live']
        self.refresh_amax()  # (now, not lazily: the next thing may be a hipGraph capture, which would record the refresh)

    def _load_state(self, sd):
        """The state arenas from a torch-layout state dict (one param group per parameter in the same order — mmcv's
        DefaultOptimizerConstructor builds exactly that, mtl/utils/optimizer.py); every tensor with an entry is live."""
        self.steps[:] = 0
        self.live[:] = False
        for _, attr, _ in self.STATE:
            getattr(self, attr).zero_()
        with torch.no_grad():
            for i, st in sd['state'].items():
                i = int(i)
                g = self.groups[i]
                for key, view in self._state_views(i).items():
                    if st.get(key) is None:  # (torch.optim.SGD: no buffer before a tensor's first step with momentum)
                        continue
                    assert tuple(st[key].shape) == tuple(g['param'].shape), (g['name'], key, tuple(st[key].shape))
                    view.copy_(st[key])
                self.steps[i] = int(st.get('step', 1))
                self.live[i] = True


class FlatAdamW(FlatArena):
    STATE = (('exp_avg', 'flat_m', 'm'), ('exp_avg_sq', 'flat_v', 'v'))

    def __init__(self, groups, betas=(0.9, 0.999), eps=1e-8, grad_clip=None, order=None):
        self.betas, self.eps = betas, eps
        super().__init__(groups, grad_clip=grad_clip, order=order)

    def _fill_table(self, dyn):
        """Columns 2, 3: 1/bc1, 1/sqrt(bc2) of each tensor's own step count."""
        b1, b2 = self.betas
        t = np.maximum(self.steps, 1).astype(np.float64)
        dyn[:, 2] = 1.0 / (1.0 - b1 ** t)
        dyn[:, 3] = 1.0 / np.sqrt(1.0 - b2 ** t)

    def _launch_update(self, s):
        b1, b2 = self.betas
        lib.call('rscotr_adamw_clip_step_r', self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.flat_m.data_ptr(),
                 self.flat_v.data_ptr(), self.chunk_seg.data_ptr(), self.chunk_off.data_ptr(), self.chunk_len.data_ptr(),
                 self.seg_dyn.data_ptr(), self.nchunks, self.sumsq.data_ptr(), self.max_norm, float(b1), float(b2),
                 float(self.eps), self.seg_amax_ptr, len(self.groups), self.chunk_amax.data_ptr(), s)

    # checkpoint interop with torch.optim.AdamW's state layout
    def state_dict(self):
        state = {i: dict(step=int(self.steps[i]), **{k: v.clone() for k, v in self._state_views(i).items()})
                 for i in range(len(self.groups)) if self.live[i]}
        # the param_groups of torch.optim.AdamW (torch 1.11) as mmcv leaves them: `initial_lr` is what mmcv's LrUpdaterHook
        # setdefault()s on resume — without it a reference resume past a decay step would take the decayed `lr` as the
        # base and decay it a second time
        return dict(state=state, param_groups=[dict(lr=float(self.lrs[i]), initial_lr=g['lr'],
                                                     weight_decay=g['weight_decay'], betas=self.betas, eps=self.eps,
                                                     amsgrad=False, maximize=False, params=[i])
                                                for i, g in enumerate(self.groups)])

    def load_state_dict(self, sd):
        """Inverse of state_dict(): also accepts a torch.optim.AdamW state dict saved by the reference."""
        self._load_state(sd)


class FlatSGD(FlatArena):
    """torch.optim.SGD (momentum, dampening, nesterov; weight decay added to the gradient) behind the same clip, as the
    norm pass + `rscotr_sgd_clip_step_r`.  No second-moment arena, and no momentum arena either when momentum == 0."""

    HONOUR_NO_GRADIENT = True  # (weight decay is part of SGD's gradient: a tensor torch would skip must not take it)

    def __init__(self, groups, momentum=0.0, dampening=0.0, nesterov=False, grad_clip=None, order=None):
        self.momentum, self.dampening, self.nesterov = float(momentum), float(dampening), bool(nesterov)
        if self.momentum < 0:
            raise ValueError(f'Invalid momentum value: {momentum}')
        if self.nesterov and (self.momentum <= 0 or self.dampening != 0):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')  # (torch.optim.SGD's words)
        self.STATE = (('momentum_buffer', 'flat_m', 'm'),) if self.momentum != 0 else ()
        super().__init__(groups, grad_clip=grad_clip, order=order)

    def _fill_table(self, dyn):
        """Column 5: this is the tensor's first step (its buffer becomes the gradient itself, without dampening)."""
        dyn[:, 5] = ((self.steps == 1) & self.live).astype(np.float32)

    def _launch_update(self, s):
        lib.call('rscotr_sgd_clip_step_r', self.flat_p.data_ptr(), self.flat_g.data_ptr(),
                 self.flat_m.data_ptr() if self.momentum != 0 else 0, self.chunk_seg.data_ptr(), self.chunk_off.data_ptr(),
                 self.chunk_len.data_ptr(), self.seg_dyn.data_ptr(), self.nchunks, self.sumsq.data_ptr(), self.max_norm,
                 self.momentum, self.dampening, int(self.nesterov), self.seg_amax_ptr, len(self.groups),
                 self.chunk_amax.data_ptr(), s)

    # checkpoint interop with torch.optim.SGD's state layout
    def state_dict(self):
        """torch.optim.SGD's layout, one param group per parameter.  It has no slot for a step count, and none is needed to
        resume: a tensor with a state entry has taken its first step (`step_counts()` carries the counts for the checkpoint's
        meta, so that a resumed run reports them as the uninterrupted one does)."""
        state = {i: ({k: v.clone() for k, v in self._state_views(i).items()} or dict(momentum_buffer=None))
                 for i in range(len(self.groups)) if self.live[i]}
        return dict(state=state, param_groups=[dict(lr=float(self.lrs[i]), initial_lr=g['lr'], momentum=self.momentum,
                                                     dampening=self.dampening, weight_decay=g['weight_decay'],
                                                     nesterov=self.nesterov, maximize=False, params=[i])
                                                for i, g in enumerate(self.groups)])

    def load_state_dict(self, sd):
        """Inverse of state_dict(): also accepts a torch.optim.SGD state dict saved by the reference."""
        self._load_state(sd)

    def step_counts(self):
        return [int(t) for t in self.steps]

    def load_step_counts(self, counts):
        """The step counts saved beside a state dict (checkpoint meta): only tensors the state dict made live take one."""
        counts = np.asarray(counts, dtype=np.int64)
        if counts.shape != self.steps.shape:
            raise ValueError(f'{counts.shape[0]} step counts for {self.steps.shape[0]} parameter groups')
        self.steps[self.live] = np.maximum(counts[self.live], 1)


def task_major_order(groups):
    """Arena order that makes each task's parameter subset a few contiguous ranges:
    backbone | neck | shared_encoder | bbox_head | seg_head | cls_head (cls = backbone+cls_head,
    det = backbone+neck+encoder+bbox_head, seg = backbone+neck+encoder+seg_head)."""
    rank = dict(backbone=0, neck=1, shared_encoder=2, bbox_head=3, seg_head=4, cls_head=5)
    idx = list(range(len(groups)))
    idx.sort(key=lambda i: (rank.get(groups[i]['name'].split('.')[0], 6), i))
    return idx


def build_optimizer(model, optimizer_cfg, optimizer_config=None):
    cfg = dict(optimizer_cfg)
    kind = cfg.get('type', 'AdamW')
    if kind not in ('AdamW', 'SGD'):
        raise NotImplementedError(f"optimizer type {kind!r}: 'AdamW' or 'SGD'")
    groups = build_param_groups(model, cfg)
    grad_clip = (optimizer_config or {}).get('grad_clip', None)
    if kind == 'SGD':
        return FlatSGD(groups, momentum=cfg.get('momentum', 0.0), dampening=cfg.get('dampening', 0.0),
                       nesterov=cfg.get('nesterov', False), grad_clip=grad_clip, order=task_major_order(groups))
    return FlatAdamW(groups, betas=tuple(cfg.get('betas', (0.9, 0.999))), eps=cfg.get('eps', 1e-8),
                     grad_clip=grad_clip, order=task_major_order(groups))
