"""LR policies per parameter group (rscotr_amd.optim.LrUpdater: mmcv 1.x's LrUpdaterHook formulas in iteration mode, restated
here in fp64), the optimizer dispatch, and FlatSGD's host side: state layout against torch.optim.SGD and resume through
build_runner.  Host logic only: FlatSGD's HIP launches are replaced by the same arithmetic in torch (the kernel itself:
tests/test_sgd_gpu.py)."""
import glob
import json
import math
import os

import numpy as np
import pytest
import torch

from test_hooks_cpu import Loader, Toy
from util import REF_CFG_DIR

T, WI, RATIO = 40, 5, 0.1
BASE = (1e-2, 1e-3)
POLICIES = dict(step=dict(policy='step', step=[3, 21], gamma=0.5),
                step_int=dict(policy='step', step=7, gamma=0.1, min_lr=2e-4),
                poly=dict(policy='poly', power=0.9, min_lr=1e-4),
                poly_default=dict(policy='poly'),
                cos_ratio=dict(policy='CosineAnnealing', min_lr_ratio=1e-2),
                cos_abs=dict(policy='CosineAnnealing', min_lr=1e-5))


def _regular(cfg, b, t):
    """The issue's closed forms, one group at a time, in Python floats (fp64)."""
    if cfg['policy'] == 'step':
        st = cfg['step']
        k = t // st if isinstance(st, int) else sum(1 for s in st if t >= s)
        lr = b * cfg.get('gamma', 0.1) ** k
        return max(lr, cfg['min_lr']) if cfg.get('min_lr') is not None else lr
    if cfg['policy'] == 'poly':
        m = cfg.get('min_lr', 0.0)
        return (b - m) * (1 - t / T) ** cfg.get('power', 1.0) + m
    target = b * cfg['min_lr_ratio'] if 'min_lr_ratio' in cfg else cfg['min_lr']
    return target + 0.5 * (b - target) * (math.cos(math.pi * t / T) + 1)


def _warm(kind, t):
    if kind is None or t >= WI:
        return 1.0
    return dict(constant=RATIO, linear=1 - (1 - t / WI) * (1 - RATIO), exp=RATIO ** (1 - t / WI))[kind]


@pytest.mark.parametrize('warmup', [None, 'constant', 'linear', 'exp'])
@pytest.mark.parametrize('name', sorted(POLICIES))
def test_policies_match_the_closed_forms(name, warmup):
    from rscotr_amd.optim import LrUpdater
    cfg = POLICIES[name]
    up = LrUpdater(**cfg) if warmup is None else LrUpdater(warmup=warmup, warmup_iters=WI, warmup_ratio=RATIO, **cfg)
    for t in (0, 1, WI - 1, WI, T // 2, T - 1):
        got = up.rates(np.array(BASE), t, T)
        assert got.shape == (2,) and got.dtype == np.float64
        for g, b in zip(got, BASE):
            want = _regular(cfg, b, t) * _warm(warmup, t)
            assert abs(g - want) <= 1e-12 * abs(want), (t, b, g, want)


def test_cosine_matches_torch_scheduler():
    from rscotr_amd.optim import LrUpdater
    b, min_lr = 1e-2, 1e-4
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=b)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T, eta_min=min_lr)
    up = LrUpdater(policy='CosineAnnealing', min_lr=min_lr)
    for t in range(T):
        assert abs(up.rates(np.array([b]), t, T)[0] - sched.get_last_lr()[0]) <= 1e-9, t
        opt.step()
        sched.step()


def test_groups_with_different_base_rates_share_no_factor():
    from rscotr_amd.optim import LrUpdater
    up = LrUpdater(policy='poly', min_lr=1e-4)
    a, b = up.rates(np.array([1e-2, 1e-3]), T // 2, T)
    assert a == pytest.approx((1e-2 - 1e-4) * 0.5 + 1e-4, rel=1e-12) and b == pytest.approx((1e-3 - 1e-4) * 0.5 + 1e-4, rel=1e-12)
    assert abs(a / b - 10) > 0.5  # (5.05e-3 / 5.5e-4 = 9.18: one scalar factor on the base rates cannot give both)


def test_step_with_min_lr_clamps():
    from rscotr_amd.optim import LrUpdater
    up = LrUpdater(policy='step', step=[2, 4], gamma=0.1, min_lr=5e-4)
    base = np.array([1e-2, 1e-3])
    assert np.array_equal(up.rates(base, 1, None), base)
    assert np.allclose(up.rates(base, 2, None), [1e-3, 5e-4], rtol=1e-12, atol=0)
    assert np.allclose(up.rates(base, 9, None), [5e-4, 5e-4], rtol=1e-12, atol=0)


def test_refusals_name_the_key():
    from rscotr_amd.optim import LrUpdater
    from rscotr_amd.runner import IterBasedRunner
    with pytest.raises(ValueError, match='max_iters'):
        LrUpdater(policy='poly').rates(np.array([1e-2]), 0, None)
    for kw, word in ((dict(policy='poly', by_epoch=True), 'by_epoch'),
                     (dict(policy='poly', warmup='linear', warmup_iters=2, warmup_by_epoch=True), 'warmup_by_epoch'),
                     (dict(policy='cyclic'), 'cyclic'), (dict(policy='poly', momentum=0.9), 'momentum'),
                     (dict(step=[3]), 'policy'), (dict(policy='step', step=[3], warmup='cosine', warmup_iters=2), 'cosine')):
        with pytest.raises(NotImplementedError, match=word):
            LrUpdater(**kw)
    with pytest.raises(ValueError, match='exactly one'):
        LrUpdater(policy='CosineAnnealing', min_lr=1e-4, min_lr_ratio=0.1)
    with pytest.raises(ValueError, match='exactly one'):
        LrUpdater(policy='CosineAnnealing')
    # the runner refuses at construction, and reads max_iters when the first iteration asks for a rate
    with pytest.raises(NotImplementedError, match='cyclic'):
        IterBasedRunner(Toy(), None, Loader(), lr_config=dict(policy='cyclic'), graph_tasks=())


def test_build_optimizer_dispatches_on_type(sgd_on_cpu):
    from rscotr_amd.optim import FlatAdamW, FlatSGD, build_optimizer
    opt = build_optimizer(Toy(), dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0005,
                                      paramwise_cfg=dict(custom_keys={'backbone': dict(lr_mult=0.1)})),
                          dict(grad_clip=dict(max_norm=0.5)))
    try:
        assert type(opt) is FlatSGD and opt.momentum == 0.9 and opt.dampening == 0.0 and not opt.nesterov and opt.max_norm == 0.5
        assert not hasattr(opt, 'flat_v') and opt.flat_m.shape == opt.flat_p.shape
        assert list(opt.base_lr) == [0.01 * 0.1] * 2 + [0.01] * 4  # (paramwise_cfg is shared with the AdamW branch)
    finally:
        opt.close()
    opt = build_optimizer(Toy(), dict(type='SGD', lr=0.01))
    assert not hasattr(opt, 'flat_m')  # momentum == 0: no buffer arena
    opt.close()
    opt = build_optimizer(Toy(), dict(type='AdamW', lr=0.01))
    assert type(opt) is FlatAdamW
    opt.close()
    with pytest.raises(NotImplementedError, match='Adam'):
        build_optimizer(Toy(), dict(type='Adam', lr=0.01))
    with pytest.raises(ValueError, match='Nesterov'):
        build_optimizer(Toy(), dict(type='SGD', lr=0.01, momentum=0.9, dampening=0.1, nesterov=True))


def _torch_sgd_step(self, table=None):
    """FlatSGD.launch_step in torch: clip_grad_norm_(max_norm) + the SGD rule on the live segments (csrc/optim.hip)."""
    dyn = (self._dyn_host if table is None else table).numpy()
    g = self.flat_g
    live = torch.zeros(self.total)
    for i, (grp, o) in enumerate(zip(self.groups, self.offsets)):
        if dyn[i, 4]:
            live[o:o + grp['param'].numel()] = 1
    norm = float((g * live).double().pow(2).sum().sqrt())
    scale = min(1.0, self.max_norm / (norm + 1e-6)) if self.max_norm > 0 else 1.0
    with torch.no_grad():
        for i, (grp, o) in enumerate(zip(self.groups, self.offsets)):
            if not dyn[i, 4]:
                continue
            n = grp['param'].numel()
            p = self.flat_p[o:o + n]
            d = g[o:o + n] * scale + float(dyn[i, 1]) * p
            if self.momentum != 0:
                buf = self.flat_m[o:o + n]
                if dyn[i, 5]:
                    buf.copy_(d)
                else:
                    buf.mul_(self.momentum).add_(d, alpha=1 - self.dampening)
                d = d + self.momentum * buf if self.nesterov else buf
            p.add_(d, alpha=-float(dyn[i, 0]))


@pytest.fixture
def sgd_on_cpu(monkeypatch):
    from rscotr_amd.optim import FlatSGD
    monkeypatch.setattr(FlatSGD, 'launch_step', _torch_sgd_step)


@pytest.mark.parametrize('momentum,dampening', [(0.9, 0.1), (0.5, 0.0)])
def test_state_dict_has_the_layout_of_torch_sgd(sgd_on_cpu, momentum, dampening):
    from rscotr_amd.optim import FlatSGD
    g = torch.Generator().manual_seed(0)
    shapes, lrs, wds = [(5, 3), (7,), (2, 2)], [1e-2, 1e-3, 5e-3], [5e-4, 0.0, 1e-2]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt = FlatSGD([dict(name=str(i), param=p, lr=lr, weight_decay=wd) for i, (p, lr, wd) in enumerate(zip(ps, lrs, wds))],
                  momentum=momentum, dampening=dampening)
    topt = torch.optim.SGD([dict(params=[p], lr=lr, weight_decay=wd) for p, lr, wd in zip(ref, lrs, wds)], lr=1.0,
                           momentum=momentum, dampening=dampening, foreach=False)
    try:
        for step in range(2):
            opt.zero_grad()
            for i in (0, 2):  # tensor 1 never receives a gradient: no state entry on either side
                gr = torch.randn(shapes[i], generator=g)
                ps[i].grad.add_(gr)
                opt.live[i] = True
                ref[i].grad = gr.clone()
            opt.step()
            topt.step()
        ours, theirs = opt.state_dict(), topt.state_dict()
        assert set(ours) == set(theirs) == {'state', 'param_groups'}
        assert set(ours['state']) == set(theirs['state']) == {0, 2}
        for i in ours['state']:
            assert set(ours['state'][i]) == set(theirs['state'][i]) == {'momentum_buffer'}
            assert torch.allclose(ours['state'][i]['momentum_buffer'], theirs['state'][i]['momentum_buffer'], rtol=1e-6, atol=1e-8)
        # the groups of torch 1.11's SGD as mmcv leaves them (`initial_lr` from its LrUpdaterHook); later torch versions add
        # switches of their own implementation, which say nothing about the update
        later = {'foreach', 'differentiable', 'fused'}
        for a, b in zip(ours['param_groups'], theirs['param_groups']):
            assert set(a) - {'initial_lr'} == set(b) - later - {'initial_lr'}
            assert set(a) == {'lr', 'initial_lr', 'momentum', 'dampening', 'weight_decay', 'nesterov', 'maximize', 'params'}
            assert all(a[k] == b[k] for k in ('lr', 'momentum', 'dampening', 'weight_decay', 'nesterov', 'maximize', 'params'))
        for a, b in zip(ps, ref):
            assert torch.allclose(a, b, rtol=1e-6, atol=1e-8)
        # a torch.optim.SGD state dict resumes here: buffers, liveness, and "the first step is behind us"
        qs = [torch.nn.Parameter(p.detach().clone()) for p in ref]
        opt.close()
        opt = FlatSGD([dict(name=str(i), param=p, lr=lr, weight_decay=wd) for i, (p, lr, wd) in enumerate(zip(qs, lrs, wds))],
                      momentum=momentum, dampening=dampening)
        opt.load_state_dict(theirs)
        assert list(opt.live) == [True, False, True] and list(opt.steps) == [1, 0, 1]
        for i in (0, 2):
            o, n = opt.offsets[i], qs[i].numel()
            assert torch.equal(opt.flat_m[o:o + n].view(shapes[i]), theirs['state'][i]['momentum_buffer'])
        assert float(opt.flat_m[opt.offsets[1]:opt.offsets[1] + 7].abs().max()) == 0.0
        # ... and goes on like torch does, and ours loads there
        topt.load_state_dict(ours)
        opt.zero_grad()
        for i in (0, 2):
            gr = torch.randn(shapes[i], generator=g)
            qs[i].grad.add_(gr)
            ref[i].grad = gr.clone()
        opt.step()
        topt.step()
        for a, b in zip(qs, ref):
            assert torch.allclose(a, b, rtol=1e-6, atol=1e-8)
    finally:
        opt.close()


def test_sgd_without_momentum_keeps_liveness_through_its_state_dict(sgd_on_cpu):
    """torch 1.11's layout for momentum == 0: an entry with `momentum_buffer: None` per stepped tensor — what keeps a resumed
    tensor decaying on the iterations of other tasks."""
    from rscotr_amd.optim import FlatSGD
    ps = [torch.nn.Parameter(torch.ones(3)) for _ in range(2)]
    opt = FlatSGD([dict(name=str(i), param=p, lr=0.1, weight_decay=0.5) for i, p in enumerate(ps)])
    try:
        opt.zero_grad()
        ps[1].grad.add_(1.0)
        opt.live[1] = True
        opt.step()
        assert torch.equal(ps[0].detach(), torch.ones(3)) and torch.allclose(ps[1].detach(), torch.full((3,), 1 - 0.1 * 1.5))
        sd = opt.state_dict()
        assert sd['state'] == {1: dict(momentum_buffer=None)}
        opt.load_state_dict(sd)
        assert list(opt.live) == [False, True]
    finally:
        opt.close()


class _Fork(torch.autograd.Function):
    """The shape of ops.layer_norm_fork: (f(x, w), x); when nothing reads the first output, backward returns None for w."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, w)
        return x * w, x

    @staticmethod
    def backward(ctx, dy, dres):
        x, w = ctx.saved_tensors
        if dy is None:
            from rscotr_amd import ops
            ops.STATE.grad_sink.no_gradient(w)
            return dres, None
        return dy * w + (0 if dres is None else dres), (dy * x).sum(0)


def test_an_undefined_gradient_does_not_make_a_tensor_live(sgd_on_cpu):
    """backbone.norm0.* on the device path: autograd runs a leaf's hooks also for a gradient nobody computed.  Such a tensor
    must stay untouched (no weight decay), as under torch, while the gradient-ready observers still hear of it."""
    from rscotr_amd.optim import FlatSGD
    w, v = torch.nn.Parameter(torch.ones(4)), torch.nn.Parameter(torch.ones(4))
    opt = FlatSGD([dict(name='w', param=w, lr=0.1, weight_decay=0.5), dict(name='v', param=v, lr=0.1, weight_decay=0.5)], momentum=0.9)
    ready = []
    opt.ready_callbacks.append(ready.append)
    try:
        x = torch.randn(3, 4)
        for used in (False, True):
            opt.zero_grad()
            o, res = _Fork.apply(x * v, w)
            (res.sum() + (o.sum() if used else 0)).backward()
            opt.step()
            assert sorted(ready) == [0, 1] and list(opt.live) == [used, True]
            assert torch.equal(w.detach(), torch.ones(4)) != used
            ready.clear()
    finally:
        opt.close()


def _cfg(tmp_path, **over):
    cfg = dict(optimizer=dict(type='SGD', lr=1e-2, momentum=0.9, dampening=0.1, weight_decay=5e-4,
                              paramwise_cfg=dict(custom_keys={'backbone': dict(lr_mult=0.1)})),
               optimizer_config=dict(grad_clip=dict(max_norm=0.5, norm_type=2)),
               lr_config=dict(policy='poly', power=0.9, min_lr=1e-4, warmup='linear', warmup_iters=2, warmup_ratio=0.1),
               runner=dict(type='IterBasedRunner', max_iters=6), checkpoint_config=dict(interval=3),
               log_config=dict(interval=3, hooks=[dict(type='TextLoggerHook')]), work_dir=str(tmp_path), resume_from=None,
               load_from=None)
    cfg.update(over)
    return cfg


def _run(tmp_path, upto=None, **over):
    from rscotr_amd.runner import build_runner
    torch.manual_seed(0)
    model = Toy()
    lines = []
    runner = build_runner(model, _cfg(tmp_path, **over), Loader(), graph_tasks=(), logger=lines.append, timestamp='t0')
    runner.data_loader.i = runner.iter
    runner.run(upto)
    return runner, model, lines


def test_sgd_poly_warmup_resumes_like_the_uninterrupted_run(tmp_path, sgd_on_cpu):
    from rscotr_amd.optim import FlatSGD
    full, model_full, _ = _run(tmp_path / 'full')
    assert type(full.optimizer) is FlatSGD
    part, _, _ = _run(tmp_path / 'part', upto=3)
    assert part.iter == 3
    resumed, model_res, lines = _run(tmp_path / 'part', auto_resume=True)
    assert any('resumed from' in l and 'iter 3' in l for l in lines) and resumed.iter == 6
    for (k, a), b in zip(model_full.state_dict().items(), model_res.state_dict().values()):
        assert torch.equal(a, b), k
    assert torch.equal(full.optimizer.flat_m, resumed.optimizer.flat_m) and float(full.optimizer.flat_m.abs().max()) > 0
    # seg_head went live one iteration after the others: 6, 6, 6, 6, 5, 5 — the counts travel in the checkpoint's meta
    assert list(full.optimizer.steps) == list(resumed.optimizer.steps) == [6, 6, 6, 6, 5, 5]
    recs = [[json.loads(l) for l in open(os.path.join(tmp_path, d, 't0.log.json'))] for d in ('full', 'part')]
    assert [r['iter'] for r in recs[0]] == [r['iter'] for r in recs[1]] == [3, 6]
    assert [r['lr'] for r in recs[0]] == [r['lr'] for r in recs[1]]
    # the logged rate is the first group's (backbone.weight: lr_mult 0.1) at the iteration that was just run
    b = 1e-2 * 0.1
    assert recs[0][0]['lr'] == pytest.approx((b - 1e-4) * (1 - 2 / 6) ** 0.9 + 1e-4, rel=1e-12)
    assert recs[0][1]['lr'] == pytest.approx((b - 1e-4) * (1 - 5 / 6) ** 0.9 + 1e-4, rel=1e-12)
    sd = full.optimizer.state_dict()
    assert sd['param_groups'][0]['lr'] == recs[0][1]['lr'] and sd['param_groups'][0]['initial_lr'] == b
    assert sd['param_groups'][2]['lr'] == pytest.approx((1e-2 - 1e-4) * (1 - 5 / 6) ** 0.9 + 1e-4, rel=1e-12)
    # the rates of the warm-up went into the tables the steps read: iteration 0 ran at 0.1 of its regular rate
    first, _, _ = _run(tmp_path / 'one', upto=1)
    assert float(first.optimizer._dyn_host[2, 0]) == pytest.approx(1e-2 * 0.1, rel=1e-6)  # (fp32 table)
    assert float(first.optimizer._dyn_host[0, 0]) == pytest.approx(1e-3 * 0.1, rel=1e-6)
    assert list(first.optimizer._dyn_host[:, 5]) == [1, 1, 1, 1, 0, 0]  # first step of backbone and cls_head, seg_head not live


def _step_configs():
    from rscotr_amd import Config
    out = []
    for path in sorted(glob.glob(os.path.join(REF_CFG_DIR, '*.py'))):
        lr_config = Config.fromfile(path).get('lr_config')
        if lr_config is not None:
            out.append((os.path.basename(path), dict(lr_config)))
    return out


def test_step_configs_keep_their_rates_to_the_bit():
    from rscotr_amd.optim import FlatAdamW, LrUpdater, StepLrUpdater
    cfgs = _step_configs()
    assert len(cfgs) >= 4 and all(c['policy'] == 'step' for _, c in cfgs)
    ps = [torch.nn.Parameter(torch.zeros(3)) for _ in range(2)]
    opt = FlatAdamW([dict(name=str(i), param=p, lr=lr, weight_decay=0.0) for i, (p, lr) in enumerate(zip(ps, (1e-4, 1e-5)))])
    try:
        for name, c in cfgs:
            old = StepLrUpdater(**{k: v for k, v in c.items() if k != 'policy'})
            new = LrUpdater(**c)
            steps = c['step'] if isinstance(c['step'], (list, tuple)) else [c['step'], 2 * c['step']]
            for s in steps:
                for t in (0, s - 1, s, s + 1):
                    want = opt.base_lr * old.factor(t)  # (what set_lr_factor put into column 0 before there were rate vectors)
                    got = new.rates(opt.base_lr, t, None)
                    assert np.array_equal(got, want), (name, t)
                    opt.set_lrs(got)
                    opt.prepare_step()
                    assert np.array_equal(opt._dyn_host[:, 0].numpy(), want.astype(np.float32)), (name, t)
                    opt.set_lr_factor(old.factor(t))
                    assert np.array_equal(opt.lrs, want)
    finally:
        opt.close()
