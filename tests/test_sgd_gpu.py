"""Fused clip + SGD HIP kernel (rscotr_sgd_clip_step_r) vs torch.optim.SGD + clip_grad_norm_ (independent primitives), the
range words it leaves, a co-training run with SGD + poly against the oracle loop, and the schedule inside replayed hipGraphs."""
import copy

import numpy as np
import pytest
import torch

from util import build_model, load_model_cfg, state_to_oracle

pytestmark = pytest.mark.gpu

# odd tails, one element, one chunk boundary (4096 elements per workgroup) crossed once and twice
SHAPES = [(33, 7), (1,), (128, 64), (5,), (4097,), (8193,), (3, 3, 3, 3)]
LRS = [1e-2, 5e-3, 2e-2, 1e-3, 1e-2, 3e-3, 2e-2]
WDS = [1e-2, 0.0, 5e-4, 1e-2, 0.0, 5e-4, 1e-1]
# the gradients have 20 800 elements of unit variance times 10 or 0.01: norms of ~1440 and ~1.44, so a bound of 5 clips the
# odd steps and leaves the even ones alone
MAX_NORM = 5.0
SGD_OPTIM = dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0005)
POLY = dict(policy='poly', power=0.9, min_lr=1e-4)
# r = |w_graph - w_eager| / |w_eager - w_0| of the replay test, measured on an MI355X (profiles/README.md): 0.0 in every run —
# the replayed graphs run the eager loop's launches on the same inputs and no reduction of the path depends on timing.
R_MEASURED = 0.0
R_GATE = min(4 * R_MEASURED, 0.08)


def _words(ops, opt):
    """The parameters' range words (all sub-words), one column per segment."""
    i = ops.RANGES.index(opt.seg_amax_ptr)
    return ops.RANGES.buf[:, i:i + len(opt.groups)].clone()


def _five_steps(cuda, momentum, dampening, nesterov, clip, check):
    from rscotr_amd import ops
    from rscotr_amd.optim import FlatSGD
    g = torch.Generator().manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(cuda)) for s in SHAPES]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    groups = [dict(name=str(i), param=p, lr=lr, weight_decay=wd) for i, (p, lr, wd) in enumerate(zip(ps, LRS, WDS))]
    opt = FlatSGD(groups, momentum=momentum, dampening=dampening, nesterov=nesterov,
                  grad_clip=dict(max_norm=MAX_NORM, norm_type=2) if clip else None)
    topt = torch.optim.SGD([dict(params=[p], lr=lr, weight_decay=wd) for p, lr, wd in zip(ref, LRS, WDS)], lr=1.0,
                           momentum=momentum, dampening=dampening, nesterov=nesterov, foreach=False)
    try:
        opt.refresh_amax()  # (the words are computed lazily, by the first step at the latest: have them before it)
        for step in range(5):
            opt.zero_grad()
            live = [0, 2, 3, 4, 5, 6] if step == 0 else list(range(7))  # tensor 1 gets its first grad at step 1
            for i in live:
                gr = torch.randn(SHAPES[i], generator=g).to(cuda) * (10.0 if step % 2 else 0.01)
                ps[i].grad.add_(gr)
                opt.live[i] = True
                ref[i].grad = gr.clone()
            if step == 0:
                ps[1].grad.fill_(123.0)  # a tensor that is not live: its arena slice counts neither in the norm nor in the step
            rates = np.asarray(LRS) * (1.0 - 0.15 * step)  # the rates change between the steps, each group's its own
            opt.set_lrs(rates)
            for grp, lr in zip(topt.param_groups, rates):
                grp['lr'] = float(lr)
            before = (ps[1].detach().clone(), opt.flat_m.clone() if momentum else None, _words(ops, opt))
            if clip:
                norm = torch.nn.utils.clip_grad_norm_([p for p in ref if p.grad is not None], MAX_NORM, 2)
                assert (float(norm) > MAX_NORM) == bool(step % 2)
            topt.step()
            opt.step()
            if not check:
                continue
            assert opt._dyn_host[:, 0].tolist() == rates.astype(np.float32).tolist()
            if clip:
                assert torch.allclose(opt.grad_norm(), norm, rtol=1e-5)
            for a, b in zip(ps, ref):
                assert torch.allclose(a, b, rtol=1e-5, atol=1e-7), (step, float((a - b).abs().max()))
            if momentum:
                for i, b in enumerate(ref):
                    buf = topt.state[b].get('momentum_buffer')
                    o = opt.offsets[i]
                    if buf is not None:
                        assert torch.allclose(opt.flat_m[o:o + b.numel()].view(b.shape), buf, rtol=1e-5, atol=1e-6), (step, i)
            else:
                assert not hasattr(opt, 'flat_m')
            # range words: the kernel's equal what a recomputation from the arena gives, bit for bit; a tensor that is not
            # live keeps its word, its weights and its buffer
            after = _words(ops, opt)
            opt.refresh_amax()
            assert torch.equal(after, _words(ops, opt)), step
            if step == 0:
                assert torch.equal(after[:, 1], before[2][:, 1]) and torch.equal(ps[1].detach(), before[0])
                if momentum:
                    o = opt.offsets[1]
                    assert torch.equal(opt.flat_m[o:o + 4], before[1][o:o + 4])
            else:
                assert not torch.equal(ps[1].detach(), before[0])
        return opt.flat_p.clone(), (opt.flat_m.clone() if momentum else None)
    finally:
        opt.close()


@pytest.mark.parametrize('clip', [True, False])
@pytest.mark.parametrize('momentum,dampening,nesterov', [(0.9, 0, False), (0.9, 0, True), (0.9, 0.1, False), (0, 0, False)])
def test_fused_sgd_matches_torch(cuda, momentum, dampening, nesterov, clip):
    """(0.9, 0.1, False): with dampening, a tensor's first step must take buf = d — a zeroed buffer gives 0.9 d."""
    _five_steps(cuda, momentum, dampening, nesterov, clip, check=True)


def test_sgd_steps_are_bit_reproducible(cuda):
    a = _five_steps(cuda, 0.9, 0.1, False, True, check=False)
    b = _five_steps(cuda, 0.9, 0.1, False, True, check=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_entry_refuses_what_torch_refuses(cuda):
    from rscotr_amd._lib import lib
    t = torch.zeros(8, device=cuda)
    tabs = (torch.zeros(1, dtype=torch.int32, device=cuda), torch.zeros(1, dtype=torch.int64, device=cuda),
            torch.full((1,), 8, dtype=torch.int32, device=cuda), torch.zeros(8, device=cuda))

    def call(p=t, g=t, m=t, n=1, momentum=0.9, dampening=0.0, nesterov=0, max_norm=0.0):
        lib.call('rscotr_sgd_clip_step_r', p.data_ptr() if p is not None else 0, g.data_ptr(), m.data_ptr() if m is not None else 0,
                 tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), tabs[3].data_ptr(), n, 0, max_norm, momentum,
                 dampening, nesterov, 0, 0, 0, 0)
    for kw, word in ((dict(nesterov=1, momentum=0.0), 'Nesterov'), (dict(nesterov=1, dampening=0.1), 'Nesterov'),
                     (dict(momentum=-0.1), 'momentum'), (dict(n=-1), 'negative'), (dict(p=None), 'null'), (dict(m=None), 'null'),
                     (dict(max_norm=1.0), 'sumsq'), (dict(p=t[1:]), 'aligned')):
        with pytest.raises(RuntimeError, match=word):
            call(**kw)
    call(n=0)
    call(m=None, momentum=0.0)  # (the segment's `live` word is 0: nothing is stepped)
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


def _poly(b, t, T):
    return (b - POLY['min_lr']) * (1 - t / T) ** POLY['power'] + POLY['min_lr']


def test_cotraining_steps_with_sgd_poly_match_oracle(cuda):
    """6 iterations of the round-robin loop (zero_grad -> backward -> clip 0.1 -> SGD at the poly rate of the iteration) with
    torch-1.11 zero-fill semantics: per-step losses agree with the oracle loop to 1e-3.  The oracle side is torch.optim.SGD over
    the oracle's own groups, with the rates of this test's closed form."""
    from oracle import model as OM
    from oracle.optim import make_groups
    from rscotr_amd import synth
    from rscotr_amd.optim import FlatSGD, LrUpdater, build_optimizer
    cfg, mcfg = load_model_cfg(tiny=True)
    model = build_model(mcfg).to(cuda)
    P = state_to_oracle(model)
    opt = build_optimizer(model, SGD_OPTIM, dict(grad_clip=dict(max_norm=0.1, norm_type=2)))
    assert type(opt) is FlatSGD
    updater = LrUpdater(**POLY)
    ogroups = make_groups({k: v for k, v in P.items() if v.requires_grad}, SGD_OPTIM)
    oparams = [g['params'][0] for g in ogroups]
    oopt = torch.optim.SGD([{k: v for k, v in g.items() if k != 'name'} for g in ogroups], lr=SGD_OPTIM['lr'], momentum=0.9,
                           weight_decay=SGD_OPTIM['weight_decay'], foreach=False)
    try:
        for it in range(6):
            task = ('cls', 'det', 'seg')[it % 3]
            b_cpu = synth.make_batch(task, 2, 64, seed=it)
            b_dev = synth.make_batch(task, 2, 64, seed=it, device=cuda)
            rnd = synth.make_rnd(model, b_cpu, seed=it)
            rnd_dev = synth.make_rnd(model, b_cpu, seed=it, device=cuda)
            opt.set_lrs(updater.rates(opt.base_lr, it, 6))
            for g in oopt.param_groups:
                g['lr'] = _poly(SGD_OPTIM['lr'], it, 6)
            out = model.train_step(dict(b_dev, rnd=rnd_dev))
            opt.zero_grad()
            out['loss'].backward()
            opt.step()
            oout = OM.train_step(P, mcfg, b_cpu, rnd)
            for p in oparams:  # torch 1.11 zero_grad: zero-fill, keep None as None
                if p.grad is not None:
                    p.grad.detach_()
                    p.grad.zero_()
            oout['loss'].backward()
            torch.nn.utils.clip_grad_norm_([p for p in oparams if p.grad is not None], 0.1, 2)
            oopt.step()
            a, b = float(out['loss']), float(oout['loss'])
            print(f'sgd co-training step {it} ({task}): loss {a:.6f} vs oracle {b:.6f}')
            assert abs(a - b) <= 1e-3 * max(abs(b), 1e-3), (it, task, a, b)
        sd = model.state_dict()
        assert torch.equal(sd['backbone.norm0.weight'].cpu(), torch.ones_like(sd['backbone.norm0.weight'].cpu()))
    finally:
        opt.close()


def test_graphed_sgd_iterations_follow_the_schedule(cuda):
    """The scenario of test_graphed_iterations_match_eager (cls and seg alternating, DropPath 0, identity batch augment) with
    SGD + poly + a linear warm-up of 3 iterations: every iteration — eager, capturing or replayed — reads the rate of ITS
    iteration from the table it owns, and the graphed run walks the eager run's trajectory."""
    from rscotr_amd import synth
    from rscotr_amd.optim import LrUpdater, build_optimizer
    from rscotr_amd.runner import IterBasedRunner
    cfg, mcfg = load_model_cfg(tiny=True)
    mcfg = copy.deepcopy(mcfg)
    mcfg['backbone']['drop_path_rate'] = 0.0
    tasks = ['cls', 'seg', 'cls', 'seg', 'cls', 'seg']
    batches = [synth.make_batch(t, 2, 64, seed=40 + i, device=cuda) for i, t in enumerate(tasks)]
    lr_config = dict(POLY, warmup='linear', warmup_iters=3, warmup_ratio=0.1)

    def run(graph_tasks):
        model = build_model(mcfg).to(cuda)
        model.cls_augments.draw = lambda *a, **k: dict(kind='identity')
        w0 = {k: p.detach().clone() for k, p in model.named_parameters()}
        opt = build_optimizer(model, SGD_OPTIM, dict(grad_clip=dict(max_norm=0.1, norm_type=2)))
        r = IterBasedRunner(model, opt, [dict(b, img_metas=[dict(m) for m in b['img_metas']]) for b in batches],
                            lr_config=lr_config, graph_tasks=graph_tasks)
        r.max_iters = len(tasks)
        logs, col0 = [], []
        for it, task in enumerate(tasks):
            logs.append(r.train_iter()['log_vars'])
            assert r.iter == it + 1
            table = r.graphed[task].table if task in r.graphed else opt._dyn_host
            col0.append(table[:, 0].clone().numpy())
        if graph_tasks:
            assert sorted(r.graphed) == ['cls', 'seg']
        torch.cuda.synchronize()
        state = (opt.steps.copy(), opt.live.copy(), opt.base_lr.copy())
        opt.close()
        return model, w0, logs, col0, state

    m_e, w0, logs_e, col_e, st_e = run(())
    m_g, _, logs_g, col_g, st_g = run(('cls', 'seg'))
    updater = LrUpdater(**lr_config)
    for it in range(2, 6):  # (2, 3: the capturing iterations; 4, 5: replays)
        want = updater.rates(st_g[2], it, len(tasks)).astype(np.float32)
        assert np.array_equal(col_g[it], want) and np.array_equal(col_e[it], want), it
    assert np.array_equal(st_g[0], st_e[0]) and np.array_equal(st_g[1], st_e[1]) and st_g[1].any()
    for it in range(2, 6):
        a, b = logs_g[it], logs_e[it]
        assert list(a) == list(b)
        for k in a:
            if 'loss' not in k:
                continue
            tol = 2e-3 if k.startswith('cls') else 1e-2  # (the tolerances of test_graphed_iterations_match_eager)
            assert abs(a[k] - b[k]) <= tol * max(abs(b[k]), 1e-3), (it, k, a[k], b[k])
    we, wg = dict(m_e.named_parameters()), dict(m_g.named_parameters())
    num = torch.sqrt(sum(((wg[k] - we[k]).double() ** 2).sum() for k in we))
    den = torch.sqrt(sum(((we[k] - w0[k]).double() ** 2).sum() for k in we))
    r = float(num / den)
    print(f'graphed vs eager SGD run: r = |w_graph - w_eager| / |w_eager - w_0| = {r:.3e}')
    # r was measured once on an MI355X (profiles/README.md) and is gated at four times that value, capped at 0.08.  The cap is
    # a heuristic, not a measurement: one dropped update among six comparable ones leaves roughly 1/6, and the cap is half of that.
    assert r <= R_GATE, r

