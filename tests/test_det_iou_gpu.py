"""The kind-parameterised det loss kernels (box loss: GIoU / IoU / DIoU / CIoU; match cost: giou / iou; QualityFocalLoss) against
the fp64 formulas of tests/det_iou_oracle.py, and the det iteration under the new holders: static against dynamic route, and
hipGraph replay against eager.

Tolerances: no new constants.  Per case the oracle is also evaluated in fp32 on the CPU and its relative error against fp64
measured; the kernel's gate is max(project gate, 4 x that error) — the project gates are those of tests/test_det_loss_gpu.py
(1e-5 on sums, 1e-4 on gradients and on the match cost), the factor 4 covers another summation order and other atan / log
implementations.  Every comparison prints the measured error and its gate."""
import copy
import functools

import pytest
import torch

import det_iou_oracle as O
from util import build_model, load_model_cfg

pytestmark = pytest.mark.gpu

SUM_GATE, GRAD_GATE, COST_GATE = 1e-5, 1e-4, 1e-4


def _rel(a, ref):
    ref = ref.detach().double().cpu()
    return float((a.detach().double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-30))


def _check(what, got, ref64, ref32, project):
    e32 = _rel(ref32, ref64)
    gate = max(project, 4 * e32)
    err = _rel(got, ref64)
    print(f'{what}: kernel {err:.3e}, fp32 oracle {e32:.3e}, gate {gate:.3e}')
    assert err <= gate, (what, err, gate)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------
# box loss
# ------------------------------------------------------------------------------------------------------------------
BOX_CASES = ('random', 'disjoint', 'nested', 'partial', 'near_identical', 'thin', 'ciou_above_half', 'ciou_below_half')
KINDS = (('giou', 'log'), ('iou', 'log'), ('iou', 'linear'), ('iou', 'square'), ('diou', 'log'), ('ciou', 'log'))


@functools.lru_cache(maxsize=None)
def _box_inputs():
    """S=3, B=2, Q=150 (B*Q = 300: past the 256-thread stride, no multiple of 64); the pair of row q is of case q % 8."""
    g = torch.Generator().manual_seed(5)
    S, B, Q = 3, 2, 150
    r = lambda *s: torch.rand(S, B, Q, *s, generator=g)
    c, wh = r(2) * 0.5 + 0.25, r(2) * 0.2 + 0.05
    case = (torch.arange(Q) % len(BOX_CASES)).view(1, 1, Q, 1).expand(S, B, Q, 1)
    thin = case == BOX_CASES.index('thin')
    wh = torch.where(thin, torch.cat([r(1) * 0.1 + 0.25, r(1) * 0.005 + 0.015], -1), wh)      # aspect 10 .. 23
    pred = torch.cat([c, wh], -1)
    tc, twh = r(2) * 0.5 + 0.25, r(2) * 0.2 + 0.05                                              # random
    jit = r(2) * 0.5 + 0.5                                                                     # in [0.5, 1]
    pick = lambda name, new, old: torch.where(case == BOX_CASES.index(name), new, old)
    tc, twh = pick('disjoint', c + (wh + 0.05) * 1.1, tc), pick('disjoint', wh * 0.9, twh)
    tc, twh = pick('nested', c + 0.02 * wh * jit, tc), pick('nested', wh * 0.5, twh)
    tc, twh = pick('partial', c + 0.3 * wh * jit, tc), pick('partial', wh * 1.1, twh)
    tc, twh = pick('near_identical', c + 1e-3, tc), pick('near_identical', wh * 1.001, twh)
    tc, twh = pick('thin', c + wh * torch.tensor([0.05, 0.2]) * jit, tc), pick('thin', wh * torch.tensor([0.93, 1.2]), twh)
    tc, twh = pick('ciou_above_half', c + 0.01 * wh * jit, tc), pick('ciou_above_half', wh * torch.tensor([0.8, 1.15]), twh)
    tc, twh = pick('ciou_below_half', c + 0.01 * wh * jit, tc), pick('ciou_below_half', wh * torch.tensor([0.5, 0.7]), twh)
    tgt = torch.cat([tc, twh], -1)
    pos = torch.rand(S, B, Q, 1, generator=g) < 0.1
    w = pos.float().expand(-1, -1, -1, 4).contiguous()
    # unmatched queries carry an all-zero target box (every other zero-weight row keeps its boxes: they must not matter)
    unmatched = ~pos & (torch.arange(Q).view(1, 1, Q, 1) % 2 == 0)
    tgt = torch.where(unmatched, torch.zeros_like(tgt), tgt)
    fac = torch.tensor([[512., 512., 512., 512.], [400., 300., 400., 300.]])
    u1, u2 = torch.randn(S, generator=g), torch.randn(S, generator=g)
    return pred, tgt, w, fac, u1, u2, case[..., 0], pos[..., 0]   # (what they hold is checked in tests/test_det_iou_cpu.py)


@functools.lru_cache(maxsize=None)
def _box_reference(kind, mode):
    """(fp64, fp32) oracle results: l1 sums, iou-loss sums, gradient of sum(l1 u1 + loss u2) wrt pred"""
    pred, tgt, w, fac, u1, u2, _, _ = _box_inputs()
    out = []
    for dt in (torch.float64, torch.float32):
        pr = pred.clone().to(dt).requires_grad_(True)
        l1, li = O.box_loss_sums_kind(pr, tgt.to(dt), w.to(dt), fac.to(dt), kind, 1e-6, mode)
        ((l1 * u1.to(dt)).sum() + (li * u2.to(dt)).sum()).backward()
        out.append((l1.detach(), li.detach(), pr.grad))
    return out


def _run_box(cuda, kind, mode):
    from rscotr_amd import ops
    pred, tgt, w, fac, u1, u2, _, _ = _box_inputs()
    pd = pred.to(cuda).requires_grad_(True)
    l1, li = ops.box_loss_sums_kind(pd, tgt.to(cuda), w.to(cuda), fac.to(cuda), kind, 1e-6, mode)
    ((l1 * u1.to(cuda)).sum() + (li * u2.to(cuda)).sum()).backward()
    return l1.detach(), li.detach(), pd.grad


@pytest.mark.parametrize('kind,mode', KINDS)
def test_box_loss_kind_sums_and_gradient(cuda, kind, mode):
    (l1_64, li_64, g_64), (l1_32, li_32, g_32) = _box_reference(kind, mode)
    l1, li, grad = _run_box(cuda, kind, mode)
    assert torch.isfinite(li).all() and torch.isfinite(grad).all()
    _check(f'{kind}/{mode} l1 sums', l1, l1_64, l1_32, SUM_GATE)
    _check(f'{kind}/{mode} loss sums', li, li_64, li_32, SUM_GATE)
    _check(f'{kind}/{mode} gradient', grad, g_64, g_32, GRAD_GATE)
    # a zero-weight row: a zero gradient whatever its boxes hold
    pos = _box_inputs()[7]
    assert float(grad.cpu()[~pos].abs().max()) == 0.0
    # run to run: the same bits
    l1b, lib_, gradb = _run_box(cuda, kind, mode)
    assert torch.equal(_bits(l1), _bits(l1b)) and torch.equal(_bits(li), _bits(lib_)) and torch.equal(_bits(grad), _bits(gradb))


def test_box_loss_kind_giou_is_the_existing_launch(cuda):
    from rscotr_amd import ops
    pred, tgt, w, fac, u1, u2, _, _ = _box_inputs()
    l1, li, grad = _run_box(cuda, 'giou', 'log')
    pd = pred.to(cuda).requires_grad_(True)
    l1o, gio = ops.box_loss_sums(pd, tgt.to(cuda), w.to(cuda), fac.to(cuda), 1e-6)
    ((l1o * u1.to(cuda)).sum() + (gio * u2.to(cuda)).sum()).backward()
    assert torch.equal(_bits(l1), _bits(l1o)) and torch.equal(_bits(li), _bits(gio)) and torch.equal(_bits(grad), _bits(pd.grad))


def test_box_loss_kind_refuses_unknown_options(cuda):
    from rscotr_amd import ops
    pred, tgt, w, fac = (x.to(cuda) for x in _box_inputs()[:4])
    with pytest.raises(ValueError, match='kind'):
        ops.box_loss_sums_kind(pred, tgt, w, fac, 'bounded')
    with pytest.raises(ValueError, match='mode'):
        ops.box_loss_sums_kind(pred, tgt, w, fac, 'iou', 1e-6, 'cubic')


# ------------------------------------------------------------------------------------------------------------------
# match cost
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cost_inputs():
    g = torch.Generator().manual_seed(6)
    S, B, Q, C, G = 2, 2, 70, 7, 5
    cls = torch.randn(S, B, Q, C, generator=g) * 2
    box = torch.cat([torch.rand(S, B, Q, 2, generator=g) * 0.8 + 0.1, torch.rand(S, B, Q, 2, generator=g) * 0.3 + 0.02], -1)
    fac = torch.tensor([[512., 512., 512., 512.], [400., 300., 400., 300.]])
    gtb = torch.cat([torch.rand(B, G, 2, generator=g) * 0.8 + 0.1, torch.rand(B, G, 2, generator=g) * 0.3 + 0.02], -1)
    gtb[:, 0] = box[0, :, 3] + 1e-3                                   # one ground truth nearly on top of a prediction
    gt = O.xyxy(gtb) * fac[:, None]
    lab = torch.randint(0, C, (B, G), generator=g)
    return cls, box, gt, lab, fac


COST_ARGS = (2.0, 5.0, 2.0, 0.25, 2.0, 1e-12)


@pytest.mark.parametrize('iou_mode', ['giou', 'iou'])
def test_match_cost_kind(cuda, iou_mode):
    from rscotr_amd import ops
    cls, box, gt, lab, fac = _cost_inputs()
    ref64 = O.match_cost_batched_kind(cls.double(), box.double(), gt.double(), lab, fac.double(), *COST_ARGS, iou_mode=iou_mode)
    ref32 = O.match_cost_batched_kind(cls, box, gt, lab, fac, *COST_ARGS, iou_mode=iou_mode)
    dev = [x.to(cuda) for x in (cls, box, gt, lab, fac)]
    out = ops.match_cost_batched_kind(*dev, *COST_ARGS, iou_mode)
    assert tuple(out.shape) == (2, 2, 70, 5)
    _check(f'match cost {iou_mode}', out, ref64, ref32, COST_GATE)
    # the IoU term on its own (the class and L1 terms are several times larger): cost(w_iou) - cost(0) against the formula
    zero = ops.match_cost_batched_kind(*dev, 2.0, 5.0, 0.0, 0.25, 2.0, 1e-12, iou_mode)
    z64 = O.match_cost_batched_kind(cls.double(), box.double(), gt.double(), lab, fac.double(), 2.0, 5.0, 0.0, 0.25, 2.0, 1e-12,
                                    iou_mode=iou_mode)
    z32 = O.match_cost_batched_kind(cls, box, gt, lab, fac, 2.0, 5.0, 0.0, 0.25, 2.0, 1e-12, iou_mode=iou_mode)
    scale = float(ref64.abs().max() / (ref64 - z64).abs().max())      # the difference inherits the absolute error of the costs
    _check(f'match cost {iou_mode}, IoU term', out - zero, ref64 - z64, ref32 - z32, COST_GATE * scale)
    if iou_mode == 'giou':
        assert torch.equal(_bits(out), _bits(ops.match_cost_batched(*dev, *COST_ARGS)))
    else:
        assert not torch.equal(out, ops.match_cost_batched(*dev, *COST_ARGS))
    with pytest.raises(ValueError, match='iou_mode'):
        ops.match_cost_batched_kind(*dev, *COST_ARGS, 'ciou')


# ------------------------------------------------------------------------------------------------------------------
# QualityFocalLoss
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _qfl_inputs():
    """S=3, N=300, C=7 (N*C = 2100 > 1024: the strided loop runs); a third of the rows foreground, their box pairs disjoint
    (s = 0), nearly identical (s ~ 1) or overlapping."""
    g = torch.Generator().manual_seed(7)
    S, N, C = 3, 300, 7
    pred = torch.randn(S, N, C, generator=g) * 3
    tgt = torch.randint(0, C, (S, N), generator=g)
    tgt[:, torch.arange(N) % 3 != 0] = C
    bp = torch.cat([torch.rand(S, N, 2, generator=g) * 0.5 + 0.25, torch.rand(S, N, 2, generator=g) * 0.2 + 0.05], -1)
    bt = bp.clone()
    kind = (torch.arange(N) // 3) % 3
    bt[:, kind == 0, :2] += bp[:, kind == 0, 2:] * 1.5                                    # disjoint
    bt[:, kind == 1] += 1e-4                                                              # s ~ 1
    bt[:, kind == 2] = bt[:, kind == 2] * (torch.rand(S, int((kind == 2).sum()), 4, generator=g) * 0.4 + 0.8)
    bt = bt * (tgt != C).unsqueeze(-1)                                                    # background rows: all-zero target box
    w = (torch.rand(S, N, generator=g) < 0.8).float() * (torch.rand(S, N, generator=g) + 0.5)
    up = torch.randn(S, generator=g)
    return pred, tgt, bp, bt, w, up


def _qfl_reference(pred, tgt, bp, bt, w, up):
    out = []
    for dt in (torch.float64, torch.float32):
        pr = pred.clone().to(dt).requires_grad_(True)
        s = O.quality_focal_loss_sum(pr, tgt, bp.to(dt), bt.to(dt), 2.0, None if w is None else w.to(dt))
        (s * up.to(dt)).sum().backward()
        out.append((s.detach(), pr.grad))
    return out


def _run_qfl(cuda, pred, tgt, bp, bt, w, up):
    from rscotr_amd import ops
    pd = pred.to(cuda).requires_grad_(True)
    bpd = bp.to(cuda).requires_grad_(True)
    s = ops.quality_focal_loss_sum(pd, tgt.to(cuda), bpd, bt.to(cuda), 2.0, None if w is None else w.to(cuda))
    (s * up.to(cuda)).sum().backward()
    assert bpd.grad is None                                                               # the score is a constant
    return s.detach(), pd.grad


@pytest.mark.parametrize('with_weight', [False, True])
def test_qfl_sum_and_gradient(cuda, with_weight):
    pred, tgt, bp, bt, w, up = _qfl_inputs()
    w = w if with_weight else None
    fg = tgt != 7
    s = O.iou(O.xyxy(bp.double()), O.xyxy(bt.double()))[fg]
    assert int((s == 0).sum()) > 50 and int((s > 0.99).sum()) > 50 and int(((s > 0.1) & (s < 0.9)).sum()) > 50
    (s64, g64), (s32, g32) = _qfl_reference(pred, tgt, bp, bt, w, up)
    got, grad = _run_qfl(cuda, pred, tgt, bp, bt, w, up)
    _check(f'qfl sums (weight {with_weight})', got, s64, s32, SUM_GATE)
    _check(f'qfl gradient (weight {with_weight})', grad, g64, g32, GRAD_GATE)
    got2, grad2 = _run_qfl(cuda, pred, tgt, bp, bt, w, up)
    assert torch.equal(_bits(got), _bits(got2)) and torch.equal(_bits(grad), _bits(grad2))


def test_qfl_saturated_logits_stay_finite(cuda):
    pred, tgt, bp, bt, w, up = _qfl_inputs()
    big = torch.where(torch.arange(pred.shape[-1]) % 2 == 0, torch.tensor(30.0), torch.tensor(-30.0)).expand_as(pred).clone()
    big[:, ::2] = -big[:, ::2]
    (s64, g64), (s32, g32) = _qfl_reference(big, tgt, bp, bt, w, up)
    got, grad = _run_qfl(cuda, big, tgt, bp, bt, w, up)
    assert torch.isfinite(got).all() and torch.isfinite(grad).all()
    _check('qfl sums at logits of +-30', got, s64, s32, SUM_GATE)
    _check('qfl gradient at logits of +-30', grad, g64, g32, GRAD_GATE)


# ------------------------------------------------------------------------------------------------------------------
# the det iteration under the new holders
# ------------------------------------------------------------------------------------------------------------------
RECIPES = {
    'diou_ioucost': dict(loss_iou=dict(type='DIoULoss', loss_weight=2.0), iou_cost=dict(type='IoUCost', iou_mode='iou', weight=2.0)),
    'ciou_qfl': dict(loss_iou=dict(type='CIoULoss', loss_weight=2.0),
                     loss_cls=dict(type='QualityFocalLoss', use_sigmoid=True, beta=2.0, loss_weight=1.0)),
}


def _tiny_cfg(recipe):
    cfg, mcfg = load_model_cfg(tiny=True)
    m = copy.deepcopy(mcfg)
    kw = RECIPES[recipe]
    m['bbox_head']['loss_iou'] = kw['loss_iou']
    if 'loss_cls' in kw:
        m['bbox_head']['loss_cls'] = kw['loss_cls']
    if 'iou_cost' in kw:
        m['train_cfg']['det']['assigner']['iou_cost'] = kw['iou_cost']
    return cfg, m


@pytest.mark.parametrize('recipe', list(RECIPES))
def test_det_static_path_equals_dynamic_path_with_the_new_losses(cuda, recipe):
    """tests/test_model_gpu.py::test_det_static_path_equals_dynamic_path_full_size on the tiny model (64 x 64, B = 2): the
    static route (kernel cost, device assignment) against the dynamic one (torch cost formula, host solver): same assignment
    indices, same losses."""
    from rscotr_amd import synth
    cfg, mcfg = _tiny_cfg(recipe)
    model = build_model(mcfg, seed=2).to(cuda)
    batch = synth.make_batch('det', 2, 64, seed=21, device=cuda)
    rnd = synth.make_rnd(model, synth.make_batch('det', 2, 64, seed=21), seed=21, device=cuda)
    res = {}
    for mode in (True, False):
        model.bbox_head.static_path = mode
        try:
            model.zero_grad(set_to_none=True)
            rec = {}
            out = model.train_step(dict(batch, rnd=rnd, record=rec))
            out['loss'].backward()
            torch.cuda.synchronize()
            res[mode] = (out, rec)
        finally:
            model.bbox_head.static_path = True
    (o1, r1), (o2, r2) = res[True], res[False]
    assert list(o1['log_vars']) == list(o2['log_vars']) and len(o1['log_vars']) == 40
    assert r1['match'].keys() == r2['match'].keys() and len(r1['match']) == 14
    for k in r1['match']:
        assert (r1['match'][k][0] == r2['match'][k][0]).all() and (r1['match'][k][1] == r2['match'][k][1]).all(), k
    for k, v in o1['log_vars'].items():
        assert v == v and abs(v - o2['log_vars'][k]) <= 1e-4 * max(abs(v), 1e-3), (k, v, o2['log_vars'][k])
    for n, p in model.named_parameters():
        assert p.grad is None or torch.isfinite(p.grad).all(), n


@pytest.mark.parametrize('recipe', list(RECIPES))
def test_graph_replay_equals_eager_with_the_new_losses(cuda, recipe):
    """tests/test_padded_gpu.py::test_padded_graph_replay_equals_eager on the tiny model: a det-only runner captures the
    iteration with the new losses and replays it; its losses in the round of the capture equal the eager runner's (the
    denoising draws differ between the two: every key but the `dn_` ones)."""
    import numpy as np
    from rscotr_amd import MODELS
    from rscotr_amd.data import build_synthetic_multidataloader
    from rscotr_amd.runner import build_runner
    cfg, mcfg = _tiny_cfg(recipe)
    logs = []
    for graphs in (True, False):
        torch.manual_seed(0)
        np.random.seed(2022)
        model = MODELS.build(copy.deepcopy(mcfg))
        model.init_weights()
        model.to(cuda).train()
        model.backbone.drop_path_rates = [0.0 for _ in model.backbone.drop_path_rates]
        loader = build_synthetic_multidataloader(cfg, cuda, size=64, batch_size=2, tasks=('det',), max_gt=6, pool=1)
        runner = build_runner(model, cfg, loader, graph_tasks=('det',) if graphs else ())
        last = None
        for i in range(3):
            out = runner.train_iter()
            if i == 1:
                last = dict(out['log_vars'])
            else:
                assert all(v == v and abs(v) < 1e6 for v in dict(out['log_vars']).values()), i
        torch.cuda.synchronize()
        assert set(runner.graphed) == ({'det'} if graphs else set())
        for n, p in model.named_parameters():
            assert torch.isfinite(p).all(), n
        logs.append(last)
        runner.optimizer.close()
    lg, le = logs
    assert list(lg) == list(le) and len(lg) > 0
    for k, v in lg.items():
        assert v == v and abs(v) < 1e6, (k, v)
        if 'dn_' in k or k.endswith('.loss') or 'loss' not in k:
            continue
        assert abs(v - le[k]) <= 5e-3 * max(abs(le[k]), 1e-2), (k, v, le[k])
