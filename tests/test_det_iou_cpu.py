"""The det head's IoU loss family (IoULoss / DIoULoss / CIoULoss next to GIoULoss), IoUCost(iou_mode='iou') and
QualityFocalLoss on the CPU: the formulas of tests/det_iou_oracle.py against values worked out by hand, the config surface
(registry, DINOHead, refusals, the unchanged default), and the shape-static det route against the dynamic one on the tiny
model with the three new ops patched by the oracle (the HIP kernels themselves: tests/test_det_iou_gpu.py)."""
import copy
import math

import pytest
import torch

import det_iou_oracle as O
from util import build_model, load_model_cfg, patch_ops_with_oracle

D = torch.float64


def _b(*v):
    return torch.tensor(v, dtype=D)


# ------------------------------------------------------------------------------------------------------------------
# hand-checked oracle values
# ------------------------------------------------------------------------------------------------------------------
def test_oracle_values_of_the_unit_offset_pair():
    """p = (0,0,2,2), t = (1,1,3,3): ov 1, union 7, enclosing box 3 x 3 (area 9, diagonal^2 18), centres (1,1) and (2,2):
    rho2 = 2.  Equal aspect ratios: CIoU's v = 0.  The eps terms move the values by < 1e-6."""
    p, t = _b(0, 0, 2, 2), _b(1, 1, 3, 3)
    assert abs(float(O.iou(p, t)) - 1 / 7) < 1e-12
    assert abs(float(O.giou(p, t)) - (1 / 7 - 2 / 9)) < 1e-12
    assert abs(float(O.diou(p, t)) - (1 / 7 - 2 / 18)) < 1e-6
    assert abs(float(O.ciou(p, t)) - (1 / 7 - 1 / 9)) < 1e-6
    assert abs(float(O.iou_loss(p, t, mode='linear')) - 6 / 7) < 1e-12
    assert abs(float(O.iou_loss(p, t, mode='square')) - (1 - 1 / 49)) < 1e-12
    assert abs(float(O.iou_loss(p, t, mode='log')) - math.log(7)) < 1e-12
    assert abs(float(O.diou_loss(p, t)) - (1 - 1 / 7 + 1 / 9)) < 1e-6
    # disjoint boxes: iou 0; IoULoss floors it at eps
    q = _b(5, 5, 6, 6)
    assert float(O.iou(p, q)) == 0.0 and abs(float(O.iou_loss(p, q, eps=1e-6, mode='log')) + math.log(1e-6)) < 1e-12


def test_oracle_ciou_with_the_aspect_term_live():
    """p = (0,0,4,2), t = (0,0,4,3): ov 8, union 12, iou 2/3 > 0.5; enclosing 4 x 3: c2 = 25; centres (2,1), (2,1.5):
    rho2 = 1/4; v = 4/pi^2 (atan(4/3) - atan(2))^2, alpha = v / (1/3 + v)."""
    p, t = _b(0, 0, 4, 2).requires_grad_(True), _b(0, 0, 4, 3)
    v = 4 / math.pi ** 2 * (math.atan(4 / 3) - math.atan(2.0)) ** 2
    alpha = v / (1 - 2 / 3 + v)
    assert alpha * v > 4e-4          # (4.96e-4: 50 times the tolerance below — the term is seen)
    want = 2 / 3 - (0.25 / 25 + alpha * v)
    got = O.ciou(p, t)
    assert abs(float(got.detach()) - want) < 1e-5
    assert abs(float(O.diou(p.detach(), t)) - (2 / 3 - 0.01)) < 1e-6
    # alpha is a constant: d ciou / d y2 = d iou - d (rho2 / c2) - alpha dv, by hand at y2 = 2 (ov = 4 y2, union = 12, c2 fixed)
    got.backward()
    d_iou = 4 / 12
    d_rho = (-(2 * 1.5 - 2) / 2) / 25                                   # rho2 = (3 - y2)^2 / 4
    d_v = 8 / math.pi ** 2 * (math.atan(4 / 3) - math.atan(2.0)) * (4 / (4 ** 2 + 2 ** 2))   # d(-atan(4 / h1)) / dh1 = 4 / (16 + h1^2)
    assert abs(float(p.grad[3]) - (d_iou - d_rho - alpha * d_v)) < 1e-5
    # below iou = 0.5 the aspect term is switched off: CIoU = DIoU
    p2, t2 = _b(0, 0, 4, 1), _b(0, 0, 4, 3)
    assert abs(float(O.ciou(p2, t2)) - float(O.diou(p2, t2))) < 1e-12


def test_oracle_qfl_row_by_hand():
    """One foreground row (C = 3, label 1, logits (0, 1, -2)) whose boxes give iou 1/7, and one background row."""
    pred = torch.tensor([[[0.0, 1.0, -2.0], [0.5, -0.5, 0.0]]], dtype=D)
    tgt = torch.tensor([[1, 3]])
    bp = torch.tensor([[[0.1, 0.1, 0.2, 0.2], [0.5, 0.5, 0.1, 0.1]]], dtype=D)   # (0,0,.2,.2)
    bt = torch.tensor([[[0.2, 0.2, 0.2, 0.2], [0.0, 0.0, 0.0, 0.0]]], dtype=D)   # (.1,.1,.3,.3)
    sg = lambda x: 1 / (1 + math.exp(-x))
    sp = lambda x: math.log(1 + math.exp(x))                                        # BCE(x, 0)
    s = 1 / 7
    row0 = sp(0.0) * sg(0.0) ** 2 + (sp(1.0) - 1.0 * s) * (s - sg(1.0)) ** 2 + sp(-2.0) * sg(-2.0) ** 2
    row1 = sum(sp(x) * sg(x) ** 2 for x in (0.5, -0.5, 0.0))
    got = O.quality_focal_loss_sum(pred, tgt, bp, bt, 2.0)
    assert abs(float(got) - (row0 + row1)) < 1e-9
    w = torch.tensor([[0.5, 0.0]], dtype=D)
    assert abs(float(O.quality_focal_loss_sum(pred, tgt, bp, bt, 2.0, w)) - 0.5 * row0) < 1e-9
    # logits of +-30 stay finite, gradient included
    big = torch.tensor([[[30.0, -30.0, 30.0], [-30.0, 30.0, -30.0]]], dtype=torch.float32, requires_grad=True)
    out = O.quality_focal_loss_sum(big, tgt, bp.float(), bt.float(), 2.0)
    out.sum().backward()
    assert torch.isfinite(out).all() and torch.isfinite(big.grad).all()


def test_oracle_box_loss_zero_weight_rows_and_giou_equals_the_existing_formula():
    from rscotr_amd import ops
    g = torch.Generator().manual_seed(0)
    S, B, Q = 2, 2, 9
    c, wh = torch.rand(S, B, Q, 2, generator=g, dtype=D) * 0.6 + 0.2, torch.rand(S, B, Q, 2, generator=g, dtype=D) * 0.3 + 0.05
    pred = torch.cat([c, wh], -1)
    tgt = torch.cat([c + 0.02, wh * 1.3], -1)
    w = torch.zeros(S, B, Q, 4, dtype=D)
    w[:, :, ::3] = 1
    tgt = tgt * w                                                     # unmatched rows carry an all-zero target box
    fac = torch.tensor([[64., 48., 64., 48.], [32., 64., 32., 64.]], dtype=D)
    f = fac.view(1, B, 1, 4)
    for kind in ('giou', 'iou', 'diou', 'ciou'):
        pr = pred.clone().requires_grad_(True)
        l1, li = O.box_loss_sums_kind(pr, tgt, w, fac, kind)
        li.sum().backward()
        per = O.box_loss(kind, O.xyxy(pred) * f, O.xyxy(tgt) * f)
        assert torch.allclose(li, (per * w.mean(-1))[:, :, ::3].flatten(1).sum(1), rtol=1e-12)
        assert torch.isfinite(pr.grad).all() and float(pr.grad[:, :, 1::3].abs().max()) == 0.0
    want = ((1 - ops._giou(ops.bbox_cxcywh_to_xyxy(pred) * f, ops.bbox_cxcywh_to_xyxy(tgt) * f, aligned=True)) * w.mean(-1)).flatten(1).sum(1)
    assert torch.allclose(O.box_loss_sums_kind(pred, tgt, w, fac, 'giou')[1], want, rtol=1e-12)


def test_match_cost_formula_takes_iou_mode():
    """ops.match_cost (the dynamic route's torch formula) against the oracle in both modes; the default is 'giou'."""
    from rscotr_amd import ops
    g = torch.Generator().manual_seed(1)
    S, Q, C, G = 2, 11, 5, 4
    cls = torch.randn(S, Q, C, generator=g, dtype=D)
    box = torch.cat([torch.rand(S, Q, 2, generator=g, dtype=D) * 0.6 + 0.2, torch.rand(S, Q, 2, generator=g, dtype=D) * 0.3 + 0.05], -1)
    gt = O.xyxy(torch.cat([torch.rand(G, 2, generator=g, dtype=D) * 0.6 + 0.2, torch.rand(G, 2, generator=g, dtype=D) * 0.3 + 0.05], -1))
    fac = torch.tensor([80., 60., 80., 60.], dtype=D)
    gt = gt * fac
    lab = torch.randint(0, C, (G,), generator=g)
    args = (2.0, 5.0, 2.0, 0.25, 2.0, 1e-12)
    for mode in ('giou', 'iou'):
        want = O.match_cost_batched_kind(cls[:, None], box[:, None], gt[None], lab[None], fac[None], *args, iou_mode=mode)[:, 0]
        got = ops.match_cost(cls, box, gt, lab, 80., 60., *args, iou_mode=mode)
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12), mode
    assert torch.equal(ops.match_cost(cls, box, gt, lab, 80., 60., *args), ops.match_cost(cls, box, gt, lab, 80., 60., *args, iou_mode='giou'))
    with pytest.raises(ValueError, match='iou_mode'):
        ops.match_cost(cls, box, gt, lab, 80., 60., *args, iou_mode='diou')


def test_gpu_box_inputs_cover_the_cases():
    """What the comparison of tests/test_det_iou_gpu.py relies on, checked on the fp64 formulas: every case among the positive rows; disjoint /
    nested / thin pairs are what they are called; no coordinate shared; CIoU's switch at iou = 0.5 not within 1e-3."""
    from test_det_iou_gpu import BOX_CASES, _box_inputs
    pred, tgt, w, fac, _, _, case, pos = _box_inputs()
    f = fac.double().view(1, 2, 1, 4)
    p, t = O.xyxy(pred.double()) * f, O.xyxy(tgt.double()) * f
    iou = O.iou(p, t)
    frac = float(pos.float().mean())
    assert 0.07 < frac < 0.13
    for k, name in enumerate(BOX_CASES):
        assert int((pos & (case == k)).sum()) >= 3, name
    is_ = lambda name: pos & (case == BOX_CASES.index(name))
    assert float(iou[is_('disjoint')].max()) == 0.0
    n = is_('nested')
    assert bool(((t[n][:, :2] > p[n][:, :2]) & (t[n][:, 2:] < p[n][:, 2:])).all())
    assert float(iou[is_('near_identical')].min()) > 0.9
    th = is_('thin')
    assert float((pred[th][:, 2] / pred[th][:, 3]).min()) >= 10.0 and float(iou[th].min()) > 0
    assert float(iou[is_('ciou_above_half')].min()) > 0.501 and float(iou[is_('ciou_below_half')].max()) < 0.499
    assert float(iou[is_('ciou_below_half')].min()) > 0
    assert float((iou[pos] - 0.5).abs().min()) > 1e-3
    assert float((p[pos] - t[pos]).abs().min()) > 1e-4            # pixels: no (nearly) shared coordinate, no sub-gradient tie
    assert float((t[~pos].abs().sum(-1) == 0).float().mean()) > 0.4


# ------------------------------------------------------------------------------------------------------------------
# config surface
# ------------------------------------------------------------------------------------------------------------------
def _head_cfg(mcfg, loss_iou=None, loss_cls=None, iou_cost=None):
    m = copy.deepcopy(mcfg)
    if loss_iou is not None:
        m['bbox_head']['loss_iou'] = loss_iou
    if loss_cls is not None:
        m['bbox_head']['loss_cls'] = loss_cls
    if iou_cost is not None:
        m['train_cfg']['det']['assigner']['iou_cost'] = iou_cost
    return m


def _build_head(m):
    from rscotr_amd import MODELS
    return MODELS.build(dict(copy.deepcopy(m['bbox_head']), train_cfg=m['train_cfg']['det'], test_cfg=m['test_cfg']['det']))


def test_holders_build_through_the_registry_and_inside_the_head():
    from rscotr_amd import MODELS, det_head
    h = MODELS.build(dict(type='IoULoss'))
    assert isinstance(h, det_head.IoULoss) and (h.kind, h.mode, h.eps, h.loss_weight) == ('iou', 'log', 1e-6, 1.0)
    assert MODELS.build(dict(type='IoULoss', linear=True, mode='square')).mode == 'linear'
    assert MODELS.build(dict(type='IoULoss', mode='square', eps=1e-4, loss_weight=3.0)).mode == 'square'
    for name, kind in (('DIoULoss', 'diou'), ('CIoULoss', 'ciou'), ('GIoULoss', 'giou')):
        h = MODELS.build(dict(type=name, loss_weight=2.0))
        assert type(h).__name__ == name and (h.kind, h.eps, h.loss_weight) == (kind, 1e-6, 2.0)
    q = MODELS.build(dict(type='QualityFocalLoss'))
    assert isinstance(q, det_head.QualityFocalLoss) and (q.use_sigmoid, q.beta, q.loss_weight) == (True, 2.0, 1.0)
    a = MODELS.build(dict(type='HungarianAssigner', cls_cost=dict(type='FocalLossCost', weight=2.0),
                          reg_cost=dict(type='BBoxL1Cost', weight=5.0, box_format='xywh'),
                          iou_cost=dict(type='IoUCost', iou_mode='iou', weight=3.0)))
    assert (a.iou_mode, a.w_iou) == ('iou', 3.0)
    cfg, mcfg = load_model_cfg(tiny=True)
    for li in ('IoULoss', 'DIoULoss', 'CIoULoss'):
        head = _build_head(_head_cfg(mcfg, loss_iou=dict(type=li, loss_weight=2.0), iou_cost=dict(type='IoUCost', iou_mode='iou', weight=2.0)))
        assert type(head.loss_iou).__name__ == li and head.assigner.iou_mode == 'iou'
    head = _build_head(_head_cfg(mcfg, loss_cls=dict(type='QualityFocalLoss', use_sigmoid=True, beta=2.0, loss_weight=1.0)))
    assert isinstance(head.loss_cls, det_head.QualityFocalLoss) and head.cls_out_channels == head.num_classes


def test_refusals():
    from rscotr_amd import MODELS
    for name in ('IoULoss', 'DIoULoss', 'CIoULoss', 'QualityFocalLoss'):
        for red in ('sum', 'none'):
            with pytest.raises(NotImplementedError, match='reduction'):
                MODELS.build(dict(type=name, reduction=red))
    with pytest.raises(NotImplementedError, match='BoundedIoULoss'):
        MODELS.build(dict(type='BoundedIoULoss', beta=0.2))
    with pytest.raises(NotImplementedError, match='use_sigmoid'):
        MODELS.build(dict(type='QualityFocalLoss', use_sigmoid=False))
    with pytest.raises(NotImplementedError, match='activated'):
        MODELS.build(dict(type='QualityFocalLoss', activated=True))
    with pytest.raises(NotImplementedError, match='mode'):
        MODELS.build(dict(type='IoULoss', mode='cubic'))
    for mode in ('diou', 'ciou', 'iof'):
        with pytest.raises(AssertionError):
            MODELS.build(dict(type='HungarianAssigner', cls_cost=dict(type='FocalLossCost', weight=2.0),
                              reg_cost=dict(type='BBoxL1Cost', weight=5.0, box_format='xywh'),
                              iou_cost=dict(type='IoUCost', iou_mode=mode, weight=2.0)))


def test_default_config_builds_the_same_objects():
    from rscotr_amd import det_head
    cfg, mcfg = load_model_cfg(tiny=True)
    head = _build_head(mcfg)
    assert type(head.loss_cls) is det_head.FocalLoss and (head.loss_cls.gamma, head.loss_cls.alpha, head.loss_cls.loss_weight) == (2.0, 0.25, 1.0)
    assert type(head.loss_iou) is det_head.GIoULoss and (head.loss_iou.kind, head.loss_iou.eps, head.loss_iou.loss_weight) == ('giou', 1e-6, 2.0)
    assert type(head.loss_bbox) is det_head.L1Loss and head.loss_bbox.loss_weight == 5.0
    a = head.assigner
    assert (a.iou_mode, a.w_cls, a.w_l1, a.w_iou, a.alpha, a.gamma, a.eps) == ('giou', 2.0, 5.0, 2.0, 0.25, 2.0, 1e-12)


# ------------------------------------------------------------------------------------------------------------------
# static route against dynamic route
# ------------------------------------------------------------------------------------------------------------------
def _patch_new_ops(monkeypatch, calls):
    from rscotr_amd import ops

    def counted(name):
        fn = getattr(O, name)

        def wrapped(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **k)
        return wrapped

    for name in ('box_loss_sums_kind', 'match_cost_batched_kind', 'quality_focal_loss_sum'):
        monkeypatch.setattr(ops, name, counted(name))
        monkeypatch.setattr(ops.losses, name, getattr(ops, name))


RECIPES = {
    'diou_ioucost': dict(loss_iou=dict(type='DIoULoss', loss_weight=2.0), iou_cost=dict(type='IoUCost', iou_mode='iou', weight=2.0)),
    'ciou_qfl': dict(loss_iou=dict(type='CIoULoss', loss_weight=2.0),
                     loss_cls=dict(type='QualityFocalLoss', use_sigmoid=True, beta=2.0, loss_weight=1.0)),
    'iou_square_qfl_ioucost': dict(loss_iou=dict(type='IoULoss', mode='square', loss_weight=2.0),
                                   loss_cls=dict(type='QualityFocalLoss', use_sigmoid=True, beta=2.0, loss_weight=1.0),
                                   iou_cost=dict(type='IoUCost', iou_mode='iou', weight=2.0)),
}


@pytest.mark.parametrize('recipe', list(RECIPES))
def test_det_static_path_equals_dynamic_path_with_the_new_losses(monkeypatch, recipe):
    """tests/test_model_cpu.py::test_det_static_path_equals_dynamic_path under the new holders: the shape-static route
    (padded ground truth, masked extra denoising slots, device-shaped assignment) and the dynamic route give the same log_vars,
    assignments and gradients, at that test's tolerances — and the two routes reach the new ops, not the default recipe's."""
    patch_ops_with_oracle(monkeypatch)
    calls = {}
    _patch_new_ops(monkeypatch, calls)
    from rscotr_amd import ops, synth
    kw = RECIPES[recipe]
    default = {}
    for name in ('box_loss_sums', 'sigmoid_focal_loss_sum', 'match_cost_batched'):
        fn = getattr(ops, name)

        def counted(*a, _fn=fn, _n=name, **k):
            default[_n] = default.get(_n, 0) + 1
            return _fn(*a, **k)
        monkeypatch.setattr(ops, name, counted)
    cfg, mcfg = load_model_cfg(tiny=True)
    model = build_model(_head_cfg(mcfg, **kw))
    seed = 3
    batch = synth.make_batch('det', 2, 64, seed=seed)
    rnd = synth.make_rnd(model, batch, seed=seed)
    res = {}
    for mode in (True, False):
        model.bbox_head.static_path = mode
        try:
            model.zero_grad(set_to_none=True)
            rec = {}
            out = model.train_step(dict(batch, rnd=rnd, record=rec))
            out['loss'].backward()
            res[mode] = (out, rec, {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
        finally:
            model.bbox_head.static_path = True
    (o1, r1, g1), (o2, r2, g2) = res[True], res[False]
    assert list(o1['log_vars']) == list(o2['log_vars']) and len(o1['log_vars']) == 40
    for k, v in o1['log_vars'].items():
        assert v == v and abs(v - o2['log_vars'][k]) <= 1e-5 * max(abs(v), 1e-3), k
    assert r1['match'].keys() == r2['match'].keys() and len(r1['match']) > 0
    for k in r1['match']:
        assert (r1['match'][k][0] == r2['match'][k][0]).all() and (r1['match'][k][1] == r2['match'][k][1]).all()
    assert g1.keys() == g2.keys()
    for n in g1:
        assert float((g1[n] - g2[n]).abs().max()) <= 1e-5 * max(float(g2[n].abs().max()), 1e-6) + 1e-7, n
    # 2 launches (matching sets, denoising sets) per route for each loss, 1 cost launch on the static route
    assert calls.get('box_loss_sums_kind') == 4 and 'box_loss_sums' not in default
    assert calls.get('quality_focal_loss_sum', 0) == (4 if 'loss_cls' in kw else 0)
    assert default.get('sigmoid_focal_loss_sum', 0) == (0 if 'loss_cls' in kw else 4)
    assert calls.get('match_cost_batched_kind', 0) == (1 if 'iou_cost' in kw else 0)
    assert default.get('match_cost_batched', 0) == (0 if 'iou_cost' in kw else 1)


def test_default_recipe_keeps_its_three_launches(monkeypatch):
    """The default config calls ops.match_cost_batched / box_loss_sums / sigmoid_focal_loss_sum with their fixed positional
    signatures (the stand-ins of tests/util.py take no other) and none of the new ops."""
    patch_ops_with_oracle(monkeypatch)
    calls = {}
    _patch_new_ops(monkeypatch, calls)
    from rscotr_amd import synth
    cfg, mcfg = load_model_cfg(tiny=True)
    model = build_model(mcfg)
    batch = synth.make_batch('det', 2, 64, seed=3)
    out = model.train_step(dict(batch, rnd=synth.make_rnd(model, batch, seed=3), record={}))
    assert float(out['loss']) == float(out['loss']) and calls == {}
