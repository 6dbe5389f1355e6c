"""FocalLoss and TverskyLoss in the seg head's `loss_decode` at the model layer, without a GPU: the oracle of the GPU tests
(tests/seg_focal_tversky_oracle.py) against plain Python loops and closed forms, the config surface, the routing of
`Mask2FormerHead.losses`, and what the contracts refuse."""
import math

import pytest
import torch
import torch.nn.functional as F

from seg_focal_tversky_oracle import (dice_inputs, focal_contract, focal_reference, tversky_contract, tversky_reference)
from test_seg_loss_weighted_cpu import _CW100, _FakeOps, _batch, _head, contract_loss

_CE = dict(type='CrossEntropyLoss', loss_name='loss_ce', loss_weight=1.0)
_FOCAL = dict(type='FocalLoss', loss_name='loss_focal', loss_weight=2.0)
_TVERSKY = dict(type='TverskyLoss', loss_name='loss_tversky', loss_weight=3.0)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def _bilinear_loops(z, H, W):
    """upsample_bilinear2d (align_corners=False) of one image (C,h,w) as nested lists of floats, pixel by pixel."""
    C, h, w = z.shape
    out = [[[0.0] * W for _ in range(H)] for _ in range(C)]

    def src(d, n_in, n_out):
        s = max((d + 0.5) * n_in / n_out - 0.5, 0.0)
        i0 = min(int(s), n_in - 1)
        return i0, min(i0 + 1, n_in - 1), s - i0

    for y in range(H):
        y0, y1, ly = src(y, h, H)
        for x in range(W):
            x0, x1, lx = src(x, w, W)
            for c in range(C):
                out[c][y][x] = ((1 - ly) * ((1 - lx) * float(z[c, y0, x0]) + lx * float(z[c, y0, x1])) +
                                ly * ((1 - lx) * float(z[c, y1, x0]) + lx * float(z[c, y1, x1])))
    return out


_LOOP_SHAPE = (1, 3, 2, 2, 5, 4)


def _loop_inputs():
    B, C, h, w, H, W = _LOOP_SHAPE
    g = torch.Generator().manual_seed(11)
    logit = (torch.randn(B, C, h, w, generator=g) * 3).double()
    label = torch.randint(0, C, (B, H, W), generator=g)
    label[0, 0, 0] = 255      # ignored
    label[0, 1, 2] = C + 2    # past the last channel, not ignored
    label[0, 4, 3] = -4       # below 0, not ignored
    return logit, label


@pytest.mark.parametrize('gamma,alpha,cw,reduction,ignore', [
    (2.0, 0.5, None, 'mean', 255), (1.5, [0.2, 0.5, 0.9], [0.5, 2.0, 1.25], 'sum', 255), (0.0, 0.25, None, 'mean', 1)])
def test_focal_oracle_agrees_with_loops_over_every_pixel_and_class(gamma, alpha, cw, reduction, ignore):
    B, C, h, w, H, W = _LOOP_SHAPE
    logit, label = _loop_inputs()
    u = _bilinear_loops(logit[0], H, W)
    total = 0.0
    for y in range(H):
        for x in range(W):
            lab = int(label[0, y, x])
            if lab == ignore:
                continue
            for c in range(C):
                t = 1.0 if lab == c else 0.0
                v = u[c][y][x]
                s = 1.0 / (1.0 + math.exp(-v))
                q = (1 - s) * t + s * (1 - t)
                bce = max(v, 0.0) - v * t + math.log1p(math.exp(-abs(v)))
                a = alpha[c] if isinstance(alpha, list) else alpha
                total += bce * (a * t + (1 - a) * (1 - t)) * q ** gamma * (cw[c] if cw else 1.0)
    want = 3.0 * (total / (B * H * W * C) if reduction == 'mean' else total)
    got = float(focal_contract(logit, label, ignore, gamma, alpha, cw, reduction, 3.0)[0].detach())
    assert want > 0 and abs(got - want) <= 1e-12 * want, (got, want)


@pytest.mark.parametrize('alpha,beta,smooth,cw,ignore', [
    (0.3, 0.7, 1.0, None, 255), (0.9, 0.1, 1e-3, [0.5, 2.0, 1.25], 255), (0.5, 0.5, 1.0, [0.5, 2.0, 1.25], 1)])
def test_tversky_oracle_agrees_with_loops_over_every_pixel_and_class(alpha, beta, smooth, cw, ignore):
    B, C, h, w, H, W = _LOOP_SHAPE
    logit, label = _loop_inputs()
    u = _bilinear_loops(logit[0], H, W)
    tp, fp, fn = [0.0] * C, [0.0] * C, [0.0] * C
    for y in range(H):
        for x in range(W):
            lab = int(label[0, y, x])
            if lab == ignore:
                continue
            lc = min(max(lab, 0), C - 1)
            m = max(u[c][y][x] for c in range(C))
            ex = [math.exp(u[c][y][x] - m) for c in range(C)]
            for c in range(C):
                p, t = ex[c] / sum(ex), 1.0 if lc == c else 0.0
                tp[c] += p * t
                fp[c] += p * (1 - t)
                fn[c] += (1 - p) * t
    total = 0.0
    for c in range(C):
        if c != ignore:
            total += (cw[c] if cw else 1.0) * (1 - (tp[c] + smooth) / (tp[c] + alpha * fp[c] + beta * fn[c] + smooth))
    want = 3.0 * total / C
    got = float(tversky_contract(logit, label, ignore, alpha, beta, smooth, cw, 3.0)[0].detach())
    assert want > 0 and abs(got - want) <= 1e-12 * want, (got, want)


def test_oracle_closed_forms():
    # all-zero logits (1,4,2,2), all-zero label (1,8,8).  Focal: BCE = ln 2, alpha weight 1/2, q = 1/2, gamma 2.
    z, y = torch.zeros(1, 4, 2, 2), torch.zeros(1, 8, 8, dtype=torch.long)
    loss, _ = focal_reference(z, y)
    assert abs(loss - 0.125 * math.log(2)) <= 1e-14
    # Tversky: p = 1/4; class 0: TP = 16, FP = 0, FN = 48; the others: TP = 0, FP = 16, FN = 0
    loss, _ = tversky_reference(z, y)
    assert abs(loss - ((1 - 17 / 50.6) + 3 * (1 - 1 / 5.8)) / 4) <= 1e-14
    # every pixel ignored: both losses 0 with a zero gradient
    logit, label, cw = dice_inputs(2, 7, 8, 8, 16, 16)
    label = torch.full_like(label, 255)
    for ref in (focal_reference, tversky_reference):
        loss, grad = ref(logit, label, class_weight=cw)
        assert loss == 0.0 and not bool(grad.any())


def test_tversky_at_one_half_is_the_soft_dice_ratio():
    """alpha = beta = 1/2, smooth 1, nothing ignored: 1 - (2 TP + 2) / (sum p + sum t + 2) per (image, class)."""
    B, C, h, w, H, W = 2, 7, 8, 8, 64, 64
    logit, label, cw = dice_inputs(B, C, h, w, H, W, ignored=0.0)
    assert not bool((label == 255).any())
    got = float(tversky_contract(logit, label, 255, 0.5, 0.5, 1.0, cw, 3.0)[0].detach())
    p = F.softmax(F.interpolate(logit.double(), size=(H, W), mode='bilinear', align_corners=False), dim=1)
    t = F.one_hot(label, C).permute(0, 3, 1, 2).double()
    ratio = (2 * (p * t).flatten(2).sum(-1) + 2) / (p.flatten(2).sum(-1) + t.flatten(2).sum(-1) + 2)
    want = float(3.0 * ((1 - ratio).mean(0) * cw.double()).sum() / C)
    assert abs(got - want) <= 1e-12 * want


def test_gradients_are_the_documented_closed_forms():
    """What the kernels evaluate, against autograd.  Focal, x = -u for the positive class and u otherwise:
    d e / d x = k q^gamma (q + gamma softplus(x) (1 - q)).  Tversky: dL/du_c = p_c (g_c - S), g_c = v (a t + b), S = sum_c g_c p_c."""
    B, C, h, w, H, W = 2, 7, 8, 8, 64, 64
    logit, label, cw = dice_inputs(B, C, h, w, H, W)
    alpha = [0.1 * (c + 1) for c in range(C)]
    _, want = focal_reference(logit, label, 1.0, gamma=1.5, alpha=alpha, class_weight=cw, reduction='sum', loss_weight=3.0)
    z = logit.double().requires_grad_(True)
    u = F.interpolate(z, size=(H, W), mode='bilinear', align_corners=False)
    ud = u.detach()
    t = F.one_hot(label.clamp(0, C - 1), C).permute(0, 3, 1, 2).double() * ((label >= 0) & (label < C)).unsqueeze(1)
    v = (label != 255).double().unsqueeze(1)
    a = torch.tensor(alpha, dtype=torch.float64).view(1, C, 1, 1)
    x = torch.where(t > 0, -ud, ud)
    q = torch.sigmoid(x)
    k = 3.0 * cw.double().view(1, C, 1, 1) * (a * t + (1 - a) * (1 - t)) * v
    dx = k * q.pow(1.5) * (q + 1.5 * F.softplus(x) * (1 - q))
    u.backward(torch.where(t > 0, -dx, dx))
    assert float((z.grad - want).abs().max()) <= 1e-12 * float(want.abs().max())

    al, be, smooth = 0.3, 0.7, 1.0
    _, want = tversky_reference(logit, label, 1.0, alpha=al, beta=be, smooth=smooth, class_weight=cw, loss_weight=3.0)
    z = logit.double().requires_grad_(True)
    u = F.interpolate(z, size=(H, W), mode='bilinear', align_corners=False)
    p = F.softmax(u.detach(), dim=1)
    t = F.one_hot(label.clamp(0, C - 1), C).permute(0, 3, 1, 2).double()
    tp = (p * t * v).flatten(2).sum(-1)
    sp, st = (p * v).flatten(2).sum(-1), (t * v).flatten(2).sum(-1)
    num, den = tp + smooth, tp + al * (sp - tp) + be * (st - tp) + smooth
    k = 3.0 * cw.double() / (C * B)
    ca = (k * (num * (1 - al - be) / den ** 2 - 1 / den))[:, :, None, None]
    cb = (k * al * num / den ** 2)[:, :, None, None]
    g = v * (ca * t + cb)
    u.backward(p * (g - (g * p).sum(1, keepdim=True)))
    assert float((z.grad - want).abs().max()) <= 1e-12 * float(want.abs().max())


# ---- the head ------------------------------------------------------------------------------------------------------------------
def test_list_forms_build_a_head():
    from rscotr_amd import MODELS, det_head, seg_head
    plain, _ = _head()
    head, _ = _head(loss_decode=[_CE, _FOCAL, _TVERSKY])
    ce, focal, tversky = list(head.loss_decode)
    assert isinstance(ce, seg_head.CrossEntropyLoss)
    assert type(focal) is seg_head.FocalLoss and type(tversky) is seg_head.TverskyLoss
    assert (focal.loss_name, focal.loss_weight, focal.gamma, focal.alpha, focal.reduction, focal.class_weight) == \
        ('loss_focal', 2.0, 2.0, 0.5, 'mean', None)
    assert (tversky.loss_name, tversky.loss_weight, tversky.smooth, tversky.alpha, tversky.beta, tversky.ignore_index,
            tversky.class_weight) == ('loss_tversky', 3.0, 1.0, 0.3, 0.7, 255, None)
    assert list(head.state_dict()) == list(plain.state_dict())  # no parameters, no buffers: the reference's keys
    # either type alone in a list, with its options
    only, _ = _head(loss_decode=[dict(type='FocalLoss', use_sigmoid=True, gamma=1.5, alpha=[0.01 * i for i in range(100)],
                                      reduction='sum', class_weight=_CW100)])
    f = only.loss_decode[0]
    assert type(f) is seg_head.FocalLoss and f.gamma == 1.5 and len(f.alpha) == 100 and f.reduction == 'sum' and f.class_weight == _CW100
    assert torch.equal(f.alpha_on(torch.device('cpu'), 100), torch.tensor([0.01 * i for i in range(100)]))
    assert list(only.state_dict()) == list(plain.state_dict())
    only, _ = _head(loss_decode=[dict(type='TverskyLoss', smooth=1e-3, class_weight=_CW100, ignore_index=7, alpha=0.9, beta=0.1)])
    t = only.loss_decode[0]
    assert type(t) is seg_head.TverskyLoss and (t.smooth, t.alpha, t.beta, t.ignore_index) == (1e-3, 0.9, 0.1, 7)
    assert list(only.state_dict()) == list(plain.state_dict())
    # the det head's FocalLoss keeps the name in MODELS; TverskyLoss is registered
    det = MODELS.build(dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0))
    assert type(det) is det_head.FocalLoss and type(det) is not seg_head.FocalLoss
    assert type(MODELS.build(dict(type='TverskyLoss'))) is seg_head.TverskyLoss


def test_refusals():
    from rscotr_amd import MODELS
    from rscotr_amd.seg_head import FocalLoss
    for name in ('FocalLoss', 'TverskyLoss'):
        with pytest.raises(NotImplementedError, match=name + '.*list'):
            _head(loss_decode=dict(type=name))
    with pytest.raises(NotImplementedError, match='DiceLoss.*list'):
        _head(loss_decode=dict(type='DiceLoss'))
    with pytest.raises(NotImplementedError, match='LovaszLoss'):
        _head(loss_decode=[_CE, _FOCAL, _TVERSKY, dict(type='LovaszLoss')])
    with pytest.raises(NotImplementedError, match='reduction'):
        _head(loss_decode=[_CE, dict(type='FocalLoss', reduction='none')])
    with pytest.raises(NotImplementedError, match='use_sigmoid'):
        _head(loss_decode=[_CE, dict(type='FocalLoss', use_sigmoid=False)])
    sampler = dict(type='OHEMPixelSampler', thresh=0.7, min_kept=100)
    with pytest.raises(NotImplementedError, match='sampler.*FocalLoss'):
        _head(loss_decode=[_CE, _FOCAL], sampler=sampler)
    assert _head(loss_decode=[_CE, _TVERSKY], sampler=sampler)[0].sampler is not None
    with pytest.raises(ValueError, match='gamma'):
        FocalLoss(gamma=-1.0)
    with pytest.raises((TypeError, ValueError)):
        FocalLoss(class_weight=3.0)
    with pytest.raises(ValueError, match='alpha'):
        MODELS.build(dict(type='TverskyLoss', alpha=0.3, beta=0.6))
    with pytest.raises(ValueError, match='alpha'):
        _head(loss_decode=[_CE, dict(type='TverskyLoss', alpha=0.5, beta=0.7)])
    for smooth in (0, -1.0):
        with pytest.raises(ValueError, match='smooth'):
            MODELS.build(dict(type='TverskyLoss', smooth=smooth))
    # class_weight / alpha lists of the wrong length raise at first use, before any device is touched
    head, _ = _head(loss_decode=[_CE, dict(type='FocalLoss', class_weight=[1.0] * 6), dict(type='FocalLoss', alpha=[0.5] * 6),
                                 dict(type='TverskyLoss', class_weight=[1.0] * 6)])
    logit, label = _batch()
    for ld in list(head.loss_decode)[1:]:
        with pytest.raises(ValueError, match=r'6\b.*\b100\b'):
            ld(logit, label.squeeze(1))


def test_op_argument_refusals():
    from rscotr_amd import ops
    logit, label, _ = dice_inputs(1, 3, 4, 4, 8, 8)
    with pytest.raises(NotImplementedError, match='reduction'):
        ops.upsample_focal(logit, label, reduction='none')
    with pytest.raises(ValueError, match='gamma'):
        ops.upsample_focal(logit, label, gamma=-0.5)
    with pytest.raises(ValueError, match='alpha'):
        ops.upsample_tversky(logit, label, alpha=0.3, beta=0.3)
    with pytest.raises(ValueError, match='smooth'):
        ops.upsample_tversky(logit, label, smooth=0.0)


def test_ops_refuse_cpu_tensors():
    """No fallback to torch: the ops are the HIP kernels or an error."""
    from rscotr_amd import ops
    logit, label, _ = dice_inputs(1, 3, 4, 4, 8, 8)
    with pytest.raises(RuntimeError):
        ops.upsample_focal(logit, label)
    with pytest.raises(RuntimeError):
        ops.upsample_tversky(logit, label)


class _FakeFamilyOps(_FakeOps):
    def upsample_focal(self, seg_logit, label, ignore_index=255, gamma=2.0, alpha=0.5, class_weight=None, reduction='mean',
                       loss_weight=1.0):
        kw = dict(ignore_index=ignore_index, gamma=gamma, alpha=alpha, class_weight=class_weight, reduction=reduction,
                  loss_weight=loss_weight)
        self.calls.append(('upsample_focal', dict(kw, grad=torch.is_grad_enabled())))
        return focal_contract(seg_logit, label, **kw)[0].float()

    def upsample_tversky(self, seg_logit, label, ignore_index=255, alpha=0.3, beta=0.7, smooth=1.0, class_weight=None,
                         loss_weight=1.0):
        kw = dict(ignore_index=ignore_index, alpha=alpha, beta=beta, smooth=smooth, class_weight=class_weight, loss_weight=loss_weight)
        self.calls.append(('upsample_tversky', dict(kw, grad=torch.is_grad_enabled())))
        return tversky_contract(seg_logit, label, **kw)[0].float()

    def upsample_ce(self, seg_logit, label, ignore_index=255):
        out = super().upsample_ce(seg_logit, label, ignore_index)
        self.calls[-1][1]['grad'] = torch.is_grad_enabled()
        return out


def _family_head(monkeypatch, **over):
    from rscotr_amd import seg_head
    head, _ = _head(**over)
    fake = _FakeFamilyOps()
    for name in ('upsample_ce', 'upsample_ce_weighted', 'upsample_focal', 'upsample_tversky'):
        monkeypatch.setattr(seg_head.ops, name, getattr(fake, name))
    return head, fake


def test_losses_dispatch_per_entry(monkeypatch):
    logit, label = _batch()
    lab = label.squeeze(1)
    plain, fake0 = _family_head(monkeypatch)
    out0 = plain.losses(logit, label)
    assert [c[0] for c in fake0.calls] == ['upsample_ce']      # the CE-only head: the path it took before
    head, fake = _family_head(monkeypatch, loss_decode=[
        _CE, dict(_FOCAL, gamma=1.5, alpha=0.25, class_weight=_CW100, reduction='sum'), dict(_TVERSKY, ignore_index=9, smooth=0.5)])
    out = head.losses(logit, label)
    assert [c[0] for c in fake.calls] == ['upsample_ce', 'upsample_focal', 'upsample_tversky']
    kf, kt = fake.calls[1][1], fake.calls[2][1]
    # the focal entry takes the HEAD's ignore_index, the Tversky entry its own; loss_weight is folded into the ops
    assert (kf['ignore_index'], kf['gamma'], kf['alpha'], kf['reduction'], kf['loss_weight']) == (255, 1.5, 0.25, 'sum', 2.0)
    assert torch.equal(kf['class_weight'], torch.tensor(_CW100))
    assert (kt['ignore_index'], kt['alpha'], kt['beta'], kt['smooth'], kt['loss_weight'], kt['class_weight']) == \
        (9, 0.3, 0.7, 0.5, 3.0, None)
    assert list(out) == ['loss_ce', 'loss_focal', 'loss_tversky', 'acc_seg']
    assert sum('loss' in k for k in out) == 3                   # MTL._parse_losses sums every key that contains 'loss'
    ref = float(focal_contract(logit, lab, 255, 1.5, 0.25, _CW100, 'sum', 2.0)[0].detach())
    assert abs(float(out['loss_focal'].detach()) - ref) <= 1e-6 * ref
    ref = float(tversky_contract(logit, lab, 9, 0.3, 0.7, 0.5, None, 3.0)[0].detach())
    assert abs(float(out['loss_tversky'].detach()) - ref) <= 1e-6 * ref
    # the CE entry of the list is the default one: the plain op, and the same numbers as the CE-only head
    head, fake = _family_head(monkeypatch, loss_decode=[_CE, _FOCAL, _TVERSKY])
    out = head.losses(logit, label)
    assert torch.equal(out['loss_ce'], out0['loss_ce']) and torch.equal(out['acc_seg'], out0['acc_seg'])
    # an OHEM sampler reaches the CE entry and not the Tversky one
    head, fake = _family_head(monkeypatch, loss_decode=[_CE, _TVERSKY], sampler=dict(type='OHEMPixelSampler', thresh=0.01, min_kept=100))
    ohem = head.losses(logit, label)
    assert [c[0] for c in fake.calls] == ['upsample_ce_weighted', 'upsample_tversky']
    assert torch.equal(ohem['loss_tversky'], out['loss_tversky'])


def test_losses_same_name_adds_up_and_no_ce_entry_reports_accuracy(monkeypatch):
    logit, label = _batch()
    lab = label.squeeze(1)
    head, fake = _family_head(monkeypatch, loss_decode=[dict(type='FocalLoss', loss_name='loss_aux', alpha=[0.005 * i for i in range(100)]),
                                                        dict(type='TverskyLoss', loss_name='loss_aux')])
    out = head.losses(logit, label)
    assert [c[0] for c in fake.calls] == ['upsample_focal', 'upsample_tversky', 'upsample_ce']
    assert fake.calls[2][1]['grad'] is False and fake.calls[0][1]['grad'] is True   # the accuracy pass carries no graph
    assert torch.equal(fake.calls[0][1]['alpha'], torch.tensor([0.005 * i for i in range(100)]))
    assert list(out) == ['loss_aux', 'acc_seg'] and not out['acc_seg'].requires_grad
    a = float(focal_contract(logit, lab, alpha=[0.005 * i for i in range(100)])[0].detach())
    b = float(tversky_contract(logit, lab)[0].detach())
    assert abs(float(out['loss_aux'].detach()) - (a + b)) <= 1e-6 * (a + b)
    plain, _ = _family_head(monkeypatch)
    assert torch.equal(out['acc_seg'], plain.losses(logit, label)['acc_seg'])
    # a CE and a focal entry of one name add up as well
    head, fake = _family_head(monkeypatch, loss_decode=[dict(type='CrossEntropyLoss', loss_name='loss_seg'),
                                                        dict(type='FocalLoss', loss_name='loss_seg')])
    out = head.losses(logit, label)
    c = float(contract_loss(logit, lab, 255)['loss'])
    f = float(focal_contract(logit, lab)[0].detach())
    assert list(out) == ['loss_seg', 'acc_seg'] and abs(float(out['loss_seg'].detach()) - (f + c)) <= 1e-6 * (f + c)
