"""DiceLoss in the seg head's `loss_decode` at the model layer, without a GPU: the oracle of the GPU tests
(tests/seg_dice_oracle.py) against a second formulation and two closed forms, the config surface, the routing of
`Mask2FormerHead.losses`, and what the contract refuses."""
import pytest
import torch
import torch.nn.functional as F

from seg_dice_oracle import dice_contract, dice_inputs, dice_reference
from test_seg_loss_weighted_cpu import _CW100, _FakeOps, _batch, _head, contract_loss

_CE_DICE = [dict(type='CrossEntropyLoss', loss_name='loss_ce', loss_weight=1.0),
            dict(type='DiceLoss', loss_name='loss_dice', loss_weight=3.0)]


def _binary_dice(pred, target, valid_mask, smooth, exponent):
    """mmseg binary_dice_loss with its @weighted_loss mean over the batch, as remembered."""
    B = pred.shape[0]
    pred, target, valid_mask = pred.reshape(B, -1), target.reshape(B, -1), valid_mask.reshape(B, -1)
    num = torch.sum(torch.mul(pred, target) * valid_mask, dim=1) * 2 + smooth
    den = torch.sum(pred.pow(exponent) + target.pow(exponent), dim=1) + smooth
    return (1 - num / den).mean()


def _mmseg_style(logit, label, ignore_index=255, smooth=1.0, class_weight=None, loss_weight=1.0):
    """DiceLoss.forward + dice_loss: a Python loop over the classes, each one a binary Dice."""
    pred = F.softmax(F.interpolate(logit.double(), size=label.shape[-2:], mode='bilinear', align_corners=False), dim=1)
    C = pred.shape[1]
    one_hot = F.one_hot(torch.clamp(label.long(), 0, C - 1), num_classes=C)
    valid_mask = (label != ignore_index).long()
    total = 0.0
    for i in range(C):
        if i != ignore_index:
            d = _binary_dice(pred[:, i], one_hot[..., i], valid_mask, smooth, 2)
            if class_weight is not None:
                d = d * float(class_weight[i])
            total = total + d
    return loss_weight * total / C


@pytest.mark.parametrize('B,C,h,w,H,W,ignore,smooth,use_cw', [
    (2, 7, 8, 8, 64, 64, 255, 1.0, False),
    (2, 7, 8, 8, 64, 64, 5, 1e-3, True),       # a skipped channel: the divisor stays 7
    (1, 3, 5, 4, 11, 9, -100, 1.0, True),
])
def test_oracle_agrees_with_the_per_class_loop(B, C, h, w, H, W, ignore, smooth, use_cw):
    logit, label, cw = dice_inputs(B, C, h, w, H, W, ignore)
    label[0, :2, :3] = C + 3  # non-ignored labels past the last channel are clamped
    cw = cw if use_cw else None
    a = dice_contract(logit, label, ignore, smooth, cw, 3.0)[0].detach()
    b = _mmseg_style(logit, label, ignore, smooth, cw, 3.0)
    assert 0 < float(a) and abs(float(a) - float(b)) <= 1e-12 * abs(float(b)), (float(a), float(b))


def test_oracle_closed_forms():
    # a perfect prediction with nothing ignored: p is the one-hot, num == den
    label = torch.randint(0, 5, (2, 16, 16), generator=torch.Generator().manual_seed(3))
    logit = 200.0 * F.one_hot(label, 5).permute(0, 3, 1, 2).float()
    loss, grad = dice_reference(logit, label)
    assert abs(loss) <= 1e-12
    # all-zero logits (1,4,2,2), all-zero label (1,8,8): p = 1/4; class 0: num = 2*16+1, den = 64/16+64+1; the others 1 / 5
    loss, _ = dice_reference(torch.zeros(1, 4, 2, 2), torch.zeros(1, 8, 8, dtype=torch.long))
    want = ((1 - 33 / 69) + 3 * (1 - 1 / 5)) / 4
    assert abs(want - 0.730434782) < 1e-8 and abs(loss - want) <= 1e-14


def test_oracle_gradient_is_the_documented_closed_form():
    """dL/du_c = p_c (g_c - S), g_c = a t v + bcoef p_c, S = sum_c g_c p_c: what the kernels evaluate, against autograd."""
    B, C, h, w, H, W = 2, 7, 8, 8, 64, 64
    logit, label, cw = dice_inputs(B, C, h, w, H, W)
    _, want = dice_reference(logit, label, 255, 1.0, cw, 3.0, scale=1.0)
    z = logit.double().requires_grad_(True)
    u = F.interpolate(z, size=(H, W), mode='bilinear', align_corners=False)
    p = F.softmax(u.detach(), dim=1)
    t = F.one_hot(label.clamp(0, C - 1), C).permute(0, 3, 1, 2).double()
    v = (label != 255).double().unsqueeze(1)
    num = 2 * (p * t * v).flatten(2).sum(-1) + 1.0
    den = (p * p + t).flatten(2).sum(-1) + 1.0
    k = 3.0 * cw.double() / (C * B)
    a, bcoef = (-2 * k / den)[:, :, None, None], (2 * k * num / den ** 2)[:, :, None, None]
    g = a * t * v + bcoef * p
    du = p * (g - (g * p).sum(1, keepdim=True))
    u.backward(du)
    assert float((z.grad - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_ce_and_dice_list_builds_a_head():
    plain, _ = _head()
    head, _ = _head(loss_decode=_CE_DICE)
    from rscotr_amd.seg_head import CrossEntropyLoss, DiceLoss
    ce, dice = list(head.loss_decode)
    assert isinstance(ce, CrossEntropyLoss) and isinstance(dice, DiceLoss)
    assert (dice.loss_name, dice.loss_weight, dice.smooth, dice.ignore_index, dice.class_weight) == ('loss_dice', 3.0, 1.0, 255, None)
    assert list(head.state_dict()) == list(plain.state_dict())  # no parameters, no buffers: the reference's keys
    # a list that holds only a Dice entry builds too; the single-dict form of loss_decode stays one CrossEntropyLoss
    only, _ = _head(loss_decode=[dict(type='DiceLoss', smooth=1e-3, class_weight=_CW100, ignore_index=7, reduction='none')])
    assert isinstance(only.loss_decode[0], DiceLoss) and only.loss_decode[0].class_weight == _CW100
    assert list(only.state_dict()) == list(plain.state_dict())
    with pytest.raises(NotImplementedError, match='DiceLoss.*list'):
        _head(loss_decode=dict(type='DiceLoss'))


def test_dice_refusals():
    from rscotr_amd import MODELS
    with pytest.raises(NotImplementedError, match='exponent'):
        MODELS.build(dict(type='DiceLoss', exponent=3))
    with pytest.raises(NotImplementedError, match='exponent'):
        _head(loss_decode=[_CE_DICE[0], dict(type='DiceLoss', exponent=3)])
    with pytest.raises(NotImplementedError, match='LovaszLoss'):
        _head(loss_decode=[_CE_DICE[0], _CE_DICE[1], dict(type='LovaszLoss')])
    with pytest.raises((TypeError, ValueError)):
        MODELS.build(dict(type='DiceLoss', class_weight=3.0))
    with pytest.raises(ValueError):
        MODELS.build(dict(type='DiceLoss', reduction='batchmean'))
    for reduction in ('mean', 'sum', 'none'):
        assert MODELS.build(dict(type='DiceLoss', reduction=reduction)).reduction == reduction
    # a class_weight of the wrong length raises at first use, before any device is touched
    head, _ = _head(loss_decode=[_CE_DICE[0], dict(type='DiceLoss', class_weight=[1.0] * 6)])
    logit, label = _batch()
    with pytest.raises(ValueError, match=r'6\b.*\b100\b'):
        head.loss_decode[1](logit, label.squeeze(1))


def test_ce_only_head_builds_the_same_objects():
    from rscotr_amd.seg_head import CrossEntropyLoss
    head, _ = _head()
    assert type(head.loss_decode) is CrossEntropyLoss and head.loss_decode.is_default and head.sampler is None
    head, _ = _head(loss_decode=[dict(type='CrossEntropyLoss', loss_name='loss_ce', loss_weight=1.0),
                                 dict(type='CrossEntropyLoss', loss_name='loss_wce', class_weight=_CW100, loss_weight=0.5)])
    assert [type(m) for m in head.loss_decode] == [CrossEntropyLoss] * 2
    assert [m.is_default for m in head.loss_decode] == [True, False]
    assert head.loss_decode[1].class_weight == _CW100
    assert torch.equal(head.loss_decode[1].weight_on(torch.device('cpu'), 100), torch.tensor(_CW100))


class _FakeDiceOps(_FakeOps):
    def upsample_dice(self, seg_logit, label, ignore_index=255, smooth=1.0, class_weight=None, loss_weight=1.0):
        self.calls.append(('upsample_dice', dict(ignore_index=ignore_index, smooth=smooth, class_weight=class_weight,
                                                 loss_weight=loss_weight, grad=torch.is_grad_enabled())))
        return dice_contract(seg_logit, label, ignore_index, smooth, class_weight, loss_weight)[0].float()

    def upsample_ce(self, seg_logit, label, ignore_index=255):
        out = super().upsample_ce(seg_logit, label, ignore_index)
        self.calls[-1][1]['grad'] = torch.is_grad_enabled()
        return out


def _dice_head(monkeypatch, **over):
    from rscotr_amd import seg_head
    head, _ = _head(**over)
    fake = _FakeDiceOps()
    for name in ('upsample_ce', 'upsample_ce_weighted', 'upsample_dice'):
        monkeypatch.setattr(seg_head.ops, name, getattr(fake, name))
    return head, fake


def test_losses_dispatch_per_entry(monkeypatch):
    logit, label = _batch()
    lab = label.squeeze(1)
    plain, fake0 = _dice_head(monkeypatch)
    out0 = plain.losses(logit, label)
    assert [c[0] for c in fake0.calls] == ['upsample_ce']      # the CE-only head: the path it took before
    head, fake = _dice_head(monkeypatch, loss_decode=_CE_DICE,
                            sampler=dict(type='OHEMPixelSampler', thresh=0.01, min_kept=100))
    out = head.losses(logit, label)
    assert [c[0] for c in fake.calls] == ['upsample_ce_weighted', 'upsample_dice']
    assert tuple(fake.calls[0][1]['ohem']) == (0.01, 100)
    # the sampler does not reach the Dice entry; its own ignore_index and smooth, loss_weight folded into the op
    kw = fake.calls[1][1]
    assert kw['ignore_index'] == 255 and kw['loss_weight'] == 3.0 and kw['smooth'] == 1.0 and kw['class_weight'] is None
    assert list(out) == ['loss_ce', 'loss_dice', 'acc_seg']
    assert sum('loss' in k for k in out) == 2                   # MTL._parse_losses sums every key that contains 'loss'
    ref = float(dice_contract(logit, lab, 255, 1.0, None, 3.0)[0].detach())
    assert abs(float(out['loss_dice'].detach()) - ref) <= 1e-6 * ref
    # without the sampler the CE entry is the default one: the plain op, and the same numbers as the CE-only head
    head, fake = _dice_head(monkeypatch, loss_decode=_CE_DICE)
    out = head.losses(logit, label)
    assert [c[0] for c in fake.calls] == ['upsample_ce', 'upsample_dice']
    assert torch.equal(out['loss_ce'], out0['loss_ce']) and torch.equal(out['acc_seg'], out0['acc_seg'])


def test_losses_same_name_adds_up_and_dice_alone_reports_accuracy(monkeypatch):
    logit, label = _batch()
    lab = label.squeeze(1)
    head, fake = _dice_head(monkeypatch, loss_decode=[
        dict(type='DiceLoss', loss_name='loss_dice', loss_weight=1.0),
        dict(type='DiceLoss', loss_name='loss_dice', loss_weight=0.5, smooth=1e-3, class_weight=_CW100, ignore_index=7)])
    out = head.losses(logit, label)
    assert [c[0] for c in fake.calls] == ['upsample_dice', 'upsample_dice', 'upsample_ce']
    assert fake.calls[2][1]['grad'] is False and fake.calls[0][1]['grad'] is True   # the accuracy pass carries no graph
    assert torch.equal(fake.calls[1][1]['class_weight'], torch.tensor(_CW100)) and fake.calls[1][1]['ignore_index'] == 7
    assert list(out) == ['loss_dice', 'acc_seg'] and not out['acc_seg'].requires_grad
    a = float(dice_contract(logit, lab)[0].detach())
    b = float(dice_contract(logit, lab, 7, 1e-3, torch.tensor(_CW100), 0.5)[0].detach())
    assert abs(float(out['loss_dice']) - (a + b)) <= 1e-6 * (a + b)
    plain, _ = _dice_head(monkeypatch)
    assert torch.equal(out['acc_seg'], plain.losses(logit, label)['acc_seg'])
    # a CE and a Dice entry of one name add up as well
    head, fake = _dice_head(monkeypatch, loss_decode=[dict(type='CrossEntropyLoss', loss_name='loss_seg'),
                                                      dict(type='DiceLoss', loss_name='loss_seg')])
    out = head.losses(logit, label)
    c = float(contract_loss(logit, lab, 255)['loss'])
    assert list(out) == ['loss_seg', 'acc_seg'] and abs(float(out['loss_seg']) - (a + c)) <= 1e-6 * (a + c)


def test_op_refuses_cpu_tensors():
    """No fallback to torch: the op is the HIP kernels or an error."""
    from rscotr_amd import ops
    logit, label, _ = dice_inputs(1, 3, 4, 4, 8, 8)
    with pytest.raises(RuntimeError):
        ops.upsample_dice(logit, label)
