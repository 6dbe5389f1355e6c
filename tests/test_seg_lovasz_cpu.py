"""LovaszLoss in the seg head's `loss_decode` at the model layer, without a GPU: the oracle of the GPU tests
(tests/seg_lovasz_oracle.py) against hand-computed closed forms and the closed-form gradient the kernels evaluate, the config
surface, the routing of `Mask2FormerHead.losses`, and what the contract refuses."""
import pytest
import torch
import torch.nn.functional as F

from seg_lovasz_oracle import lovasz_contract, lovasz_grad, lovasz_inputs, lovasz_reference
from test_seg_loss_weighted_cpu import _CW100, _FakeOps, _batch, _head

_CE = dict(type='CrossEntropyLoss', loss_name='loss_ce', loss_weight=1.0)
_LOVASZ = dict(type='LovaszLoss', reduction='none', loss_weight=3.0)
_LOVASZ_IMG = dict(type='LovaszLoss', per_image=True, classes=[0, 1, 2, 3, 4, 5], loss_weight=0.5)


def _logits_of(p0):
    """Two-channel logits (1,2,1,n) whose softmax is (p0, 1 - p0), at identity resize."""
    p0 = torch.tensor(p0, dtype=torch.float64)
    return torch.stack([p0.log(), (1 - p0).log()]).reshape(1, 2, 1, -1)


def test_oracle_two_classes_four_pixels_by_hand():
    """p_0 = (.8, .6, .3, .1), labels (0, 1, 0, 1).  Both classes have the errors (.2, .6, .7, .1), sorted (.7, .6, .2, .1).
    class 0: fg along the order (1, 0, 1, 0), G = 2: (I, U) = (1,2) (1,3) (0,3) (0,4), J = 1/2, 2/3, 1, 1, g = 1/2, 1/6, 1/3, 0
    class 1: fg along the order (0, 1, 0, 1), G = 2: (I, U) = (2,3) (1,3) (1,4) (0,4), J = 1/3, 2/3, 3/4, 1, g = 1/3, 1/3, 1/12, 1/4"""
    logit = _logits_of([0.8, 0.6, 0.3, 0.1])
    label = torch.tensor([[[0, 1, 0, 1]]])
    l0 = 0.7 / 2 + 0.6 / 6 + 0.2 / 3
    l1 = 0.7 / 3 + 0.6 / 3 + 0.2 / 12 + 0.1 / 4
    for classes, want in (('present', (l0 + l1) / 2), ('all', (l0 + l1) / 2), ([0], l0), ([1], l1)):
        loss = float(lovasz_contract(logit, label, classes=classes)[0].detach())
        assert abs(loss - want) <= 1e-14, (classes, loss, want)
    cw = torch.tensor([2.0, 0.5])
    loss = float(lovasz_contract(logit, label, class_weight=cw, loss_weight=3.0)[0].detach())
    assert abs(loss - 3.0 * (2.0 * l0 + 0.5 * l1) / 2) <= 1e-14
    # the gradient w.r.t. p_c is -+ g at the element's rank: through the softmax, dL/du_0 = p_0 p_1 (D_0 - D_1) at each pixel
    _, grad = lovasz_reference(logit, label, scale=1.0)
    p0 = torch.tensor([0.8, 0.6, 0.3, 0.1], dtype=torch.float64)
    d0 = torch.tensor([-1 / 3, 1 / 6, -1 / 2, 0.0], dtype=torch.float64) / 2      # pixels 0..3 rank 2, 1, 0, 3 in class 0
    d1 = torch.tensor([1 / 12, -1 / 3, 1 / 3, -1 / 4], dtype=torch.float64) / 2
    want = p0 * (1 - p0) * (d0 - d1)
    assert float((grad[0, 0, 0] - want).abs().max()) <= 1e-14 and float((grad[0, 1, 0] + want).abs().max()) <= 1e-14
    # an ignored pixel leaves the segment: pixel 1 out -> class 1 has G = 1
    label2 = torch.tensor([[[0, 255, 0, 1]]])
    l0 = 0.7 / 2 + 0.2 / 2                       # sorted (.7 fg, .2 fg, .1 bg): g = 1/2, 1/2, 0
    l1 = 0.7 / 2 + 0.2 / 6 + 0.1 / 3             # sorted (.7 bg, .2 bg, .1 fg), G = 1: J = 1/2, 2/3, 1
    loss = float(lovasz_contract(logit, label2)[0].detach())
    assert abs(loss - (l0 + l1) / 2) <= 1e-14


def test_oracle_perfect_prediction_absent_class_and_labels_out_of_range():
    label = torch.randint(0, 5, (2, 16, 16), generator=torch.Generator().manual_seed(3))
    logit = 200.0 * F.one_hot(label, 5).permute(0, 3, 1, 2).float()
    for per_image, reduction in ((False, 'none'), (True, 'mean')):
        loss, grad = lovasz_reference(logit, label, per_image=per_image, reduction=reduction)
        assert abs(loss) <= 1e-12
    # an absent class under 'all' / a list costs the largest p_c; under 'present' it is not summed
    logit, label, _ = lovasz_inputs(1, 4, 5, 4, 11, 9)
    label[label == 2] = 1
    p = F.softmax(F.interpolate(logit.double(), size=(11, 9), mode='bilinear', align_corners=False), dim=1)
    pmax = float(p[0, 2][label[0] != 255].max())
    assert abs(float(lovasz_contract(logit, label, classes=[2])[0].detach()) - pmax) <= 1e-14
    present = float(lovasz_contract(logit, label, classes='present')[0].detach())
    listed = float(lovasz_contract(logit, label, classes=[0, 1, 3])[0].detach())
    everything = float(lovasz_contract(logit, label, classes='all')[0].detach())
    assert abs(present - listed) <= 1e-14 and abs(everything - (3 * present + pmax) / 4) <= 1e-14
    # a non-ignored label outside [0, C) is background for every class: the same loss as any other label no summed class has
    a, b = label.clone(), label.clone()
    a[0, :3, :4], b[0, :3, :4] = 9, 3
    assert abs(float(lovasz_contract(logit, a, classes=[0, 1])[0].detach())
               - float(lovasz_contract(logit, b, classes=[0, 1])[0].detach())) <= 1e-14
    # no valid pixel: 0 with a zero gradient; per image, such an image gives 0 and still counts in the mean
    loss, grad = lovasz_reference(logit, torch.full_like(label, 255), classes='all')
    assert loss == 0.0 and not bool(grad.any())
    logit2, label2, _ = lovasz_inputs(2, 4, 5, 4, 11, 9)
    label2[0] = 255
    one = float(lovasz_contract(logit2[1:], label2[1:])[0].detach())
    assert abs(float(lovasz_contract(logit2, label2, per_image=True, reduction='mean')[0].detach()) - one / 2) <= 1e-14
    assert abs(float(lovasz_contract(logit2, label2, per_image=True, reduction='sum')[0].detach()) - one) <= 1e-14


def test_oracle_loss_is_invariant_under_the_order_of_tied_errors():
    """Logits constant over blocks tie whole groups of errors bit for bit: the loss is the same whichever way the pixels (and so
    the ties) are ordered; the gradient of a tied group only moves inside the group."""
    g = torch.Generator().manual_seed(11)
    logit = (torch.randn(1, 3, 1, 4, generator=g) * 2).repeat_interleave(6, 3)        # 4 blocks of 6 tied pixels
    label = torch.randint(0, 3, (1, 1, 24), generator=g)
    loss, grad = lovasz_reference(logit, label, classes='all')
    perm = torch.randperm(24, generator=g)
    loss_p, grad_p = lovasz_reference(logit[..., perm], label[..., perm], classes='all')
    assert loss > 0 and abs(loss - loss_p) <= 1e-13 * loss
    blocks, blocks_p = grad.reshape(3, 4, 6).sum(-1), torch.zeros(3, 4, dtype=torch.float64)
    blocks_p.index_add_(1, perm // 6, grad_p.reshape(3, 24))
    assert float((blocks - blocks_p).abs().max()) <= 1e-13 * float(blocks.abs().max())


@pytest.mark.parametrize('per_image', [False, True])
def test_oracle_gradient_is_the_documented_closed_form(per_image):
    """What the kernels evaluate, against the oracle's autograd: g_k from the integer counts (1 / U_k at a foreground element,
    I_k / (U_k (U_k - 1)) at a background one), D = -+ g_rank * class_weight / #summed, dL/du_c = p_c (D_c - sum_k p_k D_k)."""
    B, C, h, w, H, W = 2, 5, 5, 5, 37, 37
    logit, label, cw = lovasz_inputs(B, C, h, w, H, W)
    label[0][label[0] == 3] = 2       # class 3 absent from image 0 (summed per image under 'present' only where it occurs)
    reduction = 'mean' if per_image else 'none'
    loss_r, want = lovasz_reference(logit, label, 255, 'present', per_image, cw, reduction, 3.0, scale=1.0)
    z = logit.double().requires_grad_(True)
    u = F.interpolate(z, size=(H, W), mode='bilinear', align_corners=False)
    p = F.softmax(u.detach(), dim=1)
    D = torch.zeros_like(p)
    total = 0.0
    for imgs in ([[b] for b in range(B)] if per_image else [list(range(B))]):
        pb, lb = p[imgs].permute(0, 2, 3, 1).reshape(-1, C), label[imgs].reshape(-1)
        vidx = torch.nonzero(lb != 255).reshape(-1)
        present = [c for c in range(C) if bool((lb[vidx] == c).any())]
        Db = torch.zeros_like(pb)
        for c in present:
            fg = (lb[vidx] == c)
            e = (fg.double() - pb[vidx, c]).abs()
            e_s, order = torch.sort(e, descending=True, stable=True)
            fg_s = fg[order]
            G = int(fg.sum())
            Fk = fg_s.long().cumsum(0)
            k1 = torch.arange(1, fg_s.numel() + 1)
            I, U = G - Fk, G + (k1 - Fk)
            gk = torch.where(fg_s, 1.0 / U.double(), I.double() / (U.double() * (U.double() - 1)).clamp(min=1))
            assert float((gk - lovasz_grad(fg_s.double())).abs().max()) <= 1e-15
            k = 3.0 * float(cw[c]) / len(present) / (B if per_image else 1)
            total = total + k * float(torch.dot(e_s, gk))
            Db[vidx[order], c] = torch.where(fg_s, -gk, gk) * k
        D[imgs] = Db.reshape(len(imgs), H, W, C).permute(0, 3, 1, 2)
    assert abs(total - loss_r) <= 1e-13 * loss_r
    u.backward(p * (D - (p * D).sum(1, keepdim=True)))
    assert float((z.grad - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_ce_and_lovasz_list_builds_a_head():
    plain, _ = _head()
    head, _ = _head(loss_decode=[_CE, _LOVASZ])
    from rscotr_amd.seg_head import CrossEntropyLoss, LovaszLoss
    ce, lov = list(head.loss_decode)
    assert isinstance(ce, CrossEntropyLoss) and isinstance(lov, LovaszLoss)
    assert (lov.loss_name, lov.loss_weight, lov.classes, lov.per_image, lov.reduction, lov.class_weight) == \
        ('loss_lovasz', 3.0, 'present', False, 'none', None)
    assert list(head.state_dict()) == list(plain.state_dict())  # no parameters, no buffers: the reference's keys
    head, _ = _head(loss_decode=[_CE, _LOVASZ_IMG])
    lov = head.loss_decode[1]
    assert (lov.classes, lov.per_image, lov.reduction, lov.loss_weight) == ([0, 1, 2, 3, 4, 5], True, 'mean', 0.5)
    assert list(head.state_dict()) == list(plain.state_dict())
    only, _ = _head(loss_decode=[dict(type='LovaszLoss', per_image=True, reduction='sum', classes='all', class_weight=_CW100)])
    assert isinstance(only.loss_decode[0], LovaszLoss) and only.loss_decode[0].class_weight == _CW100
    with pytest.raises(NotImplementedError, match='LovaszLoss.*list'):
        _head(loss_decode=dict(type='LovaszLoss', reduction='none'))


def test_lovasz_refusals():
    from rscotr_amd import MODELS, ops
    with pytest.raises(NotImplementedError, match='binary'):
        MODELS.build(dict(type='LovaszLoss', loss_type='binary', reduction='none'))
    with pytest.raises(NotImplementedError, match='vector'):
        MODELS.build(dict(type='LovaszLoss', per_image=True, reduction='none'))
    # mmseg's constructor asserts on its own default arguments: refused by name, with the two ways out
    with pytest.raises(NotImplementedError, match=r"LovaszLoss.*reduction='none' or per_image=True"):
        MODELS.build(dict(type='LovaszLoss'))
    with pytest.raises(NotImplementedError, match='LovaszLoss'):
        _head(loss_decode=[_CE, dict(type='LovaszLoss', reduction='sum')])
    with pytest.raises(ValueError):
        MODELS.build(dict(type='LovaszLoss', reduction='batchmean'))
    with pytest.raises(ValueError):
        MODELS.build(dict(type='LovaszLoss', reduction='none', classes='some'))
    with pytest.raises(ValueError):
        MODELS.build(dict(type='LovaszLoss', reduction='none', classes=[1, 1]))
    with pytest.raises(TypeError):
        MODELS.build(dict(type='LovaszLoss', reduction='none', classes=[]))
    with pytest.raises((TypeError, ValueError)):
        MODELS.build(dict(type='LovaszLoss', reduction='none', class_weight=3.0))
    with pytest.raises(NotImplementedError, match='LovaszLoss, TverskyLoss|TverskyLoss and LovaszLoss'):
        _head(loss_decode=[_CE, dict(type='JaccardLoss')])
    # the op's own checks come before any device is touched
    logit, label, _ = lovasz_inputs(1, 3, 4, 4, 8, 8)
    with pytest.raises(ValueError, match='more than one channel'):
        ops.upsample_lovasz(logit[:, :1], label)
    with pytest.raises(NotImplementedError, match='per_image=True'):
        ops.upsample_lovasz(logit, label, reduction='mean')
    with pytest.raises(NotImplementedError, match='vector'):
        ops.upsample_lovasz(logit, label, per_image=True, reduction='none')
    with pytest.raises(ValueError, match='distinct'):
        ops.upsample_lovasz(logit, label, classes=[0, 3])
    # a class_weight of the wrong length raises at first use
    head, _ = _head(loss_decode=[_CE, dict(type='LovaszLoss', reduction='none', class_weight=[1.0] * 6)])
    logit, label = _batch()
    with pytest.raises(ValueError, match=r'6\b.*\b100\b'):
        head.loss_decode[1](logit, label.squeeze(1))


class _FakeLovaszOps(_FakeOps):
    def upsample_lovasz(self, seg_logit, label, ignore_index=255, classes='present', per_image=False, class_weight=None,
                        reduction='none', loss_weight=1.0):
        self.calls.append(('upsample_lovasz', dict(ignore_index=ignore_index, classes=classes, per_image=per_image,
                                                   class_weight=class_weight, reduction=reduction, loss_weight=loss_weight)))
        return lovasz_contract(seg_logit, label, ignore_index, classes, per_image, class_weight, reduction, loss_weight)[0].float()


def _lovasz_head(monkeypatch, **over):
    from rscotr_amd import seg_head
    head, _ = _head(**over)
    fake = _FakeLovaszOps()
    for name in ('upsample_ce', 'upsample_ce_weighted', 'upsample_lovasz'):
        monkeypatch.setattr(seg_head.ops, name, getattr(fake, name))
    return head, fake


def test_losses_dispatch_the_lovasz_entry(monkeypatch):
    logit, label = _batch()
    lab = label.squeeze(1)
    plain, _ = _lovasz_head(monkeypatch)
    out0 = plain.losses(logit, label)
    # the head's ignore_index reaches the entry (as for FocalLoss); the sampler's weight does not (as for DiceLoss)
    head, fake = _lovasz_head(monkeypatch, loss_decode=[_CE, _LOVASZ], ignore_index=7,
                              sampler=dict(type='OHEMPixelSampler', thresh=0.01, min_kept=100))
    label7 = torch.where(label == 255, torch.full_like(label, 7), label)
    out = head.losses(logit, label7)
    assert [c[0] for c in fake.calls] == ['upsample_ce_weighted', 'upsample_lovasz']
    kw = fake.calls[1][1]
    assert (kw['ignore_index'], kw['classes'], kw['per_image'], kw['reduction'], kw['loss_weight'], kw['class_weight']) == \
        (7, 'present', False, 'none', 3.0, None)
    assert list(out) == ['loss_ce', 'loss_lovasz', 'acc_seg']
    ref = float(lovasz_contract(logit, label7.squeeze(1), 7, loss_weight=3.0)[0].detach())
    assert ref > 0 and abs(float(out['loss_lovasz'].detach()) - ref) <= 1e-6 * ref
    # per image over a class list, next to the default CE entry: the plain CE op, and the CE-only head's numbers
    head, fake = _lovasz_head(monkeypatch, loss_decode=[_CE, dict(_LOVASZ_IMG, class_weight=_CW100)])
    out = head.losses(logit, label)
    assert [c[0] for c in fake.calls] == ['upsample_ce', 'upsample_lovasz']
    kw = fake.calls[1][1]
    assert (kw['ignore_index'], kw['classes'], kw['per_image'], kw['reduction']) == (255, [0, 1, 2, 3, 4, 5], True, 'mean')
    assert torch.equal(kw['class_weight'], torch.tensor(_CW100))
    assert torch.equal(out['loss_ce'], out0['loss_ce']) and torch.equal(out['acc_seg'], out0['acc_seg'])
    ref = float(lovasz_contract(logit, lab, 255, [0, 1, 2, 3, 4, 5], True, torch.tensor(_CW100), 'mean', 0.5)[0].detach())
    assert ref > 0 and abs(float(out['loss_lovasz'].detach()) - ref) <= 1e-6 * ref
    # alone in the list: the accuracy still comes from one CE forward
    head, fake = _lovasz_head(monkeypatch, loss_decode=[_LOVASZ])
    out = head.losses(logit, label)
    assert [c[0] for c in fake.calls] == ['upsample_lovasz', 'upsample_ce'] and list(out) == ['loss_lovasz', 'acc_seg']
    assert torch.equal(out['acc_seg'], out0['acc_seg'])


def test_op_refuses_cpu_tensors():
    """No fallback to torch: the op is the HIP kernels or an error."""
    from rscotr_amd import ops
    logit, label, _ = lovasz_inputs(1, 3, 4, 4, 8, 8)
    with pytest.raises(RuntimeError):
        ops.upsample_lovasz(logit, label)
